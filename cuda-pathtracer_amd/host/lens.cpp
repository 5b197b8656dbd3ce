// lens.cpp — the check of a thin lens's two numbers and the lens block, as include/ptmi.h ("thin lens") states them.  Built with
// -ffp-contract=off like everything else: every product and every sum below is rounded once.
#include "lens.h"

#include <cmath>
#include <string>

namespace ptmi {

namespace {
// length() of pt_vec.h: the products summed left to right, then the correctly rounded root
float length3(const float* v) {
    float s = v[0] * v[0];
    s += v[1] * v[1];
    s += v[2] * v[2];
    return std::sqrt(s);
}
// the reciprocal of an image size as the frame block holds it (shade_lean.h: ptmi_size_reciprocal): 0 above 2^23
float sizeReciprocal(int n) { return (n >= 1 && n <= (1 << 23)) ? 1.0f / (float)n : 0.0f; }
}  // namespace

void checkLens(float radius, float focus_distance) {
    if (std::isnan(radius)) throw LensError("lens: radius is a NaN");
    if (std::isnan(focus_distance)) throw LensError("lens: focus_distance is a NaN");
    if (std::isinf(radius)) throw LensError("lens: radius must be finite");
    if (std::isinf(focus_distance)) throw LensError("lens: focus_distance must be finite");
    if (radius < 0.0f) throw LensError("lens: radius must not be negative");
    if (!(focus_distance > 0.0f)) throw LensError("lens: focus_distance must be positive");
}

void lensBlock(const float frame12[12], int width, int height, float radius, float focus_distance, float out24[kLensBlockFloats]) {
    if (!frame12 || !out24) throw LensError("lens: NULL argument");
    if (width <= 0 || height <= 0) throw LensError("lens: width and height must be positive");
    checkLens(radius, focus_distance);
    if (!(radius > 0.0f)) throw LensError("lens: radius 0 is the pinhole, which has no lens block");
    const float *org = frame12, *llc = frame12 + 3, *hor = frame12 + 6, *ver = frame12 + 9;
    const float f = focus_distance;
    const float ka = radius / length3(hor), kb = radius / length3(ver);
    float inv_w = sizeReciprocal(width), inv_h = sizeReciprocal(height);
    if (inv_w == 0.0f || inv_h == 0.0f) inv_w = inv_h = 0.0f;             // one flag for both, as TileMap's
    for (int k = 0; k < 3; k++) {
        const float to_llc = llc[k] - org[k];
        out24[k] = org[k] + f * to_llc;                                   // llc_f
        out24[4 + k] = f * hor[k];                                        // hor_f
        out24[8 + k] = f * ver[k];                                        // ver_f
        out24[12 + k] = org[k];
        out24[16 + k] = ka * hor[k];                                      // a
        out24[20 + k] = kb * ver[k];                                      // b
    }
    out24[3] = (float)width; out24[7] = inv_w; out24[11] = (float)height; out24[15] = inv_h;
    out24[19] = 0.0f; out24[23] = 0.0f;
    for (int i = 0; i < kLensBlockFloats; i++)
        if (!std::isfinite(out24[i]))
            throw LensError("lens: the lens block is not finite (record " + std::to_string(i / 4) + ", component " + std::to_string(i % 4) +
                            "): focus_distance or radius is too large for this camera, or the camera frame has no extent");
}

}  // namespace ptmi
