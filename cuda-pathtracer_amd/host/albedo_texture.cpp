// albedo_texture.cpp — the check of an albedo texture's image, UV table and mask, as include/ptmi.h ("albedo texture") states it.
#include "albedo_texture.h"

#include <cmath>
#include <string>

#include "application_state.h"   // ArgError

namespace ptmi {

static void checkCorner(const float* uv, int i, int c) {
    const float* v = uv + ((size_t)i * kAlbedoCorners + (size_t)c) * 2;
    for (int a = 0; a < 2; a++) {
        if (!std::isfinite(v[a]))
            throw ArgError("albedo texture: uv of corner " + std::to_string(c) + " of primitive " + std::to_string(i) + " must be finite");
        if (std::fabs(v[a]) > kAlbedoMaxUV)
            throw ArgError("albedo texture: uv of corner " + std::to_string(c) + " of primitive " + std::to_string(i) + " exceeds 65536 in magnitude");
    }
}

int countTextured(int n_prims, const int* textured) {
    if (!textured) return n_prims > 0 ? n_prims : 0;
    int n = 0;
    for (int i = 0; i < n_prims; i++) n += textured[i] != 0;
    return n;
}

void checkAlbedoTexture(int width, int height, const float* texels, int filter, int n_prims, const float* uv, const int* textured) {
    if (n_prims < 1) throw ArgError("albedo texture: n_prims must be >= 1");
    if (!texels) throw ArgError("albedo texture: texels is NULL");
    if (!uv) throw ArgError("albedo texture: uv is NULL");
    if (width < 1 || width > kAlbedoMaxSide) throw ArgError("albedo texture: width must be 1 .. 4096");
    if (height < 1 || height > kAlbedoMaxSide) throw ArgError("albedo texture: height must be 1 .. 4096");
    if (filter != 0 && filter != 1) throw ArgError("albedo texture: filter must be 0 (nearest) or 1 (bilinear)");
    const size_t n_tex = (size_t)width * (size_t)height * 3;
    for (size_t t = 0; t < n_tex; t++) {
        if (!std::isfinite(texels[t])) throw ArgError("albedo texture: texel component " + std::to_string(t) + " must be finite");
        if (texels[t] < 0.0f) throw ArgError("albedo texture: texel component " + std::to_string(t) + " must not be negative");
    }
    for (int i = 0; i < n_prims; i++) {
        if (textured && textured[i] == 0) continue;             // never read
        for (int c = 0; c < 3; c++) checkCorner(uv, i, c);
    }
}

void checkAlbedoTexture(const std::vector<Primitive>& prims, int width, int height, const float* texels, int filter, int n_prims,
                        const float* uv, const int* textured) {
    if (n_prims != (int)prims.size()) throw ArgError("albedo texture: n_prims does not match the loaded scene");
    checkAlbedoTexture(width, height, texels, filter, n_prims, uv, textured);
    for (int i = 0; i < n_prims; i++)
        if (prims[i].type == PRIM_QUAD && !(textured && textured[i] == 0)) checkCorner(uv, i, 3);
}

}  // namespace ptmi
