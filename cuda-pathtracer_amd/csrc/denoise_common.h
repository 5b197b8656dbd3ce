// denoise_common.h — what the a-trous filters (denoise.hip, denoise_variance.hip) share: luminance, the B3-spline taps, the
// workgroup tile and the normal and position edge-stops of include/ptmi.h (ptmi_denoise step 2).  Everything is __forceinline__
// into the calling kernel; float32 in the order written there.
#pragma once
#include "pt_device.h"

namespace ptmi {

__device__ __forceinline__ float denoise_lum(float x, float y, float z) { return 0.2126f * x + 0.7152f * y + 0.0722f * z; }

// B3-spline taps {1/16, 1/4, 3/8, 1/4, 1/16} (exact in float)
__device__ __forceinline__ float b3(int k) { return k == 0 || k == 4 ? 0.0625f : (k == 2 ? 0.375f : 0.25f); }

// 16 x 16 pixels per workgroup: the taps of neighbouring lanes hit the same lines
constexpr int kTileX = 16, kTileY = 16;

// The edge-stops below are written out once more inside ptmi_denoise_atrous: calling them from there reorders that kernel's
// instruction stream (same length and registers, another text), and a change of denoise_variance.hip must not be one of denoise.hip.
// wn = max(0, n_p . n_q), squared normal_squarings times
__device__ __forceinline__ float denoise_wn(const float4 np, const float4 nq, int normal_squarings) {
    float wn = fmaxf(0.0f, np.x * nq.x + np.y * nq.y + np.z * nq.z);
    for (int k = 0; k < normal_squarings; k++) wn = wn * wn;
    return wn;
}

// wx = 1 / (1 + |x_p - x_q|^2 / sigma_x^2)
__device__ __forceinline__ float denoise_wx(const float4 xp, const float4 xq, float sigma_x2) {
    const float ex = xp.x - xq.x, ey = xp.y - xq.y, ez = xp.z - xq.z;
    const float d2x = ex * ex + ey * ey + ez * ez;
    return 1.0f / (1.0f + d2x / sigma_x2);
}

}  // namespace ptmi
