// denoise_common.h — the __device__ code the a-trous family (denoise.hip) and the variance estimate (denoise_variance.hip)
// share: luminance, the workgroup tile and the normal and position edge-stops of include/ptmi.h (ptmi_denoise step 2), and the
// one host function by which denoise.hip reaches the estimate's kernels.  Everything __device__ is __forceinline__ into the
// calling kernel; float32 in the order written there.
#pragma once
#include "pt_device.h"

namespace ptmi {

__device__ __forceinline__ float denoise_lum(float x, float y, float z) { return 0.2126f * x + 0.7152f * y + 0.0722f * z; }

// 16 x 16 pixels per workgroup: the taps of neighbouring lanes hit the same lines
constexpr int kTileX = 16, kTileY = 16;

// wn = max(0, n_p . n_q), squared normal_squarings times
__device__ __forceinline__ float denoise_wn(const float4 np, const float4 nq, int normal_squarings) {
    float wn = fmaxf(0.0f, np.x * nq.x + np.y * nq.y + np.z * nq.z);
    for (int k = 0; k < normal_squarings; k++) wn = wn * wn;
    return wn;
}
// Two forms: the loop costs ptmi_variance_spatial<3> 264 registers, this one costs the a-trous kernels 4 - 19 % (EXPERIMENTS.md).
// The same products in the same order, predicated (normal_squarings <= 10, the host's check).
__device__ __forceinline__ float denoise_wn_predicated(const float4& np, const float4& nq, int normal_squarings) {
    float wn = fmaxf(0.0f, np.x * nq.x + np.y * nq.y + np.z * nq.z);
#pragma unroll
    for (int k = 0; k < 10; k++) wn = k < normal_squarings ? wn * wn : wn;
    return wn;
}

// wx = 1 / (1 + |x_p - x_q|^2 / sigma_x^2)
__device__ __forceinline__ float denoise_wx(const float4 xp, const float4 xq, float sigma_x2) {
    const float ex = xp.x - xq.x, ey = xp.y - xq.y, ez = xp.z - xq.z;
    const float d2x = ex * ex + ey * ey + ez * ez;
    return 1.0f / (1.0f + d2x / sigma_x2);
}

// denoise_variance.hip: the variance estimate of launch_denoise_variance (device_scene.h) over the demodulated image `in`
// -> (c.xyz, v) in `out` and v in var_in
void launch_variance_estimate(const VarianceArgs& a, const FeatureBuffers& fb, const float* radiance, const TileMap& tm,
                              const AccumBuffers* moments, const unsigned int* counts, const float4* in, float4* out, float* var_in,
                              hipStream_t s, const TemporalVariance* temporal = nullptr);

}  // namespace ptmi
