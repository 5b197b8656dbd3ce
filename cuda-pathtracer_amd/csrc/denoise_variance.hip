// denoise_variance.hip — gfx950 kernels of the variance estimate that steers the variance-guided a-trous filter (the filter
// itself: denoise.hip), and of ptmi_read_pass_moments.  The estimate is defined, operation by operation, in include/ptmi.h
// (ptmi_denoise_variance steps 2 and 3); every value here is float32 in the order written there (built with -ffp-contract=off
// and correctly rounded division), so a numpy float32 restatement reproduces it bit for bit.
//
// Kernels
//   ptmi_variance_moments  the accumulation's variance of the pixels with two passes or more (one thread per slot) -> (c.xyz, v)
//   ptmi_variance_temporal the history's variance of the pixels with PTMI_TEMPORAL_MIN_FRAMES frames or more -> (c.xyz, v), and the mask
//   ptmi_variance_spatial  every other pixel: the weighted variance of the luminance over a (2r + 1)^2 window -> (c.xyz, v)
//   ptmi_pass_moments      mean, M2 and pass count of the stopping test, by slot -> local row-major (ptmi_read_pass_moments)
// One thread per pixel in every kernel; nothing but the staged tile of ptmi_variance_spatial is shared between threads, and that
// tile holds inputs only: a result does not depend on the launch geometry.
#include "denoise_common.h"
#include "shading.h"

namespace ptmi {

// step 2: the variance of the mean of the pass means, in the filtered signal's units.  The moments lie by slot, the images
// local row-major.
__global__ __launch_bounds__(kBlock) void ptmi_variance_moments(TileMap tm, AccumBuffers ab, const float* __restrict__ radiance,
                                                                const float4* __restrict__ in, float4* __restrict__ out,
                                                                float* __restrict__ var_in) {
    const int n = tm.local_rows * tm.width;
    const int slot = blockIdx.x * kBlock + threadIdx.x;
    if (slot >= n) return;
    const unsigned int k = ab.passes[slot];
    if (k < 2u) return;                                               // the spatial estimate's pixel
    int x, lr;
    slot_to_local(tm, slot, x, lr);
    const size_t p = (size_t)lr * (size_t)tm.width + (size_t)x;
    const float4 c = in[p];
    float v = fmaxf(0.0f, ab.m2[slot] / (float)(k * (k - 1u)));
    const float lr_ = denoise_lum(radiance[3 * p], radiance[3 * p + 1], radiance[3 * p + 2]);
    if (lr_ > 0.0f) {
        const float s = denoise_lum(c.x, c.y, c.z) / lr_;
        v = (v * s) * s;
    }
    var_in[p] = v;
    out[p] = make_float4(c.x, c.y, c.z, v);
}

// ptmi_denoise_temporal_variance's step 2: the variance of the mean of the k frames behind a pixel of the history, from the
// history's luminance statistics (mu, s2, k, 0), in the filtered signal's units.  mask: 1 where this kernel owns the pixel (k >=
// kTemporalMinFrames; a NaN k fails the test), else 0 - ptmi_variance_spatial takes it as its counts with two_spp = 1.
__global__ __launch_bounds__(kBlock) void ptmi_variance_temporal(int n, const float4* __restrict__ moments, const float* __restrict__ radiance,
                                                                 const float4* __restrict__ in, float4* __restrict__ out,
                                                                 float* __restrict__ var_in, unsigned int* __restrict__ mask) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const float4 mo = moments[p];
    const bool own = mo.z >= kTemporalMinFrames;
    mask[p] = own ? 1u : 0u;
    if (!own) return;                                                 // the spatial estimate's pixel
    const float4 c = in[p];
    float v = fmaxf(0.0f, mo.y / (mo.z - 1.0f));
    const float lr_ = denoise_lum(radiance[3 * (size_t)p], radiance[3 * (size_t)p + 1], radiance[3 * (size_t)p + 2]);
    if (lr_ > 0.0f) {
        const float s = denoise_lum(c.x, c.y, c.z) / lr_;
        v = (v * s) * s;
    }
    var_in[p] = v;
    out[p] = make_float4(c.x, c.y, c.z, v);
}

// step 3.  The (16 + 2 R)^2 tile of luminance, normal and position is staged in LDS once and read by both sweeps.  Entries
// outside the image are staged as zeros: a zero normal gives wn = 0, so such a tap adds +0 to every sum, which is what skipping
// it does.  Rows are kSpatialPitch float4 apart: ds_read_b128 serves 16-lane groups that span two rows of the workgroup's tile
// (MI355X: {0-3, 12-15, 20-27}, ...), and a pitch of 32 slots of 16 B puts lanes 20-27 on the slots lanes 4-11 would use - no two
// lanes of a group on one bank.  (A pitch of 22 leaves them two-way conflicting.)  The luminance, read alone by the second
// sweep with ds_read_b32 (32-lane groups = two rows, 32 banks), has a pitch of 48 = 16 mod 32 for the same reason.
constexpr int kSpatialMaxR = 3, kSpatialRows = kTileY + 2 * kSpatialMaxR, kSpatialPitch = 32, kSpatialLumPitch = 48;

template <int R>
__global__ __launch_bounds__(kTileX * kTileY, 4) void ptmi_variance_spatial(VarianceArgs a, FeatureBuffers fb, const unsigned int* __restrict__ counts,
                                                                         const float4* __restrict__ in, float4* __restrict__ out,
                                                                         float* __restrict__ var_in) {
    constexpr int T = kTileX + 2 * R, D = 2 * R + 1;
    const int tx = threadIdx.x % kTileX, ty = threadIdx.x / kTileX;
    const int x = blockIdx.x * kTileX + tx, y = blockIdx.y * kTileY + ty;
    __shared__ float4 s_n[kSpatialRows * kSpatialPitch], s_x[kSpatialRows * kSpatialPitch];
    __shared__ float s_l[kSpatialRows * kSpatialLumPitch];
    for (int e = threadIdx.x; e < T * T; e += kTileX * kTileY) {
        const int ey = e / T, ex = e - ey * T;
        const int qx = blockIdx.x * kTileX - R + ex, qy = blockIdx.y * kTileY - R + ey;
        float4 nq = make_float4(0.0f, 0.0f, 0.0f, 0.0f), xq = nq;
        float lq = 0.0f;
        if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
            const int q = qy * a.width + qx;
            const float4 cq = in[q];
            nq = fb.normal[q]; xq = fb.position[q];
            lq = denoise_lum(cq.x, cq.y, cq.z);
        }
        s_n[ey * kSpatialPitch + ex] = nq; s_x[ey * kSpatialPitch + ex] = xq; s_l[ey * kSpatialLumPitch + ex] = lq;
    }
    __syncthreads();
    if (x >= a.width || y >= a.height) return;
    const int p = y * a.width + x;
    if (counts && counts[p] >= a.two_spp) return;                     // ptmi_variance_moments has written this pixel
    const float4 cp = in[p];
    const float4 np = fb.normal[p], xp = fb.position[p];
    float w[D * D];
    float W = 0.0f, A = 0.0f;
#pragma unroll
    for (int j = 0; j < D; j++) {
#pragma unroll
        for (int i = 0; i < D; i++) {
            const float4 nq = s_n[(ty + j) * kSpatialPitch + tx + i], xq = s_x[(ty + j) * kSpatialPitch + tx + i];
            const float lq = s_l[(ty + j) * kSpatialLumPitch + tx + i];
            const float wq = denoise_wn_predicated(np, nq, a.normal_squarings) * denoise_wx(xp, xq, a.sigma_x2);
            w[j * D + i] = wq;
            W = W + wq;
            A = A + wq * lq;
        }
    }
    float v = 0.0f;
    if (W > 0.0f) {
        const float m = A / W;
        float B = 0.0f;
#pragma unroll
        for (int j = 0; j < D; j++) {
#pragma unroll
            for (int i = 0; i < D; i++) {
                const float lq = s_l[(ty + j) * kSpatialLumPitch + tx + i];
                const float d = lq - m;
                B = B + w[j * D + i] * (d * d);
            }
        }
        v = B / W;
    }
    var_in[p] = v;
    out[p] = make_float4(cp.x, cp.y, cp.z, v);
}

__global__ __launch_bounds__(kBlock) void ptmi_pass_moments(TileMap tm, AccumBuffers ab, float* __restrict__ mean, float* __restrict__ m2,
                                                            unsigned int* __restrict__ passes) {
    const int n = tm.local_rows * tm.width;
    const int slot = blockIdx.x * kBlock + threadIdx.x;
    if (slot >= n) return;
    int x, lr;
    slot_to_local(tm, slot, x, lr);
    const size_t p = (size_t)lr * (size_t)tm.width + (size_t)x;
    mean[p] = ab.prev[slot].w; m2[p] = ab.m2[slot]; passes[p] = ab.passes[slot];
}

void launch_variance_estimate(const VarianceArgs& a, const FeatureBuffers& fb, const float* radiance, const TileMap& tm,
                              const AccumBuffers* moments, const unsigned int* counts, const float4* in, float4* out, float* var_in,
                              hipStream_t s, const TemporalVariance* temporal) {
    const int n = a.width * a.height;
    const dim3 grid1((n + kBlock - 1) / kBlock), block1(kBlock);
    const dim3 grid2((a.width + kTileX - 1) / kTileX, (a.height + kTileY - 1) / kTileY), block2(kTileX * kTileY);
    const bool history = temporal && temporal->source == 0;           // the third route (a.two_spp is 1 there: the mask is 0 / 1)
    if (history) hipLaunchKernelGGL(ptmi_variance_temporal, grid1, block1, 0, s, n, temporal->moments, radiance, in, out, var_in, temporal->mask);
    else if (moments) hipLaunchKernelGGL(ptmi_variance_moments, grid1, block1, 0, s, tm, *moments, radiance, in, out, var_in);
    const unsigned int* skip = history ? temporal->mask : moments ? counts : nullptr;
    if (a.radius == 1) hipLaunchKernelGGL(ptmi_variance_spatial<1>, grid2, block2, 0, s, a, fb, skip, in, out, var_in);
    else if (a.radius == 2) hipLaunchKernelGGL(ptmi_variance_spatial<2>, grid2, block2, 0, s, a, fb, skip, in, out, var_in);
    else hipLaunchKernelGGL(ptmi_variance_spatial<3>, grid2, block2, 0, s, a, fb, skip, in, out, var_in);
}

void launch_pass_moments(const TileMap& tm, const AccumBuffers& ab, float* mean, float* m2, unsigned int* passes, hipStream_t s) {
    const int n = tm.local_rows * tm.width;
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_pass_moments, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, tm, ab, mean, m2, passes);
}

}  // namespace ptmi
