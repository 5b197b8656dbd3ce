// denoise_variance.hip — gfx950 kernels of the variance-guided a-trous filter (the spatial stage of SVGF, Schied et al. 2017)
// over the feature buffers of ptmi_render_features.  The filter is defined, operation by operation, in include/ptmi.h
// (ptmi_denoise_variance); every value here is float32 in the order written there (built with -ffp-contract=off and correctly
// rounded division), so a numpy float32 restatement reproduces it bit for bit.
//
// Kernels
//   ptmi_variance_demod    radiance / albedo per channel (where the albedo is not 0) -> (c.xyz, 0)
//   ptmi_variance_moments  the accumulation's variance of the pixels with two passes or more (one thread per slot) -> (c.xyz, v)
//   ptmi_variance_spatial  every other pixel: the weighted variance of the luminance over a (2r + 1)^2 window -> (c.xyz, v)
//   ptmi_variance_atrous   one iteration: 3 x 3 variance prefilter, 5 x 5 B3-spline taps of stride 2^i, the variance carried in .w
//   ptmi_variance_remod    x albedo again, the frame's tone map (resolve_pixel at k = 1) -> rgb8 + float radiance + variance_out
//   ptmi_pass_moments      mean, M2 and pass count of the stopping test, by slot -> local row-major (ptmi_read_pass_moments)
// One thread per pixel in every kernel; nothing but the staged tile of ptmi_variance_spatial is shared between threads, and that
// tile holds inputs only: a result does not depend on the launch geometry.
#include "denoise_common.h"
#include "shading.h"

namespace ptmi {

__global__ __launch_bounds__(kBlock) void ptmi_variance_demod(int n, const float* __restrict__ radiance, const float4* __restrict__ albedo,
                                                              int demodulate, float4* __restrict__ out) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    float c[3] = {radiance[3 * (size_t)p], radiance[3 * (size_t)p + 1], radiance[3 * (size_t)p + 2]};
    if (demodulate) {
        const float4 a = albedo[p];
        const float al[3] = {a.x, a.y, a.z};
#pragma unroll
        for (int ch = 0; ch < 3; ch++) if (al[ch] != 0.0f) c[ch] = c[ch] / al[ch];
    }
    out[p] = make_float4(c[0], c[1], c[2], 0.0f);
}

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

// step 3.  The (16 + 2 R)^2 tile of luminance, normal and position is staged in LDS once and read by both sweeps.  Entries
// outside the image are staged as zeros: a zero normal gives wn = 0, so such a tap adds +0 to every sum, which is what skipping
// it does.  Rows are kSpatialPitch float4 apart: ds_read_b128 serves 16-lane groups that span two rows of the workgroup's tile
// (MI355X: {0-3, 12-15, 20-27}, ...), and a pitch of 32 slots of 16 B puts lanes 20-27 on the slots lanes 4-11 would use - no two
// lanes of a group on one bank.  (A pitch of 22 leaves them two-way conflicting.)  The luminance, read alone by the second
// sweep with ds_read_b32 (32-lane groups = two rows, 32 banks), has a pitch of 48 = 16 mod 32 for the same reason.
constexpr int kSpatialMaxR = 3, kSpatialRows = kTileY + 2 * kSpatialMaxR, kSpatialPitch = 32, kSpatialLumPitch = 48;

// denoise_wn without its loop: the squarings are predicated (normal_squarings <= 10, the host's check).  With a loop per tap the
// compiler runs the (2 R + 1)^2 loops of the unrolled window as one and keeps every tap's operands live across it: 264
// registers at R = 3, one wave per SIMD.
__device__ __forceinline__ float spatial_wn(const float4& np, const float4& nq, int normal_squarings) {
    float wn = fmaxf(0.0f, np.x * nq.x + np.y * nq.y + np.z * nq.z);
#pragma unroll
    for (int k = 0; k < 10; k++) wn = k < normal_squarings ? wn * wn : wn;
    return wn;
}

template <int R>
__global__ __launch_bounds__(kTileX * kTileY, 4) void ptmi_variance_spatial(VarianceArgs a, FeatureBuffers fb, const unsigned int* __restrict__ counts,
                                                                         const float4* __restrict__ in, float4* __restrict__ out,
                                                                         float* __restrict__ var_in) {
    constexpr int T = kTileX + 2 * R, D = 2 * R + 1;
    const int tx = threadIdx.x % kTileX, ty = threadIdx.x / kTileX;
    const int x = blockIdx.x * kTileX + tx, y = blockIdx.y * kTileY + ty;
#ifndef PTMI_VARIANCE_UNSTAGED     // (never defined in the shipped build: make ab-post-lib, the estimate through the cache alone - EXPERIMENTS.md)
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
#endif
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
#ifndef PTMI_VARIANCE_UNSTAGED
            const float4 nq = s_n[(ty + j) * kSpatialPitch + tx + i], xq = s_x[(ty + j) * kSpatialPitch + tx + i];
            const float lq = s_l[(ty + j) * kSpatialLumPitch + tx + i];
#else
            const int qx = x + i - R, qy = y + j - R;
            float4 nq = make_float4(0.0f, 0.0f, 0.0f, 0.0f), xq = nq;
            float lq = 0.0f;
            if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
                const int q = qy * a.width + qx;
                const float4 cq = in[q];
                nq = fb.normal[q]; xq = fb.position[q];
                lq = denoise_lum(cq.x, cq.y, cq.z);
            }
#endif
            const float wq = spatial_wn(np, nq, a.normal_squarings) * denoise_wx(xp, xq, a.sigma_x2);
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
#ifndef PTMI_VARIANCE_UNSTAGED
                const float lq = s_l[(ty + j) * kSpatialLumPitch + tx + i];
#else
                const int qx = x + i - R, qy = y + j - R;
                float lq = 0.0f;
                if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
                    const float4 cq = in[qy * a.width + qx];
                    lq = denoise_lum(cq.x, cq.y, cq.z);
                }
#endif
                const float d = lq - m;
                B = B + w[j * D + i] * (d * d);
            }
        }
        v = B / W;
    }
    var_in[p] = v;
    out[p] = make_float4(cp.x, cp.y, cp.z, v);
}

// step 4, one iteration
__global__ __launch_bounds__(kTileX * kTileY) void ptmi_variance_atrous(VarianceArgs a, FeatureBuffers fb, int stride,
                                                                        const float4* __restrict__ in, float4* __restrict__ out) {
    const int x = blockIdx.x * kTileX + (threadIdx.x % kTileX);
    const int y = blockIdx.y * kTileY + (threadIdx.x / kTileX);
    if (x >= a.width || y >= a.height) return;
    const int p = y * a.width + x;
    const float4 cp = in[p];
    const float4 np = fb.normal[p], xp = fb.position[p];
    // the variance through a 3 x 3 Gaussian at stride 1, renormalised at the border
    float gn = 0.0f, gd = 0.0f;
#pragma unroll
    for (int j = -1; j <= 1; j++) {
        const int qy = y + j;
        if (qy < 0 || qy >= a.height) continue;
#pragma unroll
        for (int i = -1; i <= 1; i++) {
            const int qx = x + i;
            if (qx < 0 || qx >= a.width) continue;
            const float g = (j == 0 ? 0.5f : 0.25f) * (i == 0 ? 0.5f : 0.25f);
            gn = gn + g * in[qy * a.width + qx].w;
            gd = gd + g;
        }
    }
    const float tol = a.sigma_l2 * (gn / gd) + a.epsilon;
    const float lp = denoise_lum(cp.x, cp.y, cp.z);
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int qy = y + (j - 2) * stride;
        if (qy < 0 || qy >= a.height) continue;                       // taps outside the image are skipped
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const int qx = x + (i - 2) * stride;
            if (qx < 0 || qx >= a.width) continue;
            const int q = qy * a.width + qx;
            const float4 cq = in[q], nq = fb.normal[q], xq = fb.position[q];
            const float dl = lp - denoise_lum(cq.x, cq.y, cq.z);
            const float wl = 1.0f / (1.0f + (dl * dl) / tol);
            const float wn = denoise_wn(np, nq, a.normal_squarings);
            const float wx = denoise_wx(xp, xq, a.sigma_x2);
            const float w = b3(j) * b3(i) * wl * wn * wx;
            sw = sw + w;
            sx = sx + w * cq.x; sy = sy + w * cq.y; sz = sz + w * cq.z;
            sv = sv + (w * w) * cq.w;
        }
    }
    float4 o = cp;
    if (sw > 0.0f) {
        o.x = sx / sw; o.y = sy / sw; o.z = sz / sw;
        o.w = (sv / sw) / sw;                                         // (sw * sw underflows to 0 where the taps all but vanish)
    }
    out[p] = o;
}

// passthrough (0 iterations): the input radiance as it is, no demodulation round trip; the variance is in[].w either way
__global__ __launch_bounds__(kBlock) void ptmi_variance_remod(int n, const float4* __restrict__ in, const float* __restrict__ radiance,
                                                              const float4* __restrict__ albedo, int demodulate, int passthrough,
                                                              unsigned char* __restrict__ rgb8, float* __restrict__ out_radiance,
                                                              float* __restrict__ var_out) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    float4 c = in[p];
    var_out[p] = c.w;
    if (passthrough) {
        c = make_float4(radiance[3 * (size_t)p], radiance[3 * (size_t)p + 1], radiance[3 * (size_t)p + 2], 0.0f);
    } else if (demodulate) {
        const float4 a = albedo[p];
        if (a.x != 0.0f) c.x = c.x * a.x;
        if (a.y != 0.0f) c.y = c.y * a.y;
        if (a.z != 0.0f) c.z = c.z * a.z;
    }
    resolve_pixel(c, 1.0f, (size_t)p, rgb8, out_radiance);
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

void launch_denoise_variance(const VarianceArgs& a, const FeatureBuffers& fb, const float* radiance, const TileMap& tm,
                             const AccumBuffers* moments, const unsigned int* counts, int iterations, float4* buf, float* var_in,
                             float* var_out, unsigned char* out_rgb8, float* out_radiance, hipEvent_t estimated, hipStream_t s) {
    const int n = a.width * a.height;
    if (n <= 0) { (void)hipEventRecord(estimated, s); return; }
    const dim3 grid1((n + kBlock - 1) / kBlock), block1(kBlock);
    const dim3 grid2((a.width + kTileX - 1) / kTileX, (a.height + kTileY - 1) / kTileY), block2(kTileX * kTileY);
    float4* ping[2] = {buf, buf + n};
    hipLaunchKernelGGL(ptmi_variance_demod, grid1, block1, 0, s, n, radiance, fb.albedo, a.demodulate, ping[0]);
    if (moments) hipLaunchKernelGGL(ptmi_variance_moments, grid1, block1, 0, s, tm, *moments, radiance, ping[0], ping[1], var_in);
    const unsigned int* skip = moments ? counts : nullptr;
    if (a.radius == 1) hipLaunchKernelGGL(ptmi_variance_spatial<1>, grid2, block2, 0, s, a, fb, skip, ping[0], ping[1], var_in);
    else if (a.radius == 2) hipLaunchKernelGGL(ptmi_variance_spatial<2>, grid2, block2, 0, s, a, fb, skip, ping[0], ping[1], var_in);
    else hipLaunchKernelGGL(ptmi_variance_spatial<3>, grid2, block2, 0, s, a, fb, skip, ping[0], ping[1], var_in);
    (void)hipEventRecord(estimated, s);
    for (int i = 0; i < iterations; i++)                              // (c, v) starts in ping[1]
        hipLaunchKernelGGL(ptmi_variance_atrous, grid2, block2, 0, s, a, fb, 1 << i, ping[(i + 1) & 1], ping[i & 1]);
    hipLaunchKernelGGL(ptmi_variance_remod, grid1, block1, 0, s, n, ping[(iterations + 1) & 1], radiance, fb.albedo, a.demodulate,
                       iterations <= 0 ? 1 : 0, out_rgb8, out_radiance, var_out);
}

void launch_pass_moments(const TileMap& tm, const AccumBuffers& ab, float* mean, float* m2, unsigned int* passes, hipStream_t s) {
    const int n = tm.local_rows * tm.width;
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_pass_moments, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, tm, ab, mean, m2, passes);
}

}  // namespace ptmi
