// denoise.hip — gfx950 kernels of the edge-avoiding a-trous denoiser (Dammertz et al., 2010) over the feature buffers of
// ptmi_render_features.  The filter is defined, operation by operation, in include/ptmi.h (ptmi_denoise); every value here is
// float32 in the order written there (built with -ffp-contract=off and correctly rounded division), so a numpy float32
// restatement reproduces it bit for bit.
//
// Kernels
//   ptmi_denoise_demod   radiance / albedo per channel (where the albedo is not 0) -> (c.xyz, lum(c))
//   ptmi_denoise_atrous  one iteration: 5 x 5 B3-spline taps of stride 2^i, weighted by colour, normal and position
//   ptmi_denoise_remod   x albedo again, then the frame's tone map (resolve_pixel at k = 1) -> rgb8 + float radiance
// One thread per pixel in every kernel and nothing shared between threads: a result does not depend on the launch geometry.
#include "denoise_common.h"

namespace ptmi {

__global__ __launch_bounds__(kBlock) void ptmi_denoise_demod(int n, const float* __restrict__ radiance, const float4* __restrict__ albedo,
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
    out[p] = make_float4(c[0], c[1], c[2], denoise_lum(c[0], c[1], c[2]));
}

__global__ __launch_bounds__(kTileX * kTileY) void ptmi_denoise_atrous(DenoiseArgs a, FeatureBuffers fb, int stride, float sigma_c,
                                                                       const float4* __restrict__ in, float4* __restrict__ out) {
    const int x = blockIdx.x * kTileX + (threadIdx.x % kTileX);
    const int y = blockIdx.y * kTileY + (threadIdx.x / kTileX);
    if (x >= a.width || y >= a.height) return;
    const int p = y * a.width + x;
    const float4 cp = in[p];
    const float4 np = fb.normal[p], xp = fb.position[p];
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
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
            const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
            const float d2c = dr * dr + dg * dg + db * db;
            const float sc = sigma_c * (fminf(cp.w, cq.w) + a.color_floor);      // the darker of the two sets the tolerance
            const float wc = 1.0f / (1.0f + d2c / (sc * sc));
            float wn = fmaxf(0.0f, np.x * nq.x + np.y * nq.y + np.z * nq.z);
            for (int k = 0; k < a.normal_squarings; k++) wn = wn * wn;
            const float ex = xp.x - xq.x, ey = xp.y - xq.y, ez = xp.z - xq.z;
            const float d2x = ex * ex + ey * ey + ez * ez;
            const float wx = 1.0f / (1.0f + d2x / a.sigma_x2);
            const float w = b3(j) * b3(i) * wc * wn * wx;
            sw = sw + w;
            sx = sx + w * cq.x; sy = sy + w * cq.y; sz = sz + w * cq.z;
        }
    }
    float4 o = cp;
    if (sw > 0.0f) {
        o.x = sx / sw; o.y = sy / sw; o.z = sz / sw;
        o.w = denoise_lum(o.x, o.y, o.z);
    }
    out[p] = o;
}

// in == nullptr (0 iterations): the input radiance as it is, no demodulation round trip
__global__ __launch_bounds__(kBlock) void ptmi_denoise_remod(int n, const float4* __restrict__ in, const float* __restrict__ radiance,
                                                             const float4* __restrict__ albedo, int demodulate,
                                                             unsigned char* __restrict__ rgb8, float* __restrict__ out_radiance) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    float4 c;
    if (in) {
        c = in[p];
        if (demodulate) {
            const float4 a = albedo[p];
            if (a.x != 0.0f) c.x = c.x * a.x;
            if (a.y != 0.0f) c.y = c.y * a.y;
            if (a.z != 0.0f) c.z = c.z * a.z;
        }
    } else {
        c = make_float4(radiance[3 * (size_t)p], radiance[3 * (size_t)p + 1], radiance[3 * (size_t)p + 2], 0.0f);
    }
    resolve_pixel(c, 1.0f, (size_t)p, rgb8, out_radiance);
}

void launch_denoise(const DenoiseArgs& a, const FeatureBuffers& fb, const float* radiance, int iterations, const float* sigma_c,
                    float4* buf, unsigned char* out_rgb8, float* out_radiance, hipStream_t s) {
    const int n = a.width * a.height;
    if (n <= 0) return;
    const dim3 grid1((n + kBlock - 1) / kBlock), block1(kBlock);
    if (iterations <= 0) {
        hipLaunchKernelGGL(ptmi_denoise_remod, grid1, block1, 0, s, n, (const float4*)nullptr, radiance, fb.albedo, 0, out_rgb8, out_radiance);
        return;
    }
    float4* ping[2] = {buf, buf + n};
    hipLaunchKernelGGL(ptmi_denoise_demod, grid1, block1, 0, s, n, radiance, fb.albedo, a.demodulate, ping[0]);
    const dim3 grid2((a.width + kTileX - 1) / kTileX, (a.height + kTileY - 1) / kTileY), block2(kTileX * kTileY);
    for (int i = 0; i < iterations; i++)
        hipLaunchKernelGGL(ptmi_denoise_atrous, grid2, block2, 0, s, a, fb, 1 << i, sigma_c[i], ping[i & 1], ping[(i + 1) & 1]);
    hipLaunchKernelGGL(ptmi_denoise_remod, grid1, block1, 0, s, n, ping[iterations & 1], radiance, fb.albedo, a.demodulate, out_rgb8, out_radiance);
}

}  // namespace ptmi
