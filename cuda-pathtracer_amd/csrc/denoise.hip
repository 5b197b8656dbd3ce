// denoise.hip — gfx950 kernels of the a-trous family over the feature buffers of ptmi_render_features: the edge-avoiding filter
// (Dammertz et al., 2010; ptmi_denoise) and the variance-guided one (the spatial stage of SVGF, Schied et al. 2017;
// ptmi_denoise_variance), whose variance estimate is denoise_variance.hip.  Both are defined, operation by operation, in
// include/ptmi.h; every value here is float32 in the order written there (built with -ffp-contract=off and correctly rounded
// division), so a numpy float32 restatement reproduces it bit for bit.
//
// Kernels
//   ptmi_denoise_demod    radiance / albedo per channel (where the albedo is not 0) -> (c.xyz, lum(c))
//   ptmi_denoise_atrous   one iteration: 5 x 5 B3-spline taps of stride 2^i, weighted by colour, normal and position
//   ptmi_variance_atrous  one iteration: 3 x 3 variance prefilter, the same taps weighted by luminance against the variance,
//                         normal and position; the variance carried in .w
//   ptmi_denoise_remod    x albedo again, then the frame's tone map (resolve_pixel at k = 1) -> rgb8 + float radiance (+ variance_out)
// The two a-trous kernels are one tap loop (atrous_pixel) with the filter's range weight put in.  One thread per pixel in every
// kernel and nothing shared between threads: a result does not depend on the launch geometry.
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
    out[p] = make_float4(c[0], c[1], c[2], denoise_lum(c[0], c[1], c[2]));   // (the variance path overwrites .w before it reads it)
}

// B3-spline taps {1/16, 1/4, 3/8, 1/4, 1/16} (exact in float)
__device__ __forceinline__ float b3(int k) { return k == 0 || k == 4 ? 0.0625f : (k == 2 ? 0.375f : 0.25f); }

// The range weight of tap q against pixel p, and what .w carries.  ptmi_denoise: .w = lum(c); the darker of the two sets the
// colour tolerance.
struct ColourRange {
    static constexpr bool kCarriesVariance = false;
    float sigma_c, color_floor;
    __device__ __forceinline__ float operator()(const float4& cp, const float4& cq) const {
        const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
        const float d2c = dr * dr + dg * dg + db * db;
        const float sc = sigma_c * (fminf(cp.w, cq.w) + color_floor);
        return 1.0f / (1.0f + d2c / (sc * sc));
    }
};
// ptmi_denoise_variance: .w = variance; tol = sigma_l^2 x the pixel's prefiltered variance + epsilon
struct LuminanceRange {
    static constexpr bool kCarriesVariance = true;
    float tol;
    __device__ __forceinline__ float operator()(const float4& cp, const float4& cq) const {
        const float dl = denoise_lum(cp.x, cp.y, cp.z) - denoise_lum(cq.x, cq.y, cq.z);
        return 1.0f / (1.0f + (dl * dl) / tol);
    }
};

// one iteration at pixel (x, y) of the image
template <class Range>
__device__ __forceinline__ void atrous_pixel(const FilterArgs& a, const FeatureBuffers& fb, int stride, const Range& range, int x, int y,
                                             const float4* __restrict__ in, float4* __restrict__ out) {
    const int p = y * a.width + x;
    const float4 cp = in[p];
    const float4 np = fb.normal[p], xp = fb.position[p];
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
            const float wr = range(cp, cq);
            const float wn = denoise_wn(np, nq, a.normal_squarings);
            const float wx = denoise_wx(xp, xq, a.sigma_x2);
            const float w = b3(j) * b3(i) * wr * wn * wx;
            sw = sw + w;
            sx = sx + w * cq.x; sy = sy + w * cq.y; sz = sz + w * cq.z;
            if (Range::kCarriesVariance) sv = sv + (w * w) * cq.w;
        }
    }
    float4 o = cp;
    if (sw > 0.0f) {
        o.x = sx / sw; o.y = sy / sw; o.z = sz / sw;
        o.w = Range::kCarriesVariance ? (sv / sw) / sw                // (sw * sw underflows to 0 where the taps all but vanish)
                                      : denoise_lum(o.x, o.y, o.z);
    }
    out[p] = o;
}

__global__ __launch_bounds__(kTileX * kTileY) void ptmi_denoise_atrous(DenoiseArgs a, FeatureBuffers fb, int stride, float sigma_c,
                                                                       const float4* __restrict__ in, float4* __restrict__ out) {
    const int x = blockIdx.x * kTileX + (threadIdx.x % kTileX);
    const int y = blockIdx.y * kTileY + (threadIdx.x / kTileX);
    if (x >= a.width || y >= a.height) return;
    atrous_pixel(a, fb, stride, ColourRange{sigma_c, a.color_floor}, x, y, in, out);
}

__global__ __launch_bounds__(kTileX * kTileY) void ptmi_variance_atrous(VarianceArgs a, FeatureBuffers fb, int stride,
                                                                        const float4* __restrict__ in, float4* __restrict__ out) {
    const int x = blockIdx.x * kTileX + (threadIdx.x % kTileX);
    const int y = blockIdx.y * kTileY + (threadIdx.x / kTileX);
    if (x >= a.width || y >= a.height) return;
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
    atrous_pixel(a, fb, stride, LuminanceRange{a.sigma_l2 * (gn / gd) + a.epsilon}, x, y, in, out);
}

// in[].w -> var_out where there is one.  passthrough (0 iterations): the input radiance as it is, no demodulation round trip,
// and `in` is read for the variance alone
__global__ __launch_bounds__(kBlock) void ptmi_denoise_remod(int n, const float4* __restrict__ in, const float* __restrict__ radiance,
                                                             const float4* __restrict__ albedo, int demodulate, int passthrough,
                                                             unsigned char* __restrict__ rgb8, float* __restrict__ out_radiance,
                                                             float* __restrict__ var_out) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    if (var_out) var_out[p] = in[p].w;
    float4 c;
    if (passthrough) {
        c = make_float4(radiance[3 * (size_t)p], radiance[3 * (size_t)p + 1], radiance[3 * (size_t)p + 2], 0.0f);
    } else {
        c = in[p];
        if (demodulate) {
            const float4 a = albedo[p];
            if (a.x != 0.0f) c.x = c.x * a.x;
            if (a.y != 0.0f) c.y = c.y * a.y;
            if (a.z != 0.0f) c.z = c.z * a.z;
        }
    }
    resolve_pixel(c, 1.0f, (size_t)p, rgb8, out_radiance);
}

void launch_denoise(const DenoiseArgs& a, const FeatureBuffers& fb, const float* radiance, int iterations, const float* sigma_c,
                    float4* buf, unsigned char* out_rgb8, float* out_radiance, hipStream_t s) {
    const int n = a.width * a.height;
    if (n <= 0) return;
    const dim3 grid1((n + kBlock - 1) / kBlock), block1(kBlock);
    const dim3 grid2((a.width + kTileX - 1) / kTileX, (a.height + kTileY - 1) / kTileY), block2(kTileX * kTileY);
    float4* ping[2] = {buf, buf + n};
    if (iterations > 0) hipLaunchKernelGGL(ptmi_denoise_demod, grid1, block1, 0, s, n, radiance, fb.albedo, a.demodulate, ping[0]);
    for (int i = 0; i < iterations; i++)
        hipLaunchKernelGGL(ptmi_denoise_atrous, grid2, block2, 0, s, a, fb, 1 << i, sigma_c[i], ping[i & 1], ping[(i + 1) & 1]);
    hipLaunchKernelGGL(ptmi_denoise_remod, grid1, block1, 0, s, n, ping[iterations & 1], radiance, fb.albedo, a.demodulate,
                       iterations <= 0 ? 1 : 0, out_rgb8, out_radiance, (float*)nullptr);
}

void launch_denoise_variance(const VarianceArgs& a, const FeatureBuffers& fb, const float* radiance, const TileMap& tm,
                             const AccumBuffers* moments, const unsigned int* counts, int iterations, float4* buf, float* var_in,
                             float* var_out, unsigned char* out_rgb8, float* out_radiance, hipEvent_t estimated, hipStream_t s,
                             const TemporalVariance* temporal) {
    const int n = a.width * a.height;
    if (n <= 0) { (void)hipEventRecord(estimated, s); return; }
    const dim3 grid1((n + kBlock - 1) / kBlock), block1(kBlock);
    const dim3 grid2((a.width + kTileX - 1) / kTileX, (a.height + kTileY - 1) / kTileY), block2(kTileX * kTileY);
    float4* ping[2] = {buf, buf + n};
    hipLaunchKernelGGL(ptmi_denoise_demod, grid1, block1, 0, s, n, radiance, fb.albedo, a.demodulate, ping[0]);
    launch_variance_estimate(a, fb, radiance, tm, moments, counts, ping[0], ping[1], var_in, s, temporal);
    (void)hipEventRecord(estimated, s);
    for (int i = 0; i < iterations; i++)                              // (c, v) starts in ping[1]
        hipLaunchKernelGGL(ptmi_variance_atrous, grid2, block2, 0, s, a, fb, 1 << i, ping[(i + 1) & 1], ping[i & 1]);
    hipLaunchKernelGGL(ptmi_denoise_remod, grid1, block1, 0, s, n, ping[(iterations + 1) & 1], radiance, fb.albedo, a.demodulate,
                       iterations <= 0 ? 1 : 0, out_rgb8, out_radiance, var_out);
}

}  // namespace ptmi
