// temporal.hip — gfx950 kernel of the temporal accumulation with reprojection (the temporal stage of SVGF, Schied et al., 2017)
// over the feature buffers of ptmi_render_features.  The step is defined, operation by operation, in include/ptmi.h
// (ptmi_temporal_accumulate); every value here is float32 in the order written there (built with -ffp-contract=off and
// correctly rounded division), so a numpy float32 restatement reproduces it bit for bit.
//
// Kernels
//   ptmi_temporal_reproject          per pixel: the reprojection point into the history's view, 4 bilinear taps of the history gated by
//                                    normal, position and albedo, the blend by sample count; the new history (colour and count, features) goes
//                                    to the other side of the ping-pong, the result through the frame's tone map -> rgb8 + radiance
//   ptmi_temporal_reproject_moments  the same step (one body, temporal_pixel) with the luminance statistics (mu, s2, k) of
//                                    ptmi_set_temporal_moments resampled by the same taps and blended by the same alpha
// One thread per pixel; a thread reads only the previous side of the history and writes only its own pixel of the next side,
// so the result does not depend on the launch geometry.
#include "denoise_common.h"

namespace ptmi {

enum : int { kTemporalAccepted = 0, kTemporalRejected = 1, kTemporalMissed = 2 };

// THE STEP of one pixel.  MOMENTS: prev_mom / next_mom are the two sides of the statistics' ping-pong (else not touched).
template <bool MOMENTS>
__device__ __forceinline__ void temporal_pixel(const TemporalArgs& a, const FeatureBuffers& fb, const float* __restrict__ radiance,
                                               const unsigned int* __restrict__ counts, const TemporalHistory& prev,
                                               const TemporalHistory& next, unsigned char* __restrict__ rgb8,
                                               float* __restrict__ out_radiance, unsigned long long* __restrict__ stats,
                                               const float4* __restrict__ prev_mom, float4* __restrict__ next_mom) {
    const int n = a.width * a.height;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    const bool live = p < n;
    int outcome = kTemporalRejected;
    if (live) {
        const float m = counts ? (float)counts[p] : a.m;
        const f3 cur = mk3(radiance[3 * (size_t)p], radiance[3 * (size_t)p + 1], radiance[3 * (size_t)p + 2]);
        const float4 al = fb.albedo[p], nr = fb.normal[p], ps = fb.position[p];
        const float hf = al.w;
        bool reuse = false;
        f3 h = mk3(0.0f, 0.0f, 0.0f);
        float nacc = 0.0f;
        float mu_h = 0.0f, s2_h = 0.0f, k_h = 0.0f;
        if (a.history && a.still) {                          // the only tap is the pixel itself, weight 1
            const float4 c = prev.color[p];
            h = mk3(c.x, c.y, c.z); nacc = c.w;
            if (MOMENTS) { const float4 hm = prev_mom[p]; mu_h = hm.x; s2_h = hm.y; k_h = hm.z; }
            reuse = true;
        } else if (a.history && hf != 0.0f) {
            const f3 x = mk3(ps.x / hf, ps.y / hf, ps.z / hf);
            const f3 nc = mk3(nr.x / hf, nr.y / hf, nr.z / hf);
            const f3 ac = mk3(al.x / hf, al.y / hf, al.z / hf);
            const f3 o = mk3(a.cam[0], a.cam[1], a.cam[2]), llc = mk3(a.cam[3], a.cam[4], a.cam[5]);
            const f3 hor = mk3(a.cam[6], a.cam[7], a.cam[8]), ver = mk3(a.cam[9], a.cam[10], a.cam[11]);
            const f3 f = llc - o;
            const f3 nrm = cross(hor, ver);
            const f3 d = x - o;
            const float den = dot(d, nrm), fn = dot(f, nrm);
            const float sp = dot(nc, o - x), sc = dot(nc, mk3(a.origin[0], a.origin[1], a.origin[2]) - x);
            if (((fn > 0.0f && den > 0.0f) || (fn < 0.0f && den < 0.0f)) &&       // in front of the previous camera's plane
                ((sp > 0.0f && sc > 0.0f) || (sp < 0.0f && sc < 0.0f))) {          // both cameras on the same side of the surface
                const float s = fn / den;
                const f3 q = s * d - f;
                const float u = dot(q, hor) / dot(hor, hor);
                const float v = dot(q, ver) / dot(ver, ver);
                const float px = u * (float)a.width - 0.5f, py = v * (float)a.height - 0.5f;
                // beyond these bounds every tap lies outside the image (and the conversions below stay in range)
                if (px >= -1.0f && px < (float)a.width && py >= -1.0f && py < (float)a.height) {
                    const float x0f = floorf(px), y0f = floorf(py);
                    const float fx = px - x0f, fy = py - y0f;
                    const int x0 = (int)x0f, y0 = (int)y0f;
                    const float gx = 1.0f - fx, gy = 1.0f - fy;
                    float W = 0.0f, Sx = 0.0f, Sy = 0.0f, Sz = 0.0f, Sn = 0.0f;
                    float Sm = 0.0f, Ss = 0.0f, Sk = 0.0f;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int tx = x0 + (k & 1), ty = y0 + (k >> 1);
                        if (tx < 0 || tx >= a.width || ty < 0 || ty >= a.height) continue;
                        const int t = ty * a.width + tx;
                        const float4 hn = prev.normal[t];
                        if (hn.w == 0.0f) continue;                                   // every feature ray of the tap missed
                        const float4 hp = prev.position[t];
                        const f3 np = mk3(hn.x / hn.w, hn.y / hn.w, hn.z / hn.w);
                        if (!(dot(nc, np) >= a.normal_min)) continue;
                        const f3 e = x - mk3(hp.x / hn.w, hp.y / hn.w, hp.z / hn.w);
                        if (!(dot(e, e) <= a.sigma_x2)) continue;
                        const float4 ha = prev.albedo[t];
                        const f3 ea = ac - mk3(ha.x / hn.w, ha.y / hn.w, ha.z / hn.w);
                        if (!(dot(ea, ea) <= a.sigma_a2)) continue;
                        const float4 hc = prev.color[t];
                        const float w = (k & 1 ? fx : gx) * (k >> 1 ? fy : gy);     // (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy
                        W = W + w;
                        Sx = Sx + w * hc.x; Sy = Sy + w * hc.y; Sz = Sz + w * hc.z;
                        Sn = Sn + w * hc.w;
                        if (MOMENTS) {
                            const float4 hm = prev_mom[t];
                            Sm = Sm + w * hm.x; Ss = Ss + w * hm.y; Sk = Sk + w * hm.z;
                        }
                    }
                    if (W > 0.01f) {
                        h = mk3(Sx / W, Sy / W, Sz / W);
                        nacc = Sn / W;
                        if (MOMENTS) { mu_h = Sm / W; s2_h = Ss / W; k_h = Sk / W; }
                        reuse = true;
                    }
                }
            }
        }
        f3 c = cur;                                                          // a restart: the input as it is
        float cnt = m;
        float mu = 0.0f, s2 = 0.0f, kf = 1.0f;
        if (MOMENTS) mu = denoise_lum(cur.x, cur.y, cur.z);
        if (reuse) {
            cnt = fminf(nacc + m, a.max_history * m);
            const float alpha = m / cnt;
            c = mk3(h.x + alpha * (cur.x - h.x), h.y + alpha * (cur.y - h.y), h.z + alpha * (cur.z - h.z));
            if (MOMENTS) {                                                   // West's weighted update in blend form
                const float d = mu - mu_h;
                mu = mu_h + alpha * d;
                s2 = (1.0f - alpha) * (s2_h + alpha * (d * d));
                kf = fminf(k_h + 1.0f, a.max_history);
            }
            outcome = kTemporalAccepted;
        } else {
            outcome = hf == 0.0f ? kTemporalMissed : kTemporalRejected;
        }
        next.color[p] = make_float4(c.x, c.y, c.z, cnt);
        if (MOMENTS) next_mom[p] = make_float4(mu, s2, kf, 0.0f);
        float4 hn = nr;
        hn.w = hf;                                                           // (the feature pass writes 0 there)
        next.normal[p] = hn;
        next.position[p] = ps;
        next.albedo[p] = make_float4(al.x, al.y, al.z, hf);
        resolve_pixel(make_float4(c.x, c.y, c.z, 0.0f), 1.0f, (size_t)p, rgb8, out_radiance);
    }
    // one atomic per wave and outcome (every lane reaches the ballots: no early return above)
    const unsigned long long acc = __ballot(live && outcome == kTemporalAccepted);
    const unsigned long long rej = __ballot(live && outcome == kTemporalRejected);
    const unsigned long long mis = __ballot(live && outcome == kTemporalMissed);
    if ((threadIdx.x & 63) == 0) {
        if (acc) atomicAdd(&stats[0], (unsigned long long)__popcll(acc));
        if (rej) atomicAdd(&stats[1], (unsigned long long)__popcll(rej));
        if (mis) atomicAdd(&stats[2], (unsigned long long)__popcll(mis));
    }
}

__global__ __launch_bounds__(kBlock) void ptmi_temporal_reproject(TemporalArgs a, FeatureBuffers fb, const float* __restrict__ radiance,
                                                                  const unsigned int* __restrict__ counts, TemporalHistory prev,
                                                                  TemporalHistory next,
                                                                  unsigned char* __restrict__ rgb8, float* __restrict__ out_radiance,
                                                                  unsigned long long* __restrict__ stats) {
    temporal_pixel<false>(a, fb, radiance, counts, prev, next, rgb8, out_radiance, stats, nullptr, nullptr);
}

// the statistics' two sides are trailing arguments of their own: the argument block above does not move
__global__ __launch_bounds__(kBlock) void ptmi_temporal_reproject_moments(TemporalArgs a, FeatureBuffers fb, const float* __restrict__ radiance,
                                                                          const unsigned int* __restrict__ counts, TemporalHistory prev,
                                                                          TemporalHistory next,
                                                                          unsigned char* __restrict__ rgb8, float* __restrict__ out_radiance,
                                                                          unsigned long long* __restrict__ stats,
                                                                          const float4* __restrict__ prev_mom, float4* __restrict__ next_mom) {
    temporal_pixel<true>(a, fb, radiance, counts, prev, next, rgb8, out_radiance, stats, prev_mom, next_mom);
}

void launch_temporal(const TemporalArgs& a, const FeatureBuffers& fb, const float* radiance, const unsigned int* counts,
                     const TemporalHistory& prev, const TemporalHistory& next, unsigned char* rgb8,
                     float* out_radiance, unsigned long long* stats, hipStream_t s, const float4* prev_moments, float4* next_moments) {
    const int n = a.width * a.height;
    if (n <= 0) return;
    const dim3 grid((n + kBlock - 1) / kBlock), block(kBlock);
    if (next_moments)
        hipLaunchKernelGGL(ptmi_temporal_reproject_moments, grid, block, 0, s, a, fb, radiance, counts, prev, next, rgb8, out_radiance,
                           stats, prev_moments, next_moments);
    else
        hipLaunchKernelGGL(ptmi_temporal_reproject, grid, block, 0, s, a, fb, radiance, counts, prev, next, rgb8, out_radiance, stats);
}

}  // namespace ptmi
