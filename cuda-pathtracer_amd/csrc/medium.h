// medium.h — the participating medium (include/ptmi.h: "participating medium"; the block: host/medium.cpp), as ptmi_render_nee
// meets it after each walk and as the test hook (debug_hooks.hip: ptmi_debug_medium_call_k) calls it once per case.  binary32,
// uncontracted (-ffp-contract=off), in the order the header writes; the phase function in binary64, rounded once.
// The block's address is wave-uniform: every function reads the records it needs where it needs them, as scalar loads into
// registers that are free again at its end, so nothing of the medium lives across a walk.
#pragma once
#include "shading.h"
#include "rough.h"

namespace ptmi {

// THE SEGMENT [t0, t1] of the ray (o, d) up to t_end inside the box; false: empty
__device__ __forceinline__ bool medium_segment(const float4* __restrict__ medium, const f3& o, const f3& d, float t_end, float& t0, float& t1) {
    const float4 b0 = medium[0], b1 = medium[1];                  // (lo, sigma_t) (hi, g)
    const float lo[3] = {b0.x, b0.y, b0.z}, hi[3] = {b1.x, b1.y, b1.z};
    const float oa[3] = {o.x, o.y, o.z}, da[3] = {d.x, d.y, d.z};
    t0 = 0.0f; t1 = t_end;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (da[a] != 0.0f) {
            const float ta = (lo[a] - oa[a]) / da[a];
            const float tb = (hi[a] - oa[a]) / da[a];
            const float near = fminf(ta, tb), far = fmaxf(ta, tb);
            if (near > t0) t0 = near;
            if (far < t1) t1 = far;
        } else if (!(lo[a] <= oa[a] && oa[a] <= hi[a])) inside = false;
    }
    return inside && t1 > t0;
}

// TRANSMITTANCE of the ray's segment; 1 exactly where it is empty
__device__ __forceinline__ float medium_transmittance(const float4* __restrict__ medium, const f3& o, const f3& d, float t_end) {
    float t0, t1;
    if (!medium_segment(medium, o, d, t_end, t0, t1)) return 1.0f;
    return ptmi_expf(-(medium[0].w * (t1 - t0)));
}

// FREE FLIGHT with the draw u_m: true, the ray has a medium vertex at parameter tm
__device__ __forceinline__ bool medium_free_flight(const float4* __restrict__ medium, const f3& o, const f3& d, float t_end, float u_m, float& tm) {
    float t0, t1;
    const bool nonempty = medium_segment(medium, o, d, t_end, t0, t1);
    const float s = -((float)ptmi_log_d((double)u_m)) / medium[0].w;
    tm = t0 + s;
    return nonempty && tm < t1;
}

// THE PHASE FUNCTION: Henyey-Greenstein of the cosine c between the direction of travel and the scattered one
__device__ __forceinline__ float hg_value(float g, float c) {
    c = fminf(fmaxf(c, -1.0f), 1.0f);
    if (g == 0.0f) return (float)(1.0 / (4.0 * PTMI_PI_D));
    const double gd = (double)g, cd = (double)c;
    const double t = (1.0 + gd * gd) - (2.0 * gd) * cd;
    return (float)((1.0 - gd * gd) / ((4.0 * PTMI_PI_D) * (t * __builtin_sqrt(t))));
}
// its inversion: the sampled cosine of a uniform u
__device__ __forceinline__ float hg_sample(float g, float u) {
    const double ud = (double)u;
    if (g == 0.0f) return (float)(1.0 - 2.0 * ud);
    // The textbook inversion, ((1 + g^2) - q^2) / (2 g) with q = (1 - g^2) / (1 - g + 2 g u), expanded over s = 2 u - 1: as written
    // it subtracts two numbers near 1 and divides by 2 g, and below |g| ~ 1e-8 every cosine came out 0.  This form has no such
    // difference; both are the same rational function of (g, u).
    const double gd = (double)g;
    const double s = 2.0 * ud - 1.0;
    const double den = 1.0 + gd * s;
    const double g2 = gd * gd;
    const double num = ((s + (gd * (s * s + 3.0)) * 0.5) + g2 * s) + (g2 * gd) * ((s * s - 1.0) * 0.5);
    const double c = num / (den * den);
    return (float)fmin(fmax(c, -1.0), 1.0);
}
// the scattered direction about d for the sampled cosine c and the second draw v
__device__ __forceinline__ f3 hg_direction(const f3& d, float c, float v) {
    const float s = sqrt_rn(fmaxf(0.0f, 1.0f - c * c));
    const float phi = (float)((double)2.0f * PTMI_PI_D * (double)v);
    float sphi, cphi;
    ptmi_sincosf(phi, &sphi, &cphi);
    f3 T, B;
    rough_frame(d, T, B);
    return unit_vector((s * cphi) * T + (s * sphi) * B + c * d);
}

// the weight of a light sample of density p towards wi at a medium vertex reached along d: (ph / p) * mis(p, ph)
__device__ __forceinline__ float medium_light_weight(float g, const f3& d, const f3& wi, float p) {
    const float ph = hg_value(g, dot(d, wi));
    return (ph / p) * mis_power_heuristic(p, ph);
}

}  // namespace ptmi
