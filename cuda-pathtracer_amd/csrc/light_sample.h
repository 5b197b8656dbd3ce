// light_sample.h — the light and surface sampling functions of ptmi_render_nee (first_hit.hip), one call per vertex: emitter
// selection and the emitter sample, the environment's lookup and sample, the light sample's weight and the mirror / glass vertex.
// Here so that the test hook (debug_hooks.hip: ptmi_debug_nee_call_k) calls the functions the kernel calls.  rough.h holds the
// rough-metal vertex.  Compile with -ffp-contract=off (kernels.hip).
#pragma once

#include "shading.h"
#include "prim_sample.h"
#include "rough.h"

namespace ptmi {

// ---------------------------------------------------------------------------------------------
// next-event estimation with MIS (include/ptmi.h: ptmi_config.next_event; the contract, float for float, is written there).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int emitter_select(const EmitterTable& em, float u) {
    const float target = u * em.total;                       // u in (0, 1]: target <= total = cdf[n - 1]
    int lo = 0, hi = em.n - 1;
    while (lo < hi) {                                        // smallest j with target <= cdf[j]
        const int mid = (lo + hi) >> 1;
        if (target <= em.cdf[mid]) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// cos / M_PI of the reference's pdf_bsdf (integrator.h:128): a binary64 quotient rounded to float
__device__ __forceinline__ float cos_over_pi(float c) { return (float)((double)c / PTMI_PI_D); }

// the emitter sample of a vertex at o2: the record u_sel selects, the point (r1, r2) picks on it, the unit direction wi to it
// and the area density turned into one per solid angle (p_area; p_l: times omq where the environment is a light too)
struct EmitterSample {
    int index;                                               // the record: emitter `index` in load order of the emitters
    const float4* rec;                                       // its kEmitterStride float4 (rec[5]: Le)
    int slot;                                                // its leaf-order slot
    f3 wi;
    float dist2, cos_l, p_area, p_l;
    bool ok;                                                 // false: the sample weighs 0 (the emitter is seen edge on; a p_l of 0 or inf)
};
template <bool HAS_QUADS>
__device__ __forceinline__ EmitterSample emitter_sample(const EmitterTable& em, float u_sel, float r1, float r2, const f3& o2, bool env_on, float omq) {
    EmitterSample e;
    e.index = emitter_select(em, u_sel);
    const float4* rec = em.rec + (size_t)kEmitterStride * (size_t)e.index;
    const float4 a0 = rec[0], a1 = rec[1], a2 = rec[2], a3 = rec[3], a4 = rec[4];
    Geom g;
    g.v0 = xyz(a0); g.v1 = xyz(a1); g.v2 = xyz(a2); g.v3 = xyz(a3);
    g.type = __float_as_int(a2.w); g.ratio = a1.w;
    const f3 yv = sample_uniform<HAS_QUADS>(g, r1, r2);
    const f3 v = yv - o2;
    const float dist2 = dot(v, v);
    const float dist = sqrt_rn(dist2);
    const f3 wi = mk3(v.x / dist, v.y / dist, v.z / dist);
    const float cos_l = fabsf(dot(xyz(a4), wi));                      // a4: the geometric normal
    float p_l = (a3.w * dist2) / cos_l;
    e.p_area = p_l;
    if (env_on) p_l = omq * p_l;
    e.rec = rec; e.slot = __float_as_int(a0.w);
    e.wi = wi; e.dist2 = dist2; e.cos_l = cos_l; e.p_l = p_l;
    e.ok = cos_l > 0.0f && p_l > 0.0f && p_l <= FLT_MAX;     // a p_l of 0 or inf weighs 0 (no NaN)
    return e;
}

// ---------------------------------------------------------------------------------------------
// environment lighting (include/ptmi.h: "environment lighting"; the table: device_scene.h EnvTable).  The searches return the
// smallest index whose entry satisfies the test, as the contract writes them; every load is per lane from global memory.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int cdf_search(const float* __restrict__ cdf, int n, float u) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {                                        // smallest i with u <= cdf[i] (cdf[n - 1] = 1 >= u)
        const int mid = (lo + hi) >> 1;
        if (u <= cdf[mid]) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__device__ __forceinline__ int env_row(const EnvTable& ev, float y) {
    int lo = 0, hi = ev.h - 1;
    while (lo < hi) {                                        // smallest r with z[r + 1] < y; none (y = -1): h - 1
        const int mid = (lo + hi) >> 1;
        if (ev.z[mid + 1] < y) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// the texel a direction looks up: the nearest one, radiance is piecewise constant
__device__ __forceinline__ int env_texel(const EnvTable& ev, const f3& d) {
    const int r = env_row(ev, fminf(fmaxf(d.y, -1.0f), 1.0f));
    const float phi = ptmi_atan2f(d.z, d.x);
    const float s = (float)((double)phi / (2.0 * PTMI_PI_D));
    float t = s - ev.rot;
    t = t - floorf(t);
    const int j = min((int)(t * (float)ev.w), ev.w - 1);
    return r * ev.w + j;
}
// the environment's light sample: the texel (r, j) the two searches pick with r1, r2, a direction wi inside it by r3, r4; returns
// the texel (scaled radiance, pdf per solid angle)
__device__ __forceinline__ float4 env_sample(const EnvTable& ev, float r1, float r2, float r3, float r4, int& r, int& j, f3& wi) {
    r = cdf_search(ev.marginal, ev.h, r1);
    j = cdf_search(ev.row_cdf + (size_t)r * (size_t)ev.w, ev.w, r2);
    const float z0 = ev.z[r], z1 = ev.z[r + 1];
    const float ct = z1 + r3 * (z0 - z1);
    const float sth = sqrt_rn(fmaxf(0.0f, 1.0f - ct * ct));
    const float a = ((float)j + r4) / (float)ev.w + ev.rot;
    float sphi, cphi;
    ptmi_sincosf((float)((2.0 * PTMI_PI_D) * (double)a), &sphi, &cphi);
    wi = mk3(sth * cphi, ct, sth * sphi);
    return ev.texel[r * ev.w + j];
}

// the weight (f * cos * mis(p, p_b)) / p of a light sample of density p towards wi, f * cos without the colour: the cosine lobe,
// or the GGX lobe of a rough vertex; false: the sample contributes nothing
template <int SURF>
__device__ __forceinline__ bool light_weight(bool rough, const RoughVertex& rv, const f3& wi, float cos_s, float p, float& w) {
    if constexpr (SURF == 2) {
        if (rough) {
            float g, p_b;
            if (!rough_eval(rv, wi, g, p_b)) return false;
            w = (g * mis_power_heuristic(p, p_b)) / p;
            return true;
        }
    }
    const float p_b = cos_over_pi(cos_s);
    w = (p_b * mis_power_heuristic(p, p_b)) / p;
    return true;
}

// ---------------------------------------------------------------------------------------------
// specular surfaces (include/ptmi.h: "specular surfaces").  The mirror (kind 1) or glass (kind 2) vertex of a path along d on
// a primitive of stored normal nrm, sn the normal turned against d; u is the glass vertex's draw.  reflect: the path goes on
// along the reflected direction, else the refracted one; fr: the Fresnel reflectance (1 for a mirror and under total internal
// reflection); next: that direction, not normalised.  Returns the length test: false, no walk may start along next.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool specular_vertex(const f3& d, const f3& nrm, const f3& sn, int kind, float ior, float u, bool& reflect, float& fr, f3& next) {
    const f3 un = unit_vector(sn);
    const float dn = dot(d, un);
    reflect = true;
    fr = 1.0f;
    float eta = 1.0f, ci = 1.0f, ct = 1.0f;
    if (kind == 2) {                                                  // glass: one draw whatever comes of it
        eta = dot(d, nrm) < 0 ? 1.0f / ior : ior;                     // n_i / n_t: the stored normal points out of the body
        ci = fminf(1.0f, -dn);
        const float s2 = (eta * eta) * fmaxf(0.0f, 1.0f - ci * ci);
        if (!(s2 >= 1.0f) || eta == 1.0f) {                           // else total internal reflection
            ct = eta == 1.0f ? ci : sqrt_rn(1.0f - s2);               // ior 1 is no interface: F = 0 and next = d, exactly
            const float rs = (eta * ci - ct) / (eta * ci + ct);
            const float rp = (ci - eta * ct) / (ci + eta * ct);
            fr = 0.5f * (rs * rs + rp * rp);
            reflect = u <= fr;
        }
    }
    next = reflect ? d - (2.0f * dn) * un : eta * d + (eta * ci - ct) * un;
    const float len2 = dot(next, next);
    return len2 > 0.0f && len2 <= FLT_MAX;                            // no walk starts with a NaN direction
}

}  // namespace ptmi
