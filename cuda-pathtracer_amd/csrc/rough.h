// rough.h — rough metal (include/ptmi.h: "rough metal"): the isotropic GGX reflector of ptmi_render_nee's SURF = 2 instantiations.
// Everything is float32 in the header's order (the build forbids contraction); a2 is alpha * alpha.  A vertex's local frame is
// (T, B, un) with z along the unit shading normal; nothing here lives across a walk.
#pragma once

#include "shading.h"

namespace ptmi {

constexpr float kRoughMinCos2 = 1e-37f;                      // PTMI_ROUGH_MIN_COS2: below it 1 / (c * c) may overflow

struct RoughVertex {
    f3 un, T, B, wo;                                         // the frame and -d in it; co = wo.z
    float alpha, a2, lo;                                     // lo = Lambda(co)
    bool ok;                                                 // false: the grazing exit (co * co > PTMI_ROUGH_MIN_COS2 does not hold)
};

__device__ __forceinline__ float rough_lambda(float a2, float c) {
    const float c2 = c * c;
    return 0.5f * (sqrt_rn(1.0f + a2 * ((1.0f - c2) / c2)) - 1.0f);
}
// D of the unit half vector h; t is h.z^2 (a2 - 1) + 1 written without the cancellation that form has at a narrow lobe's peak
__device__ __forceinline__ float rough_d(float a2, f3 h) {
    const float t = (h.x * h.x + h.y * h.y) + a2 * (h.z * h.z);
    return a2 / (((float)PTMI_PI_D * t) * t);
}
__device__ __forceinline__ bool rough_cos_ok(float c) { return c > 0.0f && c * c > kRoughMinCos2; }   // false for a NaN

// the tangent frame sampleCosineHemisphere builds from its normal (cosine_hemisphere above), same two branches
__device__ __forceinline__ void rough_frame(f3 n, f3& tangent, f3& bitangent) {
    if (n.z < -0.9999999f) {
        tangent = mk3(0.0f, -1.0f, 0.0f);
        bitangent = mk3(-1.0f, 0.0f, 0.0f);
    } else {
        const float a = rcp_rn(1.0f + n.z);
        const float b = -n.x * n.y * a;
        tangent = mk3(1.0f - n.x * n.x * a, b, -n.x);
        bitangent = mk3(b, 1.0f - n.y * n.y * a, -n.y);
    }
}

__device__ __forceinline__ RoughVertex rough_vertex(f3 sn, f3 d, float alpha) {
    RoughVertex v;
    v.un = unit_vector(sn);
    rough_frame(v.un, v.T, v.B);
    const f3 md = -d;
    v.wo = mk3(dot(md, v.T), dot(md, v.B), dot(md, v.un));
    v.alpha = alpha; v.a2 = alpha * alpha;
    v.ok = rough_cos_ok(v.wo.z);
    v.lo = v.ok ? rough_lambda(v.a2, v.wo.z) : 0.0f;
    return v;
}

// the light sample towards wi (world): g = f * cos / tint and p_b, the density with which rough_sample produces wi
__device__ __forceinline__ bool rough_eval(const RoughVertex& v, f3 wi, float& g, float& p_b) {
    if (!v.ok) return false;
    const f3 wl = mk3(dot(wi, v.T), dot(wi, v.B), dot(wi, v.un));
    if (!rough_cos_ok(wl.z)) return false;
    const f3 h = unit_vector(v.wo + wl);
    const float dh = rough_d(v.a2, h);
    const float four_co = 4.0f * v.wo.z, one_lo = 1.0f + v.lo;
    g = dh / (four_co * (one_lo + rough_lambda(v.a2, wl.z)));
    p_b = dh / (four_co * one_lo);
    return true;
}

// the BSDF sample by visible normals (Heitz 2018): next (world, not normalised), the weight beta takes and the density of next
__device__ __forceinline__ bool rough_sample(const RoughVertex& v, float u1, float u2, f3& next, float& weight, float& p_b) {
    const f3 vh = unit_vector(mk3(v.alpha * v.wo.x, v.alpha * v.wo.y, v.wo.z));
    const float lensq = vh.x * vh.x + vh.y * vh.y;
    f3 t1v = mk3(1.0f, 0.0f, 0.0f);
    if (lensq > 0.0f) {
        const float l = sqrt_rn(lensq);
        t1v = mk3(-vh.y / l, vh.x / l, 0.0f);
    }
    const f3 t2v = cross(vh, t1v);
    const float r = sqrt_rn(u1);
    const float phi = (float)((2.0 * PTMI_PI_D) * (double)u2);
    float sphi, cphi;
    ptmi_sincosf(phi, &sphi, &cphi);
    const float t1 = r * cphi;
    float t2 = r * sphi;
    const float s = 0.5f * (1.0f + vh.z);
    t2 = (1.0f - s) * sqrt_rn(fmaxf(0.0f, 1.0f - t1 * t1)) + s * t2;
    const f3 nh = t1 * t1v + t2 * t2v + sqrt_rn(fmaxf(0.0f, 1.0f - t1 * t1 - t2 * t2)) * vh;
    const f3 h = unit_vector(mk3(v.alpha * nh.x, v.alpha * nh.y, fmaxf(0.0f, nh.z)));
    const f3 wl = (2.0f * dot(v.wo, h)) * h - v.wo;
    if (!rough_cos_ok(wl.z)) return false;
    const float one_lo = 1.0f + v.lo;
    weight = one_lo / (one_lo + rough_lambda(v.a2, wl.z));
    p_b = rough_d(v.a2, h) / ((4.0f * v.wo.z) * one_lo);
    next = wl.x * v.T + wl.y * v.B + wl.z * v.un;
    return true;
}

}  // namespace ptmi
