// pt_device.h — device helpers shared by the render kernels (kernels.hip and the files it lists) and the radiosity pre-pass (radiosity.hip and the files it lists).
// Compile with -ffp-contract=off (see include/ptmi_math.h, pt_vec.h).
#pragma once
#include "device_scene.h"
#include "wide_bvh.h"

#include <float.h>

#include <type_traits>

#include "../../include/ptmi_math.h"

namespace ptmi {

// Host side, the one idiom that turns a runtime flag into a template argument: f is a generic lambda and gets std::true_type or
// std::false_type (a walk is passed the same way, as a std::integral_constant<int, walk>).
template <typename F>
static decltype(auto) with_bool(bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// ---------------------------------------------------------------------------------------------
// RNG: cuRAND XORWOW restated (third-party algorithm; see oracle/ptmi_oracle.c header for status)
// ---------------------------------------------------------------------------------------------
struct Rng { uint32_t v0, v1, v2, v3, v4, d; };

__device__ __forceinline__ uint32_t rng_next(Rng& r) {
    const uint32_t t = r.v0 ^ (r.v0 >> 2);
    r.v0 = r.v1; r.v1 = r.v2; r.v2 = r.v3; r.v3 = r.v4;
    r.v4 = (r.v4 ^ (r.v4 << 4)) ^ (t ^ (t << 1));
    r.d += 362437u;
    return r.v4 + r.d;
}
// curand_uniform: x * 2^-32 + 2^-33, in (0, 1]
__device__ __forceinline__ float rng_uniform(Rng& r) {
    const uint32_t x = rng_next(r);
    return (float)x * 2.3283064e-10f + (2.3283064e-10f / 2.0f);
}

// The forms below draw the same numbers from the same states; they differ in how the state gets back into its six registers.
// rng_next under a divergent branch leaves the lanes that drew with the state rotated by one register against the lanes that
// did not, and the compiler copies at every join behind it.
// rng_uniform where `draw` holds, in straight-line code: the lanes that do not draw keep their state, by one select per word.
__device__ __forceinline__ float rng_uniform_if(Rng& r, bool draw) {
    const uint32_t t = r.v0 ^ (r.v0 >> 2);
    const uint32_t v = (r.v4 ^ (r.v4 << 4)) ^ (t ^ (t << 1));
    const uint32_t d = r.d + 362437u;
    r.v0 = draw ? r.v1 : r.v0; r.v1 = draw ? r.v2 : r.v1; r.v2 = draw ? r.v3 : r.v2; r.v3 = draw ? r.v4 : r.v3;
    r.v4 = draw ? v : r.v4; r.d = draw ? d : r.d;
    return (float)(v + d) * 2.3283064e-10f + (2.3283064e-10f / 2.0f);
}
// two rng_next in one step: three words move, the two new ones are written where they stay
__device__ __forceinline__ void rng_next2(Rng& r, uint32_t& x1, uint32_t& x2) {
    const uint32_t t1 = r.v0 ^ (r.v0 >> 2), t2 = r.v1 ^ (r.v1 >> 2);
    const uint32_t a = (r.v4 ^ (r.v4 << 4)) ^ (t1 ^ (t1 << 1));
    const uint32_t b = (a ^ (a << 4)) ^ (t2 ^ (t2 << 1));
    r.v0 = r.v2; r.v1 = r.v3; r.v2 = r.v4; r.v3 = a; r.v4 = b;
    r.d += 362437u; x1 = a + r.d;
    r.d += 362437u; x2 = b + r.d;
}
__device__ __forceinline__ void rng_uniform2(Rng& r, float& u1, float& u2) {
    uint32_t x1, x2;
    rng_next2(r, x1, x2);
    u1 = (float)x1 * 2.3283064e-10f + (2.3283064e-10f / 2.0f);
    u2 = (float)x2 * 2.3283064e-10f + (2.3283064e-10f / 2.0f);
}

// ---------------------------------------------------------------------------------------------
// primitive tests
// ---------------------------------------------------------------------------------------------
// fminf/fmaxf without the v_max_f32 x, x, x "canonicalize" the compiler puts in front of every min/max whose operand
// it cannot prove free of signalling NaNs (loop-carried closest_t, values loaded from LDS).  v_min/v_max/v_min3 return
// the other operand for a quiet NaN, exactly like fminf/fmaxf; they differ only for signalling NaNs, which no
// arithmetic instruction ever produces and the scene loader never stores.  Each avoided canonicalize is a half-rate op.
__device__ __forceinline__ float min_raw(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float max_raw(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float min3_raw(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float max3_raw(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

// Branch-free Moller-Trumbore accept test (edge1/edge2 arrive precomputed), used by all three walks.  The arithmetic
// is exactly triangle.h:64-96 / quad.h:56-87; the chain of early-outs becomes ONE sign test on a running minimum:
//   |a| <  eps  reject   <=>  |a| - eps      < 0      (IEEE subtraction never flips a sign; denormals are on)
//   u   <  0    reject   <=>  u              < 0
//   u   >  1    reject   <=>  1 - u          < 0
//   v   <  0    reject   <=>  v              < 0
//   u+v >  1    reject   <=>  1 - (u + v)    < 0
//   t > eps && t >= t_min  <=>  t - t_lo >= 0  with t_lo = max(t_min, nextafter(eps, +inf))
// fminf ignores NaN operands exactly where the reference's `x < 0 || x > 1` forms let a NaN through; the final
// `t < closest_t` (scene.h:90) rejects a NaN t.  Quad halves use the inclusive forms `|a| > eps`, `u >= 0 && ...`,
// which differ from the above only for |a| == eps (handled through eps_lo = nextafter(eps)) and for NaN u/v: the
// reference's quad rejects a NaN u that this chain ignores (tests/intersect_edge_sets.py: extent_set has the ray).  With
// |a| > eps, f is finite, so a NaN u or v needs an overflowing product of a quad edge and o - v0.  The host rules that out:
// SceneState::checkExtent refuses a scene with quads whose largest quad edge times its extent exceeds 2^124, and
// checkQuadOrigin holds the camera and the test hooks' rays to the same bound.  The bounds on edges (1e18)
// and coordinates (3e38) alone do not: 2^59 * 2^69 overflows.
// min/max/cmp/cndmask are half-rate on gfx950, add/sub/mul full-rate: 3 min + 5 sub replace 7 cmp + 7 cndmask.
__device__ __forceinline__ float mt_candidate(f3 v0, f3 edge1, f3 edge2, f3 o, f3 d, float eps_for_a, float t_lo) {
    const f3 h = cross(d, edge2);
    const float a = dot(edge1, h);
    const float f = rcp_exact_normal(a);                  // garbage for |a| < 2^-126, which the eps test rejects anyway
    const f3 s = o - v0;
    const float u = f * dot(s, h);
    // wave-level early-out: if the (a, u) tests already reject every lane that is testing this primitive, the second
    // half of Moller-Trumbore is skipped for the whole wave (coherent camera-ray waves do this for most primitives)
    const float m1 = min3_raw(fabsf(a) - eps_for_a, u, 1.0f - u);
    if (!__any(m1 >= 0.0f)) return __builtin_inff();
    const f3 q = cross(s, edge1);
    const float v = f * dot(d, q);
    const float t = f * dot(edge2, q);
    float m = min3_raw(m1, v, 1.0f - (u + v));
    m = min_raw(m, t - t_lo);
    return (m >= 0.0f) ? t : __builtin_inff();
}
// Triangle form: accept flag and t separately, so that the caller needs no +inf select (one half-rate op less)
__device__ __forceinline__ bool mt_accept(f3 v0, f3 edge1, f3 edge2, f3 o, f3 d, float eps_for_a, float t_lo, float closest_t, float& t) {
    const f3 h = cross(d, edge2);
    const float a = dot(edge1, h);
    const float f = rcp_exact_normal(a);
    const f3 s = o - v0;
    const float u = f * dot(s, h);
    const float m1 = min3_raw(fabsf(a) - eps_for_a, u, 1.0f - u);
    if (!__any(m1 >= 0.0f)) return false;
    const f3 q = cross(s, edge1);
    const float v = f * dot(d, q);
    t = f * dot(edge2, q);
    float m = min3_raw(m1, v, 1.0f - (u + v));
    m = min_raw(m, t - t_lo);
    return (m >= 0.0f) & (t < closest_t);          // t <= t_max && scene.h:90's strict t < closest_t; false for a NaN t
}
// The same test without the comparison against closest_t: the fast tree's walk (csrc/wide_bvh.h) needs to see t == closest_t
__device__ __forceinline__ bool mt_hit(f3 v0, f3 edge1, f3 edge2, f3 o, f3 d, float eps_for_a, float t_lo, float& t) {
    const f3 h = cross(d, edge2);
    const float a = dot(edge1, h);
    const float f = rcp_exact_normal(a);
    const f3 s = o - v0;
    const float u = f * dot(s, h);
    const float m1 = min3_raw(fabsf(a) - eps_for_a, u, 1.0f - u);
    if (!__any(m1 >= 0.0f)) return false;
    const f3 q = cross(s, edge1);
    const float v = f * dot(d, q);
    t = f * dot(edge2, q);
    float m = min3_raw(m1, v, 1.0f - (u + v));
    m = min_raw(m, t - t_lo);
    return m >= 0.0f;
}
// t_lo for a given t_min:  t > 1e-8f && t >= t_min  <=>  t >= t_lo
__device__ __forceinline__ float mt_t_lo(float t_min) {
    const float eps_up = __uint_as_float(__float_as_uint(1e-8f) + 1u);
    return t_min > 1e-8f ? t_min : eps_up;
}

__device__ __forceinline__ f3 xyz(const float4& v) { return mk3(v.x, v.y, v.z); }
struct f3p { float x, y, z; };      // one vector of a 36-byte triangle record (v0, e1, e2), read as a 12-byte load

// Frisvad frame (grid.h:287-297, form_factors.h:93-103, integrator.h:72-82: the same code three times)
__device__ __forceinline__ void build_frame(f3 n, f3& t, f3& b) {                 // grid.h:287-297
    if (n.z < -0.9999999f) { t = mk3(0.0f, -1.0f, 0.0f); b = mk3(-1.0f, 0.0f, 0.0f); return; }
    const float a = rcp_rn(1.0f + n.z);
    const float c = -n.x * n.y * a;
    t = mk3(1.0f - n.x * n.x * a, c, -n.x);
    b = mk3(c, 1.0f - n.y * n.y * a, -n.y);
}

// vector.h:198-203 to the sign of a zero: the reference's dot starts from `T sum = 0`, so three -0 products give +0, where
// dot() (pt_vec.h) gives -0.  Only where a local direction goes into atan2f does that sign reach a result - atan2f(+0, -0) is pi,
// atan2f(+0, +0) is 0, atan2f(-0, -1) is -pi - i.e. in grid_compute_pdf (shading.h) and direction_to_grid_index_local below, e.g.
// for dir == -normal == (-1, 0, 0); everywhere else a dot only meets comparisons and fmaxf(., 0).
__device__ __forceinline__ float dot_from_zero(f3 a, f3 b) { float s = 0.0f; s += a.x * b.x; s += a.y * b.y; s += a.z * b.z; return s; }

// direction_to_grid_indices_local (form_factors.h:107-130): theta over [0, pi] -> 16 rows, phi over [0, 2 pi) -> 16 columns.
// The form-factor kernel (form_factors.hip) and ptmi_radiosity_grid (radiosity.hip) bin with it; here so that the test hook (debug_hooks.hip) calls the same function.
__device__ __forceinline__ int direction_to_grid_index_local(f3 world_dir, f3 normal) {
    f3 tangent, bitangent;
    build_frame(normal, tangent, bitangent);
    const float lx = dot_from_zero(world_dir, tangent), ly = dot_from_zero(world_dir, bitangent), lz = dot(world_dir, normal);
    const float r = sqrt_rn(lx * lx + ly * ly + lz * lz);
    const float theta = (r > 0.0f) ? ptmi_acosf(fminf(lz / r, 1.0f)) : 0.0f;
    float phi = ptmi_atan2f(ly, lx);
    if (phi < 0.0f) phi = (float)((double)phi + (double)2.0f * PTMI_PI_D);
    int grid_theta = (int)fminf((float)(((double)theta / PTMI_PI_D) * kGridRes), (float)(kGridRes - 1));
    int grid_phi = (int)fminf((float)(((double)phi / ((double)2.0f * PTMI_PI_D)) * kGridRes), (float)(kGridRes - 1));
    grid_theta = max(0, min(grid_theta, kGridRes - 1));
    grid_phi = max(0, min(grid_phi, kGridRes - 1));
    return grid_theta * kGridRes + grid_phi;
}

// resolve of one pixel (integrator.h:393-407): colour sum x k -> float radiance; Reinhard, gamma 1/2.2, 8 bit -> rgb8 (either
// output may be nullptr).  The frame and pass resolves (kernels.hip) and the denoiser's tone map (denoise.hip, k = 1) share it.
__device__ __forceinline__ void resolve_pixel(const float4& D, float k, size_t out, unsigned char* __restrict__ rgb8,
                                              float* __restrict__ radiance) {
    const float c[3] = {D.x * k, D.y * k, D.z * k};
    const float gamma = 1.0f / 2.2f;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        if (radiance) radiance[out * 3 + ch] = c[ch];
        if (rgb8) {
            const float tm_ = c[ch] / (c[ch] + 1.0f);       // color / (color + 1), component-wise true division
            const float g = ptmi_powf(tm_, gamma);
            rgb8[out * 3 + ch] = (unsigned char)(255.99f * fminf(g, 1.0f));
        }
    }
}

}  // namespace ptmi
