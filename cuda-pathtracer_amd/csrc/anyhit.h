// anyhit.h — the radiosity solver's visibility question, stated once: is ANY primitive other than the pair's own two hit within
// max_dist (visibility_test_anyhit, form_factors.h:143-208).  The primitive and box tests, the reference's walk
// (visibility_blocked), the walk over the 8-wide fast tree with and without the certified walk's proof (visibility_blocked_wide,
// certified_blocked; csrc/wide_walk.h) and PAIR_BLOCKED, the one call that the form-factor kernel (form_factors.hip) makes.
// Everything is inlined into that kernel.
#pragma once
#include "pt_device.h"
#include "wide_walk.h"

namespace ptmi {

// the slopes of visibility_test_anyhit's slab test (form_factors.h:157-160): a component within 1e-8 of zero counts as 1e-8.
// (The walk over the fast tree clamps its own way, wide_inv: its boxes are padded for that.)
__device__ __forceinline__ f3 anyhit_inv(f3 d) {
    return mk3(1.0f / (fabsf(d.x) > 1e-8f ? d.x : 1e-8f), 1.0f / (fabsf(d.y) > 1e-8f ? d.y : 1e-8f), 1.0f / (fabsf(d.z) > 1e-8f ? d.z : 1e-8f));
}

// Triangle::intersect(r, 1e-5f, max_dist) (triangle.h:64-96) on a record of v0, edge1, edge2, as pt_device.h's branch-free
// Moller-Trumbore (eps 1e-8, t > 1e-8f && t >= 1e-5f, t <= max_dist), in the two stages that its callers leave between:
// anyhit_prim when the u stage rejects for the whole wave (m1 < 0 everywhere), the wide walk's per-lane loop for its own lane.
// One function with the early-out as a template argument moves the certified kernels' registers (EXPERIMENTS.md).
struct TriU { f3 s; float f, u, m1; };
__device__ __forceinline__ TriU anyhit_tri_u(f3 v0, f3 edge1, f3 edge2, f3 o, f3 d) {
    const f3 h = cross(d, edge2);
    const float a = dot(edge1, h);
    TriU k;
    k.f = rcp_exact_normal(a);
    k.s = o - v0;
    k.u = k.f * dot(k.s, h);
    k.m1 = min3_raw(fabsf(a) - 1e-8f, k.u, 1.0f - k.u);
    return k;
}
__device__ __forceinline__ bool anyhit_tri_t(const TriU& k, f3 edge1, f3 edge2, f3 d, float max_dist, float& t) {
    const f3 q = cross(k.s, edge1);
    const float v = k.f * dot(d, q);
    t = k.f * dot(edge2, q);
    float m = min3_raw(k.m1, v, 1.0f - (k.u + v));
    m = min_raw(m, t - 1e-5f);
    return (m >= 0.0f) & (t <= max_dist);
}
// Quad::intersect under the upper bound max_dist (quad.h:56-121): the smaller t of the two halves, +inf for none; the caller
// accepts t < max_dist only (quad.h:78,110)
__device__ __forceinline__ float anyhit_quad_t(f3 v0, f3 v1, f3 v2, f3 v3, f3 o, f3 d) {
    const float eps_up = __uint_as_float(__float_as_uint(1e-8f) + 1u);
    return min_raw(mt_candidate(v0, v1, v2, o, d, eps_up, 1e-5f), mt_candidate(v0, v2, v3, o, d, eps_up, 1e-5f));
}

// Primitive::intersect(r, 1e-5f, max_dist) as a yes/no question: triangle.h:82 accepts t <= t_max, quad.h:78,110
// only t < t_max (closest_t starts at t_max)
template <bool HAS_QUADS>
__device__ __forceinline__ bool anyhit_prim(const float4* __restrict__ prims, int prim_stride, int k, f3 o, f3 d, float max_dist) {
    const float4 p0 = prims[k * prim_stride], p1 = prims[k * prim_stride + 1], p2 = prims[k * prim_stride + 2];
    if (HAS_QUADS && __float_as_int(p0.w) != 0) {
        const float4 p3 = prims[k * prim_stride + 3];
        return anyhit_quad_t(xyz(p0), xyz(p1), xyz(p2), xyz(p3), o, d) < max_dist;
    }
    const f3 v0 = xyz(p0), edge1 = xyz(p1), edge2 = xyz(p2);
    const TriU ku = anyhit_tri_u(v0, edge1, edge2, o, d);
    if (!__any(ku.m1 >= 0.0f)) return false;
    float t;
    return anyhit_tri_t(ku, edge1, edge2, d, max_dist, t);
}

// slab test of visibility_test_anyhit (form_factors.h:162-180); true = the reference does NOT `continue`
__device__ __forceinline__ bool anyhit_box(const float4& n0, const float4& n1, f3 o, f3 inv, float max_dist) {
    const float EPSILON = 1e-5f;
    float t1 = (n0.x - o.x) * inv.x, t2 = (n1.x - o.x) * inv.x;
    float tmin = min_raw(t1, t2), tmax = max_raw(t1, t2);
    t1 = (n0.y - o.y) * inv.y; t2 = (n1.y - o.y) * inv.y;
    tmin = max_raw(tmin, min_raw(t1, t2)); tmax = min_raw(tmax, max_raw(t1, t2));
    t1 = (n0.z - o.z) * inv.z; t2 = (n1.z - o.z) * inv.z;
    tmin = max_raw(tmin, min_raw(t1, t2)); tmax = min_raw(tmax, max_raw(t1, t2));
    return !(tmax < EPSILON || tmin > max_dist || tmin > tmax);
}

// visibility_test_anyhit (form_factors.h:143-208).  The answer - is ANY primitive other than source/target hit within
// max_dist - does not depend on the visiting order unless children get dropped (stack_ptr >= 30), which needs a tree
// deeper than 31 levels.  DEEP = false: stackless pre-order walk (skip pointers).  DEEP = true: the reference's walk
// itself - 32-entry stack, left pushed first (so the right child is visited first), children dropped from 30 on.
template <bool HAS_QUADS, bool DEEP>
__device__ __forceinline__ bool visibility_blocked(const DeviceScene& sc, f3 o, f3 d, float max_dist, int slot_a, int slot_b) {
    const f3 inv = anyhit_inv(d);
    const float4* __restrict__ nodes = sc.nodes;
    if (!DEEP) {
        // while-while: every lane first walks nodes until it stands on a leaf whose box it hits (or runs out of
        // nodes), then the lanes test their leaves together - node steps and primitive tests do not serialise
        int cur = 0;
        const int n_nodes = sc.n_nodes;
        while (true) {
            int first = 0, count = 0;
            while (cur < n_nodes) {
                const float4 n0 = nodes[2 * cur], n1 = nodes[2 * cur + 1];
                const int a = __float_as_int(n0.w), b = __float_as_int(n1.w);
                const bool pass = anyhit_box(n0, n1, o, inv, max_dist);
                const int here = cur;
                cur = (!pass && b >= 0) ? a : here + 1;
                if (pass && b < 0) { first = a; count = -b; break; }
            }
            if (count == 0) return false;
            for (int i = 0; i < count; i++) {
                const int k = first + i;
                if (k == slot_a || k == slot_b) continue;
                if (anyhit_prim<HAS_QUADS>(sc.prims, sc.prim_stride, k, o, d, max_dist)) return true;
            }
        }
    } else {
        int stack[32];
        int sp = 0;
        stack[sp++] = 0;
        while (sp > 0) {
            const int cur = stack[--sp];
            const float4 n0 = nodes[2 * cur], n1 = nodes[2 * cur + 1];
            if (!anyhit_box(n0, n1, o, inv, max_dist)) continue;
            const int a = __float_as_int(n0.w), b = __float_as_int(n1.w);
            if (b < 0) {
                for (int i = 0; i < -b; i++) {
                    const int k = a + i;
                    if (k == slot_a || k == slot_b) continue;
                    if (anyhit_prim<HAS_QUADS>(sc.prims, sc.prim_stride, k, o, d, max_dist)) return true;
                }
            } else if (sp < 30) {
                stack[sp++] = cur + 1;      // left child (pre-order numbering)
                stack[sp++] = b;            // right child: popped first
            }
        }
        return false;
    }
}

// The same question through the opt-in fast tree (ptmi_config.fast_tree; csrc/wide_bvh.h): is any triangle other than the
// pair's own two hit within max_dist.  Same triangles, same test arithmetic (anyhit_prim's triangle form on the tree's own
// 36-byte records), conservative boxes: the answer is the reference's unless the reference's own slab test drops, by rounding,
// the box of a triangle that the ray does hit.  Stack: one 8-byte entry per tree level, entry e of lane l at stack[e * kBlock].
//
// CERT (the default for triangle scenes from RadiosityState::cert_min_prims = 256 primitives up): the reference's answer for every ray, by proof.
//   "not blocked" needs none: the fast walk reaches every triangle whose hit point lies in range (conservative boxes), the
//     reference's walk tests a subset of them with the same arithmetic.
//   "blocked by triangle k at t": the reference tests k iff every box on the way from its root to k's leaf passes ITS slab
//     test (anyhit_box - no closest-hit distance in it, so the visiting order does not matter): the proof of csrc/wide_walk.h
//     with anyhit_box as the chain's slab test and |d_a| >= 2^-26; a box of the chain failing: the reference's own walk for this ray.
// 2^-26 > 1e-8: above it anyhit_box's 1 / d is the reference's finite slope (wide_walk.h: the proof's slope bound)
constexpr float kCertSlopeSolver = 1.4901161193847656e-8f;
template <bool QUADS>
__device__ __forceinline__ bool certified_blocked(const DeviceScene& sc, float4 lo, float4 hi, float t, f3 o, f3 d, float max_dist, int slot_a, int slot_b, unsigned long long& chain) {
    const f3 q = o + t * d;
    const bool inside = CERT_LEAF_INSIDE(o, q, lo, hi);
    const bool slopes = CERT_SLOPES_OK(d, kCertSlopeSolver);
    if (inside && slopes && sc.w_cert_debug == 0) return true;
    chain++;
    const f3 inv = anyhit_inv(d);
    // The chain of wide_walk.h in its own spelling: anyhit_box only below the first box that holds Q, the margin as an && chain.
    // Through cert_chain (CERT_CHUNK: every box's slab test, the margin as a min3) the form-factor kernel spills more and the
    // solver took 5 % longer (n = 8192, certified walk: 85.4 against 80.9 ms).
    uint32_t off = cert_first_chunk(lo);
    bool ok = cert_chunks(lo) != 0u, proven = false;          // no list: fails closed
    for (int left = (int)cert_chunks(lo); left > 0 && ok && !proven; left--, off++) {
        const uint4 idx = sc.wanc[off];
        const uint32_t ni[4] = {idx.x, idx.y, idx.z, idx.w};
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint32_t j = ni[c] == 0xffffffffu ? 0u : ni[c];          // padding repeats the root
            const float4 n0 = sc.nodes[2 * (size_t)j], n1 = sc.nodes[2 * (size_t)j + 1];
            const bool holds = slopes && CERT_LEAF_INSIDE(o, q, n0, n1);
            ok = ok && (proven || holds || anyhit_box(n0, n1, o, inv, max_dist));
            proven = proven || holds;
        }
    }
    if (ok && sc.w_cert_debug < 2) return true;
    chain += 1ull << 32;
    return visibility_blocked<QUADS, false>(sc, o, d, max_dist, slot_a, slot_b);
}

template <bool CERT, bool QUADS>
__device__ __forceinline__ bool visibility_blocked_wide(const DeviceScene& sc, uint2* stack, f3 o, f3 d, float max_dist, int load_a, int load_b,
                                                        int slot_a, int slot_b, unsigned long long& chain) {
    const f3 inv = mk3(wide_inv(d.x), wide_inv(d.y), wide_inv(d.z));
    const uint32_t octinv = wide_octinv(inv);
    int sp = 0;
    uint32_t g_base = 0u, g_bits = (1u << 8) | (1u << octinv);
    while (true) {
        WIDE_NEXT_NODE(ni, g_base, g_bits, sp, stack, octinv, if (sp == 0) return false);
        const uint4* q = sc.wnodes + 8 * (size_t)ni;
        const WideStep st = wide_node_test(q[0], q[1], q[2], q[3], q[4], q[5], q[6], o, inv, octinv, 1e-5f, max_dist);
        uint32_t tris = st.tris;
        while (tris) {
            const int k = (int)st.tri_base + __ffs((int)tris) - 1;
            tris &= tris - 1u;
            const int li = sc.wload_index[k];
            if (li == load_a || li == load_b) continue;
            if (QUADS && __float_as_int(sc.wqprims[4 * (size_t)k].w) != 0) {       // a quad: quad.h:78,110 accept t < t_max only
                const float4* q = sc.wqprims + 4 * (size_t)k;
                const float tq = anyhit_quad_t(xyz(q[0]), xyz(q[1]), xyz(q[2]), xyz(q[3]), o, d);
                if (!(tq < max_dist)) continue;
                if (!CERT) return true;
                const float4 c_lo = sc.wcert[kWideCertStride * (size_t)k], c_hi = sc.wcert[kWideCertStride * (size_t)k + 1];
                return certified_blocked<QUADS>(sc, c_lo, c_hi, tq, o, d, max_dist, slot_a, slot_b, chain);
            }
            const float* r = sc.wprims + 9 * (size_t)k;
            const f3 v0 = mk3(r[0], r[1], r[2]), edge1 = mk3(r[3], r[4], r[5]), edge2 = mk3(r[6], r[7], r[8]);
            const TriU ku = anyhit_tri_u(v0, edge1, edge2, o, d);
            if (!(ku.m1 >= 0.0f)) continue;
            float t;
            if (anyhit_tri_t(ku, edge1, edge2, d, max_dist, t)) {
                if (!CERT) return true;
                // (fetching the leaf box together with the triangle record, before the test: no gain - n = 8192: 84.0 vs 84.4 ms)
                const float4 c_lo = sc.wcert[kWideCertStride * (size_t)k], c_hi = sc.wcert[kWideCertStride * (size_t)k + 1];
                return certified_blocked<QUADS>(sc, c_lo, c_hi, t, o, d, max_dist, slot_a, slot_b, chain);
            }
        }
        g_base = st.child_base; g_bits = (st.imask << 8) | st.inner;
    }
}

// The front door: the answer for the pair (i, j) of load-order indices whose leaf slots are slot_i, slot_j.  The only place that
// knows what each walk tells the pair's own two primitives by: the fast tree's by load-order index (and, on the certified walk's
// way back to the reference's walk, by leaf slot), the reference's walk by leaf slot alone.  A macro that expands to the
// expression its two callers had: as a function it moves the kernel's register allocation (EXPERIMENTS.md).
#define PAIR_BLOCKED(WIDE, HAS_QUADS, DEEP, sc, wstack, o, d, max_dist, i, j, slot_i, slot_j, chain)                              \
    ((WIDE) ? visibility_blocked_wide<(WIDE) == 2, HAS_QUADS>(sc, wstack, o, d, max_dist, i, j, slot_i, slot_j, chain)            \
            : visibility_blocked<HAS_QUADS, DEEP>(sc, o, d, max_dist, slot_i, slot_j))

}  // namespace ptmi
