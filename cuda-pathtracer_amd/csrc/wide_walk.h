// wide_walk.h — the device side of the walks over the 8-wide fast tree (csrc/wide_bvh.h) and of the certified walk's proof
// (DESIGN.md §4.9), each stated once.  ptmi_bounce_wide (bounce_wide.hip) runs these steps in phases; the Radiosity view, the
// feature pass and the test hook run wide_closest_hit; the solver (anyhit.h) runs its any-hit walk over WIDE_NEXT_NODE
// and proves its hits with the chain in its own spelling (certified_blocked).
//
// The steps that ptmi_bounce_wide runs in place are macros that expand to exactly the statements the kernel had before they
// were shared (GNU statement expressions where a value comes out).  As __forceinline__ functions they change the register
// allocation of ptmi_bounce_wide: the compiler simplifies a function on its own before it inlines it, and the kernel's
// variables passed by reference stay in memory until then.  That kernel's code must not change.
#pragma once
#include "pt_device.h"

namespace ptmi {

// ---- the walk -----------------------------------------------------------------------------------------------------------
// A ray's walk state at its start: the clamped slopes, the ray's octant, and the root as slot 0 of a virtual parent
#define WIDE_WALK_BEGIN(d, inv, octinv, g_base, g_bits) \
    { (inv) = mk3(wide_inv((d).x), wide_inv((d).y), wide_inv((d).z)); (octinv) = wide_octinv(inv); (g_base) = 0u; (g_bits) = (1u << 8) | (1u << (octinv)); }

// One step: declares ni = the node to enter next - the highest pending bit of the current group (bit ^ octinv = the child's
// slot), its index = child_base + the inner children in lower slots.  An exhausted group is replaced by the one on top of the
// stack; on_empty runs first (a walk that can end there checks sp == 0 and leaves).  The group goes back on the stack while it
// has children left.  stack: this lane's column in LDS, entry e at stack[e * kBlock].  The caller fetches the node.
#define WIDE_NEXT_NODE(ni, g_base, g_bits, sp, stack, octinv, on_empty)                                                          \
    if (((g_bits) & 0xffu) == 0u) { on_empty; (sp)--; const uint2 e = (stack)[(sp) * kBlock]; (g_base) = e.x; (g_bits) = e.y; } \
    const int bit = 31 - __clz((int)((g_bits) & 0xffu));                                                                         \
    (g_bits) ^= 1u << bit;                                                                                                       \
    const uint32_t child = (uint32_t)bit ^ (octinv);                                                                             \
    const uint32_t ni = (g_base) + (uint32_t)__popc(((g_bits) >> 8) & ((1u << child) - 1u));                                     \
    if ((g_bits) & 0xffu) { (stack)[(sp) * kBlock] = make_uint2((g_base), (g_bits)); (sp)++; }

// The boxes are padded for ray origins with |coordinate| <= w_guard (host/wide_bvh.cpp); other rays take the reference's walk
__device__ __forceinline__ bool wide_origin_ok(const DeviceScene& sc, f3 o) {
    return fmaxf(fabsf(o.x), fmaxf(fabsf(o.y), fabsf(o.z))) <= sc.w_guard;
}

// The closest-hit test of one fast-order record, the reference's arithmetic.  A triangle of wprims (v0, e1, e2): mt_hit.
__device__ __forceinline__ bool wide_tri_hit(const f3p& v0, const f3p& e1, const f3p& e2, const f3& o, const f3& d, float t_lo, float& t) {
    return mt_hit(mk3(v0.x, v0.y, v0.z), mk3(e1.x, e1.y, e1.z), mk3(e2.x, e2.y, e2.z), o, d, 1e-8f, t_lo, t);
}
// A record of wqprims (v0 | type, e1, e2, e3): a triangle the same way; a quad as Quad::intersect under an upper bound sees it
// - the smaller t of its two halves whenever that is below the bound (each half accepts t < closest, the second sees the
// first's result): quad.h:56-121
__device__ __forceinline__ bool wide_quad_hit(const float4& r0, const float4& r1, const float4& r2, const float4& r3, const f3& o, const f3& d,
                                              float t_lo, float& t) {
    if (__float_as_int(r0.w) != 0) {
        const float eps_up = __uint_as_float(__float_as_uint(1e-8f) + 1u);
        const float ta = mt_candidate(xyz(r0), xyz(r1), xyz(r2), o, d, eps_up, t_lo);
        const float tb = mt_candidate(xyz(r0), xyz(r2), xyz(r3), o, d, eps_up, t_lo);
        t = min_raw(ta, tb);
        return t < __builtin_inff();
    }
    return mt_hit(xyz(r0), xyz(r1), xyz(r2), o, d, 1e-8f, t_lo, t);
}
template <bool QUADS>
__device__ __forceinline__ bool wide_record_hit(const DeviceScene& sc, int k, f3 o, f3 d, float t_lo, float& t) {
    if (QUADS) {
        const float4* r = sc.wqprims + 4 * (size_t)k;
        return wide_quad_hit(r[0], r[1], r[2], r[3], o, d, t_lo, t);
    }
    const f3p* r = reinterpret_cast<const f3p*>(sc.wprims) + 3 * (size_t)k;
    return wide_tri_hit(r[0], r[1], r[2], o, d, t_lo, t);
}

struct WideCounts { unsigned int node_visits, prim_tests; };

// The closest hit through the fast tree for ONE ray, lane by lane (no phases): the walk of bounce_wide_body in straight-line
// form.  closest_t: the upper bound in, the hit's t out.  Among hits at equal t it keeps the smaller reference slot (wref_slot,
// the reference's rule: scene.h:89-90) and reports in tie that there was one at the final t.  Returns the fast-order record
// of the hit, -1 for none.  STATS: node visits and triangle tests into wc.
template <bool QUADS, bool STATS>
__device__ __forceinline__ int wide_closest_hit(const DeviceScene& sc, uint2* stack, f3 o, f3 d, float t_min, float& closest_t, bool& tie,
                                                WideCounts& wc) {
    f3 inv;
    uint32_t octinv, g_base, g_bits;
    WIDE_WALK_BEGIN(d, inv, octinv, g_base, g_bits);
    const float t_lo = mt_t_lo(t_min);
    int slot_hit = -1, sp = 0;
    tie = false;
    while (true) {
        WIDE_NEXT_NODE(ni, g_base, g_bits, sp, stack, octinv, if (sp == 0) break);
        const uint4* q = sc.wnodes + 8 * (size_t)ni;
        if (STATS) wc.node_visits++;
        const WideStep st = wide_node_test(q[0], q[1], q[2], q[3], q[4], q[5], q[6], o, inv, octinv, t_min, closest_t);
        for (uint32_t tris = st.tris; tris; tris &= tris - 1u) {
            const int k = (int)st.tri_base + __ffs((int)tris) - 1;
            if (STATS) wc.prim_tests++;
            float tt = 0.0f;
            if (!wide_record_hit<QUADS>(sc, k, o, d, t_lo, tt)) continue;
            if (tt < closest_t) { closest_t = tt; slot_hit = k; tie = false; }
            else if (tt == closest_t && slot_hit >= 0) {
                tie = true;
                if (sc.wref_slot[k] < sc.wref_slot[slot_hit]) slot_hit = k;
            }
        }
        g_base = st.child_base; g_bits = (st.imask << 8) | st.inner;
    }
    return slot_hit;
}

// ---- the proof of the certified walk --------------------------------------------------------------------
// A hit at Q = o + t d of triangle k is the reference's if the reference's walk reaches k's leaf: if the slab test of every
// box on the way from its root to that leaf passes.  Boxes are nested, so if Q lies inside the LEAF's box by eps on every face,
// it lies inside every ancestor's by at least as much - and eps = 2^-20 (|o_a| + M_a), M_a = max(|lo_a|, |hi_a|) of the box's
// own coordinates, is more than the reference's slab arithmetic can be off by on any box of the scene:
// t0' = fl(fl(lo - o) fl(1 / d)) is within 3 * 2^-24 |lo - o| / |d| of the true plane distance, Q_a' = fl(o_a + fl(t d_a))
// within 2 * 2^-24 (|o_a| + |t d_a|) of Q_a; a point inside the box has |Q_a| <= M_a and |t d_a| <= |o_a| + M_a, so the bounds
// sum to <= 11 * 2^-24 (|o_a| + M_a) < eps.  The margin carries to every ancestor: a face of an ancestor at X lies |X - F|
// beyond the leaf's face F, its own arithmetic error 2^-22 (|o_a| + |X|) <= 2^-22 (|o_a| + |F| + |X - F|) stays below
// eps + |X - F|.  Then every entry distance comes out <= t, every exit distance >= t, and the slab test passes whatever upper
// bound >= t the reference carries there.  (round 3 took eps from the scene's largest coordinate: one far-away primitive then
// sent every hit of the scene to the chain.)
// The bound needs 1 / d_a to be the reference's finite slope: |d_a| >= a caller's bound on every axis - 2^-60 (1 / d near
// overflow) for the path tracer's box_hit, 2^-26 for the solver's anyhit_box, which replaces |d_a| <= 1e-8 by 1e-8.  A
// smaller component, or Q within eps of a face, goes to the chain: the leaf's ancestors, leaf first, each box either holding
// Q with the margin - which settles every box above it - or passing the caller's own exact slab test.
constexpr float kCertEps = 9.5367431640625e-7f;        // 2^-20
constexpr float kCertSlope = 8.673617379884035e-19f;   // 2^-60: the path tracer's bound on |d_a|

// The one-fetch certificate: Q inside the leaf's box (wcert: lo, hi) by eps on all six faces
#define CERT_LEAF_INSIDE(o, q, lo, hi) ({                                                                                        \
    const float ex = kCertEps * (fabsf((o).x) + fmaxf(fabsf((lo).x), fabsf((hi).x))),                                            \
                ey = kCertEps * (fabsf((o).y) + fmaxf(fabsf((lo).y), fabsf((hi).y))),                                            \
                ez = kCertEps * (fabsf((o).z) + fmaxf(fabsf((lo).z), fabsf((hi).z)));                                            \
    (q).x - (lo).x >= ex && (hi).x - (q).x >= ex && (q).y - (lo).y >= ey && (hi).y - (q).y >= ey && (q).z - (lo).z >= ez && (hi).z - (q).z >= ez; })
// |d_a| >= bound on every axis
#define CERT_SLOPES_OK(d, bound) (fabsf((d).x) >= (bound) && fabsf((d).y) >= (bound) && fabsf((d).z) >= (bound))

// The leaf's ancestor list (wanc), from the leaf box's lo.w = first 4-node chunk << 5 | chunks (host: SceneState::buildFast).
// Never 0 chunks - the list starts with the leaf itself - and a 0 fails closed wherever it is read.
__device__ __forceinline__ uint32_t cert_first_chunk(float4 lo) { return __float_as_uint(lo.w) >> 5; }
__device__ __forceinline__ uint32_t cert_chunks(float4 lo) { return __float_as_uint(lo.w) & 31u; }

// One 4-node chunk of the chain, leaf first: declares bool proven (a box holds Q = o + t d with the margin, and |d_a| >=
// slope_bound) and bool failed (a box below the first such box fails `passes`, the caller's slab test: an expression of
// n0[c], n1[c]).  advance: the caller's cursor step, once the chunk's record is read.  0xffffffff pads a chunk and stands for
// the root.
#define CERT_CHUNK(proven, failed, sc, chunk, advance, o, d, t, slope_bound, passes)                                             \
    const uint4 idx = (sc).wanc[chunk];                                                                                          \
    advance;                                                                                                                     \
    const uint32_t ni[4] = {idx.x, idx.y, idx.z, idx.w};                                                                         \
    float4 n0[4], n1[4];                                                                                                         \
    _Pragma("unroll") for (int c = 0; c < 4; c++) {                                                                              \
        const uint32_t j = ni[c] == 0xffffffffu ? 0u : ni[c];                                                                    \
        n0[c] = (sc).nodes[2 * (size_t)j]; n1[c] = (sc).nodes[2 * (size_t)j + 1];                                                \
    }                                                                                                                            \
    const f3 q = (o) + (t) * (d);                                                                                                \
    const float slopes = min3_raw(fabsf((d).x), fabsf((d).y), fabsf((d).z)) - (slope_bound);                                     \
    bool proven = false, failed = false;                                                                                         \
    _Pragma("unroll") for (int c = 0; c < 4; c++) {                                                                              \
        const float ex = kCertEps * (fabsf((o).x) + fmaxf(fabsf(n0[c].x), fabsf(n1[c].x))),                                      \
                    ey = kCertEps * (fabsf((o).y) + fmaxf(fabsf(n0[c].y), fabsf(n1[c].y))),                                      \
                    ez = kCertEps * (fabsf((o).z) + fmaxf(fabsf(n0[c].z), fabsf(n1[c].z)));                                      \
        const float mx = min3_raw(q.x - n0[c].x - ex, n1[c].x - q.x - ex, slopes);                                               \
        const float my = min3_raw(q.y - n0[c].y - ey, n1[c].y - q.y - ey, q.z - n0[c].z - ez);                                   \
        const bool holds = min3_raw(mx, my, n1[c].z - q.z - ez) >= 0.0f;                                                         \
        const bool pass = (passes);                                                                                              \
        failed = failed || (!proven && !holds && !pass);                                                                         \
        proven = proven || holds;                                                                                                \
    }

// The chain for one hit at t of the triangle whose leaf box has lo, straight-line (bounce_wide_body takes it a chunk per wave
// iteration): true when a box holds Q or every box of the list passes; false - the reference's walk has to decide - when a box
// fails or the list is empty.  passes(n0, n1): the caller's slab test.
template <typename Passes>
__device__ __forceinline__ bool cert_chain(const DeviceScene& sc, float4 lo, f3 o, f3 d, float t, float slope_bound, Passes passes) {
    if (cert_chunks(lo) == 0u) return false;
    uint32_t chunk = cert_first_chunk(lo), left = cert_chunks(lo);
    while (left > 0u) {
        CERT_CHUNK(proven, failed, sc, chunk, (chunk++, left--), o, d, t, slope_bound, passes(n0[c], n1[c]));
        if (failed) return false;
        if (proven) return true;
    }
    return true;
}

}  // namespace ptmi
