// traversal.h — the walks of the render kernels, each defined once: the reference's walk in its three forms (STACK, LANE, SWEEP),
// the certified closest hit over the fast tree (csrc/wide_walk.h) and first_hit, the one-ray-at-a-time call of the Radiosity
// view, the feature pass and next-event estimation (first_hit.hip).  Everything is __forceinline__ into the calling kernel.
#pragma once
#include "pt_device.h"
#include "wide_walk.h"

namespace ptmi {

struct LaneCounters { unsigned int rays, node_visits, prim_tests, hits, top_visits, cert_chain, cert_fallback; };

// Slab test of scene.h:66-81 against [t_min, closest_t]; returns false when the reference would `continue`.
// `t0 > tmin_box ? t0 : tmin_box` is written fmaxf(t0, tmin_box): identical for every input because tmin_box /
// tmax_box are never NaN (a NaN t0/t1 - 0 * inf - is ignored by both forms) and the sign of a zero cannot reach the
// final comparison.  One v_max/v_min instead of v_cmp + v_cndmask (all of them half-rate VALU ops on gfx950).
__device__ __forceinline__ bool box_hit(const float4& n0, const float4& n1, f3 o, f3 inv, float t_min, float closest_t) {
    float t0x = (n0.x - o.x) * inv.x, t1x = (n1.x - o.x) * inv.x;
    if (inv.x < 0.0f) { const float tmp = t0x; t0x = t1x; t1x = tmp; }
    float t0y = (n0.y - o.y) * inv.y, t1y = (n1.y - o.y) * inv.y;
    if (inv.y < 0.0f) { const float tmp = t0y; t0y = t1y; t1y = tmp; }
    float t0z = (n0.z - o.z) * inv.z, t1z = (n1.z - o.z) * inv.z;
    if (inv.z < 0.0f) { const float tmp = t0z; t0z = t1z; t1z = tmp; }
    // max/min are associative and NaN-ignoring, so folding the three axes in one max3/min3 keeps the reference's result
    const float tmin_box = max3_raw(max_raw(t0x, t_min), t0y, t0z);
    const float tmax_box = min3_raw(min_raw(t1x, closest_t), t1y, t1z);
    return !(tmax_box < tmin_box);
}

// 1 / d of the slab tests (scene.h:57-59), per wave.  rcp_exact_normal is the IEEE quotient for 2^-100 <= |x| <= 2^100
// (tests/test_gpu_parity.py::test_fast_reciprocal_is_exact) and takes 5 instructions where the division takes 11, so ONE vote
// decides for the wave: if every live lane has all three components in that interval the wave takes the short form, otherwise -
// a zero, a -0, a denormal, an infinity or a NaN component in any live lane - the whole wave takes the division.  A ray direction
// is a unit vector, so only the lower bound ever acts; the upper one is tested on |x| + |y| + |z|, which is no smaller than any
// of the three and a NaN or inf when one of them is (v_min3 alone would ignore a NaN).  Lanes that are not live hold no ray.
__device__ __forceinline__ f3 ray_inv(f3 d, bool live) {
    float lo;
    asm("v_min3_f32 %0, |%1|, |%2|, |%3|" : "=v"(lo) : "v"(d.x), "v"(d.y), "v"(d.z));
    const float sum = fabsf(d.x) + fabsf(d.y) + fabsf(d.z);
    const bool in_range = (lo >= 0x1p-100f) & (sum <= 0x1p+100f);
    if (__any(live && !in_range)) return mk3(rcp_rn(d.x), rcp_rn(d.y), rcp_rn(d.z));
    return mk3(rcp_exact_normal(d.x), rcp_exact_normal(d.y), rcp_exact_normal(d.z));
}

// Primitive::intersect (primitive.h:83-90) + the closer-hit update of scene.h:89-96 for leaf slot k (per-lane k).
template <bool HAS_QUADS>
__device__ __forceinline__ void leaf_prim(const float4* __restrict__ prims, int prim_stride, int k, f3 o, f3 d, float t_lo,
                                          float& closest_t, int& slot_hit) {
    const float4 p0 = prims[k * prim_stride], p1 = prims[k * prim_stride + 1], p2 = prims[k * prim_stride + 2];
    const float eps = 1e-8f, eps_up = __uint_as_float(__float_as_uint(1e-8f) + 1u);
    float t;
    if (HAS_QUADS && __float_as_int(p0.w) != 0) {
        const float4 p3 = prims[k * prim_stride + 3];
        const float t1 = mt_candidate(xyz(p0), xyz(p1), xyz(p2), o, d, eps_up, t_lo);     // (v00, v10, v11)
        const float c1 = min_raw(t1, closest_t);
        const float t2 = mt_candidate(xyz(p0), xyz(p2), xyz(p3), o, d, eps_up, t_lo);     // (v00, v11, v01)
        t = min_raw(t2, c1);
    } else {
        float tt = 0.0f;
        const bool acc = mt_accept(xyz(p0), xyz(p1), xyz(p2), o, d, eps, t_lo, closest_t, tt);
        closest_t = acc ? tt : closest_t;
        slot_hit = acc ? k : slot_hit;
        return;
    }
    const bool closer = t < closest_t;
    closest_t = min_raw(t, closest_t);
    slot_hit = closer ? k : slot_hit;
}

// The same for the 36-byte triangle records of the packed layout (v0, e1, e2: three 12-byte loads)
__device__ __forceinline__ void leaf_prim_packed(const float* __restrict__ gprims, int k, f3 o, f3 d, float t_lo, float& closest_t, int& slot_hit) {
    const f3p* r = reinterpret_cast<const f3p*>(gprims) + 3 * (size_t)k;
    const f3p v0 = r[0], e1 = r[1], e2 = r[2];
    float tt = 0.0f;
    const bool acc = mt_accept(mk3(v0.x, v0.y, v0.z), mk3(e1.x, e1.y, e1.z), mk3(e2.x, e2.y, e2.z), o, d, 1e-8f, t_lo, closest_t, tt);
    closest_t = acc ? tt : closest_t;
    slot_hit = acc ? k : slot_hit;
}

// ---- TRAVERSAL_STACK: Scene::intersect_bvh_optimized (scene.h:50-110) with its explicit stack ------------------
// `stack` points at this lane's column of the LDS stack (entry e lives at stack[e * kBlock]).  The node about to be
// visited is kept in a register instead of being pushed and popped again; the reference's "drop both children when
// stack_ptr >= 62" rule (scene.h:101-105) is evaluated on the same stack_ptr value the reference would see.
template <bool HAS_QUADS, bool STATS>
__device__ __forceinline__ bool intersect_stack(const float4* __restrict__ nodes, const float4* __restrict__ prims, int prim_stride,
                                                int* stack, bool live, f3 o, f3 d, float t_min, float t_max,
                                                float& t_hit, int& slot_hit, LaneCounters& cn) {
    float closest_t = t_max;
    slot_hit = -1;
    const f3 inv = ray_inv(d, live);
    const float t_lo = mt_t_lo(t_min);
    int sp = 0;
    int cur = live ? 0 : -1;
    while (true) {
        if (cur < 0) {
            if (sp == 0) break;
            cur = stack[(--sp) * kBlock];
        }
        const float4 n0 = nodes[2 * cur], n1 = nodes[2 * cur + 1];
        if (STATS) cn.node_visits++;
        const int here = cur;
        cur = -1;
        if (!box_hit(n0, n1, o, inv, t_min, closest_t)) continue;
        const int a = __float_as_int(n0.w), b = __float_as_int(n1.w);
        if (b < 0) {                                       // leaf: -b primitives from slot a
            for (int i = 0; i < -b; i++) {
                if (STATS) cn.prim_tests++;
                leaf_prim<HAS_QUADS>(prims, prim_stride, a + i, o, d, t_lo, closest_t, slot_hit);
            }
        } else if (sp < 62) {                              // push right, visit left (= here + 1) next
            stack[(sp++) * kBlock] = b;
            cur = here + 1;
        }
    }
    t_hit = closest_t;
    return slot_hit >= 0;
}

// ---- TRAVERSAL_LANE: the same walk without a stack ---------------------------------------------------------------
// Pre-order numbering makes "pop" a table lookup: after a node whose box is missed the next node is its skip index,
// otherwise it is index + 1.  Valid while the reference's stack never overflows (tree depth <= 62).
template <bool HAS_QUADS, bool STATS>
__device__ __forceinline__ bool intersect_lane(const float4* __restrict__ nodes, const float4* __restrict__ prims, int prim_stride,
                                               int n_nodes, bool live, f3 o, f3 d, float t_min, float t_max,
                                               float& t_hit, int& slot_hit, LaneCounters& cn) {
    float closest_t = t_max;
    slot_hit = -1;
    const f3 inv = ray_inv(d, live);
    const float t_lo = mt_t_lo(t_min);
    int cur = live ? 0 : n_nodes;
    while (cur < n_nodes) {
        const float4 n0 = nodes[2 * cur], n1 = nodes[2 * cur + 1];
        if (STATS) cn.node_visits++;
        const int a = __float_as_int(n0.w), b = __float_as_int(n1.w);
        const bool pass = box_hit(n0, n1, o, inv, t_min, closest_t);
        int next = cur + 1;
        if (!pass && b >= 0) next = a;
        if (pass && b < 0) {
            for (int i = 0; i < -b; i++) {
                if (STATS) cn.prim_tests++;
                leaf_prim<HAS_QUADS>(prims, prim_stride, a + i, o, d, t_lo, closest_t, slot_hit);
            }
        }
        cur = next;
    }
    t_hit = closest_t;
    return slot_hit >= 0;
}

// ---- TRAVERSAL_SWEEP: the WAVE walks the node indices once -----------------------------------------------------
// Every lane's cursor only moves forward through the pre-order, so one pass n = 0..N-1 with "lanes whose cursor == n
// take part" visits, per lane, exactly the nodes and primitives of the walks above, in the same order.  n is
// wave-uniform: node and primitive records come in through scalar loads (s_load_dwordx4 -> SGPR operands), there is
// no stack, no per-lane LDS read, and lanes at different depths of the tree never serialise against each other.
// The wave pays for the UNION of its lanes' visits, so this is used only for scenes of a few dozen primitives.
// Must be called from wave-uniform control flow (dead lanes pass live = false).
template <bool HAS_QUADS>
__device__ __forceinline__ void leaf_prim_uniform(const float4* prims, int prim_stride, int k, f3 o, f3 d, float t_lo,
                                                  float& closest_t, int& slot_hit) {
    // k is wave-uniform: these are broadcast LDS reads, the operands land in VGPRs (an SGPR operand would halve
    // the issue rate of every multiply/subtract that uses it)
    const float4 p0 = prims[k * prim_stride], p1 = prims[k * prim_stride + 1], p2 = prims[k * prim_stride + 2];
    const float eps = 1e-8f, eps_up = __uint_as_float(__float_as_uint(1e-8f) + 1u);
    float t;
    if (HAS_QUADS && __builtin_amdgcn_readfirstlane(__float_as_int(p0.w)) != 0) {   // wave-uniform branch
        const float4 p3 = prims[k * prim_stride + 3];
        // Quad::intersect: closest = t_max (= closest_t); each half accepts t < closest, second half sees the first's result
        const float t1 = mt_candidate(xyz(p0), xyz(p1), xyz(p2), o, d, eps_up, t_lo);     // (v00, v10, v11), |a| > eps
        const float c1 = min_raw(t1, closest_t);
        const float t2 = mt_candidate(xyz(p0), xyz(p2), xyz(p3), o, d, eps_up, t_lo);     // (v00, v11, v01)
        t = min_raw(t2, c1);                        // == closest_t when neither half was accepted
    } else {
        float tt = 0.0f;                                                                  // !(|a| < eps)
        const bool acc = mt_accept(xyz(p0), xyz(p1), xyz(p2), o, d, eps, t_lo, closest_t, tt);
        closest_t = acc ? tt : closest_t;
        slot_hit = acc ? k : slot_hit;
        return;
    }
    const bool closer = t < closest_t;            // quad: hit && temp.t < closest_t (scene.h:89-90)
    closest_t = min_raw(t, closest_t);
    slot_hit = closer ? k : slot_hit;
}

template <bool HAS_QUADS, bool STATS>
__device__ __forceinline__ bool intersect_sweep(const float4* nodes, const float4* prims, int prim_stride,
                                                int n_nodes, bool live, f3 o, f3 d, float t_min, float t_max,
                                                float& t_hit, int& slot_hit, LaneCounters& cn) {
    float closest_t = t_max;
    slot_hit = -1;
    const f3 inv = ray_inv(d, live);
    const float t_lo = mt_t_lo(t_min);
    int cur = live ? 0 : n_nodes;
    for (int n = 0; n < n_nodes; n++) {
        if (cur == n) {
            // readfirstlane pins the index to an SGPR: inside this branch the optimiser knows cur == n and would
            // otherwise address the node through the per-lane cursor
            const int nu = __builtin_amdgcn_readfirstlane(n);
            const float4 n0 = nodes[2 * nu], n1 = nodes[2 * nu + 1];
            if (STATS) cn.node_visits++;
            const int a = __builtin_amdgcn_readfirstlane(__float_as_int(n0.w));
            const int b = __builtin_amdgcn_readfirstlane(__float_as_int(n1.w));   // wave-uniform
            const bool pass = box_hit(n0, n1, o, inv, t_min, closest_t);
            cur = n + 1;
            if (b < 0) {
                if (pass) {
                    for (int i = 0; i < -b; i++) {
                        if (STATS) cn.prim_tests++;
                        leaf_prim_uniform<HAS_QUADS>(prims, prim_stride, a + i, o, d, t_lo, closest_t, slot_hit);
                    }
                }
            } else if (!pass) cur = a;
        }
    }
    t_hit = closest_t;
    return slot_hit >= 0;
}

template <int MODE, bool HAS_QUADS, bool STATS>
__device__ __forceinline__ bool scene_intersect(const float4* __restrict__ nodes, const float4* __restrict__ prims, int prim_stride,
                                                int n_nodes, int* stack, bool live, f3 o, f3 d, float t_min, float t_max,
                                                float& t_hit, int& slot_hit, LaneCounters& cn) {
    if (MODE == TRAVERSAL_SWEEP) return intersect_sweep<HAS_QUADS, STATS>(nodes, prims, prim_stride, n_nodes, live, o, d, t_min, t_max, t_hit, slot_hit, cn);
    if (MODE == TRAVERSAL_LANE) return intersect_lane<HAS_QUADS, STATS>(nodes, prims, prim_stride, n_nodes, live, o, d, t_min, t_max, t_hit, slot_hit, cn);
    return intersect_stack<HAS_QUADS, STATS>(nodes, prims, prim_stride, stack, live, o, d, t_min, t_max, t_hit, slot_hit, cn);
}

// The certified closest hit of ONE ray, lane by lane (no phases): the walk and the proof of bounce_wide_body<..., CERT> in
// straight-line form (csrc/wide_walk.h), for callers that trace a ray at a time (the Radiosity view, the feature pass).  Returns
// the REFERENCE's hit: its leaf-order slot in ref_slot, so that the caller indexes the reference's per-primitive arrays.
// stack: this lane's column of w_depth 8-byte entries in LDS (entry e at stack[e * kBlock]).
template <bool QUADS>
__device__ __forceinline__ bool certified_closest_hit(const DeviceScene& sc, uint2* stack, f3 o, f3 d, float t_min, float& t_hit, int& ref_slot) {
    LaneCounters cn = {0, 0, 0, 0, 0, 0, 0};
    auto reference_walk = [&]() { return intersect_lane<QUADS, false>(sc.nodes, sc.prims, sc.prim_stride, sc.n_nodes, true, o, d, t_min, FLT_MAX, t_hit, ref_slot, cn); };
    if (!wide_origin_ok(sc, o)) return reference_walk();
    float closest_t = FLT_MAX;
    bool tie = false;
    WideCounts wc = {0, 0};
    const int slot_hit = wide_closest_hit<QUADS, false>(sc, stack, o, d, t_min, closest_t, tie, wc);
    if (slot_hit < 0) return false;                        // the reference can only accept triangles this walk would have found
    if (tie) return reference_walk();                      // the reference keeps the hit it visits first: let it decide
    const float4 lo = sc.wcert[kWideCertStride * (size_t)slot_hit], hi = sc.wcert[kWideCertStride * (size_t)slot_hit + 1];
    const f3 q = o + closest_t * d;
    const f3 rinv = mk3(rcp_rn(d.x), rcp_rn(d.y), rcp_rn(d.z));            // the reference's 1 / d for its slab tests
    const bool proven = (CERT_LEAF_INSIDE(o, q, lo, hi) && CERT_SLOPES_OK(d, kCertSlope)) ||
                        cert_chain(sc, lo, o, d, closest_t, kCertSlope, [=](const float4& n0, const float4& n1) { return box_hit(n0, n1, o, rinv, t_min, closest_t); });
    if (!proven) return reference_walk();
    t_hit = closest_t;
    ref_slot = sc.wref_slot[slot_hit];
    return true;
}

// The closest hit of ONE ray for callers that trace a ray at a time.  MODE TRAVERSAL_CERTIFIED: the certified walk (a dead lane
// traces nothing); TRAVERSAL_LANE / TRAVERSAL_STACK: the reference's walk.  k is the reference's leaf-order slot either way.
// smem: the kernel's dynamic LDS - this lane's column of w_depth 8-byte entries (certified) or of the reference's int stack
// (STACK; unused by LANE).  The only place that knows which of the two views a walk takes.
template <int MODE, bool HAS_QUADS>
__device__ __forceinline__ bool first_hit(const DeviceScene& sc, float4* smem, bool live, f3 o, f3 d, float t_min, float& t, int& k, LaneCounters& cn) {
    bool hit;
    if constexpr (MODE == TRAVERSAL_CERTIFIED) hit = live && certified_closest_hit<HAS_QUADS>(sc, reinterpret_cast<uint2*>(smem) + threadIdx.x, o, d, t_min, t, k);
    else hit = scene_intersect<MODE, HAS_QUADS, false>(sc.nodes, sc.prims, sc.prim_stride, sc.n_nodes, reinterpret_cast<int*>(smem) + threadIdx.x, live, o, d, t_min, FLT_MAX, t, k, cn);
    return hit;
}

}  // namespace ptmi
