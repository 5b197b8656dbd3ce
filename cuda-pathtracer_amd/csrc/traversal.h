// traversal.h — the walks of the render kernels, each defined once: the reference's walk in its three forms (STACK, LANE, SWEEP),
// the certified closest hit over the fast tree (csrc/wide_walk.h) and first_hit, the one-ray-at-a-time call of the Radiosity
// view and next-event estimation (first_hit.hip) and the feature pass (features.hip).  Everything is __forceinline__ into the calling kernel.
#pragma once
#include "pt_device.h"
#include "sweep_records.h"
#include "sweep_near_far.h"
#include "sweep_leaves.h"
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

// box_hit over a near/far node record (sweep_near_far.h): bx = (near, far) along x as this lane read it, at the offset its
// inv.x < 0.0f chose - (lo, hi), or (hi, lo) where box_hit would have swapped the two products.  The plane the swap would have
// put into a place is the one read into it, by the same predicate, so t0* and t1* have box_hit's bits for every input (a +-0,
// denormal or non-finite inv included) and the two folds are box_hit's own.
__device__ __forceinline__ bool box_hit_near_far(float2 bx, float2 by, float2 bz, f3 o, f3 inv, float t_min, float closest_t) {
    const float t0x = (bx.x - o.x) * inv.x, t1x = (bx.y - o.x) * inv.x;
    const float t0y = (by.x - o.y) * inv.y, t1y = (by.y - o.y) * inv.y;
    const float t0z = (bz.x - o.z) * inv.z, t1z = (bz.y - o.z) * inv.z;
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
__device__ __forceinline__ bool ray_inv_long(f3 d, bool live) {       // the vote: true when the wave takes the division
    float lo;
    asm("v_min3_f32 %0, |%1|, |%2|, |%3|" : "=v"(lo) : "v"(d.x), "v"(d.y), "v"(d.z));
    const float sum = fabsf(d.x) + fabsf(d.y) + fabsf(d.z);
    const bool in_range = (lo >= 0x1p-100f) & (sum <= 0x1p+100f);
    return __any(live && !in_range);
}
__device__ __forceinline__ f3 ray_inv_of(f3 d, bool long_form) {
    if (long_form) return mk3(rcp_rn(d.x), rcp_rn(d.y), rcp_rn(d.z));
    return mk3(rcp_exact_normal(d.x), rcp_exact_normal(d.y), rcp_exact_normal(d.z));
}
__device__ __forceinline__ f3 ray_inv(f3 d, bool live) { return ray_inv_of(d, ray_inv_long(d, live)); }

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

// ---- TRAVERSAL_SWEEP: the WAVE walks the node records once -------------------------------------------------------
// Every lane's cursor only moves forward through the pre-order, so one pass over the records with "lanes whose cursor stands at
// this record take part" visits, per lane, exactly the nodes and primitives of the walks above, in the same order.  The pass is
// wave-uniform: node and primitive records are broadcast LDS reads, there is no stack, and lanes at different depths of the tree
// never serialise against each other.  The wave pays for the UNION of its lanes' visits, so this is used only for scenes of a
// few dozen primitives.  Must be called from wave-uniform control flow (dead lanes pass live = false).
//
// The walk reads the sweep's own records (sweep_records.h, sweep_near_far.h; staged by stage_scene<true, true, form>) and keeps no books beside them.
// In every instantiation the cursor is the LDS ADDRESS of a node record and is itself the address of the two reads (an address
// that all active lanes share is a broadcast read; it stays a per-lane VGPR, pinned, or the optimiser would rebuild it from the
// scalar trip address with a move per pass).  "Stands at this record" is a compare against the scalar address, "next" is + the record's size, a
// miss at an interior node is one select of the record's skip lane, which staging has turned into an address.  The trip count is
// scalar and bounded by n_nodes, whatever a cursor holds.  Only the leaf flag / count and the leaf's first slot go through
// readfirstlane (scalar branch, scalar loop bound, scalar address arithmetic).  The primitive stride is a constant of the
// instantiation: 3 float4 without quads, 4 with (SceneState::chooseTraversal refuses any other).
// Five more items, each taken by the instantiations it costs no wave per SIMD and no spill (sweep_form below):
//   SWEEP_ONE_SELECT    the cursor's update is one select ahead of the leaf branch; without it, inside the two branches;
//   SWEEP_VOTED_UPDATE  closest_t and slot_hit change only behind the (a, u) vote (mt_accept_update below); without it
//                       mt_accept / mt_candidate and the selects after them, as leaf_prim has them.  Either way the slot comes
//                       from the record's slot lane, a VGPR already;
//   SWEEP_PINNED        eps, nextafter(eps) and t_lo are pinned in VGPRs: as SGPR operands of a VOP3 they cost it its full rate;
//   SWEEP_LEAF_BASE     a leaf's primitives are read at immediate offsets from one VGPR that holds the address of the leaf's
//                       first record, kSweepLeafUnroll per trip of a loop whose bound is the record's count; without it one
//                       address per primitive, from the scalar one.
//   SWEEP_NEAR_FAR      the node records are the 64-byte near/far records of sweep_near_far.h and the cursor strides by 64: each
//                       lane reads (near, far) of an axis - 8 bytes - at the record's address + the axis group + 8 where its
//                       1 / d is negative, three offsets fixed per ray and pinned in VGPRs, and the two w lanes from a fourth
//                       pair; box_hit_near_far has no swap.  Per pass three v_add_u32 and four ds_read_b64 (the lanes of one
//                       read use at most two addresses, 8 bytes apart) for six v_cndmask by SGPR lane masks and two
//                       ds_read_b128.  The predicate that chose the read is box_hit's own, so the plane box_hit would have
//                       swapped into a place after the multiplication is the one read into it before: t0* and t1* keep their
//                       bits for every input, a +-0, denormal or non-finite 1 / d included.
// Two more, taken by the builds that take SWEEP_NEAR_FAR, replace a select (half rate) by a move (full rate) under a narrowed EXEC:
//   SWEEP_MASKED_HIT    mt_accept_update writes closest_t and slot_hit in a branch on the accept mask, (m >= 0) & (t < closest_t)
//                       as before: s_and_saveexec, two v_mov_b32, s_or exec for two v_cndmask.  A lane that does not accept is
//                       not written at all, where the select copied its value into itself;
//   SWEEP_MASKED_CURSOR every lane of a node pass takes here + 64, then the lanes that miss an interior node take the skip
//                       address in a branch on (b >= 0) & !pass: one v_mov_b32 for the v_cndmask by an SGPR mask.
//                       The leaf branch keeps its place and its mask.
// An empty asm volatile in each branch keeps it a branch (the optimiser would make the selects again); the compiler leaves an
// s_cbranch_execz in front of such a block, taken when no lane of the pass accepts / misses.
// No expression of the slab test or of Moller-Trumbore differs from the walks above, and none is reordered.
//
// VALU instructions per pass in ptmi_bounce<SWEEP, ..., triangles, timed build> (ISA, before -> after): interior node 31 -> 27,
// Moller-Trumbore first half 34 + 3 after it -> 32, second half 28 -> 30 (it holds the two selects now), per leaf 3 -> 2; the
// quad build's node pass 31 -> 28, its primitive passes as before.  MI355X, parent's library against this one, three runs each,
// alternating: c2 7 667 -> 8 046 Msamples/s (+4.9 %, 35.01 -> 33.36 ms per step), c3 15 935 -> 16 417 (+3.0 %); the parent's
// runs lie within 0.3 % of each other.  With SWEEP_NEAR_FAR on top of that, the timed triangle build's interior node pass 27 -> 24,
// none of the slab test's with an SGPR mask, the same protocol: c2 8 248 -> 8 393 Msamples/s (+1.75 %, 32.55 -> 31.98 ms per step),
// every run above every run of the parent, whose runs lie within 0.45 % of each other; c4 9 454 -> 9 702 (+2.6 %, one pair); 52
// fewer VALU wave-instructions per wave-segment, 37 more LDS instructions, the LDS's busy cycles unchanged, its bank conflicts
// up 0.3 - 0.4 % (16.9 -> 17.0 cycles per wave-segment), a little beyond the parent's run-to-run difference of 0.24 %.
// With the two masked moves on top of that the counts per pass stay - interior node 24 VALU, one of them the cursor's v_mov_b32
// where the v_cndmask was; second half 30, two v_mov_b32 where its two v_cndmask were - and each masked block adds
// s_and_saveexec, s_cbranch_execz and s_or exec; 61 -> 60 VGPRs and, BATCH, 62 -> 61.  The same protocol: c2 8 321 -> 8 437
// Msamples/s (+1.4 %, 32.26 -> 31.82 ms per step), every run above every run of the parent, whose runs lie within 0.19 % of each
// other; each move alone, two runs: the hit's 8 379 and 8 445, the cursor's 8 386 and 8 403; c4 9 751 -> 9 873 (+1.2 %, one pair).
// A third item, keeping s = o - v0 from one triangle test to the next where two records of a leaf share v0, is not built: in
// cbox.obj 2 of 32 records follow a record with the same v0 in their leaf (tests/test_sweep_shared_s_host.py).
//
// SWEEP_LEAVES, taken by the builds that take SWEEP_NEAR_FAR: the wave slab-tests the LEAVES alone.  closest_t and slot_hit change
// only inside leaves, and which leaves a lane enters is decided by the leaf's own slab test, so the interior tests are work the
// result does not need - where the claim below holds.  One wave-uniform decision per segment: ray_inv's vote and the scene's leaf
// count (DeviceScene::sweep_leaves, 0 where the host's verdict on the node array is false).  Hot side: sweep_leaves_walk over the
// leaf image (sweep_leaves.h), one pass per leaf with all live lanes.  Cold side - a vote that fails, a scene without a verdict,
// every STATS build (node_visits are the reference's) - the walk above, unchanged.
//   CLAIM.  For a ray that takes ray_inv's short form, every leaf whose slab test passes has only ancestors whose slab tests
//   passed when the reference's walk (scene.h:50-110, restated in intersect_lane) visited them.  Hence the leaf-only walk enters
//   exactly the leaves the reference enters, in pre-order, with the same closest_t (induction over the leaves: closest_t changes
//   only in entered leaves), and every t and slot is the reference's, bit for bit.
//   1. Containment, as bits.  Every node's six planes bound its children's, lo_parent <= lo_child and hi_parent >= hi_child per
//      axis, and all planes are finite.  host/bvh.cpp: computeBounds gives that by construction (an exact fminf / fmaxf over a
//      superset of padded primitive boxes), but the walk does not rely on it: ptmi_sweep_leaves_verdict checks every child against
//      its parent, and the links, on the very array the kernels read, once per scene load (host/scene_state.cpp).
//   2. No NaN is born in the slab arithmetic.  The vote gives every live lane 2^-100 <= |d.a| <= 2^100 per component, so 1 / d is
//      a finite non-zero normal number and (plane - o) * inv is never 0 * inf (plane - o may overflow to +-inf: still ordered).
//      The vote does not look at o: a NaN component of o makes the two products of that axis NaN for every box, which max / min
//      ignore alike; an infinite one makes plane - o the same -+inf for every finite plane, so the two products of that axis
//      are the same +-inf for ancestor and leaf.  Either way ancestor and leaf decide alike on that axis.
//   3. Monotonicity.  Rounded subtraction of a fixed o, rounded multiplication by a fixed non-zero factor, max / max3 / min / min3
//      and flush-to-zero are monotone in numeric order (-0 and +0 count as equal: the final comparison cannot tell them apart),
//      and which plane is near is chosen by inv < 0 alone, identically for ancestor and leaf.  So tmin_box(ancestor) <=
//      tmin_box(leaf); closest_t never grows and the ancestor is visited earlier, so tmax_box(ancestor) >= tmax_box(leaf);
//      !(tmax < tmin) at the leaf implies the same at every ancestor.
//   4. Tree depth <= 62, the reference's stack rule, which the sweep and LANE assume already (SceneState::chooseTraversal).
// A leaf pass is 19 VALU (six v_sub, six v_mul, v_max, v_min, v_max3, v_min3, v_cmp and the two v_readfirstlane of the link pair;
// + 1 v_mov of the leaf's record address under the passing lanes) against 24 of a node pass: no cursor compare, no v_add_u32 of
// the three addresses (kSweepLeavesUnroll records per trip at immediate offsets), no skip move, and `pass & live` is an s_and.
// cbox.obj: 11 leaf passes per wave-segment against 17.2 node passes of 21 (tools/sweep_union_sim.py; cbox_quads.obj 7 against
// 10.8, the 64-triangle soup of tests/test_gpu_sweep_passes.py 24 against 30.7), so every scene with a verdict takes it.
// EXPERIMENTS.md has the runs and the counters.
enum : int { SWEEP_VOTED_UPDATE = 1, SWEEP_PINNED = 2, SWEEP_LEAF_BASE = 4, SWEEP_ONE_SELECT = 8, SWEEP_NEAR_FAR = 16, SWEEP_MASKED_HIT = 32, SWEEP_MASKED_CURSOR = 64,
              SWEEP_LEAVES = 128 };
constexpr int kSweepLeafUnroll = 4;
// leaf records per trip of sweep_leaves_walk, read at immediate offsets from the lane's three addresses (-DPTMI_SWEEP_LEAVES_UNROLL=1, 2 or 4)
#ifndef PTMI_SWEEP_LEAVES_UNROLL
#define PTMI_SWEEP_LEAVES_UNROLL 2
#endif
constexpr int kSweepLeavesUnroll = PTMI_SWEEP_LEAVES_UNROLL;

// experiment libraries (make ab-lib DEFS="-DPTMI_SWEEP_MASKED_HIT=0 -DPTMI_SWEEP_MASKED_CURSOR=0"): the builds that take
// SWEEP_NEAR_FAR without one or both of the masked moves.  Here and not beside bounce_sync.hip's switches: the intersect hook
// (debug_hooks.hip) takes the timed build's form from sweep_form too.
#ifndef PTMI_SWEEP_MASKED_HIT
#define PTMI_SWEEP_MASKED_HIT 1
#endif
#ifndef PTMI_SWEEP_MASKED_CURSOR
#define PTMI_SWEEP_MASKED_CURSOR 1
#endif
// -DPTMI_SWEEP_LEAVES=0: the builds that take SWEEP_NEAR_FAR without the leaf-only walk; they walk as the parent's do
#ifndef PTMI_SWEEP_LEAVES
#define PTMI_SWEEP_LEAVES 1
#endif

// The form of each instantiation, judged by registers, waves per SIMD and spills against the walk before these items (DESIGN.md
// 5 has the table).  The triangle builds take all four: 55-60 -> 59-64 VGPRs, 8 waves per SIMD and no spill as before (the
// GUIDED ones stay at their cap of 80).  The quad builds stand at 63-64 VGPRs with two Moller-Trumbore halves per record: with
// any one of the four the BATCH build starts to spill (2-9 VGPRs) and the plain one loses a wave or spills, so they keep
// leaf_prim's form on the new cursor, which leaves both without spills at 8 waves (63 and 64 VGPRs).
// SWEEP_NEAR_FAR holds three more VGPRs through the walk.  The triangle builds without STATS and GUIDED have them: 58 -> 61 and,
// BATCH, 59 -> 62, 8 waves, no scratch.  With STATS the plain build would go 64 -> 67 and lose a wave and the BATCH one spill 12
// bytes; the quad builds (64 VGPRs) spill 8-12 bytes, and with the three offsets packed into one VGPR they keep 64 / 8 / 0 but
// c3 ran 1.8 % slower (EXPERIMENTS.md); the GUIDED builds stand at their cap.  Those keep the two-vector records.
// SWEEP_MASKED_HIT and SWEEP_MASKED_CURSOR go to the builds that take SWEEP_NEAR_FAR, which give a VGPR back with them (61 -> 60,
// BATCH 62 -> 61); every other build is the code it was, byte for byte.
// SWEEP_LEAVES goes to the same builds: both walks stand in the kernel, 60 -> 62 VGPRs and, BATCH, 61 -> 63, 8 waves, no scratch.
// The quad builds were compiled with it (the leaf image beside their two-vector nodes): 64 VGPRs at 8 waves with 8 bytes of scratch
// and, BATCH, 12, where they had none - new scratch, so by the standing rule they keep their walk, byte for byte.
template <bool HAS_QUADS, bool STATS, bool GUIDED>
constexpr int sweep_form() {
    constexpr int timed = SWEEP_NEAR_FAR | (PTMI_SWEEP_MASKED_HIT ? SWEEP_MASKED_HIT : 0) | (PTMI_SWEEP_MASKED_CURSOR ? SWEEP_MASKED_CURSOR : 0) |
                          (PTMI_SWEEP_LEAVES ? SWEEP_LEAVES : 0);
    return HAS_QUADS ? 0 : ((SWEEP_ONE_SELECT | SWEEP_VOTED_UPDATE | SWEEP_PINNED | SWEEP_LEAF_BASE) | (!STATS && !GUIDED ? timed : 0));
}
// 16-byte vectors per node record in the LDS image of a form (stage_scene lays them out, the walk strides by them)
constexpr int sweep_node_vecs(int form) { return (form & SWEEP_NEAR_FAR) ? PTMI_SWEEP_NF_NODE_VECS : 2; }

// mt_accept (pt_device.h) in the sweep's form: the same arithmetic with the closer-hit update of scene.h:89-96 behind the vote,
// so that a primitive whose (a, u) test rejects the whole wave costs no select at all and t needs no initial value.  `slot` arrives in a
// VGPR (the record's slot lane).  A quad half is the same call with eps_for_a = nextafter(eps): mt_candidate's +inf, the min chain
// and `t < closest_t` of leaf_prim select exactly as (m >= 0) & (t < closest_t) does half by half - min_raw(+inf or a NaN t,
// closest_t) is closest_t, a half updates iff its t is below the closest so far, and the second half sees the first's result.
template <bool MASKED = false>
__device__ __forceinline__ void mt_accept_update(f3 v0, f3 edge1, f3 edge2, f3 o, f3 d, float eps_for_a, float t_lo, int slot,
                                                 float& closest_t, int& slot_hit) {
    const f3 h = cross(d, edge2);
    const float a = dot(edge1, h);
    const float f = rcp_exact_normal(a);
    const f3 s = o - v0;
    const float u = f * dot(s, h);
    const float m1 = min3_raw(fabsf(a) - eps_for_a, u, 1.0f - u);
    if (!__any(m1 >= 0.0f)) return;
    const f3 q = cross(s, edge1);
    const float v = f * dot(d, q);
    const float t = f * dot(edge2, q);
    float m = min3_raw(m1, v, 1.0f - (u + v));
    m = min_raw(m, t - t_lo);
    const bool acc = (m >= 0.0f) & (t < closest_t);
    if constexpr (MASKED) {
        if (acc) {                                     // the accepting lanes alone: EXEC narrowed around two moves
            closest_t = t;
            slot_hit = slot;
            asm volatile("" : "+v"(closest_t), "+v"(slot_hit));      // or the optimiser turns the branch back into two selects
        }
    } else {
        closest_t = acc ? t : closest_t;
        slot_hit = acc ? slot : slot_hit;
    }
}
// LDS by address: the 32-bit address of p, and the i-th float4 from such an address (the host pass only parses them)
__device__ __forceinline__ unsigned int lds_address(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (unsigned int)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
#else
    return 0u;
#endif
}
__device__ __forceinline__ float4 lds_vec(unsigned int address, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float vec4 __attribute__((ext_vector_type(4)));
    const vec4 v = reinterpret_cast<const __attribute__((address_space(3))) vec4*>(address)[i];
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#endif
}
// the i-th pair of floats (8 bytes) from such an address
__device__ __forceinline__ float2 lds_pair(unsigned int address, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float vec2 __attribute__((ext_vector_type(2)));
    const vec2 v = reinterpret_cast<const __attribute__((address_space(3))) vec2*>(address)[i];
    return make_float2(v.x, v.y);
#else
    return make_float2(0.0f, 0.0f);
#endif
}

template <bool HAS_QUADS, int FORM>
__device__ __forceinline__ void leaf_prim_sweep(unsigned int rec, int at, f3 o, f3 d, float eps, float eps_up, float t_lo,
                                                float& closest_t, int& slot_hit) {
    const float4 p0 = lds_vec(rec, at), p1 = lds_vec(rec, at + 1), p2 = lds_vec(rec, at + 2);   // record at vector `at` from rec
    const int slot = __float_as_int(p1.w);                                                // the slot lane (sweep_records.h)
    constexpr bool VOTED = (FORM & SWEEP_VOTED_UPDATE) != 0;
    if (HAS_QUADS && __builtin_amdgcn_readfirstlane(__float_as_int(p0.w)) != 0) {         // wave-uniform branch
        const float4 p3 = lds_vec(rec, at + 3);
        // Quad::intersect: each half accepts t < closest, the second half sees the first's result; |a| > eps
        if (VOTED) {
            mt_accept_update(xyz(p0), xyz(p1), xyz(p2), o, d, eps_up, t_lo, slot, closest_t, slot_hit);     // (v00, v10, v11)
            mt_accept_update(xyz(p0), xyz(p2), xyz(p3), o, d, eps_up, t_lo, slot, closest_t, slot_hit);     // (v00, v11, v01)
        } else {
            const float t1 = mt_candidate(xyz(p0), xyz(p1), xyz(p2), o, d, eps_up, t_lo);
            const float c1 = min_raw(t1, closest_t);
            const float t2 = mt_candidate(xyz(p0), xyz(p2), xyz(p3), o, d, eps_up, t_lo);
            const float t = min_raw(t2, c1);                        // == closest_t when neither half was accepted
            const bool closer = t < closest_t;                      // quad: hit && temp.t < closest_t (scene.h:89-90)
            closest_t = min_raw(t, closest_t);
            slot_hit = closer ? slot : slot_hit;
        }
    } else if (VOTED) {
        mt_accept_update<(FORM & SWEEP_MASKED_HIT) != 0>(xyz(p0), xyz(p1), xyz(p2), o, d, eps, t_lo, slot, closest_t, slot_hit);            // !(|a| < eps)
    } else {
        float tt = 0.0f;
        const bool acc = mt_accept(xyz(p0), xyz(p1), xyz(p2), o, d, eps, t_lo, closest_t, tt);
        closest_t = acc ? tt : closest_t;
        slot_hit = acc ? slot : slot_hit;
    }
}

// The leaf image a kernel staged (sweep_leaves.h; stage_scene hands it out): the LDS address of the first leaf record and their
// number.  n == 0: there is none - the scene's verdict is false, or the build does not take SWEEP_LEAVES - and every wave walks
// every node.
struct SweepLeaves { unsigned int at = 0; int n = 0; };

// SWEEP_LEAVES, the hot side: the wave slab-tests the n leaf records in pre-order with all its live lanes and runs each leaf's
// primitives under the lanes that pass - no cursor, no skip select, no compare of a cursor with the trip.  The three addresses are
// fixed per ray (the image's address + where (near, far) stands for the sign of 1 / d, pinned); kSweepLeavesUnroll records per
// trip are read at immediate offsets from them, the link pair at the x address + 48 (it stands twice, so both x offsets read it).
// Triangles only, no STATS (sweep_form).  inv must be ray_inv's short form for every live lane: the proof above rests on it.
template <int FORM>
__device__ __forceinline__ void sweep_leaves_walk(SweepLeaves leaves, bool live, f3 o, f3 d, f3 inv, float t_min, float eps, float t_lo,
                                                  float& closest_t, int& slot_hit) {
    constexpr unsigned int kPrimBytes = 3 * PTMI_SWEEP_VEC_BYTES;
    unsigned int ax = leaves.at + (inv.x < 0.0f ? PTMI_SWEEP_NF_FAR_FIRST : 0);      // box_hit's own predicates
    unsigned int ay = leaves.at + (inv.y < 0.0f ? PTMI_SWEEP_NF_FAR_FIRST : 0);
    unsigned int az = leaves.at + (inv.z < 0.0f ? PTMI_SWEEP_NF_FAR_FIRST : 0);
    asm("" : "+v"(ax));
    asm("" : "+v"(ay));
    asm("" : "+v"(az));
    const auto leaf = [&](int j) {                                // record j of this trip
        constexpr int kPairs = PTMI_SWEEP_LEAF_BYTES / 8;
        const float2 bx = lds_pair(ax, kPairs * j), by = lds_pair(ay, kPairs * j + 2), bz = lds_pair(az, kPairs * j + 4);
        const float2 w = lds_pair(ax, kPairs * j + PTMI_SWEEP_LEAF_LINK / 8);
        const unsigned int first = (unsigned int)__builtin_amdgcn_readfirstlane(__float_as_int(w.x));
        const int count = __builtin_amdgcn_readfirstlane(__float_as_int(w.y));
        const bool pass = box_hit_near_far(bx, by, bz, o, inv, t_min, closest_t) & live;
        if (pass) {
            unsigned int rec = first;
            asm("" : "+v"(rec));
            const auto test = [&](int i) { leaf_prim_sweep<false, FORM>(rec, i * 3, o, d, eps, eps, t_lo, closest_t, slot_hit); };
            static_assert(kSweepLeafUnroll == 4, "the four calls below");
            for (int left = count; left > 0; left -= kSweepLeafUnroll, rec += kSweepLeafUnroll * kPrimBytes) {
                test(0);
                if (left > 1) test(1);
                if (left > 2) test(2);
                if (left > 3) test(3);
            }
        }
    };
    static_assert(kSweepLeavesUnroll == 1 || kSweepLeavesUnroll == 2 || kSweepLeavesUnroll == 4, "the calls below");
    constexpr unsigned int kTripBytes = kSweepLeavesUnroll * PTMI_SWEEP_LEAF_BYTES;
    for (int left = leaves.n; left > 0; left -= kSweepLeavesUnroll, ax += kTripBytes, ay += kTripBytes, az += kTripBytes) {
        leaf(0);
        if constexpr (kSweepLeavesUnroll > 1) { if (left > 1) leaf(1); }
        if constexpr (kSweepLeavesUnroll > 2) {
            if (left > 2) leaf(2);
            if (left > 3) leaf(3);
        }
    }
}

template <bool HAS_QUADS, bool STATS, int FORM>
__device__ __forceinline__ bool intersect_sweep(const float4* nodes, const float4* prims, int n_nodes, bool live, f3 o, f3 d,
                                                float t_min, float t_max, float& t_hit, int& slot_hit, LaneCounters& cn,
                                                SweepLeaves leaves = SweepLeaves()) {
    constexpr int kPrimVecs = HAS_QUADS ? 4 : 3;
    constexpr unsigned int kPrimBytes = kPrimVecs * PTMI_SWEEP_VEC_BYTES;
    float closest_t = t_max;
    slot_hit = -1;
    const bool long_form = ray_inv_long(d, live);
    const f3 inv = ray_inv_of(d, long_form);
    float t_lo = mt_t_lo(t_min), eps = 1e-8f, eps_up = __uint_as_float(__float_as_uint(1e-8f) + 1u);
    if (FORM & SWEEP_PINNED) {
        asm("" : "+v"(t_lo));
        asm("" : "+v"(eps));
        if (HAS_QUADS) asm("" : "+v"(eps_up));
    }
    if constexpr ((FORM & SWEEP_LEAVES) != 0) {                  // one wave-uniform decision per segment: ray_inv's vote and the scene's leaf count
        static_assert(!HAS_QUADS && !STATS && (FORM & SWEEP_NEAR_FAR) && (FORM & SWEEP_LEAF_BASE) && (FORM & SWEEP_VOTED_UPDATE), "sweep_form");
        if (!long_form && leaves.n > 0) {                        // inv is the short form here
            sweep_leaves_walk<FORM>(leaves, live, o, d, inv, t_min, eps, t_lo, closest_t, slot_hit);
            t_hit = closest_t;
            return slot_hit >= 0;
        }
    }
    constexpr bool NEAR_FAR = (FORM & SWEEP_NEAR_FAR) != 0;
    constexpr unsigned int kNodeBytes = sweep_node_vecs(FORM) * PTMI_SWEEP_VEC_BYTES;
    unsigned int far_x = 0, far_y = 0, far_z = 0;             // NEAR_FAR: where in an axis group this lane's (near, far) stands
    if constexpr (NEAR_FAR) {
        far_x = inv.x < 0.0f ? PTMI_SWEEP_NF_FAR_FIRST : 0;   // box_hit's own predicates
        far_y = inv.y < 0.0f ? PTMI_SWEEP_NF_FAR_FIRST : 0;
        far_z = inv.z < 0.0f ? PTMI_SWEEP_NF_FAR_FIRST : 0;
        asm("" : "+v"(far_x));
        asm("" : "+v"(far_y));
        asm("" : "+v"(far_z));
    }
    const unsigned int first = lds_address(nodes), end = first + (unsigned int)n_nodes * kNodeBytes;
    const unsigned int prims_at = lds_address(prims);
    unsigned int cur = live ? first : end;
    for (unsigned int at = first; at < end; at += kNodeBytes) {
        if (cur == at) {
            unsigned int here = cur;
            asm("" : "+v"(here));
            float w0, w1;                                         // the record's two w lanes
            int b;                                                // wave-uniform: >= 0 interior, < 0 leaf of -b
            bool pass;
            const auto leaf_flag = [&]() {                        // between the reads and the slab test in either form
                if (STATS) cn.node_visits++;
                b = __builtin_amdgcn_readfirstlane(__float_as_int(w1));
            };
            if constexpr (NEAR_FAR) {                             // (near, far) along each axis for this lane's ray
                const float2 bx = lds_pair(here + far_x, 0), by = lds_pair(here + far_y, 2), bz = lds_pair(here + far_z, 4);
                const float2 w = lds_pair(here, 6);
                w0 = w.x; w1 = w.y;
                leaf_flag();
                pass = box_hit_near_far(bx, by, bz, o, inv, t_min, closest_t);
            } else {
                const float4 n0 = lds_vec(here, 0), n1 = lds_vec(here, 1);
                w0 = n0.w; w1 = n1.w;
                leaf_flag();
                pass = box_hit(n0, n1, o, inv, t_min, closest_t);
            }
            const unsigned int next = here + kNodeBytes, skip = __float_as_uint(w0);
            const auto leaf_pass = [&]() {                       // the lanes whose ray meets the leaf's box test its -b primitives
                const unsigned int leaf = prims_at + (unsigned int)__builtin_amdgcn_readfirstlane(__float_as_int(w0)) * kPrimBytes;
                if constexpr ((FORM & SWEEP_LEAF_BASE) != 0) {
                    unsigned int rec = leaf;
                    asm("" : "+v"(rec));
                    const auto test = [&](int i) {
                        if (STATS) cn.prim_tests++;
                        leaf_prim_sweep<HAS_QUADS, FORM>(rec, i * kPrimVecs, o, d, eps, eps_up, t_lo, closest_t, slot_hit);
                    };
                    static_assert(kSweepLeafUnroll == 4, "the four calls below");
                    for (int left = -b; left > 0; left -= kSweepLeafUnroll, rec += kSweepLeafUnroll * kPrimBytes) {
                        test(0);
                        if (left > 1) test(1);
                        if (left > 2) test(2);
                        if (left > 3) test(3);
                    }
                } else {
                    for (int i = 0; i < -b; i++) {
                        if (STATS) cn.prim_tests++;
                        leaf_prim_sweep<HAS_QUADS, FORM>(leaf + i * kPrimBytes, 0, o, d, eps, eps_up, t_lo, closest_t, slot_hit);
                    }
                }
            };
            if constexpr ((FORM & SWEEP_MASKED_CURSOR) != 0) {
                cur = next;
                if ((b >= 0) & !pass) {                          // the lanes that miss an interior node: EXEC narrowed around one move
                    cur = skip;
                    asm volatile("" : "+v"(cur));                // or the optimiser turns the branch back into a select
                }
                if (b < 0 && pass) leaf_pass();
            } else if constexpr ((FORM & SWEEP_ONE_SELECT) != 0) {
                cur = ((b >= 0) & !pass) ? skip : next;
                if (b < 0 && pass) leaf_pass();
            } else if (b < 0) {
                cur = next;
                if (pass) leaf_pass();
            } else {
                cur = pass ? next : skip;
            }
        }
    }
    t_hit = closest_t;
    return slot_hit >= 0;
}

// GUIDED: only the sweep's form depends on it (sweep_form); the caller stages the records of that form and passes the leaf image
// stage_scene handed out (the sweep's builds that take SWEEP_LEAVES read it; every other walk ignores it)
template <int MODE, bool HAS_QUADS, bool STATS, bool GUIDED = false>
__device__ __forceinline__ bool scene_intersect(const float4* __restrict__ nodes, const float4* __restrict__ prims, int prim_stride,
                                                int n_nodes, int* stack, bool live, f3 o, f3 d, float t_min, float t_max,
                                                float& t_hit, int& slot_hit, LaneCounters& cn, SweepLeaves leaves = SweepLeaves()) {
    if (MODE == TRAVERSAL_SWEEP) return intersect_sweep<HAS_QUADS, STATS, sweep_form<HAS_QUADS, STATS, GUIDED>()>(nodes, prims, n_nodes, live, o, d, t_min, t_max, t_hit, slot_hit, cn, leaves);
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

// The first-hit walk of the Radiosity view, the feature pass, next-event estimation and the test hook ptmi_debug_first_hit, chosen
// on the host: MODE TRAVERSAL_CERTIFIED the certified walk (scenes above the sweep's 64 primitives: the 8-wide tree + the proof
// per hit, else the reference's walk - the reference's hit for every ray);
// TRAVERSAL_LANE / TRAVERSAL_STACK the reference's walk.  f(integral_constant MODE, integral_constant HAS_QUADS, LDS bytes).
template <typename F>
static void first_hit_walk(const DeviceScene& sc, F&& f) {
    const bool deep = sc.traversal == TRAVERSAL_STACK;                                // per-lane walk from global memory; stack only for deep trees
    const bool cert = sc.traversal == TRAVERSAL_CERTIFIED && sc.certified_ready();
    const size_t lds = cert ? (size_t)sc.w_depth * kBlock * sizeof(uint2) : deep ? (size_t)sc.stack_entries * kBlock * sizeof(int) : 0;
    auto with_quads = [&](auto mode) { with_bool(sc.has_quads, [&](auto quads) { f(mode, quads, lds); }); };
    if (cert) with_quads(std::integral_constant<int, TRAVERSAL_CERTIFIED>{});
    else if (deep) with_quads(std::integral_constant<int, TRAVERSAL_STACK>{});
    else with_quads(std::integral_constant<int, TRAVERSAL_LANE>{});
}

}  // namespace ptmi
