// bounce_wide.hip — ptmi_bounce_wide, the bounce kernel over the opt-in fast tree (plain and certified).
// Compile with -ffp-contract=off (kernels.hip).
#include "bounce.h"

namespace ptmi {

// ---- ptmi_bounce_wide: the opt-in fast tree (csrc/wide_bvh.h) --------------------------------------------------------------
// The phased scheduling of ptmi_bounce_phased over the 8-wide SAH tree.  A NODE step enters ONE inner child: it takes the
// front-most pending child of the lane's current group (or pops a group), fetches that child's 128-byte node - one L2 line,
// or LDS for the top levels - and decides its eight children at once: hit inner children become the new current group, the
// triangles of hit leaf children a 24-bit mask that the following PRIM steps test one by one.  Stack: one (child_base,
// imask << 8 | pending) pair per tree level in LDS, entry e of lane l at stack[e * kBlock + l] - conflict-free whatever e.
// The triangle test is the exact walk's (mt_hit = mt_accept's arithmetic); equal-t hits keep the smaller reference slot.
// Measured and dropped: a UNIFIED step (a lane's pending triangle and its next node fetched and tested in one step, two phases
// to vote between): 92 registers, 5 waves per SIMD: 1 610 / 2 322 Msamples/s (an eighth / the whole 1 M-triangle frame) against
// 1 719 / 2 405 for this form at 6 waves; bounded to 6 waves it spills inside the loop (867 / 1 100).
// CERT (TRAVERSAL_CERTIFIED): the same walk made EXACT - under one stated premise.
//   PREMISE (P).  Every triangle j whose Moller-Trumbore test (mt_hit = the reference's arithmetic) accepts the ray at a distance
//   t_j inside [t_min, c] is TESTED by the fast walk while its closest_t is >= c: the slab tests of the fast walk pass for j's
//   leaf child and for all its ancestors.  Geometrically that is what "conservative boxes" means; in floating point it needs
//   the computed hit point o + t_j d to lie within the pad of j's box (2^-16 of the scene's scale, host/wide_bvh.cpp).  The
//   computed t_j is off by at most about 2^-20 (|o - v0| + t_j) / kappa, kappa = |a| / (|e1| |e2|) (a = e1 . (d x e2), the
//   determinant the test divides by; kappa = sin of the triangle's corner angle x cos of the incidence angle).  With origin and
//   hit inside the scene (|o - v0| + t_j <= 2 S) that is within the pad for kappa >= 1 / 8: there (P) is PROVEN.  Below that
//   floor - rays within about 7 degrees of a triangle's plane, slivers, needles; down at |a| ~ 1e-8 the reference itself accepts
//   distances that are numerical noise - (P) is TESTED, NOT PROVEN: tools/certified_soak.py (sheets skimmed at 1e-7 .. 1e-3 rad, fences of needles with 1e-8 .. 1e-5 short
//   edges, stacked layers of large triangles 1e-4 apart, a sloppy exporter's degenerate primitives, an outlier a million units
//   away; 0 mismatches against the walk over the reference's tree), VERDICT r3's 750 000 adversarial rays (0 mismatches) and
//   BASELINE configs[4] at its full 8.6 G samples (identical frames).
//   Under (P) the fast walk's hit (t*, k*) is the global minimum over all accepted triangles, and the reference's own walk
//   (scene.h:50-110) returns exactly the same hit if (1) it reaches k*'s leaf and (2) no second triangle is hit at exactly t*.
// (1): the reference enters a node when `!(min(t_exit, closest_t) < t_entry)` holds for it and all its ancestors, closest_t being
// whatever it is at that moment - never below the final t*; the test is monotone in closest_t, so if every ancestor of k*'s leaf
// (leaf included) passes with closest_t = t* it passes in the reference.  One fetch (the leaf's box: csrc/wide_walk.h) shows
// that for 99.7 % of the hits; the rest evaluate these slab tests themselves (box_hit, the exact walk's arithmetic) from a
// per-leaf list of ancestor node indices, leaf first, four nodes per step fetched in parallel, until a box holds the hit point
// with the margin - mostly the parent or grandparent.
// (2): every triangle hit at t* is tested by the fast walk too (P), so a tie shows as `t == closest_t` there.  A ray for which
// (1) or (2) cannot be shown - a grazed box, a shared edge, an origin outside the range the boxes were padded for - is walked
// again by the reference's own walk (intersect_lane) inside this kernel: about one ray in 10^5 on the 1 M-triangle scene.  No hit
// at all needs no check: under (P) the reference can only accept triangles the fast walk would have found.
// (What was measured on the way and dropped: EXPERIMENTS.md.)
#ifndef PTMI_PRIM_BATCH
#define PTMI_PRIM_BATCH 2
#endif
#ifndef PTMI_QUAD_BATCH
#define PTMI_QUAD_BATCH 2
#endif
#ifdef PTMI_TRACE_WAVES
// experiment-only build (tools/wide_trace.py): one 12-word record per wave of ptmi_bounce_wide - start (wall_clock64, low word),
// duration in ticks, decisions and lanes advanced per kind (NODE / PRIM / SHADE), shader clocks per kind, lanes the wave started with
// (low byte of the last word; above it: ticks after which fewer than 32 of its lanes still had work, 0 = never)
constexpr unsigned int kWideTraceCap = 1u << 19;
__device__ unsigned int g_wt_n;
__device__ unsigned int g_wt[kWideTraceCap * 12];
#endif
template <bool STATS, bool GUIDED, bool BATCH, bool CERT, bool QUADS>
__device__ __forceinline__ void bounce_wide_body(const BounceArgs& a) {
    extern __shared__ float4 smem[];
    PTMI_TR(const unsigned long long wt_t0 = (unsigned long long)wall_clock64(); unsigned int wt_n[3] = {0, 0, 0}, wt_l[3] = {0, 0, 0}, wt_half = 0; unsigned long long wt_c[3] = {0, 0, 0};)
    const int n_in = a.count_in ? *a.count_in : a.n_in;
    if ((int)(blockIdx.x * kBlock) >= n_in) return;      // grid was sized from a stale (larger) count: nothing to do
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    const bool active = idx < n_in;
    const int n_top = a.sc.w_top;
    uint4* top = reinterpret_cast<uint4*>(smem);
    for (int i = threadIdx.x; i < 8 * n_top; i += kBlock) top[i] = a.sc.wnodes[i];
    uint2* stack = reinterpret_cast<uint2*>(top + 8 * n_top) + threadIdx.x;
    __syncthreads();
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) u32x4 LdsU4;
    typedef __attribute__((address_space(1))) u32x4 GlobalU4;
    auto u4 = [](u32x4 v) { return make_uint4(v.x, v.y, v.z, v.w); };
    const LdsU4* top_lds = (const LdsU4*)top;
    const GlobalU4* wnodes_g = (const GlobalU4*)a.sc.wnodes;
    // (the certified walk shades from the line its proof has just read: DeviceScene::wcert)
    const MatSource ms = CERT ? MatSource{a.sc.wcert + 2, a.sc.wmtab, a.sc.wload_index, kWideCertStride} : MatSource{a.sc.wmats, a.sc.wmtab, a.sc.wload_index, 1};
    if (GUIDED) fill_grid_solid_angles();

    int slot = active ? (a.queue_in ? a.queue_in[idx] : idx) : 0;
    bool alive = active;
    PathRegs p = {};
    if (active) load_path(a.st, a.tm, slot, p);
    LaneCounters cn = {0, 0, 0, 0, 0, 0, 0};

    enum { PH_NODE = 0, PH_PRIM = 1, PH_SHADE = 2, PH_DONE = 3, PH_VERIFY = 4, PH_EXACT = 5 };
    constexpr int kTieFlag = 0x40000000;      // CERT: set in slot_hit while a second triangle is accepted at exactly closest_t
    const float t_min = 1e-4f, t_lo = mt_t_lo(t_min);
    // CERT keeps no state of its own through the walk: a tie is a flag in slot_hit (a closer hit clears it - only a tie at the
    // final t* matters), a ray that has to take the reference's walk is a phase (PH_EXACT), and the proof's cursor (next 4-node
    // chunk of the hit leaf's ancestor list, chunks left) lives in g_base / t_base, which are dead once the walk has ended
    int phase = alive ? PH_NODE : PH_DONE;
    int segs_left = a.segments;
    int slot_hit = -1, sp = 0;
    float closest_t = FLT_MAX;
    f3 inv;
    uint32_t octinv, g_base, g_bits;
    WIDE_WALK_BEGIN(p.d, inv, octinv, g_base, g_bits);
    uint32_t t_base = 0u, t_mask = 0u;
    if (STATS && alive) cn.rays++;
    // where the walk goes when it has run out of nodes and triangles
    auto after_walk = [&]() -> int {
        if (!CERT) return PH_SHADE;
        if (slot_hit < 0) return PH_SHADE;
        if (slot_hit & kTieFlag) return PH_EXACT;                      // a tie at t*: let the reference's walk decide
        t_base = 0xffffffffu;                                          // first the one-fetch certificate, then (rarely) the chain
        return PH_VERIFY;
    };
    auto origin_in_range = [&]() { return wide_origin_ok(a.sc, p.o); };
    if (CERT && alive && !origin_in_range()) phase = PH_EXACT;

    while (true) {
        const int c_node = __popcll(__ballot(phase == PH_NODE));
        const int c_prim = __popcll(__ballot(phase == PH_PRIM));
        // a lane whose hit has to be proven (VERIFY) votes with the SHADE lanes and takes one proof step right before that
        // phase's work - for almost every hit the only one (the leaf-box fetch).  As a phase of its own (round 3's first form)
        // the proof cost a wave iteration per ray and its stragglers waited for a majority: c5tile 1 407 -> 1 455 Msamples/s
        const int c_shade = __popcll(__ballot(phase == PH_SHADE || (CERT && phase >= PH_VERIFY)));
        if (c_node + c_prim + c_shade == 0) break;
        PTMI_TR(if (!wt_half && c_node + c_prim + c_shade < 32) wt_half = (unsigned int)((unsigned long long)wall_clock64() - wt_t0);)
        PTMI_TR(const int wt_k = c_node >= c_prim && c_node >= c_shade ? 0 : c_prim >= c_shade ? 1 : 2; const long long wt_a = clock64();
                wt_n[wt_k]++; wt_l[wt_k] += wt_k == 0 ? c_node : wt_k == 1 ? c_prim : c_shade;)
        if (c_node >= c_prim && c_node >= c_shade) {
            if (phase == PH_NODE) {
                WIDE_NEXT_NODE(ni, g_base, g_bits, sp, stack, octinv, {});
                uint4 q0, q1, q2, q3, q4, q5, q6;
                if ((int)ni < n_top) {
                    // explicit address spaces: left generic, the two branches are merged into ONE flat_load through a selected pointer
                    const LdsU4* q = top_lds + 8 * ni;
                    q0 = u4(q[0]); q1 = u4(q[1]); q2 = u4(q[2]); q3 = u4(q[3]); q4 = u4(q[4]); q5 = u4(q[5]); q6 = u4(q[6]);
                    if (STATS) cn.top_visits++;
                } else {
                    const GlobalU4* q = wnodes_g + 8 * (size_t)ni;
                    q0 = u4(q[0]); q1 = u4(q[1]); q2 = u4(q[2]); q3 = u4(q[3]); q4 = u4(q[4]); q5 = u4(q[5]); q6 = u4(q[6]);
                }
                if (STATS) cn.node_visits++;
                const WideStep st = wide_node_test(q0, q1, q2, q3, q4, q5, q6, p.o, inv, octinv, t_min, closest_t);
                g_base = st.child_base; g_bits = (st.imask << 8) | st.inner;
                t_base = st.tri_base; t_mask = st.tris;
                if (t_mask) phase = PH_PRIM;
                else if ((g_bits & 0xffu) == 0u && sp == 0) phase = after_walk();
            }
        } else if (c_prim >= c_shade) {
            if (phase == PH_PRIM) {
                // up to PTMI_PRIM_BATCH pending triangles per step: their records are fetched together (one latency), then tested
                // in ascending order
                // (scenes with quads: 64-byte records - v0 | type, e1, e2, e3, the layout of d_prims -, two per step as well: 4 096 / 16 384
                // planar quads 2 180 -> 2 290 / 1 730 -> 1 875 Msamples/s)
                constexpr int kPB = QUADS ? PTMI_QUAD_BATCH : PTMI_PRIM_BATCH;
                int kk[kPB]; bool has[kPB]; f3p r0[kPB], r1[kPB], r2[kPB]; float4 q0[kPB], q1[kPB], q2[kPB], q3[kPB];
#pragma unroll
                for (int b = 0; b < kPB; b++) {
                    has[b] = t_mask != 0u;
                    kk[b] = has[b] ? (int)t_base + __ffs((int)t_mask) - 1 : (b ? kk[b - 1] : 0);
                    t_mask &= t_mask - 1u;                                 // 0 stays 0
                    if (QUADS) {
                        const float4* r = a.sc.wqprims + 4 * (size_t)kk[b];
                        q0[b] = r[0]; q1[b] = r[1]; q2[b] = r[2]; q3[b] = r[3];
                    } else {
                        const f3p* r = reinterpret_cast<const f3p*>(a.sc.wprims) + 3 * (size_t)kk[b];
                        r0[b] = r[0]; r1[b] = r[1]; r2[b] = r[2];
                    }
                }
#pragma unroll
                for (int b = 0; b < kPB; b++) {
                    if (b > 0 && !__any(has[b])) break;
                    if (has[b]) {
                        const int k = kk[b];
                        if (STATS) cn.prim_tests++;
                        float tt = 0.0f;
                        const bool ok = QUADS ? wide_quad_hit(q0[b], q1[b], q2[b], q3[b], p.o, p.d, t_lo, tt) : wide_tri_hit(r0[b], r1[b], r2[b], p.o, p.d, t_lo, tt);
                        if (ok) {
                            if (tt < closest_t) { closest_t = tt; slot_hit = k; }
                            else if (tt == closest_t && slot_hit >= 0) {           // the reference keeps the hit it visits first (scene.h:89-90)
                                if (CERT) slot_hit |= kTieFlag;
                                else if (a.sc.wref_slot[k] < a.sc.wref_slot[slot_hit]) slot_hit = k;
                            }
                        }
                    }
                }
                if (t_mask == 0u) phase = ((g_bits & 0xffu) != 0u || sp > 0) ? PH_NODE : after_walk();
            }
        } else {
            if (CERT && phase >= PH_VERIFY) {
                if (phase == PH_VERIFY && t_base == 0xffffffffu) {
                    // ONE fetch: the box of the hit triangle's leaf in the reference's tree (the argument: csrc/wide_walk.h)
                    const float4 lo = a.sc.wcert[kWideCertStride * (size_t)slot_hit], hi = a.sc.wcert[kWideCertStride * (size_t)slot_hit + 1];
                    const f3 q = p.o + closest_t * p.d;
                    const bool inside = CERT_LEAF_INSIDE(p.o, q, lo, hi);
                    const bool finite_slopes = CERT_SLOPES_OK(p.d, kCertSlope);
                    if (inside && finite_slopes) phase = PH_SHADE;
                    else {
                        g_base = cert_first_chunk(lo); t_base = cert_chunks(lo);
                        inv = mk3(rcp_rn(p.d.x), rcp_rn(p.d.y), rcp_rn(p.d.z));       // the reference's 1 / d for its slab tests
                        if (STATS) cn.cert_chain++;
                        if (t_base == 0u) phase = PH_EXACT;                         // (no list: fails closed; the count below must not wrap)
                    }
                } else if (phase == PH_VERIFY) {
                    // one 4-node chunk of the chain, leaf first, with the reference's own slab test
                    CERT_CHUNK(proven, failed, a.sc, g_base, (g_base++, t_base--), p.o, p.d, closest_t, kCertSlope, box_hit(n0[c], n1[c], p.o, inv, t_min, closest_t));
                    if (STATS) cn.node_visits += 4;
                    if (failed) phase = PH_EXACT;
                    else if (proven || t_base == 0u) phase = PH_SHADE;
                }
                if (phase == PH_EXACT) {                               // the reference's walk itself, for this ray only
                    float t_ref = 0.0f; int slot_ref = -1;
                    const bool h = intersect_lane<QUADS, STATS>(a.sc.nodes, a.sc.prims, a.sc.prim_stride, a.sc.n_nodes, true, p.o, p.d, t_min, FLT_MAX,
                                                                t_ref, slot_ref, cn);
                    closest_t = h ? t_ref : FLT_MAX;
                    slot_hit = h ? a.sc.wfast_of_ref[slot_ref] : -1;
                    phase = PH_SHADE;
                    if (STATS) cn.cert_fallback++;
                }
            }
            if (phase == PH_SHADE) {
                const bool more = shade_step<STATS, GUIDED, true, BATCH>(a.fp, a.tm, ms, a.sc.cdfs, p, slot_hit >= 0, closest_t, slot_hit, cn, slot);
                segs_left--;
                if (more && segs_left != 0) {                          // the next segment of this pixel
                    slot_hit = -1; closest_t = FLT_MAX; sp = 0; t_mask = 0u;
                    WIDE_WALK_BEGIN(p.d, inv, octinv, g_base, g_bits);
                    phase = PH_NODE;
                    if (STATS) cn.rays++;
                    if (CERT && !origin_in_range()) phase = PH_EXACT;
                } else {
                    phase = PH_DONE;
                    if (end_visit(a, n_in, more, slot, p, segs_left)) {            // the lane goes on with the next queued pixel
                        slot_hit = -1; closest_t = FLT_MAX; sp = 0; t_mask = 0u;
                        WIDE_WALK_BEGIN(p.d, inv, octinv, g_base, g_bits);
                        phase = PH_NODE;
                        if (STATS) cn.rays++;
                        if (CERT && !origin_in_range()) phase = PH_EXACT;
                    }
                }
            }
        }
        PTMI_TR(wt_c[wt_k] += (unsigned long long)(clock64() - wt_a);)
    }

    finish_launch<STATS, false>(a, false, slot, cn);      // every visit has banked its pixel and queued it if it goes on: counters only
#ifdef PTMI_TRACE_WAVES
    {
        const unsigned int lanes0 = (unsigned int)__popcll(__ballot(active));
        if ((threadIdx.x & 63) == 0) {
            const unsigned int i = atomicAdd(&g_wt_n, 1u);
            if (i < kWideTraceCap) {
                unsigned int* w = g_wt + 12 * (size_t)i;
                w[0] = (unsigned int)wt_t0; w[1] = (unsigned int)((unsigned long long)wall_clock64() - wt_t0);
                w[2] = wt_n[0]; w[3] = wt_l[0]; w[4] = wt_n[1]; w[5] = wt_l[1]; w[6] = wt_n[2]; w[7] = wt_l[2];
                w[8] = (unsigned int)(wt_c[0] >> 4); w[9] = (unsigned int)(wt_c[1] >> 4); w[10] = (unsigned int)(wt_c[2] >> 4); w[11] = lanes0 | (wt_half << 8);
            }
        }
    }
#endif
}
#ifndef PTMI_WIDE_WAVES
#define PTMI_WIDE_WAVES 6
#endif
template <bool STATS, bool GUIDED, bool BATCH, bool CERT, bool QUADS>
__global__ __launch_bounds__(kBlock, PTMI_WIDE_WAVES) __attribute__((amdgpu_num_sgpr(80))) void ptmi_bounce_wide(BounceArgs a) {
    bounce_wide_body<STATS, GUIDED, BATCH, CERT, QUADS>(a);
    publish_count(a);
}

#ifdef PTMI_TRACE_WAVES
// copies up to cap records (12 words each) of the wide walk's wave trace to out, returns how many there were, and clears
extern "C" long long ptmi_wide_trace_read(unsigned int* out, long long cap) {
    unsigned int n = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_wt_n), sizeof n) != hipSuccess) return -1;
    const unsigned int m = n < kWideTraceCap ? n : kWideTraceCap;
    const long long k = (long long)m < cap ? (long long)m : cap;
    if (k > 0 && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wt), (size_t)k * 12 * sizeof(unsigned int)) != hipSuccess) return -1;
    const unsigned int z = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_wt_n), &z, sizeof z) != hipSuccess) return -1;
    return (long long)n;
}
#endif

BounceKernel select_bounce_wide(const BounceArgs& a) {
    return with_bool(a.stats != nullptr, [&](auto stats) {
        return with_bool(is_guided(a), [&](auto guided) {
            return with_bool(a.fp.n_frames > 1, [&](auto batch) {
                return with_bool(a.sc.traversal == TRAVERSAL_CERTIFIED, [&](auto cert) {
                    return with_bool(a.sc.wqprims != nullptr, [&](auto quads) -> BounceKernel {
                        return ptmi_bounce_wide<decltype(stats)::value, decltype(guided)::value, decltype(batch)::value, decltype(cert)::value,
                                                decltype(quads)::value>;
                    });
                });
            });
        });
    });
}

}  // namespace ptmi
