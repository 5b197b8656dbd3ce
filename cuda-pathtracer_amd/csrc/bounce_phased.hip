// bounce_phased.hip — ptmi_bounce_phased and ptmi_bounce_packed_w8, the exact walk of larger scenes in wave-scheduled phases.
// Compile with -ffp-contract=off (kernels.hip).
#include "bounce.h"

namespace ptmi {

// ---- ptmi_bounce_phased: wave-scheduled phases (LANE walk for large scenes) -----------------------------------------
// A lane is always in one of three phases: NODE (next pre-order node to visit), PRIM (pending primitives of a leaf whose
// box it hit) or SHADE (traversal finished).  Every iteration the WAVE executes the one phase that most of its lanes
// are waiting for.  A lane whose ray ends early shades and starts its next segment while its neighbours are still
// walking the tree, instead of idling until the longest ray of the wave is done (segment-synchronous per-lane walk on
// the 1M-triangle scene: 13.8 % VALU lane utilisation).  Per lane the sequence of node visits, primitive tests and RNG
// draws is exactly the reference's; only the interleaving between lanes changes.
#ifdef PTMI_TRACE_WAVES
// experiment-only build (tools/wave_trace.py, never the shipped library): where a wave's clocks go.  [0] walk clocks
// [1] shade clocks [2] walk decisions [3] shade decisions [4] lanes advanced by walk decisions [5] lanes shaded [6] wave clocks
// [7] waves [8] longest wave [9] clocks outside the loop [10] living lanes summed over decisions [11] node decisions [12] node clocks
__device__ unsigned long long g_trace[16];
#endif
#ifndef PTMI_NODE_BURST
#define PTMI_NODE_BURST 3
#endif
template <bool LDS_GEOM, bool HAS_QUADS, bool STATS, bool GUIDED, bool PACKED, bool BATCH>
__device__ __forceinline__ void bounce_phased_body(const BounceArgs& a) {
    extern __shared__ float4 smem[];
    static_assert(!(PACKED && LDS_GEOM), "the packed layout is for scenes that do not fit LDS");
    const int n_in = a.count_in ? *a.count_in : a.n_in;
    if ((int)(blockIdx.x * kBlock) >= n_in) return;      // grid was sized from a stale (larger) count: nothing to do
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    const bool active = idx < n_in;
    const float4 *nodes, *prims, *mats;
    stage_scene<LDS_GEOM>(a.sc, smem, nodes, prims, mats);
    if (PACKED) nodes = a.sc.gnodes;
    const int n_top = PACKED ? a.sc.n_top : 0;           // the top of the packed tree, staged into LDS (device_scene.h)
    if (PACKED && n_top) {
        for (int i = threadIdx.x; i < 2 * n_top; i += kBlock) smem[i] = a.sc.gnodes[i];
        __syncthreads();
    }
    const MatSource ms = PACKED ? MatSource{a.sc.gmats, a.sc.mtab, a.sc.load_index} : MatSource{mats, nullptr, nullptr};
    if (GUIDED) fill_grid_solid_angles();

    const int slot = active ? (a.queue_in ? a.queue_in[idx] : idx) : 0;
    bool alive = active;
    PathRegs p = {};
    if (active) load_path(a.st, a.tm, slot, p);
    LaneCounters cn = {0, 0, 0, 0, 0, 0, 0};

    enum { PH_NODE = 0, PH_PRIM = 1, PH_SHADE = 2, PH_DONE = 3 };
    const int n_nodes = PACKED ? a.sc.n_pos : a.sc.n_nodes, prim_stride = a.sc.prim_stride;     // cursor >= n_nodes: walk finished
    const float t_min = 1e-4f, t_lo = mt_t_lo(t_min);
    int phase = alive ? PH_NODE : PH_DONE;
    int segs_left = a.segments;
    int cur = 0, pk = 0, pend = 0, slot_hit = -1;
    float closest_t = FLT_MAX;
    f3 inv = mk3(rcp_rn(p.d.x), rcp_rn(p.d.y), rcp_rn(p.d.z));
    if (STATS && alive) cn.rays++;

    PTMI_TR(const long long tr_t0 = clock64(); long long tr_walk = 0, tr_shade = 0, tr_node = 0; unsigned tr_nw = 0, tr_ns = 0, tr_lw = 0, tr_ls = 0, tr_alive = 0, tr_nn = 0;)
    while (true) {
        const int c_node = __popcll(__ballot(phase == PH_NODE));
        const int c_prim = __popcll(__ballot(phase == PH_PRIM));
        const int c_shade = __popcll(__ballot(phase == PH_SHADE));
        if (c_node + c_prim + c_shade == 0) break;
        PTMI_TR(const long long tr_a = clock64(); tr_alive += c_node + c_prim + c_shade;
                const int tr_kind = c_node >= c_prim && c_node >= c_shade ? 0 : c_prim >= c_shade ? 1 : 2;
                if (tr_kind == 0) { tr_nw++; tr_nn++; tr_lw += c_node; } else if (tr_kind == 1) { tr_nw++; tr_lw += c_prim; } else { tr_ns++; tr_ls += c_shade; })
        if (c_node >= c_prim && c_node >= c_shade) {
            // a short burst of node steps per scheduling decision: in large scenes a ray visits ~10 nodes between two
            // leaves, and the three ballots + branches of a decision cost about as much as a node test
#pragma unroll
            for (int burst = 0; burst < PTMI_NODE_BURST; burst++) {
                if (phase == PH_NODE) {                                // one node of Scene::intersect_bvh_optimized (scene.h:63-106)
                    float4 n0, n1;
                    if (PACKED && cur < n_top) { n0 = smem[2 * cur]; n1 = smem[2 * cur + 1]; if (STATS) cn.top_visits++; }
                    else { n0 = nodes[2 * cur]; n1 = nodes[2 * cur + 1]; }
                    if (STATS) cn.node_visits++;
                    const int na = __float_as_int(n0.w), nb = __float_as_int(n1.w);
                    const bool pass = box_hit(n0, n1, p.o, inv, t_min, closest_t);
                    int next;
                    if (PACKED) {                                      // explicit links (device_scene.h, PACKED LAYOUT)
                        if (nb < 0) {
                            next = ~nb;
                            if (pass) { pk = na >> 3; pend = pk + (na & 7); phase = PH_PRIM; }
                        } else next = pass ? nb : na;
                    } else {                                           // pre-order: left child = cur + 1, a = skip index
                        next = cur + 1;
                        if (nb < 0) {
                            if (pass) { pk = na; pend = na - nb; phase = PH_PRIM; }
                        } else if (!pass) next = na;
                    }
                    cur = next;
                    if (phase == PH_NODE && cur >= n_nodes) phase = PH_SHADE;
                }
            }
        } else if (c_prim >= c_shade) {
            if (phase == PH_PRIM) {                                    // one primitive of the leaf loop (scene.h:85-99)
                if (STATS) cn.prim_tests++;
                if (PACKED && !HAS_QUADS) leaf_prim_packed(a.sc.gprims, pk, p.o, p.d, t_lo, closest_t, slot_hit);
                else leaf_prim<HAS_QUADS>(prims, prim_stride, pk, p.o, p.d, t_lo, closest_t, slot_hit);
                pk++;
                if (pk == pend) phase = cur >= n_nodes ? PH_SHADE : PH_NODE;
            }
        } else {
            if (phase == PH_SHADE) {
                const bool more = shade_step<STATS, GUIDED, PACKED, BATCH>(a.fp, a.tm, ms, a.sc.cdfs, p, slot_hit >= 0, closest_t, slot_hit, cn, slot);
                segs_left--;
                if (!more) { alive = false; phase = PH_DONE; }
                else if (segs_left == 0) phase = PH_DONE;              // state goes back to HBM with the next ray ready
                else {
                    cur = 0; slot_hit = -1; closest_t = FLT_MAX;
                    inv = mk3(rcp_rn(p.d.x), rcp_rn(p.d.y), rcp_rn(p.d.z));
                    phase = PH_NODE;
                    if (STATS) cn.rays++;
                }
            }
        }
        PTMI_TR(const long long tr_d = clock64() - tr_a; if (tr_kind == 2) tr_shade += tr_d; else tr_walk += tr_d; if (tr_kind == 0) tr_node += tr_d;)
    }
    PTMI_TR(const long long tr_loop = clock64() - tr_t0;)

    if (active) store_path(a.st, slot, p);
    finish_launch<STATS>(a, alive, slot, cn);
#ifdef PTMI_TRACE_WAVES
    if ((threadIdx.x & 63) == 0) {
        const unsigned long long tot = (unsigned long long)(clock64() - tr_t0);
        const unsigned long long v[13] = {(unsigned long long)tr_walk, (unsigned long long)tr_shade, tr_nw, tr_ns, tr_lw, tr_ls, tot, 1ull, 0ull,
                                          tot - (unsigned long long)tr_loop, tr_alive, tr_nn, (unsigned long long)tr_node};
        for (int i = 0; i < 13; i++) if (i != 8) atomicAdd(&g_trace[i], v[i]);
        atomicMax(&g_trace[8], tot);
    }
#endif
}
template <bool LDS_GEOM, bool HAS_QUADS, bool STATS, bool GUIDED, bool PACKED, bool BATCH>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_num_sgpr(80))) void ptmi_bounce_phased(BounceArgs a) {
    bounce_phased_body<LDS_GEOM, HAS_QUADS, STATS, GUIDED, PACKED, BATCH>(a);
    publish_count(a);
}
// The packed walk of a triangle scene, BSDF sampling, bounded to 8 waves per SIMD (64 VGPRs, 11 spilled outside the walk
// loop): for frames with more waves than the device holds, where a wave more per SIMD is worth +5 % (whole 1 M-triangle frame
// 1 037 -> 1 088 Msamples/s, half +4.6 %); the chain-bound case keeps the 7-wave kernel (an eighth of that frame: -5 % with
// this one) - host/launch_rule.h decides per launch
template <bool STATS, bool BATCH>
__global__ __launch_bounds__(kBlock, 8) __attribute__((amdgpu_num_sgpr(80))) void ptmi_bounce_packed_w8(BounceArgs a) {
    bounce_phased_body<false, false, STATS, false, true, BATCH>(a);
    publish_count(a);
}

#ifdef PTMI_TRACE_WAVES
extern "C" int ptmi_trace_read(unsigned long long* out) {       // reads and clears the counters
    unsigned long long z[16] = {};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trace), sizeof(z)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_trace), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif

// The packed layout (TRAVERSAL_PACKED) is never LDS-resident; its 8-wave build is
// for triangle scenes with BSDF sampling and more waves than the device holds (BounceArgs::many_waves)
BounceKernel select_bounce_phased(const BounceArgs& a) {
    const bool packed = a.sc.traversal == TRAVERSAL_PACKED;
    return with_bool(a.stats != nullptr, [&](auto stats) {
        return with_bool(a.fp.n_frames > 1, [&](auto batch) {
            if (packed && a.many_waves && !is_guided(a) && !a.sc.has_quads)
                return BounceKernel(ptmi_bounce_packed_w8<decltype(stats)::value, decltype(batch)::value>);
            return with_bool(a.sc.has_quads, [&](auto quads) {
                return with_bool(is_guided(a), [&](auto guided) -> BounceKernel {
                    if (packed)
                        return ptmi_bounce_phased<false, decltype(quads)::value, decltype(stats)::value, decltype(guided)::value, true, decltype(batch)::value>;
                    return with_bool(a.sc.lds_resident, [&](auto geom) -> BounceKernel {
                        return ptmi_bounce_phased<decltype(geom)::value, decltype(quads)::value, decltype(stats)::value, decltype(guided)::value, false,
                                                  decltype(batch)::value>;
                    });
                });
            });
        });
    });
}

}  // namespace ptmi
