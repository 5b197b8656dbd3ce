// bounce.h — what the bounce kernel families share: their one argument block, the head and the tail of a launch, and one kernel
// selector per family (bounce_sync.hip, bounce_phased.hip, bounce_wide.hip).  kernels.hip: select_bounce_kernel maps a scene's
// traversal to its family.
#pragma once
#include "shading.h"
#include "sweep_records.h"
#include "frame_block.h"

namespace ptmi {

// The one argument of every bounce kernel
struct BounceArgs {
    DeviceScene sc; TileMap tm; PathState st; FrameParams fp;
    const int* queue_in; int n_in;          // n_in: upper bound known to the host (sizes the grid)
    const int* count_in;                    // device-side exact count of queue_in (nullptr: n_in is exact)
    int* queue_out; int* count_out;
    int segments;
    StatCounters* stats;
    int many_waves;                         // 1: more waves than the device holds at once (picks the 8-wave build of the packed walk)
    // count publishing (nullptr: off): the LAST workgroup of the launch to finish stores the launch's output count to a
    // host-mapped pinned slot and zeroes the next launch's counter, so a chunk's stream carries kernels only - no fill and
    // no 4-byte copy between two launches, each of which waits for a CU slot on a saturated GPU (r02: 11 % of c5frame)
    int* done_count;                        // workgroups of this launch that have finished (device memory, zero between launches)
    int* next_count;                        // the counter the next launch of this chunk will add to
    int* host_count;                        // pinned host memory, device address
    // cursor != nullptr: queue entries beyond the launch's threads are handed out through *cursor (zero at launch) to lanes whose
    // pixel has finished (the 8-wide walks; LaunchSchedule::refill_waves)
    int* cursor;
    // cost != nullptr: segments each pixel has taken in this frame, added to at the end of every visit (the next frame's launch
    // order: heaviest first, RenderState::orderByCost); cost_max: their maximum
    unsigned int* cost; unsigned int* cost_max;
};

// Every bounce kernel has this signature; a family's selector returns the ONE instantiation that `a` selects (its host-side
// handle: launch it, or ask the runtime for its occupancy).
using BounceKernel = void (*)(BounceArgs);
#pragma GCC visibility push(hidden)      // between the library's own files: the exported symbols stay the launchers
BounceKernel select_bounce_sync(const BounceArgs& a);        // TRAVERSAL_SWEEP / LANE / STACK: ptmi_bounce
BounceKernel select_bounce_phased(const BounceArgs& a);      // TRAVERSAL_PHASED / PACKED: ptmi_bounce_phased, ptmi_bounce_packed_w8
BounceKernel select_bounce_wide(const BounceArgs& a);        // TRAVERSAL_WIDE / CERTIFIED: ptmi_bounce_wide
#pragma GCC visibility pop

// guided = sampling_mode != SAMPLING_BSDF and CDF records present; otherwise the lean BSDF instantiation runs
inline bool is_guided(const BounceArgs& a) { return a.fp.sampling_mode != 0 && a.sc.cdfs != nullptr; }

// experiment-only builds (make trace-lib): the clock accounting of the phased and the wide kernels, compiled out otherwise
#ifdef PTMI_TRACE_WAVES
#define PTMI_TR(...) __VA_ARGS__
#else
#define PTMI_TR(...)
#endif

// stage the scene into LDS (when LDS_GEOM) and return the LDS cursor after it: [nodes | prims | mats], ptmi_scene_lds_vecs
// (sweep_records.h) vectors.  SWEEP_RECORDS: the node and primitive records in the sweep's form (ptmi_sweep_prepare) - the one
// place where a kernel that walks with intersect_sweep gets its records, the bounce kernel and the test hook alike - and, between
// the primitives and the materials, the frame block of fp / tm (frame_block.h: ptmi_sweep_lds_vecs vectors in all; the hook, which
// has no frame, passes none and leaves the block's place unwritten).  The block is at mats - PTMI_FRAME_BLOCK_VECS: frame_block_of(mats).
// SWEEP_FORM: the form of the walk that will read the records (traversal.h: sweep_form) - with SWEEP_NEAR_FAR the nodes are the
// near/far records of sweep_near_far.h, 4 vectors each (ptmi_sweep_near_far_lds_vecs vectors in all), otherwise 2 each; with
// SWEEP_LEAVES the scene's sc.sweep_leaves leaf records (sweep_leaves.h) follow the materials and `leaves` names them
// (ptmi_sweep_leaves_lds_vecs vectors in all; none where the scene's count is 0).
template <bool LDS_GEOM, bool SWEEP_RECORDS = false, int SWEEP_FORM = 0>
__device__ __forceinline__ float4* stage_scene(const DeviceScene& sc, float4* lds, const float4*& nodes, const float4*& prims, const float4*& mats,
                                               const FrameParams* fp, const TileMap* tm, SweepLeaves& leaves) {
    static_assert(LDS_GEOM || !SWEEP_RECORDS, "the sweep's records exist in LDS only");
    static_assert(SWEEP_RECORDS || SWEEP_FORM == 0, "a form belongs to the sweep's records");
    constexpr bool NEAR_FAR = (SWEEP_FORM & SWEEP_NEAR_FAR) != 0;
    nodes = sc.nodes; prims = sc.prims; mats = sc.mats;
    if (LDS_GEOM) {
        const int n_node_vec = sweep_node_vecs(SWEEP_FORM) * sc.n_nodes, n_prim_vec = sc.prim_stride * sc.n_prims, n_mat_vec = 3 * sc.n_prims;
        const int mats_at = n_node_vec + n_prim_vec + (SWEEP_RECORDS ? PTMI_FRAME_BLOCK_VECS : 0);
        if (SWEEP_RECORDS) {
            if (NEAR_FAR) ptmi_sweep_near_far_prepare(reinterpret_cast<const ptmi_vec_bits*>(sc.nodes), sc.n_nodes, reinterpret_cast<ptmi_vec_bits*>(lds),
                                                      lds_address(lds), (int)threadIdx.x, kBlock);
            ptmi_sweep_prepare(reinterpret_cast<const ptmi_vec_bits*>(sc.nodes), NEAR_FAR ? 0 : sc.n_nodes, reinterpret_cast<const ptmi_vec_bits*>(sc.prims),
                               sc.prim_stride, sc.n_prims, reinterpret_cast<ptmi_vec_bits*>(lds), reinterpret_cast<ptmi_vec_bits*>(lds + n_node_vec),
                               lds_address(lds), (int)threadIdx.x, kBlock);
            if (fp && threadIdx.x == kBlock - 1)      // one lane of the last wave: the first waves have the most records to prepare
                ptmi_frame_block_pack(fp->cam_origin, fp->cam_llc, fp->cam_hor, fp->cam_ver, tm->width, tm->height, tm->inv_width, tm->inv_height,
                                      reinterpret_cast<ptmi_vec_bits*>(lds + n_node_vec + n_prim_vec));
        } else {
            for (int i = threadIdx.x; i < n_node_vec; i += kBlock) lds[i] = sc.nodes[i];
            for (int i = threadIdx.x; i < n_prim_vec; i += kBlock) lds[n_node_vec + i] = sc.prims[i];
        }
        for (int i = threadIdx.x; i < n_mat_vec; i += kBlock) lds[mats_at + i] = sc.mats[i];
        nodes = lds; prims = lds + n_node_vec; mats = lds + mats_at;
        lds += mats_at + n_mat_vec;
        if constexpr ((SWEEP_FORM & SWEEP_LEAVES) != 0) {
            if (sc.sweep_leaves > 0)
                ptmi_sweep_leaves_prepare(reinterpret_cast<const ptmi_vec_bits*>(sc.nodes), sc.n_nodes, sc.prim_stride, reinterpret_cast<ptmi_vec_bits*>(lds),
                                          lds_address(prims), (int)threadIdx.x, kBlock);
            leaves.at = lds_address(lds);
            leaves.n = sc.sweep_leaves;
            lds += PTMI_SWEEP_LEAF_VECS * sc.sweep_leaves;
        }
        __syncthreads();
    }
    return lds;
}

// the same for the callers whose form has no leaf image (every walk but the sweep's builds that take SWEEP_LEAVES)
template <bool LDS_GEOM, bool SWEEP_RECORDS = false, int SWEEP_FORM = 0>
__device__ __forceinline__ float4* stage_scene(const DeviceScene& sc, float4* lds, const float4*& nodes, const float4*& prims, const float4*& mats,
                                               const FrameParams* fp = nullptr, const TileMap* tm = nullptr) {
    static_assert((SWEEP_FORM & SWEEP_LEAVES) == 0, "a form with SWEEP_LEAVES stages the leaf image: pass the SweepLeaves it fills");
    SweepLeaves none;
    return stage_scene<LDS_GEOM, SWEEP_RECORDS, SWEEP_FORM>(sc, lds, nodes, prims, mats, fp, tm, none);
}

// the frame block of a scene staged with SWEEP_RECORDS (mats: what stage_scene handed out)
__device__ __forceinline__ const float4* frame_block_of(const float4* mats) { return mats - PTMI_FRAME_BLOCK_VECS; }

// kernel tail shared by both bounce kernels: active-path compaction (one atomic per wave reserves queue space, lanes
// scatter by prefix popcount) and the optional workload counters
template <bool STATS, bool COMPACT = true>
__device__ __forceinline__ void finish_launch(const BounceArgs& a, bool alive, int slot, const LaneCounters& cn) {
    if (COMPACT) {
        const unsigned long long mask = __ballot(alive);
        const int lane = threadIdx.x & 63;
        int base = 0;
        if (lane == 0 && mask) base = atomicAdd(a.count_out, __popcll(mask));
        base = __shfl(base, 0);
        if (alive) a.queue_out[base + __popcll(mask & ((1ull << lane) - 1ull))] = slot;
    }
    if (STATS) {
        unsigned long long r = cn.rays, nv = cn.node_visits, pt = cn.prim_tests, h = cn.hits, tv = cn.top_visits;
        unsigned long long cc = cn.cert_chain, cf = cn.cert_fallback;
        for (int off = 32; off > 0; off >>= 1) {
            r += __shfl_down(r, off); nv += __shfl_down(nv, off); pt += __shfl_down(pt, off); h += __shfl_down(h, off); tv += __shfl_down(tv, off);
            cc += __shfl_down(cc, off); cf += __shfl_down(cf, off);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&a.stats->rays, r); atomicAdd(&a.stats->node_visits, nv);
            atomicAdd(&a.stats->prim_tests, pt); atomicAdd(&a.stats->hits, h);
            if (tv) atomicAdd(&a.stats->top_node_visits, tv);
            if (cc) atomicAdd(&a.stats->cert_chain, cc);
            if (cf) atomicAdd(&a.stats->cert_fallback, cf);
        }
    }
}

// Tail of every bounce kernel when count publishing is on: every WAVE of the grid passes here exactly once (also the ones
// that found nothing to do), after its own reservation in count_out - no workgroup barrier, a finished wave leaves at once
// (with a barrier in front of one arrival per workgroup the waves that finish early keep their registers until the
// workgroup's slowest is through: whole 1 M-triangle frame -4 %).  count_out is only ever touched by device-scope atomics,
// so the last arrival reads the sum.
__device__ __forceinline__ void publish_count(const BounceArgs& a) {
    if (!a.host_count) return;
    if ((threadIdx.x & 63) == 0) {
        __threadfence();
        if (atomicAdd(a.done_count, 1) == (int)(gridDim.x * (kBlock / 64)) - 1) {
            const int c = atomicAdd(a.count_out, 0);
            atomicExch(a.next_count, 0); atomicExch(a.next_count + 1, 0);      // output count, refill cursor
            atomicExch(a.done_count, 0);
            __hip_atomic_store(a.host_count, c, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// The end of a pixel's VISIT to a launch: all its samples are done (!more), or it has had its a.segments segments of this launch.
// Its state goes back to HBM; a pixel that is not through joins the output queue; and when the launch has fewer lanes than queue
// entries (BounceArgs::cursor) the lane takes the next entry no lane has taken yet - true: `slot` / `p` hold that pixel, with
// segs_left segments to go.  Call from the lanes whose visits end now (divergent code): they share one atomicAdd per counter.
__device__ __forceinline__ bool end_visit(const BounceArgs& a, int n_in, bool more, int& slot, PathRegs& p, int& segs_left) {
    store_path(a.st, slot, p);
    if (a.cost) {                                      // what this visit cost, for the next frame's launch order
        const unsigned int c = a.cost[slot] + (unsigned int)(a.segments - segs_left);
        a.cost[slot] = c;
        if (!more) atomicMax(a.cost_max, c);
    }
    const int lane = threadIdx.x & 63;
    const unsigned long long ending = __ballot(1), surviving = __ballot(more);
    const int first = __ffsll((long long)ending) - 1;
    int out_base = 0, in_base = 0;
    if (lane == first) {
        if (surviving) out_base = atomicAdd(a.count_out, __popcll(surviving));
        if (a.cursor) in_base = atomicAdd(a.cursor, __popcll(ending));
    }
    out_base = __shfl(out_base, first); in_base = __shfl(in_base, first);
    if (more) a.queue_out[out_base + __popcll(surviving & ((1ull << lane) - 1ull))] = slot;
    const int entry = (int)(gridDim.x * kBlock) + in_base + __popcll(ending & ((1ull << lane) - 1ull));
    if (!(a.cursor && entry < n_in)) return false;
    slot = a.queue_in ? a.queue_in[entry] : entry;
    load_path(a.st, a.tm, slot, p);
    segs_left = a.segments;
    return true;
}

}  // namespace ptmi
