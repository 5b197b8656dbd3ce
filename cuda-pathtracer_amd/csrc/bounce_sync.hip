// bounce_sync.hip — ptmi_bounce, the segment-synchronous bounce kernel (scenes up to 64 primitives, and the deep-tree fallback).
// Compile with -ffp-contract=off (kernels.hip).
#include "bounce.h"

// experiment libraries (make ab-lib DEFS=-DPTMI_SWEEP_LATE=0 / -DPTMI_SWEEP_FRAME_BLOCK=0): the sweep's shade step as it was,
// shade_step; shade_step_sweep with the camera from kernel arguments.  The walk's own switches, -DPTMI_SWEEP_MASKED_HIT=0 and
// -DPTMI_SWEEP_MASKED_CURSOR=0, stand beside sweep_form in traversal.h, which the intersect hook reads too
#ifndef PTMI_SWEEP_FRAME_BLOCK
#define PTMI_SWEEP_FRAME_BLOCK 1
#endif
#ifndef PTMI_SWEEP_LATE
#define PTMI_SWEEP_LATE 1
#endif

namespace ptmi {

// ---- ptmi_bounce: segment-synchronous form (SWEEP and STACK walks) ------------------------------------------------
// Every wave traces one ray segment per lane, then shades, K times.  LDS: [nodes | prims | mats] when LDS_GEOM (always
// for SWEEP), then the traversal stacks (STACK only).
// amdgpu_num_sgpr(80): with <= 80 SGPRs eight 256-thread workgroups fit a CU instead of six
// (MI355X_MICROARCH.md, residency rule); measured +2.4 %, no spills.
// GUIDED instantiations would take ~100 VGPRs (4 waves per SIMD); capped at 80 (6 waves, 68 bytes of spills): grid
// sampling +13 %, MIS +9 % on the benchmark frame (5 waves +8 %, 7 the same as 6, 8 waves +10 % / +3 %).
// The sweep's BATCH builds and its quad builds without STATS are held to 8 waves per SIMD (64 VGPRs): left alone the quad build
// takes 65 for the address cursor (traversal.h: intersect_sweep) and drops to 7 waves; held, it takes 63 and spills nothing.
template <int MODE, bool LDS_GEOM, bool HAS_QUADS, bool STATS, bool GUIDED, bool BATCH>
__device__ __forceinline__ void bounce_body(const BounceArgs& a) {
    extern __shared__ float4 smem[];
    static_assert(MODE != TRAVERSAL_SWEEP || LDS_GEOM, "the sweep reads the scene through LDS broadcasts");
    const int n_in = a.count_in ? *a.count_in : a.n_in;
    if ((int)(blockIdx.x * kBlock) >= n_in) return;      // grid was sized from a stale (larger) count: nothing to do
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    const bool active = idx < n_in;
    const float4 *nodes, *prims, *mats;
    float4* lds;
    SweepLeaves leaves;
    if constexpr (MODE == TRAVERSAL_SWEEP) lds = stage_scene<LDS_GEOM, true, sweep_form<HAS_QUADS, STATS, GUIDED>()>(a.sc, smem, nodes, prims, mats, &a.fp, &a.tm, leaves);      // the records of this build's walk, with the frame block
    else lds = stage_scene<LDS_GEOM>(a.sc, smem, nodes, prims, mats);
    constexpr bool LEAN = MODE == TRAVERSAL_SWEEP && !STATS && !GUIDED;      // shading.h: shade_step
    constexpr bool LATE = LEAN && PTMI_SWEEP_LATE;                           // shading.h: shade_step_sweep
    constexpr bool FRAME = LATE && PTMI_SWEEP_FRAME_BLOCK;                   // its camera branch reads the frame block stage_scene laid out
    FrameBlock fb;
    if constexpr (FRAME) fb = frame_block(frame_block_of(mats), a.tm);
    int* stack = reinterpret_cast<int*>(lds) + threadIdx.x;
    if (GUIDED) fill_grid_solid_angles();

    const int slot = active ? (a.queue_in ? a.queue_in[idx] : idx) : 0;
    bool alive = active;
    PathRegs p = {};
    if (active) load_path(a.st, a.tm, slot, p);
    LaneCounters cn = {0, 0, 0, 0, 0, 0, 0};

    for (int seg = 0; seg < a.segments; seg++) {
        if (!__any(alive)) break;
        // the whole wave enters the traversal together (finished lanes ride along masked): required by SWEEP
        float t = 0.0f; int k = -1;
        if (STATS && alive) cn.rays++;
        const bool hit = scene_intersect<MODE, HAS_QUADS, STATS, GUIDED>(nodes, prims, a.sc.prim_stride, a.sc.n_nodes, stack, alive,
                                                                       p.o, p.d, 1e-4f, FLT_MAX, t, k, cn, leaves);
        if constexpr (LATE) {
            if (alive) alive = shade_step_sweep<BATCH, FRAME>(a.fp, a.tm, fb, mats, p, hit, t, k, slot);
        } else {
            if (alive) alive = shade_step<STATS, GUIDED, false, BATCH, LEAN>(a.fp, a.tm, MatSource{mats, nullptr, nullptr}, a.sc.cdfs, p, hit, t, k, cn, slot);
        }
    }

    if (active) store_path(a.st, slot, p);
    finish_launch<STATS>(a, alive, slot, cn);
}
template <int MODE, bool LDS_GEOM, bool HAS_QUADS, bool STATS, bool GUIDED, bool BATCH>
__global__ __launch_bounds__(kBlock, GUIDED ? 6 : ((BATCH || (HAS_QUADS && !STATS)) && MODE == TRAVERSAL_SWEEP ? 8 : 1)) __attribute__((amdgpu_num_sgpr(80))) void ptmi_bounce(BounceArgs a) {
    bounce_body<MODE, LDS_GEOM, HAS_QUADS, STATS, GUIDED, BATCH>(a);
    publish_count(a);
}

// SWEEP exists only with the scene in LDS; LANE and STACK in both forms
BounceKernel select_bounce_sync(const BounceArgs& a) {
    const auto pick = [&](auto mode, auto geom) {
        return with_bool(a.sc.has_quads, [&](auto quads) {
            return with_bool(a.stats != nullptr, [&](auto stats) {
                return with_bool(is_guided(a), [&](auto guided) {
                    return with_bool(a.fp.n_frames > 1, [&](auto batch) -> BounceKernel {
                        return ptmi_bounce<decltype(mode)::value, decltype(geom)::value, decltype(quads)::value, decltype(stats)::value,
                                           decltype(guided)::value, decltype(batch)::value>;
                    });
                });
            });
        });
    };
    switch (a.sc.traversal) {
        case TRAVERSAL_SWEEP: return pick(std::integral_constant<int, TRAVERSAL_SWEEP>{}, std::true_type{});
        case TRAVERSAL_LANE: return with_bool(a.sc.lds_resident, [&](auto geom) { return pick(std::integral_constant<int, TRAVERSAL_LANE>{}, geom); });
        default: return with_bool(a.sc.lds_resident, [&](auto geom) { return pick(std::integral_constant<int, TRAVERSAL_STACK>{}, geom); });
    }
}

}  // namespace ptmi
