// launch_rule.h — how a path-tracing run is cut into ptmi_bounce launches: segments per launch, refill, launch order by cost,
// the automatic chunk count and, per launch, whether the rest of the frame fits.  Pure arithmetic over plain numbers: nothing
// of HIP is included, so the rule runs (and is tested, tests/test_launch_rule.py) without a GPU.  host/render_run.cpp feeds it.
#pragma once
#include <algorithm>
#include <cstdlib>

namespace ptmi {

// The A/B hooks of the launch loop, read from the environment once per run (tools and one test change them between two frames
// of one process): PTMI_PUBLISH=1, PTMI_REFILL=0, PTMI_ORDER=0 | 1 | number of classes
struct LaunchOverrides {
    bool publish = false;                            // count publishing (render_run.cpp: armCount)
    bool refill_off = false;                         // PTMI_REFILL=0; any other value changes nothing
    bool order_set = false, order_on = false;        // PTMI_ORDER: 0 switches the cost order off, any other value forces it on
    int order_value = 0;                             // ... and a value above 1 is also the class count
    static LaunchOverrides fromEnv() {
        LaunchOverrides o;
        if (const char* e = getenv("PTMI_PUBLISH")) o.publish = e[0] == '1';
        if (const char* e = getenv("PTMI_REFILL")) o.refill_off = e[0] == '0';                   // A/B hooks of round 4 (tools/occupancy_probe.py)
        if (const char* e = getenv("PTMI_ORDER")) { o.order_set = true; o.order_on = e[0] != '0'; o.order_value = atoi(e); }
        return o;
    }
};

// The effective walk of the run (after the fast-tree and certified fallbacks), as the rule sees it.  None set: LANE or STACK.
struct LaunchWalk {
    bool phased = false;                             // PHASED, PACKED, WIDE or CERTIFIED: the wave-scheduled per-lane walks
    bool wide = false;                               // WIDE or CERTIFIED: the 8-wide walks (a subset of phased)
    bool sweep = false;                              // SWEEP
};

struct LaunchRuleInput {
    LaunchWalk walk;
    int segments_per_launch = 0, spp = 1;            // AppConfig; segments_per_launch 0: the rule decides
    long long n_local = 0;
    int n_frames = 1;
    bool nee = false;                                // one launch of ptmi_render_nee: no chunks, no refill, no launch order by cost
    bool is_pass = false;                            // an accumulation pass: its queue runs as one chunk
    int want_chunks = 0;                             // RenderState: 0 = automatic, else forced
    long long wave_slots = 0;                        // bounce_resident_waves(), 0 where needsWaveSlots() says it is not asked
    LaunchOverrides over;
};

struct LaunchRule {
    // "the rest of the frame": bounded so that one launch stays well below a minute (a lane of the 1 M-triangle scene does
    // ~4 000 segments per second; BASELINE's 2048 spp x 8 bounces = 16 384 segments at most = ONE 1.45 s launch per chunk.  A
    // boundary in mid-frame is dear: with 8 192 the same frame took 1.58 s)
    static constexpr int kRestOfFrameSegments = 65536;

    int segments = 32, rest_segments = kRestOfFrameSegments;
    long long fit_pct = 30, wave_slots = 0;
    bool phased = false;
    bool refill = false;
    int run_ahead = 2;                               // launches the host keeps queued per chunk
    bool order_by_cost = false;
    int order_classes = 16;
    int n_frames = 1;
    int auto_chunks = 0;                             // the chunk count the walk wants; 0: the rule asks for no change

    // Whether the occupancy query is made at all: only where the rule decides the segments and the walk has a use for the answer
    static bool needsWaveSlots(const LaunchWalk& w, int segments_per_launch) { return segments_per_launch <= 0 && (w.phased || w.sweep); }

    static LaunchRule plan(const LaunchRuleInput& in) {
        LaunchRule p;
        const LaunchWalk& w = in.walk;
        p.phased = w.phased; p.n_frames = in.n_frames;
        p.wave_slots = needsWaveSlots(w, in.segments_per_launch) ? in.wave_slots : 0;
        // segments per launch: 32 while the device has more waves to run than it holds at once; once the pixels still active fit
        // (an eighth of a 2048^2 frame per GPU from its first launch on; the last stretch of any other frame), the frame is as
        // long as the chain of its heaviest pixels, every launch boundary makes it wait for the slowest wave once more, and the
        // rest of the frame goes into ONE launch per chunk (1 M-triangle scene, 1/8 of the frame: 47 instead of 59 ms; with more
        // waves than slots one launch is slower, the second round starts a whole chain late) - DESIGN.md 5
        // (the phased kernels: spp / 4, see below)
        p.segments = in.segments_per_launch > 0 ? in.segments_per_launch : 32;
        // The phased kernels keep their lanes busy across sample boundaries, so a launch boundary buys them only the compaction; with
        // many samples per pixel fewer, longer launches win: spp / 4 segments, at least 32, at most 512 (1 M-triangle scene, certified
        // walk, Msamples/s with 32 / 128 / 512 segments: an eighth of the frame at 2048 spp 1 787 / 1 895 / 1 943, at 256 spp 1 706 /
        // 1 801 / -; the whole frame at 512 spp 2 444 / 2 531 / 2 514 (256), at 64 spp 2 341 / 2 267 / -)
        if (w.phased && in.segments_per_launch <= 0) p.segments = std::min(512, std::max(32, in.spp / 4));
        // "the rest of the frame" for the 8-wide walks: at most 512 segments, then compaction - what a 64-spp frame has left at that
        // point anyway; with BASELINE's 2048 spp the pixels of a tile finish far apart, and re-packing the living ones every 512
        // segments beats one launch to the end (an eighth of the 1 M-triangle frame, 2048 spp: 1 943 against 1 824 Msamples/s)
        p.rest_segments = w.wide ? std::max(p.segments, 512) : kRestOfFrameSegments;
        // The sweep's cost per segment does not shrink with its living lanes, so its waves want the compaction of every 32nd
        // segment for longer: with the phased kernels' threshold c2 loses 7 %, c3 8 %; at 0.3 x the wave slots a small frame
        // gains (cbox 256^2 +14 %, 362^2 +15 %; 512^2 = 0.5 x the slots -11 % with one launch) and c2's last stretch +0.5 %.
        p.fit_pct = w.phased ? 120 : 30;
        // Refill (device_scene.h: LaunchSchedule): a launch of the 8-wide walks has at most as many waves as the device holds at once, and
        // a lane whose pixel has had its visit takes the next queued pixel - no wave waits for a slot, no lane idles while pixels are
        // queued, and the frame needs no launch boundary to re-pack its lanes before the queue has run dry
        // (the sweep of the small LDS-resident scenes does not gain: with refill its waves lose the coherence their shared walk lives on -
        // c2 5 685 Msamples/s in image order, 6 790 in cost order, against 6 717 for its 32-segment launches on the same box)
        p.refill = w.wide && in.segments_per_launch <= 0 && p.wave_slots > 0 && !in.nee && !in.over.refill_off;
        p.run_ahead = p.refill ? 1 : 2;              // (a refill launch takes the frame to its end: nothing to run ahead with)
        // launch order by last frame's cost: in 16 classes, and only while the frame has at most three pixels per lane of the
        // launch - an eighth of the 1 M-triangle frame (1.3 per lane) gains 9 % at 64 spp and 12 % at 2048 spp; the whole frame (10.7
        // per lane) has no tail to speak of and loses 6 % with its launch order torn from the image order (neighbouring waves share
        // the lines of the scene they fetch).  Classes 2 / 4 / 8 / 16 / 32 / 64 / 256 on the eighth at 64 spp: 1 681 / 1 685 / 1 879 / 1 897 /
        // 1 875 / 1 860 / 1 819 Msamples/s against 1 735 in image order.
        p.order_by_cost = in.n_local <= 3ll * 64 * p.wave_slots;
        if (in.over.order_set) { p.order_by_cost = in.over.order_on; if (in.over.order_value > 1) p.order_classes = in.over.order_value; }
        // With refill one launch keeps every wave slot busy by itself: a second chunk's kernel only competes with it (an eighth of the
        // 1 M-triangle frame 1 661 -> 1 716 Msamples/s with one chunk, the whole frame 2 600 -> 2 795; three chunks: 1 628 / 2 501).  The
        // automatic choice follows the walk; a forced count (config.streams) stays.
        if (!in.is_pass && !in.nee && in.want_chunks == 0) p.auto_chunks = p.refill ? 1 : (in.n_local >= (1ll << 18) ? 2 : 1);
        return p;
    }

    // the cost order is for ONE refill launch over the whole frame: one chunk, no batch
    bool costOrder(int n_chunks) const { return refill && n_chunks == 1 && n_frames == 1 && order_by_cost; }

    // ---- per launch; active: the pixels still in flight in all chunks, bound: those of the launch's own chunk ----
    static long long waves(long long pixels) { return (pixels + 63) / 64; }
    // the pixels still active fit the device (by fit_pct of its wave slots): the rest of the frame goes into this launch
    bool fits(long long active) const { return wave_slots > 0 && waves(active) * 100 <= wave_slots * fit_pct; }
    // more waves than bounce_resident_waves(): an 8-wave build where there is one
    bool manyWaves(long long active) const { return phased && wave_slots > 0 && waves(active) >= 2 * wave_slots; }
    // a refill launch's share of the device's wave slots, by its chunk's share of the pixels still in flight (rounded down: the
    // chunks together must not ask for more waves than fit at once, or the surplus starts a whole launch late); 0: no refill
    int maxWaves(long long active, long long bound) const {
        return refill && active > 0 ? std::max(4, (int)(wave_slots * bound / active) & ~3) : 0;
    }
    int launchSegments(long long active) const { return refill ? kRestOfFrameSegments : fits(active) ? rest_segments : segments; }
};

}  // namespace ptmi
