// render_run.cpp — one render run: a frame, a frame batch or an accumulation pass (renderFrame(s), accumPass), and selectFrame.
// How the run is cut into launches is launch_rule.h's decision; this file issues them.
#include "application_state.h"
#include "launch_rule.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace ptmi {

void renderFrame(ApplicationState& g, FrameStats* stats) { renderFrames(g, 1, stats); }

void selectFrame(ApplicationState& g, int frame) {
    RenderState& r = g.render;
    if (r.accum.pass > 0) throw ArgError("selectFrame: the image buffers hold an accumulation pass, not a frame batch");
    if (!r.d_state.A || r.batch_spp <= 0) throw ArgError("selectFrame: nothing rendered yet");
    if (frame < 0 || frame >= r.batch_frames) throw ArgError("selectFrame: frame index outside the last batch");
    PTMI_HIP(hipSetDevice(g.device_id));
    if (r.resolve_gate) PTMI_HIP(hipStreamWaitEvent(r.stream, r.resolve_gate, 0));
    const float4* src = frame == r.batch_frames - 1 ? nullptr : r.d_frame_color + (size_t)frame * r.n_local;
    launch_resolve(r.tile, r.d_state, r.batch_spp, r.d_image, r.d_radiance, r.stream, src);
    PTMI_HIP(hipGetLastError());
    if (r.download_image && r.n_local) PTMI_HIP(hipMemcpyAsync(r.h_image, r.d_image, r.n_local * 3, hipMemcpyDeviceToHost, r.stream));
    PTMI_HIP(hipStreamSynchronize(r.stream));
}

namespace {
using Chunk = RenderState::Chunk;
constexpr int kRing = RenderState::kCountRing;        // count slots: launch i reads (i-1) % kRing, writes i % kRing

// One accumulation pass through renderRun: its queue is r.accum.chunk (d_queue_init / n: the pixels still active)
struct PassRun { AdaptRule rule; int active_after = 0; };

// whatever way renderRun is left, nothing of this frame is still in flight (an exception thrown between two
// launches must not let the next frame start on top of the chunk streams' queued work)
struct Drain {
    RenderState& r; bool armed = true;
    ~Drain() {
        if (!armed) return;
        for (int c = 0; c < RenderState::kMaxChunks; c++) if (r.chunk[c].stream) (void)hipStreamSynchronize(r.chunk[c].stream);
        (void)hipStreamSynchronize(r.stream);
    }
};

// What the pieces of one run share.  A frame (pass == nullptr) or an accumulation pass: the same launch loop, a frame's
// launches exactly as they always were
struct Run {
    ApplicationState& g;
    RenderState& r;
    const DeviceScene& scene;                          // the scene as this run walks it (effectiveScene)
    const FrameParams& fp;
    int n_frames;
    PassRun* pass;
    bool timed;                                        // the caller wants FrameStats: every launch is bracketed by an event pair
    hipStream_t s;                                     // the frame's stream: begin, NEE launch, resolve, downloads
    Chunk* chunks = nullptr;                           // a pass runs its queue as one chunk on chunk 0's stream
    int n_chunks = 0;                                  // (NEE: none)
    // launch order by cost (prepareCostOrder): the first launch's queue, and where this frame's costs are written
    const int* first_queue = nullptr;
    unsigned int *cost_now = nullptr, *cost_max_now = nullptr;
    size_t n_ev = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> kernel_events = {};   // (e0, e1) around every bounce / NEE launch of a timed run
    uint64_t launches = 0, visits = 0;

    // the run's next event: from the context's pool, in the order asked for - none is created once the pool is warm
    hipEvent_t event() {
        if (n_ev == g.event_pool.size()) { hipEvent_t ev; PTMI_HIP(hipEventCreate(&ev)); g.event_pool.push_back(ev); }
        return g.event_pool[n_ev++];
    }
    hipEvent_t record(hipStream_t on) { const hipEvent_t ev = event(); PTMI_HIP(hipEventRecord(ev, on)); return ev; }
    hipEvent_t stamp(hipStream_t on) { return timed ? record(on) : nullptr; }     // one end of a kernel's event pair
    int queueLength() const { return pass ? chunks[0].n : (int)r.n_local; }       // the pixels this run renders
};

void checkBatch(const ApplicationState& g, int n_frames) {
    if (n_frames < 1 || n_frames > 256) throw ArgError("renderFrames: n_frames must be in [1, 256]");
    if (n_frames > 1 && g.config.spp >= (1 << 16)) throw ArgError("renderFrames: a batch needs spp < 65536");
    if (n_frames > 1 && (unsigned long long)(n_frames - 1) * g.render.n_local >= (1ull << 31))
        throw ArgError("renderFrames: (n_frames - 1) * local pixels must stay below 2^31");
    if (n_frames > 1 && g.config.current_integrator == IntegratorType::Radiosity)
        throw ArgError("renderFrames: the Radiosity integrator renders one frame per call");
}

// what a frame and a pass both need
void checkRenderable(const ApplicationState& g, const char* who) {
    if (!g.scene.d_nodes) throw ArgError(std::string(who) + ": no scene loaded");
    if (!g.render.d_state.A) throw ArgError(std::string(who) + ": buffers not allocated (call updateResolution first)");
    if (g.config.spp < 1 || g.config.spp >= (1 << 24)) throw ArgError("spp must be in [1, 2^24)");
    if (g.config.max_depth < 1 || g.config.max_depth > 255) throw ArgError("max_depth must be in [1, 255]");
}

// camera update, the config's fields and, for a batch, the buffer of the completed frames' colour sums
FrameParams frameParams(ApplicationState& g, int n_frames) {
    RenderState& r = g.render;
    FrameParams fp;
    cameraFrameParams(g, fp);
    fp.spp = g.config.spp; fp.max_depth = g.config.max_depth;
    fp.sampling_mode = (int)g.config.sampling_mode; fp.mis_bsdf_fraction = g.config.mis_bsdf_fraction;
    if (n_frames > 1) {
        if (r.frame_color_frames < (size_t)(n_frames - 1)) {
            if (r.d_frame_color) { (void)hipFree(r.d_frame_color); r.d_frame_color = nullptr; r.frame_color_frames = 0; }
            r.d_frame_color = (float4*)hipMallocSafe((size_t)(n_frames - 1) * std::max<size_t>(r.n_local, 1) * sizeof(float4), "d_frame_color");
            r.frame_color_frames = (size_t)(n_frames - 1);
        }
        fp.n_frames = n_frames; fp.sample_mask = 0xffffu; fp.frame_color = r.d_frame_color; fp.n_local = (int)r.n_local;
    }
    return fp;
}

// The scene as this run walks it: the loaded scene's choice, after the fast-tree and certified fallbacks
DeviceScene effectiveScene(ApplicationState& g) {
    // the opt-in fast tree: built at the first frame that asks for it; quad scenes keep the exact walk
    if (g.config.fast_tree && !g.scene.fastReady() && g.config.current_integrator == IntegratorType::PathTracing)
        g.scene.buildFast();
    DeviceScene scene = g.scene.d_scene;
    if (g.config.fast_tree && g.scene.fastReady()) scene.traversal = TRAVERSAL_WIDE;
    if (scene.traversal == TRAVERSAL_CERTIFIED && !scene.certified_ready()) scene.traversal = scene.gnodes ? TRAVERSAL_PACKED : TRAVERSAL_PHASED;
    return scene;
}

// The launch rule for this run (launch_rule.h); the occupancy query is made only where the rule has a use for the answer
LaunchRule planLaunches(const ApplicationState& g, const DeviceScene& scene, const FrameParams& fp, int n_frames, bool is_pass, bool nee,
                        const LaunchOverrides& over) {
    const int trav = scene.traversal;
    LaunchRuleInput in;
    in.walk.wide = trav == TRAVERSAL_WIDE || trav == TRAVERSAL_CERTIFIED;
    in.walk.phased = trav == TRAVERSAL_PHASED || trav == TRAVERSAL_PACKED || in.walk.wide;
    in.walk.sweep = trav == TRAVERSAL_SWEEP;
    in.segments_per_launch = g.config.segments_per_launch; in.spp = g.config.spp;
    in.n_local = (long long)g.render.n_local; in.n_frames = n_frames;
    in.nee = nee; in.is_pass = is_pass; in.want_chunks = g.render.want_chunks;
    if (LaunchRule::needsWaveSlots(in.walk, in.segments_per_launch)) in.wave_slots = bounce_resident_waves(scene, fp, g.config.collect_stats, g.n_cus);
    in.over = over;
    return LaunchRule::plan(in);
}

// The Radiosity integrator's frame (application.h:193-197): one launch, no queue.  Returns the event that ends the frame's time
hipEvent_t runRadiosityFrame(Run& run) {
    RenderState& r = run.r;
    if (r.resolve_gate) PTMI_HIP(hipStreamWaitEvent(run.s, r.resolve_gate, 0));
    launch_render_radiosity(run.g.scene.d_scene, r.tile, r.d_state, run.fp, r.d_image, r.d_radiance, run.s);
    PTMI_HIP(hipGetLastError());
    const hipEvent_t ev_done = run.record(run.s);
    if (r.download_image && r.n_local) PTMI_HIP(hipMemcpyAsync(r.h_image, r.d_image, r.n_local * 3, hipMemcpyDeviceToHost, run.s));
    PTMI_HIP(hipStreamSynchronize(run.s));
    return ev_done;
}

// Launch order of a refill frame: the pixels that took the most segments in the last frame first.  A pixel has ONE path in
// flight, so the heaviest pixels are as long as the frame whatever the GPU does meanwhile; started last - in image order the
// top rows of the tile are taken when the first background pixels are through - they end a background pixel's length after
// the rest.  The costs are the last frame's (same pixels, usually the same view); a first frame runs in image order.
void prepareCostOrder(Run& run, int order_classes) {
    RenderState& r = run.r;
    const int cur = (int)(r.cost_frame & 1), prev = cur ^ 1;
    if (r.cost_valid) {
        launch_order_by_cost(run.chunks[0].d_queue_init, run.chunks[0].n, r.d_cost[prev], r.d_cost_max + prev, r.d_cost_hist, r.d_queue_ordered, order_classes, run.s);
        run.first_queue = r.d_queue_ordered;
    }
    PTMI_HIP(hipMemsetAsync(r.d_cost[cur], 0, std::max<size_t>(r.n_local, 1) * sizeof(unsigned int), run.s));
    PTMI_HIP(hipMemsetAsync(r.d_cost_max + cur, 0, sizeof(unsigned int), run.s));
    run.cost_now = r.d_cost[cur]; run.cost_max_now = r.d_cost_max + cur;
    r.cost_valid = false;                              // until this frame is through
}

// the per-lane features' tables as they are now; blocks (route_rule.h): with the lens and the medium blocks, which throw before anything is launched
PerLaneTables perLaneTables(ApplicationState& g, bool blocks) {
    return {g.env.table(g.config.next_event, g.scene.d_emitters.n), g.scene.surfaceTable(), g.scene.vertexNormalTable(), g.scene.albedoTable(),
            g.scene.hasRough(), blocks ? lensDeviceBlock(g) : nullptr, blocks ? mediumDeviceBlock(g) : nullptr};
}

// the per-lane route (route_rule.h): ONE launch of ptmi_render_nee on the frame's stream; the whole frame, batch or pass
void runNeeLaunch(Run& run, const PerLaneTables& tables) {
    ApplicationState& g = run.g;
    const int n = run.queueLength();
    const hipEvent_t e0 = run.stamp(run.s);
    launch_render_nee(g.scene.d_scene, g.scene.d_emitters, tables, g.config.next_event, run.r.tile, run.r.d_state, run.fp,
                      run.pass ? run.chunks[0].d_queue_init : nullptr, n, run.pass ? run.pass->rule.first != 0 : true, run.s);
    PTMI_HIP(hipGetLastError());
    const hipEvent_t e1 = run.stamp(run.s);
    if (run.timed) run.kernel_events.push_back({e0, e1});
    run.launches = n > 0 ? 1 : 0; run.visits = (uint64_t)n;
}

// ---- a launch's output count: two ways for the host to learn it --------------------------------------------------------------
// Copy + event (the default): the host zeroes the launch's count slot, copies the count out behind the launch and waits for the
// event behind the copy.
// Count publishing (device_scene.h: CountPublish): the launch's last wave stores the output count to
// pinned host memory and zeroes the next counter, so a chunk's stream carries kernels only - no fill and no 4-byte copy
// between two launches (profiles/r02_kernel_stats_c5frame.csv: copyBuffer 11.2 % of the summed GPU time).  Built, parity
// green (100 GPU tests with it on), and measured SLOWER where it was meant to help: whole 1 M-triangle frame, exact walk
// 245.5 -> 262.0 ms, fast tree 120.5 -> 125.4 ms; an eighth of the frame +-0.  The blits' time is waiting
// time behind the other chunk's kernel, not GPU time the frame is short of.  Off by default; PTMI_PUBLISH=1 turns it on.

// before the launch that writes ring slot `slot`
CountPublish armCount(Chunk& ch, int slot, bool publish) {
    CountPublish pub;
    if (publish) {
        pub.done_count = ch.d_count + 4 * kRing; pub.next_count = ch.d_count + 4 * ((slot + 1) % kRing); pub.host_count = ch.d_hcount + slot;
        __atomic_store_n(ch.h_count + slot, -1, __ATOMIC_RELEASE);      // "not there yet"
    } else PTMI_HIP(hipMemsetAsync(ch.d_count + 4 * slot, 0, 4 * sizeof(int), ch.stream));     // output count, refill cursor, finished pixels
    return pub;
}
// behind that launch (count publishing: the kernel sends it itself)
void sendCount(Chunk& ch, int slot, bool publish, hipEvent_t done) {
    if (publish) return;
    PTMI_HIP(hipMemcpyAsync(ch.h_count + slot, ch.d_count + 4 * slot, sizeof(int), hipMemcpyDeviceToHost, ch.stream));
    PTMI_HIP(hipEventRecord(done, ch.stream));
}
int waitCount(Chunk& ch, int slot, bool publish, hipEvent_t done) {
    if (publish) {
        // the launch's last workgroup stores the count here; the stream is asked now and then so that a launch that
        // died (or never ran) surfaces as an error instead of an endless wait
        unsigned long long spins = 0;
        while (__atomic_load_n(ch.h_count + slot, __ATOMIC_ACQUIRE) < 0) {
            if ((++spins & 0xffffu) == 0) {
                const hipError_t q = hipStreamQuery(ch.stream);
                if (q != hipErrorNotReady && __atomic_load_n(ch.h_count + slot, __ATOMIC_ACQUIRE) < 0) {
                    if (q != hipSuccess) throw HipError(q, std::string("bounce launch failed: ") + hipGetErrorString(q));
                    throw HipError(hipErrorUnknown, "bounce launch finished without publishing its count");
                }
            }
            __builtin_ia32_pause();
        }
    } else PTMI_HIP(hipEventSynchronize(done));
    return ch.h_count[slot];
}

// one chunk's place in the queue loop
struct ChunkRun { int bound, last_out = 0, issued = 0, retired = 0; bool finished; hipEvent_t done[kRing]; };

// the next launch of chunk c: it advances each active pixel of the chunk by the rule's segments and compacts
void issueLaunch(Run& run, const LaunchRule& rule, bool publish, ChunkRun* runs, int c) {
    RenderState& r = run.r;
    ChunkRun& u = runs[c]; Chunk& ch = run.chunks[c];
    const int slot_out = u.issued % kRing;
    const CountPublish pub = armCount(ch, slot_out, publish);
    const hipEvent_t e0 = run.stamp(ch.stream);
    long long active = 0;                               // pixels still in flight, as far as the host has seen (counts only shrink)
    for (int k = 0; k < run.n_chunks; k++) active += runs[k].finished ? 0 : runs[k].bound;
    LaunchSchedule sched;
    sched.max_waves = rule.maxWaves(active, u.bound);
    if (sched.max_waves > 0) {                          // a refill launch
        sched.cursor = ch.d_count + 4 * slot_out + 1;
        sched.cost = run.cost_now; sched.cost_max = run.cost_max_now;
    }
    launch_bounce(run.scene, r.tile, r.d_state, run.fp, u.issued == 0 ? (run.first_queue ? run.first_queue : ch.d_queue_init) : ch.d_queue[(u.issued - 1) & 1], u.bound,
                  u.issued == 0 ? nullptr : ch.d_count + 4 * ((u.issued - 1) % kRing), ch.d_queue[u.issued & 1], ch.d_count + 4 * slot_out,
                  rule.launchSegments(active), run.g.config.collect_stats ? r.d_stats : nullptr, rule.manyWaves(active), ch.stream, pub, sched);
    PTMI_HIP(hipGetLastError());                       // launch-time failures (bad LDS size, ...) surface here, not a frame later
    const hipEvent_t e1 = run.stamp(ch.stream);
    if (run.timed) run.kernel_events.push_back({e0, e1});
    sendCount(ch, slot_out, publish, u.done[slot_out]);
    u.issued++;
}

// queue-driven loop: every launch advances each active pixel of its chunk by `segments` ray segments and compacts.
// A launch reads its exact input count from device memory (the previous launch's output counter), so the host
// does not wait for each count: per chunk it runs rule.run_ahead launches ahead, sizing grids with the newest count it
// HAS seen (counts only shrink), and stops once a count of 0 has come back; the launches already queued behind it
// find an empty queue and exit.  The chunks' streams run concurrently.
void runQueueLoop(Run& run, const LaunchRule& rule, bool publish, hipEvent_t ev_ready) {
    Chunk* chunks = run.chunks;
    const int n_chunks = run.n_chunks;
    ChunkRun runs[RenderState::kMaxChunks];
    for (int c = 0; c < n_chunks; c++) {
        runs[c].bound = chunks[c].n; runs[c].finished = chunks[c].n == 0;
        for (int i = 0; i < kRing; i++) runs[c].done[i] = run.event();
        PTMI_HIP(hipStreamWaitEvent(chunks[c].stream, ev_ready, 0));   // frame_begin (and the stats reset) precede every chunk's first launch
        if (publish) PTMI_HIP(hipMemsetAsync(chunks[c].d_count, 0, (4 * kRing + 1) * sizeof(int), chunks[c].stream));   // once per frame
    }
    auto busy = [&] { for (int c = 0; c < n_chunks; c++) if (!runs[c].finished || runs[c].retired < runs[c].issued) return true; return false; };
    while (busy()) {
        for (int c = 0; c < n_chunks; c++)
            while (!runs[c].finished && runs[c].issued - runs[c].retired < rule.run_ahead) issueLaunch(run, rule, publish, runs, c);
        for (int c = 0; c < n_chunks; c++) {         // retire each chunk's oldest outstanding launch: its count is the new bound
            ChunkRun& u = runs[c];
            if (u.retired == u.issued) continue;
            const int slot = u.retired % kRing;
            const int out_count = waitCount(chunks[c], slot, publish, u.done[slot]);
            run.launches++;                            // every issued launch counts (rocprof sees the trailing empty ones too)
            if (u.retired == 0 || u.last_out > 0) run.visits += (uint64_t)(u.retired == 0 ? chunks[c].n : u.last_out);
            u.last_out = out_count; u.bound = out_count;
            u.retired++;
            if (out_count == 0) u.finished = true;
        }
    }
    for (int c = 0; c < n_chunks; c++)               // the resolve pass waits for every chunk
        PTMI_HIP(hipStreamWaitEvent(run.s, run.record(chunks[c].stream), 0));
}

// The end of a path-tracing run: a pass's stopping test, resolve, downloads, the final synchronise and what the context
// remembers of the run.  Returns the event that ends the run's time
hipEvent_t finishRun(Run& run) {
    ApplicationState& g = run.g; RenderState& r = run.r; PassRun* pass = run.pass;
    const hipStream_t s = run.s;
    int active_after = 0;
    if (pass) {                                        // the stopping test: the next pass's queue and its length
        RenderState::Accum& a = r.accum;
        PTMI_HIP(hipMemsetAsync(a.d_out_count, 0, sizeof(int), s));
        launch_adapt(r.d_state, a.ab, pass->rule, run.chunks[0].d_queue_init, run.chunks[0].n, a.d_active[a.cur ^ 1], a.d_out_count, s);
        PTMI_HIP(hipGetLastError());
    }
#ifndef PTMI_EXPERIMENT_NO_RESOLVE_GATE      // (never defined in the shipped build: make ab-host-lib, to see the asynchronous-exchange test fail without it)
    if (r.resolve_gate) PTMI_HIP(hipStreamWaitEvent(s, r.resolve_gate, 0));   // a gather of the previous frame may still read the tile
#endif
    if (pass) launch_resolve_counts(r.tile, r.d_state, r.accum.ab.passes, g.config.spp, r.d_image, r.d_radiance, r.accum.d_counts, s);
    else launch_resolve(r.tile, r.d_state, g.config.spp, r.d_image, r.d_radiance, s);
    const hipEvent_t ev_end = run.record(s);
    if (pass) PTMI_HIP(hipMemcpyAsync(&active_after, r.accum.d_out_count, sizeof(int), hipMemcpyDeviceToHost, s));
    // cudaMemcpy(h_image, d_image, img_size, DeviceToHost), application.h:211 ("Memory Transfer" stage)
    if (r.download_image && r.n_local) PTMI_HIP(hipMemcpyAsync(r.h_image, r.d_image, r.n_local * 3, hipMemcpyDeviceToHost, s));
    PTMI_HIP(hipStreamSynchronize(s));                 // cudaDeviceSynchronize, application.h:199
    PTMI_HIP(hipGetLastError());
    if (pass) pass->active_after = active_after;       // (select_frame has nothing to resolve after a pass: batch_spp stays 0)
    else { r.batch_frames = run.n_frames; r.batch_spp = g.config.spp; }
    r.dn.image_current = true;
    r.dn.image_pass = pass != nullptr;
    if (run.cost_now) { r.cost_valid = true; r.cost_frame++; }
    return ev_end;
}

// the statistics of a path-tracing run (everything is through: the events have happened)
void runStats(const Run& run, hipEvent_t ev_begin, hipEvent_t ev_end, FrameStats* stats) {
    const ApplicationState& g = run.g;
    stats->seconds = elapsedMs(ev_begin, ev_end) * 1e-3;
    double kms = 0.0;
    for (const auto& e : run.kernel_events) kms += elapsedMs(e.first, e.second);
    stats->bounce_kernel_ms = kms;
    stats->bounce_launches = run.launches;
    stats->path_visits = run.visits;
    stats->samples = (uint64_t)run.queueLength() * (uint64_t)g.config.spp * (uint64_t)run.n_frames;
    if (g.config.collect_stats) {
        StatCounters c;
        PTMI_HIP(hipMemcpy(&c, run.r.d_stats, sizeof c, hipMemcpyDeviceToHost));
        stats->rays = c.rays; stats->node_visits = c.node_visits; stats->prim_tests = c.prim_tests; stats->hits = c.hits;
        stats->top_node_visits = c.top_node_visits; stats->cert_chain = c.cert_chain; stats->cert_fallback = c.cert_fallback;
    }
}

// check, plan (the launch rule), begin, one of three bodies (Radiosity, NEE, the queue loop), finish, statistics
void renderRun(ApplicationState& g, int n_frames, FrameStats* stats, PassRun* pass) {
    RenderState& r = g.render;
    checkBatch(g, n_frames);
    checkRenderable(g, "renderFrame");
    PTMI_HIP(hipSetDevice(g.device_id));
    const FrameParams fp = frameParams(g, n_frames);
    // what ptmi_select_frame may resolve: nothing until THIS path-tracing run has completed (a Radiosity frame or a run that
    // threw leaves the colour sums of some earlier run behind, and resolving those would overwrite a valid image)
    r.batch_frames = 1; r.batch_spp = 0;
    r.dn.image_current = false;                        // what ptmi_denoise may filter: likewise, only a completed path-tracing run

    const bool path_tracing = g.config.current_integrator == IntegratorType::PathTracing;
    const Route route = routeOf(presentFeatures(g, g.config.next_event), (int)g.config.current_integrator);
    const bool nee = route.per_lane;
    const PerLaneTables tables = perLaneTables(g, route.blocks);
    const DeviceScene scene = effectiveScene(g);
    const LaunchOverrides over = LaunchOverrides::fromEnv();
    const LaunchRule rule = planLaunches(g, scene, fp, n_frames, pass != nullptr, nee, over);
    Drain drain{r};
    if (path_tracing && rule.auto_chunks != 0 && rule.auto_chunks != r.n_chunks) { PTMI_HIP(hipStreamSynchronize(r.stream)); r.setupChunks(rule.auto_chunks); }
    if (pass) r.accum.chunk.stream = r.chunk[0].stream;
    Run run{g, r, scene, fp, n_frames, pass, stats != nullptr, r.stream};
    run.chunks = pass ? &r.accum.chunk : r.chunk;
    run.n_chunks = nee ? 0 : pass ? 1 : r.n_chunks;

    const hipEvent_t ev_begin = run.record(run.s);
    if (g.config.collect_stats) PTMI_HIP(hipMemsetAsync(r.d_stats, 0, sizeof(StatCounters), run.s));
    hipEvent_t ev_end;
    if (!path_tracing) ev_end = runRadiosityFrame(run);
    else {
        if (nee) {}                                    // the NEE kernel starts its own camera rays
        else if (pass) launch_pass_begin(r.tile, r.d_state, fp, run.chunks[0].d_queue_init, run.chunks[0].n, pass->rule.first != 0, run.s);
        else launch_frame_begin(r.tile, r.d_state, fp, run.s);
        if (rule.costOrder(run.n_chunks)) prepareCostOrder(run, rule.order_classes);
        const hipEvent_t ev_ready = run.record(run.s);
        if (nee) runNeeLaunch(run, tables);
        else runQueueLoop(run, rule, over.publish, ev_ready);
        ev_end = finishRun(run);
    }
    drain.armed = false;
    if (!stats) return;
    if (path_tracing) runStats(run, ev_begin, ev_end, stats);
    else {
        *stats = FrameStats();
        stats->seconds = elapsedMs(ev_begin, ev_end) * 1e-3;
        stats->samples = (uint64_t)r.n_local * (uint64_t)g.config.spp;
    }
}
}  // namespace

void renderFrames(ApplicationState& g, int n_frames, FrameStats* stats) {
    accumReset(g);                                     // a frame starts its sums from zero (ptmi_frame_begin)
    renderRun(g, n_frames, stats, nullptr);
}

// ------------------------------------------------------------------------------------------------
// progressive / adaptive accumulation (include/ptmi.h: ptmi_accum_pass)
// ------------------------------------------------------------------------------------------------
void accumReset(ApplicationState& g) {
    g.render.accum.pass = 0;
    g.render.accum.n_active = 0;
}

void accumPass(ApplicationState& g, const AdaptiveParams* params, PassStats* stats) {
    RenderState& r = g.render;
    RenderState::Accum& a = r.accum;
    if (g.config.current_integrator == IntegratorType::Radiosity) throw ArgError("accumPass: the Radiosity integrator has no accumulation passes");
    checkRenderable(g, "accumPass");
    if (params) {
        const AdaptiveParams& p = *params;
        if (p.min_passes < 2) throw ArgError("accumPass: min_passes must be >= 2");
        if (p.max_passes < p.min_passes || p.max_passes > 65536) throw ArgError("accumPass: max_passes must be in [min_passes, 65536]");
        if ((long long)p.max_passes * g.config.spp >= (1ll << 24)) throw ArgError("accumPass: max_passes * spp must stay below 2^24");
        if (!(p.threshold >= 0.0f) || !std::isfinite(p.threshold)) throw ArgError("accumPass: threshold must be finite and >= 0");
        if (!(p.floor > 0.0f) || !std::isfinite(p.floor)) throw ArgError("accumPass: floor must be finite and > 0");
        if (a.pass >= p.max_passes) throw ArgError("accumPass: the accumulation has reached max_passes (ptmi_accum_reset starts another)");
    }
    if (a.pass > 0 && a.n_active == 0) throw ArgError("accumPass: the accumulation is finished (ptmi_accum_reset starts another)");
    if ((long long)(a.pass + 1) * g.config.spp >= (1ll << 24)) throw ArgError("accumPass: a pixel's sample count must stay below 2^24");
    PTMI_HIP(hipSetDevice(g.device_id));
    const bool first = a.pass == 0;
    if (first) {
        if (!a.allocated()) r.allocateAccum();
        a.n_active = (int)r.n_local;
        a.cur = 0;
    }
    PassRun run;
    run.rule.first = first ? 1 : 0;
    run.rule.stopping = params ? 1 : 0;
    run.rule.min_passes = params ? params->min_passes : 0;
    run.rule.max_passes = params ? params->max_passes : 0;
    run.rule.threshold = params ? params->threshold : 0.0f;
    run.rule.floor_ = params ? params->floor : 0.0f;
    run.rule.inv_spp = rcp_rn((float)g.config.spp);
    a.chunk.d_queue_init = first ? nullptr : a.d_active[a.cur];       // pass 1: every local pixel (identity queue)
    a.chunk.n = a.n_active;
    const int before = a.n_active, k = a.pass + 1;
    FrameStats fs;
    a.pass = 0;                                        // until this pass is through: a pass that throws leaves no accumulation
    renderRun(g, 1, &fs, &run);
    a.pass = k;
    a.cur ^= 1;
    a.n_active = run.active_after;
    if (stats) {
        stats->pass = k;
        stats->active_before = (uint64_t)before; stats->active_after = (uint64_t)run.active_after;
        stats->frame = fs;
    }
}

void readSampleCounts(const ApplicationState& g, uint32_t* counts) {
    const RenderState& r = g.render;
    if (!r.d_state.A) throw ArgError("readSampleCounts: buffers not allocated");
    if (r.accum.pass == 0 || !r.accum.allocated()) { std::memset(counts, 0, r.n_local * sizeof(uint32_t)); return; }
    PTMI_HIP(hipSetDevice(g.device_id));
    PTMI_HIP(hipMemcpy(counts, r.accum.d_counts, r.n_local * sizeof(uint32_t), hipMemcpyDeviceToHost));
}

// ------------------------------------------------------------------------------------------------
// test hook: one stopping test plus resolve on given state (include/ptmi.h: ptmi_debug_accum_step)
// ------------------------------------------------------------------------------------------------
// What accumPass and finishRun do around a pass's render, without the render: the state by slot goes into the context's own
// buffers, then the launches of finishRun's pass half, in its order, on the frame's stream.  No kernel of its own.
int debugAccumStep(ApplicationState& g, const float* sums, const float* prev, const float* m2, const uint32_t* passes, const int* queue,
                   int n_queue, const AdaptiveParams* params, bool first, int* queue_out) {
    RenderState& r = g.render;
    RenderState::Accum& a = r.accum;
    if (g.config.current_integrator == IntegratorType::Radiosity) throw ArgError("debugAccumStep: the Radiosity integrator has no accumulation passes");
    checkRenderable(g, "debugAccumStep");
    const size_t n = r.n_local;
    if (n_queue < 0 || (size_t)n_queue > n) throw ArgError("debugAccumStep: the queue's length must be in [0, local pixels]");
    if (queue) {
        std::vector<char> seen(n, 0);
        for (int i = 0; i < n_queue; i++) {
            if (queue[i] < 0 || (size_t)queue[i] >= n) throw ArgError("debugAccumStep: a queue entry lies outside the local slots");
            if (seen[queue[i]]) throw ArgError("debugAccumStep: a slot is queued twice");
            seen[queue[i]] = 1;
        }
    }
    PTMI_HIP(hipSetDevice(g.device_id));
    if (!a.allocated()) r.allocateAccum();
    if (a.pass == 0) a.cur = 0;
    const int k = a.pass + 1;
    a.pass = 0;                                        // until the step is through, as in accumPass
    r.batch_frames = 1; r.batch_spp = 0;
    r.dn.image_current = false;
    AdaptRule rule;
    rule.first = first ? 1 : 0;
    rule.stopping = params ? 1 : 0;
    rule.min_passes = params ? params->min_passes : 0;
    rule.max_passes = params ? params->max_passes : 0;
    rule.threshold = params ? params->threshold : 0.0f;
    rule.floor_ = params ? params->floor : 0.0f;
    rule.inv_spp = rcp_rn((float)g.config.spp);
    std::vector<float4> h_D(n), h_prev(n);
    for (size_t i = 0; i < n; i++) {
        h_D[i] = make_float4(sums[3 * i], sums[3 * i + 1], sums[3 * i + 2], 0.0f);      // .w: the sample index, rewritten when a pass begins
        h_prev[i] = make_float4(prev[4 * i], prev[4 * i + 1], prev[4 * i + 2], prev[4 * i + 3]);
    }
    const hipStream_t s = r.stream;
    Drain drain{r};
    int n_out = 0;
    if (n) {
        PTMI_HIP(hipMemcpyAsync(r.d_state.D, h_D.data(), n * sizeof(float4), hipMemcpyHostToDevice, s));
        PTMI_HIP(hipMemcpyAsync(a.ab.prev, h_prev.data(), n * sizeof(float4), hipMemcpyHostToDevice, s));
        PTMI_HIP(hipMemcpyAsync(a.ab.m2, m2, n * sizeof(float), hipMemcpyHostToDevice, s));
        PTMI_HIP(hipMemcpyAsync(a.ab.passes, passes, n * sizeof(unsigned int), hipMemcpyHostToDevice, s));
    }
    if (queue && n_queue) PTMI_HIP(hipMemcpyAsync(a.d_active[a.cur], queue, (size_t)n_queue * sizeof(int), hipMemcpyHostToDevice, s));
    // the pass half of finishRun
    PTMI_HIP(hipMemsetAsync(a.d_out_count, 0, sizeof(int), s));
    launch_adapt(r.d_state, a.ab, rule, queue ? a.d_active[a.cur] : nullptr, n_queue, a.d_active[a.cur ^ 1], a.d_out_count, s);
    PTMI_HIP(hipGetLastError());
    if (r.resolve_gate) PTMI_HIP(hipStreamWaitEvent(s, r.resolve_gate, 0));
    launch_resolve_counts(r.tile, r.d_state, a.ab.passes, g.config.spp, r.d_image, r.d_radiance, a.d_counts, s);
    PTMI_HIP(hipGetLastError());
    PTMI_HIP(hipMemcpyAsync(&n_out, a.d_out_count, sizeof(int), hipMemcpyDeviceToHost, s));
    if (r.download_image && n) PTMI_HIP(hipMemcpyAsync(r.h_image, r.d_image, n * 3, hipMemcpyDeviceToHost, s));
    PTMI_HIP(hipStreamSynchronize(s));
    PTMI_HIP(hipGetLastError());
    if (n_out < 0 || n_out > n_queue) throw HipError(hipErrorUnknown, "debugAccumStep: the stopping test returned a count outside its queue");
    if (n_out) PTMI_HIP(hipMemcpy(queue_out, a.d_active[a.cur ^ 1], (size_t)n_out * sizeof(int), hipMemcpyDeviceToHost));
    drain.armed = false;
    r.dn.image_current = true;
    r.dn.image_pass = true;
    a.pass = k;
    a.cur ^= 1;
    a.n_active = n_out;
    return n_out;
}

}  // namespace ptmi
