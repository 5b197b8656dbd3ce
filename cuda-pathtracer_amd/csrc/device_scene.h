// device_scene.h — HBM/LDS data layout of the render path and the kernel launch API.
//
// Everything the kernels touch is an array of 16-byte vectors so that a wave
// reads/writes 1 KiB per instruction (global_load_dwordx4, ds_read_b128).
//
// SCENE (read-only, replicated on every GPU; staged into LDS when it fits)
//   nodes[2*i+0] = (bbox.min.xyz, bits(a))         a: inner -> SKIP index (first node after this subtree in pre-order),
//                                                     leaf  -> first primitive slot
//   nodes[2*i+1] = (bbox.max.xyz, bits(b))         b: inner -> right child (>0), leaf -> -prim_count (<0)
//   Nodes are numbered in pre-order (bvh.h:154-218), so an inner node's left child is always i+1 and the
//   reference's "push right, push left, pop" order (scene.h:101-105) is exactly "i+1 if the box is hit, else skip".
//   prims[S*k+0] = (v0.xyz, bits(type))            k = LEAF-ORDER slot (reference's bvh_indices applied on the host,
//   prims[S*k+1] = (v1-v0 | v10-v00, 0)              so a leaf's primitives are contiguous); S = 3 for triangle-only
//   prims[S*k+2] = (v2-v0 | v11-v00, 0)              scenes, 4 when quads are present.  Edges are precomputed with the
//   prims[S*k+3] = (      - | v01-v00, 0)            same float subtraction the reference performs per test.
//   mats[3*k+0]  = (normal.xyz, bits(load-order primitive index))
//   mats[3*k+1]  = (Kd.xyz, 0)
//   mats[3*k+2]  = (Ke.xyz, 0)
//
// PATH STATE (read+written once per launch per active pixel; slot = local pixel)
//   A[slot] = (ray.o.xyz, throughput.x)
//   B[slot] = (ray.d.xyz, throughput.y)
//   C[slot] = (L_sample.xyz, throughput.z)         L_sample = radiance of the sample in flight (integrator.h:204)
//   D[slot] = (color.xyz, bits(sample_idx << 8 | depth))   color = sum of finished samples (integrator.h:390)
//   E[slot] = xorwow v[0..3]                       RNG stream of the pixel: strictly sequential, which is why a
//   F[slot] = (xorwow v[4], weyl d)                pixel has exactly one path in flight
//   = 88 B per pixel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_vec.h"

namespace ptmi {

struct DeviceScene {
    const float4* nodes = nullptr;
    const float4* prims = nullptr;
    const float4* mats = nullptr;
    int n_nodes = 0, n_prims = 0;
    int prim_stride = 3;      // float4 per primitive
    int has_quads = 0;
    int stack_entries = 1;    // min(bvh depth + 1, 64); only the STACK traversal uses it
    int lds_resident = 0;     // 1: nodes+prims+mats are staged into LDS by every workgroup (LANE/STACK traversal)
    int traversal = 1;        // TraversalMode
    int sweep_leaves = 0;     // leaves of the tree where the sweep may test the leaf boxes alone (sweep_leaves.h: the verdict holds and the
                              // launch rule takes it); 0: it walks every node.  Stands in what was padding: no other field moves
    // Guided sampling (SamplingMode != BSDF): one PrecomputedCDF record per primitive in LOAD order
    // (render_config.h:24-31: pdf[256], row_sums[8], marginal_cdf[8], row_cdfs[256], total_weight, is_valid = 530
    // dwords = 2120 B), HBM/L2-resident, read per hit through the load-order index kept in mats[3k].w.  nullptr = none.
    const float* cdfs = nullptr;
    // Per-primitive radiosity (Triangle/Quad::radiosity, the radiosity solver's output in the reference): float4 per
    // LEAF-ORDER slot, read by ptmi_render_radiosity only.  nullptr = all zero (as after loading a scene).
    const float4* radiosity = nullptr;
    // TRAVERSAL_PACKED (scenes too large for LDS): the same tree in a cache-line-friendly order, see PACKED LAYOUT below.
    const float4* gnodes = nullptr;    // 2 float4 per record position
    int n_pos = 0;                     // record positions (incl. padding); a cursor >= n_pos ends the walk
    const float* gprims = nullptr;     // triangle-only scenes: 9 floats (v0, e1, e2) per leaf-order slot; nullptr: use prims
    const float4* gmats = nullptr;     // (normal.xyz, bits(row of mtab)) per leaf-order slot
    const float4* mtab = nullptr;      // distinct (Kd, Ke) pairs, 2 float4 per row
    const int* load_index = nullptr;   // leaf-order slot -> load-order primitive index (guided sampling reads cdfs through it)
    int n_top = 0, top_depth = 0;      // positions < n_top (the nodes of depth <= top_depth, level by level) are staged into LDS
    // TRAVERSAL_WIDE (opt-in fast tree, csrc/wide_bvh.h): 8-wide nodes of 128 bytes, breadth-first; per-triangle arrays in the
    // fast tree's own leaf order ("fast order")
    const uint4* wnodes = nullptr;     // 8 uint4 per node
    int w_nodes = 0, w_top = 0;        // nodes < w_top (whole levels) are staged into LDS by every workgroup
    int w_depth = 0;                   // entries of the walk's per-lane LDS stack = levels of the tree - 1
    const float* wprims = nullptr;     // 9 floats (v0, e1, e2) per fast-order triangle
    const float4* wmats = nullptr;     // (normal.xyz, bits(row of mtab)) per fast-order triangle
    const float4* wmtab = nullptr;     // distinct (Kd, Ke) pairs, 2 float4 per row
    const int* wload_index = nullptr;  // fast order -> load-order primitive index
    const int* wref_slot = nullptr;    // fast order -> reference leaf-order slot (equal-t hits keep the smaller one, scene.h:89-90)
    // TRAVERSAL_CERTIFIED: what the VERIFY phase and the fallback read (bounce_wide.hip: ptmi_bounce_wide, CERT)
    const uint4* wanc = nullptr;       // per reference leaf: its ancestors' pre-order node indices (leaf included), 4 per chunk, 0xffffffff pads
    const float4* wqprims = nullptr;   // scenes with quads: 64-byte records (v0 | type, e1, e2, e3) in the fast tree's order instead of wprims
    const float4* wcert = nullptr;     // kWideCertStride float4 per fast-order triangle, one 64-byte line per hit: (leaf box min, bits(first chunk << 5 |
                                       // chunks of the leaf's list)) (leaf box max, 0) (wmats' entry) (0)
    float w_big = 0.0f;                // the scene's scale (host/wide_bvh.h: WideBVH::scale); informational since the certificate takes eps from each box
    int w_cert_debug = 0;              // test hook of the solver's certified walk: 1 every blocked ray takes the ancestor chain, 2 the reference's walk
    const int* wfast_of_ref = nullptr; // reference leaf-order slot -> fast order
    float w_guard = 0.0f;              // the boxes are padded for ray origins with |coordinate| <= w_guard; others take the reference's walk
    // The certified walk can run on this scene.  SceneState::buildFast sets every w* pointer at once, after all its uploads:
    // wprims, wref_slot and (scenes with quads) wqprims with wnodes; wcert, wanc and wfast_of_ref together when the ancestor
    // lists fit; freeFast clears them all.
    PT_HD bool certified_ready() const { return wnodes && wcert && wanc; }
};
// PACKED LAYOUT.  On the 1 M-triangle scene the phased walk is bound by the rate at which L2 misses are served (it runs at
// the same speed with 2 and with 7 waves per SIMD, with and without half of its node reads moved to LDS): what counts is the
// number of distinct 128-byte lines a ray touches.  In pre-order a node's left child shares its line, its right child never
// does.  Here the two children of a node are ONE 64-byte pair, and pairs are laid out in pre-order of their parents, so a
// 128-byte line holds (L, R, LL, LR): the sibling that the walk comes back to after a subtree - or goes to at once when the
// left box is missed - arrived with the first fetch.  Measured on 1000 rays of that scene: 43 -> 28 distinct node lines per
// ray.  Links are explicit record positions (the tree and the visiting order are the reference's, scene.h:63-106):
//   inner  (min, bits(skip position)) (max, bits(left child position))      right child = left + 1; positions > 0
//   leaf   (min, bits(first slot << 3 | count)) (max, bits(~next position)) count <= 7; next = pre-order successor
//   position n_pos = "past the end".  Record 1 pads the root to a pair.
// Primitives of triangle-only scenes shrink from 48 to 36 bytes (three 12-byte loads) and the material record from 48 to 16
// bytes + a table of the distinct (Kd, Ke) pairs: fewer lines per leaf and per hit, and a smaller footprint in L2/MALL.
constexpr int kCdfDwords = 530, kCdfPdf = 0, kCdfRowSums = 256, kCdfMarginal = 264, kCdfRowCdfs = 272, kCdfTotal = 528, kCdfValid = 529;

// How ptmi_bounce walks the BVH.  All three visit the same nodes and primitives in the same order per ray.
enum TraversalMode {
    TRAVERSAL_SWEEP = 0,   // tiny scenes: the WAVE walks node indices 0..N-1 once, node/primitive data are wave-uniform
                           // scalar loads (SGPR operands), lanes whose own cursor equals the index take part
    TRAVERSAL_LANE = 1,    // general: every lane walks its own pre-order cursor (stackless, skip pointers)
    TRAVERSAL_STACK = 2,   // trees deeper than 62: explicit LDS stack with the reference's drop rule (scene.h:101-105)
    TRAVERSAL_PHASED = 3,  // large scenes: the stackless per-lane walk with wave-scheduled phases (ptmi_bounce_phased):
                           // lanes whose ray ends early shade and start their next segment instead of idling
    TRAVERSAL_PACKED = 4,  // scenes too large for LDS: PHASED over the packed layout (sibling pairs, 36-byte triangles)
    TRAVERSAL_WIDE = 5,    // opt-in (ptmi_config.fast_tree): PHASED over the 8-wide SAH tree of csrc/wide_bvh.h; the one walk
                           // that does NOT visit the reference's nodes - same triangles, same hit arithmetic, other boxes
    TRAVERSAL_CERTIFIED = 6,   // WIDE + a proof per ray that the reference's walk returns the same hit (slab tests of the hit
                           // leaf's ancestors in the reference's tree, tie detection), else the reference's walk for that ray: exact
};

struct PathState {
    float4* A = nullptr; float4* B = nullptr; float4* C = nullptr; float4* D = nullptr;
    uint4* E = nullptr; uint2* F = nullptr;
};

struct TileMap {              // local row -> global row (ptmi.h: ptmi_tiling)
    int width = 0, height = 0;
    int n_ranks = 1, rank = 0, row_block = 8;
    int local_rows = 0;
    int tile8 = 0;            // 1: consecutive slots enumerate 8x8 pixel tiles (needs width % 8 == 0 and local_rows % 8 == 0)
    // ptmi_size_reciprocal(width), (height) (shade_lean.h), both set or both 0: the pixel jitter's short division (shading.h:
    // div_by_size).  0: the IEEE division - a TileMap that nobody gave them, or a size above 2^23.
    float inv_width = 0.0f, inv_height = 0.0f;
};

struct FrameParams {
    float cam_origin[3], cam_llc[3], cam_hor[3], cam_ver[3];
    int spp, max_depth;
    int sampling_mode;          // SamplingMode (render_config.h:38-44)
    float mis_bsdf_fraction;    // Scene::mis_bsdf_fraction (scene.h:217)
    // Frame batches (renderFrames): n_frames successive frames of unchanged scene / camera / config rendered as ONE pipelined
    // run - a pixel that has finished frame k banks its colour sum in frame_color[k * n_local + slot] and starts frame k + 1 at
    // once (its RNG stream simply goes on, as between two renderFrame() calls), so the stragglers of frame k share the GPU with
    // the head of frame k + 1.  The frame index lives above the sample index: sample_idx = frame << 16 | sample (batches need
    // spp < 65536, n_frames <= 256); a single frame keeps all 24 bits for the sample index (sample_mask 0xffffff).
    int n_frames = 1;
    unsigned int sample_mask = 0xffffffu;
    float4* frame_color = nullptr;     // (n_frames - 1) * n_local colour sums of the completed frames; the last frame's stays in D
    int n_local = 0;
};

struct StatCounters { unsigned long long rays, node_visits, prim_tests, hits, top_node_visits, cert_chain, cert_fallback; };

constexpr int kBlock = 256;
constexpr int kXorwowJumpWords = 32 * 160 * 5;   // 32 matrices T^(2^67 * 2^k), 160 rows of 5 words

// ---- launchers (kernels.hip; the Radiosity view and NEE: first_hit.hip; the features: features.hip; the hooks: debug_hooks.hip) ------------------------------------------------
// render_init (integrator.h:274-280): seeds every local pixel's stream and clears its state.
void launch_render_init(const TileMap& tm, const PathState& st, const uint32_t* d_jump, uint64_t seed_base, hipStream_t s);
// First camera ray of the frame for every local pixel (sample 0 of the spp loop, integrator.h:383-387).
void launch_frame_begin(const TileMap& tm, const PathState& st, const FrameParams& fp, hipStream_t s);
// The hot kernel: advances every queued path by up to `segments` ray segments, regenerating camera rays when a
// sample ends; appends still-unfinished pixels to queue_out (wave ballot + prefix popcount, one atomic per wave).
// queue_in == nullptr means "all local pixels" (identity queue); n_in is then the pixel count.  count_in (device
// pointer, may be nullptr) holds the exact length of queue_in when the host only knows the upper bound n_in: the
// host can then enqueue launches ahead of the counts coming back.
int bounce_resident_waves(const DeviceScene& sc, const FrameParams& fp, bool stats, int n_cus);
// Count publishing: with host_count set, the last workgroup of the launch to finish stores the output count to *host_count
// (host-mapped pinned memory; the host polls it), zeroes *next_count (the next launch's counter) and *done_count (its own
// arrival counter): no fill or copy command between two launches of a chunk.  All three nullptr: the host resets and reads.
struct CountPublish { int* done_count = nullptr; int* next_count = nullptr; int* host_count = nullptr; };
// Scheduling of one launch; it does not change a result.  max_waves > 0 (with cursor: a device int the caller zeroed): the launch
// has at most max_waves waves, and a lane whose pixel has had its visit (all samples done, or `segments` segments in this launch)
// takes the next queue entry no lane has taken yet - one atomicAdd on *cursor per scheduling decision with ending lanes.  With
// max_waves = the waves the device holds at once, no wave of a launch waits for a slot and no lane idles while pixels are queued.
// (The 8-wide walks; other kernels ignore it.)
// cost / cost_max: per-pixel segment counts of this frame and their maximum (the walk adds to them at the end of every visit).
struct LaunchSchedule { int max_waves = 0; int* cursor = nullptr; unsigned int* cost = nullptr; unsigned int* cost_max = nullptr; };
// Launch order by cost: queue[0 .. n) = the entries of queue_in (nullptr: 0 .. n - 1) in `classes` (2 .. 256, a power of two)
// classes of descending cost[entry] (class width cost_max / classes); inside a class the entries keep their order up to the order in
// which the 256-entry workgroups of the pass reserve their ranges.  hist: 2 x 256 device ints of scratch.  The heaviest pixels of a
// frame are as long as the frame: started first, they end with it instead of after it.
void launch_order_by_cost(const int* queue_in, int n, const unsigned int* cost, const unsigned int* cost_max, int* hist, int* queue, int classes, hipStream_t s);
void launch_bounce(const DeviceScene& sc, const TileMap& tm, const PathState& st, const FrameParams& fp,
                   const int* queue_in, int n_in, const int* count_in, int* queue_out, int* count_out, int segments,
                   StatCounters* stats /* nullptr: counters compiled out */,
                   bool many_waves /* more waves than bounce_resident_waves(): an 8-wave build where there is one */, hipStream_t s,
                   const CountPublish& pub = CountPublish(), const LaunchSchedule& sched = LaunchSchedule());
// render_radiosity (integrator.h:460-504): the alternative "Radiosity" integrator of renderFrame (application.h:193-197):
// spp camera rays per pixel, first hit only, Le + per-primitive radiosity, sqrt gamma, 8-bit (+ float mean).
void launch_render_radiosity(const DeviceScene& sc, const TileMap& tm, const PathState& st, const FrameParams& fp,
                             unsigned char* rgb8, float* radiance, hipStream_t s);
// mean, Reinhard, gamma, 8-bit (integrator.h:393-407) + float radiance.  color_src: the per-slot colour sums to resolve
// (nullptr = the path state's D array, i.e. the frame just finished; else a slice of FrameParams::frame_color)
void launch_resolve(const TileMap& tm, const PathState& st, int spp, unsigned char* rgb8, float* radiance, hipStream_t s,
                    const float4* color_src = nullptr);

// ---- accumulation passes (include/ptmi.h: ptmi_accum_pass) -------------------------------------------------------------
// Per-pixel state of the stopping test, by slot, n_local each (RenderState::Accum allocates it at the first pass).
struct AccumBuffers {
    float4* prev = nullptr;          // S_{k-1}.xyz (the colour sum after the pixel's last pass), mean of the pass means
    float* m2 = nullptr;             // sum of squared deviations of the pass means (Welford)
    unsigned int* passes = nullptr;  // passes the pixel has taken in this accumulation
};
struct AdaptRule {
    int first;                       // 1: pass 1 (no state read)
    int stopping;                    // 0: plain progressive, no pixel stops
    int min_passes, max_passes;
    float threshold, floor_, inv_spp;
};
// ptmi_frame_begin for the n pixels of queue (nullptr: all local pixels): first camera ray of the pass, sample index 0, colour
// sum kept (first: zeroed)
void launch_pass_begin(const TileMap& tm, const PathState& st, const FrameParams& fp, const int* queue, int n, bool first, hipStream_t s);
// the stopping test of the n pixels of queue_in that took the pass; the ones that go on are appended to queue_out (*count_out,
// zeroed by the caller)
void launch_adapt(const PathState& st, const AccumBuffers& ab, const AdaptRule& rule, const int* queue_in, int n, int* queue_out,
                  int* count_out, hipStream_t s);
// launch_resolve with each pixel's own count passes[slot] * spp (all local pixels); counts: that count, local row-major
void launch_resolve_counts(const TileMap& tm, const PathState& st, const unsigned int* passes, int spp, unsigned char* rgb8,
                           float* radiance, unsigned int* counts, hipStream_t s);

// ---- feature buffers and the denoiser (include/ptmi.h: ptmi_render_features, ptmi_denoise) ---------------------------------
// Per local pixel, local row-major (the order of ptmi_read_image), the means over the g x g first hits of the feature pass.
struct FeatureBuffers {
    float4* albedo = nullptr;        // (Kd.xyz, hit fraction); Kd x the image's value where the shaded albedo is asked for
    float4* normal = nullptr;        // (stored primitive normal.xyz, 0); the interpolated normal where the shaded normal is asked for
    float4* position = nullptr;      // (hit point o + t d .xyz, 0)
};
// flags: PTMI_FEATURE_* (include/ptmi.h: "shaded features").  The SHADED instantiation runs only where a flag is set AND its
// table is present (at.rec for bit 0, vn.rec for bit 1); every other call launches the kernel as it was before the flags.
struct VertexNormalTable;
struct AlbedoTable;
void launch_features(const DeviceScene& sc, const TileMap& tm, const FrameParams& fp, int g, const FeatureBuffers& fb,
                     const VertexNormalTable& vn, const AlbedoTable& at, int flags, hipStream_t s);
// The constants of one run that the two a-trous filters share (csrc/denoise.hip; the contracts are written out in include/ptmi.h)
struct FilterArgs {
    int width, height;               // the whole frame (a single rank)
    int demodulate;                  // 1: filter radiance / albedo (per channel, where the albedo is not 0)
    int normal_squarings;
    float sigma_x2;                  // sigma_x * sigma_x (> 0)
};
struct DenoiseArgs : FilterArgs {
    float color_floor;
};
// iterations passes of the edge-avoiding a-trous filter over radiance (3 floats per pixel, local row-major) guided by fb; the
// filtered radiance -> out_radiance (3 floats per pixel) and its tone map -> out_rgb8.  buf: 2 x width x height float4 of scratch.
// sigma_c[i]: the colour sigma of iteration i.
void launch_denoise(const DenoiseArgs& a, const FeatureBuffers& fb, const float* radiance, int iterations, const float* sigma_c,
                    float4* buf, unsigned char* out_rgb8, float* out_radiance, hipStream_t s);

// The variance-guided filter's own constants (the estimate: csrc/denoise_variance.hip; the contract: include/ptmi.h, ptmi_denoise_variance)
struct VarianceArgs : FilterArgs {
    float sigma_l2;                  // sigma_luminance * sigma_luminance
    float epsilon;
    int radius;                      // of the spatial estimate's window, 1 .. 3
    unsigned int two_spp;            // 2 * config.spp: a pass image's pixel with this many samples has two pass means
};
// The variance estimate (moments != nullptr: the accumulation's statistics where a pixel has two passes or more - counts: its
// samples per pixel, local row-major - and the spatial estimate elsewhere; nullptr: spatial everywhere) -> var_in, then
// iterations passes of the variance-guided a-trous filter over radiance guided by fb; the filtered radiance -> out_radiance, its
// tone map -> out_rgb8, the filtered variance -> var_out.  buf: 2 x width x height float4 of scratch.  `estimated` is recorded
// between the estimate and the filter.
// temporal != nullptr (ptmi_denoise_temporal_variance): radiance and fb are the history's, moments and counts are nullptr, and the
// estimate is the third route - the history's luminance statistics where a pixel has kTemporalMinFrames frames or more (with
// temporal->source = 0), the spatial estimate elsewhere.
struct TemporalVariance {
    const float4* moments = nullptr; // (mu, s2, k, 0) of the history, local row-major
    unsigned int* mask = nullptr;    // width x height of scratch: 1 where the temporal estimate wrote the pixel, else 0
    int source = 0;                  // 1: the spatial estimate everywhere (moments and mask are not touched)
};
constexpr float kTemporalMinFrames = 4.0f;   // PTMI_TEMPORAL_MIN_FRAMES
void launch_denoise_variance(const VarianceArgs& a, const FeatureBuffers& fb, const float* radiance, const TileMap& tm,
                             const AccumBuffers* moments, const unsigned int* counts, int iterations, float4* buf, float* var_in,
                             float* var_out, unsigned char* out_rgb8, float* out_radiance, hipEvent_t estimated, hipStream_t s,
                             const TemporalVariance* temporal = nullptr);
// the stopping test's state by slot -> local row-major arrays of n_local each
void launch_pass_moments(const TileMap& tm, const AccumBuffers& ab, float* mean, float* m2, unsigned int* passes, hipStream_t s);

// ---- temporal accumulation with reprojection (include/ptmi.h: ptmi_temporal_accumulate) ------------------------------------
// The step's constants (csrc/temporal.hip; the contract is written out in include/ptmi.h)
struct TemporalArgs {
    int width, height;               // the whole frame (a single rank)
    int history;                     // 0: the history is empty (every pixel restarts)
    int still;                       // 1: camera frame and resolution bit-identical to the history's
    float cam[12];                   // the history's camera frame: origin, lower-left corner, horizontal, vertical
    float origin[3];                 // the current camera's origin
    float m;                         // the input's samples per pixel where there are no per-pixel counts (config.spp)
    float max_history;               // (float)max_history
    float normal_min;
    float sigma_x2;                  // sigma_x * sigma_x
    float sigma_a2;                  // sigma_albedo * sigma_albedo
};
// One side of the history's ping-pong, local row-major
struct TemporalHistory {
    float4* color = nullptr;         // (colour.xyz, sample count)
    float4* normal = nullptr;        // (the feature normal .xyz, hit fraction) of the history's view
    float4* position = nullptr;      // (the feature position .xyz, 0) of the history's view
    float4* albedo = nullptr;        // (the feature albedo .xyz, hit fraction) of the history's view
};
// One step: the current radiance (3 floats per pixel) with its sample counts (counts, or a.m everywhere where counts ==
// nullptr) and features fb over the history prev -> next; the result -> out_radiance and its tone map
// -> rgb8; accepted / rejected / missed pixels are added to stats[0..2].  next_moments != nullptr (ptmi_set_temporal_moments):
// the luminance statistics (mu, s2, k, 0) per pixel travel with the history, prev_moments -> next_moments (both sides of a
// ping-pong of their own, so that TemporalHistory and the plain kernel's argument block stay what they were).
void launch_temporal(const TemporalArgs& a, const FeatureBuffers& fb, const float* radiance, const unsigned int* counts,
                     const TemporalHistory& prev, const TemporalHistory& next, unsigned char* rgb8,
                     float* out_radiance, unsigned long long* stats, hipStream_t s, const float4* prev_moments = nullptr,
                     float4* next_moments = nullptr);

// ---- next-event estimation (include/ptmi.h: ptmi_config.next_event) ------------------------------------------------------
// The emitter table of the loaded scene (host: SceneState::buildEmitters / upload; include/ptmi.h states which primitives are
// emitters and how cdf and pdf_area are made), in load order; nothing is sized for a handful of lights (the 1 M-triangle scene
// has 65 536).  Kept apart from DeviceScene so that no other kernel's arguments change.
//   cdf[j]                   running sum of w over emitters 0..j (binary search of u * total)
//   rec[kEmitterStride*j+0]  (v0.xyz, bits(leaf-order slot))     the slot: a shadow ray is visible iff its closest hit is it
//   rec[kEmitterStride*j+1]  (v1.xyz, quad area ratio)          Primitive::sampleAreaRatio (1 for triangles)
//   rec[kEmitterStride*j+2]  (v2.xyz, bits(type))
//   rec[kEmitterStride*j+3]  (v3.xyz, pdf_area)                 v3: quads only
//   rec[kEmitterStride*j+4]  (geometric normal.xyz, 0)
//   rec[kEmitterStride*j+5]  (Le.xyz, 0)
//   pdf_area[k]              per LEAF-ORDER slot: (geometric normal.xyz, pdf_area) of an emitter, 0 for every other primitive
constexpr int kEmitterStride = 6;
struct EmitterTable {
    const float* cdf = nullptr;
    const float4* rec = nullptr;
    const float4* pdf_area = nullptr;  // n_prims entries, also without emitters
    int n = 0;
    float total = 0.0f;
};
// The NEE frame / pass: one lane per queued pixel (queue nullptr: all local pixels, n of them) runs fp.n_frames x spp samples
// of the estimator of include/ptmi.h to their end; frame k < n_frames - 1 is banked in fp.frame_color, the last colour sum
// stays in D.  first: the sums start from zero (a frame, pass 1), else they go on from D (later passes).
// ---- environment lighting (include/ptmi.h: ptmi_set_environment) ----------------------------------------------------------
// The sampling table of the context's lat-long map (host/environment.cpp builds it, RenderState::Env owns the device copy).
// All of it stays in global memory: a vertex makes at most two binary searches and one texel read against a whole BVH walk,
// and first_hit_walk fixes the scene's LDS size.  texel == nullptr: no environment.
//   z[r]                 h + 1 row boundaries in cos(theta), z[0] = 1 ... z[h] = -1; row r covers z[r + 1] < d.y <= z[r]
//   marginal[r]          float CDF over the rows (ends at exactly 1; all zero for a map of total 0)
//   row_cdf[r * w + j]   float CDF over the columns of row r (all zero for a row of weight 0)
//   texel[r * w + j]     (scaled radiance.xyz, pdf per solid angle of the two searches picking this texel)
struct EnvTable {
    const float* z = nullptr;
    const float* marginal = nullptr;
    const float* row_cdf = nullptr;
    const float4* texel = nullptr;
    int w = 0, h = 0;
    float rot = 0.0f;                  // rotation_deg / 360.0f: the turn of column 0 from +x towards +z
    float q = 0.0f;                    // the EFFECTIVE probability that a vertex's light sample goes to the environment
    int sampled = 0;                   // next_event and total > 0: a vertex draws five numbers and selects by q
};
// ---- specular surfaces (include/ptmi.h: ptmi_set_surfaces) -----------------------------------------------------------------
// One record per LEAF-ORDER slot, the order of mats and EmitterTable::pdf_area (SceneState::setSurfaces permutes the caller's
// load-order table): (bits(kind), param), kind PTMI_SURFACE_*, param the ior of glass and the alpha of rough metal.  An array of its own: the bounce kernels stage mats into LDS and
// the packed layouts copy it, and none of them may change.  rec == nullptr: every surface is diffuse (no table, or all kinds 0).
struct SurfaceTable {
    const float2* rec = nullptr;
};
// ---- vertex normals (include/ptmi.h: ptmi_set_vertex_normals) ---------------------------------------------------------------
// S = DeviceScene::prim_stride float4 per LEAF-ORDER slot, the order of prims (SceneState::setVertexNormals permutes the caller's
// load-order table): rec[S * k + c] = (corner c's normal.xyz, c == 0 ? bits(1 smooth | 0 flat) : 0), corners in the order of the
// primitive's vertices; a triangle's 4th entry in a scene with quads is zero.  An array of its own, as SurfaceTable is and for the
// same reason.  rec == nullptr: every primitive is flat (no table, or a table without a smooth primitive).
struct VertexNormalTable {
    const float4* rec = nullptr;
};
// ---- albedo texture (include/ptmi.h: ptmi_set_albedo_texture) ---------------------------------------------------------------
// rec: TWO float4 per LEAF-ORDER slot, the order of prims (SceneState::setAlbedoTexture permutes the caller's load-order table),
// whatever prim_stride is: rec[2 * k] = (u0, v0, u1, v1), rec[2 * k + 1] = (u2, v2, u3, v3), corners in the order of the
// primitive's vertices; a triangle's (u3, v3) is zero.  An UNTEXTURED slot holds a quiet NaN in rec[2 * k].x (and zeros after it):
// a textured primitive's UVs are checked finite, so the first 16-byte read decides and the second is made for a textured slot only.
// texel: height x width float4 (rgb, 0), row-major, row 0 first.  filter: 0 nearest, 1 bilinear.  An array pair of its own, as
// SurfaceTable and VertexNormalTable are and for the same reason.  rec == nullptr: no primitive is textured (no table, or a table
// without a textured primitive).
struct AlbedoTable {
    const float4* rec = nullptr;
    const float4* texel = nullptr;
    int width = 0, height = 0, filter = 0;
};
// What the per-lane features (host/route_rule.h) hand the per-lane kernel; an absent table or block selects the instantiation without its code
struct PerLaneTables {
    EnvTable env; SurfaceTable surf; VertexNormalTable vn; AlbedoTable at;
    bool rough = false;                // surf holds a rough-metal record (SURF = 2; else the delta kinds' SURF = 1, which never reads a kind 3)
    const float4 *lens = nullptr, *medium = nullptr;   // the thin lens's block (host/lens.cpp) and the medium's (host/medium.cpp); nullptr: the pinhole, vacuum
};
// fp.n_frames x spp samples per queued pixel.  t.env.texel == nullptr, t.surf.rec == nullptr, t.vn.rec == nullptr and t.at.rec == nullptr:
// the NEE kernel exactly as it was; that instantiation IGNORES next_event (the host routes a frame here only when it is set, and
// the switch folds to true).  Else the ENV, SPEC, SMOOTH and / or TEX instantiation, which reads next_event and runs either estimator.
void launch_render_nee(const DeviceScene& sc, const EmitterTable& em, const PerLaneTables& t, bool next_event, const TileMap& tm, const PathState& st,
                       const FrameParams& fp, const int* queue, int n, bool first, hipStream_t s);

size_t bounce_lds_bytes(const DeviceScene& sc);
size_t bounce_lds_bytes_wide(const DeviceScene& sc);      // dynamic LDS of the 8-wide walks for this scene (top of the tree + stacks)

// ---- radiosity pre-pass (radiosity.hip, form_factors.hip) ----------------------------------------------------------------
// Load-order geometry the form-factor kernels sample (the traversal keeps using the leaf-order prims above):
//   geo[6*p+0] = (v0 | v00, bits(type))      geo[6*p+3] = (-  | v01, 0)
//   geo[6*p+1] = (v1 | v10, area)            geo[6*p+4] = (normal, 0)
//   geo[6*p+2] = (v2 | v11, area_ratio)      geo[6*p+5] = (centroid, 0)
// area / area_ratio / centroid are computed on the host with the float expressions of triangle.h:28, quad.h:31 and
// primitive.h:92-98, 161-170 (pure functions of the vertices).
constexpr int kGridRes = 16, kGridSize = 256;
struct RadiosityBuffers {
    const float4* geo = nullptr;
    const int* slot_of = nullptr;      // load-order index -> leaf-order slot (to skip source/target in the visibility test)
    const float4* bsdf = nullptr;      // (bsdf.xyz, 0), load order
    float4* radiosity = nullptr;       // (rgb, 0), load order
    float4* unshot[2] = {nullptr, nullptr};   // Jacobi double buffer
    float* form_factors = nullptr;     // n * n, row i = receiver
    unsigned int* grid = nullptr;      // n * 256 visible-sample counts (Triangle/Quad::grid; integers, so exact in any order)
    float4* rad_grid = nullptr;        // n * 256 (rgb, 0)  (Triangle/Quad::radiosity_grid)
    unsigned long long* rays = nullptr;   // shadow rays cast (1 counter)
    uint32_t* row_jump = nullptr;      // Monte-Carlo form factors: per receiver i the GF(2) matrix T^(2^67 * (i * n)) (160 rows x 5 words), the part
                                       // of a pair's XORWOW skip-ahead that all pairs of row i share (ptmi_ff_row_jumps); nullptr: not used
    int n = 0;
    int bvh_depth = 0;                 // > 30: the visibility walk keeps the reference's explicit stack and drop rule
    int fast_tree = 0;                 // the visibility walk: 0 the reference's, 1 DeviceScene's fast tree (opt-in), 2 the certified walk
};
struct RadiosityParams {
    int num_iterations, mc_samples, use_monte_carlo, enable_filtering, use_bilateral;
    float filter_sigma_spatial, filter_sigma_range;
};
// calculate_form_factors_mc_kernel / calculate_form_factors_kernel (form_factors.h:219-415) incl. formfactor_rand_init
// (:85-89, fused: a pair's XORWOW stream is derived where it is used) and initialize_directional_grids (:71-83)
void launch_form_factors(const DeviceScene& sc, const RadiosityBuffers& rb, const RadiosityParams& prm, const uint32_t* d_jump, hipStream_t s);
// radiosity_iteration_kernel (form_factors.h:441-465), Jacobi: reads unshot[src], writes unshot[1 - src]
void launch_radiosity_iteration(const RadiosityBuffers& rb, int src, hipStream_t s);
// update_radiosity_grid (form_factors.h:405-439) + the optional filter (grid_filter.h:103-165, 251-312)
void launch_radiosity_grid(const RadiosityBuffers& rb, const RadiosityParams& prm, hipStream_t s);
// precomputeCDFs / precomputeCDFsFromFiltered (application_state.h:492-585, 587-680) on the device: n records of kCdfDwords
// floats from (src_kind 0) float4 radiosity grids, (1) packed float3 grids, (2) pdf values, n * 256 entries each
void launch_cdf_records(int n, const void* d_src, int src_kind, float* d_out, hipStream_t s);
// filter_pdfs_for_primitives (grid_filter.h:420-507): d_rgb n*256*3 radiosity grids, d_counts n*256 count grids (or nullptr
// = zero); outputs n*256 filtered + per-primitive normalised pdfs
void launch_filter_pdfs(int n, const float* d_rgb, const float* d_counts, float* d_out_formfactor, float* d_out_radiosity,
                        bool bilateral, float sigma_spatial, float sigma_range, hipStream_t s);

// test hooks
void launch_debug_intersect(const DeviceScene& sc, int n, const float* o, const float* d, float t_min, float t_max,
                            int* hit, int* prim, float* t, float* p, float* nrm, hipStream_t s);
void launch_debug_intersect_wide(const DeviceScene& sc, int n, const float* o, const float* d, float t_min, float t_max,
                                 int* hit, int* prim, float* t, unsigned long long* counts /* 2, may be nullptr */, hipStream_t s);
void launch_debug_first_hit(const DeviceScene& sc, int n, const float* o, const float* d, float t_min, int* hit, int* prim, float* t, hipStream_t s);
void launch_debug_rng(const uint32_t* d_jump, uint64_t seed_base, int n_pixels, const int* pixels, int count, float* out, hipStream_t s);
void launch_debug_rcp(unsigned int first_bits, unsigned long long count, unsigned long long* d_out, hipStream_t s);
void launch_debug_sqrt(unsigned int first_bits, unsigned long long count, unsigned long long* d_out, hipStream_t s);
void launch_debug_ray_inv(int n, const float* d, const int* live, float* out, hipStream_t s);
// the shade step's short forms (debug_hooks.hip); d_out of the sincos check: 13 words, [2] preset to ~0, the rest to 0
void launch_debug_sincos_lean_check(unsigned int first_bits, unsigned long long count, unsigned long long* d_out, hipStream_t s);
void launch_debug_sincos_lean(int n, const float* x, const int* live, float* out /* 4n */, hipStream_t s);
void launch_debug_size_div(float W, float inv, unsigned int first_bits, unsigned long long count, unsigned long long* d_out, hipStream_t s);
void launch_debug_unit_voted(int n, const float* w, const int* live, float* out /* 6n */, hipStream_t s);
void launch_debug_cosine(int n, const float* normals, const float* u, const float* v, float* out, hipStream_t s);
void launch_debug_guided(int n, int op, const float* recs, const int* rec_idx, const float* normals, const float* in3,
                         const uint32_t* states, float* out, int* used, hipStream_t s);
void launch_debug_math(int n, int op, const float* a, const float* b, double* out /* 2n */, hipStream_t s);
void launch_debug_grid_index(int n, const float* dirs, const float* normals, int* out, hipStream_t s);
// ptmi_debug_nee_call (include/ptmi.h): floats in and out and ints out per case
constexpr int kNeeCallIn = 16, kNeeCallOutF = 16, kNeeCallOutI = 4;
void launch_debug_nee_call(bool has_quads, int n, int op, const EmitterTable& em, const EnvTable& ev, const float* in /* n * kNeeCallIn */,
                           float* out_f /* n * kNeeCallOutF */, int* out_i /* n * kNeeCallOutI */, hipStream_t s);
// ptmi_debug_vertex_normal (include/ptmi.h): vertex_normal (vertex_normal.h) of leaf-order slot slots[i] at p[3i ..] -> out[4i ..]
void launch_debug_vertex_normal(const DeviceScene& sc, const VertexNormalTable& vn, int n, const int* slots, const float* p, float* out /* 4n */,
                                hipStream_t s);
// ptmi_debug_albedo (include/ptmi.h): albedo_at (albedo_texture.h) of leaf-order slot slots[i] at p[3i ..] -> out[6i ..]
void launch_debug_albedo(const DeviceScene& sc, const AlbedoTable& at, int n, const int* slots, const float* p, float* out /* 6n */, hipStream_t s);
// ptmi_debug_lens_ray (include/ptmi.h): lens_ray_at (lens.h) over the block `lens` for pixel (px[i], py[i]) and the uniforms
// r[4i ..] = r3 r4 r1 r2 -> out[6i ..] = o, d
void launch_debug_lens_ray(const float4* lens, int n, const int* px, const int* py, const float* r, float* out /* 6n */, hipStream_t s);
// ptmi_debug_medium_call (include/ptmi.h): the functions of medium.h over the block each case carries
constexpr int kMediumCallIn = 20, kMediumCallOut = 8;
void launch_debug_medium_call(int n, int op, const float* in /* n * kMediumCallIn, 16-byte aligned */, float* out /* n * kMediumCallOut */, hipStream_t s);

}  // namespace ptmi
