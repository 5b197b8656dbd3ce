// application_state.h — host-side mirror of the reference's state objects for the render path
// (include/application_state.h: RenderState :77-130, SceneState :136-256/367-490, AppConfig :262-293,
//  ApplicationState :299-308; renderFrame: include/application.h:157-216).
//
// Differences by design: no global g_state (a ptmi_ctx owns one ApplicationState per GPU), no GL/ImGui,
// no radiosity/grid-guiding members, device memory is SoA (csrc/device_scene.h) instead of the 4364-byte
// Primitive records, and the render loop is a queue-driven sequence of ptmi_bounce launches instead of
// one thread-per-pixel megakernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../csrc/device_scene.h"
#include "bvh.h"
#include "environment.h"
#include "surfaces.h"
#include "vertex_normals.h"
#include "albedo_texture.h"
#include "lens.h"
#include "medium.h"
#include "file_manager.h"
#include "pbrt_loader.h"
#include "route_rule.h"
#include "sensor.h"
#include "wide_bvh.h"

namespace ptmi {

struct HipError : std::runtime_error {
    hipError_t code;
    HipError(hipError_t c, const std::string& what) : std::runtime_error(what), code(c) {}
};
struct IoError : std::runtime_error { using std::runtime_error::runtime_error; };
struct ArgError : std::runtime_error { using std::runtime_error::runtime_error; };
struct DistError : std::runtime_error { using std::runtime_error::runtime_error; };   // RCCL missing or an nccl* call failed

// a HIP call that throws HipError on failure
#define PTMI_HIP(call)                                                                                   \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) throw HipError(e_, std::string(#call) + ": " + hipGetErrorString(e_));     \
    } while (0)

inline float elapsedMs(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    PTMI_HIP(hipEventElapsedTime(&ms, a, b));
    return ms;
}

// cudaMallocSafe (utils/cuda_utils.h:54-60): throws on failure
void* hipMallocSafe(size_t bytes, const char* name);

enum class IntegratorType { PathTracing = 0, Radiosity = 1 };                       // application_state.h:50-53
enum class SamplingMode { SAMPLING_BSDF = 0, SAMPLING_FORMFACTOR = 1, SAMPLING_RADIOSITY = 2, SAMPLING_MIS = 3, SAMPLING_TOPK = 4 };   // render_config.h:38-44

struct AppConfig {                                   // application_state.h:262-293 (path-relevant members)
    int spp = 1;
    int max_depth = 5;                               // literal 5 in integrator.h:389
    SamplingMode sampling_mode = SamplingMode::SAMPLING_BSDF;
    uint64_t seed_base = 2023;                       // integrator.h:279
    f3 camera_origin = {0.5f, 3.0f, 8.5f}, look_at = {0.0f, 2.5f, 0.0f}, up = {0.0f, 1.0f, 0.0f};
    float fov = 40.0f;
    bool convert_quads_to_triangles = false;
    bool orbit = true;                               // renderFrame() always calls updateCameraOrbit()
    int segments_per_launch = 0;                     // 0 = default
    bool collect_stats = false;
    float mis_bsdf_fraction = 0.5f;                  // application_state.h:292 / scene.h:217
    IntegratorType current_integrator = IntegratorType::PathTracing;   // application_state.h:283
    bool fast_tree = false;                          // new: walk the opt-in 8-wide SAH tree instead of the reference's (csrc/wide_bvh.h)
    bool next_event = false;                         // new: next-event estimation with MIS (include/ptmi.h: ptmi_config.next_event)
};

// The participating medium of a scene (include/ptmi.h: "participating medium"): the caller's numbers and the device copy of the
// block (host/medium.cpp).  sigma_t 0 is no medium.
struct MediumState {
    Medium m;
    float4* d_block = nullptr;                       // three float4, allocated by the first run that needs them
    float h_block[kMediumBlockFloats] = {};          // what d_block holds
    bool uploaded = false;
    bool on() const { return m.sigma_t > 0.0f; }
    void drop() { m = Medium(); }
    ~MediumState();
};

struct SceneState {
    std::vector<Primitive> h_primitives;             // load order
    std::vector<BVHNode> bvh_nodes;                  // pre-order
    std::vector<int> bvh_indices;                    // leaf order -> load order
    int bvh_depth = 0;
    int num_tris = 0, num_quads = 0;
    std::string scene_file;
    // Quad::intersect rejects a NaN u or v, the device's running minimum ignores one (csrc/pt_device.h); a NaN there needs an
    // overflowing product of a quad edge and o - v0 ("the quad test at the extent check").  upload() refuses a
    // scene with quads whose largest quad edge times the largest |o - v0| a path can reach exceeds kQuadReachBound, and every
    // origin that comes from outside the scene - the camera, a test hook's rays - is held to the same bound (checkQuadOrigin).
    // The camera is a pinhole: every camera ray starts AT the camera's origin, which is what a frame checks.  A camera whose rays start
    // elsewhere (a lens) has to hand checkQuadOrigin the farthest such point.
    static constexpr double kQuadReachBound = 0x1p124;
    float quad_edge_max = 0.0f;                      // largest |component| of a quad's v[k] - v[0]; 0 without quads
    float coord_lo[3] = {0, 0, 0}, coord_hi[3] = {0, 0, 0};      // bounds of every vertex of the scene
    void checkExtent();                              // the device's limits on a scene (edges, coordinates, the bound above); throws ArgError
    double quadReach(const float* o) const;          // largest |o_a - x_a| over the scene's points x, with the rounding of a hit point
    void checkQuadOrigin(const float* o, const float* d, const char* who) const;     // throws ArgError; non-finite rays pass (no primitive accepts them)

    float4 *d_nodes = nullptr, *d_prims = nullptr, *d_mats = nullptr;
    // packed layout for TRAVERSAL_PACKED (csrc/device_scene.h), built for scenes of at least packed_min_nodes nodes
    float4 *d_gnodes = nullptr, *d_gmats = nullptr, *d_mtab = nullptr;
    float* d_gprims = nullptr;
    int* d_load_index = nullptr;
    int packed_min_nodes = 8192;
    int packed_top_records = 512;                    // record positions of the packed layout kept in LDS (32 B each: 16 KB,
                                                     // 7 waves per SIMD stay resident); < 2: none
    // opt-in fast tree for TRAVERSAL_WIDE (csrc/wide_bvh.h), built at the first frame that asks for it (AppConfig::fast_tree)
    WideBVH h_wide;
    WideBVHParams wide_params;
    bool certified_default = true;                   // scenes above the sweep's 64 primitives (triangles and quads) walk CERTIFIED by default
    bool fast_declined = false;                      // the last buildFast() failed: the automatic choices do not ask again for this scene
    static constexpr int kWideMaxLevels = 24;        // deepest 8-wide tree the walk's LDS stack takes (buildFast)
    int wide_top_nodes = 80;                         // whole levels of the fast tree kept in LDS while they fit this many nodes (128 B each)
    uint4* d_wnodes = nullptr;
    float* d_wprims = nullptr;
    float4 *d_wmats = nullptr, *d_wmtab = nullptr;
    int *d_wload_index = nullptr, *d_wref_slot = nullptr;
    uint4* d_wanc = nullptr;                         // TRAVERSAL_CERTIFIED: ancestor lists of the reference's leaves, see buildFast
    float4* d_wcert = nullptr;
    float4* d_wqprims = nullptr;
    int* d_wfast_of_ref = nullptr;
    void buildFast();                                // host build + upload (triangles and quads); throws ArgError when the builder or the walk's LDS budget declines the scene
    void freeFast();
    bool fastReady() const { return d_wnodes != nullptr; }
    DeviceScene d_scene;
    // guided sampling: per-primitive PrecomputedCDF records (render_config.h:24-31), load order
    std::vector<float> h_precomputed_cdfs;           // n_prims * kCdfDwords: host copy, fetched on demand (precomputedCdfsHost)
    const std::vector<float>& precomputedCdfsHost();
    // the records are built on the device (csrc/radiosity.hip: ptmi_cdf_records); d_src: see launch_cdf_records
    void precomputeCDFsDevice(const void* d_src, int src_kind, hipStream_t stream);
    float* d_precomputed_cdfs = nullptr;
    // precomputeCDFs — application_state.h:492-585, from per-primitive 16x16 radiosity grids (n_prims*256*3 floats, load
    // order; nullptr drops the records).  The radiosity solver that fills the grids in the reference is out of scope:
    // the grids are an input.
    void precomputeCDFs(const float* radiosity_grids_rgb);
    // what the radiosity grids / count grids currently are (kept for the filter button); load order
    std::vector<float> h_radiosity_grids;            // n_prims * 256 * 3, empty = none
    std::vector<float> h_count_grids;                // n_prims * 256 (Triangle/Quad::grid), empty = zero
    std::vector<float> h_filtered_formfactor, h_filtered_radiosity;   // n_prims * 256 each, after precomputeCDFsFromFiltered
    // "Apply Filter & Rebuild CDFs" (ui_windows.h:154-167): filter_pdfs_for_primitives (grid_filter.h:420-507) on the
    // device, then precomputeCDFsFromFiltered (application_state.h:587-680)
    void precomputeCDFsFromFiltered(bool use_bilateral, float sigma_spatial, float sigma_range, hipStream_t stream);
    // per-primitive radiosity for the Radiosity integrator (render_radiosity); n_prims*3 floats, load order; nullptr = zero
    float4* d_radiosity = nullptr;
    void setRadiosity(const float* rgb);
    // next-event estimation: the emitter table (csrc/device_scene.h: EmitterTable), built by both host loaders in load order
    // (buildEmitters), uploaded with the scene and freed with it
    std::vector<int> h_emit_prim;                    // load-order index of emitter j
    std::vector<float> h_emit_cdf;                   // running sum c_j
    float h_emit_total = 0.0f;                       // c_last (1 where the table was built in binary64)
    std::vector<f3> h_emit_normal;                   // geometric normal of emitter j
    std::vector<float> h_pdf_area;                   // per primitive, load order (0: not an emitter)
    float4 *d_emit_rec = nullptr, *d_pdf_area = nullptr;
    float* d_emit_cdf = nullptr;
    EmitterTable d_emitters;
    // specular surfaces (include/ptmi.h: ptmi_set_surfaces): the caller's load-order table by leaf-order slot (csrc/device_scene.h:
    // SurfaceTable).  It indexes primitives, so it goes with the scene (cleanup).  A table whose kinds are all 0 is kept as no
    // table: d_surfaces stays nullptr and a frame takes the route it takes without one.
    // surface_counts: the table's primitives of kind 0 .. 3 (all 0 without one); a rough-metal primitive (kind 3, "rough metal")
    // selects the kernel's SURF = 2 instantiations.
    int n_mirror = 0, n_glass = 0;
    int surface_counts[4] = {0, 0, 0, 0};
    float2* d_surfaces = nullptr;
    bool hasSpecular() const { return d_surfaces != nullptr; }         // a mirror, glass or rough-metal primitive
    bool hasRough() const { return d_surfaces != nullptr && surface_counts[3] > 0; }
    // checked by the caller (checkSurfaces / checkSurfacesRough); kind nullptr drops the table; roughness nullptr: 0.3
    void setSurfaces(const int* kind, const float* ior, const float* roughness = nullptr);
    SurfaceTable surfaceTable() const { SurfaceTable t; t.rec = d_surfaces; return t; }
    // vertex normals (include/ptmi.h: ptmi_set_vertex_normals): the caller's load-order table by leaf-order slot (csrc/device_scene.h:
    // VertexNormalTable).  It goes with the scene (cleanup).  A table without a smooth primitive is kept as no table:
    // d_vertex_normals stays nullptr and a frame takes the route it takes without one.
    int n_smooth = 0;
    float4* d_vertex_normals = nullptr;
    bool hasVertexNormals() const { return d_vertex_normals != nullptr; }
    // checked and classified by the caller (checkVertexNormals, classifyVertexNormals: smooth per load-order primitive and their
    // number); normals nullptr, or no smooth primitive, drops the table
    void setVertexNormals(const float* normals, const std::vector<unsigned char>& smooth, int smooth_count);
    VertexNormalTable vertexNormalTable() const { VertexNormalTable t; t.rec = d_vertex_normals; return t; }
    // albedo texture (include/ptmi.h: ptmi_set_albedo_texture): the caller's load-order UV table by leaf-order slot and the image as
    // float4 texels (csrc/device_scene.h: AlbedoTable).  It goes with the scene (cleanup).  A table without a textured primitive is
    // kept as no table: both arrays stay nullptr and a frame takes the route it takes without one.
    int n_textured = 0, tex_width = 0, tex_height = 0, tex_filter = 0;
    float4* d_albedo_rec = nullptr;
    float4* d_albedo_texels = nullptr;
    bool hasAlbedoTexture() const { return d_albedo_rec != nullptr; }
    // checked by the caller (checkAlbedoTexture); texels nullptr, or no textured primitive, drops the table
    void setAlbedoTexture(int width, int height, const float* texels, int filter, const float* uv, const int* textured);
    AlbedoTable albedoTable() const {
        AlbedoTable t; t.rec = d_albedo_rec; t.texel = d_albedo_texels; t.width = tex_width; t.height = tex_height; t.filter = tex_filter; return t;
    }
    // participating medium (include/ptmi.h: ptmi_set_medium): its box is in scene coordinates, so it goes with the scene (cleanup)
    MediumState medium;
    int sweep_max_prims = 64;                        // scenes up to this many primitives use the wave-uniform sweep
    int force_traversal = -1;                        // test/benchmark override (TraversalMode), -1 = automatic

    // loadScene — application_state.h:367-464.  Throws IoError where the reference prints and returns.
    void loadScene(const std::string& filename, int subdivision_count, bool convert_quads);
    void loadSceneArrays(std::vector<Primitive> prims);
    // host half only (parse + convert + subdivide + BVH), no device involved
    void loadSceneHost(const std::string& filename, int subdivision_count, bool convert_quads);
    void loadSceneArraysHost(std::vector<Primitive> prims);
    void chooseTraversal();                          // picks d_scene.traversal from size/depth and the two knobs below
    void buildPacked();                              // (re)builds the packed layout if the scene qualifies; chooseTraversal() after it
    void cleanup();                                  // application_state.h:466-490
    ~SceneState() { cleanup(); }

private:
    void buildBVH();                                 // RayTracingManager::buildAccelStructure (ray_tracing_backend.h:81-129)
    void buildEmitters();                            // the host half of the emitter table
    void upload();                                   // SoA re-layout + H2D
    void freePacked();
};

// RadiosityState — application_state.h:200-216, 688-787: the radiosity pre-pass that produces what the guided sampling
// modes and the Radiosity integrator read.  Differences by design: the solver works on SoA arrays instead of a device
// copy of the 4364-byte Primitive records; no n^2 curandStates (streams are derived in the kernel); the reference's
// per-iteration update_radiosity_grid (+ filter), whose result every later iteration overwrites, runs once at the end;
// radiosity_history (no reader in the reference outside primitive.h) is not kept.
struct RadiosityStats { double seconds = 0, form_factor_ms = 0, iteration_ms = 0, grid_ms = 0; uint64_t pairs = 0, rays = 0, cert_chain = 0, cert_fallback = 0; int walk = 0; };
struct RadiosityState {
    int num_iterations = 10, mc_samples = 64;        // application_state.h:208
    bool use_monte_carlo = true, is_calculated = false;
    int force_walk = -1;                             // new (debug): -1 automatic, 0 the reference's visibility walk, 2 the certified walk (3 / 4: its chain / its fallback for every blocked ray)
    int cert_min_prims = 256;                        // new: automatic choice takes the certified walk from this many triangles up
    RadiosityBuffers d;                              // device arrays (owned)
    int final_unshot = 0;                            // which d.unshot[] holds the last iteration's unshot radiosity
    // results on the host, load order (filled by runSolver)
    std::vector<float> h_radiosity, h_unshot, h_radiosity_grid;   // n*3, n*3, n*256*3
    std::vector<float> h_grid;                                     // n*256 visible-sample counts
    bool grids_are_scene_grids = false;                            // the scene's radiosity grids are still this solution's
    bool host_grids_current = false;                               // h_radiosity_grid / h_grid are fetched on demand
    void fetchGrids();                                             // D2H of the two n*256 grids (33 + 8 MB at n = 8192)
    void runSolver(SceneState& scene, const uint32_t* d_jump, bool enable_filtering, bool use_bilateral,
                   float filter_sigma_spatial, float filter_sigma_range, hipStream_t stream, RadiosityStats* stats,
                   bool fast_tree = false /* AppConfig::fast_tree: the visibility walk through the opt-in 8-wide tree */);
    void readFormFactors(float* out) const;          // n*n floats, row = receiver
    void cleanup();                                  // application_state.h:779-787
    ~RadiosityState() { cleanup(); }
};

struct RenderState {
    int width = 800, height = 800;                   // DEFAULT_WIDTH/HEIGHT, application_state.h:42-43
    TileMap tile;                                    // rows of the frame this GPU renders
    Sensor h_camera;
    PathState d_state;                               // path state + RNG (replaces d_rand_state)
    unsigned char* d_image = nullptr;                // RGB8, local rows
    float* d_radiance = nullptr;                     // float3 mean radiance, local rows
    unsigned char* h_image = nullptr;                // RGB8, local rows, PINNED: RenderState::h_image (application_state.h:77, 99);
                                                     // renderFrame() ends with the D2H into it (application.h:211) when download_image
    bool download_image = false;
    // frame batches (renderFrames): colour sums of the batch's completed frames, (n_frames - 1) * n_local float4
    float4* d_frame_color = nullptr;
    size_t frame_color_frames = 0;                   // capacity in frames
    int batch_frames = 1, batch_spp = 0;             // what the last render call produced (selectFrame)
    hipEvent_t resolve_gate = nullptr;               // not owned: while set, the next resolve waits for it (a frame gather still
                                                     // reading this rank's tile, csrc/dist.hip)
    // The local pixels are dealt to kMaxChunks independent queues (256-slot blocks, round-robin), each driven through
    // its own stream: while one chunk's launch drains (kernel tail, state write-back burst) the other chunk's
    // workgroups keep the CUs busy.  Chunks share nothing but the read-only scene.
    static constexpr int kMaxChunks = 4, kCountRing = 4;
    struct Chunk {
        hipStream_t stream = nullptr;
        int n = 0;                                   // pixels in this chunk
        int *d_queue_init = nullptr, *d_queue[2] = {nullptr, nullptr}, *d_count = nullptr;
        int* h_count = nullptr;                      // pinned + coherent, kCountRing entries
        int* d_hcount = nullptr;                     // the same memory as the device addresses it (count publishing)
        bool owns_init_queue = false;                // false: d_queue_init points into somebody else's memory (a pass's queue)
        void allocate(size_t capacity, bool own_init_queue);   // queues of `capacity` entries + the count ring; the stream is the context's
        void release();
    } chunk[kMaxChunks];
    int n_chunks = 1;
    int want_chunks = 0;                             // 0 = automatic, else forced (scheduling knob)
    StatCounters* d_stats = nullptr;
    // launch order by cost (refill launches): the segments every pixel took in the last frame and in the one being rendered
    // (d_cost[frame & 1], n_local each, + their maxima), the scratch of the ordering pass and the ordered queue
    unsigned int* d_cost[2] = {nullptr, nullptr};
    unsigned int* d_cost_max = nullptr;              // [2]
    int* d_cost_hist = nullptr;                      // 512
    int* d_queue_ordered = nullptr;                  // n_local
    unsigned long long cost_frame = 0;               // frames rendered with cost accounting since allocateBuffers
    bool cost_valid = false;                         // d_cost[(cost_frame - 1) & 1] holds a whole frame's costs of the pixels as they are numbered now
    uint32_t* d_jump = nullptr;                      // XORWOW skip-ahead matrices (owned by the ctx, set before allocateBuffers)
    uint64_t seed_base = 2023;
    hipStream_t stream = nullptr;
    size_t n_local = 0;
    bool allow_tile8 = false;                        // scheduling knob (test/benchmark override)
    // Progressive / adaptive accumulation (accumPass): the colour sums of D go on from pass to pass; per pixel the state of the
    // stopping test, the queue of the pixels the next pass renders and the bounce queues of a pass (one chunk of n_local entries,
    // driven through chunk[0]'s stream).  Allocated by the first pass, freed with the other buffers.
    struct Accum {
        int pass = 0;                                // passes of the current accumulation (0: none; the next pass is pass 1)
        int n_active = 0;                            // pixels the next pass renders (the last stopping test's count)
        int cur = 0;                                 // d_active[cur]: the next pass's queue
        int* d_active[2] = {nullptr, nullptr};
        AccumBuffers ab;
        unsigned int* d_counts = nullptr;            // samples per pixel, local row-major (ptmi_read_sample_counts)
        int* d_out_count = nullptr;                  // the stopping test's output count
        Chunk chunk;                                 // d_queue_init is not owned: it points at the pass's queue (nullptr at pass 1)
        bool allocated() const { return d_counts != nullptr; }
    } accum;
    // Feature buffers of the local pixels (renderFeatures) and the denoiser's outputs and scratch (denoise); allocated at first
    // use, freed with the other buffers.  Nothing here is read by a frame or a pass.
    struct Denoise {
        FeatureBuffers fb;
        int grid = 0;                                // g of the feature pass the buffers hold
        bool features_valid = false;                 // false: never computed, or stale (scene, camera, resolution, config changed)
        bool image_current = false;                  // the image buffers hold a path-tracing frame or pass rendered since the
                                                     // last such change (what ptmi_denoise may filter)
        bool image_pass = false;                     // that image is an accumulation pass (samples per pixel: accum.d_counts)
        unsigned char* d_rgb8 = nullptr;             // denoised image, local row-major like d_image
        float* d_radiance = nullptr;
        float4* d_buf = nullptr;                     // 2 x n_local: the filter's ping-pong buffers
        bool denoised = false;                       // d_rgb8 / d_radiance hold a result
        double features_ms = 0.0, denoise_ms = 0.0;  // device time of the last feature pass / filter run
        // the variance-guided filter (denoiseVariance): its result goes to d_rgb8 / d_radiance, its scratch is d_buf
        float* d_var_in = nullptr;                   // the variance that steered the last run, local row-major
        float* d_var_out = nullptr;                  // that variance after the last iteration
        bool variance_valid = false;                 // they hold a run's values; stale under the rules of features_valid
        unsigned int* d_owned = nullptr;             // denoiseTemporalVariance: 1 where the history's statistics gave the variance; its own first run allocates it
        double estimate_ms = 0.0, filter_ms = 0.0;   // device time of the last variance estimate / variance-guided filter
    } dn;
    // The temporal accumulation's history (temporalAccumulate) and outputs; allocated at first use, freed with the other
    // buffers.  Nothing here is read by a frame, a pass or ptmi_denoise.
    struct Temporal {
        TemporalHistory side[2];                     // the ping-pong: side[cur] is the history
        int cur = 0;
        bool valid = false;                          // false: the history is empty
        float cam[12] = {};                          // the history's camera frame (ptmi_get_camera_frame) and resolution
        int width = 0, height = 0;
        int grid = 0;                                // g of the features the history holds
        unsigned char* d_rgb8 = nullptr;             // the last step's result, local row-major like d_image
        float* d_radiance = nullptr;
        unsigned long long* d_stats = nullptr;       // accepted, rejected, missed of the last step
        bool stepped = false;                        // d_rgb8 / d_radiance hold a result
        // ptmi_set_temporal_moments: (mu, s2, k, 0) per pixel, a ping-pong that turns with side[]; allocated by the first step
        // with the switch on, meaningful while `valid` (the switch empties the history whenever it changes)
        float4* moments[2] = {nullptr, nullptr};
    } tp;

    void allocateBuffers();                         // application_state.h:91-123 (+ render_init)
    void updateResolution(int w, int h, const TileMap* tiling);   // application_state.h:125-129
    void freeBuffers();
    void setupChunks(int n);                         // deals the local pixels to n queues (allocateBuffers; renderFrames when the walk's launch rule wants another count)
    void freeChunks();
    void allocateAccum();
    void freeAccum();
    void freeDenoise();
    void freeTemporal();
    ~RenderState() { freeBuffers(); }
};

// Multi-GPU frame exchange (csrc/dist.hip): one RCCL communicator per ctx (one process per GPU), a stream of its own, and
// on the destination rank the staging + whole-frame buffers.  New in this implementation (the reference is single-GPU).
struct DistState {
    void* comm = nullptr;                            // ncclComm_t
    int n_ranks = 1, rank = 0;
    hipStream_t stream = nullptr;
    hipEvent_t gather_done = nullptr;
    bool pending = false;                            // a gather has been enqueued and not waited for
    bool failed = false;                             // an nccl* call failed: every later ptmi_dist_* call reports it until re-initialised
    int* d_token = nullptr;                          // barrier payload
    // destination side, (re)allocated per frame geometry
    unsigned char *d_stage_rgb = nullptr, *d_frame_rgb = nullptr;
    float *d_stage_rad = nullptr, *d_frame_rad = nullptr;
    long long* d_tile_offset = nullptr;              // per rank: first element of its tile in the staging buffers
    std::vector<long long> h_tile_offset;
    int frame_w = 0, frame_h = 0, frame_row_block = 0, frame_ranks = 0;
    bool have_rgb = false, have_rad = false;         // what the frame buffers hold

    void init(const void* unique_id128, int n_ranks, int rank);      // ncclCommInitRank
    void gatherFrame(const struct RenderState& r, int dst_rank, int what /* 1 rgb8 | 2 radiance */);   // enqueues, does not wait
    void wait();
    void barrier();                                  // all ranks (1-int all-reduce + stream sync)
    double allreduceMax(double v);
    int commCount() const;                           // ncclCommCount: the ranks RCCL itself reports
    void check() const;                              // throws unless initialised and healthy
    void finalize();
    ~DistState() { finalize(); }
private:
    void ensureFrame(const TileMap& tm, bool want_rgb, bool want_rad);
    void freeFrame();
};
void distUniqueId(void* out128);                     // ncclGetUniqueId
void debugPlaceTiles(int width, int height, int n_ranks, int row_block, const unsigned char* h_tiles_rgb, const float* h_tiles_rad,
                     unsigned char* out_rgb, float* out_rad, hipStream_t s);

// The environment light of a context (include/ptmi.h: ptmi_set_environment): the host table and its device copy.  It belongs
// to the context, like the camera: scene loads keep it.
struct EnvState {
    EnvParams params;
    EnvHostTable h;
    float *d_z = nullptr, *d_marginal = nullptr, *d_row_cdf = nullptr;
    float4* d_texel = nullptr;
    bool present() const { return d_texel != nullptr; }
    void set(int width, int height, const float* rgb, const EnvParams& p);   // builds, then replaces the device copy; throws before anything changes
    void drop();
    // the kernel's view for one run: q and the estimator's switches follow the config and the loaded scene's emitter count
    EnvTable table(bool next_event, int n_emitters) const;
    ~EnvState() { drop(); }
};

// The thin lens of a context (include/ptmi.h: "thin lens"): two numbers that belong to the context, like the camera - scene loads,
// ptmi_update_resolution and ptmi_set_camera keep them - and the device copy of the block derived from them (host/lens.cpp).
struct LensState {
    float radius = 0.0f;                             // 0: the pinhole
    float focus = 0.0f;                              // <= 0: not set - the default, |origin - lookat| of the current camera
    float4* d_block = nullptr;                       // six float4, allocated by the first run that needs them
    float h_block[kLensBlockFloats] = {};            // what d_block holds
    bool uploaded = false;
    bool on() const { return radius > 0.0f; }
    ~LensState();
};

struct FrameStats {
    double seconds = 0, bounce_kernel_ms = 0;
    uint64_t bounce_launches = 0, path_visits = 0, samples = 0, rays = 0, node_visits = 0, prim_tests = 0, hits = 0, top_node_visits = 0,
             cert_chain = 0, cert_fallback = 0;
};

struct ApplicationState {
    int device_id = 0;
    int n_cus = 0;                                   // compute units of the device
    RenderState render;
    SceneState scene;
    RadiosityState radiosity;
    DistState dist;
    AppConfig config;
    int feature_shading = 0;                         // PTMI_FEATURE_* (include/ptmi.h: ptmi_set_feature_shading); the context's, not the scene's
    int temporal_moments = 0;                        // ptmi_set_temporal_moments; the context's, not the scene's
    EnvState env;
    LensState lens;
    std::vector<uint32_t> h_jump;                    // 32 x 160 x 5 words
    std::vector<hipEvent_t> event_pool;

    explicit ApplicationState(int device);
    ~ApplicationState();
};
// The per-lane features present (route_rule.h: a mask of 1 << RouteFeature); next_event: the config's, or the one coming in
inline unsigned presentFeatures(const ApplicationState& g, bool next_event) {
    return next_event << kRouteNextEvent | g.env.present() << kRouteEnvironment | g.scene.hasSpecular() << kRouteSurfaces | g.scene.hasVertexNormals() << kRouteVertexNormals |
           g.scene.hasAlbedoTexture() << kRouteAlbedoTexture | g.lens.on() << kRouteLens | g.scene.medium.on() << kRouteMedium;
}

// renderFrame — application.h:157-216: camera update, launches, device sync.  Results stay on the device.
void renderFrame(ApplicationState& g_state, FrameStats* stats);
// n_frames successive renderFrame() calls with nothing changed in between, as one pipelined run (device_scene.h:
// FrameParams::n_frames).  Frame by frame the images are bit-identical to n_frames separate calls; afterwards the image
// buffers hold the LAST frame and selectFrame(j) resolves any frame of the batch into them.
void renderFrames(ApplicationState& g_state, int n_frames, FrameStats* stats);
void selectFrame(ApplicationState& g_state, int frame);

// Progressive / adaptive accumulation (include/ptmi.h: ptmi_accum_pass): one pass adds config.spp samples to every pixel still
// active, applies the stopping test (rule == nullptr: none) and resolves every pixel by its own sample count.
struct AdaptiveParams { int min_passes = 4, max_passes = 64; float threshold = 0.02f, floor = 0.01f; };
struct PassStats {
    int pass = 0;
    uint64_t active_before = 0, active_after = 0;
    FrameStats frame;                                // seconds: the whole pass, stopping test and resolve included
};
void accumReset(ApplicationState& g_state);
void accumPass(ApplicationState& g_state, const AdaptiveParams* params, PassStats* stats);
void readSampleCounts(const ApplicationState& g_state, uint32_t* counts);
// Test hook (include/ptmi.h: ptmi_debug_accum_step): the pass half of a pass's end - stopping test, resolve by counts - on
// state given by slot instead of rendered; n = n_local.  Returns the length of queue_out
int debugAccumStep(ApplicationState& g_state, const float* sums /* 3n */, const float* prev /* 4n */, const float* m2 /* n */,
                   const uint32_t* passes /* n */, const int* queue /* n_queue, or nullptr: 0 .. n_queue - 1 */, int n_queue,
                   const AdaptiveParams* params, bool first, int* queue_out /* n_queue */);

// Feature buffers and the edge-avoiding a-trous denoiser (include/ptmi.h: ptmi_render_features, ptmi_denoise).
struct DenoiseParams {
    int iterations = 5;
    float sigma_color = 4.0f, color_floor = 2.0f;    // measured: cbox 128^2 at 8 spp
    float sigma_position = 0.0f;                     // <= 0: 2 % of the scene's bounding-box diagonal
    int normal_squarings = 7, feature_grid = 2, demodulate = 1;
};
// an (rgb8, radiance) pair of n_local pixels to the host; either destination may be NULL
void readImagePair(int device_id, size_t n_local, const unsigned char* d_rgb8, const float* d_radiance, unsigned char* rgb8, float* radiance);
void featuresStale(ApplicationState& g_state);       // the triggers that restart an accumulation: features and image are stale
void featuresRedefined(ApplicationState& g_state);   // ptmi_set_feature_shading: features, variance and history go; image and accumulation stay
void renderFeatures(ApplicationState& g_state, int grid);
void readFeatures(const ApplicationState& g_state, float* albedo, float* normal, float* position, float* hit_fraction);
void checkDenoiseParams(const DenoiseParams& p);     // throws ArgError for a parameter out of range
void denoise(ApplicationState& g_state, const DenoiseParams& p);
void readDenoised(const ApplicationState& g_state, unsigned char* rgb8, float* radiance);

// The variance-guided a-trous filter (include/ptmi.h: ptmi_denoise_variance): ptmi_denoise's inputs and outputs, steered by a
// per-pixel variance - the accumulation's statistics where they exist, a spatial estimate elsewhere.
struct VarianceParams {
    int iterations = 5;
    float sigma_luminance = 2.0f, epsilon = 1e-2f;   // measured: cbox 128^2, a frame of 8 spp and an adaptive run
    float sigma_position = 0.0f;                     // <= 0: 2 % of the scene's bounding-box diagonal
    int normal_squarings = 7, feature_grid = 2, demodulate = 1;
    int source = 0;                                  // 0: the accumulation's statistics where they exist; 1: always spatial
    int spatial_radius = 3;
};
void checkVarianceParams(const VarianceParams& p);   // throws ArgError for a parameter out of range
void denoiseVariance(ApplicationState& g_state, const VarianceParams& p);
void readVariance(const ApplicationState& g_state, float* variance_in, float* variance_out);
void readPassMoments(const ApplicationState& g_state, float* mean, float* m2, uint32_t* passes);

// Temporal accumulation with reprojection (include/ptmi.h: ptmi_temporal_accumulate).
struct TemporalParams {
    int max_history = 32;
    float normal_min = 0.9f;
    float sigma_position = 0.0f;                     // <= 0: 1 % of the scene's bounding-box diagonal
    int feature_grid = 2;
    float sigma_albedo = 0.1f;
};
struct TemporalStats {
    uint64_t accepted = 0, rejected = 0, missed = 0;
    double seconds = 0.0, features_ms = 0.0;
};
void temporalReset(ApplicationState& g_state);       // empties the history
void checkTemporalParams(const TemporalParams& p);   // throws ArgError for a parameter out of range
void temporalAccumulate(ApplicationState& g_state, const TemporalParams& p, TemporalStats* stats);
void readTemporal(const ApplicationState& g_state, unsigned char* rgb8, float* radiance);
void readHistoryCounts(const ApplicationState& g_state, float* counts);
void denoiseTemporal(ApplicationState& g_state, const DenoiseParams& p);
// The history's luminance statistics (include/ptmi.h: ptmi_set_temporal_moments) and the variance-guided filter steered by them.
void setTemporalMoments(ApplicationState& g_state, int on);          // a new value empties the history
void readTemporalMoments(const ApplicationState& g_state, float* mean, float* variance, float* frames);
void debugSetTemporalMoments(ApplicationState& g_state, const float* mean, const float* variance, const float* frames);
// Test hook (include/ptmi.h: ptmi_debug_set_filter_inputs): radiance and features of the current resolution, given instead of rendered
void debugSetFilterInputs(ApplicationState& g_state, const float* radiance, const float* albedo, const float* normal, const float* position,
                          const float* hit_fraction, int grid);
void denoiseTemporalVariance(ApplicationState& g_state, const VarianceParams& p);

bool packBvhNodes(const std::vector<BVHNode>& bvh_nodes, int top_records, std::vector<float4>& g, int& n_pos, int& n_top, int& top_depth);

// GF(2) matrices T^(2^67 * 2^k), k = 0..31, of the xorwow state transition (cuRAND's subsequence skip-ahead).
std::vector<uint32_t> buildXorwowJumpMatrices();

std::vector<int> localRowMap(const TileMap& tm);
int countLocalRows(int height, int n_ranks, int rank, int row_block);

// camera update (application.h:161-163) and the camera fields of a frame's parameters (render_state.cpp; frames and feature passes)
void cameraFrameParams(ApplicationState& g_state, FrameParams& fp);

// the focus distance in force: the one ptmi_set_lens gave, else |origin - lookat| of the current camera
float lensFocus(const ApplicationState& g_state);
// The lens block for the camera, resolution and lens as they are now, on the device: derived again at every call and uploaded
// where it differs from what the device holds, so no setter has to remember it.  nullptr: the pinhole.  Throws LensError where
// the block is not finite.  Nothing may be in flight on the context's streams (every run ends with a synchronise).
const float4* lensDeviceBlock(ApplicationState& g_state);
// The medium block of the scene's medium on the device, uploaded where it differs from what the device holds.  nullptr: no medium.
// Nothing may be in flight on the context's streams.
const float4* mediumDeviceBlock(ApplicationState& g_state);

}  // namespace ptmi
