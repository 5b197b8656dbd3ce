/* ptmi.h — C ABI of libptmi.so, the MI355X-native drop-in for the per-pixel
 * path-tracing render loop of USharma002/CUDA-PathTracer.
 *
 * The reference has no plugin/FFI layer; its hot path is reached through three
 * host entry points that mutate one global ApplicationState `g_state`
 * (include/application_state.h:299-308, defined src/main.cu:51):
 *
 *   SceneState::loadScene(filename, subdivision_count, convert_quads)
 *                                   include/application_state.h:367-464
 *   RenderState::allocateBuffers() / updateResolution(w, h)
 *                                   include/application_state.h:91-129
 *   renderFrame()                   include/application.h:157-216
 *
 * A `ptmi_ctx` is that ApplicationState bound to one GPU; each function below
 * names the reference interface it replaces.  Plain pointers and sizes only;
 * every function returns 0 on success or a negative PTMI_E_* code and never
 * throws across the boundary; `ptmi_last_error()` gives the message of the
 * last failure on the calling thread.  One host thread per ctx.
 *
 * There is NO CPU fallback behind this ABI: without a usable HIP device
 * `ptmi_ctx_create` fails with PTMI_E_NO_DEVICE.
 */
#ifndef PTMI_H
#define PTMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_OK            0
#define PTMI_E_INVALID    -1   /* bad argument / state (message says which) */
#define PTMI_E_IO         -2   /* scene file missing, unsupported extension, no primitives */
#define PTMI_E_NO_DEVICE  -3   /* no HIP device / wrong architecture */
#define PTMI_E_HIP        -4   /* a HIP runtime call failed (message carries hipGetErrorString) */
#define PTMI_E_NOMEM      -5   /* device or host allocation failed (reference: cudaMallocSafe throws, utils/cuda_utils.h:54-60) */
#define PTMI_E_DIST       -6   /* librccl could not be loaded or an nccl* call failed (message carries ncclGetErrorString) */

typedef struct ptmi_ctx ptmi_ctx;

/* Camera = the Sensor constructor arguments plus its public yaw/pitch members
 * (include/rendering/sensor.h:16-29, 84-86).  orbit = 1 reproduces renderFrame(),
 * which calls updateCameraOrbit() before every launch (application.h:161,
 * sensor.h:56-67): the origin is re-derived from yaw/pitch/radius, radius being
 * |origin - lookat| of the constructor call.  orbit = 0 uses `origin` as is
 * (Sensor::setPosition, sensor.h:69-72).  Defaults: AppConfig,
 * application_state.h:285-286, and sensor.h:24-25. */
typedef struct {
    float origin[3];      /* (0.5, 3, 8.5) */
    float lookat[3];      /* (0, 2.5, 0)   */
    float vup[3];         /* (0, 1, 0)     */
    float vfov_deg;       /* 40            */
    float yaw_deg;        /* 90            */
    float pitch_deg;      /* 0             */
    int   orbit;          /* 1             */
} ptmi_camera;

/* AppConfig members the path reads (application_state.h:262-293) plus the two
 * values the reference hard-codes: max_depth = 5 (integrator.h:389) and the RNG
 * seed base 2023 (integrator.h:279). */
typedef struct {
    int      spp;             /* AppConfig::spp, default 1 (UI range 1-1000, ui_windows.h:84) */
    int      max_depth;       /* 5 = reference behaviour */
    int      sampling_mode;   /* SamplingMode (render_config.h:38-44): 0 BSDF, 1 FORMFACTOR, 2 RADIOSITY, 4 TOPK (all three: pure
                               * grid sampling, integrator.h:242-257), 3 MIS (integrator.h:238-241).  Modes 1-4 need the records
                               * of ptmi_set_radiosity_grids; without them they fall back to cosine sampling exactly as the
                               * reference does for primitives with an empty grid (integrator.h:258-261) */
    uint64_t seed_base;       /* 2023 */
    /* scheduling knob, results are independent of it: ray segments each path
     * advances per kernel launch before state returns to HBM and the active
     * queue is compacted (1 = pure wavefront, large = megakernel-like). 0 = default: 32 for the small LDS-resident
     * scenes; scenes above 64 primitives render a frame as ONE launch of one wave per wave slot whose lanes take the
     * next queued pixel when theirs is through, in the order of the last frame's per-pixel cost */
    int      segments_per_launch;
    int      collect_stats;   /* 1: also count rays / node visits / primitive tests (slower build of the kernel) */
    /* scheduling knob, results are independent of it: which 64 pixels share a wave.  0 = default (64x1 row strips),
     * 1 = 8x8 pixel tiles (when width and this rank's row count are multiples of 8; measured -1 % with the sweep walk,
     * +1 % with the per-lane walk).  Takes effect at the next ptmi_update_resolution. */
    int      wave_tiles;
    /* scheduling knob, results are independent of it: number of independent pixel chunks, each driven through its own
     * HIP stream so that one chunk's kernel tail overlaps the other's body.  0 = default (2 for frames of >= 2^18 local
     * pixels, else 1), 1 = single stream.  Takes effect at the next ptmi_update_resolution. */
    int      streams;
    float    mis_bsdf_fraction;   /* AppConfig::mis_bsdf_fraction, 0.5 (application_state.h:292) */
    int      integrator;          /* AppConfig::current_integrator (application_state.h:50-53, 283): 0 = PathTracing,
                                   * 1 = Radiosity: renderFrame launches render_radiosity (integrator.h:460-504) - first hit,
                                   * Le + per-primitive radiosity, sqrt gamma - instead of the path tracer */
    int      download_image;      /* 1: ptmi_render_frame ends like renderFrame() does, with the D2H of the 8-bit image into the
                                   * ctx's pinned host image (RenderState::h_image, application.h:211) - read it through
                                   * ptmi_host_image.  0 (default): results stay on the device until asked for */
    int      fast_tree;           /* 0 (default): every ray's hit is the one the reference's walk over its own tree
                                   * (rendering/bvh.h:156-218) returns - frames bit-identical to the reference's.  (Scenes above
                                   * 64 primitives get there through an 8-wide binned-SAH tree plus a per-ray proof, else the
                                   * reference's walk for that ray: the certified walk)  1: opt-in, the same tree
                                   * WITHOUT the proof (last bullet; about 7 % faster): primitives, hit arithmetic, RNG
                                   * draws and shading are untouched; a ray's hit can differ only where two primitives are hit at
                                   * exactly the same t or where the reference's own slab test drops a grazing box
                                   * (cuda-pathtracer_amd/csrc/wide_bvh.h: 1 pixel of 4 M on a 1 M-triangle frame).
                                   * ptmi_run_radiosity_solver reads the switch too: its
                                   * visibility walk (form_factors.h:143-208) then skips the proof as well (n = 8192: 84 -> 71 ms;
                                   * 2 of 67 M form factors differ) */
    int      next_event;          /* 0 (default): the reference's estimator.  1: next-event estimation with MIS - every path vertex
                                   * also samples a point on an emitter and traces one shadow ray to it (the contract: "next-event
                                   * estimation" below).  Needs integrator 0, sampling_mode 0 and fast_tree 0 (ptmi_set_config
                                   * returns PTMI_E_INVALID otherwise).  segments_per_launch, wave_tiles, streams and collect_stats
                                   * have no effect on it: the counters stay 0; seconds, samples, bounce_kernel_ms and
                                   * bounce_launches are filled in */
} ptmi_config;

/* Framebuffer sharding (new in this implementation; the reference is single-GPU).
 * Rows are dealt to ranks in blocks of `row_block` rows, round-robin:
 * global row y belongs to rank (y / row_block) % n_ranks.  RNG streams are keyed
 * by the GLOBAL pixel index (integrator.h:278-279), so the union of all ranks'
 * rows is bit-identical to a single-GPU frame. */
typedef struct {
    int n_ranks;      /* 1 */
    int rank;         /* 0 */
    int row_block;    /* 8 */
} ptmi_tiling;

typedef struct {
    double   seconds;          /* device time of the frame (HIP events around all launches) */
    double   bounce_kernel_ms; /* summed duration of the dominant kernel (ptmi_bounce) */
    uint64_t bounce_launches;  /* launches issued, incl. the 1-2 queued behind the one that emptied the queue (they exit at once) */
    uint64_t path_visits;      /* sum over launches of queued pixels: each reads + writes its 88-byte state once */
    uint64_t samples;          /* local pixels * spp */
    uint64_t rays, node_visits, prim_tests, hits;   /* only with collect_stats */
    uint64_t top_node_visits;  /* of node_visits, those served from the LDS-staged top of the packed layout (large scenes; else 0) */
    uint64_t cert_chain;       /* certified walk (traversal 6), with collect_stats: hits whose one-fetch certificate did not apply and
                                * whose leaf's ancestors were slab-tested one by one */
    uint64_t cert_fallback;    /* ... and rays that were walked again by the reference's own walk (ties, grazed boxes, far origins) */
} ptmi_stats;

/* RadiosityState + the filter switches of AppConfig (application_state.h:207-209, 290-291), defaults in comments */
typedef struct {
    int   num_iterations;         /* "Radiosity Steps" 10 (UI range 0..50) */
    int   mc_samples;             /* 64 (UI range 4..256) */
    int   use_monte_carlo;        /* 1: calculate_form_factors_mc_kernel, 0: point-to-point calculate_form_factors_kernel */
    int   enable_filtering;       /* AppConfig::enable_grid_filtering 0 */
    int   use_bilateral;          /* 1 (0: gaussian) */
    float filter_sigma_spatial;   /* 1.5 */
    float filter_sigma_range;     /* 0.3 */
} ptmi_radiosity_params;

typedef struct {
    double   seconds;             /* device time of the whole solve */
    double   form_factor_ms, iteration_ms, grid_ms;
    uint64_t pairs;               /* n_prims^2 */
    uint64_t rays;                /* shadow rays cast by the form-factor kernel */
    uint64_t cert_chain;          /* certified walk: blocked rays whose proof needed the exact slab tests over the blocker's ancestors */
    uint64_t cert_fallback;       /* certified walk: rays that went through the reference's own walk */
    int      walk;                /* the visibility walk used: 0 the reference's tree, 1 the opt-in fast tree (ptmi_config.fast_tree),
                                   * 2 certified (fast tree + per-ray proof: the reference's answers; default from 256 triangles up) */
} ptmi_radiosity_stats;

/* ---- lifetime ------------------------------------------------------------ */
/* initializeApplication()'s device setup (application.h:92-148). device_id: HIP ordinal. */
int  ptmi_ctx_create(int device_id, ptmi_ctx** out);
void ptmi_ctx_destroy(ptmi_ctx*);                       /* SceneState::cleanup + buffer frees, application_state.h:466-490 */
const char* ptmi_last_error(void);
void ptmi_default_camera(ptmi_camera*);                 /* AppConfig() defaults */
void ptmi_default_config(ptmi_config*);
void ptmi_default_tiling(ptmi_tiling*);

/* ---- SceneState::loadScene (application_state.h:367-464) ------------------ */
/* Parses .obj/.mtl with the reference loader's rules (utils/file_manager.h:39-273),
 * optionally converts quads to triangles (application_state.h:323-365) and
 * subdivides (rendering/form_factors.h:475-574), builds the reference's BVH
 * (rendering/bvh.h:76-219) and uploads an SoA copy.  Replaces any previous scene. */
int ptmi_load_scene(ptmi_ctx*, const char* filename, int subdivision_count, int convert_quads);
/* Same, from arrays (procedural scenes).  type[i]: 0 triangle, 1 quad; verts: n*4*3
 * floats (4th vertex ignored for triangles); normal/bsdf/Le: n*3 floats. */
int ptmi_load_scene_arrays(ptmi_ctx*, int n, const int* type, const float* verts,
                           const float* normal, const float* bsdf, const float* Le);
int ptmi_scene_info(const ptmi_ctx*, int* n_prims, int* n_tris, int* n_quads, int* n_bvh_nodes, int* bvh_depth);
/* Host copies for inspection/tests; arrays sized from ptmi_scene_info. Any pointer may be NULL. */
int ptmi_scene_get_prims(const ptmi_ctx*, int* type, float* verts, float* normal, float* bsdf, float* Le);
int ptmi_scene_get_bvh(const ptmi_ctx*, float* bmin, float* bmax, int* left, int* right, int* count, int* indices);

/* ---- SceneState::precomputeCDFs (application_state.h:492-585) -----------------------------------------------------
 * Per-primitive 16x16 directional radiosity grids -> the 2120-byte PrecomputedCDF records the guided sampling modes
 * read (render_config.h:24-31).  rgb: n_prims * 256 * 3 floats in load order (n_prims must match the loaded scene);
 * NULL drops the records.  In the reference the grids come out of the radiosity pre-pass (form_factors.h), here out of
 * ptmi_run_radiosity_solver (which makes this call itself) or from the caller.  Loading another scene drops the records.
 * The reference's second path of initGridFromPrimitive (integrator.h:44-54: precomputed_cdfs == nullptr, the grid rebuilt
 * per hit from the primitive's raw radiosity grid) cannot arise here: records are built whenever grids are set. */
int ptmi_set_radiosity_grids(ptmi_ctx*, int n_prims, const float* rgb);
/* host copy of the records, n_prims * 530 dwords (is_valid as an int bit pattern); returns PTMI_E_INVALID if there are none */
int ptmi_get_precomputed_cdfs(const ptmi_ctx*, float* out);
/* Per-primitive radiosity (Triangle/Quad::radiosity; n_prims * 3 floats, load order; NULL = zero) shown by the Radiosity
 * integrator: the radiosity solver's output (ptmi_run_radiosity_solver sets it) or the caller's. */
int ptmi_set_radiosity(ptmi_ctx*, int n_prims, const float* rgb);

/* ---- RadiosityState::runSolver (application_state.h:688-777) + what the UI does right after it (ui_windows.h:185-192):
 * SceneState::precomputeCDFs() and the upload of the solved primitives.  Runs on the GPU: form factors for all
 * n_prims^2 pairs (form_factors.h:219-415), num_iterations Jacobi steps (:441-465), the directional radiosity grids
 * (:405-439) and the optional filter (grid_filter.h).  Afterwards the guided sampling modes and the Radiosity integrator
 * use the solution, exactly as if ptmi_set_radiosity_grids / ptmi_set_radiosity had been called with it.
 * The n_prims^2 form factors stay on the device (4 n^2 bytes) until the next solve, scene load or ctx destruction. */
/* "Apply Filter & Rebuild CDFs" (ui_windows.h:154-167): filter_pdfs_for_primitives (grid_filter.h:420-507: luminance of the
 * radiosity grids and the count grids through the 5x5 bilateral / gaussian float filter, each primitive normalised to
 * sum 1) + SceneState::precomputeCDFsFromFiltered (application_state.h:587-680): the guided sampling modes then use
 * records built from the filtered luminance.  Needs radiosity grids (a solver run or ptmi_set_radiosity_grids).
 * "Use Raw CDFs" (ui_windows.h:173-177) = ptmi_use_raw_cdfs: precomputeCDFs() again from the unfiltered grids.
 * NON-FINITE VALUES in grids, form factors and sigmas (a NaN against each comparison, the NaN entries a VALID record can hold,
 * a sigma whose 2 * sigma * sigma is 0, a non-finite direction): see the paragraph of that name under ptmi_debug_cdf_records,
 * whose hooks run these calls' kernels on given values. */
int ptmi_apply_grid_filter(ptmi_ctx*, int use_bilateral, float sigma_spatial, float sigma_range);
int ptmi_use_raw_cdfs(ptmi_ctx*);
/* d_filtered_formfactor / d_filtered_radiosity (application_state.h:160-161), n_prims * 256 floats each; either may be NULL */
int ptmi_get_filtered_pdfs(const ptmi_ctx*, float* formfactor, float* radiosity);
/* (The count grids - Triangle/Quad::grid - are only ever filled by ptmi_run_radiosity_solver; after ptmi_set_radiosity_grids
 * alone they are zero, as after loadScene in the reference, and the filtered form-factor pdf is all zero.) */
void ptmi_default_radiosity_params(ptmi_radiosity_params*);
int ptmi_run_radiosity_solver(ptmi_ctx*, const ptmi_radiosity_params*, ptmi_radiosity_stats* stats /* may be NULL */);
/* The solution in load order; any pointer may be NULL.  form_factors n*n (row = receiver), radiosity n*3, unshot n*3,
 * grid n*256 (visible-sample counts per direction cell, Triangle/Quad::grid), radiosity_grid n*256*3. */
int ptmi_get_radiosity_solution(const ptmi_ctx*, float* form_factors, float* radiosity, float* unshot, float* grid, float* radiosity_grid);

/* ---- RenderState::allocateBuffers / updateResolution (application_state.h:91-129)
 * (Re)allocates the image, path-state and RNG buffers for this rank's rows of a
 * width x height frame and runs render_init (integrator.h:274-280), i.e. RNG
 * streams are re-seeded on every call, as in the reference. */
int ptmi_update_resolution(ptmi_ctx*, int width, int height, const ptmi_tiling* tiling /* NULL = single GPU */);
int ptmi_set_camera(ptmi_ctx*, const ptmi_camera*);
int ptmi_set_config(ptmi_ctx*, const ptmi_config*);
/* Derived camera exactly as Sensor holds it after updateCameraOrbit()/updateCamera():
 * origin, lower_left_corner, horizontal, vertical (12 floats). */
int ptmi_get_camera_frame(const ptmi_ctx*, float* out12);
int ptmi_local_rows(const ptmi_ctx*, int* n_rows);      /* rows of the frame this rank renders */
/* global row index of each local row, n_rows ints */
int ptmi_local_row_map(const ptmi_ctx*, int* rows_out);

/* ---- renderFrame (application.h:157-216) ----------------------------------
 * Renders config.spp samples for every local pixel (RNG state carries over
 * from the previous frame, as in the reference) and leaves the results on the
 * device.  Asynchronous work is complete when it returns. */
int ptmi_render_frame(ptmi_ctx*, ptmi_stats* stats /* may be NULL */);

/* n_frames successive ptmi_render_frame calls with nothing changed in between (scene, camera, config), as ONE pipelined run:
 * a pixel that has finished frame k starts frame k + 1 at once - its RNG stream goes on exactly as it does between two
 * renderFrame() calls - so the few long-running pixels at the end of frame k share the GPU with the head of frame k + 1
 * instead of leaving it idle.  Frame by frame the images are bit-identical to n_frames separate calls.  Afterwards the image
 * buffers hold the LAST frame (what n calls would leave); ptmi_select_frame(j) puts frame j of the batch there instead
 * (then ptmi_read_image / ptmi_gather_frame / ptmi_host_image as usual).  n_frames in [1, 256]; a batch of more than one frame
 * needs spp < 65536 and the PathTracing integrator.  stats cover the whole batch. */
int ptmi_render_frames(ptmi_ctx*, int n_frames, ptmi_stats* stats /* may be NULL */);
int ptmi_select_frame(ptmi_ctx*, int frame /* 0 .. n_frames-1 of the last ptmi_render_frame(s) call */);

/* Results.  Both images hold this rank's rows only, local row-major
 * (local_rows x width x 3); local row r is global row ptmi_local_row_map()[r];
 * row 0 of the frame is the BOTTOM row (v = y/H from the lower-left corner,
 * integrator.h:384-385; the reference flips on PNG save, ui_windows.h:205).
 * rgb8   : the reference's output (mean -> Reinhard -> gamma 2.2 -> 8 bit, integrator.h:393-407)
 * radiance: mean linear radiance before tone mapping (float), an addition for parity checks. */
int ptmi_device_image(const ptmi_ctx*, void** d_rgb8, void** d_radiance);           /* device pointers (for RCCL gathers) */
int ptmi_read_image(const ptmi_ctx*, unsigned char* rgb8, float* radiance);          /* D2H of the local rows; either may be NULL */
/* D2D copy of the local rows into caller-owned DEVICE buffers (e.g. the send buffers of an RCCL gather); either may be NULL */
int ptmi_copy_image_device(const ptmi_ctx*, void* d_rgb8_dst, void* d_radiance_dst);

/* RenderState::h_image (application_state.h:77): the pinned host copy of this rank's 8-bit rows that ptmi_render_frame fills
 * when config.download_image is set; valid until the next ptmi_update_resolution / ptmi_ctx_destroy. */
int ptmi_host_image(const ptmi_ctx*, const unsigned char** rgb8, uint64_t* n_bytes);

/* ---- multi-GPU: the frame-end exchange (new in this implementation) ------------------------------------------
 * One process (or host thread) and one ctx per GPU; every rank loads the same scene and renders its rows
 * (ptmi_update_resolution with ptmi_tiling {n_ranks, rank, row_block}); no data-path collective.  The ONE exchange step
 * of a frame is ptmi_gather_frame: every rank's tile goes to dst_rank over RCCL (direct ncclSend per peer /
 * N-1 ncclRecv on dst in one group: xGMI is point-to-point, every peer pushes over its own link), exact tile sizes, and
 * a kernel on dst places the rows into the whole frame.  librccl.so.1 is loaded on the first ptmi_dist_* call
 * (environment PTMI_RCCL_LIB = a file to load in its place).
 *
 *   rank 0:  ptmi_dist_unique_id(id)  -> ship the 128 bytes to every rank (MPI, a file, torch.distributed, ...)
 *   all   :  ptmi_dist_init(ctx, id, n_ranks, rank)        (collective: ncclCommInitRank)
 *   per frame, all ranks: ptmi_render_frame(ctx, ...); ptmi_gather_frame(ctx, 0, PTMI_GATHER_RGB8)
 *   dst   :  ptmi_read_frame(ctx, rgb8, NULL)  or  ptmi_frame_device(...)
 *
 * ptmi_gather_frame only ENQUEUES (a stream of its own): frames are independent, so the next ptmi_render_frame may
 * start at once; its resolve pass waits on the device for the gather that still reads this rank's tile.
 * ptmi_gather_wait / ptmi_read_frame / ptmi_dist_barrier wait for it. */
#define PTMI_UNIQUE_ID_BYTES 128
#define PTMI_GATHER_RGB8     1     /* the reference's output, 3 B/pixel */
#define PTMI_GATHER_RADIANCE 2     /* float mean radiance, 12 B/pixel */
int ptmi_dist_unique_id(void* out_id /* PTMI_UNIQUE_ID_BYTES */);
/* Between processes RCCL needs dmabuf IPC on this driver stack: export HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment of every
 * rank BEFORE anything in the process initialises HIP (the library does not set it for you).
 * After an nccl* call has failed the communicator is marked failed: every later ptmi_dist_* / ptmi_gather_frame call returns
 * PTMI_E_DIST until ptmi_dist_finalize + ptmi_dist_init. */
int ptmi_dist_init(ptmi_ctx*, const void* id /* PTMI_UNIQUE_ID_BYTES */, int n_ranks, int rank);
int ptmi_dist_comm_count(ptmi_ctx*, int* n_ranks);       /* ncclCommCount: the ranks RCCL itself reports for this communicator */
int ptmi_dist_finalize(ptmi_ctx*);                       /* also done by ptmi_ctx_destroy */
int ptmi_gather_frame(ptmi_ctx*, int dst_rank, int what /* PTMI_GATHER_RGB8 | PTMI_GATHER_RADIANCE */);
int ptmi_gather_wait(ptmi_ctx*);
/* dst_rank only: the assembled width x height frame (row 0 = bottom), device pointers (NULL for a part never gathered) */
int ptmi_frame_device(const ptmi_ctx*, void** d_rgb8, void** d_radiance);
/* dst_rank only: waits for the gather, then D2H of the whole frame; either may be NULL */
int ptmi_read_frame(ptmi_ctx*, unsigned char* rgb8, float* radiance);
int ptmi_dist_barrier(ptmi_ctx*);                        /* all ranks; also drains this rank's gather stream */
int ptmi_dist_allreduce_max(ptmi_ctx*, double* value);   /* in/out: max over ranks (timing: max-over-ranks of a step time) */

/* ---- host-only halves (no device touched; usable without a GPU) ----------------
 * The parse/convert/subdivide/BVH half of loadScene and the camera/tiling arithmetic, for
 * inspection and for tests of the host logic. */
typedef struct ptmi_host_scene ptmi_host_scene;
int  ptmi_host_scene_load(const char* filename, int subdivision_count, int convert_quads, ptmi_host_scene** out);
int  ptmi_host_scene_from_arrays(int n, const int* type, const float* verts, const float* normal,
                                 const float* bsdf, const float* Le, ptmi_host_scene** out);
void ptmi_host_scene_free(ptmi_host_scene*);
/* The limits a scene must keep to be loaded onto the device, checked without one: finite coordinates, edges shorter than 1e18 and,
 * where the scene has quads, largest quad edge x the scene's extent <= 2^124 (the products of the quad test must not overflow:
 * the reference's quad rejects a NaN barycentric that the device's test would not see).  origin (3 floats, may be NULL): a ray
 * origin outside the scene - a camera - held to the same bound.  PTMI_OK, or the error ptmi_load_scene_arrays / a frame gives. */
int  ptmi_host_scene_check_extent(ptmi_host_scene*, const float* origin);
int  ptmi_host_scene_info(const ptmi_host_scene*, int* n_prims, int* n_tris, int* n_quads, int* n_bvh_nodes, int* bvh_depth);
int  ptmi_host_scene_get_prims(const ptmi_host_scene*, int* type, float* verts, float* normal, float* bsdf, float* Le);
int  ptmi_host_scene_get_bvh(const ptmi_host_scene*, float* bmin, float* bmax, int* left, int* right, int* count, int* indices);
/* The emitter table of next-event estimation (see "next-event estimation" below) in load order: prim (load-order index of emitter
 * j) and cdf (c_j) have n_emitters entries each, pdf_area has n_prims (0 for every primitive that is not an emitter).  Any
 * pointer may be NULL (ask for the count first). */
int  ptmi_host_emitters(const ptmi_host_scene*, int* n_emitters, int* prim, float* cdf, float* pdf_area);
/* Sensor after allocateBuffers() + renderFrame()'s camera update for a width x height frame (12 floats). */
/* "Save PNG" (ui/ui_windows.h:195-210): 8-bit RGB file of a whole frame as ptmi_read_image returns it (row 0 = bottom);
 * rows are flipped on write like stbi_flip_vertically_on_write(1) does. */
int  ptmi_write_png(const char* path, int width, int height, const unsigned char* rgb8_bottom_up);
int  ptmi_host_camera_frame(const ptmi_camera*, int width, int height, float* out12);
/* Layout of one PrecomputedCDF record as ptmi_get_precomputed_cdfs returns it and as the kernels read it
 * (render_config.h:24-31): out[0] = bytes per record, out[1..6] = byte offsets of pdf, row_sums, marginal_cdf, row_cdfs,
 * total_weight, is_valid; out[7..9] = GRID_RES, GRID_SIZE, GRID_HALF_RES (render_config.h:7-9). */
int  ptmi_host_cdf_record_layout(int* out10);
/* rows of a `height`-row frame owned by `tiling->rank`; rows_out may be NULL to query the count only */
int  ptmi_host_local_row_map(int height, const ptmi_tiling* tiling, int* n_rows, int* rows_out);

/* ---- unit-test hooks: single stages of the path on the device ------------- */
/* The destination's row-placement step of ptmi_gather_frame alone: tiles in rank order with their exact sizes
 * (sum = width*height*3 elements) -> whole frame.  Either pair may be NULL. */
int ptmi_debug_place_tiles(ptmi_ctx*, int width, int height, int n_ranks, int row_block, const unsigned char* tiles_rgb8,
                           const float* tiles_radiance, unsigned char* out_rgb8, float* out_radiance);
/* Overrides how ptmi_bounce walks the BVH (results are identical in every mode): force_mode -1 = automatic,
 * 0 = wave-uniform sweep, 1 = per-lane stackless, 2 = explicit stack, 3 = per-lane with wave-scheduled phases,
 * 4 = 3 over the packed layout (sibling-pair node order, 36-byte triangles; only where that layout was built, else 3);
 * 6 = certified: the 8-wide tree of ptmi_config.fast_tree + a per-ray proof that the reference's walk returns the same hit,
 *     else the reference's walk for that ray (results identical, the node / test counters are its own) - the automatic choice
 *     of every scene above sweep_max_prims whose tree is no deeper than 62;
 * sweep_max_prims = largest scene (primitives)
 * the automatic choice still sweeps (default 64).  Trees deeper than 62 always use the stack walk.
 * out_mode (may be NULL) receives the mode now in effect for the loaded scene, or -1 without a scene. */
int ptmi_debug_set_traversal(ptmi_ctx*, int force_mode, int sweep_max_prims, int* out_mode);
/* The mode in effect for the loaded scene (-1 without one), nothing changed. */
int ptmi_debug_get_traversal(const ptmi_ctx*, int* out_mode);
/* The visibility walk of the radiosity pre-pass's form-factor kernel: force_walk -1 = automatic (certified from min_prims
 * triangles up, default 256; else the reference's), 0 = the reference's own tree, 2 = certified (the fast tree + a per-ray
 * proof that the reference's any-hit walk answers the same; triangle scenes no deeper than 30; test hooks: 3 / 4 = certified
 * with every blocked ray sent through the proof's second stage / through the reference's own walk).  Form factors are identical
 * either way; ptmi_config.fast_tree (no proof, tolerance mode) takes precedence.  Applies to the next ptmi_run_radiosity_solver. */
int ptmi_debug_set_solver_walk(ptmi_ctx*, int force_walk, int min_prims);
/* The packed layout of traversal mode 4 is built for scenes that do not fit LDS, have at least min_nodes BVH nodes (default
 * 8192), a tree no deeper than 62 and no leaf of more than 7 primitives.  Applies to the loaded scene at once and to later
 * loads; n_positions (may be NULL) receives the number of record positions built (0 = none).  Results do not depend on it. */
int ptmi_debug_set_packed_min_nodes(ptmi_ctx*, int min_nodes, int* n_positions);
/* How much of the packed tree every workgroup keeps in LDS: the nodes of depth <= D, D the largest depth whose levels fit
 * top_records 32-byte records (default 512 = 16 KB; 0 = none; at most 2048).  Applies to the loaded scene at once and to
 * later loads; n_top / top_depth (may be NULL) receive what was built.  Results do not depend on it. */
int ptmi_debug_set_packed_top(ptmi_ctx*, int top_records, int* n_top, int* top_depth);
/* Scene::intersect (scene.h:39-110) for n rays given as-is (no normalisation). out_*: n each; p/nrm 3n. */
int ptmi_debug_intersect(ptmi_ctx*, int n, const float* o, const float* d, float t_min, float t_max,
                         int* hit, int* prim, float* t, float* p, float* nrm);
/* The opt-in fast tree (ptmi_config.fast_tree; cuda-pathtracer_amd/csrc/wide_bvh.h).  Builder knobs: max_leaf 1..3 triangles per
 * leaf child (default 3), c_trav / c_tri = SAH cost of a box level / a triangle test (1, 1), top_nodes = whole levels kept in
 * LDS while they fit this many 128-byte nodes (80).  Rebuilds the loaded scene's fast tree at once and
 * applies to later loads; any out pointer may be NULL. */
int ptmi_debug_set_fast_tree(ptmi_ctx*, int max_leaf, float c_trav, float c_tri, int top_nodes, int* n_nodes, int* depth, int* n_top);
/* Closest hit through the fast tree for n rays as given (the walk of ptmi_bounce_wide).  prim: load-order index or -1;
 * counts (may be NULL): [0] node visits, [1] triangle tests, summed over the rays. */
int ptmi_debug_intersect_fast(ptmi_ctx*, int n, const float* o, const float* d, float t_min, float t_max,
                              int* hit, int* prim, float* t, uint64_t* counts);
/* first_hit for n rays as given: the closest hit of the Radiosity view and the feature pass, by the walk they take for the loaded
 * scene (the certified walk where the scene has it, else the reference's walk, LANE or STACK); t_max is theirs, FLT_MAX.  prim:
 * load-order index or -1.  The answer is the reference's hit in every mode. */
int ptmi_debug_first_hit(ptmi_ctx*, int n, const float* o, const float* d, float t_min, int* hit, int* prim, float* t);
/* Host-only halves of the same: build the fast tree of a host scene, and walk it on the CPU decision for decision as the
 * kernel does (tests of the builder without a GPU). */
int ptmi_host_fast_tree_build(ptmi_host_scene*, int max_leaf, float c_trav, float c_tri, int* n_nodes, int* depth, double* sah);
/* shape of the built tree: out[0..8] = nodes with that many children, out[9..12] = leaf children with 0..3 triangles */
int ptmi_host_fast_tree_stats(const ptmi_host_scene*, int* out13);
int ptmi_host_fast_tree_intersect(const ptmi_host_scene*, int n, const float* o, const float* d, float t_min, float t_max,
                                  int* prim, float* t, uint64_t* counts /* [0] node visits [1] triangle tests [2] deepest stack */);
/* render_init + curand_uniform: first `count` uniforms of pixel stream (seed_base+pixel, subsequence pixel). */
int ptmi_debug_rng(ptmi_ctx*, uint64_t seed_base, int n_pixels, const int* pixels, int count, float* out /* n_pixels*count */);
/* Compares the kernels' short reciprocal (1 v_rcp + 4 fma, used for Moller-Trumbore's 1/a) with the IEEE quotient for
 * the `count` consecutive float bit patterns starting at first_bits; reports how many differ and the first one. */
int ptmi_debug_rcp_check(ptmi_ctx*, uint32_t first_bits, uint64_t count, uint64_t* mismatches, uint32_t* first_bad_bits);
/* The same for the kernels' short square root (v_sqrt_f32 + two residual fmas, no denormal scaling) against the correctly
 * rounded one. */
int ptmi_debug_sqrt_check(ptmi_ctx*, uint32_t first_bits, uint64_t count, uint64_t* mismatches, uint32_t* first_bad_bits);
/* The walks' 1 / d for n directions (3 floats each).  Cases 64w .. 64w + 63 form one wave and share its vote between the short
 * reciprocal and the IEEE division; live[i] == 0 makes case i a lane without a ray, which has no say in the vote. */
int ptmi_debug_ray_inv(ptmi_ctx*, int n, const float* d, const int* live, float* out_inv /* 3n */);
/* The shade step's short forms (csrc/shade_lean.h, csrc/shading.h, csrc/pt_vec.h), built with the bounce kernels' flags.
 * sincos_lean_check: the cosine sample's sincos behind its wave vote against ptmi_sincosf for `count` consecutive bit patterns from
 * first_bits: patterns whose sin / cos differ (the voted result, or - in [0, (float)(2 pi)] and not flagged - the short form
 * itself), the first of them, the lanes in that interval that raised the ambiguity flag, and up to 8 of their patterns.
 * sincos_lean / unit_voted: the voted sincos of x[i] / the voted normalisation of w[3i..3i+3) per wave - cases 64v .. 64v + 63 form
 * one wave, live[i] == 0 makes case i a lane that is not active, as in ptmi_debug_ray_inv.  out: per case the voted result, then
 * the long form's (sin, cos, sin, cos / 3 + 3 floats); zero for a case that is not live.
 * size_div_check: the pixel jitter's a / size for `count` consecutive bit patterns of a against the IEEE division, with the
 * reciprocal chosen as the renderer chooses it; lean = 1 if this size takes the short form, 0 if it keeps the division. */
int ptmi_debug_sincos_lean_check(ptmi_ctx*, uint32_t first_bits, uint64_t count, uint64_t* bad_sin, uint64_t* bad_cos,
                                 uint32_t* first_bad_bits, uint64_t* flagged, uint32_t* flagged_bits /* 8 */, int* n_flagged_bits);
int ptmi_debug_sincos_lean(ptmi_ctx*, int n, const float* x, const int* live, float* out /* 4n */);
int ptmi_debug_unit_voted(ptmi_ctx*, int n, const float* w, const int* live, float* out /* 6n */);
int ptmi_debug_size_div_check(ptmi_ctx*, int size, uint32_t first_bits, uint64_t count, uint64_t* mismatches, uint32_t* first_bad_bits,
                              int* lean);
/* sampleCosineHemisphere (integrator.h:62-85) with explicit (u, v). */
int ptmi_debug_cosine_sample(ptmi_ctx*, int n, const float* normals, const float* u, const float* v, float* out_dirs);
/* Guided sampling per call, through the bounce kernels' own device functions (debug_hooks.hip: ptmi_debug_guided_k).  Case i
 * draws from XORWOW state states[6i..6i+6) (v0..v4, d); used[i] = draws made, counted from d = 0.  op: 0 sampleCosineHemisphere,
 * 1 Grid::sample, 2 Grid::computePDF (dir = in3), 3 sampleMIS (bsdf_prob = in3[0]), 4 misPowerHeuristic(in3[0], in3[1]),
 * 5 render's tone-map of colour in3.  Ops 1-3 read record rec_idx[i] of the n_recs PrecomputedCDF records (530 words each).
 * out: 6 floats per case - direction (op 5: the three 8-bit values), then pdf / weight / heuristic (op 5: radiance). */
int ptmi_debug_guided_sample(ptmi_ctx*, int op, int n, int n_recs, const float* recs, const int* rec_idx, const float* normals,
                             const float* in3, const uint32_t* states, float* out /* n*6 */, int* used /* n */);
/* The numerics contract per call: the gfx950 build of include/ptmi_math.h and the IEEE primitives the kernels rely on (debug_hooks.hip:
 * ptmi_debug_math_k, built with the bounce kernels' flags).  One operation on n cases (a[i], b[i]); out holds two doubles per case,
 * float and int results promoted to double (exact), the second 0 where an operation has one result.  oracle/ptmi_oracle.c's
 * po_math_batch is the host build of the same operations under the same numbers. */
enum {
    PTMI_MATH_SINCOS_D = 0,   /* ptmi_sincos_d of (double)a           -> sin, cos */
    PTMI_MATH_TAN_D    = 1,   /* ptmi_tan_d of (double)a */
    PTMI_MATH_LOG_D    = 2,   /* ptmi_log_d of (double)a */
    PTMI_MATH_EXP_D    = 3,   /* ptmi_exp_d of (double)a */
    PTMI_MATH_ATAN2_D  = 4,   /* ptmi_atan2_d of (double)a, (double)b  a = y, b = x */
    PTMI_MATH_SINCOSF  = 5,   /* ptmi_sincosf of a                     -> sin, cos */
    PTMI_MATH_POWF     = 6,   /* ptmi_powf of a, b */
    PTMI_MATH_EXPF     = 7,   /* ptmi_expf of a */
    PTMI_MATH_ATAN2F   = 8,   /* ptmi_atan2f of a, b                   a = y, b = x */
    PTMI_MATH_ACOSF    = 9,   /* ptmi_acosf of a */
    PTMI_MATH_DIV      = 10,  /* a / b in binary32 */
    PTMI_MATH_RCP      = 11,  /* rcp_rn(a) = 1.0f / a */
    PTMI_MATH_SQRT     = 12,  /* sqrt_rn(a) */
    PTMI_MATH_ROUND    = 13,  /* (float)((double)a * (double)b): the product is exact, so this is the one rounding to binary32 */
    PTMI_MATH_TRUNC    = 14,  /* (int)a, (int)(double)a; |a| < 2^31 (outside it the conversion is undefined in C) */
    PTMI_MATH_OPS      = 15
};
int ptmi_debug_math(ptmi_ctx*, int op, int n, const float* a, const float* b, double* out /* n*2 */);
/* direction_to_grid_index_local (form_factors.h:107-130), the function the form-factor kernel bins with, on n (direction, normal)
 * pairs as given: out[i] = theta row * 16 + phi column.  oracle: po_direction_to_grid_index. */
int ptmi_debug_grid_index(ptmi_ctx*, int n, const float* dirs, const float* normals, int* out /* n */);
/* The light and surface sampling functions of the next-event kernel per call (debug_hooks.hip: ptmi_debug_nee_call_k, built with
 * the kernel's flags, calling the kernel's own functions of csrc/light_sample.h and csrc/rough.h).  One op on n cases against the
 * context's own device tables: the emitter table of the loaded scene, the table of ptmi_set_environment, and q, omq and env_on as a
 * frame with next_event set has them (q = 1 without emitters; env_on: the map's total > 0).  in: PTMI_NEE_CALL_IN floats per case,
 * read from the front in the order listed; out_f: PTMI_NEE_CALL_OUT_F floats and out_i: PTMI_NEE_CALL_OUT_I ints per case, written
 * from the front in the order listed and zero behind.  Floats a function leaves undefined after a false verdict are unspecified.
 * n = 0 does nothing.  The ENV ops need an environment, EMITTER_SAMPLE a scene with an emitter, ENV_LOOKUP finite directions (the
 * kernel never looks up another); anything else is PTMI_E_INVALID. */
enum {
    PTMI_NEE_CALL_ENV_LOOKUP     = 0,  /* texel(d)  in: d  out_i: row, column  out_f: texel rgb, texel pdf */
    PTMI_NEE_CALL_ENV_SAMPLE     = 1,  /* step 3' in: r1, r2, r3, r4  out_i: row, column  out_f: wi, texel pdf, texel rgb */
    PTMI_NEE_CALL_EMITTER_SAMPLE = 2,  /* in: u_sel (after its rescaling by q), r1, r2, o2  out_i: emitter index j, leaf-order slot, guards
                                        * (cos_l > 0 and 0 < p_l <= FLT_MAX)  out_f: wi, dist2, cos_l, p_l, p_l times omq where env_on (else p_l) */
    PTMI_NEE_CALL_SPECULAR       = 3,  /* in: d, stored normal n_k, kind (1 or 2, as a float), ior, u  out_i: reflected, the length test
                                        * out_f: F (1 for a mirror and under total internal reflection), next, next normalised */
    PTMI_NEE_CALL_ROUGH_VERTEX   = 4,  /* in: sn, d, alpha  out_i: the grazing test of co  out_f: un, T, B, wo, Lambda(co) (0 where the test fails) */
    PTMI_NEE_CALL_ROUGH_EVAL     = 5,  /* in: sn, d, alpha, wi  out_i: contributes  out_f: g, p_b */
    PTMI_NEE_CALL_ROUGH_SAMPLE   = 6,  /* in: sn, d, alpha, u1, u2  out_i: the path goes on  out_f: next (not normalised), weight, p_b */
    PTMI_NEE_CALL_LIGHT_WEIGHT   = 7,  /* in: rough (0 or 1), sn, d, alpha, wi, cos_s, p  out_i: contributes without and with a rough-metal table
                                        * out_f: the weight (f cos mis(p, p_b)) / p without such a table (the cosine lobe) and with one */
    PTMI_NEE_CALL_OPS            = 8,
    PTMI_NEE_CALL_IN = 16, PTMI_NEE_CALL_OUT_F = 16, PTMI_NEE_CALL_OUT_I = 4
};
int ptmi_debug_nee_call(ptmi_ctx*, int op, int n, const float* in, float* out_f, int* out_i);

/* ---- progressive and adaptive accumulation (new in this implementation) -------------------------------------------------
 * A frame is an independent estimate of config.spp samples per pixel.  An ACCUMULATION instead goes on from pass to pass:
 * ptmi_accum_pass adds config.spp samples to every local pixel that is still active, applies the stopping test below and
 * resolves the image buffers that ptmi_read_image / ptmi_copy_image_device / ptmi_gather_frame / ptmi_host_image (with
 * download_image) read: every pixel as mean -> Reinhard -> gamma -> 8 bit of ITS OWN sample count n, with the arithmetic of a
 * frame's resolve and rcp_rn((float)n) as the factor.  A pixel's colour sum after k passes of spp samples is the float a single
 * frame of k * spp samples from the same stream position sums, bit for bit, so every pixel equals the frame at its own count.
 *
 * Streams are not re-seeded: an accumulation starts wherever the streams stand, as a frame does (after
 * ptmi_update_resolution: freshly seeded).  The accumulation is RESET - the next pass is pass 1 and starts from zero sums - by
 * ptmi_accum_reset and by every call that changes what a frame would show: ptmi_set_camera, a successful ptmi_set_config,
 * a successful ptmi_set_environment, ptmi_update_resolution, the scene loads, ptmi_set_radiosity_grids, ptmi_set_radiosity, ptmi_apply_grid_filter,
 * ptmi_use_raw_cdfs, ptmi_run_radiosity_solver, and ptmi_render_frame / ptmi_render_frames (which behave exactly as before).
 * PTMI_E_INVALID: the Radiosity integrator (config.integrator = 1), ptmi_select_frame after a pass, parameters out of range
 * or NaN, a pass after the accumulation has finished (no pixel active) or reached params->max_passes, and a pass that would
 * take a pixel to 2^24 samples.
 *
 * THE STOPPING RULE, per pixel after its pass k, in float32 in the order written (the library is built with
 * -ffp-contract=off; S = the pixel's colour sum after the pass, S_0 = 0, mean_0 = M2_0 = 0):
 *     d     = S_k - S_{k-1}                                         (per channel)
 *     y     = (0.2126f * d.x + 0.7152f * d.y + 0.0722f * d.z) * inv_spp        inv_spp = rcp_rn((float)spp)
 *     delta = y - mean;  mean = mean + delta / (float)k;  M2 = M2 + delta * (y - mean)
 *     a     = threshold * (mean + floor)
 *     stop  <=>  k == max_passes  or  (k >= min_passes  and  M2 <= a * a * (float)(k * (k - 1)))   (k * (k - 1): uint32)
 * i.e. the standard error of the mean of the pass means, sqrt(M2 / (k (k - 1))), is at most threshold x (mean + floor).  It
 * reads nothing but the pixel's own sums: neighbours, launch order, tiling and the walk never change a decision.
 * params == NULL: a plain progressive pass - every pixel renders, none stops.
 * NON-FINITE VALUES (an overflowed firefly in S: Inf, then Inf - Inf).  The rule is IEEE arithmetic and nothing else: a NaN or
 * infinite channel of S makes y, mean and M2 non-finite (an Inf d gives mean = Inf and y - mean = NaN), and a NaN M2 stays a NaN
 * in every later pass.  A comparison with a NaN is false, so "M2 <= ..." fails for a NaN M2 and for a NaN bound: such a pixel
 * never stops by its spread and runs until k == max_passes stops it, which needs no M2.  An M2 a few ulps below zero (the
 * update can round it there) compares like a zero and stops; with threshold == 0 the bound is 0 and only M2 <= 0 stops.  The
 * pixel resolves as its sum says (NaN and Inf tone-map to 255, see ptmi_denoise's NON-FINITE VALUES).  No other pixel is
 * affected - not its moments, its decision, its place among the survivors of its wave, its image - since the test reads the
 * pixel's own sums alone.  ptmi_denoise_variance (source = 0) takes max(0, M2 / (k (k - 1))) by fmaxf: a negative and a NaN M2
 * both give variance 0.
 *
 * Multi-GPU: every rank adapts its own rows.  The distributed loop, per pass on every rank:
 *     ptmi_accum_pass(ctx, &params, &st); double a = (double)st.active_after; ptmi_dist_allreduce_max(ctx, &a);
 *     if (a == 0) break;   (then ptmi_gather_frame as after a frame; a rank that has finished skips its further passes)
 * The gather is unchanged. */
typedef struct {
    int   min_passes;   /* passes every pixel takes before it may stop; >= 2 (a spread needs two pass means) */
    int   max_passes;   /* >= min_passes, <= 65536; max_passes * config.spp < 2^24 */
    float threshold;    /* relative standard error at which a pixel stops, >= 0 */
    float floor;        /* added to the mean in the test, > 0: keeps dark pixels from running to max_passes on noise alone */
} ptmi_adaptive_params;
typedef struct {
    int      pass;            /* passes of this accumulation so far */
    uint64_t active_before;   /* local pixels this pass rendered */
    uint64_t active_after;    /* still active after its stopping test (0: the accumulation is finished) */
    uint64_t samples;         /* samples this pass added (active_before * spp) */
    double   seconds;         /* device time of the pass, stopping test and resolve included */
    /* the ptmi_stats fields of the pass (rays .. cert_fallback only with config.collect_stats) */
    double   bounce_kernel_ms;
    uint64_t bounce_launches, path_visits;
    uint64_t rays, node_visits, prim_tests, hits, top_node_visits, cert_chain, cert_fallback;
} ptmi_pass_stats;
void ptmi_default_adaptive_params(ptmi_adaptive_params*);   /* min_passes 4, max_passes 64, threshold 0.02, floor 0.01 */
int  ptmi_accum_reset(ptmi_ctx*);
int  ptmi_accum_pass(ptmi_ctx*, const ptmi_adaptive_params* /* NULL: plain progressive */, ptmi_pass_stats* /* may be NULL */);
/* samples per local pixel of the current accumulation (0 everywhere before its first pass), local rows x width, local
 * row-major like ptmi_read_image */
int  ptmi_read_sample_counts(const ptmi_ctx*, uint32_t* counts);

/* ---- feature buffers and an edge-avoiding a-trous denoiser (new in this implementation) -----------------------------------
 * FEATURE PASS.  ptmi_render_features traces g x g camera rays per local pixel (g = grid, 1..4) through the stratum centres
 * and keeps, per pixel, the means of the first hits' albedo (Kd), stored primitive normal, hit point and hit fraction ("shaded
 * features", below, makes the first two the textured colour and the interpolated normal on request).  It uses
 * no RNG (the pixel streams are neither read nor written) and changes no image, sum or accumulation state.  In float32, in
 * the order written (-ffp-contract=off, correctly rounded division):
 *     for j = 0 .. g-1 (outer), i = 0 .. g-1 (inner):
 *         u = ((float)x + ((float)i + 0.5f) / (float)g) / (float)width      x, y: the GLOBAL pixel (row 0 = bottom)
 *         v = ((float)y + ((float)j + 0.5f) / (float)g) / (float)height
 *         ray = the camera's get_ray(u, v) of a frame (a frame's camera_ray with the jitter replaced by the stratum centre)
 *         hit = the reference's closest hit for t > 1e-4 (the walk of the Radiosity view: certified above 64 primitives)
 *         if hit: A = A + Kd;  N = N + normal;  P = P + (o + t * d);  H = H + 1.0f      (per component; sums start at +0)
 *     k = rcp_rn((float)(g * g));  albedo = A * k, normal = N * k, position = P * k, hit_fraction = H * k
 * A miss adds nothing (the same as adding zeros).  The pass works on tiled contexts: every rank computes its own rows.
 * ptmi_read_features returns the buffers of the last feature pass in local row-major order (that of ptmi_read_image): albedo,
 * normal and position 3 floats per pixel, hit_fraction 1; any pointer may be NULL.
 * Features go STALE under the calls that restart an accumulation (see ptmi_accum_pass: scene loads, camera, resolution,
 * config, environment, radiosity changes); ptmi_read_features then fails until the next ptmi_render_features, and ptmi_denoise recomputes them.
 *
 * THE FILTER.  ptmi_denoise filters the radiance that ptmi_read_image would return (the selected frame, or the last
 * accumulation pass) into buffers of its own; the frame image, colour sums, streams and accumulation state are untouched, so the
 * next frame, pass or read is bit-identical to one without the denoise.  With iterations = 0 the output is the input (no
 * demodulation round trip): radiance equal, rgb8 equal to ptmi_read_image's.  Otherwise, float32 in the order written:
 *   1. c = radiance; with demodulate, per channel: if albedo.ch != 0: c.ch = c.ch / albedo.ch
 *      lum(c) = 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z
 *   2. for iteration it = 0 .. iterations-1, stride s = 2^it, sigma_c = sigma_color * 2^-it (exact), for every pixel p, over
 *      the taps q = p + (di * s, dj * s), dj = -2..2 (outer, rows), di = -2..2 (inner, columns); a q outside the image is skipped:
 *         h   = H[dj + 2] * H[di + 2]                          H = {1/16, 1/4, 3/8, 1/4, 1/16}
 *         a   = sigma_c * (min(lum(c_p), lum(c_q)) + color_floor)    (the darker of the two: a firefly or an emitter next to a
                                                                       dimmer pixel weighs little from either side)
 *         wc  = 1 / (1 + ((dr*dr + dg*dg) + db*db) / (a * a))          (dr, dg, db) = c_p - c_q
 *         wn  = max(0, (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z), then wn = wn * wn normal_squarings times
 *         wx  = 1 / (1 + ((ex*ex + ey*ey) + ez*ez) / (sigma_x * sigma_x))     (ex, ey, ez) = position_p - position_q
 *         w   = (((h * wc) * wn) * wx);   W = W + w;   S.ch = S.ch + w * c_q.ch         (W, S start at +0, taps in order)
 *      c'_p = S / W per channel (true division) if W > 0, else c'_p = c_p;  every pixel reads the previous iteration's c.
 *      sigma_x = sigma_position, or for sigma_position <= 0: 0.02f * sqrtf((dx*dx + dy*dy) + dz*dz) with (dx, dy, dz) = max - min
 *      of the root box of the scene's BVH (ptmi_scene_get_bvh node 0); sigma_x * sigma_x is computed in float.
 *   3. with demodulate, per channel: if albedo.ch != 0: c.ch = c.ch * albedo.ch
 *   4. radiance = c; rgb8 = the frame's tone map of c (c / (c + 1), to the power 1 / 2.2f by ptmi_math.h's powf, 255.99f * min(., 1), truncated).
 * Features are the current ones for params->feature_grid, recomputed first if stale or of another grid.  A pixel every
 * feature ray missed has normal 0, so all its taps weigh 0 and it keeps its input.
 * NON-FINITE VALUES (an overflowed firefly: Inf, then Inf - Inf).  Everywhere in this header's filters min and max are C's fminf
 * and fmaxf - of a NaN and a number they give the number - and a comparison with a NaN is false, so "if W > 0" fails for a NaN W;
 * everything else is IEEE arithmetic, in which NaN and Inf propagate.  For step 2, per iteration:
 *   - a NaN in c_p or c_q makes wc, w and so the W of p NaN: p keeps its value of the previous iteration, whole (c'_p = c_p).  A
 *     NaN pixel therefore stays NaN and never spreads: each pixel with a tap on it passes through unfiltered in that iteration.
 *   - c_q = +-Inf next to a finite c_p gives wc = 0 and w * c_q = 0 * Inf = NaN: W stays finite and c'_p becomes NaN in the
 *     channels that are Inf in c_q.  An Inf pixel itself has the tap p = q with Inf - Inf = NaN and keeps its value.  So an Inf
 *     turns the pixels that tap it in that iteration (p +- {0, s, 2s} in x and in y) into NaN, which then behave as above.
 *   - a NaN in n_p or n_q gives wn = max(0, NaN) = 0: the tap weighs 0 like a miss (the pixel is skipped by its neighbours and,
 *     its own taps all weighing 0, keeps its input), provided wc and wx are finite: 0 * NaN is NaN.
 *   - position_q = +-Inf gives wx = 0 at a finite p (the tap weighs 0); at p = q, Inf - Inf makes W NaN and p keeps its input.  A NaN
 *     position makes wx NaN at every tap that reads it: those pixels keep their values in every iteration.
 * After `iterations` iterations a non-finite input pixel can have changed only the pixels within 2 * (2^iterations - 1) of it in x
 * and in y (the sum of the strides' reach); of those only the ones named above can be non-finite, the others are finite but are
 * not what they would be without it.  Every pixel outside that square is bit-identical to a run without the non-finite value.
 * Steps 1 and 3 are per pixel; step 4's min(., 1) turns a NaN into 255.
 * PTMI_E_INVALID: a context tiled over more than one rank (the filter needs rows of other ranks), the Radiosity integrator, no
 * image to filter, and parameters out of range or NaN.  "No image" means no path-tracing frame or pass has completed since the
 * last call that makes features stale (the list above), so the image and its features always show the same scene and view:
 * after ptmi_update_resolution, ptmi_set_camera, ptmi_set_config, a scene load, ... render first (a Radiosity frame does not
 * count); ptmi_select_frame keeps the batch's image current. */
typedef struct {
    int   iterations;        /* 5; 0 .. 10 */
    float sigma_color;       /* 4.0; relative colour tolerance of iteration 0, 1e-4 .. 1e4 */
    float color_floor;       /* 2.0; added to the luminance in the colour weight (radiance units), 1e-6 .. 1e4 */
    float sigma_position;    /* 0 (<= 0: 2 % of the scene's bounding-box diagonal); else 1e-6 .. 1e12 */
    int   normal_squarings;  /* 7 (normal weight = max(0, n_p . n_q)^128); 0 .. 10 */
    int   feature_grid;      /* 2; the g of the feature pass, 1 .. 4 */
    int   demodulate;        /* 1: filter radiance / albedo; 0: the radiance itself */
} ptmi_denoise_params;
void ptmi_default_denoise_params(ptmi_denoise_params*);
/* the parameter check of ptmi_denoise alone (no context, no device): 0 or PTMI_E_INVALID with the message */
int  ptmi_check_denoise_params(const ptmi_denoise_params*);
int  ptmi_render_features(ptmi_ctx*, int grid);
int  ptmi_read_features(const ptmi_ctx*, float* albedo, float* normal, float* position, float* hit_fraction);
int  ptmi_denoise(ptmi_ctx*, const ptmi_denoise_params* /* NULL: defaults */);
/* the last denoise's result, local row-major like ptmi_read_image; either may be NULL */
int  ptmi_read_denoised(const ptmi_ctx*, unsigned char* rgb8, float* radiance);
/* device time (hipEvents) of the last feature pass and of the last filter run (feature pass excluded), in ms */
int  ptmi_denoise_timing(const ptmi_ctx*, double* features_ms, double* denoise_ms);

/* ---- variance-guided a-trous filter (new in this implementation) ----------------------------------------------------------
 * ptmi_denoise_variance is the spatial stage of SVGF (Schied et al. 2017): ptmi_denoise's a-trous filter with the colour
 * edge-stop replaced by a luminance edge-stop whose tolerance is the pixel's own standard deviation, and with that variance
 * carried through the iterations.  A converged pixel is left nearly alone, a noisy one is blurred.  Inputs, validity rules and
 * outputs are ptmi_denoise's: it filters the radiance ptmi_read_image would return into the denoiser's output buffers
 * (ptmi_read_denoised), recomputes stale features, and leaves frames, sums, streams, the accumulation and the temporal history
 * untouched; a ptmi_denoise after it gives what it gives alone.  The variance it was steered by and the variance left after the
 * last iteration are kept (ptmi_read_variance) until the next call that makes features stale.
 *
 * THE FILTER, float32 in the order written (-ffp-contract=off, correctly rounded division); lum, H, wn, wx and sigma_x are
 * ptmi_denoise's; taps outside the image are skipped:
 *   1. c = radiance, demodulated as in ptmi_denoise step 1;  l_p = lum(c_p).
 *   2. VARIANCE FROM THE ACCUMULATION, with source = 0, where the image is a pass of the current accumulation and the pixel has
 *      taken k >= 2 passes (M2: the stopping rule's, ptmi_read_pass_moments):
 *         v  = max(0, M2 / (float)(k * (k - 1)))         (k * (k - 1): uint32, as in the stopping rule) - the variance of the
 *                                                        mean of the pixel's pass means, in radiance units;
 *         lr = lum(radiance_p);  if lr > 0:  s = l_p / lr;  v = (v * s) * s        (into the filtered signal's units)
 *      (the max: Welford's M2 can round to a negative of a few ulps for a pixel whose pass means are all equal; a negative
 *      variance would make the tolerance of step 4 negative.)
 *   3. SPATIAL VARIANCE, for every other pixel (a frame, a selected frame, a pixel with one pass, source = 1): over the window
 *      q = p + (di, dj), dj = -r..r (outer), di = -r..r (inner), r = spatial_radius, p itself included, with w = wn * wx:
 *         W = sum w;   m = (sum w * l_q) / W;   v = (sum w * ((l_q - m) * (l_q - m))) / W         (sums from +0, in tap order)
 *      two sweeps over the window, the second with the first's m.  W > 0 does not hold (every feature ray of p missed): v = 0.
 *      The one-sweep form E[l^2] - E[l]^2 is not used: at l = 1e3 with a spread of 1e-2 both of its terms are 1e6, where a
 *      float's ulp is 0.06, and their difference, the variance 1e-4, is lost entirely.  The two-sweep form loses only what
 *      the mean's own rounding costs: with n taps and u = 2^-24 a relative error of at most (n u l / spread)^2 + (n + 2) u,
 *      about 0.1 there for the 7 x 7 window (measured: 1e-4) and ~1e-5 where l is of the spread's size.
 *   4. for iteration it = 0 .. iterations-1, stride s = 2^it, on (c.xyz, v) per pixel, every pixel reading the previous
 *      iteration's values:
 *         gv = (sum G[dj+1] * G[di+1] * v_q) / (sum G[dj+1] * G[di+1])     over the 3 x 3 window q = p + (di, dj) at stride 1
 *                                                        (whatever s is), dj outer, di inner, G = {1/4, 1/2, 1/4}; both sums
 *                                                        (num = num + g * v_q, den = den + g, from +0) over the taps inside the image
 *         a  = (sigma_luminance * sigma_luminance) * gv + epsilon
 *      over ptmi_denoise's 5 x 5 taps q = p + (di * s, dj * s), in its order:
 *         dl = lum(c_p) - lum(c_q);   wl = 1 / (1 + (dl * dl) / a);   w = (((h * wl) * wn) * wx)
 *         W = W + w;   S.ch = S.ch + w * c_q.ch;   V = V + (w * w) * v_q
 *      if W > 0:  c'_p = S / W per channel,  v'_p = (V / W) / W;  else both are kept.  (Two divisions, not V / (W * W): for a
 *      pixel whose taps all but vanish - wn is a 128th power - W * W underflows to 0 while W > 0, and V / 0 is inf or NaN.)
 *      sigma_luminance does not shrink with the iteration: the variance does, and takes the tolerance with it.  The rational
 *      kernel stands in for SVGF's exp, as wc and wx do in ptmi_denoise.
 *   5. remodulation and tone map as ptmi_denoise steps 3 - 4.  variance_in = the v of steps 2 - 3, variance_out = v after the
 *      last iteration, both in the filtered signal's units (radiance / albedo with demodulate).
 * With iterations = 0 the output is the input, as ptmi_denoise's; variance_in is computed all the same and variance_out equals it.
 * NON-FINITE VALUES follow ptmi_denoise's rule (max is fmaxf, a comparison with a NaN is false, the rest is IEEE):
 *   - step 2: max(0, NaN) = 0 - a NaN M2 gives variance 0.
 *   - step 3: a NaN or Inf l_q makes m and v NaN at every p whose window holds q and whose W > 0 (0 * Inf is NaN too); a NaN
 *     n_p or n_q gives wn = 0, a skipped tap; a W that is NaN (a non-finite position of p) fails W > 0: v = 0.
 *   - step 4: a NaN v_q within the 3 x 3 window makes a NaN, a NaN a or l makes w and W NaN, and p keeps (c_p, v_p) of the
 *     previous iteration; a NaN v_q at a tap of finite weight makes v'_p NaN and leaves c'_p alone; an Inf c_q at a finite a_p
 *     gives wl = 0 and w * c_q = NaN: c'_p is NaN in those channels.  Normals and positions act as in ptmi_denoise.
 * A non-finite input pixel can change - and make non-finite - only the pixels within spatial_radius + 2 * (2^iterations - 1) of
 * it in x and in y (with iterations = 0: within spatial_radius, variance alone); every other pixel's colour and variances are
 * bit-identical to a run without it.
 * PTMI_E_INVALID: ptmi_denoise's conditions with ptmi_denoise's messages; ptmi_read_variance without a current result;
 * ptmi_read_pass_moments before the accumulation's first pass.
 * ptmi_read_pass_moments returns the stopping rule's mean, M2 and k per local pixel (pixels that have stopped keep theirs). */
typedef struct {
    int   iterations;        /* 5; 0 .. 10 */
    float sigma_luminance;   /* 2.0; luminance tolerance in standard deviations, 1e-4 .. 1e4 */
    float epsilon;           /* 0.01; added to the luminance tolerance's square (a floor of 0.1 in luminance), 1e-12 .. 1e4 */
    float sigma_position;    /* as ptmi_denoise_params */
    int   normal_squarings;  /* as ptmi_denoise_params */
    int   feature_grid;      /* as ptmi_denoise_params */
    int   demodulate;        /* as ptmi_denoise_params */
    int   source;            /* 0 auto: the accumulation's statistics where they exist, else spatial; 1: always spatial */
    int   spatial_radius;    /* 3 (a 7 x 7 window); 1 .. 3 */
} ptmi_variance_params;
void ptmi_default_variance_params(ptmi_variance_params*);
/* the parameter check of ptmi_denoise_variance alone (no context, no device): 0 or PTMI_E_INVALID with the message */
int  ptmi_check_variance_params(const ptmi_variance_params*);
int  ptmi_denoise_variance(ptmi_ctx*, const ptmi_variance_params* /* NULL: defaults */);
/* the last ptmi_denoise_variance's variances, one float per pixel, local row-major like ptmi_read_image; either may be NULL */
int  ptmi_read_variance(const ptmi_ctx*, float* variance_in, float* variance_out);
/* device time (hipEvents) of the last run's variance estimate (steps 1 - 3) and of its filter (steps 4 - 5), in ms */
int  ptmi_variance_timing(const ptmi_ctx*, double* estimate_ms, double* filter_ms);
/* the stopping test's state of the current accumulation, local row-major; any pointer may be NULL */
int  ptmi_read_pass_moments(const ptmi_ctx*, float* mean, float* m2, uint32_t* passes);

/* ---- temporal accumulation with reprojection (new in this implementation) ------------------------------------------------
 * ptmi_temporal_accumulate blends the current image into a per-pixel HISTORY carried across views: the history of the last
 * view is reprojected into the current one through the feature buffers, accepted where the geometry agrees, and mixed with
 * the current image by sample count (the temporal stage of SVGF, Schied et al. 2017).  The BSDF is Lambertian and the scene
 * static, so a surface point's outgoing radiance does not depend on the view: reprojected history is unbiased except for
 * what the resampling blurs.  The output can then go through the a-trous filter (ptmi_denoise_temporal).
 *
 * INPUTS of a step: the radiance ptmi_read_image would return (it must be current, under ptmi_denoise's rule), its samples
 * per pixel m (config.spp after a frame or a selected frame; after an accumulation pass the pixel's own count,
 * ptmi_read_sample_counts), and the features for params->feature_grid (recomputed first if stale or of another grid, as
 * ptmi_denoise does).  The HISTORY holds per pixel a colour c and a float sample count n, a copy of the features of the
 * view it was last updated in (albedo, normal, position, hit fraction), and that view's camera frame (the 12 floats of
 * ptmi_get_camera_frame) and resolution.
 *
 * THE STEP, per local pixel p, float32 in the order written (-ffp-contract=off, correctly rounded division);
 * dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, cross(a, b) = (a.y*b.z - a.z*b.y, -(a.x*b.z - a.z*b.x), a.x*b.y - a.y*b.x):
 *   0. STILL CAMERA: if the history is not empty and the camera frame and resolution are bit-identical to the history's,
 *      the only tap is p itself with weight 1: h = c_hist(p), n_acc = n_hist(p) (pixels every feature ray missed included);
 *      go to 5.  With max_history large a still camera gives the per-pixel running mean of its frames.
 *   1. RESTART if the history is empty or p's hit fraction hf is 0: c = c_cur, n = m (as they are, no blend); go to 6.
 *   2. x = position / hf, n_c = normal / hf, a_c = albedo / hf (per component, true division: the feature sums count hits only).
 *   3. (o, llc, hor, ver) = the history's camera frame, o_cur = the current one's origin;  f = llc - o;  nrm = cross(hor, ver);
 *      d = x - o;  den = dot(d, nrm);  fn = dot(f, nrm);  sp = dot(n_c, o - x);  sc = dot(n_c, o_cur - x);
 *      unless ((fn > 0 and den > 0) or (fn < 0 and den < 0)) and ((sp > 0 and sc > 0) or (sp < 0 and sc < 0)): no taps
 *      (restart, as 1) - x must lie in front of the previous camera, and both cameras on the same side of the surface (the
 *      two sides of a wall are lit differently);
 *      s = fn / den;  q = s * d - f (per component);  u = dot(q, hor) / dot(hor, hor);  v = dot(q, ver) / dot(ver, ver);
 *      px = u * (float)width - 0.5f;  py = v * (float)height - 0.5f      (width, height: the history's resolution)
 *   4. fx = px - floorf(px), fy = py - floorf(py); the taps, in this order, with weights
 *         (x0, y0): (1 - fx) * (1 - fy);  (x0 + 1, y0): fx * (1 - fy);  (x0, y0 + 1): (1 - fx) * fy;  (x0 + 1, y0 + 1): fx * fy
 *      with x0 = floorf(px), y0 = floorf(py) (global pixels, row 0 = bottom).  A tap t is skipped if it lies outside the image,
 *      if its history hit fraction hf_t is 0, if dot(n_c, n_t) >= normal_min does not hold, if dot(e, e) <= sigma_x * sigma_x
 *      does not hold, or if dot(ea, ea) <= sigma_albedo * sigma_albedo does not hold, where n_t = normal_t / hf_t,
 *      e = x - position_t / hf_t, ea = a_c - albedo_t / hf_t (the history's features, per component; the albedo test keeps
 *      an emitter (Kd = 0) and the surface around it from bleeding into each other through the resampling).  Over
 *      the taps kept, in order, from +0:  W = W + w;  S.ch = S.ch + w * c_t.ch;  Sn = Sn + w * n_t.
 *      If W > 0.01f:  h = S / W per channel, n_acc = Sn / W;  else restart as in 1.
 *   5. n' = min(n_acc + m, (float)max_history * m);  alpha = m / n';  c = h + alpha * (c_cur - h) per channel;  n = n'.
 *   6. radiance = c; rgb8 = the frame's tone map of c (resolve at k = 1, as ptmi_denoise); both to buffers of the step's own
 *      (ptmi_read_temporal).  Then the history becomes the current view's: c, n, the current features, camera frame, resolution.
 *   sigma_x = sigma_position, or for sigma_position <= 0: 0.01f * sqrtf((dx*dx + dy*dy) + dz*dz) with (dx, dy, dz) = max - min
 *   of the root box of the scene's BVH (as ptmi_denoise computes its 2 %).
 * NON-FINITE VALUES.  Every test of steps 3 and 4 is written so that a NaN fails it (">= normal_min does not hold"): a NaN or
 * Inf in p's features or in a tap's leaves the tap, or p, without history - a restart.  A NaN or Inf in a kept tap's colour c_t
 * goes into S and so into c: it travels with the surface point, one bilinear footprint per step, until that point restarts
 * (max_history = 1 does not stop it: alpha = 1 still computes h + (c_cur - h), which is NaN for a NaN h).  Step 5's min is
 * fminf: a NaN n_acc (only from a NaN count in the history, which no step writes) gives n' = max_history * m.  A non-finite
 * c_cur makes c non-finite.  No pixel other than those whose kept taps read a non-finite colour, and p itself for c_cur, is
 * affected.
 * Stats: accepted = pixels whose history was reused (0 or 5), missed = restarts of pixels with hf = 0, rejected = every other
 * restart (an empty history included); they add up to the local pixel count.
 *
 * STATE.  ptmi_set_camera keeps the history.  Every other call that restarts an accumulation empties it: scene loads,
 * ptmi_update_resolution, a successful ptmi_set_config, a successful ptmi_set_environment (the light changes, not the view: there
 * is nothing to reproject), the radiosity setters and solver; so does ptmi_temporal_reset.  A
 * step writes only buffers of its own: frames, passes, streams, the accumulation, the validity of the feature buffers and
 * ptmi_denoise's results are what they would be without it (it may recompute the features, as ptmi_denoise does).
 * ptmi_read_history_counts returns n per local pixel (0 everywhere while the history is empty).
 * ptmi_denoise_temporal runs ptmi_denoise's filter, unchanged, over the history's colour guided by the history's features
 * (its view's albedo, normal, position); the result is read with ptmi_read_denoised.
 * PTMI_E_INVALID: a context tiled over more than one rank (taps cross ranks), the Radiosity integrator, no current image,
 * parameters out of range or NaN; ptmi_denoise_temporal with an empty history or a feature_grid other than the history's. */
typedef struct {
    int   max_history;      /* 32; cap on n in units of the current input's m (alpha >= 1 / max_history); 1 .. 65536 */
    float normal_min;       /* 0.9; a tap is accepted only if n_c . n_t >= normal_min; -1 .. 1 */
    float sigma_position;   /* 0 (<= 0: 1 % of the scene's bounding-box diagonal); else 1e-6 .. 1e12 */
    int   feature_grid;     /* 2; g of the feature pass used for reprojection, 1 .. 4 */
    float sigma_albedo;     /* 0.1; a tap is accepted only if |a_c - a_t|^2 <= sigma_albedo^2; 0 .. 1e6 */
} ptmi_temporal_params;
typedef struct {
    uint64_t accepted, rejected, missed;   /* local pixels: history reused / restarted / restarted, every feature ray missed */
    double   seconds;                      /* device time of the step (the feature pass excluded) */
    double   features_ms;                  /* device time of the feature pass the step ran (0 if none) */
} ptmi_temporal_stats;
void ptmi_default_temporal_params(ptmi_temporal_params*);
/* the parameter check of ptmi_temporal_accumulate alone (no context, no device): 0 or PTMI_E_INVALID with the message */
int  ptmi_check_temporal_params(const ptmi_temporal_params*);
int  ptmi_temporal_reset(ptmi_ctx*);
int  ptmi_temporal_accumulate(ptmi_ctx*, const ptmi_temporal_params* /* NULL: defaults */, ptmi_temporal_stats* /* may be NULL */);
/* the last step's result, local row-major like ptmi_read_image; either may be NULL */
int  ptmi_read_temporal(const ptmi_ctx*, unsigned char* rgb8, float* radiance);
/* the history's sample count n per local pixel, local row-major */
int  ptmi_read_history_counts(const ptmi_ctx*, float* counts);
int  ptmi_denoise_temporal(ptmi_ctx*, const ptmi_denoise_params* /* NULL: defaults */);

/* ---- temporal luminance statistics: the history steers the variance filter (new in this implementation) -------------------
 * ptmi_set_temporal_moments(ctx, 1) makes the history carry, per pixel, the weighted mean and variance of the luminances that
 * went into it and the number of frames behind it; ptmi_denoise_temporal_variance is ptmi_denoise_variance's filter over the
 * history with that variance in the place of the accumulation's (the temporal and spatial stages of SVGF joined).  The switch
 * belongs to the context and is kept over scene loads, as ptmi_set_feature_shading's flags are; the default is 0.  A call that
 * changes the value empties the history, as ptmi_temporal_reset does, and changes nothing else (image, accumulation, features and
 * the denoiser's results stay); a call with the current value does nothing; a value other than 0 and 1 is PTMI_E_INVALID.
 * With 0 nothing of this section runs or is allocated and ptmi_temporal_accumulate is, bit for bit, what it is without it.
 *
 * With 1, each side of the history's ping-pong gains one float4 per pixel, (mu, s2, k, 0): mu the weighted mean luminance of the
 * inputs behind the pixel, s2 their weighted population variance, k the number of frames behind it (a float).  They are
 * allocated by the first step that needs them, freed with the history's other buffers and empty whenever the history is.
 *
 * ADDITION TO THE STEP of ptmi_temporal_accumulate, float32 in the order written; lum is ptmi_denoise's:
 *   l = lum(c_cur).
 *   RESTART (steps 1, 3 and 4, whatever the reason):  mu = l;  s2 = +0;  k = 1.
 *   STILL CAMERA (step 0):  mu_h, s2_h, k_h = the pixel's own.
 *   REPROJECTED (step 4): over the taps kept for the colour, in the same order and with the same weights w, from +0:
 *      Sm = Sm + w * mu_t;  Ss = Ss + w * s2_t;  Sk = Sk + w * k_t;   then  mu_h = Sm / W;  s2_h = Ss / W;  k_h = Sk / W.
 *   BLEND, with step 5's own alpha = m / n':
 *      d = l - mu_h;   mu = mu_h + alpha * d;   s2 = (1 - alpha) * (s2_h + alpha * (d * d));
 *      k = fminf(k_h + 1, (float)max_history).
 * This is West's weighted incremental variance (1979) in blend form: with weights m_i and an uncapped history s2 is the population
 * variance of the inputs' luminances (Welford's M2 / n for equal m); once max_history binds alpha is constant and s2 is the
 * exponentially weighted variance.  The raw-moment form E[l^2] - E[l]^2 is not used, for the reason given under
 * ptmi_denoise_variance step 3: carried over 2 .. 32 frames of 627 pixels it is off by up to 2e-5 of the variance at l = 1 +- 0.2
 * and by 4e3 x the variance at l = 1e3 +- 1e-2, where the blend form stays within 8e-7 and 8e-3 (the input's own quantisation) of
 * binary64 (tests/test_temporal_moments_host.py).
 * The bilinear resampling of s2 ignores the spread between the taps' means (the variance of a mixture is the mean variance plus
 * the variance of the means); SVGF does the same.
 * NON-FINITE VALUES, from IEEE arithmetic and fminf: a non-finite c_cur makes mu and s2 non-finite, and they travel with that
 * surface point only, as a non-finite colour does; a NaN k_h gives k = max_history; alpha = 1 (max_history = 1) gives
 * s2 = 0 * (...), which is 0, or NaN for a non-finite operand.
 * ptmi_read_temporal_moments returns (mu, s2, k) of the history, local row-major, any pointer may be NULL.
 *
 * ptmi_denoise_temporal_variance runs THE FILTER of ptmi_denoise_variance, steps 1 and 3 - 5 unchanged, over the history's
 * colour guided by the history's features, exactly as ptmi_denoise_temporal does for ptmi_denoise.  Step 2 is replaced by
 *   2. TEMPORAL VARIANCE, with source = 0, where the pixel has k >= PTMI_TEMPORAL_MIN_FRAMES (SVGF's choice):
 *         v  = fmaxf(0, s2 / (k - 1))                    the variance of the mean of k equally weighted frames;
 *         lr = lum(history colour_p);  if lr > 0:  s = l_p / lr;  v = (v * s) * s      (the unit conversion of step 2)
 *      Every other pixel (a NaN k included), and every pixel with source = 1, takes the spatial estimate of step 3.
 * Once max_history binds the mean is exponential and its variance is sigma^2 alpha / (2 - alpha), about half of sigma^2 / (k - 1)
 * at k = max_history: the estimate is then about 2 x too large; for unequal m it is approximate as well.  It errs towards more
 * blur, never towards a negative or zero tolerance (fmaxf(0, NaN) = 0; epsilon keeps the tolerance positive).
 * Results: ptmi_read_denoised and ptmi_read_variance; ptmi_variance_timing times it.  A ptmi_denoise_temporal or
 * ptmi_denoise_variance after it gives what it gives alone.
 * ptmi_debug_set_temporal_moments (test hook) overwrites (mu, s2, k) of the history's current side, local row-major, with
 * unchecked values (non-finite ones are legitimate) and touches nothing else: with ptmi_debug_set_filter_inputs every decision
 * above can be reached on constructed state.  It has no kernel: a host-side interleave and one copy.
 * PTMI_E_INVALID: ptmi_read_temporal_moments, ptmi_denoise_temporal_variance and ptmi_debug_set_temporal_moments with the switch
 * off or the history empty; ptmi_denoise_temporal_variance with a feature_grid other than the history's or parameters
 * ptmi_check_variance_params refuses (its messages); a NULL array for the hook. */
#define PTMI_TEMPORAL_MIN_FRAMES 4.0f
int  ptmi_set_temporal_moments(ptmi_ctx*, int on);
int  ptmi_get_temporal_moments(const ptmi_ctx*, int* on);
int  ptmi_read_temporal_moments(const ptmi_ctx*, float* mean, float* variance, float* frames);
int  ptmi_denoise_temporal_variance(ptmi_ctx*, const ptmi_variance_params* /* NULL: defaults */);
int  ptmi_debug_set_temporal_moments(ptmi_ctx*, const float* mean /* n */, const float* variance /* n */, const float* frames /* n */);

/* ---- next-event estimation with multiple importance sampling (new in this implementation) --------------------------------------
 * ptmi_config.next_event = 1: at every path vertex a point on an emitter is sampled and one shadow ray traced to it, and the power
 * heuristic combines that sample with the BSDF sample (Veach 1997), so the estimator stays unbiased.  It applies to
 * ptmi_render_frame, ptmi_render_frames (ptmi_select_frame as usual), ptmi_accum_pass (progressive and adaptive: a pass continues
 * the pixel's sums) and tiled contexts (streams are keyed by the global pixel); ptmi_denoise, ptmi_temporal_accumulate and
 * ptmi_gather_frame take the NEE image as they take any other.  Colour sums, the resolve and the tone map are a frame's; a pixel's
 * RNG stream carries over between frames as it does without NEE.  One launch runs every queued pixel's samples to their end.
 *
 * THE EMITTER TABLE (built by both scene loaders, ptmi_host_emitters), in the order written (-ffp-contract=off):
 *     area_i = Triangle/Quad::area (triangle.h:28, quad.h:31: 0.5f * length(cross(v1 - v0, v2 - v0)) for a triangle,
 *              0.5f * (length(cross(v10 - v00, v01 - v00)) + length(cross(v11 - v10, v11 - v01))) for a quad), float32
 *     ng_i   = unit_vector(cross(v1 - v0, v2 - v0)) for a triangle, unit_vector(cross(v10 - v00, v01 - v00)) for a quad, float32
 *              (vector.h:205-218): the GEOMETRIC normal, whatever the stored normal is
 *     the candidates are the primitives with a finite ng_i, in load order; a quad only if it is planar,
 *              fabsf(dot(ng_i, v11 - v00)) <= 1e-4f * length(v11 - v00) (the walk splits a quad along v00-v11, sampleUniform
 *              along v10-v01: only for a planar quad do both cover one surface)
 *     w_i    = area_i * ((Le.x + Le.y) + Le.z), float32
 *     the emitters are the candidates with w_i > 0 whose weight the running sum does not absorb: c_j = c_{j-1} + w_j from
 *              c_{-1} = +0, and a candidate with c + w == c (select() could never return it) is skipped; total = c_last;
 *              pdf_area_j = (w_j / total) / area_j; every other primitive has pdf_area = 0
 *     OVERFLOW: if some candidate's w_i > FLT_MAX or c + w_i > FLT_MAX, the table is built in binary64 instead:
 *              W_i = (double)area_i * (((double)Le.x + Le.y) + Le.z) over the candidates with 0 < W_i < inf, C_k their running
 *              sum from 0, T = C_last; c_j = (float)(C_k / T), skipping a candidate whose c rounds to the one before;
 *              pdf_area_j = (float)((W_j / T) / area_j); total = 1.  Le up to FLT_MAX keeps a finite table.
 *     select(u), u in (0, 1]: the smallest j with u * total <= c_j
 *
 * THE ESTIMATOR, per sample.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; c * (a, b, c) and a * b per component; x / PI =
 * (float)((double)x / M_PI); mis(a, b) = misPowerHeuristic (integrator.h:91-96): 0 if a <= 0, else (a*a) / (a*a + b*b).
 * The camera ray and its two draws are exactly a frame's; beta = (1, 1, 1), L = (0, 0, 0), p_b_prev = 0.  For depth = 0 ..
 * max_depth - 1, as integrator.h:189-268 (all draws curand_uniform of the pixel's stream):
 *   1. the reference's closest hit of (o, d) for t > 1e-4; none: the sample ends.  Primitive k, stored normal n_k, Kd, Le_k,
 *      p = o + t * d.  If depth >= 1 and pdf_area_k > 0:
 *          p_l = (pdf_area_k * (t * t)) / fabsf(dot(ng_k, d));   w = mis(p_b_prev, p_l);   L = L + (beta * Le_k) * w
 *      else (depth 0, or not an emitter):  L = L + beta * Le_k
 *   2. depth > 2: Russian roulette with one draw; beta = beta * Kd; the |beta| < 1e-5 exit - all exactly as the reference.
 *      sn = dot(d, n_k) < 0 ? n_k : -n_k;  o' = p + 1e-4f * sn   (the reference's spawn point, integrator.h:266)
 *   3. NEE, if depth + 1 < max_depth and the scene has an emitter.  ALWAYS three draws, u_sel, r1, r2, in this order, whatever
 *      comes of them:  j = select(u_sel);  y = Primitive::sampleUniform of emitter j with (r1, r2) (primitive.h:150-191);
 *          v = y - o';  dist2 = dot(v, v);  dist = sqrtf(dist2);  wi = (v.x / dist, v.y / dist, v.z / dist)
 *          cos_s = dot(sn, wi);  cos_l = fabsf(dot(ng_j, wi));  p_l = (pdf_area_j * dist2) / cos_l     ng_j: the table's
 *      if cos_s > 0, cos_l > 0 and 0 < p_l <= FLT_MAX (a p_l of 0 or inf weighs 0), and the reference's closest hit of (o', wi)
 *      for t > 1e-4 is emitter j itself (the same walk as the path rays):
 *          p_b = cos_s / PI;  w = (p_b * mis(p_l, p_b)) / p_l;  L = L + (beta * Le_j) * w
 *   4. two draws u, v; depth = depth + 1; if depth < max_depth:  next = sampleCosineHemisphere(sn, u, v) (integrator.h:62-85),
 *      p_b_prev = fmaxf(dot(sn, next), 0) / PI,  o = o',  d = unit_vector(next); else the sample ends.
 * At the end of the sample colour = colour + L (integrator.h:390).
 * The two MIS weights of an emitter point sum to 1 wherever both strategies can produce it, so every pixel's expected value is
 * that of the reference's estimator.  Both pdfs convert area to solid angle with the geometric normal ng, so this holds for any
 * stored normal (the loaders store a corner's vn or N, smooth normals included); the stored normal keeps its role on the
 * shading side (sn, the cosine lobe), as in the reference.  A primitive that is no emitter (a non-planar quad, an absorbed
 * weight) is found by BSDF samples alone, with weight 1.  Without an emitter in the scene NEE draws nothing and a frame is the
 * reference's frame. */

/* ---- environment lighting: an importance-sampled lat-long radiance map (new in this implementation) -----------------------------
 * Without an environment a ray that leaves the geometry ends its sample and adds nothing.  ptmi_set_environment gives the
 * context a radiance map over all directions: a path ray that misses looks it up, and with ptmi_config.next_event = 1 the map is
 * also a light that every vertex can sample, combined with the BSDF sample by the power heuristic as the emitters are.  The map
 * belongs to the context, like the camera: it survives scene loads.  Frames, batches, passes (progressive and adaptive), tiled
 * contexts, ptmi_denoise, ptmi_temporal_accumulate and ptmi_gather_frame work as they do without one; a context with an
 * environment renders both values of next_event through the per-lane kernel of next-event estimation, so segments_per_launch,
 * wave_tiles, streams and collect_stats have no effect on it (see ptmi_config.next_event).  Without an environment nothing in
 * the library behaves differently.
 *
 * ptmi_set_environment: rgb holds height * width * 3 floats, row 0 at +y, rows top to bottom; NULL drops the environment
 * (width, height and the parameters are then ignored).  A successful call restarts an accumulation, makes features stale and
 * empties the temporal history.  PTMI_E_INVALID, with nothing changed: width or height < 1, width * height > 2^25, a texel
 * that is negative, NaN or infinite before or after the scale, a total power that overflows float, parameters out of range
 * (scale finite and >= 0, rotation_deg in [-360, 360], select_fraction in [0, 1]), and a current config with integrator = 1,
 * sampling_mode != 0 or fast_tree = 1; ptmi_set_config rejects those three while an environment is set (the restrictions of
 * next_event, for the same reasons).  ptmi_environment_info: 0 x 0 and total 0 without one.
 *
 * THE MAP, w x h texels.  Rows are bands of equal cos(theta) boundaries, columns divide phi evenly; y is up:
 *     z_r     = (float)cos(pi r / h): the cosine ptmi_sincos_d gives for (PTMI_PI_D * (double)r) / (double)h, r = 0 .. h;
 *               z_0 = 1, z_h = -1 exactly
 *     rot     = rotation_deg / 360.0f (float): column 0 starts at the angle 2 pi rot from +x towards +z
 *     E_rj    = rgb * scale per channel (float)
 *     Omega_r = ((2.0 * PTMI_PI_D) / (double)w) * ((double)z_r - (double)z_{r+1})          the solid angle of a texel of row r
 * THE LOOKUP texel(d) of a direction d, float32 in the order written (nearest texel: radiance is piecewise constant, so the
 * sampling density below is exactly proportional to what is looked up):
 *     y = fminf(fmaxf(d.y, -1), 1);   r = the smallest r in 0 .. h-1 with z_{r+1} < y, or h - 1 if there is none (y = -1)
 *     phi = atan2f(d.z, d.x);  s = (float)((double)phi / (2.0 * PTMI_PI_D));  t = s - rot;  t = t - floorf(t)
 *     j = min((int)(t * (float)w), w - 1)                     (atan2f, sincosf here and below: ptmi_math.h's ptmi_atan2f, ptmi_sincosf)
 * THE TABLE (ptmi_host_env_table; built on the host at every ptmi_set_environment and uploaded), binary64 unless it says float:
 *     W_rj = Omega_r * (((double)E.x + (double)E.y) + (double)E.z)                         (the emitter table's channel sum)
 *     R_rj = R_r,j-1 + W_rj from 0 (row running sums), T_r = R_r,w-1;  M_r = M_{r-1} + T_r from 0,  total = (float)M_{h-1}
 *     c_rj = (float)(R_rj / T_r) if T_r > 0, else 0;   m_r = (float)(M_r / M_{h-1}) if M_{h-1} > 0, else 0
 *            (float CDFs that end at exactly 1; a row or a map of weight 0 keeps zeros and can never be selected)
 *     P_rj = ((double)m_r - (double)m_{r-1}) * ((double)c_rj - (double)c_r,j-1)            m_{-1} = c_r,-1 = 0
 *     pdf_rj = (float)(P_rj / Omega_r) if P_rj > 0, else 0
 * P_rj is the probability with which the two searches below pick texel (r, j) - differences of the STORED floats - so pdf is
 * the sampler's density per solid angle whatever rounding the CDFs took.  A texel or row whose CDF step rounds to nothing has
 * pdf 0: it is found by BSDF samples alone, with weight 1 (the emitter table's rule for absorbed weights).  total == 0 (an
 * all-black map, scale = 0): the environment is never sampled and no draw is made for it.
 * texel (ptmi_host_env_table): h * w * 4 floats (E.x, E.y, E.z, pdf); z: h + 1; marginal_cdf: h; row_cdf: h * w.
 *
 * THE ESTIMATOR is that of "next-event estimation" above (with next_event = 0: the reference's, integrator.h:189-268, with its
 * draws) with these changes; beta, L, p_b_prev, sn, o', mis, x / PI and dot as written there.
 *   1'. the closest-hit walk of (o, d) finds nothing:  (E, pdf) = texel(d);  the sample ends after
 *          next_event = 1, total > 0 and depth >= 1:   w = mis(p_b_prev, q * pdf);   L = L + (beta * E) * w
 *          else:                                       L = L + beta * E          (beta = (1, 1, 1) at depth 0: the background)
 *       next_event = 0 changes nothing else, so an all-zero map gives the bits of a frame without a map.
 *   With next_event = 1 and total > 0 ("the environment is sampled"; otherwise steps 1 and 3 are exactly those above and a frame
 *   with an all-zero map is bit-identical to the NEE frame without one):
 *       q = 1 if the scene has no emitter, else select_fraction
 *   1.  an emitter found at depth >= 1 weighs  w = mis(p_b_prev, (1.0f - q) * p_l)
 *   3'. if depth + 1 < max_depth: ALWAYS five draws u_sel, r1, r2, r3, r4, in this order, whatever comes of them.
 *       If u_sel <= q, the environment:
 *          r = the smallest row with r1 <= m_r;   j = the smallest column with r2 <= c_rj
 *          ct = z_{r+1} + r3 * (z_r - z_{r+1});   st = sqrtf(fmaxf(0, 1 - ct * ct))
 *          a = ((float)j + r4) / (float)w + rot;  (sp, cp) = sincosf((float)((2.0 * PTMI_PI_D) * (double)a))
 *          wi = (st * cp, ct, st * sp);   (E, pdf) = texel (r, j) itself, no second lookup
 *          cos_s = dot(sn, wi);  p_e = q * pdf
 *          if cos_s > 0, 0 < p_e <= FLT_MAX, and the reference's closest-hit walk of (o', wi) for t > 1e-4 finds nothing:
 *              p_b = cos_s / PI;  w = (p_b * mis(p_e, p_b)) / p_e;  L = L + (beta * E) * w
 *       else the emitter table, step 3 above with u' = (u_sel - q) / (1.0f - q) in place of u_sel and
 *          p_l' = (1.0f - q) * p_l in place of p_l, in the test 0 < p_l' <= FLT_MAX and in the weight.
 *       A strategy whose selection probability is 0 is never drawn (u_sel is in (0, 1]) and weighs nothing: mis(a, 0) = 1.
 * The two MIS weights of a direction sum to 1 wherever both strategies can produce it - a missed direction by the BSDF sample
 * (density p_b) and by the environment sample (q * pdf), an emitter point by the BSDF sample and by the emitter sample
 * ((1 - q) * p_l) - so every pixel's expected value is that of the estimator without next_event.  A sampled direction looks up
 * its own texel except where rounding puts it on a texel boundary; its E and pdf are the sampled texel's either way. */
typedef struct {
    float scale;            /* 1: every texel is multiplied by it on upload (float), >= 0, finite */
    float rotation_deg;     /* 0: the map turned about +y, [-360, 360] */
    float select_fraction;  /* 0.5: with next_event, the probability q that a vertex's light sample goes to the
                               environment and not to the emitter table; in [0, 1] */
} ptmi_env_params;
void ptmi_default_env_params(ptmi_env_params*);
/* the parameter check of ptmi_set_environment alone (no context, no device): 0 or PTMI_E_INVALID with the message */
int  ptmi_check_env_params(const ptmi_env_params*);
int  ptmi_set_environment(ptmi_ctx*, int width, int height, const float* rgb /* h*w*3, row 0 = +y; NULL drops it */,
                          const ptmi_env_params* /* NULL: defaults */);
int  ptmi_environment_info(const ptmi_ctx*, int* width, int* height, float* total);   /* 0 x 0 without one */
/* host-only: the sampling table of a map, for inspection and CPU tests (any output pointer may be NULL) */
int  ptmi_host_env_table(int width, int height, const float* rgb, const ptmi_env_params* /* NULL: defaults */,
                         float* z /* h+1 */, float* marginal_cdf /* h */, float* row_cdf /* h*w */,
                         float* texel /* h*w*4: scaled rgb, pdf per solid angle */, float* total);

/* ---- specular surfaces: mirror and glass (new in this implementation) ----------------------------------------------------------
 * Every surface the loaders produce is Lambertian.  ptmi_set_surfaces gives the loaded scene a table with one kind per
 * primitive, in load order as ptmi_set_radiosity: diffuse (today's surface), a perfect mirror, or smooth glass with an index of
 * refraction.  The primitive's bsdf colour is the specular tint: Kr of a mirror, and on glass it tints reflection and
 * transmission alike.  Le is added as on any surface.  The table indexes primitives, so a scene load drops it (the environment,
 * which belongs to the context, survives one).  A table whose kinds are all 0 is no table: the context takes exactly the route
 * it takes without one.  A context whose table has a specular primitive renders both values of next_event through the per-lane
 * kernel of next-event estimation, as a context with an environment does (so segments_per_launch, wave_tiles, streams and
 * collect_stats have no effect on it); frames, batches, passes (progressive and adaptive), tiled contexts, ptmi_denoise,
 * ptmi_temporal_accumulate and ptmi_gather_frame work as they do without one.
 * ptmi_run_radiosity_solver, the Radiosity view (integrator = 1) and ptmi_render_features IGNORE the table: the solver and the
 * view treat every primitive as the diffuse surface its bsdf describes, and the feature pass keeps reporting bsdf as albedo.
 *
 * ptmi_set_surfaces: kind NULL drops the table (n_prims and ior are then ignored); ior NULL means 1.5 for every primitive.  A
 * successful call restarts an accumulation, makes features stale and empties the temporal history.  PTMI_E_INVALID, with nothing
 * changed: no scene loaded, n_prims != ptmi_scene_info's count, a kind outside 0 .. 2, an ior that is NaN, infinite or outside
 * [1, 8] (every entry is checked; it is READ for glass only), and - for a table with a specular primitive - a current config with
 * integrator = 1, sampling_mode != 0 or fast_tree = 1; ptmi_set_config rejects those three while such a table is set (the
 * restrictions of an environment, for the same reasons).  ptmi_check_surfaces makes the checks that need no context (n_prims >= 1,
 * kind not NULL, the kinds, the iors).  ptmi_surfaces_info: the table's mirror and glass primitives, 0 and 0 without a table.
 *
 * THE ESTIMATOR is that of "next-event estimation" and "environment lighting" above (with next_event = 0: the reference's, with
 * its draws), float32 in the order written, sqrtf correctly rounded and / the IEEE quotient; beta, L, p_b_prev, sn, o', dot, mis
 * as written there; kind_k and ior_k are primitive k's entries.  A sample carries one more flag, spec_prev = false at the camera.
 *   1.  An emitter found while spec_prev is set counts in full, as at depth 0: L = L + beta * Le_k, no MIS weight (no light
 *       sample could have produced it).  1'. likewise: a path ray that leaves the scene while spec_prev is set adds beta * E.
 *   2.  Russian roulette, beta = beta * bsdf_k, the |beta| < 1e-5 exit, sn and o' are unchanged: a specular vertex is a vertex.
 *   A vertex with kind_k = 0 then goes on with steps 3 (3') and 4 exactly as above, draw for draw, and sets spec_prev = false.
 *   A vertex with kind_k != 0 makes none of the draws of step 3 (3') and traces no shadow ray, makes neither draw of step 4, and:
 *       un = unit_vector(sn)                 (stored normals may be tilted against the geometry and need not have unit length)
 *       dn = dot(d, un)
 *       mirror (kind 1), no draw:            reflect
 *       glass (kind 2), ALWAYS one draw u, made here, whatever comes of it:
 *           eta = dot(d, n_k) < 0 ? 1.0f / ior_k : ior_k       the ratio n_i / n_t; the stored normal points out of the body
 *           ci = fminf(1, -dn);   s2 = (eta * eta) * fmaxf(0, 1 - ci * ci)
 *           if s2 >= 1 and eta != 1: reflect (total internal reflection); else
 *               ct = eta == 1 ? ci : sqrtf(1 - s2)      (ior 1 is no interface: rs = rp = F = 0 and next = d + 0 * un, so d
 *                                                         exactly at every angle; 1 - s2 would form ci^2 as 1 - (1 - ci * ci)
 *                                                         and lose it near grazing incidence, where s2 even rounds to 1;
 *                                                         at ci = 0 F is 0 / 0, u <= F is false: refract, next = d)
 *               rs = (eta * ci - ct) / (eta * ci + ct);   rp = (ci - eta * ct) / (ci + eta * ct)
 *               F = 0.5f * (rs * rs + rp * rp)
 *               if u <= F: reflect; else refract
 *       depth = depth + 1; if depth >= max_depth the sample ends (after the draw, as step 4 ends it after its two)
 *       reflect:   next = d - (2 * dn) * un,                 o = o' = p + 1e-4f * sn
 *       refract:   next = eta * d + (eta * ci - ct) * un,    o = p - 1e-4f * sn
 *       len2 = dot(next, next): unless len2 > 0 and len2 <= FLT_MAX the sample ends here, before anything is traced (a zero or
 *       non-finite stored normal: no walk is ever started with a NaN direction)
 *       d = unit_vector(next);  spec_prev = true;  p_b_prev keeps its value (it is not read while spec_prev is set)
 * Choosing reflection with probability F and transmission with 1 - F cancels the Fresnel factor, so beta takes only the tint.
 * Transmitted radiance is NOT scaled by eta^2 (the change of solid angle across the interface).  That is exact whenever the
 * camera and every light are outside closed glass bodies - each path then crosses as often inwards as outwards and the factors
 * cancel - and it is what this estimator assumes.  A light sample is never aimed through glass or at a mirror's image: light that
 * reaches a diffuse surface through a specular one is found by BSDF sampling alone, for both values of next_event, and both
 * count vertices alike, so their expected values are equal. */
#define PTMI_SURFACE_DIFFUSE 0
#define PTMI_SURFACE_MIRROR  1
#define PTMI_SURFACE_GLASS   2
/* host only, no context: 0 or PTMI_E_INVALID with the message */
int  ptmi_check_surfaces(int n_prims, const int* kind, const float* ior /* NULL: none to check */);
int  ptmi_set_surfaces(ptmi_ctx*, int n_prims, const int* kind /* NULL drops the table */, const float* ior /* NULL: 1.5 everywhere */);
int  ptmi_surfaces_info(const ptmi_ctx*, int* n_mirror, int* n_glass);   /* 0, 0 without a table */

/* ---- rough metal: a GGX surface kind with light sampling and MIS (new in this implementation) -----------------------------------
 * PTMI_SURFACE_ROUGH is an isotropic GGX microfacet reflector with height-correlated Smith masking, sampled by visible normals
 * (Heitz 2018); the primitive's bsdf colour is a constant tint, as on the mirror (no angle-dependent Fresnel, no energy
 * compensation for multiple scattering).  Unlike mirror and glass it TAKES light samples, towards emitters and the environment.
 * ptmi_set_surfaces_rough is ptmi_set_surfaces with kinds 0 .. 3 and one more array: roughness (NULL: 0.3 for every primitive),
 * every entry finite and in [0.05, 1] (every entry is checked; it is READ for kind 3 only; below 0.05 the mirror is the right
 * tool).  alpha = roughness * roughness, in float, computed on the host.  Everything "specular surfaces" says of ptmi_set_surfaces
 * holds for it unchanged: the state a successful call resets, the configs refused while a table with a non-diffuse primitive is
 * set and the call refused under them, the scene load that drops the table, "an all-diffuse table is no table", the route frames
 * take.  ptmi_set_surfaces and ptmi_check_surfaces keep rejecting kind 3.  ptmi_check_surfaces_rough makes the checks that need
 * no context.  ptmi_surface_counts: the table's primitives of kind 0 .. 3, all 0 without a table; ptmi_surfaces_info keeps
 * reporting the mirror and glass counts of whatever table is set.  A context whose table has no rough primitive renders exactly
 * what it rendered before this kind existed.
 *
 * THE ESTIMATOR is that of "specular surfaces", float32 in the order written, sqrtf correctly rounded, / the IEEE quotient,
 * sincosf = ptmi_sincosf; a + b + c = (a + b) + c, a * b * c = (a * b) * c, also per component of vectors; dot, mis, beta, L,
 * p_b_prev, sn, o' as written above; unit_vector(v) = v * (1.0f / sqrtf(dot(v, v))) (vector.h); cross(a, b) = (a.y*b.z - a.z*b.y,
 * -(a.x*b.z - a.z*b.x), a.x*b.y - a.y*b.x); PI = (float)PTMI_PI_D; alpha and a2 = alpha * alpha are primitive k's.
 * Steps 1 and 2 are unchanged: emission, roulette, beta = beta * bsdf_k, the |beta| < 1e-5 exit, sn and o'.  A vertex with
 * kind_k = 3 then sets spec_prev = false and:
 *   frame    un = unit_vector(sn);  (T, B) is the tangent frame sampleCosineHemisphere (integrator.h:62-85) builds from un:
 *                if un.z < -0.9999999f:  T = (0, -1, 0), B = (-1, 0, 0)
 *                else a = 1.0f / (1.0f + un.z);  b = -un.x * un.y * a;
 *                     T = (1.0f - un.x * un.x * a, b, -un.x);  B = (b, 1.0f - un.y * un.y * a, -un.y)
 *            wo = (dot(-d, T), dot(-d, B), dot(-d, un));  co = wo.z
 *            ok(c) := c > 0 and c * c > PTMI_ROUGH_MIN_COS2       (false for a NaN)
 *            Lambda(c) = 0.5f * (sqrtf(1.0f + a2 * ((1.0f - c * c) / (c * c))) - 1.0f)
 *            D(h), h a unit half vector: t = (h.x * h.x + h.y * h.y) + a2 * (h.z * h.z);  D = a2 / (PI * t * t)
 *                (t is h.z^2 (a2 - 1) + 1; that form cancels at the peak of a narrow lobe, where t is about a2, and at roughness
 *                0.05 leaves D with an error of several per cent)
 *   draws    the light-sample draws of step 3 (3') under exactly a diffuse vertex's condition, then two draws u1, u2 (the u, v of
 *            step 4), then depth = depth + 1 and the depth test: a path's draws depend only on the kinds it meets, and a rough
 *            vertex draws what a diffuse one draws.
 *   grazing  if ok(co) does not hold (grazing incidence, a zero or non-finite stored normal) the vertex makes no light sample and
 *            no BSDF sample: the path ends after the draws and the depth count.
 *   light sample towards wi (an emitter's point or an environment direction), in place of p_b = cos_s / PI and its weight; the
 *            visibility walk and the tests cos_s > 0 (with sn as stored), cos_l > 0, 0 < p_l <= FLT_MAX stay as they are:
 *                wl = (dot(wi, T), dot(wi, B), dot(wi, un));  ci = wl.z;  the sample needs ok(ci)
 *                h = unit_vector(wo + wl)
 *                g   = D(h) / ((4.0f * co) * (1.0f + Lambda(co) + Lambda(ci)))           f * cos / tint
 *                p_b = D(h) / ((4.0f * co) * (1.0f + Lambda(co)))                        the density of the BSDF sample below
 *                w = (g * mis(p_l, p_b)) / p_l;  L = L + (beta * Le_j) * w;  with p_e and E for the environment likewise
 *   BSDF sample, after the depth test:
 *                vh = unit_vector((alpha * wo.x, alpha * wo.y, wo.z))
 *                l2 = vh.x * vh.x + vh.y * vh.y;  T1 = l2 > 0 ? (-vh.y / sqrtf(l2), vh.x / sqrtf(l2), 0) : (1, 0, 0);  T2 = cross(vh, T1)
 *                r = sqrtf(u1);  (sp, cp) = sincosf((float)((2.0 * PTMI_PI_D) * (double)u2));  t1 = r * cp;  t2 = r * sp
 *                s = 0.5f * (1.0f + vh.z);  t2 = (1.0f - s) * sqrtf(fmaxf(0, 1.0f - t1 * t1)) + s * t2
 *                nh = t1 * T1 + t2 * T2 + sqrtf(fmaxf(0, 1.0f - t1 * t1 - t2 * t2)) * vh
 *                h = unit_vector((alpha * nh.x, alpha * nh.y, fmaxf(0, nh.z)))
 *                wl = (2.0f * dot(wo, h)) * h - wo;  ci = wl.z;  unless ok(ci) the path ends (the sample went below the horizon)
 *                beta = beta * ((1.0f + Lambda(co)) / (1.0f + Lambda(co) + Lambda(ci)))
 *                p_b_prev = D(h) / ((4.0f * co) * (1.0f + Lambda(co)))
 *                next = wl.x * T + wl.y * B + wl.z * un;  len2 = dot(next, next): unless len2 > 0 and len2 <= FLT_MAX the path ends
 *                o = o';  d = unit_vector(next)
 *            A path that ends here keeps the light sample it has just made.  What the next ray finds - an emitter, or the
 *            environment - is weighed mis(p_b_prev, ...) by steps 1 and 1'.
 * g / p_b is exactly the weight beta takes, so the two MIS weights of a direction sum to 1 and both values of next_event have
 * the same expected value; the weight is at most 1 (energy lost to masking is not put back).  PTMI_ROUGH_MIN_COS2 keeps
 * (1 - c * c) / (c * c) finite (c * c may otherwise be a subnormal number whose quotient overflows, and the weight would be
 * inf / inf), whatever the device does with subnormal numbers; it ends paths that meet the surface at less than 3.2e-19 rad.
 * D(h) >= a2 / PI > 0 up to rounding, so p_b > 0.  p_b <= 1 / (2 PI alpha^3) (the largest D, 1 / (PI a2), at normal incidence gives
 * 1 / (4 PI a2); towards grazing 4 co (1 + Lambda(co)) falls to its limit 2 alpha), which is 1.02e7 at roughness 0.05: no
 * square in mis overflows. */
#define PTMI_SURFACE_ROUGH 3
#define PTMI_ROUGH_MIN_COS2 1e-37f
/* host only, no context: 0 or PTMI_E_INVALID with the message */
int  ptmi_check_surfaces_rough(int n_prims, const int* kind, const float* ior /* NULL: none to check */, const float* roughness /* NULL: none to check */);
int  ptmi_set_surfaces_rough(ptmi_ctx*, int n_prims, const int* kind /* NULL drops the table */, const float* ior /* NULL: 1.5 everywhere */,
                             const float* roughness /* NULL: 0.3 everywhere */);
int  ptmi_surface_counts(const ptmi_ctx*, int counts[4]);   /* primitives of kind 0 .. 3; all 0 without a table */

/* ---- vertex normals: per-corner normals interpolated at path vertices (new in this implementation) ------------------------------
 * The loaders keep ONE normal per primitive, as the reference does, so a tessellated sphere shades as a polyhedron.
 * ptmi_set_vertex_normals gives the loaded scene a table of corner normals, n_prims x 4 x 3 floats in load order, a primitive's
 * corners in the order of ptmi_load_scene_arrays' verts (v0 v1 v2 | v00 v10 v11 v01); a triangle's 4th entry is ignored.  The
 * table belongs to the scene exactly as the surface table does: a scene load drops it.
 *
 * FLAT AND SMOOTH.  A primitive is flat when every corner normal that is read (3 for a triangle, 4 for a quad) compares equal
 * (==, component for component, so -0.0 equals 0.0) to its stored normal; otherwise it is smooth.  A flat primitive's vertex takes
 * the stored normal, untouched.  A table without a smooth primitive is no table: the context takes exactly the route it takes
 * without one.  A context whose table has a smooth primitive renders both values of next_event through the per-lane kernel of
 * next-event estimation, as a context with an environment or a specular surface does; frames, batches, passes, tiled contexts,
 * ptmi_denoise, ptmi_temporal_accumulate and ptmi_gather_frame work as they do without one.
 * ptmi_run_radiosity_solver and the Radiosity view (integrator = 1) ignore the table, and so does ptmi_render_features unless
 * ptmi_set_feature_shading asks ("shaded features"): the feature normal stays the stored one.
 *
 * ptmi_set_vertex_normals: normals NULL drops the table (n_prims is then ignored).  A successful call restarts an accumulation,
 * makes features stale and empties the temporal history, as ptmi_set_surfaces does.  PTMI_E_INVALID, with nothing changed (every
 * check is made before anything changes, and the new array is uploaded before the old one is freed): no scene loaded, n_prims !=
 * ptmi_scene_info's count, a NaN or infinite component in a corner that is read (zero-length corner normals are allowed), and -
 * for a table with a smooth primitive - a current config with integrator = 1, sampling_mode != 0 or fast_tree = 1;
 * ptmi_set_config rejects those three while such a table is set.  ptmi_check_vertex_normals makes the checks that need no context:
 * n_prims >= 1, normals not NULL, corners 0 .. 2 of every primitive finite (the 4th corner's check needs the primitive's type:
 * ptmi_set_vertex_normals and ptmi_host_classify_vertex_normals make it for quads).  ptmi_vertex_normals_info: the number of
 * smooth primitives, 0 without a table.  ptmi_host_classify_vertex_normals: the classification on the host, without a context -
 * type and stored (n_prims x 3) as ptmi_scene_get_prims gives them; smooth (may be NULL) receives 1 per smooth primitive.
 *
 * THE NORMAL of a vertex at p = o + t d on a smooth primitive k; binary32 in the order written, no fused multiply-add, / the IEEE
 * quotient, dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z and unit_vector(v) = v * (1.0f / sqrtf(dot(v, v))) (vector.h); n_k is
 * the stored normal, and "take the stored normal" means N = n_k as it is.
 *   triangle, with v0 and the edges e1 = v1 - v0, e2 = v2 - v0 as the walk holds them (float subtractions) and corner normals
 *   (n0, n1, n2):
 *       w = p - v0
 *       d00 = dot(e1, e1);  d01 = dot(e1, e2);  d11 = dot(e2, e2);  d20 = dot(w, e1);  d21 = dot(w, e2)
 *       den = d00 * d11 - d01 * d01;   unless den > 0 and den <= FLT_MAX take the stored normal (a zero-area or huge triangle)
 *       r1 = (d11 * d20 - d01 * d21) / den;   r2 = (d00 * d21 - d01 * d20) / den
 *       b1 = r1 < 0 ? 0 : (r1 > 1 ? 1 : r1);   m = 1 - b1;   b2 = r2 < 0 ? 0 : (r2 > m ? m : r2);   b0 = m - b2
 *           (comparisons, not fminf / fmaxf: a NaN stays a NaN; a point outside the primitive clamps onto it)
 *       S = (b0 * n0 + b1 * n1) + b2 * n2     per component
 *       len2 = dot(S, S);   unless len2 > 0 and len2 <= FLT_MAX take the stored normal (the corner normals cancel, or a NaN)
 *       N = unit_vector(S)
 *   quad, with the edges e1 = v10 - v00, e2 = v11 - v00, e3 = v01 - v00 and corner normals (n00, n10, n11, n01): the two halves
 *   the walk tests, (v00, v10, v11) and (v00, v11, v01).  den, r1, r2 of the first half are formed over (e1, e2) as above.  If that
 *   den is valid and the raw r1 >= 0 the first half gives N as a triangle with (n00, n10, n11).  Otherwise the second half does,
 *   over (e2, e3) with (n00, n11, n01), and where its den is not valid either the vertex takes the stored normal.
 * THE ESTIMATOR is that of "rough metal" (and of every section it builds on) with ONE change: N replaces n_k where step 2 forms sn
 * - after the roulette and the |beta| < 1e-5 exit, not at the hit - and everything below reads it from there: sn is N turned
 * against d, o' = p + 1e-4f * sn, the glass interface's side (dot(d, N) < 0), the mirror, the rough frame, the cosine sample and
 * every cos_s.  Nothing else moves: step 1's emitter pdf keeps the geometric normal of the emitter table, and draws, depth count,
 * roulette and exits are unchanged.
 * WHAT FOLLOWS FROM THIS, and is not corrected: N may lie on the other side of the surface than the geometric normal as seen from
 * d (near silhouettes of a coarse mesh).  sn then points INTO the body: o' starts below the surface, the cosine lobe faces
 * inwards, and a light sample's cos_s > 0 test passes for directions behind the geometry.  The results are light leaks and dark
 * rims on coarse meshes; a finer tessellation narrows them, nothing here removes them.  In a closed scene whose reachable
 * primitives all have the same Le and Kd the expected value is unchanged all the same. */
/* host only, no context: 0 or PTMI_E_INVALID with the message */
int  ptmi_check_vertex_normals(int n_prims, const float* normals);
int  ptmi_host_classify_vertex_normals(int n_prims, const int* type, const float* stored /* n_prims*3 */, const float* normals,
                                       int* smooth /* n_prims, may be NULL */, int* n_smooth /* may be NULL */);
int  ptmi_set_vertex_normals(ptmi_ctx*, int n_prims, const float* normals /* n_prims*4*3, load order, corner order of ptmi_load_scene_arrays' verts; 4th ignored for triangles; NULL drops the table */);
int  ptmi_vertex_normals_info(const ptmi_ctx*, int* n_smooth);   /* 0 without a table */
/* test hook: the kernel's own function (csrc/vertex_normal.h) once per case on the loaded scene and table.  prim: load-order
 * indices; p: 3n points; out: 4n - N.xyz, then 1.0 where N was interpolated and 0.0 where the vertex keeps the stored normal (a
 * flat primitive, a fallback, no table).  PTMI_E_INVALID: no scene, a prim out of range. */
int  ptmi_debug_vertex_normal(ptmi_ctx*, int n, const int* prim /* load order */, const float* p /* 3n */, float* out /* 4n */);

/* ---- albedo texture: a UV-mapped image modulating Kd at path vertices (new in this implementation) ------------------------------
 * The loaders keep ONE colour per primitive, as the reference does (its OBJ loader reads no vt or map_Kd, its PBRT importer counts
 * a textured Kd as 1 1 1).  ptmi_set_albedo_texture gives the loaded scene ONE image - an atlas covers many materials - of
 * height x width x 3 floats, linear RGB, row-major, and a table of corner UVs, n_prims x 4 x 2 floats in load order, a primitive's
 * corners in the order of ptmi_load_scene_arrays' verts (v0 v1 v2 | v00 v10 v11 v01) as in the vertex-normal table; a triangle's
 * 4th UV is ignored.  textured (n_prims ints, NULL: all) marks the primitives the image applies to; UVs of the others are never
 * read and may hold anything.  The table belongs to the scene exactly as the surface and vertex-normal tables do: a scene load
 * drops it.  Ke is never textured.
 *
 * A table without a textured primitive is no table: the context takes exactly the route it takes without one.  A context with a
 * textured primitive renders both values of next_event through the per-lane kernel of next-event estimation, as a context with an
 * environment, a specular surface or a smooth primitive does; frames, batches, passes, tiled contexts, ptmi_denoise,
 * ptmi_denoise_variance, ptmi_temporal_accumulate and ptmi_gather_frame work as they do without one.  ptmi_run_radiosity_solver
 * and the Radiosity view (integrator = 1) ignore the texture, and so does ptmi_render_features unless ptmi_set_feature_shading asks
 * ("shaded features"): the feature albedo stays Kd_k, so the denoisers demodulate by the untextured colour.
 *
 * ptmi_set_albedo_texture: texels NULL drops the texture (every other argument is then ignored).  A successful call restarts an
 * accumulation, makes features stale and empties the temporal history, as ptmi_set_surfaces does.  PTMI_E_INVALID, with nothing
 * changed (every check is made before anything changes, and the new arrays are uploaded before the old ones are freed): no scene
 * loaded; n_prims != ptmi_scene_info's count; width or height outside 1 .. 4096; filter not 0 (nearest) or 1 (bilinear); a texel
 * component that is not finite or is negative; a UV component that is read, of a textured primitive, that is not finite or whose
 * magnitude exceeds 65536; and - with a textured primitive - a current config with integrator = 1, sampling_mode != 0 or
 * fast_tree = 1; ptmi_set_config rejects those three while such a table is set.  ptmi_check_albedo_texture makes the checks that
 * need no context: n_prims >= 1, texels and uv not NULL, the ranges, the texels, and corners 0 .. 2 of every textured primitive
 * (the 4th corner's check needs the primitive's type: ptmi_set_albedo_texture makes it for textured quads).
 * ptmi_albedo_texture_info: the number of textured primitives and the image's width, height and filter, all 0 without a table.
 *
 * THE UV of a vertex at p = o + t d on a textured primitive k; binary32 in the order written, no fused multiply-add.  The weights
 * b0, b1, b2 are those of "vertex normals", character for character: w = p - v0, den, r1, r2 over the edges of the half,
 * b1 = r1 < 0 ? 0 : (r1 > 1 ? 1 : r1);  m = 1 - b1;  b2 = r2 < 0 ? 0 : (r2 > m ? m : r2);  b0 = m - b2 (comparisons), a triangle's one
 * half (e1, e2) with corners (0, a, b) = (0, 1, 2), a quad's first half (e1, e2) with corners (0, 1, 2) where its den is valid (den >
 * 0 and den <= FLT_MAX) and the raw r1 >= 0, otherwise its second half (e2, e3) with corners (0, 2, 3).  Where the half so chosen
 * has no valid den the weights are (1, 0, 0) and nothing is blended: (u, v) = (u_0, v_0), the first corner's as stored.  Otherwise,
 * per coordinate:
 *       u = (b0 * u_0 + b1 * u_a) + b2 * u_b
 * and then for both:
 *       s = u - floorf(u);   s = (s >= 0 && s < 1) ? s : 0        (repeat; -1e-9f gives 1.0f and a NaN gives a NaN: both pin to 0)
 * THE TEXEL.  Row 0 of the image is v in [0, 1 / height); nothing is flipped.  s_u, s_v the wrapped coordinates.
 *   nearest:   i = (int)(s_u * (float)width);   if (i > width - 1) i = width - 1;   j likewise from s_v and height;
 *              T = texel[j * width + i]
 *   bilinear:  x = s_u * (float)width - 0.5f;   x0 = floorf(x);   fx = x - x0;   i0 = (int)x0;   i1 = i0 + 1
 *              if (i0 < 0) i0 = width - 1;   if (i1 > width - 1) i1 = 0          (repeat at the seam)
 *              y0, fy, j0, j1 likewise from s_v and height; per channel
 *              a = (1 - fx) * T[j0][i0] + fx * T[j0][i1];   b = (1 - fx) * T[j1][i0] + fx * T[j1][i1];   T = (1 - fy) * a + fy * b
 *              every product rounded, every sum rounded.  (1 - f) + f == 1 in binary32 for every f in [0, 1), so an image of all
 *              ones gives T = 1 exactly under both filters.
 * THE ESTIMATOR is that of "vertex normals" (and of every section it builds on) with ONE change: Kd(p) = Kd_k * T, per component,
 * replaces Kd_k wherever step 2 reads the primitive's colour - the beta = beta * Kd before the |beta| < 1e-5 exit - so the texture
 * tints mirror, glass and rough metal exactly as Kd_k does.  The lookup happens after the roulette: a path the roulette ends never
 * makes it.  Draws, depth count, roulette, exits, emitter pdf and light sampling are unchanged, and an untextured primitive in a
 * textured scene uses Kd_k untouched. */
/* host only, no context: 0 or PTMI_E_INVALID with the message */
int  ptmi_check_albedo_texture(int width, int height, const float* texels, int filter, int n_prims, const float* uv, const int* textured);
int  ptmi_set_albedo_texture(ptmi_ctx*, int width, int height, const float* texels /* height*width*3, linear RGB, row-major; NULL drops the texture */,
                             int filter /* 0 nearest, 1 bilinear */, int n_prims, const float* uv /* n_prims*4*2, load order */,
                             const int* textured /* n_prims, nonzero: textured; NULL: all */);
int  ptmi_albedo_texture_info(const ptmi_ctx*, int* n_textured, int* width, int* height, int* filter);   /* all 0 without one */
/* test hook: the kernel's own function (csrc/albedo_texture.h) once per case on the loaded scene and table.  prim: load-order
 * indices; p: 3n points; out: 6n - s_u, s_v, T.rgb, then 1.0 for a textured primitive; for an untextured one, or with no table:
 * 0, 0, 1, 1, 1, 0.  PTMI_E_INVALID: no scene, a prim out of range. */
int  ptmi_debug_albedo(ptmi_ctx*, int n, const int* prim /* load order */, const float* p /* 3n */, float* out /* 6n */);

/* ---- shaded features: textured albedo and interpolated normals in the feature buffers (new in this implementation) --------------
 * "vertex normals" and "albedo texture" change what a surface is at a path vertex; the feature pass records the stored normal and
 * the untextured Kd_k all the same, so ptmi_denoise, ptmi_denoise_variance, ptmi_temporal_accumulate and ptmi_denoise_temporal
 * filter a texture as signal (they demodulate by a constant) and a smooth ball facet by facet.  ptmi_set_feature_shading lets the
 * feature pass record what the path tracer shades with.  It is opt-in and a property of the CONTEXT, as ptmi_config is: default 0,
 * kept over scene loads, allowed on tiled contexts and under every config (the feature pass runs under all of them).  A flag whose
 * table is absent has no effect, at once and for as long as the table stays absent; it takes effect when the table is set.
 *
 * THE FEATURE PASS is that of ptmi_render_features, float for float, with TWO changes per hit, inside `if hit`, where k is the hit
 * primitive and p = o + t * d is the ONE float triple that is also added to P:
 *   with PTMI_FEATURE_TEXTURED_ALBEDO, an albedo table set and k textured:
 *       Kd(p) = Kd_k * T  per component (a rounded product);   A = A + Kd(p)  (the rounded sum)
 *       T is THE TEXEL of "albedo texture" at THE UV of p, filter and wrap as there.  Otherwise A = A + Kd_k.
 *   with PTMI_FEATURE_SHADING_NORMAL, a vertex-normal table set and k smooth:
 *       N = N + Ns(p),  Ns(p) THE NORMAL of "vertex normals" at p: the interpolated unit normal, and the stored normal n_k
 *       wherever that section takes the stored normal (den or len2 not valid).  Otherwise N = N + n_k.
 * Everything else stays: the strata and their order, the sums' order, rcp_rn((float)(g * g)), misses, tiling, no RNG.  With flags
 * 0, or with no table that a set flag names, the pass is ptmi_render_features' bit for bit (the same kernel runs).  The interpolated
 * normal is NOT turned against d, as n_k is not.
 * The surface table is still ignored: a mirror's or a pane's feature albedo is its (possibly textured) tint, its feature normal
 * its own (possibly interpolated) normal.  Following a specular chain to the first diffuse vertex is out of scope.
 * ptmi_run_radiosity_solver and the Radiosity view ignore both tables whatever the flags say.
 *
 * ptmi_set_feature_shading with a value other than the context's: the feature buffers and the variance buffers become invalid
 * (ptmi_read_features / ptmi_read_variance fail until they are computed again; the filters recompute the features) and the temporal
 * history empties, since it holds albedo and normal of the old kind.  It does NOT restart an accumulation and does NOT make the
 * image stale - nothing about rendering changed - so a ptmi_denoise directly after it filters the current image with recomputed
 * features.  With the value the context already has it changes nothing.  PTMI_E_INVALID, with nothing changed: flags outside
 * 0 .. 3.  ptmi_check_feature_shading makes that check without a context. */
#define PTMI_FEATURE_TEXTURED_ALBEDO 1   /* the feature albedo is Kd(p) = Kd_k * T of "albedo texture" */
#define PTMI_FEATURE_SHADING_NORMAL  2   /* the feature normal is the interpolated normal of "vertex normals" */
/* host only, no context: 0 or PTMI_E_INVALID with the message */
int  ptmi_check_feature_shading(int flags);
int  ptmi_set_feature_shading(ptmi_ctx*, int flags);       /* default 0: ptmi_render_features as it is without this section */
int  ptmi_feature_shading(const ptmi_ctx*, int* flags);

/* ---- thin lens: depth of field with an aperture and a focus distance (new in this implementation) -------------------------------
 * The reference's sensor is a pinhole.  ptmi_set_lens gives the context a thin lens: a disc of `radius` around the camera's
 * origin, in the plane that (hor, ver) of ptmi_get_camera_frame span, and a plane of sharp focus at `focus_distance` along the
 * optical axis, both in scene units.  The two numbers belong to the CONTEXT, as the camera does: a scene load,
 * ptmi_update_resolution and ptmi_set_camera keep them.  radius >= 0; 0 is the pinhole and the default.  focus_distance > 0; a
 * context that was given none focuses at |origin - lookat| of the current camera (of ptmi_set_camera's origin and lookat, binary32,
 * products summed left to right), and follows the camera until ptmi_set_lens names a distance.
 *
 * radius == 0 is NO LENS: no extra draws, no block, and the frame takes the route and the kernels it takes without this section,
 * bit for bit; ptmi_stats.bounce_launches is what it was.  A context with radius > 0 renders both values of next_event through
 * the per-lane kernel of next-event estimation (one launch), as a context with an environment does; frames, batches,
 * ptmi_select_frame, passes, tiled contexts, ptmi_denoise, ptmi_denoise_variance, ptmi_temporal_accumulate and ptmi_gather_frame
 * work as they do without one.
 * WHAT THE LENS DOES NOT TOUCH.  ptmi_render_features and the Radiosity view (integrator = 1) keep the pinhole through the lens
 * centre: albedo, normal and position stay sharp while the image blurs, and the filters and the temporal step run unchanged on
 * those guides (blurred guides and a lens-aware reprojection are out of scope).  ptmi_run_radiosity_solver ignores the lens.
 *
 * THE LENS BLOCK is derived on the host from the frame (org, llc, hor, ver) of ptmi_get_camera_frame and the image size W x H,
 * again whenever the camera, the resolution or the lens has changed; binary32, every operation rounded, no fused multiply-add.
 * With f = focus_distance, R = radius, per component where a vector is written:
 *       hor_f = f * hor          ver_f = f * ver          llc_f = org + f * (llc - org)
 *       a = (R / length(hor)) * hor                       b = (R / length(ver)) * ver          length(v) = sqrtf((v.x^2 + v.y^2) + v.z^2)
 * as six records of four floats: (llc_f, W) (hor_f, 1/W) (ver_f, H) (org, 1/H) (a, 0) (b, 0); 1/W and 1/H as the sweep's frame block
 * has them (both 0 where a size exceeds 2^23) and not read by the lens ray.
 * THE LENS RAY of a sample of pixel (x, y).  The two lens draws come FIRST, the two jitter draws second (the order has no meaning
 * beyond letting the restatement wrap the pinhole's; tests/lens_oracle.py):
 *       r3 = uniform   r4 = uniform   r1 = uniform   r2 = uniform
 *       rho = sqrtf(r3)   phi = (float)(2 pi r4), the product in binary64 as the cosine sample forms it   (s, c) = ptmi_sincosf of phi
 *       dx = rho * c      dy = rho * s
 *       o = (org + dx * a) + dy * b
 *       u = ((float)x + r1) / (float)W      v = ((float)y + r2) / (float)H                          (as without a lens)
 *       d = unit_vector(((llc_f + u * hor_f) + v * ver_f) - o)
 * so a lens ray is the sensor's get_ray over the per-sample frame (o, llc_f, hor_f, ver_f), and a point of the plane at depth f
 * has the same (u, v) from every point of the lens.  Everything after the primary ray - THE ESTIMATOR of whatever sections apply -
 * is unchanged.
 *
 * ptmi_check_lens: host only, no context.  PTMI_E_INVALID with a message: a NaN in either number, an infinite one, radius < 0,
 * focus_distance <= 0, and - with radius > 0 - a lens block over ptmi_default_camera at a square image that is not finite (a
 * context's own camera is checked by ptmi_set_lens and at every render).
 * ptmi_host_lens_block: the block, 24 floats, of a lens with radius > 0 over ptmi_host_camera_frame(cam, width, height); host only.
 * PTMI_E_INVALID, with out24 untouched: what ptmi_check_lens rejects, radius == 0 (there is no block), width or height < 1, and a
 * block with a value that is not finite - f so large that f * hor overflows, a frame without extent.
 * ptmi_set_lens: radius == 0 with focus_distance <= 0 is accepted and means "no lens, no focus distance of the context's own".
 * Otherwise PTMI_E_INVALID, with nothing changed: what ptmi_check_lens(radius, focus_distance)'s checks of the two numbers reject;
 * with radius > 0, a current config with sampling_mode != 0 or fast_tree = 1 (ptmi_set_config rejects those two while a lens is
 * set; integrator = 1 is allowed and ignores the lens), and - once a resolution is set - a block over the current camera that is
 * not finite.  A camera or resolution set later that makes the block non-finite fails the render call instead, with the same
 * message.  Values other than the context's invalidate exactly what ptmi_set_camera invalidates: an accumulation restarts and the
 * feature buffers (with them the variance buffers) go stale; the temporal history is kept, as a camera move keeps it.  The values
 * the context already has change nothing.
 * ptmi_lens: the radius and the focus distance in force (the default where the context has none of its own). */
/* host only, no context: 0 or PTMI_E_INVALID with the message */
int  ptmi_check_lens(float radius, float focus_distance);
int  ptmi_host_lens_block(const ptmi_camera*, int width, int height, float radius, float focus_distance, float* out24);
int  ptmi_set_lens(ptmi_ctx*, float radius, float focus_distance);
int  ptmi_lens(const ptmi_ctx*, float* radius, float* focus_distance);   /* either may be NULL */
/* test hooks.  ptmi_debug_lens_block: the block as the device holds it, derived for the camera, resolution and lens as they are
 * now.  ptmi_debug_lens_ray: the kernel's own function (csrc/lens.h) once per case over that block, on given uniforms instead
 * of the stream's: pixel (px[i], py[i]), r[4i ..] = r3 r4 r1 r2; out[6i ..] = o, d.  r3 must lie in [2^-33, 1], a uniform's range.
 * PTMI_E_INVALID: no lens (radius 0), no resolution set. */
int  ptmi_debug_lens_block(ptmi_ctx*, float* out24);
int  ptmi_debug_lens_ray(ptmi_ctx*, int n, const int* px, const int* py, const float* r /* 4n */, float* out /* 6n */);

/* ---- participating medium: a homogeneous fog box (new in this implementation) --------------------------------------------------
 * Without this section every ray travels through vacuum.  ptmi_set_medium gives the loaded SCENE one homogeneous medium inside an
 * axis-aligned box [lo, hi] in scene coordinates: extinction sigma_t per scene unit (achromatic, so one distance sample serves
 * all three channels), single-scattering albedo per channel in [0, 1], and the Henyey-Greenstein asymmetry g, |g| <= 0.9, g > 0
 * scattering forward.  The medium belongs to the scene, because its box is in scene coordinates: a scene load drops it, as it
 * drops the surface table.
 *
 * sigma_t == 0, or a NULL medium, is NO MEDIUM (not a medium of density 0): no extra draw, no block, and the frame takes the
 * route and the launch counts it takes without this section and comes out bit for bit the same (a next-event frame runs the
 * per-lane kernel's instantiation without the medium, which has one more, unread, argument).  A scene with a medium renders both values
 * of next_event through the per-lane kernel of next-event estimation (one launch), as a context with a lens does; frames,
 * batches, ptmi_select_frame, passes and tiled contexts work as they do without one.
 * WHAT THE MEDIUM DOES NOT TOUCH.  ptmi_render_features, the Radiosity view (integrator = 1) and ptmi_run_radiosity_solver ignore
 * the medium: the guides of the filters and of the temporal step stay those of the surfaces.  The guided sampling modes and
 * fast_tree are refused with a medium, by ptmi_set_medium and by ptmi_set_config.
 *
 * THE MEDIUM BLOCK, three records of four floats, the caller's numbers unchanged: (lo, sigma_t) (hi, g) (albedo, 0).
 * Everything below is binary32, every operation rounded, no fused multiply-add, unless binary64 is named.
 * THE SEGMENT [t0, t1] of a ray (o, d) that ends at t_end (the walk's t at a hit, +inf at a miss):
 *       t0 = 0      t1 = t_end      inside = true
 *       per axis a = x, y, z in this order:
 *         d_a != 0:   ta = (lo_a - o_a) / d_a      tb = (hi_a - o_a) / d_a           (IEEE divisions)
 *                     near = fminf(ta, tb)         far = fmaxf(ta, tb)
 *                     if (near > t0) t0 = near     if (far < t1) t1 = far
 *         d_a == 0:   if not (lo_a <= o_a and o_a <= hi_a) inside = false
 *       the segment is non-empty iff inside and t1 > t0
 * TRANSMITTANCE  T = ptmi_expf of -(sigma_t * (t1 - t0)) for a non-empty segment; an empty one has T = 1 exactly.
 * FREE FLIGHT.  With a medium every path ray makes ONE draw u_m directly after its walk returns, before anything else happens at
 * the vertex, whether or not the ray meets the box; shadow rays make none.
 *       s = -((float)l) / sigma_t, l = ptmi_log_d of (double)u_m     tm = t0 + s
 * If the segment is non-empty and tm < t1 the ray has a MEDIUM VERTEX at x = o + tm * d.  Otherwise the hit or the miss is
 * processed exactly as without a medium, with weight 1: the probability of passing is the transmittance.
 * THE PHASE FUNCTION, binary64 from the float inputs, +, -, *, / and the IEEE square root only, rounded once to float:
 *       hg(c):  c = fminf(fmaxf(c, -1), 1);  g == 0: (float)(1 / (4 pi))
 *               else  t = (1 + g * g) - (2 * g) * c       (float)((1 - g * g) / ((4 pi) * (t * sqrt(t))))
 *       the sampled cosine of a uniform u:   g == 0: (float)(1 - 2 * u)
 *               else  s = 2 * u - 1      den = 1 + g * s      g2 = g * g
 *                     num = ((s + (g * (s * s + 3)) * 0.5) + g2 * s) + (g2 * g) * ((s * s - 1) * 0.5)
 *                     c = num / (den * den)                          (float)min(max(c, -1), 1)
 *       (the textbook inversion ((1 + g^2) - q^2) / (2 g), q = (1 - g^2) / (1 - g + 2 g u), expanded over s: the same rational
 *       function without its difference of two numbers near 1, which below |g| ~ 1e-8 returned the cosine 0 for every u)
 * THE MEDIUM VERTEX follows the order of a surface vertex of "next-event estimation":
 *   1. nothing is emitted;
 *   2. the roulette at depth > 2 on tp, then tp = tp * albedo and the length(tp) < 1e-5f exit;
 *   3. the light sample, with the same three draws (five with a sampled environment) under the same condition
 *      nee_on && depth + 1 < max_depth && (emitters or a sampled environment): the emitter or the environment is sampled from x
 *      itself - no offset, no test of a cosine at the vertex - and with wi the unit direction and p_l the sample's density
 *            ph = hg(dot(d, wi))      w = (ph / p_l) * mis_power_heuristic(p_l, ph)      contrib = (tp * Le) * w
 *      the shadow ray starts at x;
 *   4. the phase sample with the two draws u, v; depth++ and the depth exit; then
 *            c = the sampled cosine of u      s = sqrtf(fmaxf(0, 1 - c * c))      phi = (float)(2 pi v), the product in binary64
 *            (sp, cp) = ptmi_sincosf of phi   (T, B) the tangent frame of "rough metal" about d
 *            d' = unit_vector(((s * cp) * T + (s * sp) * B) + c * d)      o' = x
 *      pb_prev = hg(c) of the sampled cosine itself (not of a recomputed dot product), and the path ray is no specular one: the
 *      next hit or miss takes its MIS weight from pb_prev, as after a cosine sample.
 * SHADOW RAYS.  Every shadow ray, from a surface vertex or a medium vertex, multiplies its contribution by T of its own segment
 * when it is found visible: L = L + contrib * T, with t_end the shadow walk's t for an emitter and +inf for the environment.
 * Both strategies weigh with the same pair (pb, p_l): the transmittance to the next vertex is common to both and cancels against
 * the free-flight density, so the weights of a path sum to 1.
 *
 * ptmi_check_medium: host only.  PTMI_E_INVALID with a message of its own for: a field that is not finite, lo >= hi on an axis,
 * sigma_t < 0, an albedo outside [0, 1], |g| > 0.9.
 * ptmi_set_medium: NULL, or sigma_t == 0 (checked like any other), drops the medium.  Otherwise PTMI_E_INVALID with nothing
 * changed: what ptmi_check_medium rejects; no scene loaded; a config with sampling_mode != 0 or fast_tree = 1; and, with quads
 * in the scene, a corner of the box that fails the bound every ray origin outside the scene is held to (rays now start inside
 * the box).  A medium other than the scene's restarts an accumulation; the feature buffers and the temporal history stay.
 * ptmi_medium_info: the medium in force (ptmi_default_medium's values without one) and whether there is one.
 * ptmi_host_medium_block: the block, 12 floats; host only; PTMI_E_INVALID, out12 untouched: what ptmi_check_medium rejects.
 * ptmi_debug_medium_call: test hook; the kernel's own functions (csrc/medium.h) once per case over the block of the GIVEN medium
 * in `in`, PTMI_MEDIUM_CALL_IN floats per case, PTMI_MEDIUM_CALL_OUT floats out per case (zero where an op writes nothing):
 *       in[0..11] the block   in[12..14] o   in[15..17] d   in[18] t_end   in[19] u (u_m, the cosine, or the uniform)
 *   op 0  segment and T:  out = nonempty (0 | 1), t0, t1, T          (t0, t1 as the loop leaves them, also where empty)
 *   op 1  free flight:    out = vertex (0 | 1), tm, x
 *   op 2  hg value:       out = hg(u) with g = in[7]
 *   op 3  hg sample:      out = the sampled cosine of u, hg of it, d' about d with v = in[18]
 * u_m must lie in [2^-33, 1], a uniform's range, and sigma_t > 0. */
typedef struct { float lo[3], hi[3]; float sigma_t; float albedo[3]; float g; } ptmi_medium;
#define PTMI_MEDIUM_BLOCK_FLOATS 12
#define PTMI_MEDIUM_CALL_IN  20
#define PTMI_MEDIUM_CALL_OUT 8
void ptmi_default_medium(ptmi_medium*);                    /* the unit box [0, 1]^3, sigma_t 0 (no medium), albedo 1, g 0 */
int  ptmi_check_medium(const ptmi_medium*);
int  ptmi_set_medium(ptmi_ctx*, const ptmi_medium* /* NULL drops it */);
int  ptmi_medium_info(const ptmi_ctx*, ptmi_medium* out, int* on);   /* either may be NULL */
int  ptmi_host_medium_block(const ptmi_medium*, float* out12);
int  ptmi_debug_medium_call(ptmi_ctx*, int op, int n, const float* in /* n * PTMI_MEDIUM_CALL_IN */, float* out /* n * PTMI_MEDIUM_CALL_OUT */);

/* test hook: the inputs of ptmi_denoise, ptmi_denoise_variance (source = 1) and ptmi_temporal_accumulate, given instead of
 * rendered, so that every data-dependent decision of their kernels can be reached on constructed images.  n = width x height
 * of the current resolution; all arrays local row-major like ptmi_read_image.  The call
 *   - uploads radiance into the buffer ptmi_read_image reads and writes its rgb8 beside it by the tone map of ptmi_denoise
 *     step 4 (the denoiser's own 0-iteration kernel; no kernel of the hook's own);
 *   - uploads the features as ptmi_render_features writes them: albedo.w = hit_fraction, normal.w = position.w = 0;
 *   - leaves the context as a finished frame plus a finished feature pass of `grid` would: image current and not a pass,
 *     features valid for `grid`, no current variance, nothing denoised.
 * It touches nothing else: not the temporal history (so: inject view A, step, ptmi_set_camera(B), inject view B, step - and the
 * second step's history is constructed), not the accumulation, the colour sums or the streams.  A later frame or pass
 * overwrites the image, a call that makes features stale makes both stale, as after a rendered frame.  Values are not
 * checked: non-finite ones are legitimate inputs (see NON-FINITE VALUES under ptmi_denoise).
 * PTMI_E_INVALID, the context unchanged: a NULL argument, no scene loaded, no resolution set, a context tiled over more than
 * one rank, the Radiosity integrator, grid outside 1 .. 4. */
int  ptmi_debug_set_filter_inputs(ptmi_ctx*, const float* radiance /* 3n */, const float* albedo /* 3n */, const float* normal /* 3n */,
                                  const float* position /* 3n */, const float* hit_fraction /* n */, int grid);

/* test hook: one stopping test plus resolve of an accumulation on state given instead of rendered, so that every decision of
 * THE STOPPING RULE, the compaction of the next pass's queue and the resolve at per-pixel counts can be reached on constructed
 * values.  n = the local pixels of the current resolution.  All inputs lie BY SLOT, as the kernels hold them, not by pixel:
 * without 8 x 8 slot tiles (config.wave_tiles = 0, or a width, local row count or row_block that is no multiple of 8) slot s is
 * local pixel (row s / width, column s % width); with them, slot s is pixel (in & 7, in >> 3) of tile s >> 6 (in = s & 63), the
 * tiles row-major, width / 8 to a row.
 *   sums   S_k.xyz: the colour sums after the pass                  prev   S_{k-1}.xyz and the mean, 4 floats per slot
 *   m2, passes      M2 and the passes taken BEFORE this one (k = passes + 1)
 *   queue  n_queue distinct slots, the pixels that took the pass; NULL: the slots 0 .. n_queue - 1
 *   params NULL: a plain progressive pass.  Its fields are used as given (not range-checked as ptmi_accum_pass checks them)
 *   first  != 0: pass 1 - prev, m2 and passes are not read for the queued slots (they count as zero)
 * The call
 *   - uploads the inputs into the context's own buffers (allocated, if there are none yet, as a first pass allocates them);
 *   - zeroes the output count and runs the product's stopping test over the queue, then its resolve by counts over all local
 *     pixels, exactly as the end of ptmi_accum_pass does (no kernel of the hook's own): the queued slots take the rule with
 *     inv_spp of config.spp; every slot, queued or not, is resolved at passes[slot] * config.spp samples;
 *   - returns the next pass's queue in queue_out (room for n_queue entries) and its length in *n_out.  The queue's contract is
 *     the product's: the slots that go on, once each; the survivors of each 64 consecutive input positions contiguous and in
 *     input order; the order of those groups among themselves unspecified;
 *   - leaves the context as a finished pass leaves it: an accumulation with a pass count one higher, *n_out pixels active, that
 *     queue the next pass's, the image current and marked as a pass.
 * So ptmi_read_image, ptmi_read_sample_counts, ptmi_read_pass_moments, ptmi_denoise_variance (source = 0) and a following
 * ptmi_accum_pass act on the constructed state.  The streams, the features and the temporal history are untouched.  It works on
 * a tiled context (its local slots).  Values are not checked: non-finite sums and moments are legitimate inputs (NON-FINITE
 * VALUES under THE STOPPING RULE).
 * PTMI_E_INVALID: a NULL argument other than queue and params, no scene loaded, no resolution set, the Radiosity integrator,
 * n_queue outside [0, n], a queue entry outside [0, n) or repeated. */
int  ptmi_debug_accum_step(ptmi_ctx*, const float* sums /* 3n */, const float* prev /* 4n */, const float* m2 /* n */,
                           const uint32_t* passes /* n */, const int* queue /* n_queue, or NULL */, int n_queue,
                           const ptmi_adaptive_params* params /* or NULL */, int first, int* queue_out /* n_queue */, int* n_out);

/* test hook: the launch order of a refill frame on given costs.  queue_out = the n entries of queue_in (NULL: 0 .. n - 1) as the
 * product's ordering pass places them for cost[entry] (n_cost values), cost_max and `classes`:
 *     shift = the smallest s in 0 .. 7 with (256 >> s) <= classes, 7 if there is none    (classes >= 256: 0; 1 or 2: 7)
 *     class(entry) = (255 - floor(256 * min(cost, cost_max) / (cost_max + 1))) >> shift          (64-bit integers)
 * Classes ascend along queue_out, i.e. costs descend class by class; inside a class the entries of one block of 256 consecutive
 * input positions are contiguous and in input order, the order of the blocks among themselves unspecified.  hist: the pass's
 * 512 ints when it is through - hist[c] = entries of class c, hist[256 + c] = the END of class c in queue_out.  The call uses
 * buffers of its own and changes nothing in the context.
 * PTMI_E_INVALID: a NULL argument other than queue_in, n or n_cost < 1, classes < 1, a queue entry outside [0, n_cost), and
 * without queue_in n > n_cost. */
int  ptmi_debug_order_by_cost(ptmi_ctx*, int n, const int* queue_in /* n, or NULL */, const uint32_t* cost /* n_cost */, int n_cost,
                              uint32_t cost_max, int classes, int* queue_out /* n */, int* hist /* 512 */);

/* test hooks: the kernels that turn a radiosity solution into the records guided sampling reads (csrc/radiosity.hip), on given
 * grids and form factors.  Each uses buffers of its own, changes nothing in the context, launches the product's own kernel through
 * its own launch function and has no kernel of its own.  Values are not checked: non-finite ones are legitimate inputs.
 * ptmi_debug_cdf_records: n PrecomputedCDF records of 530 words (ptmi_host_cdf_record_layout) from n grids of 256 cells, row-major
 *   (theta, phi).  src_kind 0: four floats per cell (r, g, b, w) as the solver holds them - w is not read;  1: three floats per
 *   cell, as ptmi_set_radiosity_grids takes them;  2: one float per cell, a ready pdf, as ptmi_apply_grid_filter's records take it.
 *   Kinds 0 and 1 take pdf = 0.2126f * r + 0.7152f * g + 0.0722f * b, every operation rounded, left to right.
 * ptmi_debug_filter_pdfs: "Apply Filter & Rebuild CDFs" up to the pdfs: the luminance of rgb and the count grid (NULL: zero), each
 *   through the 5 x 5 float filter and divided by its sequential 256-term sum unless that sum <= 1e-12f; out_formfactor from the
 *   counts, out_radiosity from the luminance, n * 256 each.
 * ptmi_debug_radiosity_grid: update_radiosity_grid of the solver over a world of n primitives given by centre and normal alone:
 *   out[i] = primitive i's 16 x 16 rgb grid, cell(direction i -> j) += form_factors[i * n + j] * radiosity[j] in ascending j, for
 *   every j != i unless F_ij <= 0.0f or the distance r < 1e-6f; then, with enable_filtering, the 5 x 5 rgb filter.
 * NON-FINITE VALUES.  The comparisons are the reference's and a NaN fails each of them: a NaN form factor is not `<= 0` and IS
 *   added (it makes its cell NaN); a NaN distance is not `< 1e-6f`; a NaN sum is not `<= 1e-12f` and divides; a NaN filter weight
 *   total is not `> 1e-6f`, so the cell keeps its centre value - which is also what a sigma so small that 2 * sigma * sigma is 0
 *   in binary32 gives everywhere (the centre weight is exp(-0 / 0)).  A NaN row sum is not `< 1e-6f`: the row's CDF is NaN up to
 *   its forced last entry 1.  A record is valid where total > 1e-6f, and a VALID record can hold NaN: an inf cell gives total =
 *   inf, 1 / total = 0 and a marginal of inf * 0 up to its forced last entry, so sampling always picks row 7.  Sampling such
 *   records is defined (the linear search takes the first entry with xi <= cdf, a NaN never) and pinned by the tests.  Centres
 *   and normals must be finite and normals nonzero: a non-finite direction makes the cell index a float -> int conversion of a
 *   NaN, which is undefined on the host and on the device alike and is not specified here.
 * PTMI_E_INVALID: a NULL argument other than counts, n < 1, src_kind outside 0 .. 2. */
int  ptmi_debug_cdf_records(ptmi_ctx*, int n, int src_kind, const float* src /* n * 256 * (4 | 3 | 1) */, float* out /* n * 530 */);
int  ptmi_debug_filter_pdfs(ptmi_ctx*, int n, const float* rgb /* n*256*3 */, const float* counts /* n*256, or NULL */, int use_bilateral,
                            float sigma_spatial, float sigma_range, float* out_formfactor /* n*256 */, float* out_radiosity /* n*256 */);
int  ptmi_debug_radiosity_grid(ptmi_ctx*, int n, const float* centre /* 3n */, const float* normal /* 3n */,
                               const float* form_factors /* n*n */, const float* radiosity /* 3n */, int enable_filtering,
                               int use_bilateral, float sigma_spatial, float sigma_range, float* out /* n*256*3 */);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_H */
