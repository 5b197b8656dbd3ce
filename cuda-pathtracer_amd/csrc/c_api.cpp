// c_api.cpp — the C ABI of libptmi.so (include/ptmi.h) over the host-side state objects.
#include "c_api_common.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

using namespace ptmi;

std::string& ptmi::lastErrorText() { thread_local std::string text; return text; }

namespace {
void needRoute(const ptmi_ctx* c, RouteFeature f) {   // a per-lane feature is being switched on: the config as it is must allow it (host/route_rule.h)
    needNone(featureRefusal(f, (int)c->app.config.current_integrator, (int)c->app.config.sampling_mode, c->app.config.fast_tree));
}

// a call that changes what a frame would show: the accumulation restarts, the feature buffers go stale and the temporal
// history empties (ptmi_set_camera keeps the history: reprojecting it into the new view is the temporal step's job)
void viewChanged(ApplicationState& app) { accumReset(app); featuresStale(app); temporalReset(app); }
f3 v3(const float* p) { return mk3(p[0], p[1], p[2]); }

// FrameStats -> the C structs that carry its fields (ptmi_stats, ptmi_pass_stats)
template <class Dst>
void copy_frame_stats(const FrameStats& fs, Dst& d) {
    d.seconds = fs.seconds; d.bounce_kernel_ms = fs.bounce_kernel_ms; d.bounce_launches = fs.bounce_launches; d.path_visits = fs.path_visits;
    d.samples = fs.samples; d.rays = fs.rays; d.node_visits = fs.node_visits; d.prim_tests = fs.prim_tests; d.hits = fs.hits;
    d.top_node_visits = fs.top_node_visits; d.cert_chain = fs.cert_chain; d.cert_fallback = fs.cert_fallback;
}

std::vector<Primitive> prims_from_arrays(int n, const int* type, const float* verts, const float* normal, const float* bsdf, const float* Le) {
    need(type && verts && normal && bsdf && Le, "NULL argument");
    need(n > 0, "n must be positive");
    std::vector<Primitive> prims((size_t)n);
    for (int i = 0; i < n; i++) {
        Primitive& p = prims[i];
        need(type[i] == 0 || type[i] == 1, "type must be 0 (triangle) or 1 (quad)");
        p.type = type[i] ? PRIM_QUAD : PRIM_TRIANGLE;
        for (int k = 0; k < 4; k++) p.v[k] = v3(verts + ((size_t)i * 4 + k) * 3);
        if (p.type == PRIM_TRIANGLE) p.v[3] = mk3(0, 0, 0);
        p.normal = v3(normal + (size_t)i * 3); p.bsdf = v3(bsdf + (size_t)i * 3); p.Le = v3(Le + (size_t)i * 3);
    }
    return prims;
}
}  // namespace

extern "C" {

const char* ptmi_last_error(void) { return lastErrorText().c_str(); }

void ptmi_default_camera(ptmi_camera* c) {
    const AppConfig d;
    c->origin[0] = d.camera_origin.x; c->origin[1] = d.camera_origin.y; c->origin[2] = d.camera_origin.z;
    c->lookat[0] = d.look_at.x; c->lookat[1] = d.look_at.y; c->lookat[2] = d.look_at.z;
    c->vup[0] = d.up.x; c->vup[1] = d.up.y; c->vup[2] = d.up.z;
    c->vfov_deg = d.fov; c->yaw_deg = 90.0f; c->pitch_deg = 0.0f; c->orbit = 1;
}
void ptmi_default_config(ptmi_config* c) {
    const AppConfig d;
    c->spp = d.spp; c->max_depth = d.max_depth; c->sampling_mode = (int)d.sampling_mode; c->seed_base = d.seed_base;
    c->segments_per_launch = 0; c->collect_stats = 0; c->wave_tiles = 0; c->streams = 0; c->mis_bsdf_fraction = d.mis_bsdf_fraction; c->integrator = 0;
    c->download_image = 0; c->fast_tree = 0; c->next_event = 0;
}
void ptmi_default_tiling(ptmi_tiling* t) { t->n_ranks = 1; t->rank = 0; t->row_block = 8; }

int ptmi_ctx_create(int device_id, ptmi_ctx** out) {
    // (multi-process GPU work - the RCCL gather - needs HSA_ENABLE_IPC_MODE_LEGACY=0 on this driver stack.  The CALLER exports it
    // before anything initialises HIP: a setenv from here would come too late for a process that already has, and races with
    // getenv in other threads; include/ptmi.h says so at ptmi_dist_init)
    return guarded([&] { need(out != nullptr, "out is NULL"); *out = nullptr; *out = new ptmi_ctx(device_id); });
}
void ptmi_ctx_destroy(ptmi_ctx* c) { delete c; }

int ptmi_load_scene(ptmi_ctx* c, const char* filename, int subdivision_count, int convert_quads) {
    return guarded([&] {
        need(c && filename, "ctx/filename is NULL");
        need(subdivision_count >= 0 && subdivision_count <= 10, "subdivision_count must be in [0, 10]");   // UI range, ui_windows.h:213
        PTMI_HIP(hipSetDevice(c->app.device_id));
        c->app.config.convert_quads_to_triangles = convert_quads != 0;
        c->app.radiosity.cleanup();                       // a solution belongs to the scene it was computed for
        viewChanged(c->app);
        c->app.scene.loadScene(filename, subdivision_count, convert_quads != 0);
    });
}

int ptmi_load_scene_arrays(ptmi_ctx* c, int n, const int* type, const float* verts, const float* normal,
                           const float* bsdf, const float* Le) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        c->app.radiosity.cleanup();
        viewChanged(c->app);
        c->app.scene.loadSceneArrays(prims_from_arrays(n, type, verts, normal, bsdf, Le));
    });
}

static void scene_info(const SceneState& s, int* n_prims, int* n_tris, int* n_quads, int* n_bvh_nodes, int* bvh_depth) {
    if (n_prims) *n_prims = (int)s.h_primitives.size();
    if (n_tris) *n_tris = s.num_tris;
    if (n_quads) *n_quads = s.num_quads;
    if (n_bvh_nodes) *n_bvh_nodes = (int)s.bvh_nodes.size();
    if (bvh_depth) *bvh_depth = s.bvh_depth;
}
static void scene_get_prims(const SceneState& sc, int* type, float* verts, float* normal, float* bsdf, float* Le) {
    {
        const auto& ps = sc.h_primitives;
        for (size_t i = 0; i < ps.size(); i++) {
            const Primitive& p = ps[i];
            if (type) type[i] = (int)p.type;
            if (verts) for (int k = 0; k < 4; k++) { verts[(i * 4 + k) * 3] = p.v[k].x; verts[(i * 4 + k) * 3 + 1] = p.v[k].y; verts[(i * 4 + k) * 3 + 2] = p.v[k].z; }
            if (normal) { normal[i * 3] = p.normal.x; normal[i * 3 + 1] = p.normal.y; normal[i * 3 + 2] = p.normal.z; }
            if (bsdf) { bsdf[i * 3] = p.bsdf.x; bsdf[i * 3 + 1] = p.bsdf.y; bsdf[i * 3 + 2] = p.bsdf.z; }
            if (Le) { Le[i * 3] = p.Le.x; Le[i * 3 + 1] = p.Le.y; Le[i * 3 + 2] = p.Le.z; }
        }
    }
}
static void scene_get_bvh(const SceneState& s, float* bmin, float* bmax, int* left, int* right, int* count, int* indices) {
    {
        for (size_t i = 0; i < s.bvh_nodes.size(); i++) {
            const BVHNode& n = s.bvh_nodes[i];
            if (bmin) { bmin[i * 3] = n.bbox.min.x; bmin[i * 3 + 1] = n.bbox.min.y; bmin[i * 3 + 2] = n.bbox.min.z; }
            if (bmax) { bmax[i * 3] = n.bbox.max.x; bmax[i * 3 + 1] = n.bbox.max.y; bmax[i * 3 + 2] = n.bbox.max.z; }
            if (left) left[i] = n.left_child;
            if (right) right[i] = n.right_child;
            if (count) count[i] = n.prim_count;
        }
        if (indices) std::memcpy(indices, s.bvh_indices.data(), s.bvh_indices.size() * sizeof(int));
    }
}

int ptmi_scene_info(const ptmi_ctx* c, int* n_prims, int* n_tris, int* n_quads, int* n_bvh_nodes, int* bvh_depth) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); scene_info(c->app.scene, n_prims, n_tris, n_quads, n_bvh_nodes, bvh_depth); });
}
int ptmi_scene_get_prims(const ptmi_ctx* c, int* type, float* verts, float* normal, float* bsdf, float* Le) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); scene_get_prims(c->app.scene, type, verts, normal, bsdf, Le); });
}
int ptmi_scene_get_bvh(const ptmi_ctx* c, float* bmin, float* bmax, int* left, int* right, int* count, int* indices) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); scene_get_bvh(c->app.scene, bmin, bmax, left, right, count, indices); });
}

int ptmi_host_scene_load(const char* filename, int subdivision_count, int convert_quads, ptmi_host_scene** out) {
    return guarded([&] {
        need(filename && out, "NULL argument");
        need(subdivision_count >= 0 && subdivision_count <= 10, "subdivision_count must be in [0, 10]");
        *out = nullptr;
        std::unique_ptr<ptmi_host_scene> hs(new ptmi_host_scene);
        hs->scene.loadSceneHost(filename, subdivision_count, convert_quads != 0);
        *out = hs.release();
    });
}
int ptmi_host_scene_from_arrays(int n, const int* type, const float* verts, const float* normal,
                                const float* bsdf, const float* Le, ptmi_host_scene** out) {
    return guarded([&] {
        need(out != nullptr, "out is NULL");
        *out = nullptr;
        std::unique_ptr<ptmi_host_scene> hs(new ptmi_host_scene);
        hs->scene.loadSceneArraysHost(prims_from_arrays(n, type, verts, normal, bsdf, Le));
        *out = hs.release();
    });
}
void ptmi_host_scene_free(ptmi_host_scene* s) { delete s; }
int ptmi_host_scene_check_extent(ptmi_host_scene* s, const float* origin) {
    return guarded([&] {
        need(s != nullptr, "scene is NULL");
        s->scene.checkExtent();
        if (origin) s->scene.checkQuadOrigin(origin, nullptr, "origin");
    });
}
int ptmi_host_scene_info(const ptmi_host_scene* s, int* n_prims, int* n_tris, int* n_quads, int* n_bvh_nodes, int* bvh_depth) {
    return guarded([&] { need(s != nullptr, "scene is NULL"); scene_info(s->scene, n_prims, n_tris, n_quads, n_bvh_nodes, bvh_depth); });
}
int ptmi_host_scene_get_prims(const ptmi_host_scene* s, int* type, float* verts, float* normal, float* bsdf, float* Le) {
    return guarded([&] { need(s != nullptr, "scene is NULL"); scene_get_prims(s->scene, type, verts, normal, bsdf, Le); });
}
int ptmi_host_scene_get_bvh(const ptmi_host_scene* s, float* bmin, float* bmax, int* left, int* right, int* count, int* indices) {
    return guarded([&] { need(s != nullptr, "scene is NULL"); scene_get_bvh(s->scene, bmin, bmax, left, right, count, indices); });
}
int ptmi_host_emitters(const ptmi_host_scene* s, int* n_emitters, int* prim, float* cdf, float* pdf_area) {
    return guarded([&] {
        need(s != nullptr, "scene is NULL");
        const SceneState& sc = s->scene;
        const size_t ne = sc.h_emit_prim.size();
        if (n_emitters) *n_emitters = (int)ne;
        if (prim) std::memcpy(prim, sc.h_emit_prim.data(), ne * sizeof(int));
        if (cdf) std::memcpy(cdf, sc.h_emit_cdf.data(), ne * sizeof(float));
        if (pdf_area) std::memcpy(pdf_area, sc.h_pdf_area.data(), sc.h_pdf_area.size() * sizeof(float));
    });
}
int ptmi_write_png(const char* path, int width, int height, const unsigned char* rgb8) {
    return guarded([&] {
        need(path && rgb8, "NULL argument");
        need(width > 0 && height > 0, "width/height must be positive");
        if (!writePNG(path, width, height, rgb8)) throw IoError(std::string("cannot write ") + path);
    });
}
int ptmi_host_camera_frame(const ptmi_camera* cam, int width, int height, float* out12) {
    return guarded([&] {
        need(cam && out12, "NULL argument");
        need(width > 0 && height > 0, "width and height must be positive");
        Sensor s(v3(cam->origin), v3(cam->lookat), v3(cam->vup), cam->vfov_deg, 1.0f);   // application.h:107-113
        s.yaw = cam->yaw_deg; s.pitch = cam->pitch_deg;
        s.image_width = width; s.image_height = height;
        s.aspect = (float)width / (float)height;                                        // application_state.h:108
        cameraFrame12(s, cam->orbit != 0, out12);                                       // application.h:161
    });
}
int ptmi_host_cdf_record_layout(int* out10) {
    return guarded([&] {
        need(out10 != nullptr, "NULL argument");
        const int v[10] = {kCdfDwords * 4, kCdfPdf * 4, kCdfRowSums * 4, kCdfMarginal * 4, kCdfRowCdfs * 4, kCdfTotal * 4, kCdfValid * 4,
                           kGridRes, kGridSize, kGridRes / 2};
        std::memcpy(out10, v, sizeof v);
    });
}
int ptmi_host_local_row_map(int height, const ptmi_tiling* t, int* n_rows, int* rows_out) {
    return guarded([&] {
        need(t && n_rows, "NULL argument");
        need(height > 0 && t->n_ranks >= 1 && t->rank >= 0 && t->rank < t->n_ranks && t->row_block >= 1, "bad tiling");
        TileMap tm; tm.height = height; tm.n_ranks = t->n_ranks; tm.rank = t->rank; tm.row_block = t->row_block;
        const std::vector<int> rows = localRowMap(tm);
        *n_rows = (int)rows.size();
        if (rows_out) std::memcpy(rows_out, rows.data(), rows.size() * sizeof(int));
    });
}

int ptmi_set_radiosity_grids(ptmi_ctx* c, int n_prims, const float* rgb) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        need(c->app.scene.d_nodes != nullptr, "no scene loaded");
        need(rgb == nullptr || n_prims == (int)c->app.scene.h_primitives.size(), "n_prims does not match the loaded scene");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        c->app.radiosity.grids_are_scene_grids = false;               // the caller's grids replace the solver's
        viewChanged(c->app);
        c->app.scene.precomputeCDFs(rgb);
    });
}
int ptmi_set_radiosity(ptmi_ctx* c, int n_prims, const float* rgb) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        need(c->app.scene.d_nodes != nullptr, "no scene loaded");
        need(rgb == nullptr || n_prims == (int)c->app.scene.h_primitives.size(), "n_prims does not match the loaded scene");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        viewChanged(c->app);
        c->app.scene.setRadiosity(rgb);
    });
}
void ptmi_default_radiosity_params(ptmi_radiosity_params* p) {
    if (!p) return;
    p->num_iterations = 10; p->mc_samples = 64; p->use_monte_carlo = 1;
    p->enable_filtering = 0; p->use_bilateral = 1; p->filter_sigma_spatial = 1.5f; p->filter_sigma_range = 0.3f;
}
int ptmi_run_radiosity_solver(ptmi_ctx* c, const ptmi_radiosity_params* p, ptmi_radiosity_stats* stats) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        need(c->app.scene.d_nodes != nullptr, "no scene loaded");
        ptmi_radiosity_params prm;
        if (p) prm = *p; else ptmi_default_radiosity_params(&prm);
        need(prm.num_iterations >= 0 && prm.num_iterations <= 1000, "num_iterations must be in [0, 1000]");
        need(prm.mc_samples >= 1 && prm.mc_samples <= 65536, "mc_samples must be in [1, 65536]");
        need(prm.filter_sigma_spatial > 0.0f && prm.filter_sigma_range > 0.0f, "filter sigmas must be positive");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        RadiosityState& r = c->app.radiosity;
        viewChanged(c->app);
        r.num_iterations = prm.num_iterations; r.mc_samples = prm.mc_samples; r.use_monte_carlo = prm.use_monte_carlo != 0;
        RadiosityStats st;
        r.runSolver(c->app.scene, c->app.render.d_jump, prm.enable_filtering != 0, prm.use_bilateral != 0,
                    prm.filter_sigma_spatial, prm.filter_sigma_range, c->app.render.stream, &st, c->app.config.fast_tree);
        // the grids (Triangle/Quad::grid, ::radiosity_grid) stay on the device; the host copies the filter button and
        // "Use Raw CDFs" work from are fetched when one of them is pressed (sync_solver_grids)
        c->app.scene.h_count_grids.clear(); c->app.scene.h_radiosity_grids.clear();
        r.grids_are_scene_grids = true;
        c->app.scene.h_filtered_formfactor.clear(); c->app.scene.h_filtered_radiosity.clear();
        c->app.scene.precomputeCDFsDevice(r.d.rad_grid, 0, c->app.render.stream);   // ui_windows.h:189, from the solver's device grids
        c->app.scene.setRadiosity(r.h_radiosity.data());                 // ui_windows.h:190-191 (primitive upload)
        if (stats) {
            stats->seconds = st.seconds; stats->form_factor_ms = st.form_factor_ms; stats->iteration_ms = st.iteration_ms;
            stats->grid_ms = st.grid_ms; stats->pairs = st.pairs; stats->rays = st.rays;
            stats->cert_chain = st.cert_chain; stats->cert_fallback = st.cert_fallback; stats->walk = st.walk;
        }
    });
}
int ptmi_get_radiosity_solution(const ptmi_ctx* c, float* form_factors, float* radiosity, float* unshot, float* grid, float* radiosity_grid) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        const RadiosityState& r = c->app.radiosity;
        need(r.is_calculated, "no radiosity solution (run ptmi_run_radiosity_solver first)");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        if (grid || radiosity_grid) const_cast<RadiosityState&>(r).fetchGrids();
        if (form_factors) r.readFormFactors(form_factors);
        if (radiosity) std::memcpy(radiosity, r.h_radiosity.data(), r.h_radiosity.size() * sizeof(float));
        if (unshot) std::memcpy(unshot, r.h_unshot.data(), r.h_unshot.size() * sizeof(float));
        if (grid) std::memcpy(grid, r.h_grid.data(), r.h_grid.size() * sizeof(float));
        if (radiosity_grid) std::memcpy(radiosity_grid, r.h_radiosity_grid.data(), r.h_radiosity_grid.size() * sizeof(float));
    });
}
// after a solver run the scene's grids live on the device only: bring them to the host side the first time they are needed
static void sync_solver_grids(ptmi_ctx* c) {
    RadiosityState& r = c->app.radiosity;
    if (!r.is_calculated) return;
    if (c->app.scene.h_count_grids.empty()) { r.fetchGrids(); c->app.scene.h_count_grids = r.h_grid; }
    if (c->app.scene.h_radiosity_grids.empty() && r.grids_are_scene_grids) { r.fetchGrids(); c->app.scene.h_radiosity_grids = r.h_radiosity_grid; }
}
int ptmi_apply_grid_filter(ptmi_ctx* c, int use_bilateral, float sigma_spatial, float sigma_range) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        need(c->app.scene.d_nodes != nullptr, "no scene loaded");
        need(sigma_spatial > 0.0f && sigma_range > 0.0f, "filter sigmas must be positive");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        sync_solver_grids(c);
        viewChanged(c->app);
        c->app.scene.precomputeCDFsFromFiltered(use_bilateral != 0, sigma_spatial, sigma_range, c->app.render.stream);
    });
}
int ptmi_use_raw_cdfs(ptmi_ctx* c) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        sync_solver_grids(c);
        need(!c->app.scene.h_radiosity_grids.empty(), "the scene has no radiosity grids");
        viewChanged(c->app);
        c->app.scene.precomputeCDFs(c->app.scene.h_radiosity_grids.data());
    });
}
int ptmi_get_filtered_pdfs(const ptmi_ctx* c, float* formfactor, float* radiosity) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        need(!c->app.scene.h_filtered_radiosity.empty(), "no filtered pdfs (call ptmi_apply_grid_filter first)");
        if (formfactor) std::memcpy(formfactor, c->app.scene.h_filtered_formfactor.data(), c->app.scene.h_filtered_formfactor.size() * sizeof(float));
        if (radiosity) std::memcpy(radiosity, c->app.scene.h_filtered_radiosity.data(), c->app.scene.h_filtered_radiosity.size() * sizeof(float));
    });
}
int ptmi_get_precomputed_cdfs(const ptmi_ctx* c, float* out) {
    return guarded([&] {
        need(c && out, "NULL argument");
        need(c->app.scene.d_precomputed_cdfs != nullptr, "no precomputed CDFs");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        const std::vector<float>& h = const_cast<SceneState&>(c->app.scene).precomputedCdfsHost();
        std::memcpy(out, h.data(), h.size() * sizeof(float));
    });
}

int ptmi_update_resolution(ptmi_ctx* c, int width, int height, const ptmi_tiling* tiling) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        TileMap tm;
        if (tiling) { tm.n_ranks = tiling->n_ranks; tm.rank = tiling->rank; tm.row_block = tiling->row_block; }
        c->app.render.seed_base = c->app.config.seed_base;
        viewChanged(c->app);
        c->app.render.updateResolution(width, height, tiling ? &tm : nullptr);
    });
}

int ptmi_set_camera(ptmi_ctx* c, const ptmi_camera* cam) {
    return guarded([&] {
        need(c && cam, "NULL argument");
        AppConfig& cfg = c->app.config;
        cfg.camera_origin = v3(cam->origin); cfg.look_at = v3(cam->lookat); cfg.up = v3(cam->vup);
        cfg.fov = cam->vfov_deg; cfg.orbit = cam->orbit != 0;
        accumReset(c->app);
        featuresStale(c->app);
        Sensor& s = c->app.render.h_camera;
        const int w = s.image_width, h = s.image_height; const float aspect = s.aspect;
        s = Sensor(cfg.camera_origin, cfg.look_at, cfg.up, cfg.fov, 1.0f);    // application.h:107-113
        s.yaw = cam->yaw_deg; s.pitch = cam->pitch_deg;
        s.image_width = w; s.image_height = h;
        if (w > 0) { s.aspect = aspect; s.updateCamera(); }
    });
}

int ptmi_set_config(ptmi_ctx* c, const ptmi_config* cfg) {
    return guarded([&] {
        need(c && cfg, "NULL argument");
        need(cfg->spp >= 1 && cfg->spp < (1 << 24), "spp must be in [1, 2^24)");
        need(cfg->max_depth >= 1 && cfg->max_depth <= 255, "max_depth must be in [1, 255]");
        need(cfg->sampling_mode >= 0 && cfg->sampling_mode <= 4, "sampling_mode must be 0..4 (render_config.h:38-44)");
        need(cfg->mis_bsdf_fraction >= 0.0f && cfg->mis_bsdf_fraction <= 1.0f, "mis_bsdf_fraction must be in [0, 1]");
        need(cfg->integrator == 0 || cfg->integrator == 1, "integrator must be 0 (PathTracing) or 1 (Radiosity)");
        need(cfg->segments_per_launch >= 0, "segments_per_launch must be >= 0");
        need(cfg->streams >= 0 && cfg->streams <= RenderState::kMaxChunks, "streams must be 0..4");
        need(cfg->next_event == 0 || cfg->next_event == 1, "next_event must be 0 or 1");
        needNone(configRefusal(presentFeatures(c->app, cfg->next_event != 0), cfg->integrator, cfg->sampling_mode, cfg->fast_tree));
        AppConfig& a = c->app.config;                    // every check is above this line: a rejected config changes nothing
        a.spp = cfg->spp; a.max_depth = cfg->max_depth; a.sampling_mode = (SamplingMode)cfg->sampling_mode;
        a.mis_bsdf_fraction = cfg->mis_bsdf_fraction;
        a.current_integrator = cfg->integrator ? IntegratorType::Radiosity : IntegratorType::PathTracing;
        a.seed_base = cfg->seed_base; a.segments_per_launch = cfg->segments_per_launch; a.collect_stats = cfg->collect_stats != 0;
        c->app.render.allow_tile8 = cfg->wave_tiles != 0;
        c->app.render.want_chunks = cfg->streams;
        c->app.render.download_image = cfg->download_image != 0;
        a.fast_tree = cfg->fast_tree != 0;
        a.next_event = cfg->next_event != 0;
        viewChanged(c->app);
    });
}

void ptmi_default_env_params(ptmi_env_params* p) {
    if (!p) return;
    const EnvParams d;
    p->scale = d.scale; p->rotation_deg = d.rotation_deg; p->select_fraction = d.select_fraction;
}
static EnvParams env_params(const ptmi_env_params* p) {
    EnvParams e;
    if (p) { e.scale = p->scale; e.rotation_deg = p->rotation_deg; e.select_fraction = p->select_fraction; }
    return e;
}
int ptmi_check_env_params(const ptmi_env_params* p) {
    return guarded([&] { need(p != nullptr, "NULL argument"); checkEnvParams(env_params(p)); });
}
int ptmi_set_environment(ptmi_ctx* c, int width, int height, const float* rgb, const ptmi_env_params* p) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        if (rgb) {
            needRoute(c, kRouteEnvironment);
            c->app.env.set(width, height, rgb, env_params(p));       // every check is done before anything changes
        } else c->app.env.drop();
        viewChanged(c->app);                                         // other light: the temporal history holds another image
    });
}
int ptmi_environment_info(const ptmi_ctx* c, int* width, int* height, float* total) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        const EnvState& e = c->app.env;
        if (width) *width = e.present() ? e.h.width : 0;
        if (height) *height = e.present() ? e.h.height : 0;
        if (total) *total = e.present() ? e.h.total : 0.0f;
    });
}
int ptmi_host_env_table(int width, int height, const float* rgb, const ptmi_env_params* p, float* z, float* marginal_cdf, float* row_cdf,
                        float* texel, float* total) {
    return guarded([&] {
        EnvHostTable t;
        buildEnvTable(width, height, rgb, env_params(p), t);
        if (z) std::memcpy(z, t.z.data(), t.z.size() * sizeof(float));
        if (marginal_cdf) std::memcpy(marginal_cdf, t.marginal.data(), t.marginal.size() * sizeof(float));
        if (row_cdf) std::memcpy(row_cdf, t.row_cdf.data(), t.row_cdf.size() * sizeof(float));
        if (texel) std::memcpy(texel, t.texel.data(), t.texel.size() * sizeof(float));
        if (total) *total = t.total;
    });
}

int ptmi_check_surfaces(int n_prims, const int* kind, const float* ior) {
    return guarded([&] { checkSurfaces(n_prims, kind, ior); });
}
// ptmi_set_surfaces (rough_api false: kinds 0 .. 2, no roughness) and ptmi_set_surfaces_rough
static void setSurfacesChecked(ptmi_ctx* c, int n_prims, const int* kind, const float* ior, const float* roughness, bool rough_api) {
    needScene(c);
    if (kind) {
        need(n_prims == (int)c->app.scene.h_primitives.size(), "n_prims does not match the loaded scene");
        if (rough_api) checkSurfacesRough(n_prims, kind, ior, roughness);
        else checkSurfaces(n_prims, kind, ior);
        bool specular = false;
        for (int i = 0; i < n_prims; i++) specular = specular || kind[i] != kSurfaceDiffuse;
        if (specular) needRoute(c, kRouteSurfaces);
    }
    c->app.scene.setSurfaces(kind, ior, roughness);              // every check is done before anything changes
    viewChanged(c->app);                                         // other materials: the temporal history holds another image
}
int ptmi_set_surfaces(ptmi_ctx* c, int n_prims, const int* kind, const float* ior) {
    return guarded([&] { setSurfacesChecked(c, n_prims, kind, ior, nullptr, false); });
}
int ptmi_check_surfaces_rough(int n_prims, const int* kind, const float* ior, const float* roughness) {
    return guarded([&] { checkSurfacesRough(n_prims, kind, ior, roughness); });
}
int ptmi_set_surfaces_rough(ptmi_ctx* c, int n_prims, const int* kind, const float* ior, const float* roughness) {
    return guarded([&] { setSurfacesChecked(c, n_prims, kind, ior, roughness, true); });
}
int ptmi_surface_counts(const ptmi_ctx* c, int counts[4]) {
    return guarded([&] {
        need(c != nullptr && counts != nullptr, "NULL argument");
        for (int i = 0; i < 4; i++) counts[i] = c->app.scene.surface_counts[i];
    });
}
int ptmi_surfaces_info(const ptmi_ctx* c, int* n_mirror, int* n_glass) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        if (n_mirror) *n_mirror = c->app.scene.n_mirror;
        if (n_glass) *n_glass = c->app.scene.n_glass;
    });
}

int ptmi_check_vertex_normals(int n_prims, const float* normals) {
    return guarded([&] { checkVertexNormals(n_prims, normals); });
}
int ptmi_host_classify_vertex_normals(int n_prims, const int* type, const float* stored, const float* normals, int* smooth, int* n_smooth) {
    return guarded([&] {
        need(type && stored, "NULL argument");
        checkVertexNormals(n_prims, normals);
        std::vector<Primitive> prims((size_t)n_prims);
        for (int i = 0; i < n_prims; i++) {
            need(type[i] == 0 || type[i] == 1, "type must be 0 (triangle) or 1 (quad)");
            prims[i].type = type[i] ? PRIM_QUAD : PRIM_TRIANGLE;
            prims[i].normal = mk3(stored[3 * i], stored[3 * i + 1], stored[3 * i + 2]);
        }
        checkVertexNormals(prims, n_prims, normals);
        std::vector<unsigned char> s;
        const int count = classifyVertexNormals(prims, normals, s);
        if (smooth) for (int i = 0; i < n_prims; i++) smooth[i] = s[i];
        if (n_smooth) *n_smooth = count;
    });
}
int ptmi_set_vertex_normals(ptmi_ctx* c, int n_prims, const float* normals) {
    return guarded([&] {
        needScene(c);
        std::vector<unsigned char> smooth;
        int smooth_count = 0;
        if (normals) {
            checkVertexNormals(c->app.scene.h_primitives, n_prims, normals);
            smooth_count = classifyVertexNormals(c->app.scene.h_primitives, normals, smooth);
            if (smooth_count > 0) needRoute(c, kRouteVertexNormals);
        }
        c->app.scene.setVertexNormals(normals, smooth, smooth_count);   // every check is done before anything changes
        viewChanged(c->app);                                         // other shading: the temporal history holds another image
    });
}
int ptmi_vertex_normals_info(const ptmi_ctx* c, int* n_smooth) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        if (n_smooth) *n_smooth = c->app.scene.n_smooth;
    });
}

int ptmi_check_albedo_texture(int width, int height, const float* texels, int filter, int n_prims, const float* uv, const int* textured) {
    return guarded([&] { checkAlbedoTexture(width, height, texels, filter, n_prims, uv, textured); });
}
int ptmi_set_albedo_texture(ptmi_ctx* c, int width, int height, const float* texels, int filter, int n_prims, const float* uv, const int* textured) {
    return guarded([&] {
        needScene(c);
        if (texels) {
            checkAlbedoTexture(c->app.scene.h_primitives, width, height, texels, filter, n_prims, uv, textured);
            if (countTextured(n_prims, textured) > 0) needRoute(c, kRouteAlbedoTexture);
        }
        c->app.scene.setAlbedoTexture(width, height, texels, filter, uv, textured);   // every check is done before anything changes
        viewChanged(c->app);                                         // other colours: the temporal history holds another image
    });
}
int ptmi_albedo_texture_info(const ptmi_ctx* c, int* n_textured, int* width, int* height, int* filter) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        const SceneState& sc = c->app.scene;
        if (n_textured) *n_textured = sc.n_textured;
        if (width) *width = sc.tex_width;
        if (height) *height = sc.tex_height;
        if (filter) *filter = sc.tex_filter;
    });
}

static void checkFeatureShading(int flags) {
    need(flags >= 0 && flags <= 3, "feature shading: flags must be in [0, 3] (PTMI_FEATURE_TEXTURED_ALBEDO | PTMI_FEATURE_SHADING_NORMAL)");
}
int ptmi_check_feature_shading(int flags) {
    return guarded([&] { checkFeatureShading(flags); });
}
int ptmi_set_feature_shading(ptmi_ctx* c, int flags) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        checkFeatureShading(flags);
        if (flags == c->app.feature_shading) return;
        c->app.feature_shading = flags;
        featuresRedefined(c->app);                                   // the image and an accumulation stay as they are
    });
}
int ptmi_feature_shading(const ptmi_ctx* c, int* flags) {
    return guarded([&] {
        need(c && flags, "NULL argument");
        *flags = c->app.feature_shading;
    });
}

// the frame ptmi_host_camera_frame derives (no context)
static void hostCameraFrame(const ptmi_camera* cam, int width, int height, float* out12) {
    Sensor s(v3(cam->origin), v3(cam->lookat), v3(cam->vup), cam->vfov_deg, 1.0f);
    s.yaw = cam->yaw_deg; s.pitch = cam->pitch_deg;
    s.image_width = width; s.image_height = height;
    s.aspect = (float)width / (float)height;
    cameraFrame12(s, cam->orbit != 0, out12);
}
int ptmi_check_lens(float radius, float focus_distance) {
    return guarded([&] {
        checkLens(radius, focus_distance);
        if (!(radius > 0.0f)) return;
        ptmi_camera cam; ptmi_default_camera(&cam);      // no context, no camera: the block over the default camera, a square image
        float frame[12], block[kLensBlockFloats];
        hostCameraFrame(&cam, 1, 1, frame);
        lensBlock(frame, 1, 1, radius, focus_distance, block);
    });
}
int ptmi_host_lens_block(const ptmi_camera* cam, int width, int height, float radius, float focus_distance, float* out24) {
    return guarded([&] {
        need(cam && out24, "NULL argument");
        need(width > 0 && height > 0, "width and height must be positive");
        float frame[12], block[kLensBlockFloats];
        hostCameraFrame(cam, width, height, frame);
        lensBlock(frame, width, height, radius, focus_distance, block);
        std::memcpy(out24, block, sizeof block);         // a rejected call writes nothing
    });
}
int ptmi_set_lens(ptmi_ctx* c, float radius, float focus_distance) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        LensState& l = c->app.lens;
        float focus = focus_distance;
        if (radius == 0.0f && !(focus_distance > 0.0f) && !std::isnan(focus_distance)) focus = 0.0f;   // "no lens": the focus is the default again
        else checkLens(radius, focus_distance);
        if (radius > 0.0f) {
            needRoute(c, kRouteLens);
            if (c->app.render.tile.width > 0) {          // a resolution is set: the block over the camera as it is now must be finite
                float frame[12], block[kLensBlockFloats];
                cameraFrame12(c->app.render.h_camera, c->app.config.orbit, frame);
                lensBlock(frame, c->app.render.tile.width, c->app.render.tile.height, radius, focus, block);
            }
        }
        if (radius == l.radius && focus == l.focus) return;   // every check is above this line
        l.radius = radius; l.focus = focus;
        accumReset(c->app);                              // what ptmi_set_camera drops
        featuresStale(c->app);
    });
}
int ptmi_lens(const ptmi_ctx* c, float* radius, float* focus_distance) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        if (radius) *radius = c->app.lens.radius;
        if (focus_distance) *focus_distance = lensFocus(c->app);
    });
}

// ---- participating medium --------------------------------------------------------------------------------------------------------
static Medium mediumOf(const ptmi_medium* p) {
    Medium m;
    for (int k = 0; k < 3; k++) { m.lo[k] = p->lo[k]; m.hi[k] = p->hi[k]; m.albedo[k] = p->albedo[k]; }
    m.sigma_t = p->sigma_t; m.g = p->g;
    return m;
}
static void mediumTo(const Medium& m, ptmi_medium* p) {
    for (int k = 0; k < 3; k++) { p->lo[k] = m.lo[k]; p->hi[k] = m.hi[k]; p->albedo[k] = m.albedo[k]; }
    p->sigma_t = m.sigma_t; p->g = m.g;
}
void ptmi_default_medium(ptmi_medium* p) {
    if (p) mediumTo(Medium(), p);
}
int ptmi_check_medium(const ptmi_medium* p) {
    return guarded([&] { need(p != nullptr, "NULL argument"); checkMedium(mediumOf(p)); });
}
int ptmi_host_medium_block(const ptmi_medium* p, float* out12) {
    return guarded([&] {
        need(p && out12, "NULL argument");
        float block[kMediumBlockFloats];
        mediumBlock(mediumOf(p), block);
        std::memcpy(out12, block, sizeof block);         // a rejected call writes nothing
    });
}
int ptmi_set_medium(ptmi_ctx* c, const ptmi_medium* p) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        MediumState& s = c->app.scene.medium;
        Medium m;                                        // NULL: no medium
        if (p) { m = mediumOf(p); checkMedium(m); }
        if (m.sigma_t > 0.0f) {
            need(c->app.scene.d_nodes != nullptr, "no scene loaded");
            needRoute(c, kRouteMedium);
            float corners[24];                           // rays now start inside the box: its corners are the farthest such points
            mediumCorners(m, corners);
            for (int i = 0; i < 8; i++) c->app.scene.checkQuadOrigin(corners + 3 * i, nullptr, "medium");
        } else m = Medium();                             // sigma_t 0 is no medium, whatever the other fields say
        bool same = m.sigma_t == s.m.sigma_t && m.g == s.m.g;       // by value: -0 is the 0 the scene has
        for (int k = 0; k < 3; k++) same = same && m.lo[k] == s.m.lo[k] && m.hi[k] == s.m.hi[k] && m.albedo[k] == s.m.albedo[k];
        if (same) return;                                // every check is above this line
        s.m = m;
        accumReset(c->app);                              // the feature buffers and the temporal history do not see the medium:
        c->app.render.dn.image_current = false;          // they stay; the image and the accumulation's variance show the old one
        c->app.render.dn.variance_valid = false;
    });
}
int ptmi_medium_info(const ptmi_ctx* c, ptmi_medium* out, int* on) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        const MediumState& s = c->app.scene.medium;
        if (out) mediumTo(s.m, out);
        if (on) *on = s.on() ? 1 : 0;
    });
}

int ptmi_get_camera_frame(const ptmi_ctx* c, float* out12) {
    return guarded([&] {
        need(c && out12, "NULL argument");
        cameraFrame12(c->app.render.h_camera, c->app.config.orbit, out12);              // what renderFrame() would derive
    });
}

int ptmi_local_rows(const ptmi_ctx* c, int* n_rows) {
    return guarded([&] { need(c && n_rows, "NULL argument"); *n_rows = c->app.render.tile.local_rows; });
}
int ptmi_local_row_map(const ptmi_ctx* c, int* rows_out) {
    return guarded([&] {
        need(c && rows_out, "NULL argument");
        const std::vector<int> rows = localRowMap(c->app.render.tile);
        std::memcpy(rows_out, rows.data(), rows.size() * sizeof(int));
    });
}

int ptmi_render_frame(ptmi_ctx* c, ptmi_stats* stats) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        FrameStats fs;
        renderFrame(c->app, stats ? &fs : nullptr);
        if (stats) copy_frame_stats(fs, *stats);
    });
}

int ptmi_render_frames(ptmi_ctx* c, int n_frames, ptmi_stats* stats) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        FrameStats fs;
        renderFrames(c->app, n_frames, stats ? &fs : nullptr);
        if (stats) copy_frame_stats(fs, *stats);
    });
}
int ptmi_select_frame(ptmi_ctx* c, int frame) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); selectFrame(c->app, frame); });
}

int ptmi_device_image(const ptmi_ctx* c, void** d_rgb8, void** d_radiance) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        need(c->app.render.d_image != nullptr, "buffers not allocated");
        if (d_rgb8) *d_rgb8 = c->app.render.d_image;
        if (d_radiance) *d_radiance = c->app.render.d_radiance;
    });
}

int ptmi_read_image(const ptmi_ctx* c, unsigned char* rgb8, float* radiance) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        const RenderState& r = c->app.render;
        need(r.d_image != nullptr, "buffers not allocated");
        readImagePair(c->app.device_id, r.n_local, r.d_image, r.d_radiance, rgb8, radiance);                        // application.h:211
    });
}

int ptmi_copy_image_device(const ptmi_ctx* c, void* d_rgb8_dst, void* d_radiance_dst) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        const RenderState& r = c->app.render;
        need(r.d_image != nullptr, "buffers not allocated");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        if (d_rgb8_dst) PTMI_HIP(hipMemcpyAsync(d_rgb8_dst, r.d_image, r.n_local * 3, hipMemcpyDeviceToDevice, r.stream));
        if (d_radiance_dst) PTMI_HIP(hipMemcpyAsync(d_radiance_dst, r.d_radiance, r.n_local * 3 * sizeof(float), hipMemcpyDeviceToDevice, r.stream));
        PTMI_HIP(hipStreamSynchronize(r.stream));
    });
}

int ptmi_host_image(const ptmi_ctx* c, const unsigned char** rgb8, uint64_t* n_bytes) {
    return guarded([&] {
        need(c && rgb8, "NULL argument");
        need(c->app.render.h_image != nullptr, "buffers not allocated");
        *rgb8 = c->app.render.h_image;
        if (n_bytes) *n_bytes = (uint64_t)c->app.render.n_local * 3;
    });
}

// ---- multi-GPU frame exchange (csrc/dist.hip) ----
int ptmi_dist_unique_id(void* out_id) {
    return guarded([&] { need(out_id != nullptr, "NULL argument"); distUniqueId(out_id); });
}
int ptmi_dist_init(ptmi_ctx* c, const void* id, int n_ranks, int rank) {
    return guarded([&] {
        need(c && id, "NULL argument");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        c->app.render.resolve_gate = nullptr;
        c->app.dist.init(id, n_ranks, rank);
    });
}
int ptmi_dist_finalize(ptmi_ctx* c) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        c->app.render.resolve_gate = nullptr;
        c->app.dist.finalize();
    });
}
int ptmi_gather_frame(ptmi_ctx* c, int dst_rank, int what) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        c->app.dist.gatherFrame(c->app.render, dst_rank, what);
        c->app.render.resolve_gate = c->app.dist.gather_done;
    });
}
int ptmi_gather_wait(ptmi_ctx* c) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); PTMI_HIP(hipSetDevice(c->app.device_id)); c->app.dist.wait(); });
}
int ptmi_frame_device(const ptmi_ctx* c, void** d_rgb8, void** d_radiance) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        const DistState& d = c->app.dist;
        need(d.d_frame_rgb || d.d_frame_rad, "no gathered frame on this rank (ptmi_gather_frame with dst_rank = this rank first)");
        if (d_rgb8) *d_rgb8 = d.have_rgb ? d.d_frame_rgb : nullptr;
        if (d_radiance) *d_radiance = d.have_rad ? d.d_frame_rad : nullptr;
    });
}
int ptmi_read_frame(ptmi_ctx* c, unsigned char* rgb8, float* radiance) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        DistState& d = c->app.dist;
        PTMI_HIP(hipSetDevice(c->app.device_id));
        need(!rgb8 || d.have_rgb, "the 8-bit frame was never gathered to this rank");
        need(!radiance || d.have_rad, "the radiance frame was never gathered to this rank");
        d.wait();
        const size_t n = (size_t)d.frame_w * (size_t)d.frame_h * 3;
        if (rgb8) PTMI_HIP(hipMemcpy(rgb8, d.d_frame_rgb, n, hipMemcpyDeviceToHost));
        if (radiance) PTMI_HIP(hipMemcpy(radiance, d.d_frame_rad, n * sizeof(float), hipMemcpyDeviceToHost));
    });
}
int ptmi_dist_barrier(ptmi_ctx* c) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); PTMI_HIP(hipSetDevice(c->app.device_id)); c->app.dist.barrier(); });
}
int ptmi_dist_allreduce_max(ptmi_ctx* c, double* value) {
    return guarded([&] {
        need(c && value, "NULL argument");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        *value = c->app.dist.allreduceMax(*value);
    });
}
int ptmi_dist_comm_count(ptmi_ctx* c, int* n_ranks) {
    return guarded([&] { need(c && n_ranks, "NULL argument"); PTMI_HIP(hipSetDevice(c->app.device_id)); *n_ranks = c->app.dist.commCount(); });
}

int ptmi_host_fast_tree_build(ptmi_host_scene* s, int max_leaf, float c_trav, float c_tri, int* n_nodes, int* depth, double* sah) {
    return guarded([&] {
        need(s != nullptr, "scene is NULL");
        need(max_leaf >= 1 && max_leaf <= kWideMaxLeaf, "max_leaf must be 1..3");
        need(c_trav >= 0.0f && c_tri > 0.0f, "c_trav must be >= 0 and c_tri > 0");
        SceneState& sc = s->scene;
        sc.wide_params.max_leaf = max_leaf; sc.wide_params.c_trav = c_trav; sc.wide_params.c_tri = c_tri;
        try { buildWideBVH(sc.h_primitives, sc.wide_params, sc.h_wide); }
        catch (const std::invalid_argument& e) { throw ArgError(e.what()); }
        if (n_nodes) *n_nodes = sc.h_wide.n_nodes;
        if (depth) *depth = sc.h_wide.depth;
        if (sah) *sah = sc.h_wide.sah;
    });
}
int ptmi_host_fast_tree_stats(const ptmi_host_scene* s, int* out13) {
    return guarded([&] {
        need(s && out13, "NULL argument");
        need(!s->scene.h_wide.empty(), "no fast tree built (ptmi_host_fast_tree_build)");
        for (int i = 0; i < 9; i++) out13[i] = s->scene.h_wide.fill_hist[i];
        for (int i = 0; i < 4; i++) out13[9 + i] = s->scene.h_wide.leaf_hist[i];
    });
}
int ptmi_host_fast_tree_intersect(const ptmi_host_scene* s, int n, const float* o, const float* d, float t_min, float t_max,
                                  int* prim, float* t, uint64_t* counts) {
    return guarded([&] {
        need(s && o && d && prim && t, "NULL argument");
        const SceneState& sc = s->scene;
        need(!sc.h_wide.empty(), "no fast tree built (ptmi_host_fast_tree_build)");
        std::vector<int> ref_slot(sc.h_primitives.size());
        for (size_t k = 0; k < sc.bvh_indices.size(); k++) ref_slot[(size_t)sc.bvh_indices[k]] = (int)k;
        WideWalkCounters cn;
        for (int i = 0; i < n; i++) {
            float th = 0.0f;
            prim[i] = wideIntersectHost(sc.h_wide, sc.h_primitives, ref_slot, v3(o + 3 * i), v3(d + 3 * i), t_min, t_max, th, &cn);
            t[i] = prim[i] >= 0 ? th : 0.0f;
        }
        if (counts) { counts[0] = cn.node_visits; counts[1] = cn.prim_tests; counts[2] = cn.max_stack; }
    });
}

// ---- progressive and adaptive accumulation ----
void ptmi_default_adaptive_params(ptmi_adaptive_params* p) {
    if (!p) return;
    const AdaptiveParams d;
    p->min_passes = d.min_passes; p->max_passes = d.max_passes; p->threshold = d.threshold; p->floor = d.floor;
}
int ptmi_accum_reset(ptmi_ctx* c) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); accumReset(c->app); });
}
int ptmi_accum_pass(ptmi_ctx* c, const ptmi_adaptive_params* params, ptmi_pass_stats* stats) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        AdaptiveParams prm;
        if (params) { prm.min_passes = params->min_passes; prm.max_passes = params->max_passes; prm.threshold = params->threshold; prm.floor = params->floor; }
        PassStats ps;
        accumPass(c->app, params ? &prm : nullptr, stats ? &ps : nullptr);
        if (stats) {
            stats->pass = ps.pass; stats->active_before = ps.active_before; stats->active_after = ps.active_after;
            copy_frame_stats(ps.frame, *stats);
        }
    });
}
int ptmi_read_sample_counts(const ptmi_ctx* c, uint32_t* counts) {
    return guarded([&] { need(c && counts, "NULL argument"); readSampleCounts(c->app, counts); });
}

// ---- feature buffers and the denoiser ----
static DenoiseParams denoise_params_from(const ptmi_denoise_params& p) {
    DenoiseParams d;
    d.iterations = p.iterations; d.sigma_color = p.sigma_color; d.color_floor = p.color_floor; d.sigma_position = p.sigma_position;
    d.normal_squarings = p.normal_squarings; d.feature_grid = p.feature_grid; d.demodulate = p.demodulate;
    return d;
}
void ptmi_default_denoise_params(ptmi_denoise_params* p) {
    if (!p) return;
    const DenoiseParams d;
    p->iterations = d.iterations; p->sigma_color = d.sigma_color; p->color_floor = d.color_floor; p->sigma_position = d.sigma_position;
    p->normal_squarings = d.normal_squarings; p->feature_grid = d.feature_grid; p->demodulate = d.demodulate;
}
int ptmi_check_denoise_params(const ptmi_denoise_params* p) {
    return guarded([&] { need(p != nullptr, "params is NULL"); checkDenoiseParams(denoise_params_from(*p)); });
}
int ptmi_render_features(ptmi_ctx* c, int grid) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); renderFeatures(c->app, grid); });
}
int ptmi_read_features(const ptmi_ctx* c, float* albedo, float* normal, float* position, float* hit_fraction) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); readFeatures(c->app, albedo, normal, position, hit_fraction); });
}
int ptmi_denoise(ptmi_ctx* c, const ptmi_denoise_params* params) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        ptmi_denoise_params p;
        ptmi_default_denoise_params(&p);
        denoise(c->app, denoise_params_from(params ? *params : p));
    });
}
int ptmi_read_denoised(const ptmi_ctx* c, unsigned char* rgb8, float* radiance) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); readDenoised(c->app, rgb8, radiance); });
}
int ptmi_denoise_timing(const ptmi_ctx* c, double* features_ms, double* denoise_ms) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        if (features_ms) *features_ms = c->app.render.dn.features_ms;
        if (denoise_ms) *denoise_ms = c->app.render.dn.denoise_ms;
    });
}

// ---- the variance-guided filter ----
static VarianceParams variance_params_from(const ptmi_variance_params& p) {
    VarianceParams v;
    v.iterations = p.iterations; v.sigma_luminance = p.sigma_luminance; v.epsilon = p.epsilon; v.sigma_position = p.sigma_position;
    v.normal_squarings = p.normal_squarings; v.feature_grid = p.feature_grid; v.demodulate = p.demodulate;
    v.source = p.source; v.spatial_radius = p.spatial_radius;
    return v;
}
void ptmi_default_variance_params(ptmi_variance_params* p) {
    if (!p) return;
    const VarianceParams v;
    p->iterations = v.iterations; p->sigma_luminance = v.sigma_luminance; p->epsilon = v.epsilon; p->sigma_position = v.sigma_position;
    p->normal_squarings = v.normal_squarings; p->feature_grid = v.feature_grid; p->demodulate = v.demodulate;
    p->source = v.source; p->spatial_radius = v.spatial_radius;
}
int ptmi_check_variance_params(const ptmi_variance_params* p) {
    return guarded([&] { need(p != nullptr, "params is NULL"); checkVarianceParams(variance_params_from(*p)); });
}
int ptmi_denoise_variance(ptmi_ctx* c, const ptmi_variance_params* params) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        ptmi_variance_params p;
        ptmi_default_variance_params(&p);
        denoiseVariance(c->app, variance_params_from(params ? *params : p));
    });
}
int ptmi_read_variance(const ptmi_ctx* c, float* variance_in, float* variance_out) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); readVariance(c->app, variance_in, variance_out); });
}
int ptmi_variance_timing(const ptmi_ctx* c, double* estimate_ms, double* filter_ms) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        if (estimate_ms) *estimate_ms = c->app.render.dn.estimate_ms;
        if (filter_ms) *filter_ms = c->app.render.dn.filter_ms;
    });
}
int ptmi_read_pass_moments(const ptmi_ctx* c, float* mean, float* m2, uint32_t* passes) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); readPassMoments(c->app, mean, m2, passes); });
}

// ---- temporal accumulation with reprojection ----
static TemporalParams temporal_params_from(const ptmi_temporal_params& p) {
    TemporalParams t;
    t.max_history = p.max_history; t.normal_min = p.normal_min; t.sigma_position = p.sigma_position; t.feature_grid = p.feature_grid;
    t.sigma_albedo = p.sigma_albedo;
    return t;
}
void ptmi_default_temporal_params(ptmi_temporal_params* p) {
    if (!p) return;
    const TemporalParams t;
    p->max_history = t.max_history; p->normal_min = t.normal_min; p->sigma_position = t.sigma_position; p->feature_grid = t.feature_grid;
    p->sigma_albedo = t.sigma_albedo;
}
int ptmi_check_temporal_params(const ptmi_temporal_params* p) {
    return guarded([&] { need(p != nullptr, "params is NULL"); checkTemporalParams(temporal_params_from(*p)); });
}
int ptmi_temporal_reset(ptmi_ctx* c) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); temporalReset(c->app); });
}
int ptmi_temporal_accumulate(ptmi_ctx* c, const ptmi_temporal_params* params, ptmi_temporal_stats* stats) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        ptmi_temporal_params p;
        ptmi_default_temporal_params(&p);
        TemporalStats st;
        temporalAccumulate(c->app, temporal_params_from(params ? *params : p), &st);
        if (stats) {
            stats->accepted = st.accepted; stats->rejected = st.rejected; stats->missed = st.missed;
            stats->seconds = st.seconds; stats->features_ms = st.features_ms;
        }
    });
}
int ptmi_read_temporal(const ptmi_ctx* c, unsigned char* rgb8, float* radiance) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); readTemporal(c->app, rgb8, radiance); });
}
int ptmi_read_history_counts(const ptmi_ctx* c, float* counts) {
    return guarded([&] { need(c && counts, "NULL argument"); readHistoryCounts(c->app, counts); });
}
int ptmi_denoise_temporal(ptmi_ctx* c, const ptmi_denoise_params* params) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        ptmi_denoise_params p;
        ptmi_default_denoise_params(&p);
        denoiseTemporal(c->app, denoise_params_from(params ? *params : p));
    });
}

// ---- the history's luminance statistics and the variance-guided filter steered by them ----
static_assert(PTMI_TEMPORAL_MIN_FRAMES == kTemporalMinFrames, "the header's constant is the kernel's");
int ptmi_set_temporal_moments(ptmi_ctx* c, int on) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); setTemporalMoments(c->app, on); });
}
int ptmi_get_temporal_moments(const ptmi_ctx* c, int* on) {
    return guarded([&] { need(c && on, "NULL argument"); *on = c->app.temporal_moments; });
}
int ptmi_read_temporal_moments(const ptmi_ctx* c, float* mean, float* variance, float* frames) {
    return guarded([&] { need(c != nullptr, "ctx is NULL"); readTemporalMoments(c->app, mean, variance, frames); });
}
int ptmi_denoise_temporal_variance(ptmi_ctx* c, const ptmi_variance_params* params) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        ptmi_variance_params p;
        ptmi_default_variance_params(&p);
        denoiseTemporalVariance(c->app, variance_params_from(params ? *params : p));
    });
}

}  // extern "C"
