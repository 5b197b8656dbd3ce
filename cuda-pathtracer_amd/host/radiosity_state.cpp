// radiosity_state.cpp — the host half of the radiosity pre-pass: RadiosityState (application_state.h:688-787).  runSolver chooses
// the visibility walk, uploads the load-order geometry and runs the solver's kernels (csrc/radiosity.hip lists them).
#include "application_state.h"

#include <chrono>
#include <cstring>

namespace ptmi {

void RadiosityState::cleanup() {
    void* ptrs[] = {(void*)d.geo, (void*)d.slot_of, (void*)d.bsdf, d.radiosity, d.unshot[0], d.unshot[1], d.form_factors, d.grid, d.rad_grid, d.rays, d.row_jump};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    d = RadiosityBuffers();
    is_calculated = false; host_grids_current = false; grids_are_scene_grids = false;
}

void RadiosityState::runSolver(SceneState& scene, const uint32_t* d_jump, bool enable_filtering, bool use_bilateral,
                               float filter_sigma_spatial, float filter_sigma_range, hipStream_t stream, RadiosityStats* stats, bool fast_tree) {
    if (!scene.d_nodes) throw ArgError("runSolver: no scene loaded");
    const int n = (int)scene.h_primitives.size();
    if (n > 46340) throw ArgError("runSolver: more than 46340 primitives (the pair index i * n + j is an int in the reference too)");
    if (num_iterations < 0 || num_iterations > 1000) throw ArgError("runSolver: num_iterations out of range");
    if (mc_samples < 1 || mc_samples > 65536) throw ArgError("runSolver: mc_samples out of range");
    const bool timing = getenv("PTMI_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_start = now();
    cleanup();                                                                       // :703
    const double t_cleanup = now();
    // for (i) setRadiosity(Le), setUnshotRad(Le)  (:697-701) + the load-order geometry the kernels sample
    std::vector<float4> geo((size_t)n * 6), bsdf((size_t)n), rad((size_t)n);
    std::vector<int> slot_of((size_t)n);
    for (int k = 0; k < n; k++) slot_of[scene.bvh_indices[k]] = k;
    for (int p = 0; p < n; p++) {
        const Primitive& pr = scene.h_primitives[p];
        const f3 c = pr.centroid();
        int type = (int)pr.type; float type_bits; std::memcpy(&type_bits, &type, 4);
        geo[6 * p + 0] = make_float4(pr.v[0].x, pr.v[0].y, pr.v[0].z, type_bits);
        geo[6 * p + 1] = make_float4(pr.v[1].x, pr.v[1].y, pr.v[1].z, pr.area());
        geo[6 * p + 2] = make_float4(pr.v[2].x, pr.v[2].y, pr.v[2].z, pr.sampleAreaRatio());
        geo[6 * p + 3] = make_float4(pr.v[3].x, pr.v[3].y, pr.v[3].z, 0.0f);
        geo[6 * p + 4] = make_float4(pr.normal.x, pr.normal.y, pr.normal.z, 0.0f);
        geo[6 * p + 5] = make_float4(c.x, c.y, c.z, 0.0f);
        bsdf[p] = make_float4(pr.bsdf.x, pr.bsdf.y, pr.bsdf.z, 0.0f);
        rad[p] = make_float4(pr.Le.x, pr.Le.y, pr.Le.z, 0.0f);
    }
    auto upload = [&](const void* src, size_t bytes, const char* name) {
        void* p = hipMallocSafe(bytes, name);
        if (src) PTMI_HIP(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
        return p;
    };
    d.n = n; d.bvh_depth = scene.bvh_depth;
    // the visibility walk: 0 the reference's own (stackless over its tree), 1 the opt-in fast tree (AppConfig::fast_tree), 2 the
    // certified walk - the fast tree + a per-ray proof that the reference's any-hit walk gives the same answer (csrc/anyhit.h:
    // certified_blocked) - the default for triangle scenes from cert_min_prims primitives up; trees are built on first use
    {
        const bool can = scene.bvh_depth <= 30;
        int walk = 0;
        if (can && fast_tree) walk = 1;
        else if (can && (force_walk >= 2 || (force_walk < 0 && scene.certified_default && n >= cert_min_prims))) walk = 2;
        if (walk) {
            // the automatic choice falls back to the reference's walk for a scene the builder declines (and does not ask again);
            // a walk the caller asked for by name (fast_tree, force_walk) reports the failure
            const bool automatic = !fast_tree && force_walk < 0;
            if (!scene.fastReady() && !(automatic && scene.fast_declined)) {
                try { scene.buildFast(); }
                catch (const ArgError&) { if (!automatic) throw; }
            }
            if (!scene.fastReady()) walk = 0;
            if (walk == 2 && !scene.d_scene.certified_ready()) walk = 0;
        }
        d.fast_tree = walk;
    }
    d.geo = (const float4*)upload(geo.data(), geo.size() * sizeof(float4), "d_radiosity_geo");
    d.slot_of = (const int*)upload(slot_of.data(), slot_of.size() * sizeof(int), "d_radiosity_slot_of");
    d.bsdf = (const float4*)upload(bsdf.data(), bsdf.size() * sizeof(float4), "d_radiosity_bsdf");
    d.radiosity = (float4*)upload(rad.data(), rad.size() * sizeof(float4), "d_radiosity_primitives");
    d.unshot[0] = (float4*)upload(rad.data(), rad.size() * sizeof(float4), "d_radiosity_unshot0");
    d.unshot[1] = (float4*)upload(nullptr, rad.size() * sizeof(float4), "d_radiosity_unshot1");
    d.form_factors = (float*)upload(nullptr, (size_t)n * (size_t)n * sizeof(float), "d_form_factors");
    d.grid = (unsigned int*)upload(nullptr, (size_t)n * kGridSize * sizeof(unsigned int), "d_radiosity_grid_counts");
    d.rad_grid = (float4*)upload(nullptr, (size_t)n * kGridSize * sizeof(float4), "d_radiosity_grids");
    d.rays = (unsigned long long*)upload(nullptr, 3 * sizeof(unsigned long long), "d_radiosity_rays");   // rays, certified: chains, fallbacks
    // the part of the pairs' XORWOW skip-ahead that a row shares: one 160 x 160 GF(2) matrix per receiver (3.2 KB; n = 8192: 26 MB;
    // form factors 82.8 -> 79.1 ms there, 19.7 -> 14.9 ms with 4 samples; at n = 2048 the extra kernel costs what it saves)
    if (use_monte_carlo && n >= 4096) d.row_jump = (uint32_t*)upload(nullptr, (size_t)n * 160 * 5 * sizeof(uint32_t), "d_radiosity_row_jump");
    PTMI_HIP(hipMemset(d.rays, 0, 3 * sizeof(unsigned long long)));

    RadiosityParams prm;
    prm.num_iterations = num_iterations; prm.mc_samples = mc_samples; prm.use_monte_carlo = use_monte_carlo ? 1 : 0;
    prm.enable_filtering = enable_filtering ? 1 : 0; prm.use_bilateral = use_bilateral ? 1 : 0;
    prm.filter_sigma_spatial = filter_sigma_spatial; prm.filter_sigma_range = filter_sigma_range;

    struct Events {                                    // destroyed on every exit path
        hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } events;
    const double t_alloc = now();
    hipEvent_t* ev = events.e;
    for (int k = 0; k < 4; k++) PTMI_HIP(hipEventCreate(&ev[k]));
    PTMI_HIP(hipEventRecord(ev[0], stream));
    DeviceScene ff_scene = scene.d_scene;
    ff_scene.w_cert_debug = force_walk == 3 ? 1 : force_walk == 4 ? 2 : 0;
    launch_form_factors(ff_scene, d, prm, d_jump, stream);                       // :726-741
    PTMI_HIP(hipGetLastError());
    PTMI_HIP(hipEventRecord(ev[1], stream));
    for (int it = 0; it < num_iterations; ++it) launch_radiosity_iteration(d, it & 1, stream);   // :748-771
    final_unshot = num_iterations & 1;
    PTMI_HIP(hipGetLastError());
    PTMI_HIP(hipEventRecord(ev[2], stream));
    if (num_iterations > 0) launch_radiosity_grid(d, prm, stream);
    PTMI_HIP(hipGetLastError());
    PTMI_HIP(hipEventRecord(ev[3], stream));
    PTMI_HIP(hipStreamSynchronize(stream));
    const double t_kernels = now();

    // cudaMemcpy(h_primitives, d_radiosity_primitives, ...) (:773): the solution comes back to the host
    std::vector<float4> h4((size_t)n);
    auto unpack = [&](const float4* dev, size_t count, std::vector<float>& out) {
        PTMI_HIP(hipMemcpy(h4.data(), dev, count * sizeof(float4), hipMemcpyDeviceToHost));
        out.resize(count * 3);
        for (size_t k = 0; k < count; k++) { out[3 * k] = h4[k].x; out[3 * k + 1] = h4[k].y; out[3 * k + 2] = h4[k].z; }
    };
    unpack(d.radiosity, (size_t)n, h_radiosity);
    unpack(d.unshot[final_unshot], (size_t)n, h_unshot);
    h_radiosity_grid.clear(); h_grid.clear(); host_grids_current = false;             // the two big grids stay on the device until asked for
    is_calculated = true;
    if (timing) fprintf(stderr, "[ptmi] runSolver: cleanup %.1f ms, geometry+alloc+upload %.1f ms, kernels %.1f ms, download %.1f ms\n",
                        t_cleanup - t_start, t_alloc - t_cleanup, t_kernels - t_alloc, now() - t_kernels);
    if (stats) {
        float ms = 0.0f;
        *stats = RadiosityStats();
        PTMI_HIP(hipEventElapsedTime(&ms, ev[0], ev[3])); stats->seconds = ms * 1e-3;
        PTMI_HIP(hipEventElapsedTime(&ms, ev[0], ev[1])); stats->form_factor_ms = ms;
        PTMI_HIP(hipEventElapsedTime(&ms, ev[1], ev[2])); stats->iteration_ms = ms;
        PTMI_HIP(hipEventElapsedTime(&ms, ev[2], ev[3])); stats->grid_ms = ms;
        stats->pairs = (uint64_t)n * (uint64_t)n;
        unsigned long long rays[3] = {0, 0, 0};
        PTMI_HIP(hipMemcpy(rays, d.rays, sizeof rays, hipMemcpyDeviceToHost));
        stats->rays = rays[0]; stats->cert_chain = rays[1]; stats->cert_fallback = rays[2]; stats->walk = d.fast_tree;
    }
}

void RadiosityState::fetchGrids() {
    if (!is_calculated) throw ArgError("no radiosity solution");
    if (host_grids_current) return;
    const size_t cells = (size_t)d.n * kGridSize;
    std::vector<float4> h4(cells);
    PTMI_HIP(hipMemcpy(h4.data(), d.rad_grid, cells * sizeof(float4), hipMemcpyDeviceToHost));
    h_radiosity_grid.resize(cells * 3);
    for (size_t k = 0; k < cells; k++) { h_radiosity_grid[3 * k] = h4[k].x; h_radiosity_grid[3 * k + 1] = h4[k].y; h_radiosity_grid[3 * k + 2] = h4[k].z; }
    std::vector<unsigned int> counts(cells);
    PTMI_HIP(hipMemcpy(counts.data(), d.grid, cells * sizeof(unsigned int), hipMemcpyDeviceToHost));
    h_grid.resize(cells);
    for (size_t k = 0; k < cells; k++) h_grid[k] = (float)counts[k];
    host_grids_current = true;
}

void RadiosityState::readFormFactors(float* out) const {
    if (!is_calculated) throw ArgError("no radiosity solution");
    PTMI_HIP(hipMemcpy(out, d.form_factors, (size_t)d.n * (size_t)d.n * sizeof(float), hipMemcpyDeviceToHost));
}

}  // namespace ptmi
