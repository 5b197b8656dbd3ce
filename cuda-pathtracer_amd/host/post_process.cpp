// post_process.cpp — what runs on a finished image: feature buffers, the a-trous denoiser, temporal accumulation
#include "application_state.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace ptmi {

// ------------------------------------------------------------------------------------------------
// feature buffers and the denoiser (include/ptmi.h: ptmi_render_features, ptmi_denoise)
// ------------------------------------------------------------------------------------------------
void featuresStale(ApplicationState& g) {
    g.render.dn.features_valid = false;
    g.render.dn.variance_valid = false;
    g.render.dn.image_current = false;                 // the image shows the scene / view / config as it was before the change
}

// the features change their meaning and the image does not (ptmi_set_feature_shading): the image stays current and an
// accumulation goes on; the temporal history holds albedo and normal of the old kind
void featuresRedefined(ApplicationState& g) {
    g.render.dn.features_valid = false;
    g.render.dn.variance_valid = false;
    temporalReset(g);
}

static void needEvents(ApplicationState& g, size_t n) {
    while (g.event_pool.size() < n) { hipEvent_t ev; PTMI_HIP(hipEventCreate(&ev)); g.event_pool.push_back(ev); }
}

void readImagePair(int device_id, size_t n_local, const unsigned char* d_rgb8, const float* d_radiance, unsigned char* rgb8, float* radiance) {
    PTMI_HIP(hipSetDevice(device_id));
    if (rgb8 && n_local) PTMI_HIP(hipMemcpy(rgb8, d_rgb8, n_local * 3, hipMemcpyDeviceToHost));
    if (radiance && n_local) PTMI_HIP(hipMemcpy(radiance, d_radiance, n_local * 3 * sizeof(float), hipMemcpyDeviceToHost));
}

void renderFeatures(ApplicationState& g, int grid) {
    RenderState& r = g.render;
    RenderState::Denoise& d = r.dn;
    if (grid < 1 || grid > 4) throw ArgError("renderFeatures: grid must be in [1, 4]");
    if (!g.scene.d_nodes) throw ArgError("renderFeatures: no scene loaded");
    if (!r.d_state.A) throw ArgError("renderFeatures: buffers not allocated (call updateResolution first)");
    PTMI_HIP(hipSetDevice(g.device_id));
    const size_t n = std::max<size_t>(r.n_local, 1);
    if (!d.fb.albedo) {
        try {
            d.fb.albedo = (float4*)hipMallocSafe(n * sizeof(float4), "features.albedo");
            d.fb.normal = (float4*)hipMallocSafe(n * sizeof(float4), "features.normal");
            d.fb.position = (float4*)hipMallocSafe(n * sizeof(float4), "features.position");
        } catch (...) { r.freeDenoise(); throw; }
    }
    d.features_valid = false;
    FrameParams fp;
    cameraFrameParams(g, fp);
    needEvents(g, 2);
    PTMI_HIP(hipEventRecord(g.event_pool[0], r.stream));
    launch_features(g.scene.d_scene, r.tile, fp, grid, d.fb, g.scene.vertexNormalTable(), g.scene.albedoTable(), g.feature_shading, r.stream);
    PTMI_HIP(hipGetLastError());
    PTMI_HIP(hipEventRecord(g.event_pool[1], r.stream));
    PTMI_HIP(hipStreamSynchronize(r.stream));
    d.features_ms = elapsedMs(g.event_pool[0], g.event_pool[1]);
    d.grid = grid;
    d.features_valid = true;
}

void readFeatures(const ApplicationState& g, float* albedo, float* normal, float* position, float* hit_fraction) {
    const RenderState& r = g.render;
    if (!r.dn.features_valid) throw ArgError("readFeatures: no current feature buffers (ptmi_render_features first)");
    PTMI_HIP(hipSetDevice(g.device_id));
    std::vector<float4> h(r.n_local);
    const float4* src[3] = {r.dn.fb.albedo, r.dn.fb.normal, r.dn.fb.position};
    float* dst[3] = {albedo, normal, position};
    for (int k = 0; k < 3; k++) {
        if (!dst[k] && !(k == 0 && hit_fraction)) continue;
        if (r.n_local) PTMI_HIP(hipMemcpy(h.data(), src[k], r.n_local * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < r.n_local; i++) {
            if (dst[k]) { dst[k][3 * i] = h[i].x; dst[k][3 * i + 1] = h[i].y; dst[k][3 * i + 2] = h[i].z; }
            if (k == 0 && hit_fraction) hit_fraction[i] = h[i].w;
        }
    }
}

// the parameters the two a-trous filters share
// test hook: the filters' inputs, given instead of rendered
void debugSetFilterInputs(ApplicationState& g, const float* radiance, const float* albedo, const float* normal, const float* position,
                          const float* hit_fraction, int grid) {
    RenderState& r = g.render;
    RenderState::Denoise& d = r.dn;
    if (!g.scene.d_nodes) throw ArgError("no scene loaded");
    if (!r.d_state.A || !r.d_image || !r.d_radiance) throw ArgError("buffers not allocated (call updateResolution first)");
    if (r.tile.n_ranks != 1) throw ArgError("the context is tiled over more than one rank");
    if (g.config.current_integrator == IntegratorType::Radiosity) throw ArgError("the Radiosity integrator's image is not filtered");
    if (grid < 1 || grid > 4) throw ArgError("grid must be in [1, 4]");
    PTMI_HIP(hipSetDevice(g.device_id));
    const size_t n = r.n_local;                         // every size is the context's: width x height of the current resolution
    if (!d.fb.albedo) {                                 // as renderFeatures allocates them
        const size_t cap = n > 0 ? n : 1;
        try {
            d.fb.albedo = (float4*)hipMallocSafe(cap * sizeof(float4), "features.albedo");
            d.fb.normal = (float4*)hipMallocSafe(cap * sizeof(float4), "features.normal");
            d.fb.position = (float4*)hipMallocSafe(cap * sizeof(float4), "features.position");
        } catch (...) { r.freeDenoise(); throw; }
    }
    // the uploads are enqueued behind whatever the stream still holds of an earlier filter run, and waited for below
    std::vector<float4> h_a(n), h_n(n), h_x(n);
    for (size_t i = 0; i < n; i++) {
        h_a[i] = make_float4(albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2], hit_fraction[i]);
        h_n[i] = make_float4(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], 0.0f);
        h_x[i] = make_float4(position[3 * i], position[3 * i + 1], position[3 * i + 2], 0.0f);
    }
    d.features_valid = false;
    d.image_current = false;
    if (r.resolve_gate) PTMI_HIP(hipStreamWaitEvent(r.stream, r.resolve_gate, 0));   // a gather may still read the image
    if (n) {
        PTMI_HIP(hipMemcpyAsync(d.fb.albedo, h_a.data(), n * sizeof(float4), hipMemcpyHostToDevice, r.stream));
        PTMI_HIP(hipMemcpyAsync(d.fb.normal, h_n.data(), n * sizeof(float4), hipMemcpyHostToDevice, r.stream));
        PTMI_HIP(hipMemcpyAsync(d.fb.position, h_x.data(), n * sizeof(float4), hipMemcpyHostToDevice, r.stream));
        PTMI_HIP(hipMemcpyAsync(r.d_radiance, radiance, n * 3 * sizeof(float), hipMemcpyHostToDevice, r.stream));
        // rgb8 by the product's resolve at k = 1: the denoiser's tone map in its 0-iteration form reads the radiance alone
        DenoiseArgs a{};
        a.width = r.tile.width; a.height = r.tile.local_rows;
        launch_denoise(a, d.fb, r.d_radiance, 0, nullptr, nullptr, r.d_image, nullptr, r.stream);
        PTMI_HIP(hipGetLastError());
    }
    PTMI_HIP(hipStreamSynchronize(r.stream));
    d.grid = grid;
    d.features_valid = true;
    d.image_current = true;
    d.image_pass = false;
    d.variance_valid = false;
    d.denoised = false;
}

static void checkIterations(int iterations) {
    if (iterations < 0 || iterations > 10) throw ArgError("denoise: iterations must be in [0, 10]");
}
static void checkGuideParams(float sigma_position, int normal_squarings, int feature_grid, int demodulate) {
    if (!(sigma_position <= 0.0f || (sigma_position >= 1e-6f && sigma_position <= 1e12f)))
        throw ArgError("denoise: sigma_position must be <= 0 (automatic) or in [1e-6, 1e12]");
    if (normal_squarings < 0 || normal_squarings > 10) throw ArgError("denoise: normal_squarings must be in [0, 10]");
    if (feature_grid < 1 || feature_grid > 4) throw ArgError("denoise: feature_grid must be in [1, 4]");
    if (demodulate != 0 && demodulate != 1) throw ArgError("denoise: demodulate must be 0 or 1");
}

void checkDenoiseParams(const DenoiseParams& p) {
    checkIterations(p.iterations);
    if (!(p.sigma_color >= 1e-4f && p.sigma_color <= 1e4f)) throw ArgError("denoise: sigma_color must be in [1e-4, 1e4]");
    if (!(p.color_floor >= 1e-6f && p.color_floor <= 1e4f)) throw ArgError("denoise: color_floor must be in [1e-6, 1e4]");
    checkGuideParams(p.sigma_position, p.normal_squarings, p.feature_grid, p.demodulate);
}

void checkVarianceParams(const VarianceParams& p) {
    checkIterations(p.iterations);
    if (!(p.sigma_luminance >= 1e-4f && p.sigma_luminance <= 1e4f)) throw ArgError("denoise: sigma_luminance must be in [1e-4, 1e4]");
    if (!(p.epsilon >= 1e-12f && p.epsilon <= 1e4f)) throw ArgError("denoise: epsilon must be in [1e-12, 1e4]");
    checkGuideParams(p.sigma_position, p.normal_squarings, p.feature_grid, p.demodulate);
    if (p.source != 0 && p.source != 1) throw ArgError("denoise: source must be 0 (automatic) or 1 (spatial)");
    if (p.spatial_radius < 1 || p.spatial_radius > 3) throw ArgError("denoise: spatial_radius must be in [1, 3]");
}

// sigma_x of the denoiser and of the temporal step for sigma_position <= 0: fraction x the diagonal of the root box of the
// scene's BVH, in float
static float autoSigmaPosition(const ApplicationState& g, float fraction, const char* who) {
    const AABB& b = g.scene.bvh_nodes.at(0).bbox;
    const float dx = b.max.x - b.min.x, dy = b.max.y - b.min.y, dz = b.max.z - b.min.z;
    const float sigma_x = fraction * std::sqrt(dx * dx + dy * dy + dz * dz);
    if (!(sigma_x >= 1e-6f && sigma_x <= 1e12f)) throw ArgError(std::string(who) + ": the scene's bounding box gives no usable sigma_position; set one");
    return sigma_x;
}

// the constants the two filters share, from either's (checked) parameters
template <class Params>
static void filterArgs(const ApplicationState& g, const Params& p, FilterArgs& a) {
    a.width = g.render.tile.width; a.height = g.render.tile.local_rows;
    a.demodulate = p.demodulate; a.normal_squarings = p.normal_squarings;
    const float sigma_x = p.sigma_position > 0.0f ? p.sigma_position : autoSigmaPosition(g, 0.02f, "denoise");   // 2 %
    a.sigma_x2 = sigma_x * sigma_x;
}

// the filter's constants for p (parameters checked first); sigma_c[i]: the colour sigma of iteration i
static DenoiseArgs denoiseArgs(const ApplicationState& g, const DenoiseParams& p, float* sigma_c) {
    checkDenoiseParams(p);
    DenoiseArgs a;
    filterArgs(g, p, a);
    a.color_floor = p.color_floor;
    for (int i = 0; i < p.iterations; i++) sigma_c[i] = std::ldexp(p.sigma_color, -i);     // sigma_color x 2^-i, exact
    return a;
}

// the outputs and scratch of the two filters, allocated together at the first run of either
static void allocateDenoiseOutputs(RenderState& r) {
    RenderState::Denoise& d = r.dn;
    if (d.d_rgb8) return;
    const size_t n = std::max<size_t>(r.n_local, 1);
    try {
        d.d_radiance = (float*)hipMallocSafe(n * 3 * sizeof(float), "denoise.radiance");
        d.d_buf = (float4*)hipMallocSafe(2 * n * sizeof(float4), "denoise.buf");
        d.d_var_in = (float*)hipMallocSafe(n * sizeof(float), "denoise.variance_in");
        d.d_var_out = (float*)hipMallocSafe(n * sizeof(float), "denoise.variance_out");
        d.d_rgb8 = (unsigned char*)hipMallocSafe(n * 3, "denoise.rgb8");                   // last: set means complete
    } catch (...) {
        for (void* q : {(void*)d.d_radiance, (void*)d.d_buf, (void*)d.d_var_in, (void*)d.d_var_out}) if (q) (void)hipFree(q);
        d.d_radiance = nullptr; d.d_buf = nullptr; d.d_var_in = nullptr; d.d_var_out = nullptr;
        throw;
    }
}

// A filter on the context's stream, timed: the outputs allocated, the resolve gate waited for, enqueue(mark) between a begin and
// an end event, and its end waited for.  *ms: the device time - up to `mark`, which enqueue then records, where ms_after_mark is
// given, and the rest there.
template <class Enqueue>
static void runFilter(ApplicationState& g, Enqueue&& enqueue, double* ms, double* ms_after_mark = nullptr) {
    RenderState& r = g.render;
    PTMI_HIP(hipSetDevice(g.device_id));
    allocateDenoiseOutputs(r);
    needEvents(g, 3);
    const hipEvent_t begin = g.event_pool[0], end = g.event_pool[1], mark = g.event_pool[2];
    r.dn.denoised = false;
    if (r.resolve_gate) PTMI_HIP(hipStreamWaitEvent(r.stream, r.resolve_gate, 0));
    PTMI_HIP(hipEventRecord(begin, r.stream));
    enqueue(mark);
    PTMI_HIP(hipGetLastError());
    PTMI_HIP(hipEventRecord(end, r.stream));
    PTMI_HIP(hipStreamSynchronize(r.stream));
    *ms = elapsedMs(begin, ms_after_mark ? mark : end);
    if (ms_after_mark) *ms_after_mark = elapsedMs(mark, end);
    r.dn.denoised = true;
}

// the filter over radiance guided by fb into the denoiser's outputs (what ptmi_read_denoised returns)
static void denoiseRun(ApplicationState& g, const DenoiseArgs& a, int iterations, const float* sigma_c, const FeatureBuffers& fb,
                       const float* radiance) {
    RenderState::Denoise& d = g.render.dn;
    runFilter(g, [&](hipEvent_t) { launch_denoise(a, fb, radiance, iterations, sigma_c, d.d_buf, d.d_rgb8, d.d_radiance, g.render.stream); },
              &d.denoise_ms);
}

// what the filters and the temporal step ask of the context before they look at their parameters, in the caller's words
static void checkFilterable(const ApplicationState& g, const std::string& who, const char* why_one_rank, const char* done) {
    const RenderState& r = g.render;
    if (r.tile.n_ranks > 1) throw ArgError(who + ": the context is tiled over more than one rank (" + why_one_rank + ")");
    if (g.config.current_integrator == IntegratorType::Radiosity) throw ArgError(who + ": the Radiosity integrator's image is not " + done);
    if (!g.scene.d_nodes || !r.d_state.A || !r.dn.image_current)
        throw ArgError(who + ": no image rendered yet (none since the last change of scene, camera, resolution or config)");
}
static void checkDenoisable(const ApplicationState& g) { checkFilterable(g, "denoise", "the filter needs rows of other ranks", "denoised"); }

void denoise(ApplicationState& g, const DenoiseParams& p) {
    RenderState& r = g.render;
    RenderState::Denoise& d = r.dn;
    checkDenoisable(g);
    float sigma_c[10];
    const DenoiseArgs a = denoiseArgs(g, p, sigma_c);
    if (!d.features_valid || d.grid != p.feature_grid) renderFeatures(g, p.feature_grid);
    denoiseRun(g, a, p.iterations, sigma_c, d.fb, r.d_radiance);
}

void readDenoised(const ApplicationState& g, unsigned char* rgb8, float* radiance) {
    const RenderState& r = g.render;
    if (!r.dn.denoised) throw ArgError("readDenoised: nothing denoised yet (ptmi_denoise first)");
    readImagePair(g.device_id, r.n_local, r.dn.d_rgb8, r.dn.d_radiance, rgb8, radiance);
}

// ------------------------------------------------------------------------------------------------
// the variance-guided filter (include/ptmi.h: ptmi_denoise_variance)
// ------------------------------------------------------------------------------------------------
void denoiseVariance(ApplicationState& g, const VarianceParams& p) {
    RenderState& r = g.render;
    RenderState::Denoise& d = r.dn;
    checkDenoisable(g);
    checkVarianceParams(p);
    VarianceArgs a;
    filterArgs(g, p, a);
    a.sigma_l2 = p.sigma_luminance * p.sigma_luminance;
    a.epsilon = p.epsilon;
    a.radius = p.spatial_radius;
    a.two_spp = 2u * (unsigned int)g.config.spp;
    if (!d.features_valid || d.grid != p.feature_grid) renderFeatures(g, p.feature_grid);
    // the stopping test's moments describe the image only while it is a pass of the current accumulation
    const bool moments = p.source == 0 && d.image_pass && r.accum.pass > 0 && r.accum.allocated();
    d.variance_valid = false;
    runFilter(g, [&](hipEvent_t estimated) {
        launch_denoise_variance(a, d.fb, r.d_radiance, r.tile, moments ? &r.accum.ab : nullptr, r.accum.d_counts, p.iterations, d.d_buf,
                                d.d_var_in, d.d_var_out, d.d_rgb8, d.d_radiance, estimated, r.stream);
    }, &d.estimate_ms, &d.filter_ms);
    d.variance_valid = true;
}

void readVariance(const ApplicationState& g, float* variance_in, float* variance_out) {
    const RenderState& r = g.render;
    if (!r.dn.variance_valid) throw ArgError("readVariance: no current variance (ptmi_denoise_variance first)");
    PTMI_HIP(hipSetDevice(g.device_id));
    if (variance_in && r.n_local) PTMI_HIP(hipMemcpy(variance_in, r.dn.d_var_in, r.n_local * sizeof(float), hipMemcpyDeviceToHost));
    if (variance_out && r.n_local) PTMI_HIP(hipMemcpy(variance_out, r.dn.d_var_out, r.n_local * sizeof(float), hipMemcpyDeviceToHost));
}

void readPassMoments(const ApplicationState& g, float* mean, float* m2, uint32_t* passes) {
    const RenderState& r = g.render;
    if (!r.d_state.A || r.accum.pass == 0 || !r.accum.allocated()) throw ArgError("readPassMoments: the accumulation has no pass yet (ptmi_accum_pass first)");
    if (!r.n_local) return;
    PTMI_HIP(hipSetDevice(g.device_id));
    const size_t n = r.n_local;
    float* d_tmp = (float*)hipMallocSafe(3 * n * sizeof(float), "pass_moments");
    try {
        launch_pass_moments(r.tile, r.accum.ab, d_tmp, d_tmp + n, (unsigned int*)(d_tmp + 2 * n), r.stream);
        PTMI_HIP(hipGetLastError());
        PTMI_HIP(hipStreamSynchronize(r.stream));
        if (mean) PTMI_HIP(hipMemcpy(mean, d_tmp, n * sizeof(float), hipMemcpyDeviceToHost));
        if (m2) PTMI_HIP(hipMemcpy(m2, d_tmp + n, n * sizeof(float), hipMemcpyDeviceToHost));
        if (passes) PTMI_HIP(hipMemcpy(passes, d_tmp + 2 * n, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    } catch (...) { (void)hipFree(d_tmp); throw; }
    (void)hipFree(d_tmp);
}

// ------------------------------------------------------------------------------------------------
// temporal accumulation with reprojection (include/ptmi.h: ptmi_temporal_accumulate)
// ------------------------------------------------------------------------------------------------
void temporalReset(ApplicationState& g) { g.render.tp.valid = false; }

void checkTemporalParams(const TemporalParams& p) {
    if (p.max_history < 1 || p.max_history > 65536) throw ArgError("temporal: max_history must be in [1, 65536]");
    if (!(p.normal_min >= -1.0f && p.normal_min <= 1.0f)) throw ArgError("temporal: normal_min must be in [-1, 1]");
    if (!(p.sigma_position <= 0.0f || (p.sigma_position >= 1e-6f && p.sigma_position <= 1e12f)))
        throw ArgError("temporal: sigma_position must be <= 0 (automatic) or in [1e-6, 1e12]");
    if (p.feature_grid < 1 || p.feature_grid > 4) throw ArgError("temporal: feature_grid must be in [1, 4]");
    if (!(p.sigma_albedo >= 0.0f && p.sigma_albedo <= 1e6f)) throw ArgError("temporal: sigma_albedo must be in [0, 1e6]");
}

void temporalAccumulate(ApplicationState& g, const TemporalParams& p, TemporalStats* stats) {
    RenderState& r = g.render;
    RenderState::Temporal& t = r.tp;
    RenderState::Denoise& d = r.dn;
    checkFilterable(g, "temporal", "taps cross ranks", "accumulated");
    checkTemporalParams(p);
    TemporalArgs a;
    a.width = r.tile.width; a.height = r.tile.local_rows;
    const float sigma_x = p.sigma_position > 0.0f ? p.sigma_position : autoSigmaPosition(g, 0.01f, "temporal");     // 1 %
    a.sigma_x2 = sigma_x * sigma_x;
    a.sigma_a2 = p.sigma_albedo * p.sigma_albedo;
    a.normal_min = p.normal_min;
    a.max_history = (float)p.max_history;
    a.m = (float)g.config.spp;
    const unsigned int* counts = d.image_pass ? r.accum.d_counts : nullptr;     // a pass: every pixel's own count
    float cam[12];
    cameraFrame12(r.h_camera, g.config.orbit, cam);                             // the frame the next render would use
    double features_ms = 0.0;
    if (!d.features_valid || d.grid != p.feature_grid) { renderFeatures(g, p.feature_grid); features_ms = d.features_ms; }
    PTMI_HIP(hipSetDevice(g.device_id));
    const size_t n = std::max<size_t>(r.n_local, 1);
    if (!t.d_rgb8) {
        try {
            for (TemporalHistory& h : t.side) {
                h.color = (float4*)hipMallocSafe(n * sizeof(float4), "temporal.color");
                h.normal = (float4*)hipMallocSafe(n * sizeof(float4), "temporal.normal");
                h.position = (float4*)hipMallocSafe(n * sizeof(float4), "temporal.position");
                h.albedo = (float4*)hipMallocSafe(n * sizeof(float4), "temporal.albedo");
            }
            t.d_radiance = (float*)hipMallocSafe(n * 3 * sizeof(float), "temporal.radiance");
            t.d_stats = (unsigned long long*)hipMallocSafe(3 * sizeof(unsigned long long), "temporal.stats");
            t.d_rgb8 = (unsigned char*)hipMallocSafe(n * 3, "temporal.rgb8");
        } catch (...) { r.freeTemporal(); throw; }
    }
    if (g.temporal_moments && !t.moments[0]) {
        try {
            for (float4*& q : t.moments) q = (float4*)hipMallocSafe(n * sizeof(float4), "temporal.moments");
        } catch (...) { r.freeTemporal(); throw; }
    }
    a.history = t.valid ? 1 : 0;
    a.still = t.valid && std::memcmp(cam, t.cam, sizeof cam) == 0 && t.width == a.width && t.height == a.height ? 1 : 0;
    std::memcpy(a.cam, t.cam, sizeof a.cam);
    std::memcpy(a.origin, cam, sizeof a.origin);
    needEvents(g, 2);
    const int next = t.cur ^ 1;
    unsigned long long h_stats[3] = {0, 0, 0};
    t.stepped = false;
    PTMI_HIP(hipMemsetAsync(t.d_stats, 0, sizeof h_stats, r.stream));
    if (r.resolve_gate) PTMI_HIP(hipStreamWaitEvent(r.stream, r.resolve_gate, 0));
    PTMI_HIP(hipEventRecord(g.event_pool[0], r.stream));
    launch_temporal(a, d.fb, r.d_radiance, counts, t.side[t.cur], t.side[next], t.d_rgb8, t.d_radiance, t.d_stats, r.stream,
                    g.temporal_moments ? t.moments[t.cur] : nullptr, g.temporal_moments ? t.moments[next] : nullptr);
    PTMI_HIP(hipGetLastError());
    PTMI_HIP(hipEventRecord(g.event_pool[1], r.stream));
    PTMI_HIP(hipMemcpyAsync(h_stats, t.d_stats, sizeof h_stats, hipMemcpyDeviceToHost, r.stream));
    PTMI_HIP(hipStreamSynchronize(r.stream));
    t.cur = next;
    t.valid = true;
    std::memcpy(t.cam, cam, sizeof cam);
    t.width = a.width; t.height = a.height;
    t.grid = p.feature_grid;
    t.stepped = true;
    if (stats) {
        stats->accepted = h_stats[0]; stats->rejected = h_stats[1]; stats->missed = h_stats[2];
        stats->seconds = elapsedMs(g.event_pool[0], g.event_pool[1]) * 1e-3;
        stats->features_ms = features_ms;
    }
}

void readTemporal(const ApplicationState& g, unsigned char* rgb8, float* radiance) {
    const RenderState& r = g.render;
    if (!r.tp.stepped) throw ArgError("readTemporal: no temporal step yet (ptmi_temporal_accumulate first)");
    readImagePair(g.device_id, r.n_local, r.tp.d_rgb8, r.tp.d_radiance, rgb8, radiance);
}

void readHistoryCounts(const ApplicationState& g, float* counts) {
    const RenderState& r = g.render;
    if (!r.d_state.A) throw ArgError("readHistoryCounts: buffers not allocated");
    if (!r.tp.valid) { std::fill(counts, counts + r.n_local, 0.0f); return; }
    PTMI_HIP(hipSetDevice(g.device_id));
    std::vector<float4> h(r.n_local);
    if (r.n_local) PTMI_HIP(hipMemcpy(h.data(), r.tp.side[r.tp.cur].color, r.n_local * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < r.n_local; i++) counts[i] = h[i].w;
}

void denoiseTemporal(ApplicationState& g, const DenoiseParams& p) {
    RenderState& r = g.render;
    const RenderState::Temporal& t = r.tp;
    if (!t.valid) throw ArgError("denoise_temporal: the history is empty (ptmi_temporal_accumulate first)");
    float sigma_c[10];
    const DenoiseArgs a = denoiseArgs(g, p, sigma_c);
    if (p.feature_grid != t.grid) throw ArgError("denoise_temporal: feature_grid differs from the history's");
    FeatureBuffers fb;
    fb.albedo = t.side[t.cur].albedo; fb.normal = t.side[t.cur].normal; fb.position = t.side[t.cur].position;
    denoiseRun(g, a, p.iterations, sigma_c, fb, t.d_radiance);        // the last step's radiance is the history's colour
}

// ------------------------------------------------------------------------------------------------
// the history's luminance statistics (include/ptmi.h: ptmi_set_temporal_moments, ptmi_denoise_temporal_variance)
// ------------------------------------------------------------------------------------------------
void setTemporalMoments(ApplicationState& g, int on) {
    if (on != 0 && on != 1) throw ArgError("temporal_moments: on must be 0 or 1");
    if (on == g.temporal_moments) return;
    g.temporal_moments = on;
    temporalReset(g);                                  // a history without statistics cannot go on with them, nor the reverse
}

// the statistics of the history's current side, or the reason there are none
static float4* currentMoments(const ApplicationState& g, const char* who) {
    const RenderState::Temporal& t = g.render.tp;
    if (!g.temporal_moments) throw ArgError(std::string(who) + ": the temporal moments are off (ptmi_set_temporal_moments first)");
    if (!t.valid || !t.moments[t.cur]) throw ArgError(std::string(who) + ": the history is empty (ptmi_temporal_accumulate first)");
    return t.moments[t.cur];
}

void readTemporalMoments(const ApplicationState& g, float* mean, float* variance, float* frames) {
    const float4* d_mom = currentMoments(g, "read_temporal_moments");
    const size_t n = g.render.n_local;
    PTMI_HIP(hipSetDevice(g.device_id));
    std::vector<float4> h(n);
    if (n) PTMI_HIP(hipMemcpy(h.data(), d_mom, n * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) {
        if (mean) mean[i] = h[i].x;
        if (variance) variance[i] = h[i].y;
        if (frames) frames[i] = h[i].z;
    }
}

void debugSetTemporalMoments(ApplicationState& g, const float* mean, const float* variance, const float* frames) {
    float4* d_mom = currentMoments(g, "debug_set_temporal_moments");
    const size_t n = g.render.n_local;
    PTMI_HIP(hipSetDevice(g.device_id));
    std::vector<float4> h(n);
    for (size_t i = 0; i < n; i++) h[i] = make_float4(mean[i], variance[i], frames[i], 0.0f);
    if (n) PTMI_HIP(hipMemcpy(d_mom, h.data(), n * sizeof(float4), hipMemcpyHostToDevice));   // (every step ends with a synchronise)
}

void denoiseTemporalVariance(ApplicationState& g, const VarianceParams& p) {
    RenderState& r = g.render;
    RenderState::Denoise& d = r.dn;
    const RenderState::Temporal& t = r.tp;
    TemporalVariance tv;
    tv.moments = currentMoments(g, "denoise_temporal_variance");
    checkVarianceParams(p);
    if (p.feature_grid != t.grid) throw ArgError("denoise_temporal_variance: feature_grid differs from the history's");
    VarianceArgs a;
    filterArgs(g, p, a);
    a.sigma_l2 = p.sigma_luminance * p.sigma_luminance;
    a.epsilon = p.epsilon;
    a.radius = p.spatial_radius;
    a.two_spp = 1u;                                    // the spatial estimate skips the pixels whose mask is 1
    PTMI_HIP(hipSetDevice(g.device_id));
    if (!d.d_owned) d.d_owned = (unsigned int*)hipMallocSafe(std::max<size_t>(r.n_local, 1) * sizeof(unsigned int), "denoise.owned");
    tv.mask = d.d_owned;
    tv.source = p.source;
    FeatureBuffers fb;
    fb.albedo = t.side[t.cur].albedo; fb.normal = t.side[t.cur].normal; fb.position = t.side[t.cur].position;
    d.variance_valid = false;
    runFilter(g, [&](hipEvent_t estimated) {           // the last step's radiance is the history's colour
        launch_denoise_variance(a, fb, t.d_radiance, r.tile, nullptr, nullptr, p.iterations, d.d_buf, d.d_var_in, d.d_var_out, d.d_rgb8,
                                d.d_radiance, estimated, r.stream, &tv);
    }, &d.estimate_ms, &d.filter_ms);
    d.variance_valid = true;
}

}  // namespace ptmi
