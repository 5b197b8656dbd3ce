// ref_integrator_harness.cpp — thin C-ABI driver around the REFERENCE's own shading half: rendering/integrator.h
// (sampleCosineHemisphere, misPowerHeuristic, sampleMIS, integrator, render_init, render, render_radiosity) and
// rendering/grid.h (Grid::loadPrecomputed / initFromRadiosity / sample / computePDF), over the reference's Scene, BVHBuilder
// and Sensor.
//
// TEST INFRASTRUCTURE ONLY.  Built by oracle/Makefile into oracle/_ref/libptmi_ref_integrator.so where the reference tree
// AND NVIDIA's own <cuda_runtime.h> exist (as libptmi_ref_obj.so).  The reference headers are included BY PATH from where
// they lie, unmodified; nothing of them is copied.  What the build supplies around them:
//   - NVIDIA's genuine <cuda_runtime.h> (grid.h includes it; found by oracle/Makefile);
//   - oracle/shim/curand_kernel.h: a project-written stand-in for the closed cuRAND API (curandState, curand_init,
//     curand_uniform).  Stream mode draws through the oracle's generator, whose seed scramble and float mapping stay
//     unpinned; scripted mode feeds caller-supplied raw words.  See that file;
//   - libm: cosf, sinf, sincosf, powf, acosf and atan2f are routed to include/ptmi_math.h by macros placed after <cmath>.
//     That is the project's numerics contract (tests/test_numerics_contract.py pins it separately); the reference's own
//     libm on its target is CUDA's, which is not glibc's either.  sqrtf, fminf, fmaxf and division stay IEEE;
//   - host definitions of the kernel built-ins threadIdx / blockIdx / blockDim (thread-local, set per pixel), and of clock64
//     and atomicAdd, which only the profiled variants (ENABLE_KERNEL_PROFILING, render_config.h) call.
// The only restated code is ref_radiance(): render()'s six-line sample loop around integrator() with a free max_depth
// (render() fixes 5) and the radiance kept before the tone-map.
//
// SceneState::precomputeCDFs itself lives in application_state.h (GL) and is not reachable here, but its arithmetic for the
// upper hemisphere is Grid::initFromRadiosity / initFromFormFactor + buildCDFs (grid.h:51-134), which leaves its result in
// public arrays: ref_grid_record() runs it, and tests/test_guided_record_sets_host.py requires the oracle's records
// (po_scene_get_cdfs, po_cdf_records) to be those, bit for bit, on constructed edge grids.  The records' layout is pinned by
// tests/test_oracle_vs_ref.py.
#include <cuda_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <sstream>
#include <vector>

#include "../include/ptmi_math.h"

// ---- libm of the numerics contract (see the header comment) ----
static inline float ptmi_ref_cosf(float x) { float s, c; ptmi_sincosf(x, &s, &c); return c; }
static inline float ptmi_ref_sinf(float x) { float s, c; ptmi_sincosf(x, &s, &c); return s; }
#define cosf ptmi_ref_cosf
#define sinf ptmi_ref_sinf
#define sincosf ptmi_sincosf
#define powf ptmi_powf
#define acosf ptmi_acosf
#define atan2f ptmi_atan2f

using std::max;
using std::min;

// ---- kernel built-ins on the host ----
static thread_local uint3 ptmi_ref_threadIdx, ptmi_ref_blockIdx;
static thread_local dim3 ptmi_ref_blockDim;
#define threadIdx ptmi_ref_threadIdx
#define blockIdx ptmi_ref_blockIdx
#define blockDim ptmi_ref_blockDim
static inline long long clock64() { return 0; }
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) {
    return __atomic_fetch_add(p, v, __ATOMIC_RELAXED);
}

#include <curand_kernel.h>   // oracle/shim/

#include "core/vector.h"
#include "core/ray.h"
#include "rendering/primitive.h"
#include "rendering/bvh.h"
#include "rendering/scene.h"
#include "rendering/sensor.h"
#include "rendering/integrator.h"

#ifdef _OPENMP
#include <omp.h>
#endif

static_assert(sizeof(PrecomputedCDF) == 530 * sizeof(float), "PrecomputedCDF is 530 words");

namespace {
struct CoutSilencer {   // BVHBuilder logs every step to std::cout (bvh.h:84-99)
    std::streambuf* old; std::ostringstream sink;
    CoutSilencer() : old(std::cout.rdbuf(sink.rdbuf())) {}
    ~CoutSilencer() { std::cout.rdbuf(old); }
};
struct RefScene {
    Primitive* prims = nullptr; int n = 0;
    std::vector<BVHNode> nodes; std::vector<int> indices;
    std::vector<PrecomputedCDF> cdfs;
    Scene scene;
};
Vector3f v3(const float* p) { return Vector3f(p[0], p[1], p[2]); }
void put3(float* out, const Vector3f& v) { for (int k = 0; k < 3; k++) out[k] = v[k]; }

curandState scripted(const uint32_t* words, int n) {
    curandState s;
    std::memset(&s, 0, sizeof s);
    s.script = words; s.n_script = n;
    return s;
}
int consumed(const curandState& s) { return s.overrun ? -1 : s.used; }   // -1: the script ran out

Grid grid_over(const PrecomputedCDF* rec) { Grid g; g.loadPrecomputed(rec); return g; }

// the Sensor as the reference's host flow leaves it (ref_harness.cpp: ref_camera)
Sensor make_sensor(const float* cam /* lookfrom3 lookat3 vup3 vfov yaw pitch orbit */, int width, int height) {
    Sensor s(v3(cam), v3(cam + 3), v3(cam + 6), cam[9], 1.0f);
    s.image_width = width; s.image_height = height;
    s.aspect = (float)width / (float)height;
    s.updateCamera();
    if (cam[12] != 0.0f) { s.yaw = cam[10]; s.pitch = cam[11]; s.updateCameraOrbit(); }
    return s;
}
void set_thread(int x, int y) {   // one 16 x 16 block per tile, as the reference launches (BLOCK_X, BLOCK_Y)
    ptmi_ref_blockDim = dim3(BLOCK_X, BLOCK_Y, 1);
    ptmi_ref_blockIdx.x = x / BLOCK_X; ptmi_ref_blockIdx.y = y / BLOCK_Y; ptmi_ref_blockIdx.z = 0;
    ptmi_ref_threadIdx.x = x % BLOCK_X; ptmi_ref_threadIdx.y = y % BLOCK_Y; ptmi_ref_threadIdx.z = 0;
}
int threads(int n) {
#ifdef _OPENMP
    return n > 0 ? n : omp_get_num_procs();
#else
    return 1;
#endif
}
// render_init over the whole frame, one "thread" per pixel
std::vector<curandState> init_states(int width, int height, int n_threads) {
    std::vector<curandState> st((size_t)width * height);
#pragma omp parallel for schedule(static) num_threads(threads(n_threads))
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) { set_thread(x, y); render_init(width, height, st.data()); }
    return st;
}
}  // namespace

extern "C" {

// ---- per call, scripted raw words.  Each returns the number of words drawn (-1: more than supplied). ----
int ref_sample_cosine_hemisphere(const float* n, const uint32_t* words, int n_words, float* out_dir) {
    curandState s = scripted(words, n_words);
    put3(out_dir, sampleCosineHemisphere(v3(n), &s));
    return consumed(s);
}
float ref_mis_power_heuristic(float a, float b) { return misPowerHeuristic(a, b); }

// rec: one PrecomputedCDF record (530 words).  out_valid: Grid::isValid() after loadPrecomputed.
int ref_grid_sample(const float* rec, const float* n, const uint32_t* words, int n_words, float* out_dir, float* out_pdf,
                    int* out_valid) {
    Grid g = grid_over(reinterpret_cast<const PrecomputedCDF*>(rec));
    *out_valid = g.isValid() ? 1 : 0;
    curandState s = scripted(words, n_words);
    float pdf = 0.0f;
    put3(out_dir, g.sample(v3(n), &s, pdf));
    *out_pdf = pdf;
    return consumed(s);
}
float ref_grid_pdf(const float* rec, const float* dir, const float* n) {
    return grid_over(reinterpret_cast<const PrecomputedCDF*>(rec)).computePDF(v3(dir), v3(n));
}
int ref_sample_mis(const float* rec, const float* n, float bsdf_prob, const uint32_t* words, int n_words, float* out_dir,
                   float* out_weight, int* out_used_bsdf) {
    Grid g = grid_over(reinterpret_cast<const PrecomputedCDF*>(rec));
    curandState s = scripted(words, n_words);
    float w = 0.0f; bool used = false;
    put3(out_dir, sampleMIS(g, v3(n), &s, w, bsdf_prob, used));
    *out_weight = w; *out_used_bsdf = used ? 1 : 0;
    return consumed(s);
}

// ---- records ----
// Grid::initFromRadiosity (kind 1: 256 rgb triples) or Grid::initFromFormFactor (kind 2: 256 ready pdf values) + buildCDFs
// (grid.h:51-134) on one grid, copied out in the PrecomputedCDF layout.  buildCDFs fills the upper hemisphere only: the
// words of row_cdfs[128..255] are returned as zero (application_state.h:560-565 fills them; the tests assert that formula).
int ref_grid_record(int kind, const float* src, float* out_rec) {
    if (kind != 1 && kind != 2) return -1;
    Grid g;
    if (kind == 1) {
        std::vector<Vector3f> rgb(GRID_SIZE);
        for (int c = 0; c < GRID_SIZE; c++) rgb[c] = v3(src + 3 * c);
        g.initFromRadiosity(rgb.data());
    } else g.initFromFormFactor(src);
    PrecomputedCDF rec;
    std::memset(&rec, 0, sizeof rec);
    std::memcpy(rec.pdf, g.pdf, sizeof g.pdf);
    std::memcpy(rec.row_sums, g.row_sums, sizeof g.row_sums);
    std::memcpy(rec.marginal_cdf, g.marginal_cdf, sizeof g.marginal_cdf);
    std::memcpy(rec.row_cdfs, g.row_cdfs, sizeof(float) * GRID_HALF_RES * GRID_RES);
    rec.total_weight = g.total_weight;
    rec.is_valid = g.isValid() ? 1 : 0;
    std::memcpy(out_rec, &rec, sizeof rec);
    return 0;
}

// ---- scenes ----
// Arrays as ref_harness.cpp's ref_scene_create; radiosity: n*3 (NULL = zero), cdfs: n*530 words (the oracle's records;
// NULL = Scene::precomputed_cdfs stays null), rad_grids: n*256*3 (NULL = zero; only read when cdfs is NULL - the
// initFromRadiosity fallback of initGridFromPrimitive).
void* ref_int_scene_create(int n, const int* type, const float* verts, const float* normal, const float* bsdf,
                           const float* Le, const float* radiosity, const float* cdfs, const float* rad_grids,
                           float mis_fraction) {
    CoutSilencer quiet;
    RefScene* rs = new RefScene;
    rs->n = n; rs->prims = new Primitive[n];
    for (int i = 0; i < n; i++) {
        const float* v = verts + (size_t)i * 12;
        if (type[i] == PRIM_TRIANGLE) {
            Triangle t(v3(v), v3(v + 3), v3(v + 6), v3(bsdf + 3 * i), v3(normal + 3 * i));   // as file_manager.h:212
            t.Le = v3(Le + 3 * i);
            rs->prims[i] = Primitive(t);
        } else {
            Quad q(v3(v), v3(v + 3), v3(v + 6), v3(v + 9), v3(bsdf + 3 * i));               // as file_manager.h:233
            q.normal = v3(normal + 3 * i);
            q.Le = v3(Le + 3 * i);
            rs->prims[i] = Primitive(q);
        }
        if (radiosity) rs->prims[i].setRadiosity(v3(radiosity + 3 * i));
        if (rad_grids) {
            Vector3f* g = rs->prims[i].getRadiosityGrid();
            for (int c = 0; c < GRID_SIZE; c++) g[c] = v3(rad_grids + ((size_t)i * GRID_SIZE + c) * 3);
        }
    }
    BVHBuilder builder(rs->prims, n);
    rs->nodes = builder.nodes; rs->indices = builder.primitive_indices;
    rs->scene = Scene(rs->prims, n, rs->nodes.data(), rs->indices.data());
    if (cdfs) {
        rs->cdfs.resize(n);
        std::memcpy(rs->cdfs.data(), cdfs, sizeof(PrecomputedCDF) * (size_t)n);
        rs->scene.precomputed_cdfs = rs->cdfs.data();
    }
    rs->scene.mis_bsdf_fraction = mis_fraction;
    return rs;
}
void ref_int_scene_free(void* h) { RefScene* rs = (RefScene*)h; if (!rs) return; delete[] rs->prims; delete rs; }

// ---- whole frames, stream mode: render_init + render (depth 5, rgb8) and render_radiosity, kernels run once per pixel ----
// cam: lookfrom[3] lookat[3] vup[3] vfov yaw pitch orbit (13 floats).  rgb8: width*height*3, row 0 = bottom.
void ref_render(void* h, const float* cam, int width, int height, int spp, int mode, int n_threads, unsigned char* rgb8) {
    RefScene* rs = (RefScene*)h;
    Sensor sensor = make_sensor(cam, width, height);
    std::vector<curandState> st = init_states(width, height, n_threads);
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads(n_threads))
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) { set_thread(x, y); render(rgb8, &sensor, &rs->scene, st.data(), spp, (SamplingMode)mode); }
}
void ref_render_radiosity(void* h, const float* cam, int width, int height, int spp, int n_threads, unsigned char* rgb8) {
    RefScene* rs = (RefScene*)h;
    Sensor sensor = make_sensor(cam, width, height);
    std::vector<curandState> st = init_states(width, height, n_threads);
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads(n_threads))
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) { set_thread(x, y); render_radiosity(rgb8, &sensor, &rs->scene, st.data(), spp); }
}

// Per-pixel radiance (color / spp, before the tone-map) at any depth.  RESTATED: the sample loop of render()
// (integrator.h, the kernel's first lines through `color /= float(spp)`) around the reference's own integrator().
void ref_radiance(void* h, const float* cam, int width, int height, int spp, int max_depth, int mode, int n_threads,
                  float* radiance) {
    RefScene* rs = (RefScene*)h;
    Sensor sensor = make_sensor(cam, width, height);
    std::vector<curandState> st = init_states(width, height, n_threads);
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads(n_threads))
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            curandState* local_rng = &st[(size_t)y * width + x];
            Vector3f color(0.0f, 0.0f, 0.0f);
            for (int s = 0; s < spp; s++) {
                float u = (x + curand_uniform(local_rng)) / float(sensor.image_width);
                float v = (y + curand_uniform(local_rng)) / float(sensor.image_height);
                Ray ray = sensor.get_ray(u, v);
                Vector3f sample_color(0.0f, 0.0f, 0.0f);
                integrator(&rs->scene, ray, sample_color, max_depth, local_rng, (SamplingMode)mode);
                color += sample_color;
            }
            color /= float(spp);
            put3(radiance + ((size_t)y * width + x) * 3, color);
        }
}

}  // extern "C"
