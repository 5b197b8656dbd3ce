// ref_solver_harness.cpp — thin C-ABI driver around the REFERENCE's own radiosity pre-pass: rendering/form_factors.h
// (direction_to_grid_indices_local, visibility_test_anyhit, formfactor_rand_init, calculate_form_factors_mc_kernel,
// calculate_form_factors_kernel, update_radiosity_grid, radiosity_iteration_kernel, subdivide_primitives) and
// rendering/grid_filter.h (every kernel and the three host wrappers filter_radiosity_grids,
// filter_radiosity_grids_gaussian, filter_pdfs_for_primitives), over the reference's Primitive and BVHBuilder.
//
// TEST INFRASTRUCTURE ONLY.  Built by oracle/Makefile into oracle/_ref/libptmi_ref_solver.so on the condition of
// libptmi_ref_integrator.so (the reference tree and NVIDIA's own <cuda_runtime.h> exist).  The reference headers are included
// BY PATH from where they lie, unmodified, with ONE exception: grid_filter.h's host wrappers launch kernels with
// `name<<<g, b>>>(`, which no host compiler parses.  The recipe runs oracle/delaunch.py, which rewrites exactly those launch
// statements to `PTMI_REF_LAUNCH(name, g, b)(` into a copy in a temporary directory outside the repository, puts that
// directory first on the include path and removes it when the recipe ends.  What the build supplies around the headers:
//   - NVIDIA's genuine <cuda_runtime.h> and <device_launch_parameters.h>, included before the macros below;
//   - oracle/shim/curand_kernel.h (stream mode: the oracle's generator; scripted mode: caller-supplied raw words);
//   - libm: cosf, sinf, acosf, atan2f, expf and powf are routed to include/ptmi_math.h (the project's numerics contract, as in
//     ref_integrator_harness.cpp); sqrtf, fminf, fmaxf, fabsf and division stay IEEE;
//   - host definitions of threadIdx / blockIdx / blockDim / gridDim and of atomicAdd (float, int, unsigned);
//   - PTMI_REF_LAUNCH(k, g, b): a callable that loops over the g x b threads (x fastest), sets the index variables and
//     calls k once per thread, so that the reference's own wrappers run as written;
//   - cudaMalloc / cudaFree / cudaMemcpy / cudaDeviceSynchronize renamed by macro to host stand-ins (malloc, free, memmove,
//     nothing);
//   - OptixLogger set to NONE and std::cout redirected while reference code runs.
//
// The only restated code is the launch sequence of RadiosityState::runSolver (application_state.h:688-777: that header
// needs GL): ref_sol_solve() below.  convertQuadsToTriangles and precomputeCDFs stay behind GL too and remain restated in
// the oracle (the CDF arithmetic is pinned through Grid::initFromRadiosity, see ref_integrator_harness.cpp).
//
// THE HARNESS'S RULES, NOT THE REFERENCE'S - where the reference is not a function of its inputs, the harness fixes what
// oracle/ptmi_oracle.c documents:
//   - radiosity_iteration_kernel races on unshot_rad.  Every thread of one launch reads the state as it was before the
//     launch: thread i runs on the snapshot and only primitive i of its result is kept.
//   - The MC kernel's float atomics into radiosity_grid have no order in the reference.  Here the threads of one receiver
//     run in ascending j (PTMI_REF_LAUNCH's x-fastest loop).  The count grid sums integers and is exact in any order.
//   - The 5-argument Triangle constructor and the reference's loader leave history_index / history_count undefined;
//     the harness zeroes them, so that store_radiosity_history_kernel writes inside its array.  Nothing read here depends
//     on the history.
#include <cuda_runtime.h>
#include <device_launch_parameters.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
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
#define expf ptmi_expf

using std::max;
using std::min;

// ---- kernel built-ins on the host ----
static uint3 ptmi_ref_threadIdx, ptmi_ref_blockIdx;
static dim3 ptmi_ref_blockDim, ptmi_ref_gridDim;
#define threadIdx ptmi_ref_threadIdx
#define blockIdx ptmi_ref_blockIdx
#define blockDim ptmi_ref_blockDim
#define gridDim ptmi_ref_gridDim
static inline float atomicAdd(float* p, float v) { float old = *p; *p = old + v; return old; }
static inline int atomicAdd(int* p, int v) { int old = *p; *p = old + v; return old; }
static inline unsigned atomicAdd(unsigned* p, unsigned v) { unsigned old = *p; *p = old + v; return old; }

template <class K>
struct PtmiRefLaunch {
    K k; dim3 g, b;
    template <class... A>
    void operator()(A... a) const {
        ptmi_ref_gridDim = g; ptmi_ref_blockDim = b;
        for (unsigned bz = 0; bz < g.z; bz++) for (unsigned by = 0; by < g.y; by++) for (unsigned bx = 0; bx < g.x; bx++)
            for (unsigned tz = 0; tz < b.z; tz++) for (unsigned ty = 0; ty < b.y; ty++) for (unsigned tx = 0; tx < b.x; tx++) {
                ptmi_ref_blockIdx.x = bx; ptmi_ref_blockIdx.y = by; ptmi_ref_blockIdx.z = bz;
                ptmi_ref_threadIdx.x = tx; ptmi_ref_threadIdx.y = ty; ptmi_ref_threadIdx.z = tz;
                k(a...);
            }
    }
};
template <class K>
static inline PtmiRefLaunch<K> ptmi_ref_make_launch(K k, dim3 g, dim3 b) { return PtmiRefLaunch<K>{k, g, b}; }
#define PTMI_REF_LAUNCH(k, g, b) ptmi_ref_make_launch(k, dim3(g), dim3(b))

// ---- the CUDA runtime calls of grid_filter.h's wrappers, on the host ----
template <class T>
static inline int ptmi_ref_cudaMalloc(T** p, size_t bytes) { *p = (T*)std::malloc(bytes ? bytes : 1); return 0; }
static inline int ptmi_ref_cudaFree(void* p) { std::free(p); return 0; }
static inline int ptmi_ref_cudaMemcpy(void* dst, const void* src, size_t bytes, int) { std::memmove(dst, src, bytes); return 0; }
static inline int ptmi_ref_cudaDeviceSynchronize() { return 0; }
#define cudaMalloc ptmi_ref_cudaMalloc
#define cudaFree ptmi_ref_cudaFree
#define cudaMemcpy ptmi_ref_cudaMemcpy
#define cudaDeviceSynchronize ptmi_ref_cudaDeviceSynchronize

#include <curand_kernel.h>   // oracle/shim/

#include "core/vector.h"
#include "core/ray.h"
#include "rendering/primitive.h"
#include "rendering/bvh.h"
#include "rendering/form_factors.h"   // includes rendering/grid_filter.h: the de-launched copy, first on the include path

#ifndef ENABLE_GRID_FILTERING
#error "rendering/grid_filter.h did not come in through form_factors.h"
#endif

namespace {
struct Quiet {   // BVHBuilder and subdivide_primitives write to std::cout; the logger is a singleton with a level
    std::streambuf* old; std::ostringstream sink;
    Quiet() : old(std::cout.rdbuf(sink.rdbuf())) { OptixLogger::getInstance().setLogLevel(OptixLogLevel::NONE); }
    ~Quiet() { std::cout.rdbuf(old); }
};
struct RefScene {
    Primitive* prims = nullptr; int n = 0;
    std::vector<BVHNode> nodes; std::vector<int> indices;
};
Vector3f v3(const float* p) { return Vector3f(p[0], p[1], p[2]); }
void put3(float* out, const Vector3f& v) { for (int k = 0; k < 3; k++) out[k] = v[k]; }

Primitive make_prim(int type, const float* v, const float* normal, const float* bsdf, const float* Le) {
    if (type == PRIM_TRIANGLE) {
        Triangle t(v3(v), v3(v + 3), v3(v + 6), v3(bsdf), v3(normal));   // as file_manager.h:212
        t.Le = v3(Le); t.history_index = 0; t.history_count = 0;
        for (int c = 0; c < GRID_SIZE; c++) { t.grid[c] = 0.0f; t.radiosity_grid[c] = Vector3f(0.0f, 0.0f, 0.0f); }
        return Primitive(t);
    }
    Quad q(v3(v), v3(v + 3), v3(v + 6), v3(v + 9), v3(bsdf));            // as file_manager.h:233
    q.normal = v3(normal); q.Le = v3(Le); q.history_index = 0; q.history_count = 0;
    return Primitive(q);
}
void set_thread_1d(int i, int block) {
    ptmi_ref_gridDim = dim3(i / block + 1); ptmi_ref_blockDim = dim3(block);
    ptmi_ref_blockIdx.x = i / block; ptmi_ref_blockIdx.y = ptmi_ref_blockIdx.z = 0;
    ptmi_ref_threadIdx.x = i % block; ptmi_ref_threadIdx.y = ptmi_ref_threadIdx.z = 0;
}
// thread (x, y) of a launch with 8 x 8 blocks, as runSolver launches both form-factor kernels
void set_thread_2d(int x, int y) {
    ptmi_ref_gridDim = dim3(x / 8 + 1, y / 8 + 1); ptmi_ref_blockDim = dim3(8, 8);
    ptmi_ref_blockIdx.x = x / 8; ptmi_ref_blockIdx.y = y / 8; ptmi_ref_blockIdx.z = 0;
    ptmi_ref_threadIdx.x = x % 8; ptmi_ref_threadIdx.y = y % 8; ptmi_ref_threadIdx.z = 0;
}
// the working copy runSolver uploads: radiosity = unshot = Le (application_state.h:697-701), grids zeroed by
// initialize_directional_grids (:709-712)
std::vector<Primitive> working_copy(const RefScene* rs) {
    std::vector<Primitive> w(rs->prims, rs->prims + rs->n);
    for (int i = 0; i < rs->n; ++i) {
        Vector3f Le = w[i].getLe();
        w[i].setRadiosity(Le);
        w[i].setUnshotRad(Le);
    }
    int block_size = 256;
    int grid_size = (rs->n + block_size - 1) / block_size;
    PTMI_REF_LAUNCH(initialize_directional_grids, grid_size, block_size)(w.data(), rs->n);
    return w;
}
void get_grids(Primitive& p, float* out_grid, float* out_rad_grid) {
    if (out_grid) std::memcpy(out_grid, p.getGrid(), sizeof(float) * GRID_SIZE);
    if (out_rad_grid) for (int c = 0; c < GRID_SIZE; c++) put3(out_rad_grid + 3 * c, p.getRadiosityGrid()[c]);
}
// radiosity_iteration_kernel under the harness's snapshot rule (header comment)
void iterate_snapshot(Primitive* prims, float* ff, int n) {
    std::vector<Primitive> result(n);
    for (int i = 0; i < n; i++) {
        Primitive before = prims[i];
        set_thread_1d(i, 256);
        radiosity_iteration_kernel(prims, ff, n);
        result[i] = prims[i];
        prims[i] = before;
    }
    for (int i = 0; i < n; i++) prims[i] = result[i];
}
std::vector<Primitive> with_grids(int n, const float* rgb, const float* counts) {
    std::vector<Primitive> w;
    const float tri[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, nrm[3] = {0, 0, 1}, half[3] = {0.5f, 0.5f, 0.5f}, zero[3] = {0, 0, 0};
    const float quad[12] = {0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0};
    for (int i = 0; i < n; i++) {   // every second primitive a quad: both arms of the type switches (grid_filter.h:363-367)
        w.push_back(make_prim(i % 2, i % 2 ? quad : tri, nrm, half, zero));
        for (int c = 0; c < GRID_SIZE; c++) {
            w[i].getRadiosityGrid()[c] = v3(rgb + ((size_t)i * GRID_SIZE + c) * 3);
            w[i].getGrid()[c] = counts ? counts[(size_t)i * GRID_SIZE + c] : 0.0f;
        }
    }
    return w;
}
}  // namespace

extern "C" {

// ---- scenes: arrays as ref_harness.cpp's ref_scene_create ----
void* ref_sol_scene_create(int n, const int* type, const float* verts, const float* normal, const float* bsdf, const float* Le) {
    Quiet quiet;
    RefScene* rs = new RefScene;
    rs->n = n; rs->prims = new Primitive[n];
    for (int i = 0; i < n; i++) rs->prims[i] = make_prim(type[i], verts + (size_t)i * 12, normal + 3 * i, bsdf + 3 * i, Le + 3 * i);
    BVHBuilder builder(rs->prims, n);
    rs->nodes = builder.nodes; rs->indices = builder.primitive_indices;
    return rs;
}
void ref_sol_scene_free(void* h) { RefScene* rs = (RefScene*)h; if (!rs) return; delete[] rs->prims; delete rs; }
int ref_sol_scene_num_prims(void* h) { return ((RefScene*)h)->n; }
void ref_sol_scene_get_prims(void* h, int* type, float* verts, float* normal, float* bsdf, float* Le) {
    RefScene* rs = (RefScene*)h;
    for (int i = 0; i < rs->n; i++) {
        const Primitive& p = rs->prims[i];
        float* v = verts + (size_t)i * 12;
        type[i] = (int)p.type;
        for (int k = 0; k < 12; k++) v[k] = 0.0f;
        if (p.type == PRIM_TRIANGLE) { put3(v, p.tri.v0); put3(v + 3, p.tri.v1); put3(v + 6, p.tri.v2); }
        else { put3(v, p.quad.v00); put3(v + 3, p.quad.v10); put3(v + 6, p.quad.v11); put3(v + 9, p.quad.v01); }
        put3(normal + 3 * i, p.getNormal()); put3(bsdf + 3 * i, p.getBSDF()); put3(Le + 3 * i, p.getLe());
    }
}

// ---- per call ----
// direction_to_grid_indices_local (form_factors.h:107-128): grid_theta * GRID_RESOLUTION + grid_phi, as every caller forms it
int ref_sol_grid_index(const float* dir, const float* normal) {
    int grid_theta = -1, grid_phi = -1;
    direction_to_grid_indices_local(v3(dir), v3(normal), grid_theta, grid_phi);
    return grid_theta * GRID_RESOLUTION + grid_phi;
}
// visibility_test_anyhit (:144-209) on n rays built by Ray's constructor, as both kernels build theirs; out[k] = blocked.
// use_bvh == 0 passes bvh_nodes = nullptr: the function's own linear search (:199-207), which drops nothing - a ray that
// it blocks and the tree walk does not is one whose blocker sat under a dropped child.
void ref_sol_visibility(void* h, int use_bvh, int n_rays, const float* o, const float* d, const float* max_dist, const int* source,
                        const int* target, int* out) {
    RefScene* rs = (RefScene*)h;
    for (int k = 0; k < n_rays; k++) {
        Ray r(v3(o + 3 * k), v3(d + 3 * k));
        out[k] = visibility_test_anyhit(r, max_dist[k], use_bvh ? rs->nodes.data() : nullptr, rs->indices.data(), rs->prims, rs->n, source[k], target[k]) ? 1 : 0;
    }
}
// formfactor_rand_init (:84-88) for the given thread indices, stream mode: out = the six state words per index
void ref_sol_rand_init(int num_pairs, int n_idx, const int* idx, uint32_t* out_state) {
    std::vector<curandState> st((size_t)num_pairs);
    for (int k = 0; k < n_idx; k++) {
        set_thread_1d(idx[k], 256);
        formfactor_rand_init(num_pairs, st.data());
        std::memcpy(out_state + 6 * (size_t)k, st[idx[k]].s, sizeof(uint32_t) * 6);
    }
}

// calculate_form_factors_mc_kernel (use_mc) or calculate_form_factors_kernel for the given receiver rows, every j, on the
// working copy runSolver uploads and with formfactor_rand_init's states.  out_ff: n_rows * n; out_grid: n_rows * 256;
// out_rad_grid: n_rows * 256 * 3 (each may be NULL).
int ref_sol_ff_rows(void* h, int use_mc, int mc_samples, int n_rows, const int* rows, float* out_ff, float* out_grid,
                    float* out_rad_grid) {
    RefScene* rs = (RefScene*)h; const int n = rs->n;
    Quiet quiet;
    std::vector<Primitive> w = working_copy(rs);
    std::vector<float> ff((size_t)n * n, -1.0f);
    std::vector<curandState> st(use_mc ? (size_t)n * n : 0);
    for (int r = 0; r < n_rows; r++) {
        const int i = rows[r];
        if (i < 0 || i >= n) return -1;
        for (int j = 0; j < n; j++) {
            if (use_mc) {
                set_thread_1d(i * n + j, 256);
                formfactor_rand_init(n * n, st.data());
                set_thread_2d(j, i);   // i = y, j = x (:224-225)
                calculate_form_factors_mc_kernel(ff.data(), w.data(), n, mc_samples, st.data(), rs->nodes.data(), rs->indices.data());
            } else {
                set_thread_2d(i, j);   // i = x, j = y (:357-358)
                calculate_form_factors_kernel(ff.data(), w.data(), n, rs->nodes.data(), rs->indices.data());
            }
        }
        if (out_ff) std::memcpy(out_ff + (size_t)r * n, ff.data() + (size_t)i * n, sizeof(float) * n);
        get_grids(w[i], out_grid ? out_grid + (size_t)r * GRID_SIZE : nullptr, out_rad_grid ? out_rad_grid + (size_t)r * GRID_SIZE * 3 : nullptr);
    }
    return 0;
}

// One thread (i, j) of calculate_form_factors_mc_kernel on SCRIPTED raw words.  out_grid / out_rad_grid: receiver i's grids
// after this pair alone; returns the words drawn, *out_overrun set where the script ran out.
int ref_sol_mc_pair(void* h, int i, int j, int n_samples, const uint32_t* words, int n_words, float* out_F, float* out_grid,
                    float* out_rad_grid, int* out_overrun) {
    RefScene* rs = (RefScene*)h; const int n = rs->n;
    Quiet quiet;
    std::vector<Primitive> w = working_copy(rs);
    std::vector<float> ff((size_t)n * n, -1.0f);
    std::vector<curandState> st((size_t)n * n);
    std::memset(st.data(), 0, sizeof(curandState) * st.size());
    curandState& s = st[(size_t)i * n + j];
    s.script = words; s.n_script = n_words;
    set_thread_2d(j, i);
    calculate_form_factors_mc_kernel(ff.data(), w.data(), n, n_samples, st.data(), rs->nodes.data(), rs->indices.data());
    *out_F = ff[(size_t)i * n + j];
    get_grids(w[i], out_grid, out_rad_grid);
    *out_overrun = s.overrun;
    return s.used;
}

// update_radiosity_grid (:408-442) on the scene's primitives with the given form factors (n * n) and radiosity (n * 3)
void ref_sol_update_grid(void* h, const float* form_factors, const float* radiosity, float* out_rad_grid) {
    RefScene* rs = (RefScene*)h; const int n = rs->n;
    std::vector<Primitive> w(rs->prims, rs->prims + n);
    std::vector<float> ff(form_factors, form_factors + (size_t)n * n);
    for (int i = 0; i < n; i++) w[i].setRadiosity(v3(radiosity + 3 * i));
    dim3 grid_rad((n + 255) / 256, 1), block_rad(256, 1);
    PTMI_REF_LAUNCH(update_radiosity_grid, grid_rad, block_rad)(w.data(), ff.data(), n);
    for (int i = 0; i < n; i++) get_grids(w[i], nullptr, out_rad_grid + (size_t)i * GRID_SIZE * 3);
}

// radiosity_iteration_kernel (:444-467), one launch under the snapshot rule, from the given radiosity and unshot (n * 3)
void ref_sol_iterate(void* h, const float* form_factors, const float* radiosity, const float* unshot, float* out_radiosity,
                     float* out_unshot) {
    RefScene* rs = (RefScene*)h; const int n = rs->n;
    std::vector<Primitive> w(rs->prims, rs->prims + n);
    std::vector<float> ff(form_factors, form_factors + (size_t)n * n);
    for (int i = 0; i < n; i++) { w[i].setRadiosity(v3(radiosity + 3 * i)); w[i].setUnshotRad(v3(unshot + 3 * i)); }
    iterate_snapshot(w.data(), ff.data(), n);
    for (int i = 0; i < n; i++) { put3(out_radiosity + 3 * i, w[i].getRadiosity()); put3(out_unshot + 3 * i, w[i].getUnshotRad()); }
}

// RESTATED launch sequence of RadiosityState::runSolver (application_state.h:688-777) around the reference's own kernels
// and wrappers; the parameters are po_radiosity_params' fields.
int ref_sol_solve(void* h, int num_iterations, int mc_samples, int use_monte_carlo, int enable_filtering, int use_bilateral,
                  float filter_sigma_spatial, float filter_sigma_range, float* out_ff, float* out_radiosity, float* out_unshot,
                  float* out_grid, float* out_rad_grid) {
    RefScene* rs = (RefScene*)h; const int num_prims = rs->n;
    Quiet quiet;
    std::vector<Primitive> w = working_copy(rs);                          // :697-712
    Primitive* d_radiosity_primitives = w.data();
    std::vector<float> ff((size_t)num_prims * num_prims, 0.0f);
    float* d_form_factors = ff.data();
    BVHNode* d_bvh = rs->nodes.data(); int* d_indices = rs->indices.data();

    size_t num_pairs = (size_t)num_prims * num_prims;                     // :714-721
    std::vector<curandState> states(num_pairs);
    curandState* d_rand_states = states.data();
    int init_threads = 256, init_blocks = (num_pairs + init_threads - 1) / init_threads;
    PTMI_REF_LAUNCH(formfactor_rand_init, init_blocks, init_threads)(num_pairs, d_rand_states);

    dim3 threads(8, 8), blocks((num_prims + 7) / 8, (num_prims + 7) / 8);   // :730-738
    if (use_monte_carlo) {
        PTMI_REF_LAUNCH(calculate_form_factors_mc_kernel, blocks, threads)(
            d_form_factors, d_radiosity_primitives, num_prims, mc_samples, d_rand_states, d_bvh, d_indices);
    } else {
        PTMI_REF_LAUNCH(calculate_form_factors_kernel, blocks, threads)(
            d_form_factors, d_radiosity_primitives, num_prims, d_bvh, d_indices);
    }

    dim3 grid_rad((num_prims + 255) / 256, 1), block_rad(256, 1);         // :746-771
    for (int i = 0; i < num_iterations; ++i) {
        PTMI_REF_LAUNCH(store_radiosity_history_kernel, grid_rad, block_rad)(d_radiosity_primitives, num_prims);
        iterate_snapshot(d_radiosity_primitives, d_form_factors, num_prims);
        PTMI_REF_LAUNCH(update_radiosity_grid, grid_rad, block_rad)(d_radiosity_primitives, d_form_factors, num_prims);
        if (enable_filtering) {
            if (use_bilateral) {
                filter_radiosity_grids(d_radiosity_primitives, num_prims, GRID_RES,
                    filter_sigma_spatial, filter_sigma_range);
            } else {
                filter_radiosity_grids_gaussian(d_radiosity_primitives, num_prims, GRID_RES,
                    filter_sigma_spatial);
            }
        }
    }
    if (out_ff) std::memcpy(out_ff, d_form_factors, sizeof(float) * num_pairs);
    for (int i = 0; i < num_prims; i++) {
        if (out_radiosity) put3(out_radiosity + 3 * i, w[i].getRadiosity());
        if (out_unshot) put3(out_unshot + 3 * i, w[i].getUnshotRad());
        get_grids(w[i], out_grid ? out_grid + (size_t)i * GRID_SIZE : nullptr, out_rad_grid ? out_rad_grid + (size_t)i * GRID_SIZE * 3 : nullptr);
    }
    return 0;
}

// ---- the three filter wrappers of grid_filter.h, as written, on n primitives that carry the given grids ----
// filter_radiosity_grids (bilateral) / filter_radiosity_grids_gaussian: rgb n * 256 * 3 in, filtered grids out
void ref_sol_filter_grids(int n, const float* rgb, int use_bilateral, float sigma_spatial, float sigma_range, float* out) {
    std::vector<Primitive> w = with_grids(n, rgb, nullptr);
    if (use_bilateral) filter_radiosity_grids(w.data(), n, GRID_RES, sigma_spatial, sigma_range);
    else filter_radiosity_grids_gaussian(w.data(), n, GRID_RES, sigma_spatial);
    for (int i = 0; i < n; i++) get_grids(w[i], nullptr, out + (size_t)i * GRID_SIZE * 3);
}
// filter_pdfs_for_primitives: rgb n * 256 * 3 and counts n * 256 (NULL = zero) in, the two normalised pdf buffers out
void ref_sol_filter_pdfs(int n, const float* rgb, const float* counts, int use_bilateral, float sigma_spatial, float sigma_range,
                         float* out_formfactor, float* out_radiosity) {
    std::vector<Primitive> w = with_grids(n, rgb, counts);
    filter_pdfs_for_primitives(w.data(), out_formfactor, out_radiosity, n, GRID_RES, use_bilateral != 0, sigma_spatial, sigma_range);
}

// ---- subdivide_primitives (:520-574): a new scene handle (no tree) holding the subdivided list ----
void* ref_sol_subdivide(void* h, int num_subdivisions) {
    RefScene* rs = (RefScene*)h;
    Quiet quiet;
    std::vector<Primitive> in(rs->prims, rs->prims + rs->n);
    std::vector<Primitive> out = subdivide_primitives(in, num_subdivisions);
    RefScene* o = new RefScene;
    o->n = (int)out.size(); o->prims = new Primitive[out.size()];
    for (size_t i = 0; i < out.size(); i++) o->prims[i] = out[i];
    return o;
}

}  // extern "C"
