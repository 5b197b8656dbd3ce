// radiosity.hip — gfx950 kernels of the radiosity pre-pass: RadiosityState::runSolver
// (application_state.h:688-777; host/radiosity_state.cpp) and its kernels (form_factors.h:71-467, grid_filter.h:35-312).
//
// Compile with -ffp-contract=off (see include/ptmi_math.h, pt_vec.h): every output except the num_iterations == 0
// radiosity grid (order-dependent float atomics in the reference itself) is bit-identical to oracle/ptmi_oracle.c.
//
// The solver's files
//   anyhit.h           the visibility question of a pair - is anything else hit between the two sample points - stated once:
//                      the reference's any-hit walk, the walk over the fast tree, the certified walk's proof, pair_blocked
//   form_factors.hip   ptmi_form_factors and launch_form_factors: one WORKGROUP per receiver i (the reference: one thread
//                      per (i, j) pair).  The workgroup owns row i of the form-factor matrix and primitive i's two
//                      directional grids, so the reference's global atomics become LDS adds and one plain store per cell.
//                      Pairs are culled first (form_factors.h:234-256: ~2/3 of all pairs in a closed scene) and the
//                      survivors compacted through an LDS queue, so the Monte-Carlo loop runs on dense waves.  The
//                      reference keeps n^2 curandStates (48 B each) that nothing reads after the kernel; here a pair's
//                      XORWOW stream is derived where it is used, for surviving pairs only (ptmi_ff_row_jumps).
//   radiosity.hip      this file: everything after the form factors, with its launchers
//     ptmi_radiosity_iterate, ptmi_radiosity_iterate_tiled
//                           radiosity_iteration_kernel (form_factors.h:441-465) with the race removed (Jacobi)
//     ptmi_radiosity_grid   update_radiosity_grid (form_factors.h:405-439) + the optional 5x5 filter (grid_filter.h);
//                           one workgroup per primitive, one thread per grid cell, contributions added in ascending j
//     ptmi_filter_pdfs      filter_pdfs_for_primitives (grid_filter.h:329-507)
//     ptmi_cdf_records      SceneState::precomputeCDFs: one PrecomputedCDF record per primitive
#include "pt_device.h"

namespace ptmi {

namespace {

// radiosity_iteration_kernel (form_factors.h:441-465): one thread per receiver, ascending j - the float sum is a
// sequential chain per row, so rows are the only parallelism and the kernel is bound by that chain (~12 VALU ops per
// j), provided the row data arrive in time: a lane streams its own row in 64-float groups (sixteen 16-byte loads),
// the NEXT group's loads are issued before the current group is consumed; unshot[] is staged through LDS in chunks and
// read as a broadcast.  One wave per workgroup, so the 64-row groups spread over as many CUs as possible.
constexpr int kIterChunk = 1024, kIterBlock = 64, kIterGroup = 64;
struct RowGroup { float4 q[kIterGroup / 4]; };
__device__ __forceinline__ void load_group(RowGroup& g, const float* p) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll
    for (int k = 0; k < kIterGroup / 4; k++) g.q[k] = p4[k];
}
__device__ __forceinline__ void consume_group(const RowGroup& g, const float4* u, int j0, int i, f3& incident_rad) {
#pragma unroll
    for (int k = 0; k < kIterGroup / 4; k++) {
        const float f[4] = {g.q[k].x, g.q[k].y, g.q[k].z, g.q[k].w};
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float4 uj = u[4 * k + c];
            const bool take = (j0 + 4 * k + c != i) & (f[c] > 0.0f);
            const float tx = incident_rad.x + f[c] * uj.x, ty = incident_rad.y + f[c] * uj.y, tz = incident_rad.z + f[c] * uj.z;
            incident_rad.x = take ? tx : incident_rad.x;            // per component: a struct select goes through scratch
            incident_rad.y = take ? ty : incident_rad.y;
            incident_rad.z = take ? tz : incident_rad.z;
        }
    }
}
__global__ __launch_bounds__(kIterBlock) void ptmi_radiosity_iterate(RadiosityBuffers rb, int src) {
    __shared__ float4 u_lds[kIterChunk];
    const int n = rb.n;
    const int i = blockIdx.x * kIterBlock + threadIdx.x;
    const int row_i = min(i, n - 1);                           // lanes past the end walk the last row and store nothing
    const float* __restrict__ row = rb.form_factors + (size_t)row_i * (size_t)n;
    const float4* __restrict__ unshot = rb.unshot[src];
    const int n_vec = (n & 3) == 0 ? (n / kIterGroup) * kIterGroup : 0;   // rows start on 16-byte boundaries only if n % 4 == 0
    f3 incident_rad = mk3(0.0f, 0.0f, 0.0f);
    RowGroup ga, gb;
    if (n_vec > 0) load_group(ga, row);
    for (int base = 0; base < n; base += kIterChunk) {         // kIterChunk is a multiple of 2 * kIterGroup
        const int m = min(kIterChunk, n - base);
        __syncthreads();
        for (int k = threadIdx.x; k < m; k += kIterBlock) u_lds[k] = unshot[base + k];
        __syncthreads();
        int jj = 0;
        for (; base + jj + 2 * kIterGroup <= n_vec && jj + 2 * kIterGroup <= m; jj += 2 * kIterGroup) {
            load_group(gb, row + base + jj + kIterGroup);
            consume_group(ga, u_lds + jj, base + jj, i, incident_rad);
            if (base + jj + 3 * kIterGroup <= n_vec) load_group(ga, row + base + jj + 2 * kIterGroup);
            consume_group(gb, u_lds + jj + kIterGroup, base + jj + kIterGroup, i, incident_rad);
        }
        if (base + jj + kIterGroup <= n_vec && jj + kIterGroup <= m) {      // an odd group left over at the end of the vector part
            consume_group(ga, u_lds + jj, base + jj, i, incident_rad);
            jj += kIterGroup;
            if (base + jj + kIterGroup <= n_vec) load_group(ga, row + base + jj);
        }
        for (; jj < m; jj++) {
            const float F_ij = row[base + jj];
            if (base + jj != i && F_ij > 0.0f) incident_rad = incident_rad + F_ij * xyz(u_lds[jj]);
        }
    }
    if (i >= n) return;
    const f3 bsdf = xyz(rb.bsdf[i]);
    const f3 reflected = mk3(fminf(bsdf.x * incident_rad.x, incident_rad.x), fminf(bsdf.y * incident_rad.y, incident_rad.y),
                             fminf(bsdf.z * incident_rad.z, incident_rad.z));
    const f3 rad = xyz(rb.radiosity[i]) + reflected;
    rb.radiosity[i] = make_float4(rad.x, rad.y, rad.z, 0.0f);
    rb.unshot[1 - src][i] = make_float4(reflected.x, reflected.y, reflected.z, 0.0f);
}


// ---- ptmi_radiosity_iterate_tiled: the same step as an HBM stream ----------------------------------------------------------
// The Jacobi step reads the n x n form-factor matrix once (4 n^2 bytes: 268 MB at n = 8192) and does 6 flops per entry,
// so its roofline is HBM bandwidth; what holds it back is that every row's sum is ONE sequential float chain (ascending j -
// the reference's order, form_factors.h:452-459, which fixes the bits).  With a lane per row (the kernel above) a wave reads
// 64 rows at a 4n-byte stride - 64 cache lines per load instruction - and its chain costs 11 instructions per j.
// Here a 64-thread workgroup owns R = 8 (or 16) rows:
//   * loading: one global_load_dwordx4 per lane covers 256 consecutive floats of ONE row (1 KiB, fully coalesced); R of
//     them are an R x 256 tile, issued for tile t + 1 before tile t is consumed (R KiB in flight per wave), staged in LDS
//     with a row stride of 260 floats (the lanes of a 16-lane group then read different rows from different banks);
//   * summing: lane = channel * R + row, i.e. the three colour channels of a row are three lanes, each with ONE running
//     sum.  F is read from LDS as a broadcast to the row's three lanes, the unshot radiosity as a per-channel (SoA)
//     broadcast to a channel's sixteen.  Entries the reference skips (`j != i && F_ij > 0.0f` false: the diagonal, F <= 0,
//     columns past n) are stored as +0 in the tile, and adding 0 * u_j changes nothing while u_j is finite - so per j the
//     chain is one multiply and one add (the lane-per-row kernel: 3 + 3 + 3 selects + 2 compares); a tile holding a
//     non-finite unshot value takes the compare / select form.  Same sums in the same order: bit-identical to the kernel
//     above and to the oracle.
constexpr int kTileCols = 256, kTileStride = kTileCols + 4, kUStride = kTileCols / 4 + 1;
template <int kTileRows>
__global__ __launch_bounds__(64) void ptmi_radiosity_iterate_tiled(RadiosityBuffers rb, int src) {
    __shared__ float4 f_lds[kTileRows * kTileStride / 4];
    __shared__ float4 u_lds[4][kUStride];                             // [channel][column], channels on different banks
    const int n = rb.n, lane = threadIdx.x;
    const int row0 = blockIdx.x * kTileRows;
    const int ch = lane / kTileRows, r = lane % kTileRows, i = row0 + r;   // the lane's running sum: channel ch (>= 3: none) of row i
    const float* __restrict__ F = rb.form_factors;
    const float4* __restrict__ unshot = rb.unshot[src];
    const int n_tiles = (n + kTileCols - 1) / kTileCols;
    float4 fr[kTileRows], ur[4];
    auto issue = [&](int t) {                                         // tile t -> registers (n % 4 == 0: a float4 never straddles n)
        const int col = t * kTileCols + 4 * lane;
#pragma unroll
        for (int k = 0; k < kTileRows; k++) {
            const int rk = min(row0 + k, n - 1);
            fr[k] = col < n ? *reinterpret_cast<const float4*>(F + (size_t)rk * (size_t)n + col) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int j = t * kTileCols + lane + 64 * c;
            ur[c] = j < n ? unshot[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    };
    bool u_finite = true;                                             // wave-uniform: every unshot value of the tile is finite
    auto commit = [&](int t) {                                        // registers -> LDS
        // entries the reference skips (F_ij <= 0, or NaN) become +0: with a finite u_j, `sum + 0 * u_j` leaves the running sum
        // as it is (it is never -0: it starts at +0), so the chain below needs no compare / select per entry
#pragma unroll
        for (int k = 0; k < kTileRows; k++)
            f_lds[(k * kTileStride) / 4 + lane] = make_float4(fmaxf(fr[k].x, 0.0f), fmaxf(fr[k].y, 0.0f), fmaxf(fr[k].z, 0.0f), fmaxf(fr[k].w, 0.0f));
        bool fin = true;
#pragma unroll
        for (int c = 0; c < 4; c++) fin = fin && isfinite(ur[c].x) && isfinite(ur[c].y) && isfinite(ur[c].z);
        u_finite = __all(fin);
        float* us = reinterpret_cast<float*>(u_lds);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int jl = lane + 64 * c;
            us[0 * 4 * kUStride + jl] = ur[c].x; us[1 * 4 * kUStride + jl] = ur[c].y; us[2 * 4 * kUStride + jl] = ur[c].z; us[3 * 4 * kUStride + jl] = 0.0f;
        }
        __syncthreads();
        const int d = i - t * kTileCols;                              // the diagonal entry of row i, if it lies in this tile
        if (ch == 0 && d >= 0 && d < kTileCols) reinterpret_cast<float*>(f_lds)[r * kTileStride + d] = 0.0f;
        __syncthreads();
    };
    float acc = 0.0f;
    issue(0);
    for (int t = 0; t < n_tiles; t++) {
        commit(t);
        if (t + 1 < n_tiles) issue(t + 1);
        const float4* frow = f_lds + (r * kTileStride) / 4;
        const float4* urow = u_lds[min(ch, 3)];
        if (u_finite) {
#pragma unroll 8
            for (int q = 0; q < kTileCols / 4; q++) {
                const float4 f4 = frow[q], u4 = urow[q];
                acc = acc + f4.x * u4.x; acc = acc + f4.y * u4.y; acc = acc + f4.z * u4.z; acc = acc + f4.w * u4.w;
            }
        } else {                                                      // an infinite or NaN unshot value: 0 * u_j would not be 0
#pragma unroll 4
            for (int q = 0; q < kTileCols / 4; q++) {
                const float4 f4 = frow[q], u4 = urow[q];
                float tsum;
                tsum = acc + f4.x * u4.x; acc = f4.x > 0.0f ? tsum : acc;
                tsum = acc + f4.y * u4.y; acc = f4.y > 0.0f ? tsum : acc;
                tsum = acc + f4.z * u4.z; acc = f4.z > 0.0f ? tsum : acc;
                tsum = acc + f4.w * u4.w; acc = f4.w > 0.0f ? tsum : acc;
            }
        }
        __syncthreads();                                              // the tile is consumed before commit(t + 1) overwrites it
    }
    if (i >= n) return;
    float* rad = reinterpret_cast<float*>(rb.radiosity + i);
    float* out = reinterpret_cast<float*>(rb.unshot[1 - src] + i);
    if (ch > 3) return;
    if (ch == 3) { out[3] = 0.0f; return; }
    const float bsdf = reinterpret_cast<const float*>(rb.bsdf + i)[ch];
    const float reflected = fminf(bsdf * acc, acc);
    rad[ch] = rad[ch] + reflected;
    out[ch] = reflected;
}

// grid_filter.h:35-41, 55-101 (bilateral), 221-249 (gaussian)
__device__ __forceinline__ float gaussian_weight(float distance, float sigma) { return ptmi_expf(-(distance * distance) / (2.0f * sigma * sigma)); }
__device__ __forceinline__ float luminance_from_rgb(f3 rgb) { return 0.2126f * rgb.x + 0.7152f * rgb.y + 0.0722f * rgb.z; }
__device__ __forceinline__ f3 filter_cell(const float4* g, int center_i, int center_j, bool bilateral, float sigma_spatial, float sigma_range) {
    const f3 center_val = xyz(g[center_i * kGridRes + center_j]);
    const float center_lum = luminance_from_rgb(center_val);
    f3 weighted_sum = mk3(0.0f, 0.0f, 0.0f);
    float total_weight = 0.0f;
    for (int di = -2; di <= 2; di++)
        for (int dj = -2; dj <= 2; dj++) {
            const int ni = center_i + di;
            const int nj = (center_j + dj + kGridRes) % kGridRes;
            if (ni < 0 || ni >= kGridRes) continue;
            const f3 neighbor_val = xyz(g[ni * kGridRes + nj]);
            const float spatial_dist = sqrt_rn((float)(di * di + dj * dj));
            float weight = gaussian_weight(spatial_dist, sigma_spatial);
            if (bilateral) {
                const float range_dist = fabsf(center_lum - luminance_from_rgb(neighbor_val));
                weight = weight * gaussian_weight(range_dist, sigma_range);
            }
            weighted_sum = weighted_sum + weight * neighbor_val;
            total_weight += weight;
        }
    if (total_weight > 1e-6f) return div_scalar(weighted_sum, total_weight);
    return center_val;
}

// update_radiosity_grid (form_factors.h:405-439): workgroup = primitive i, thread = grid cell.  Phase A computes, in
// parallel, which cell each j falls into (the acos/atan2 part); phase B lets every cell's owner add its contributions
// in ascending j, the order of the reference's single thread per primitive.
constexpr int kGridChunk = 2048;
__global__ __launch_bounds__(kBlock) void ptmi_radiosity_grid(RadiosityBuffers rb, RadiosityParams prm) {
    __shared__ unsigned short cell[kGridChunk];
    __shared__ float4 g[kGridSize];
    const int n = rb.n;
    const int i = blockIdx.x;
    const int tid = threadIdx.x;
    const f3 center_i = xyz(rb.geo[6 * i + 5]), normal_i = xyz(rb.geo[6 * i + 4]);
    const float* __restrict__ row = rb.form_factors + (size_t)i * (size_t)n;
    f3 acc = mk3(0.0f, 0.0f, 0.0f);
    for (int base = 0; base < n; base += kGridChunk) {
        const int m = min(kGridChunk, n - base);
        for (int jj = tid; jj < m; jj += kBlock) {
            const int j = base + jj;
            unsigned short c = 0xffffu;
            if (j != i && !(row[j] <= 0.0f)) {                // form_factors.h:424 skips F_ij <= 0: a NaN form factor is taken
                f3 dir_ij = xyz(rb.geo[6 * j + 5]) - center_i;
                const float r = length(dir_ij);
                if (!(r < 1e-6f)) {
                    dir_ij = div_scalar(dir_ij, r);
                    c = (unsigned short)direction_to_grid_index_local(dir_ij, normal_i);
                }
            }
            cell[jj] = c;
        }
        __syncthreads();
        for (int jj = 0; jj < m; jj++) {
            if (cell[jj] == tid) {
                const int j = base + jj;
                acc = acc + row[j] * xyz(rb.radiosity[j]);
            }
        }
        __syncthreads();
    }
    if (prm.enable_filtering) {                              // application_state.h:759-767
        g[tid] = make_float4(acc.x, acc.y, acc.z, 0.0f);
        __syncthreads();
        acc = filter_cell(g, tid / kGridRes, tid % kGridRes, prm.use_bilateral != 0, prm.filter_sigma_spatial, prm.filter_sigma_range);
    }
    rb.rad_grid[(size_t)i * kGridSize + tid] = make_float4(acc.x, acc.y, acc.z, 0.0f);
}

// filter_pdfs_for_primitives (grid_filter.h:329-507): luminance of the radiosity grid and the count grid, each through
// the 5x5 float filter (bilateral :381-406 / gaussian :352-379) and normalize_pdf_kernel (:409-418, a sequential sum).
__device__ __forceinline__ float filter_cell_float(const float* src, int ci, int cj, bool bilateral, float sigma_spatial, float sigma_range) {
    const float center = src[ci * kGridRes + cj];
    float weighted_sum = 0.0f, total_weight = 0.0f;
    for (int di = -2; di <= 2; di++)
        for (int dj = -2; dj <= 2; dj++) {
            const int ni = ci + di, nj = (cj + dj + kGridRes) % kGridRes;
            if (ni < 0 || ni >= kGridRes) continue;
            float w = gaussian_weight(sqrt_rn((float)(di * di + dj * dj)), sigma_spatial);
            if (bilateral) w = w * gaussian_weight(fabsf(center - src[ni * kGridRes + nj]), sigma_range);
            weighted_sum += src[ni * kGridRes + nj] * w;
            total_weight += w;
        }
    if (total_weight > 1e-6f) return weighted_sum / total_weight;
    return center;
}
__global__ __launch_bounds__(kBlock) void ptmi_filter_pdfs(const float* __restrict__ rgb, const float* __restrict__ counts,
                                                           float* __restrict__ out_formfactor, float* __restrict__ out_radiosity,
                                                           int bilateral, float sigma_spatial, float sigma_range) {
    __shared__ float lum[kGridSize], cnt[kGridSize], f_lum[kGridSize], f_cnt[kGridSize];
    __shared__ float sums[2];
    const size_t base = (size_t)blockIdx.x * kGridSize;
    const int tid = threadIdx.x;
    const float* c = rgb + (base + tid) * 3;
    lum[tid] = luminance_from_rgb(mk3(c[0], c[1], c[2]));                      // luminanceFromRGB (grid_filter.h:39-41)
    cnt[tid] = counts ? counts[base + tid] : 0.0f;
    __syncthreads();
    f_lum[tid] = filter_cell_float(lum, tid / kGridRes, tid % kGridRes, bilateral != 0, sigma_spatial, sigma_range);
    f_cnt[tid] = filter_cell_float(cnt, tid / kGridRes, tid % kGridRes, bilateral != 0, sigma_spatial, sigma_range);
    __syncthreads();
    if (tid == 0 || tid == 64) {                                               // one lane of two different waves
        const float* src = tid == 0 ? f_lum : f_cnt;
        float sum = 0.0f;
        for (int i = 0; i < kGridSize; i++) sum += src[i];
        sums[tid ? 1 : 0] = sum;
    }
    __syncthreads();
    out_radiosity[base + tid] = (sums[0] <= 1e-12f) ? f_lum[tid] : f_lum[tid] / sums[0];
    out_formfactor[base + tid] = (sums[1] <= 1e-12f) ? f_cnt[tid] : f_cnt[tid] / sums[1];
}

// SceneState::precomputeCDFs / precomputeCDFsFromFiltered (application_state.h:492-585, 587-680): one PrecomputedCDF record
// per primitive, one thread each - every sum runs in the reference's order.  SRC 0: float4 radiosity grids (the solver's),
// 1: packed float3 grids (host-supplied), 2: ready pdf values (filtered luminance).
template <int SRC>
__global__ __launch_bounds__(kBlock) void ptmi_cdf_records(const void* __restrict__ src, float* __restrict__ out, int n) {
    // one workgroup per primitive, one thread per cell; the sequential sums are done by one thread per row (and thread 0
    // for the marginal) from LDS, in the reference's order
    __shared__ float pdf[kGridSize], row_cdfs[kGridSize], row_sums[kGridRes / 2], marginal[kGridRes / 2];
    __shared__ float total;
    constexpr int GRID_HALF_RES = kGridRes / 2;
    const float GRID_INV_RES = 1.0f / kGridRes;
    const int p = blockIdx.x, i = threadIdx.x;
    float v;
    if (SRC == 0) { const float4 c = static_cast<const float4*>(src)[(size_t)p * kGridSize + i]; v = luminance_from_rgb(xyz(c)); }
    else if (SRC == 1) { const float* c = static_cast<const float*>(src) + ((size_t)p * kGridSize + i) * 3; v = luminance_from_rgb(mk3(c[0], c[1], c[2])); }
    else v = static_cast<const float*>(src)[(size_t)p * kGridSize + i];
    pdf[i] = v;
    __syncthreads();
    if (i < GRID_HALF_RES) {
        float row_sum = 0.0f;
        for (int u = 0; u < kGridRes; u++) row_sum += pdf[i * kGridRes + u];
        row_sums[i] = row_sum;
    }
    __syncthreads();
    if (i == 0) {
        float total_weight = 0.0f;
        for (int r = 0; r < GRID_HALF_RES; r++) total_weight += row_sums[r];
        float running = 0.0f;
        const float inv_total = (total_weight > 1e-6f) ? (1.0f / total_weight) : 0.0f;
        for (int r = 0; r < GRID_HALF_RES; r++) { running += row_sums[r]; marginal[r] = running * inv_total; }
        marginal[GRID_HALF_RES - 1] = 1.0f;
        total = total_weight;
    }
    if (i < kGridRes) {                                   // thread i = row i
        const int ro = i * kGridRes;
        if (i >= GRID_HALF_RES || row_sums[i] < 1e-6f) {
            for (int u = 0; u < kGridRes; u++) row_cdfs[ro + u] = (float)(u + 1) * GRID_INV_RES;
        } else {
            float running_row = 0.0f;
            const float inv_row_sum = 1.0f / row_sums[i];
            for (int u = 0; u < kGridRes; u++) { running_row += pdf[ro + u]; row_cdfs[ro + u] = running_row * inv_row_sum; }
            row_cdfs[ro + kGridRes - 1] = 1.0f;
        }
    }
    __syncthreads();
    float* cdf = out + (size_t)p * kCdfDwords;
    cdf[kCdfPdf + i] = pdf[i];
    cdf[kCdfRowCdfs + i] = row_cdfs[i];
    if (i < GRID_HALF_RES) { cdf[kCdfRowSums + i] = row_sums[i]; cdf[kCdfMarginal + i] = marginal[i]; }
    if (i == 0) { cdf[kCdfTotal] = total; cdf[kCdfValid] = __int_as_float(total > 1e-6f ? 1 : 0); }
}

}  // namespace

void launch_radiosity_iteration(const RadiosityBuffers& rb, int src, hipStream_t s) {
    if (rb.n <= 0) return;
    static const bool force_rows = getenv("PTMI_RADIOSITY_ROWS") != nullptr;        // A/B knob: the lane-per-row kernel
    // rows per 64-thread workgroup: 8 (24 summing lanes, n / 8 waves: 4 per CU at n = 8192) measured 83 us per step at n = 8192
    // against 91 us with 16 (48 summing lanes, 2 waves per CU): more waves, more row data in flight
    static const int tile_rows = getenv("PTMI_RADIOSITY_TILE_ROWS") ? atoi(getenv("PTMI_RADIOSITY_TILE_ROWS")) : 8;
    if ((rb.n & 3) == 0 && rb.n >= 64 && !force_rows) {                              // rows are 16-byte aligned only if n % 4 == 0
        if (tile_rows == 16) hipLaunchKernelGGL(ptmi_radiosity_iterate_tiled<16>, dim3((rb.n + 15) / 16), dim3(64), 0, s, rb, src);
        else hipLaunchKernelGGL(ptmi_radiosity_iterate_tiled<8>, dim3((rb.n + 7) / 8), dim3(64), 0, s, rb, src);
    }
    else
        hipLaunchKernelGGL(ptmi_radiosity_iterate, dim3((rb.n + kIterBlock - 1) / kIterBlock), dim3(kIterBlock), 0, s, rb, src);
}

void launch_cdf_records(int n, const void* d_src, int src_kind, float* d_out, hipStream_t s) {
    if (n <= 0) return;
    const dim3 grid(n), block(kBlock);
    if (src_kind == 0) hipLaunchKernelGGL(ptmi_cdf_records<0>, grid, block, 0, s, d_src, d_out, n);
    else if (src_kind == 1) hipLaunchKernelGGL(ptmi_cdf_records<1>, grid, block, 0, s, d_src, d_out, n);
    else hipLaunchKernelGGL(ptmi_cdf_records<2>, grid, block, 0, s, d_src, d_out, n);
}

void launch_filter_pdfs(int n, const float* d_rgb, const float* d_counts, float* d_out_formfactor, float* d_out_radiosity,
                        bool bilateral, float sigma_spatial, float sigma_range, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_filter_pdfs, dim3(n), dim3(kBlock), 0, s, d_rgb, d_counts, d_out_formfactor, d_out_radiosity,
                       bilateral ? 1 : 0, sigma_spatial, sigma_range);
}

void launch_radiosity_grid(const RadiosityBuffers& rb, const RadiosityParams& prm, hipStream_t s) {
    if (rb.n <= 0) return;
    hipLaunchKernelGGL(ptmi_radiosity_grid, dim3(rb.n), dim3(kBlock), 0, s, rb, prm);
}

}  // namespace ptmi
