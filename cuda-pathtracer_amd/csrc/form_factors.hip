// form_factors.hip — ptmi_form_factors, the first kernel of the radiosity pre-pass (radiosity.hip lists the solver's files), with
// what only it uses: the pairs' XORWOW skip-ahead (gf2_apply, ptmi_ff_row_jumps, pair_rng_init), the Monte-Carlo and the
// point-to-point form factor of one pair (mc_pair, p2p_pair) and launch_form_factors.  Its visibility walks are csrc/anyhit.h.
// Compile with -ffp-contract=off (see include/ptmi_math.h, pt_vec.h).
#include "pt_device.h"
#include "anyhit.h"
#include "prim_sample.h"

namespace ptmi {

namespace {

constexpr int kQueueCap = 2 * kBlock;

__device__ __forceinline__ Geom load_geom(const float4* __restrict__ geo, int p) {
    const float4 a = geo[6 * p], b = geo[6 * p + 1], c = geo[6 * p + 2], d = geo[6 * p + 3], e = geo[6 * p + 4], f = geo[6 * p + 5];
    Geom g;
    g.v0 = xyz(a); g.v1 = xyz(b); g.v2 = xyz(c); g.v3 = xyz(d);
    g.type = __float_as_int(a.w); g.area = b.w; g.ratio = c.w;
    g.normal = xyz(e); g.centroid = xyz(f);
    return g;
}

// formfactor_rand_init (form_factors.h:85-89): curand_init(12345 + idx, idx, 0).  Block-synchronous: one 160x160 GF(2)
// matrix T^(2^67 * 2^k) at a time is staged in LDS and applied by the threads whose idx has bit k set.
// ROW (rb.row_jump): idx = i * n + j, and the skip-ahead T^(2^67 idx) = T^(2^67 i n) T^(2^67 j) (powers of one matrix commute, the
// exponents add as integers, carries included): the first factor is the same for every pair of receiver i and comes precomputed
// (ptmi_ff_row_jumps), so a pair applies one matrix per set bit of j (< n) plus that one - 7.5 instead of 13 at n = 8192.
__device__ __forceinline__ void gf2_apply(const uint32_t* M, uint32_t (&v)[5]) {
    uint32_t r[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int w = 0; w < 5; w++) {
        const uint32_t word = v[w];
        for (int b = 0; b < 32; b++) {
            const uint32_t m = 0u - ((word >> b) & 1u);
            const uint32_t* row = &M[(w * 32 + b) * 5];
            r[0] ^= row[0] & m; r[1] ^= row[1] & m; r[2] ^= row[2] & m; r[3] ^= row[3] & m; r[4] ^= row[4] & m;
        }
    }
#pragma unroll
    for (int w = 0; w < 5; w++) v[w] = r[w];
}
// P_i = T^(2^67 * (i * n)) for every receiver i: the product of the table's matrices T^(2^67 * 2^k) over the set bits k of i * n.
// A matrix is stored as the images of the 160 basis vectors (row r = M e_r, 5 words), so (B A) e_r = B applied to row r of A.
__global__ __launch_bounds__(kBlock) void ptmi_ff_row_jumps(uint32_t* __restrict__ out, int n, const uint32_t* __restrict__ jump) {
    __shared__ uint32_t A[160 * 5], B[160 * 5];
    const int i = blockIdx.x, tid = threadIdx.x;
    const unsigned int hi = (unsigned int)(i * n);
    for (int x = tid; x < 160 * 5; x += kBlock) A[x] = (x / 5) / 32 == x % 5 ? (1u << ((x / 5) % 32)) : 0u;      // the identity: row r = e_r
    __syncthreads();
    for (int k = 0; k < 32; k++) {
        if (!((hi >> k) & 1u)) continue;                                  // block-uniform
        for (int x = tid; x < 160 * 5; x += kBlock) B[x] = jump[k * 160 * 5 + x];
        __syncthreads();
        uint32_t v[5] = {0u, 0u, 0u, 0u, 0u};
        if (tid < 160) { for (int w = 0; w < 5; w++) v[w] = A[tid * 5 + w]; gf2_apply(B, v); }
        __syncthreads();
        if (tid < 160) for (int w = 0; w < 5; w++) A[tid * 5 + w] = v[w];
        __syncthreads();
    }
    for (int x = tid; x < 160 * 5; x += kBlock) out[(size_t)i * 160 * 5 + x] = A[x];
}

__device__ __forceinline__ void pair_rng_init(uint32_t* M, const uint32_t* __restrict__ jump, bool have, unsigned int idx, Rng& out,
                                              const uint32_t* __restrict__ row_jump = nullptr, unsigned int j = 0u, bool row_is_identity = false) {
    const unsigned long long seed = 12345ull + (unsigned long long)idx;
    const uint32_t s0 = ((uint32_t)seed) ^ 0xaad26b49u;
    const uint32_t s1 = (uint32_t)(seed >> 32) ^ 0xf7dcefddu;
    const uint32_t t0 = 1099087573u * s0;
    const uint32_t t1 = 2591861531u * s1;
    uint32_t v[5] = {123456789u + t0, 362436069u ^ t0, 521288629u + t1, 88675123u ^ t1, 5783321u + t0};
    const uint32_t d = 6615241u + t1 + t0;
    const unsigned int bits = row_jump ? j : idx;                        // with the row's shared factor: only the bits of j here
    for (int k = 0; k < 32; k++) {
        const bool mine = have && ((bits >> k) & 1u);
        if (!__syncthreads_or(mine ? 1 : 0)) continue;
        for (int i = threadIdx.x; i < 160 * 5; i += kBlock) M[i] = jump[k * 160 * 5 + i];
        __syncthreads();
        if (mine) gf2_apply(M, v);
        __syncthreads();
    }
    if (row_jump && !row_is_identity) {                                   // block-uniform: T^(2^67 i n), the same for the whole row
        for (int i = threadIdx.x; i < 160 * 5; i += kBlock) M[i] = row_jump[i];
        __syncthreads();
        if (have) gf2_apply(M, v);
        __syncthreads();
    }
    out = Rng{v[0], v[1], v[2], v[3], v[4], d};
}

// the sample loop and F_ij of calculate_form_factors_mc_kernel (form_factors.h:259-365) for one surviving pair
// The emitter's record is read again for every sample (it is L1-resident, and only the sample's first lines use it): its
// 13 - 18 registers do not have to live through the visibility walk, where the kernel is short of them (7 waves per SIMD).
template <bool HAS_QUADS, bool DEEP, bool RAD0, int WIDE>
__device__ __forceinline__ float mc_pair(const DeviceScene& sc, uint2* wstack, int i, const Geom& gi, const float4* __restrict__ geo, int j, int slot_i, int slot_j,
                                         int actual_samples, Rng& rng, f3 radiosity_j, unsigned int* counts, float* radg, unsigned int& rays, unsigned long long& chain) {
    float visibility_sum = 0.0f, cos_i_sum = 0.0f, cos_j_sum = 0.0f, dist_sum = 0.0f;
    int valid_samples = 0;
    for (int s = 0; s < actual_samples; ++s) {
        asm volatile("" ::: "memory");                                          // keeps the loads below inside the loop
        const Geom gj = load_geom(geo, j);
        float r1 = rng_uniform(rng), r2 = rng_uniform(rng);
        const f3 p_i = sample_uniform<HAS_QUADS>(gi, r1, r2);
        r1 = rng_uniform(rng); r2 = rng_uniform(rng);
        const f3 p_j = sample_uniform<HAS_QUADS>(gj, r1, r2);
        f3 sample_dir = p_j - p_i;
        const float r = length(sample_dir);
        if (r < 1e-6f) continue;
        sample_dir = div_scalar(sample_dir, r);
        const float cos_theta_i = dot(gi.normal, sample_dir);
        const float cos_theta_j = -dot(gj.normal, sample_dir);
        if (cos_theta_i <= 0.0f || cos_theta_j <= 0.0f) continue;
        const f3 ro = p_i + 1e-4f * gi.normal;
        const f3 rd = unit_vector(sample_dir);                                  // Ray's constructor normalises again (ray.h:9-12)
        rays++;
        const bool blocked = PAIR_BLOCKED(WIDE, HAS_QUADS, DEEP, sc, wstack, ro, rd, r - 2e-4f, i, j, slot_i, slot_j, chain);
        if (!blocked) {
            visibility_sum += 1.0f; cos_i_sum += cos_theta_i; cos_j_sum += cos_theta_j; dist_sum += r;
            valid_samples++;
            const int grid_idx = direction_to_grid_index_local(sample_dir, gi.normal);
            atomicAdd(&counts[grid_idx], 1u);
            if (RAD0) {
                const float geometric_weight = (cos_theta_i * cos_theta_j) / (r * r);
                const f3 contrib = gj.area * (geometric_weight * radiosity_j);
                atomicAdd(&radg[3 * grid_idx], contrib.x); atomicAdd(&radg[3 * grid_idx + 1], contrib.y); atomicAdd(&radg[3 * grid_idx + 2], contrib.z);
            }
        }
    }
    if (valid_samples > 0) {
        const float avg_cos_i = cos_i_sum / (float)valid_samples;
        const float avg_cos_j = cos_j_sum / (float)valid_samples;
        const float avg_dist = dist_sum / (float)valid_samples;
        const float visibility_fraction = visibility_sum / (float)actual_samples;
        const float area_j = geo[6 * j + 1].w;
        const float F_ij = (float)((double)(visibility_fraction * (avg_cos_i * avg_cos_j * area_j)) /
                                   (PTMI_PI_D * (double)avg_dist * (double)avg_dist));
        return fmaxf(0.0f, fminf(F_ij, 1.0f));
    }
    return 0.0f;
}

// calculate_form_factors_kernel (form_factors.h:368-415) after its culling tests
template <bool HAS_QUADS, bool DEEP, int WIDE>
__device__ __forceinline__ float p2p_pair(const DeviceScene& sc, uint2* wstack, int i, int j, const Geom& gi, const Geom& gj, int slot_i, int slot_j, unsigned int& rays,
                                          unsigned long long& chain) {
    const f3 vec_ij = gj.centroid - gi.centroid;
    const float r = length(vec_ij);
    const f3 dir_ij = div_scalar(vec_ij, r);
    const float cos_theta_i = dot(gi.normal, dir_ij);
    const float cos_theta_j = dot(gj.normal, -dir_ij);
    const f3 ro = gi.centroid + 1e-4f * gi.normal;
    const f3 rd = unit_vector(dir_ij);
    rays++;
    if (PAIR_BLOCKED(WIDE, HAS_QUADS, DEEP, sc, wstack, ro, rd, r - 2e-4f, i, j, slot_i, slot_j, chain)) return 0.0f;
    const float ff = (float)((double)(cos_theta_i * cos_theta_j * gj.area) / (PTMI_PI_D * (double)r * (double)r));
    return fmaxf(0.0f, ff);
}

// 7 waves per SIMD (72 VGPRs, 23 dwords spilled) instead of the 4 the kernel asks for by itself (112 VGPRs): the any-hit walks
// wait on L2, and more waves in flight are worth more than the spills cost - n = 8192: 4 / 5 / 6 / 7 / 8 waves 168.6 / 151.6 /
// 139.0 / 134.8 / 133.5 ms, and 131.4 ms at 7 waves with the emitter's record re-read per sample (mc_pair); n = 2048: 7 waves
// 14.5 ms, 8 waves 15.0 ms
#ifndef PTMI_FF_WIDE_WAVES
#define PTMI_FF_WIDE_WAVES 6
#endif
// WIDE (1: the opt-in fast tree, 2: the certified walk - the default from 256 triangles up): the visibility walk goes through
// visibility_blocked_wide; its node test wants ~80 registers, so that build is bounded to 6 waves per SIMD (n = 8192, fast tree:
// 4 / 5 / 6 waves 78.8 / 74.9 / 70.4 ms; certified: 5 / 6 / 7 waves 84.1 / 84.4 / 83.5 ms; the reference's walk: 130.4) and keeps
// its per-lane stack in dynamic LDS (depth x 2 KB per workgroup)
template <bool MC, bool HAS_QUADS, bool DEEP, bool RAD0, int WIDE>
__global__ __launch_bounds__(kBlock, WIDE ? PTMI_FF_WIDE_WAVES : 7) void ptmi_form_factors(DeviceScene sc, RadiosityBuffers rb, int n_samples,
                                                            const uint32_t* __restrict__ jump) {
    extern __shared__ uint2 ff_wstack[];
    uint2* wstack = ff_wstack + threadIdx.x;
    __shared__ uint32_t M[160 * 5];
    __shared__ unsigned int counts[kGridSize];
    __shared__ float radg[RAD0 ? 3 * kGridSize : 1];
    __shared__ int2 queue[kQueueCap];
    __shared__ int q_n;
    __shared__ unsigned int rays_wg;
    const int n = rb.n;
    const int i = blockIdx.x;
    const int tid = threadIdx.x;
    const Geom gi = load_geom(rb.geo, i);
    const int slot_i = rb.slot_of[i];
    float* __restrict__ row = rb.form_factors + (size_t)i * (size_t)n;
    counts[tid] = 0u;
    if (RAD0) { radg[3 * tid] = 0.0f; radg[3 * tid + 1] = 0.0f; radg[3 * tid + 2] = 0.0f; }
    if (tid == 0) { q_n = 0; rays_wg = 0u; }
    __syncthreads();
    unsigned int rays = 0u;
    unsigned long long chain = 0ull;              // certified walk: rays that took the ancestor chain (low word) / the reference's walk (high word)

    for (int base = 0; base < n; base += kBlock) {
        const int j = base + tid;
        int samples = 0;                                    // 0: this pair's form factor is already decided (0)
        if (j < n) {
            if (j != i) {
                const float4 cj = rb.geo[6 * j + 5], nj = rb.geo[6 * j + 4];
                if (MC) {                                   // form_factors.h:234-256
                    const f3 dir_ij = xyz(cj) - gi.centroid;
                    const float dist_sq = dir_ij.x * dir_ij.x + dir_ij.y * dir_ij.y + dir_ij.z * dir_ij.z;
                    const float dist = sqrt_rn(dist_sq);
                    if (!(dist < 1e-6f)) {
                        const f3 dir_norm = div_scalar(dir_ij, dist);
                        const float cos_i_approx = dot(gi.normal, dir_norm);
                        const float cos_j_approx = -dot(xyz(nj), dir_norm);
                        if (!(cos_i_approx <= 0.0f || cos_j_approx <= 0.0f)) {
                            const float area_j = rb.geo[6 * j + 1].w;
                            const float approx_ff = (float)((double)(cos_i_approx * cos_j_approx * area_j) / (PTMI_PI_D * (double)dist_sq));
                            samples = n_samples;
                            if (approx_ff < 0.001f) samples = max(1, n_samples / 4);
                            else if (approx_ff < 0.01f) samples = max(2, n_samples / 2);
                        }
                    }
                } else {                                    // form_factors.h:385-401
                    const f3 vec_ij = xyz(cj) - gi.centroid;
                    const float r = length(vec_ij);
                    if (!(r < 1e-6f)) {
                        const f3 dir_ij = div_scalar(vec_ij, r);
                        const float cos_theta_i = dot(gi.normal, dir_ij);
                        const float cos_theta_j = dot(xyz(nj), -dir_ij);
                        if (!(cos_theta_i <= 0.0f || cos_theta_j <= 0.0f)) samples = 1;
                    }
                }
            }
            if (samples == 0) row[j] = 0.0f;
        }
        if (samples) { const int pos = atomicAdd(&q_n, 1); queue[pos] = make_int2(j, samples); }
        __syncthreads();
        const bool last = base + kBlock >= n;
        while (q_n >= kBlock || (last && q_n > 0)) {        // q_n is block-uniform between barriers
            const int total = q_n;
            const int take = min(total, kBlock);
            const bool have = tid < take;
            const int2 e = have ? queue[total - take + tid] : make_int2(0, 0);
            __syncthreads();
            if (tid == 0) q_n = total - take;
            Rng rng = {0u, 0u, 0u, 0u, 0u, 0u};
            if (MC) pair_rng_init(M, jump, have, (unsigned int)(i * n + e.x), rng, rb.row_jump ? rb.row_jump + (size_t)i * 160 * 5 : nullptr,
                                  (unsigned int)e.x, i == 0);
            if (have) {
                const int slot_j = rb.slot_of[e.x];
                float F;
                if (MC) F = mc_pair<HAS_QUADS, DEEP, RAD0, WIDE>(sc, wstack, i, gi, rb.geo, e.x, slot_i, slot_j, e.y, rng, xyz(rb.radiosity[e.x]), counts, radg, rays, chain);
                else F = p2p_pair<HAS_QUADS, DEEP, WIDE>(sc, wstack, i, e.x, gi, load_geom(rb.geo, e.x), slot_i, slot_j, rays, chain);
                row[e.x] = F;
            }
            __syncthreads();
        }
    }
    atomicAdd(&rays_wg, rays);
    __syncthreads();
    rb.grid[(size_t)i * kGridSize + tid] = counts[tid];     // initialize_directional_grids + the kernel's atomics, in one store
    rb.rad_grid[(size_t)i * kGridSize + tid] = RAD0 ? make_float4(radg[3 * tid], radg[3 * tid + 1], radg[3 * tid + 2], 0.0f)
                                                    : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (tid == 0 && rb.rays) atomicAdd(rb.rays, (unsigned long long)rays_wg);
    if (WIDE == 2 && rb.rays) {                    // one pair of atomics per wave (the two 32-bit words cannot carry into each other: a lane's rays stay far below 2^32)
        unsigned long long c = chain;
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
        if ((threadIdx.x & 63) == 0 && c) { atomicAdd(rb.rays + 1, c & 0xffffffffull); atomicAdd(rb.rays + 2, c >> 32); }
    }
}

}  // namespace

// The kernel for (Monte-Carlo, quads, deep tree, num_iterations == 0) and the walk that RadiosityState::runSolver chose in
// rb.fast_tree: 1 the opt-in fast tree, no certificate; 2 the certified walk - the reference's answers, through the fast tree.
// A walk whose records are missing, and every walk over a deep tree, is the reference's own (0).
void launch_form_factors(const DeviceScene& sc, const RadiosityBuffers& rb, const RadiosityParams& prm, const uint32_t* d_jump, hipStream_t s) {
    if (rb.n <= 0) return;
    const dim3 grid(rb.n);
    const bool mc = prm.use_monte_carlo != 0, quads = sc.has_quads != 0, deep = rb.bvh_depth > 30, rad0 = mc && prm.num_iterations == 0;
    if (mc && rb.row_jump) hipLaunchKernelGGL(ptmi_ff_row_jumps, grid, dim3(kBlock), 0, s, rb.row_jump, rb.n, d_jump);
    const bool records = quads ? sc.wqprims != nullptr : sc.wprims != nullptr;
    const int walk = deep ? 0 : rb.fast_tree == 1 && sc.wnodes && records ? 1 : rb.fast_tree == 2 && records && sc.certified_ready() ? 2 : 0;
    const size_t lds = walk ? (size_t)sc.w_depth * kBlock * sizeof(uint2) : 0;     // the fast tree's per-lane stack
    const auto launch = [&](auto wide) {
        with_bool(mc, [&](auto mc_) {
            with_bool(quads, [&](auto quads_) {
                with_bool(deep, [&](auto deep_) {
                    with_bool(rad0, [&](auto rad0_) {
                        constexpr bool MC = decltype(mc_)::value, DEEP = decltype(deep_)::value, RAD0 = decltype(rad0_)::value;
                        constexpr int WIDE = decltype(wide)::value;
                        if constexpr (!(DEEP && WIDE) && !(RAD0 && !MC))      // what cannot occur is not compiled
                            hipLaunchKernelGGL((ptmi_form_factors<MC, decltype(quads_)::value, DEEP, RAD0, WIDE>), grid, dim3(kBlock), lds, s, sc, rb,
                                               mc ? prm.mc_samples : 0, d_jump);
                    });
                });
            });
        });
    };
    if (walk == 1) launch(std::integral_constant<int, 1>{});
    else if (walk == 2) launch(std::integral_constant<int, 2>{});
    else launch(std::integral_constant<int, 0>{});
}

}  // namespace ptmi
