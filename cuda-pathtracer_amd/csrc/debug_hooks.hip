// debug_hooks.hip — the test hooks: the render kernels' own device functions (traversal.h, shading.h, light_sample.h, rough.h),
// one call per case.  Compile with -ffp-contract=off (kernels.hip).
#include "bounce.h"
#include "light_sample.h"
#include "vertex_normal.h"
#include "albedo_texture.h"
#include "lens.h"
#include "medium.h"
#include "../../include/ptmi.h"      // PTMI_MATH_*

namespace ptmi {

// ---------------------------------------------------------------------------------------------
// test hooks
// ---------------------------------------------------------------------------------------------
template <int MODE, bool HAS_QUADS>
__global__ __launch_bounds__(kBlock) void ptmi_debug_intersect_k(DeviceScene sc, int n, const float* o, const float* d, float t_min,
                                                                 float t_max, int* hit, int* prim, float* t_out, float* p_out, float* n_out) {
    extern __shared__ float4 smem[];
    int* stack = reinterpret_cast<int*>(smem) + threadIdx.x;
    // SWEEP walks the records ptmi_bounce's sweep walks, in the timed build's form: staged by the same stage_scene (LANE and STACK
    // read global memory here)
    const float4 *nodes, *prims, *mats;
    SweepLeaves leaves;
    stage_scene<MODE == TRAVERSAL_SWEEP, MODE == TRAVERSAL_SWEEP, MODE == TRAVERSAL_SWEEP ? sweep_form<HAS_QUADS, false, false>() : 0>(sc, smem, nodes, prims, mats, nullptr, nullptr, leaves);
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    const int j = live ? i : 0;
    const f3 ro = mk3(o[3 * j], o[3 * j + 1], o[3 * j + 2]), rd = mk3(d[3 * j], d[3 * j + 1], d[3 * j + 2]);
    LaneCounters cn = {0, 0, 0, 0, 0, 0, 0};
    float t = 0.0f; int k = -1;
    const bool h = scene_intersect<MODE, HAS_QUADS, false>(nodes, prims, sc.prim_stride, sc.n_nodes, stack, live, ro, rd, t_min, t_max, t, k, cn, leaves);
    if (!live) return;
    hit[i] = h ? 1 : 0;
    prim[i] = h ? __float_as_int(sc.mats[3 * k].w) : -1;
    t_out[i] = h ? t : 0.0f;
    const f3 p = h ? ro + t * rd : mk3(0, 0, 0);
    const f3 nn = h ? xyz(sc.mats[3 * k]) : mk3(0, 0, 0);
    p_out[3 * i] = p.x; p_out[3 * i + 1] = p.y; p_out[3 * i + 2] = p.z;
    n_out[3 * i] = nn.x; n_out[3 * i + 1] = nn.y; n_out[3 * i + 2] = nn.z;
}

void launch_debug_intersect(const DeviceScene& sc, int n, const float* o, const float* d, float t_min, float t_max,
                            int* hit, int* prim, float* t, float* p, float* nrm, hipStream_t s) {
    if (n <= 0) return;
    const dim3 grid((n + kBlock - 1) / kBlock), block(kBlock);
    // the sweep stages the scene as ptmi_bounce does (bounce_lds_bytes counts it); the other walks need their stacks only
    const size_t lds = sc.traversal == TRAVERSAL_SWEEP ? bounce_lds_bytes(sc) : (size_t)sc.stack_entries * kBlock * sizeof(int);
    const int walk =sc.traversal == TRAVERSAL_PHASED || sc.traversal == TRAVERSAL_PACKED || sc.traversal == TRAVERSAL_CERTIFIED ? TRAVERSAL_LANE : sc.traversal;   // the phased kernels walk like LANE
    const auto launch = [&](auto mode) {
        with_bool(sc.has_quads, [&](auto quads) {
            hipLaunchKernelGGL((ptmi_debug_intersect_k<decltype(mode)::value, decltype(quads)::value>), grid, block, lds, s, sc, n, o, d, t_min, t_max, hit, prim, t, p, nrm);
        });
    };
    if (walk == TRAVERSAL_SWEEP) launch(std::integral_constant<int, TRAVERSAL_SWEEP>{});
    else if (walk == TRAVERSAL_LANE) launch(std::integral_constant<int, TRAVERSAL_LANE>{});
    else launch(std::integral_constant<int, TRAVERSAL_STACK>{});
}

// Closest hit through the fast tree for n rays (test hook): wide_closest_hit, the walk of the Radiosity view and the features
template <bool QUADS>
__global__ __launch_bounds__(kBlock) void ptmi_debug_intersect_wide_k(DeviceScene sc, int n, const float* o, const float* d, float t_min,
                                                                      float t_max, int* hit, int* prim, float* t_out,
                                                                      unsigned long long* counts /* [0] node visits [1] triangle tests */) {
    extern __shared__ float4 smem[];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const f3 ro = mk3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    float closest_t = t_max;
    bool tie = false;
    WideCounts wc = {0, 0};
    const int slot_hit = wide_closest_hit<QUADS, true>(sc, reinterpret_cast<uint2*>(smem) + threadIdx.x, ro, rd, t_min, closest_t, tie, wc);
    hit[i] = slot_hit >= 0 ? 1 : 0;
    prim[i] = slot_hit >= 0 ? sc.wload_index[slot_hit] : -1;
    t_out[i] = slot_hit >= 0 ? closest_t : 0.0f;
    if (counts) { atomicAdd(&counts[0], (unsigned long long)wc.node_visits); atomicAdd(&counts[1], (unsigned long long)wc.prim_tests); }
}
void launch_debug_intersect_wide(const DeviceScene& sc, int n, const float* o, const float* d, float t_min, float t_max,
                                 int* hit, int* prim, float* t, unsigned long long* counts, hipStream_t s) {
    if (n <= 0) return;
    const size_t lds = (size_t)sc.w_depth * kBlock * sizeof(uint2);
    const dim3 grid((n + kBlock - 1) / kBlock), block(kBlock);
    with_bool(sc.has_quads, [&](auto quads) {
        hipLaunchKernelGGL(ptmi_debug_intersect_wide_k<decltype(quads)::value>, grid, block, lds, s, sc, n, o, d, t_min, t_max, hit, prim, t, counts);
    });
}

// first_hit (traversal.h) for n rays (test hook): the walk of the Radiosity view and the feature pass in the scene's own mode -
// the certified walk where the scene has it, else LANE or STACK - chosen and given its LDS by first_hit_walk as theirs is.  The
// reference's leaf-order slot becomes the load index.
template <int MODE, bool HAS_QUADS>
__global__ __launch_bounds__(kBlock) void ptmi_debug_first_hit_k(DeviceScene sc, int n, const float* o, const float* d, float t_min,
                                                                 int* hit, int* prim, float* t_out) {
    extern __shared__ float4 smem[];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    const int j = live ? i : 0;
    const f3 ro = mk3(o[3 * j], o[3 * j + 1], o[3 * j + 2]), rd = mk3(d[3 * j], d[3 * j + 1], d[3 * j + 2]);
    LaneCounters cn = {0, 0, 0, 0, 0, 0, 0};
    float t = 0.0f; int k = -1;
    const bool h = first_hit<MODE, HAS_QUADS>(sc, smem, live, ro, rd, t_min, t, k, cn);
    if (!live) return;
    hit[i] = h ? 1 : 0;
    prim[i] = h ? __float_as_int(sc.mats[3 * k].w) : -1;
    t_out[i] = h ? t : 0.0f;
}
void launch_debug_first_hit(const DeviceScene& sc, int n, const float* o, const float* d, float t_min, int* hit, int* prim, float* t, hipStream_t s) {
    if (n <= 0) return;
    first_hit_walk(sc, [&](auto mode, auto quads, size_t lds) {
        hipLaunchKernelGGL((ptmi_debug_first_hit_k<decltype(mode)::value, decltype(quads)::value>), dim3((n + kBlock - 1) / kBlock), dim3(kBlock), lds, s,
                           sc, n, o, d, t_min, hit, prim, t);
    });
}

__global__ void ptmi_debug_rng_k(const uint32_t* __restrict__ jump, unsigned long long seed_base, int n_pixels,
                                 const int* pixels, int count, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const unsigned int pix = (unsigned int)pixels[i];
    const unsigned long long seed = seed_base + (unsigned long long)pix;
    const uint32_t s0 = ((uint32_t)seed) ^ 0xaad26b49u, s1 = (uint32_t)(seed >> 32) ^ 0xf7dcefddu;
    const uint32_t t0 = 1099087573u * s0, t1 = 2591861531u * s1;
    uint32_t v[5] = {123456789u + t0, 362436069u ^ t0, 521288629u + t1, 88675123u ^ t1, 5783321u + t0};
    for (int k = 0; k < 32; k++) {
        if (!((pix >> k) & 1u)) continue;
        uint32_t r[5] = {0, 0, 0, 0, 0};
        for (int w = 0; w < 5; w++)
            for (int b = 0; b < 32; b++)
                if ((v[w] >> b) & 1u) for (int c = 0; c < 5; c++) r[c] ^= jump[(k * 160 + w * 32 + b) * 5 + c];
        for (int w = 0; w < 5; w++) v[w] = r[w];
    }
    Rng rng = {v[0], v[1], v[2], v[3], v[4], 6615241u + t1 + t0};
    for (int c = 0; c < count; c++) out[(size_t)i * count + c] = rng_uniform(rng);
}

void launch_debug_rng(const uint32_t* d_jump, uint64_t seed_base, int n_pixels, const int* pixels, int count, float* out, hipStream_t s) {
    if (n_pixels <= 0) return;
    hipLaunchKernelGGL(ptmi_debug_rng_k, dim3((n_pixels + 63) / 64), dim3(64), 0, s, d_jump, (unsigned long long)seed_base,
                       n_pixels, pixels, count, out);
}

// exhaustive check of rcp_exact_normal against the IEEE quotient over a range of bit patterns
__global__ void ptmi_debug_rcp_k(unsigned int first, unsigned long long count, unsigned long long* out /* [0]=mismatches [1]=first bad bits+1 */) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long bad = 0, first_bad = ~0ull;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < count; i += stride) {
        const unsigned int bits = first + (unsigned int)i;
        const float a = __uint_as_float(bits);
        const float want = 1.0f / a, got = rcp_exact_normal(a);
        if (__float_as_uint(want) != __float_as_uint(got) && !(want != want && got != got)) { bad++; if (first_bad == ~0ull) first_bad = bits; }
    }
    if (bad) { atomicAdd(&out[0], bad); atomicMin(&out[1], first_bad); }
}
void launch_debug_rcp(unsigned int first, unsigned long long count, unsigned long long* d_out, hipStream_t s) {
    hipLaunchKernelGGL(ptmi_debug_rcp_k, dim3(4096), dim3(256), 0, s, first, count, d_out);
}

// the same for sqrt_lean against sqrt_rn
__global__ void ptmi_debug_sqrt_k(unsigned int first, unsigned long long count, unsigned long long* out /* [0]=mismatches [1]=first bad bits */) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long bad = 0, first_bad = ~0ull;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < count; i += stride) {
        const unsigned int bits = first + (unsigned int)i;
        const float a = __uint_as_float(bits);
        const float want = sqrt_rn(a), got = sqrt_lean(a);
        if (__float_as_uint(want) != __float_as_uint(got) && !(want != want && got != got)) { bad++; if (first_bad == ~0ull) first_bad = bits; }
    }
    if (bad) { atomicAdd(&out[0], bad); atomicMin(&out[1], first_bad); }
}
void launch_debug_sqrt(unsigned int first, unsigned long long count, unsigned long long* d_out, hipStream_t s) {
    hipLaunchKernelGGL(ptmi_debug_sqrt_k, dim3(4096), dim3(256), 0, s, first, count, d_out);
}

// ray_inv, the walks' 1 / d behind its wave vote: case i is lane i & 63 of wave i / 64 (one wave per workgroup), so the caller
// chooses which directions vote together.  A lane past n rides along as a dead one.
__global__ __launch_bounds__(64) void ptmi_debug_ray_inv_k(int n, const float* __restrict__ d, const int* __restrict__ live, float* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool in = i < n;
    const f3 dir = in ? mk3(d[3 * i], d[3 * i + 1], d[3 * i + 2]) : mk3(0.0f, 0.0f, 0.0f);
    const f3 inv = ray_inv(dir, in && live[i] != 0);
    if (in) { out[3 * i] = inv.x; out[3 * i + 1] = inv.y; out[3 * i + 2] = inv.z; }
}
void launch_debug_ray_inv(int n, const float* d, const int* live, float* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_debug_ray_inv_k, dim3((n + 63) / 64), dim3(64), 0, s, n, d, live, out);
}

// sincos_2pi_lean, the cosine sample's sincos behind its wave vote, against ptmi_sincosf over a range of bit patterns.
// out: [0] patterns whose sin differs, [1] whose cos differs, [2] the first such pattern, [3] lanes that raised the flag,
// [4..4+kLeanFlaggedKept) the first flagged patterns that were recorded (in no order).  A pattern counts as different if the voted
// result differs, or if it is not flagged and the short form itself differs (its wave may have gone the long way for a neighbour).
constexpr int kLeanFlaggedKept = 8;
__global__ void ptmi_debug_sincos_lean_check_k(unsigned int first, unsigned long long count, unsigned long long* out) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long bad_s = 0, bad_c = 0, first_bad = ~0ull, flagged = 0;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < count; i += stride) {
        const unsigned int bits = first + (unsigned int)i;
        const float x = __uint_as_float(bits);
        float ws, wc, s, c, fs, fc;
        ptmi_sincosf(x, &ws, &wc);
        sincos_2pi_lean(x, &s, &c);
        const bool flag = ptmi_sincos_2pi_fast(x, &fs, &fc) != 0;
        const bool in_domain = bits <= PTMI_TWO_PI_F_BITS;
        const bool ds = __float_as_uint(s) != __float_as_uint(ws) || (in_domain && !flag && __float_as_uint(fs) != __float_as_uint(ws));
        const bool dc = __float_as_uint(c) != __float_as_uint(wc) || (in_domain && !flag && __float_as_uint(fc) != __float_as_uint(wc));
        bad_s += ds; bad_c += dc;
        if ((ds || dc) && first_bad == ~0ull) first_bad = bits;
        if (in_domain && flag) {
            if (flagged == 0) {
                const unsigned long long at = atomicAdd(&out[4 + kLeanFlaggedKept], 1ull);
                if (at < (unsigned long long)kLeanFlaggedKept) out[4 + at] = bits;
            }
            flagged++;
        }
    }
    if (bad_s) atomicAdd(&out[0], bad_s);
    if (bad_c) atomicAdd(&out[1], bad_c);
    if (first_bad != ~0ull) atomicMin(&out[2], first_bad);
    if (flagged) atomicAdd(&out[3], flagged);
}
void launch_debug_sincos_lean_check(unsigned int first, unsigned long long count, unsigned long long* d_out, hipStream_t s) {
    hipLaunchKernelGGL(ptmi_debug_sincos_lean_check_k, dim3(4096), dim3(256), 0, s, first, count, d_out);
}

// sincos_2pi_lean per wave: case i is lane i & 63 of wave i / 64 (one wave per workgroup), as ptmi_debug_ray_inv_k; a case with
// live[i] == 0 is a lane that is not active at the call.  out: 4 per case - the voted sin and cos, then ptmi_sincosf's.
__global__ __launch_bounds__(64) void ptmi_debug_sincos_lean_k(int n, const float* __restrict__ x, const int* __restrict__ live, float* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n || live[i] == 0) return;
    float s, c, ws, wc;
    sincos_2pi_lean(x[i], &s, &c);
    ptmi_sincosf(x[i], &ws, &wc);
    out[4 * i] = s; out[4 * i + 1] = c; out[4 * i + 2] = ws; out[4 * i + 3] = wc;
}
void launch_debug_sincos_lean(int n, const float* x, const int* live, float* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_debug_sincos_lean_k, dim3((n + 63) / 64), dim3(64), 0, s, n, x, live, out);
}

// div_by_size, the pixel jitter's division by an image size W with the reciprocal inv the host took for it (0: the IEEE division),
// against a / W over a range of bit patterns of a.  W and inv are kernel arguments, as TileMap's are.
__global__ void ptmi_debug_size_div_k(float W, float inv, unsigned int first, unsigned long long count, unsigned long long* out /* [0]=mismatches [1]=first bad bits */) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long bad = 0, first_bad = ~0ull;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < count; i += stride) {
        const unsigned int bits = first + (unsigned int)i;
        const float a = __uint_as_float(bits);
        const float want = a / W, got = div_by_size(a, W, inv);
        if (__float_as_uint(want) != __float_as_uint(got) && !(want != want && got != got)) { bad++; if (first_bad == ~0ull) first_bad = bits; }
    }
    if (bad) { atomicAdd(&out[0], bad); atomicMin(&out[1], first_bad); }
}
void launch_debug_size_div(float W, float inv, unsigned int first, unsigned long long count, unsigned long long* d_out, hipStream_t s) {
    hipLaunchKernelGGL(ptmi_debug_size_div_k, dim3(4096), dim3(256), 0, s, W, inv, first, count, d_out);
}

// unit_vector_voted, the Ray constructor's normalisation behind its wave vote, laid out as ptmi_debug_sincos_lean_k.
// out: 6 per case - the voted vector, then unit_vector's.
__global__ __launch_bounds__(64) void ptmi_debug_unit_voted_k(int n, const float* __restrict__ w, const int* __restrict__ live, float* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n || live[i] == 0) return;
    const f3 v = mk3(w[3 * i], w[3 * i + 1], w[3 * i + 2]);
    const f3 got = unit_vector_voted(v), want = unit_vector(v);
    out[6 * i] = got.x; out[6 * i + 1] = got.y; out[6 * i + 2] = got.z;
    out[6 * i + 3] = want.x; out[6 * i + 4] = want.y; out[6 * i + 5] = want.z;
}
void launch_debug_unit_voted(int n, const float* w, const int* live, float* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_debug_unit_voted_k, dim3((n + 63) / 64), dim3(64), 0, s, n, w, live, out);
}

// cosine_hemisphere with explicit (u, v), in its LEAN form: the sweep kernel's, with the voted sincos (tests/test_gpu_parity.py
// holds it to the oracle).  The form without LEAN, which every other kernel keeps, is op 0 of ptmi_debug_guided_k below
// (tests/test_gpu_integrator_vs_ref.py).
__global__ void ptmi_debug_cosine_k(int n, const float* normals, const float* u, const float* v, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f3 r = cosine_hemisphere<true>(mk3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]), u[i], v[i]);
    out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
}

void launch_debug_cosine(int n, const float* normals, const float* u, const float* v, float* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_debug_cosine_k, dim3((n + 255) / 256), dim3(256), 0, s, n, normals, u, v, out);
}

// Guided sampling per call (test hook): the bounce kernels' own cosine_hemisphere, grid_sample, grid_compute_pdf, sample_mis,
// mis_power_heuristic and resolve_pixel on n cases, each drawing from its own XORWOW state (6 words: v0..v4, d).  The tests
// pass states whose next raw outputs are scripted words and d = 0, so used[i] = d / 362437 counts the draws a call made.
//   op 0 cosine_hemisphere(normal, u, v), u and v drawn as integrator.h:63-64 draws them   -> out[0..2] direction
//   op 1 grid_sample(record, normal)                                                      -> direction, out[3] pdf
//   op 2 grid_compute_pdf(record, dir = in3, normal)                                      -> out[3] pdf
//   op 3 sample_mis(record, normal, bsdf_prob = in3[0])                                   -> direction, out[3] weight
//   op 4 mis_power_heuristic(in3[0], in3[1])                                              -> out[3]
//   op 5 resolve_pixel(colour = in3, k = 1)                                               -> out[0..2] rgb8, out[3..5] radiance
// recs: records of kCdfDwords words, rec_idx[i] picks case i's (ops 1-3 only; the host checks the indices).  out: 6 per case.
__global__ __launch_bounds__(kBlock) void ptmi_debug_guided_k(int n, int op, const float* __restrict__ recs, const int* __restrict__ rec_idx,
                                                              const float* __restrict__ normals, const float* __restrict__ in3,
                                                              const uint32_t* __restrict__ states, float* __restrict__ out,
                                                              int* __restrict__ used) {
    fill_grid_solid_angles();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t* s = states + (size_t)i * 6;
    Rng rng = {s[0], s[1], s[2], s[3], s[4], s[5]};
    const f3 nrm = mk3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
    const f3 a = mk3(in3[3 * i], in3[3 * i + 1], in3[3 * i + 2]);
    const float* g = (op >= 1 && op <= 3) ? recs + (size_t)rec_idx[i] * kCdfDwords : nullptr;
    float r[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    f3 dir = mk3(0.0f, 0.0f, 0.0f);
    if (op == 0) {
        const float u = rng_uniform(rng);
        const float v = rng_uniform(rng);
        dir = cosine_hemisphere(nrm, u, v);
    } else if (op == 1) {
        dir = grid_sample(g, nrm, rng, r[3]);
    } else if (op == 2) {
        r[3] = grid_compute_pdf(g, a, nrm);
    } else if (op == 3) {
        dir = sample_mis(g, nrm, rng, r[3], a.x);
    } else if (op == 4) {
        r[3] = mis_power_heuristic(a.x, a.y);
    } else if (op == 5) {
        unsigned char rgb[3];
        resolve_pixel(make_float4(a.x, a.y, a.z, 0.0f), 1.0f, 0, rgb, &r[3]);
        dir = mk3((float)rgb[0], (float)rgb[1], (float)rgb[2]);
    }
    r[0] = dir.x; r[1] = dir.y; r[2] = dir.z;
    for (int c = 0; c < 6; c++) out[(size_t)i * 6 + c] = r[c];
    used[i] = (int)(rng.d / 362437u);
}

void launch_debug_guided(int n, int op, const float* recs, const int* rec_idx, const float* normals, const float* in3,
                         const uint32_t* states, float* out, int* used, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_debug_guided_k, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n, op, recs, rec_idx, normals, in3,
                       states, out, used);
}

// The numerics contract per call (test hook): include/ptmi_math.h's device build and the IEEE primitives the kernels rely on,
// one operation on n cases (a[i], b[i]); two doubles per case, float and int results promoted (exact).  op: PTMI_MATH_*.
__global__ void ptmi_debug_math_k(int n, int op, const float* __restrict__ a_in, const float* __restrict__ b_in, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float a = a_in[i], b = b_in[i];
    double r0 = 0.0, r1 = 0.0;
    float f0 = 0.0f, f1 = 0.0f;
    switch (op) {
        case PTMI_MATH_SINCOS_D: ptmi_sincos_d((double)a, &r0, &r1); break;
        case PTMI_MATH_TAN_D:    r0 = ptmi_tan_d((double)a); break;
        case PTMI_MATH_LOG_D:    r0 = ptmi_log_d((double)a); break;
        case PTMI_MATH_EXP_D:    r0 = ptmi_exp_d((double)a); break;
        case PTMI_MATH_ATAN2_D:  r0 = ptmi_atan2_d((double)a, (double)b); break;
        case PTMI_MATH_SINCOSF:  ptmi_sincosf(a, &f0, &f1); r0 = (double)f0; r1 = (double)f1; break;
        case PTMI_MATH_POWF:     r0 = (double)ptmi_powf(a, b); break;
        case PTMI_MATH_EXPF:     r0 = (double)ptmi_expf(a); break;
        case PTMI_MATH_ATAN2F:   r0 = (double)ptmi_atan2f(a, b); break;
        case PTMI_MATH_ACOSF:    r0 = (double)ptmi_acosf(a); break;
        case PTMI_MATH_DIV:      r0 = (double)(a / b); break;
        case PTMI_MATH_RCP:      r0 = (double)rcp_rn(a); break;
        case PTMI_MATH_SQRT:     r0 = (double)sqrt_rn(a); break;
        case PTMI_MATH_ROUND:    r0 = (double)(float)((double)a * (double)b); break;
        case PTMI_MATH_TRUNC:    r0 = (double)(int)a; r1 = (double)(int)(double)a; break;
        default: break;
    }
    out[2 * (size_t)i] = r0; out[2 * (size_t)i + 1] = r1;
}
void launch_debug_math(int n, int op, const float* a, const float* b, double* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_debug_math_k, dim3((n + 255) / 256), dim3(256), 0, s, n, op, a, b, out);
}

// direction_to_grid_index_local (pt_device.h), the form-factor kernel's binning, on n (direction, normal) pairs
__global__ void ptmi_debug_grid_index_k(int n, const float* __restrict__ dirs, const float* __restrict__ normals, int* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = direction_to_grid_index_local(mk3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]),
                                           mk3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]));
}
void launch_debug_grid_index(int n, const float* dirs, const float* normals, int* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_debug_grid_index_k, dim3((n + 255) / 256), dim3(256), 0, s, n, dirs, normals, out);
}

// The light and surface sampling functions of ptmi_render_nee per call (test hook; include/ptmi.h: ptmi_debug_nee_call states
// each op's inputs and outputs): light_sample.h and rough.h on n cases against the context's own tables - em the loaded scene's
// emitters, ev the environment as a frame with next_event set sees it (ev.q, ev.sampled).  in: kNeeCallIn floats per case;
// out_f: kNeeCallOutF floats and out_i: kNeeCallOutI ints per case, zero where an op writes nothing.  An output a function
// leaves undefined after a false verdict stays zero.
template <bool HAS_QUADS>
__global__ __launch_bounds__(kBlock) void ptmi_debug_nee_call_k(int n, int op, EmitterTable em, EnvTable ev, const float* __restrict__ in,
                                                                float* __restrict__ out_f, int* __restrict__ out_i) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float* a = in + (size_t)i * kNeeCallIn;
    float f[kNeeCallOutF];
    int k[kNeeCallOutI];
    for (int c = 0; c < kNeeCallOutF; c++) f[c] = 0.0f;
    for (int c = 0; c < kNeeCallOutI; c++) k[c] = 0;
    const auto put3 = [&](int at, const f3& v) { f[at] = v.x; f[at + 1] = v.y; f[at + 2] = v.z; };
    if (op == PTMI_NEE_CALL_ENV_LOOKUP) {
        const int t = env_texel(ev, mk3(a[0], a[1], a[2]));
        const float4 te = ev.texel[t];
        k[0] = t / ev.w; k[1] = t - k[0] * ev.w;
        f[0] = te.x; f[1] = te.y; f[2] = te.z; f[3] = te.w;
    } else if (op == PTMI_NEE_CALL_ENV_SAMPLE) {
        f3 wi;
        const float4 te = env_sample(ev, a[0], a[1], a[2], a[3], k[0], k[1], wi);
        put3(0, wi);
        f[3] = te.w; f[4] = te.x; f[5] = te.y; f[6] = te.z;
    } else if (op == PTMI_NEE_CALL_EMITTER_SAMPLE) {
        const bool env_on = ev.texel != nullptr && ev.sampled != 0;  // ptmi_render_nee's env_on, q and omq
        const float q = ev.texel != nullptr ? ev.q : 0.0f, omq = 1.0f - q;
        const EmitterSample e = emitter_sample<HAS_QUADS>(em, a[0], a[1], a[2], mk3(a[3], a[4], a[5]), env_on, omq);
        k[0] = e.index; k[1] = e.slot; k[2] = e.ok ? 1 : 0;
        put3(0, e.wi);
        f[3] = e.dist2; f[4] = e.cos_l; f[5] = e.p_area; f[6] = e.p_l;
    } else if (op == PTMI_NEE_CALL_SPECULAR) {
        const f3 d = mk3(a[0], a[1], a[2]), nrm = mk3(a[3], a[4], a[5]);
        const f3 sn = dot(d, nrm) < 0 ? nrm : -nrm;                   // integrator.h:221-222, as the kernel turns it
        bool reflect; float fr; f3 next;
        const bool walk = specular_vertex(d, nrm, sn, (int)a[6], a[7], a[8], reflect, fr, next);
        k[0] = reflect ? 1 : 0; k[1] = walk ? 1 : 0;
        f[0] = fr;
        put3(1, next);
        put3(4, unit_vector(next));
    } else {                                                          // the rough ops: a vertex of (sn, d, alpha) first
        const bool lw = op == PTMI_NEE_CALL_LIGHT_WEIGHT;
        const float* b = lw ? a + 1 : a;
        const RoughVertex v = rough_vertex(mk3(b[0], b[1], b[2]), mk3(b[3], b[4], b[5]), b[6]);
        if (op == PTMI_NEE_CALL_ROUGH_VERTEX) {
            k[0] = v.ok ? 1 : 0;
            put3(0, v.un); put3(3, v.T); put3(6, v.B); put3(9, v.wo);
            f[12] = v.lo;
        } else if (op == PTMI_NEE_CALL_ROUGH_EVAL) {
            float g = 0.0f, p_b = 0.0f;
            k[0] = rough_eval(v, mk3(b[7], b[8], b[9]), g, p_b) ? 1 : 0;
            f[0] = g; f[1] = p_b;
        } else if (op == PTMI_NEE_CALL_ROUGH_SAMPLE) {
            f3 next = mk3(0.0f, 0.0f, 0.0f);
            float wgt = 0.0f, p_b = 0.0f;
            k[0] = v.ok && rough_sample(v, b[7], b[8], next, wgt, p_b) ? 1 : 0;   // as the kernel calls it: the grazing exit first
            put3(0, next);
            f[3] = wgt; f[4] = p_b;
        } else {                                                      // PTMI_NEE_CALL_LIGHT_WEIGHT
            const bool rough = a[0] != 0.0f;
            const f3 wi = mk3(b[7], b[8], b[9]);
            float w0 = 0.0f, w2 = 0.0f;
            k[0] = light_weight<0>(rough, v, wi, b[10], b[11], w0) ? 1 : 0;
            k[1] = light_weight<2>(rough, v, wi, b[10], b[11], w2) ? 1 : 0;
            f[0] = w0; f[1] = w2;
        }
    }
    for (int c = 0; c < kNeeCallOutF; c++) out_f[(size_t)i * kNeeCallOutF + c] = f[c];
    for (int c = 0; c < kNeeCallOutI; c++) out_i[(size_t)i * kNeeCallOutI + c] = k[c];
}
void launch_debug_nee_call(bool has_quads, int n, int op, const EmitterTable& em, const EnvTable& ev, const float* in, float* out_f, int* out_i,
                           hipStream_t s) {
    if (n <= 0) return;
    with_bool(has_quads, [&](auto quads) {
        hipLaunchKernelGGL(ptmi_debug_nee_call_k<decltype(quads)::value>, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n, op, em, ev, in, out_f, out_i);
    });
}

// vertex_normal (vertex_normal.h) as ptmi_render_nee calls it - nrm comes in as the slot's stored normal - on n (leaf-order slot,
// point) cases against the context's own scene and table (test hook; include/ptmi.h: ptmi_debug_vertex_normal)
template <bool HAS_QUADS>
__global__ __launch_bounds__(kBlock) void ptmi_debug_vertex_normal_k(DeviceScene sc, VertexNormalTable vn, int n, const int* __restrict__ slots,
                                                                     const float* __restrict__ p, float* __restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int k = slots[i];
    f3 nrm = xyz(sc.mats[3 * k]);
    const bool smooth = vertex_normal<HAS_QUADS>(sc, vn, k, mk3(p[3 * i], p[3 * i + 1], p[3 * i + 2]), nrm);
    out[4 * i] = nrm.x; out[4 * i + 1] = nrm.y; out[4 * i + 2] = nrm.z; out[4 * i + 3] = smooth ? 1.0f : 0.0f;
}
void launch_debug_vertex_normal(const DeviceScene& sc, const VertexNormalTable& vn, int n, const int* slots, const float* p, float* out, hipStream_t s) {
    if (n <= 0) return;
    with_bool(sc.has_quads != 0, [&](auto quads) {
        hipLaunchKernelGGL(ptmi_debug_vertex_normal_k<decltype(quads)::value>, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, sc, vn, n, slots, p, out);
    });
}

// albedo_at's lookup (albedo_texture.h) as ptmi_render_nee makes it on n (leaf-order slot, point) cases against the context's own
// scene and table (test hook; include/ptmi.h: ptmi_debug_albedo): the wrapped coordinates, T, and 1.0 for a textured slot
template <bool HAS_QUADS>
__global__ __launch_bounds__(kBlock) void ptmi_debug_albedo_k(DeviceScene sc, AlbedoTable at, int n, const int* __restrict__ slots,
                                                              const float* __restrict__ p, float* __restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const AlbedoLookup r = albedo_lookup<HAS_QUADS>(sc, at, slots[i], mk3(p[3 * i], p[3 * i + 1], p[3 * i + 2]));
    f3 one = mk3(1.0f, 1.0f, 1.0f);
    albedo_at<HAS_QUADS>(sc, at, slots[i], mk3(p[3 * i], p[3 * i + 1], p[3 * i + 2]), one);   // the kernel's entry: 1 * T
    out[6 * i] = r.su; out[6 * i + 1] = r.sv;
    out[6 * i + 2] = one.x; out[6 * i + 3] = one.y; out[6 * i + 4] = one.z;
    out[6 * i + 5] = r.textured ? 1.0f : 0.0f;
}
void launch_debug_albedo(const DeviceScene& sc, const AlbedoTable& at, int n, const int* slots, const float* p, float* out, hipStream_t s) {
    if (n <= 0) return;
    with_bool(sc.has_quads != 0, [&](auto quads) {
        hipLaunchKernelGGL(ptmi_debug_albedo_k<decltype(quads)::value>, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, sc, at, n, slots, p, out);
    });
}

// lens_ray_at (lens.h) as ptmi_render_nee calls it, on given uniforms instead of the stream's (test hook; include/ptmi.h:
// ptmi_debug_lens_ray): the origin on the lens, then the unit direction
__global__ __launch_bounds__(kBlock) void ptmi_debug_lens_ray_k(const float4* __restrict__ lens, int n, const int* __restrict__ px, const int* __restrict__ py,
                                                                const float* __restrict__ r, float* __restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    f3 o, d;
    lens_ray_at(lens, px[i], py[i], r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3], o, d);
    out[6 * i] = o.x; out[6 * i + 1] = o.y; out[6 * i + 2] = o.z;
    out[6 * i + 3] = d.x; out[6 * i + 4] = d.y; out[6 * i + 5] = d.z;
}

void launch_debug_lens_ray(const float4* lens, int n, const int* px, const int* py, const float* r, float* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_debug_lens_ray_k, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, lens, n, px, py, r, out);
}

// The functions of medium.h as ptmi_render_nee calls them, once per case (test hook; include/ptmi.h: ptmi_debug_medium_call states
// the layouts).  Each case carries its own block in front of its ray: 20 floats are 80 bytes, so the block stays 16-byte aligned.
__global__ __launch_bounds__(kBlock) void ptmi_debug_medium_call_k(int n, int op, const float* __restrict__ in, float* __restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float* a = in + (size_t)i * kMediumCallIn;
    const float4* medium = reinterpret_cast<const float4*>(a);
    const f3 o = mk3(a[12], a[13], a[14]), d = mk3(a[15], a[16], a[17]);
    const float t_end = a[18], u = a[19], g = a[7];
    float f[kMediumCallOut];
    for (int c = 0; c < kMediumCallOut; c++) f[c] = 0.0f;
    if (op == 0) {
        float t0, t1;
        f[0] = medium_segment(medium, o, d, t_end, t0, t1) ? 1.0f : 0.0f;
        f[1] = t0; f[2] = t1;
        f[3] = medium_transmittance(medium, o, d, t_end);
    } else if (op == 1) {
        float tm;
        f[0] = medium_free_flight(medium, o, d, t_end, u, tm) ? 1.0f : 0.0f;
        const f3 x = o + tm * d;
        f[1] = tm; f[2] = x.x; f[3] = x.y; f[4] = x.z;
    } else if (op == 2) {
        f[0] = hg_value(g, u);
    } else {
        const float c = hg_sample(g, u);
        const f3 nd = hg_direction(d, c, t_end);
        f[0] = c; f[1] = hg_value(g, c); f[2] = nd.x; f[3] = nd.y; f[4] = nd.z;
    }
    for (int c = 0; c < kMediumCallOut; c++) out[(size_t)i * kMediumCallOut + c] = f[c];
}

void launch_debug_medium_call(int n, int op, const float* in, float* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_debug_medium_call_k, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n, op, in, out);
}

}  // namespace ptmi
