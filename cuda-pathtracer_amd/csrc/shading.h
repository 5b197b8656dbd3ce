// shading.h — what a render kernel does between two walks, each defined once: slot <-> pixel, the camera ray, the per-lane path
// registers, the reference's sampling functions (cosine hemisphere, grid, MIS) and shade_step, one iteration of integrator()'s
// depth loop.  Everything is __forceinline__ into the calling kernel.
#pragma once
#include "pt_device.h"
#include "shade_lean.h"
#include "traversal.h"

namespace ptmi {

// slot -> (x, local row).  With tile8 a wave's 64 consecutive slots are an 8x8 pixel tile instead of a 64x1 strip:
// its camera rays span a smaller solid angle and its bounce rays start closer together, so the wave-synchronous
// sweep visits a smaller union of nodes and primitives.  Pure scheduling: results are keyed by the pixel.
__device__ __forceinline__ void slot_to_local(const TileMap& tm, int slot, int& x, int& lr) {
    if (tm.tile8) {
        const int tile = slot >> 6, in = slot & 63;
        const int tiles_per_row = tm.width >> 3;
        const int ty = tile / tiles_per_row, tx = tile - ty * tiles_per_row;
        lr = (ty << 3) + (in >> 3);
        x = (tx << 3) + (in & 7);
    } else {
        lr = slot / tm.width;
        x = slot - lr * tm.width;
    }
}
__device__ __forceinline__ int global_pixel(const TileMap& tm, int slot, int& x, int& y) {
    int lr;
    slot_to_local(tm, slot, x, lr);
    y = ((lr / tm.row_block) * tm.n_ranks + tm.rank) * tm.row_block + (lr % tm.row_block);
    return y * tm.width + x;
}

// ---------------------------------------------------------------------------------------------
// camera (sensor.h:31-33 + ray.h:9-12) and the per-sample jitter (integrator.h:384-385)
// ---------------------------------------------------------------------------------------------
// get_ray(u, v) of the sensor: the ray through (u, v) of the image plane.  camera_dir_raw is its direction before the Ray
// constructor normalises it; shade_step normalises it together with the bounce directions of the lanes that go on.
__device__ __forceinline__ f3 camera_dir_raw(const FrameParams& fp, float u, float v, f3& o) {
    const f3 org = mk3(fp.cam_origin[0], fp.cam_origin[1], fp.cam_origin[2]);
    const f3 llc = mk3(fp.cam_llc[0], fp.cam_llc[1], fp.cam_llc[2]);
    const f3 hor = mk3(fp.cam_hor[0], fp.cam_hor[1], fp.cam_hor[2]);
    const f3 ver = mk3(fp.cam_ver[0], fp.cam_ver[1], fp.cam_ver[2]);
    o = org;
    return llc + u * hor + v * ver - org;
}
// a / W for an image size W.  inv is TileMap's reciprocal of that size (ptmi_size_reciprocal, taken once on the host): where it
// is set (1 <= W <= 2^23) the quotient takes ptmi_div_by_size_lean's three operations - the bits of a / W for a in [2^-33, W],
// shade_lean.h - and where it is 0 the IEEE division.  inv is the same for the whole launch, so this is a scalar branch.
// tests/test_gpu_shade_lean_forms.py::test_division_by_image_size checks every a for sixteen sizes, and a size above 2^23.
// The four-argument form takes the decision from its caller (camera_dir_block: once per launch, in a scalar register); the device
// hook of that test runs through it as well.
__device__ __forceinline__ float div_by_size(float a, float W, float inv, bool lean) {
    if (lean) return ptmi_div_by_size_lean(a, W, inv);
    return a / W;
}
__device__ __forceinline__ float div_by_size(float a, float W, float inv) { return div_by_size(a, W, inv, inv != 0.0f); }
// the per-sample jitter: (x + r1) / width, (y + r2) / height with the two uniforms already drawn; x + r1 lies in [2^-33, width].
// LEAN: div_by_size (shade_step's tail in the kernels that take the short forms); otherwise the IEEE divisions.
template <bool LEAN = false>
__device__ __forceinline__ f3 camera_dir_raw(const FrameParams& fp, const TileMap& tm, int x, int y, float r1, float r2, f3& o) {
    const float u = LEAN ? div_by_size((float)x + r1, (float)tm.width, tm.inv_width) : ((float)x + r1) / (float)tm.width;
    const float v = LEAN ? div_by_size((float)y + r2, (float)tm.height, tm.inv_height) : ((float)y + r2) / (float)tm.height;
    return camera_dir_raw(fp, u, v, o);
}
// The frame block a sweep kernel staged in LDS (frame_block.h, bounce.h: stage_scene) and the two decisions of div_by_size, taken
// once per launch from TileMap's reciprocals: bit 0 width, bit 1 height take the short division.  (bits << 1) != 0 is inv != 0.0f
// for every float, a NaN included, in scalar integer operations: the value stays in a scalar register and the branch on it scalar.
struct FrameBlock {
    const float4* v = nullptr;      // nullptr: a kernel that does not read the block
    int lean_sizes = 0;
};
__device__ __forceinline__ FrameBlock frame_block(const float4* v, const TileMap& tm) {
    int lean_sizes = ((__float_as_uint(tm.inv_width) << 1) != 0u ? 1 : 0) | ((__float_as_uint(tm.inv_height) << 1) != 0u ? 2 : 0);
    lean_sizes = __builtin_amdgcn_readfirstlane(lean_sizes);
    asm("" : "+s"(lean_sizes));      // one scalar register for the length of the kernel, not two kernel arguments fetched again per segment
    return FrameBlock{v, lean_sizes};
}
// camera_dir_raw<true> from the frame block: four broadcast 16-byte LDS reads instead of eighteen scalar kernel arguments, which
// the segment loop of ptmi_bounce<SWEEP> has no registers for (it parked them in vector lanes and fetched them again per segment),
// and every operand of the twelve operations in a vector register.  The same expressions on the same bits.
__device__ __forceinline__ f3 camera_dir_block(const FrameBlock& fb, int x, int y, float r1, float r2, f3& o) {
    const float4 b0 = fb.v[0], b1 = fb.v[1], b2 = fb.v[2], b3 = fb.v[3];      // (llc, W) (hor, 1 / W) (ver, H) (org, 1 / H)
    const float a = (float)x + r1, b = (float)y + r2;
    // read here, not hoisted: in front of the loop the two tests become two 64-bit lane masks, which the loop has no registers for
    int lean_sizes = fb.lean_sizes;
    asm volatile("" : "+s"(lean_sizes));
    const float u = div_by_size(a, b0.w, b1.w, (lean_sizes & 1) != 0);
    const float v = div_by_size(b, b2.w, b3.w, (lean_sizes & 2) != 0);
    o = xyz(b3);
    return xyz(b0) + u * xyz(b1) + v * xyz(b2) - xyz(b3);
}
// IEEE 1 / len: nothing bounds the length of a camera's un-normalised direction
__device__ __forceinline__ void camera_ray_uv(const FrameParams& fp, float u, float v, f3& o, f3& d) {
    d = unit_vector(camera_dir_raw(fp, u, v, o));
}
__device__ __forceinline__ void camera_ray(const FrameParams& fp, const TileMap& tm, int x, int y, Rng& rng, f3& o, f3& d) {
    const float r1 = rng_uniform(rng);
    const float r2 = rng_uniform(rng);
    d = unit_vector(camera_dir_raw(fp, tm, x, y, r1, r2, o));
}

// ptmi_sincosf(phi) of the cosine sample's phi = (float)(2 pi v), per wave.  ptmi_sincos_2pi_fast (shade_lean.h: explicit binary64
// fmas, no quadrant branches, about half of ptmi_sincosf's binary64 operations) gives ptmi_sincosf's bits for every phi in
// [0, (float)(2 pi)] that it does not flag as next to a rounding boundary (255 of the 1 086 918 620 arguments).  ONE vote decides:
// if any active lane is flagged or holds a phi outside that interval - a -0, a negative value, a NaN or anything above; one
// unsigned compare of the bit pattern - the whole wave calls ptmi_sincosf, otherwise every lane keeps the short form's results.
// tests/test_shade_lean_forms_host.py proves the short form on the host and tests/test_gpu_shade_lean_forms.py on the device,
// both over all arguments; the latter pins the vote as well.  The domain compare stands first: outside the domain the short
// form's quadrant comes from a conversion that may be out of range (inf, NaN), and its flag then means nothing and is not read.
__device__ __forceinline__ void sincos_2pi_lean(float phi, float* s, float* c) {
    const bool outside = __float_as_uint(phi) > PTMI_TWO_PI_F_BITS;
    const bool flagged = ptmi_sincos_2pi_fast(phi, s, c) != 0;
    if (__any(outside || flagged)) ptmi_sincosf(phi, s, c);
}

// sampleCosineHemisphere (integrator.h:62-85) with the two uniforms already drawn
//   LEAN: sincos_2pi_lean(phi) for ptmi_sincosf(phi): phi = (float)(2 pi v) with v a curand uniform lies in [0, (float)(2 pi)], and
//     the vote covers the rest.  The same bits either way; the kernels that keep ptmi_sincosf are listed at shade_step.
// The lean forms (pt_vec.h) stand where the operand's range is known; each gives sqrt_rn's / rcp_rn's bits on that range:
//   sqrt_lean(u), sqrt_lean(1 - u): u is a curand uniform, in [2^-33, 1]; 1 - u is 0 or >= 2^-24
//   1 / (1 + n.z): n is the unit normal of a primitive that was hit, and this branch has n.z >= -0.9999999f = -(1 - 2^-23),
//     so 1 + n.z is in [2^-23, 2]
//   the final normalisation: (tangent, bitangent, n) is an orthonormal frame to rounding and x^2 + y^2 + z^2 = u + (1 - u),
//     so the squared length is 1 to a few ulp - far inside [2^-96, 2^100], and its root inside [2^-100, 2^100]
template <bool LEAN = false>
__device__ __forceinline__ f3 cosine_hemisphere(f3 n, float u, float v) {
    const float r = sqrt_lean(u);
    const float phi = (float)((double)2.0f * PTMI_PI_D * (double)v);      // 2.0f * M_PI * v with a double M_PI
    float sphi, cphi;
    if (LEAN) sincos_2pi_lean(phi, &sphi, &cphi);
    else ptmi_sincosf(phi, &sphi, &cphi);
    const float x = r * cphi;
    const float y = r * sphi;
    const float z = sqrt_lean(fmaxf(0.0f, 1.0f - u));
    f3 tangent, bitangent;
    if (n.z < -0.9999999f) {
        tangent = mk3(0.0f, -1.0f, 0.0f);
        bitangent = mk3(-1.0f, 0.0f, 0.0f);
    } else {
        const float a = rcp_exact_normal(1.0f + n.z);
        const float b = -n.x * n.y * a;
        tangent = mk3(1.0f - n.x * n.x * a, b, -n.x);
        bitangent = mk3(b, 1.0f - n.y * n.y * a, -n.y);
    }
    return unit_vector_lean(x * tangent + y * bitangent + z * n);
}

// Per-lane path registers (the 88-byte HBM record, unpacked).
struct PathRegs {
    f3 o, d, tp, L, color;
    Rng rng;
    unsigned int sample_idx;
    int depth, px, py;
};

__device__ __forceinline__ void load_path(const PathState& st, const TileMap& tm, int slot, PathRegs& p) {
    const float4 A = st.A[slot], B = st.B[slot], C = st.C[slot], D = st.D[slot];
    const uint4 E = st.E[slot]; const uint2 F = st.F[slot];
    p.o = xyz(A); p.d = xyz(B); p.L = xyz(C); p.color = xyz(D);
    p.tp = mk3(A.w, B.w, C.w);
    const unsigned int meta = __float_as_uint(D.w);
    p.sample_idx = meta >> 8; p.depth = (int)(meta & 0xffu);
    p.rng = Rng{E.x, E.y, E.z, E.w, F.x, F.y};
    global_pixel(tm, slot, p.px, p.py);
}
__device__ __forceinline__ void store_path(const PathState& st, int slot, const PathRegs& p) {
    st.A[slot] = make_float4(p.o.x, p.o.y, p.o.z, p.tp.x);
    st.B[slot] = make_float4(p.d.x, p.d.y, p.d.z, p.tp.y);
    st.C[slot] = make_float4(p.L.x, p.L.y, p.L.z, p.tp.z);
    st.D[slot] = make_float4(p.color.x, p.color.y, p.color.z, __uint_as_float((p.sample_idx << 8) | (unsigned int)p.depth));
    st.E[slot] = make_uint4(p.rng.v0, p.rng.v1, p.rng.v2, p.rng.v3);
    st.F[slot] = make_uint2(p.rng.v4, p.rng.d);
}

// ---------------------------------------------------------------------------------------------
// Guided sampling: Grid over a PrecomputedCDF record (rendering/grid.h), MIS (integrator.h:91-167)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int linear_search_cdf(const float* __restrict__ cdf, int size, float xi) {   // grid.h:233-240
    xi = fminf(fmaxf(xi, 0.0f), 0.999999f);
    int r = size - 1;
    for (int i = size - 1; i >= 0; i--) if (xi < cdf[i]) r = i;      // first i with xi < cdf[i]
    return r;
}
// The cell's solid angle (grid.h:248-252) depends on theta_idx only: the eight values fmaxf(solid_angle, 1e-6f) are
// evaluated once per workgroup (fill_grid_solid_angles, same expressions) instead of one binary64 sincos per bounce.
__shared__ float g_grid_solid_angle[8];
__device__ __forceinline__ void fill_grid_solid_angles() {     // call from block-uniform code, before the first shade_step
    if (threadIdx.x < 8) {
        const int theta_idx = threadIdx.x;
        const float theta_center = (float)((double)(((float)theta_idx + 0.5f) * 0.125f) * (PTMI_PI_D * 0.5f));
        float st, ct;
        ptmi_sincosf(theta_center, &st, &ct);
        const float sin_theta = fmaxf(st, 0.01f);
        const float solid_angle = (float)(((double)sin_theta * ((PTMI_PI_D * 0.5f) / 8)) * (2.0f * PTMI_PI_D / 16));
        g_grid_solid_angle[theta_idx] = fmaxf(solid_angle, 1e-6f);
    }
    __syncthreads();
}
__device__ __forceinline__ float grid_pdf_for_cell(const float* __restrict__ g, int theta_idx, int phi_idx) {   // grid.h:242-253
    const float cell_value = g[kCdfPdf + theta_idx * 16 + phi_idx];
    if (cell_value < 1e-8f) return 1e-6f;
    const float cell_prob = cell_value / fmaxf(g[kCdfTotal], 1e-6f);
    return cell_prob / g_grid_solid_angle[theta_idx];
}
__device__ __forceinline__ f3 grid_sample(const float* __restrict__ g, f3 normal, Rng& rng, float& out_pdf) {   // grid.h:141-188
    const float xi1 = rng_uniform(rng);
    const float xi2 = rng_uniform(rng);
    const int theta_idx = linear_search_cdf(g + kCdfMarginal, 8, xi1);
    const int phi_idx = linear_search_cdf(g + kCdfRowCdfs + theta_idx * 16, 16, xi2);
    const float jitter_theta = rng_uniform(rng);
    const float jitter_phi = rng_uniform(rng);
    float theta = (float)((double)(((float)theta_idx + jitter_theta) * 0.125f) * (PTMI_PI_D * 0.5f));
    theta = fminf(theta, (float)(PTMI_PI_D * 0.5f - (double)0.01f));
    const float phi = (float)((double)((((float)phi_idx + jitter_phi) * 0.0625f) * 2.0f) * PTMI_PI_D);
    float sin_t, cos_t, sin_p, cos_p;
    ptmi_sincosf(theta, &sin_t, &cos_t);
    ptmi_sincosf(phi, &sin_p, &cos_p);
    f3 tangent, bitangent;
    build_frame(normal, tangent, bitangent);
    const f3 world = unit_vector((sin_t * cos_p) * tangent + (sin_t * sin_p) * bitangent + cos_t * normal);
    out_pdf = grid_pdf_for_cell(g, theta_idx, phi_idx);
    return world;
}
__device__ __forceinline__ float grid_compute_pdf(const float* __restrict__ g, f3 dir, f3 normal) {   // grid.h:200-216, 299-310
    f3 tangent, bitangent;
    build_frame(normal, tangent, bitangent);
    const float lx = dot_from_zero(dir, tangent), ly = dot_from_zero(dir, bitangent), lz = dot(dir, normal);
    const float theta = ptmi_acosf(fminf(fmaxf(lz, -1.0f), 1.0f));
    float phi = ptmi_atan2f(ly, lx);
    if (phi < 0.0f) phi = (float)((double)phi + (double)2.0f * PTMI_PI_D);
    if ((double)theta > PTMI_PI_D * 0.5f) return 0.0f;
    int theta_idx = (int)(((double)theta * ((double)2.0f / PTMI_PI_D)) * 8);
    int phi_idx = (int)(((double)phi * ((double)0.5f / PTMI_PI_D)) * 16);
    theta_idx = max(0, min(theta_idx, 7));
    phi_idx = max(0, min(phi_idx, 15));
    return grid_pdf_for_cell(g, theta_idx, phi_idx);
}
__device__ __forceinline__ float mis_power_heuristic(float pdf_a, float pdf_b) {   // integrator.h:91-96
    if (pdf_a <= 0.0f) return 0.0f;
    const float a2 = pdf_a * pdf_a, b2 = pdf_b * pdf_b;
    return a2 / (a2 + b2);
}
__device__ __forceinline__ f3 sample_mis(const float* __restrict__ g, f3 normal, Rng& rng, float& weight, float bsdf_prob) {   // integrator.h:112-167
    const float BSDF_PROB = fmaxf(fminf(bsdf_prob, 0.99f), 0.01f);
    const float GRID_PROB = 1.0f - BSDF_PROB;
    const float xi = rng_uniform(rng);
    f3 dir;
    if (xi < BSDF_PROB) {
        const float u = rng_uniform(rng), v = rng_uniform(rng);
        dir = cosine_hemisphere(normal, u, v);
        const float cos_theta = fmaxf(dot(dir, normal), 0.0f);
        const float pdf_bsdf = (float)((double)cos_theta / PTMI_PI_D);
        const float pdf_grid = grid_compute_pdf(g, dir, normal);
        const float mis_w = mis_power_heuristic(pdf_bsdf, pdf_grid);
        weight = (pdf_bsdf > 1e-6f) ? mis_w / BSDF_PROB : 0.0f;
    } else {
        float pdf_grid;
        dir = grid_sample(g, normal, rng, pdf_grid);
        const float cos_theta = fmaxf(dot(dir, normal), 0.0f);
        const float pdf_bsdf = (float)((double)cos_theta / PTMI_PI_D);
        const float mis_w = mis_power_heuristic(pdf_grid, pdf_bsdf);
        if (pdf_grid > 1e-6f && cos_theta > 0.0f) {
            const float w = (float)((double)(mis_w * cos_theta) / ((PTMI_PI_D * (double)pdf_grid) * (double)GRID_PROB));
            weight = fminf(w, 10.0f);
        } else weight = 0.0f;
    }
    return dir;
}

// One iteration of integrator()'s depth loop after the intersection (integrator.h:198-266), plus the end of the
// sample and the head of the next spp iteration (integrator.h:383-390) when the path ends.
// Returns true while the pixel still has a ray to trace; false once all spp samples are done.
// GUIDED: the grid / MIS branches of integrator.h:232-263 are compiled in (sampling_mode != SAMPLING_BSDF with CDF
// records present); the plain BSDF instantiation carries none of that code.
// Material record of leaf-order slot k: plain layout mats[3k..3k+2], packed layout (normal, table row) + (Kd, Ke) table.
struct MatSource { const float4* mats; const float4* mtab; const int* load_index; int stride = 1; };      // PACKED: entry k at mats[k * stride]
template <bool PACKED>
__device__ __forceinline__ void fetch_material(const MatSource& ms, int k, f3& n, f3& bsdf, f3& Le, int& row) {
    if (PACKED) {
        const float4 m = ms.mats[(size_t)k * ms.stride];
        n = xyz(m); row = __float_as_int(m.w);
        bsdf = xyz(ms.mtab[2 * row]); Le = xyz(ms.mtab[2 * row + 1]);
    } else {
        const float4 m = ms.mats[3 * k];
        n = xyz(m); row = __float_as_int(m.w);                                    // here: the load-order primitive index
        bsdf = xyz(ms.mats[3 * k + 1]); Le = xyz(ms.mats[3 * k + 2]);
    }
}
// LEAN: the four short forms of the direction tail - sincos_2pi_lean in the cosine sample, div_by_size for the pixel jitter,
// unit_vector_voted for the Ray constructor's normalisation, rcp_exact_normal for the roulette's 1 / rr_prob.  Each gives the
// bits of the form it stands for, so LEAN changes no result.  Only ptmi_bounce<SWEEP> without STATS and GUIDED sets it: that
// kernel keeps its 8 waves per SIMD with all four (54 -> 55 VGPRs), while the phased kernels at 64 VGPRs lose a wave to any one
// of them and the wide and GUIDED kernels, already spilling at their register caps, spill more (EXPERIMENTS.md).
template <bool STATS, bool GUIDED, bool PACKED = false, bool BATCH = false, bool LEAN = false>
__device__ __forceinline__ bool shade_step(const FrameParams& fp, const TileMap& tm, const MatSource& ms, const float* cdfs, PathRegs& p,
                                           bool hit, float t, int k, LaneCounters& cn, int slot) {
    bool end_sample = !hit;                                                       // integrator.h:198-201
    // Plain BSDF sampling (!GUIDED): a lane either goes on with its path (go_on) or ends its sample; which of the two is settled
    // first, and the direction of the next segment - a cosine sample about sn or the next camera ray - is then drawn, built and
    // normalised ONCE for all lanes in the tail below, instead of once per kind at a fraction of the lanes each.
    bool go_on = false;
    f3 hp, sn;                                                                    // of the lanes that go on
    if (hit) {
        if (STATS) cn.hits++;
        f3 n, bsdf, Le; int row;
        fetch_material<PACKED>(ms, k, n, bsdf, Le, row);
        hp = p.o + t * p.d;                                                       // triangle.h:90
        p.L = p.L + p.tp * Le;                                                    // integrator.h:204
        if (p.depth > 2) {                                                        // integrator.h:207-212
            const float max_tp = fmaxf(p.tp.x, fmaxf(p.tp.y, p.tp.z));
            const float rr_prob = fminf(max_tp, 0.95f);
            if (rng_uniform(p.rng) > rr_prob) end_sample = true;
            else {
                // 1 / rr_prob (integrator.h:211).  LEAN: by the short reciprocal, no vote: a lane is here with rng_uniform <= rr_prob,
                // a uniform is >= 2^-33 and rr_prob = fminf(max_tp, 0.95f) <= 0.95 (a NaN max_tp gives 0.95), so rr_prob lies in
                // [2^-33, 0.95], inside rcp_exact_normal's interval (test_gpu_shade_lean_forms.py::test_roulette_reciprocal)
                const float inv_rr = LEAN ? rcp_exact_normal(rr_prob) : rcp_rn(rr_prob);
                p.tp = mk3(p.tp.x * inv_rr, p.tp.y * inv_rr, p.tp.z * inv_rr);
            }
        }
        if (!end_sample) {
            p.tp = p.tp * bsdf;                                                   // integrator.h:215
            if (length_below_1em5(length_squared(p.tp))) end_sample = true;       // integrator.h:218, length(tp) < 1e-5f
            else {
                sn = dot(p.d, n) < 0 ? n : -n;                                    // integrator.h:221-222
                // initGridFromPrimitive (integrator.h:31-57): the primitive's precomputed record, if it is valid
                const float* g = nullptr;
                if (GUIDED) {
                    const float* rec = cdfs + (size_t)(PACKED ? ms.load_index[k] : row) * kCdfDwords;
                    if (__float_as_int(rec[kCdfValid]) != 0) g = rec;
                }
                if (GUIDED && g) {
                    f3 next;
                    float weight = 1.0f;
                    if (fp.sampling_mode == 3) {                                  // SAMPLING_MIS, integrator.h:238-241
                        next = sample_mis(g, sn, p.rng, weight, fp.mis_bsdf_fraction);
                    } else {                                                      // pure grid sampling, integrator.h:242-257
                        float grid_pdf;
                        next = grid_sample(g, sn, p.rng, grid_pdf);
                        const float cos_theta = fmaxf(dot(next, sn), 0.0f);
                        weight = (float)((double)cos_theta / (PTMI_PI_D * (double)fmaxf(grid_pdf, 1e-6f)));
                        weight = fminf(fmaxf(weight, 0.0f), 10.0f);
                    }
                    p.tp = mk3(p.tp.x * weight, p.tp.y * weight, p.tp.z * weight);
                    p.depth++;
                    if (p.depth < fp.max_depth) {
                        p.o = hp + 1e-4f * sn;                                    // integrator.h:266
                        p.d = unit_vector(next);
                    } else end_sample = true;
                } else if (GUIDED) {                                              // the cosine fallback :258-261
                    const float u = rng_uniform(p.rng);                           // integrator.h:63-64
                    const float v = rng_uniform(p.rng);
                    p.depth++;
                    if (p.depth < fp.max_depth) {
                        const f3 next = cosine_hemisphere(sn, u, v);              // integrator.h:230
                        p.o = hp + 1e-4f * sn;                                    // integrator.h:266
                        p.d = unit_vector(next);                                  // Ray ctor normalises again
                    } else end_sample = true;                                     // loop bound; the draws above are still consumed
                } else {                                                          // BSDF mode
                    p.depth++;
                    if (p.depth < fp.max_depth) go_on = true;
                    else {                                                        // loop bound: the reference has drawn u and v by now
                        rng_next(p.rng); rng_next(p.rng);                         // (integrator.h:63-64); the stream moves on, nothing reads them
                        end_sample = true;
                    }
                }
            }
        }
    }
    if (end_sample) {
        p.color = p.color + p.L;                                                  // integrator.h:390
        p.sample_idx++;
        if (!BATCH) {
            if (p.sample_idx >= (unsigned int)fp.spp) return false;
        } else if ((p.sample_idx & fp.sample_mask) >= (unsigned int)fp.spp) {     // the spp loop of this frame is through
            const unsigned int frame = p.sample_idx >> 16;
            if (frame + 1u >= (unsigned int)fp.n_frames) return false;
            // frame batch: bank this frame's colour sum and go straight on with the next frame's first sample
            fp.frame_color[frame * (unsigned int)fp.n_local + (unsigned int)slot] = make_float4(p.color.x, p.color.y, p.color.z, 0.0f);   // < 2^31 (host check)
            p.sample_idx = (frame + 1u) << 16;
            p.color = mk3(0.0f, 0.0f, 0.0f);
        }
        if (GUIDED) {
            camera_ray(fp, tm, p.px, p.py, p.rng, p.o, p.d);                      // next iteration of the spp loop
            p.tp = mk3(1.0f, 1.0f, 1.0f); p.L = mk3(0.0f, 0.0f, 0.0f); p.depth = 0;
        }
    }
    if (!GUIDED) {
        // every lane still here draws two uniforms: (u, v) of sampleCosineHemisphere (integrator.h:63-64) where the path goes on,
        // the pixel jitter of the next sample (integrator.h:384-385) where it ended - the same two draws, in the same order
        const float r1 = rng_uniform(p.rng);
        const float r2 = rng_uniform(p.rng);
        f3 w;
        if (go_on) {
            w = cosine_hemisphere<LEAN>(sn, r1, r2);                              // integrator.h:230
            p.o = hp + 1e-4f * sn;                                                // integrator.h:266
        } else {
            w = camera_dir_raw<LEAN>(fp, tm, p.px, p.py, r1, r2, p.o);            // next iteration of the spp loop
            p.tp = mk3(1.0f, 1.0f, 1.0f); p.L = mk3(0.0f, 0.0f, 0.0f); p.depth = 0;
        }
        // the Ray constructor's normalisation (ray.h:9-12) of either kind: a bounce direction has length 1 to rounding, but nothing
        // bounds the camera's un-normalised one: IEEE sqrt and 1 / len, or (LEAN) one vote per wave between the short forms and
        // those (pt_vec.h)
        p.d = LEAN ? unit_vector_voted(w) : unit_vector(w);
    }
    return true;
}

// shade_step<false, false, false, BATCH, true> as ptmi_bounce<SWEEP> without STATS and GUIDED takes it: the same expressions, the
// same draws in the same order, every lane the same results - written so that the path state keeps its registers through the
// segment.  In shade_step the state is assigned inside nested divergent branches, the compiler gives each branch's values
// registers of their own, and every join copies them back: 62 v_mov_b32 and 4 v_readlane_b32 on the hot path of that kernel's
// segment loop.  Here
//   - the decisions (roulette, throughput below the bound, depth limit) are lane flags taken in straight-line code, and each
//     field of the state is written once, in place, by the lanes the flag selects;
//   - L is final before tp changes (the scheduler otherwise sinks the emission behind the material's last LDS word and keeps
//     the old tp alive beside the new one);
//   - the roulette's draw is rng_uniform_if, the two draws of the tail are rng_uniform2 (pt_device.h);
//   - FRAME: the next camera ray reads the frame block (camera_dir_block).
// What the lanes outside a flag compute - a reciprocal of a roulette probability nobody drew against, a material of slot 0 for a
// lane that hit nothing - is never selected.  A pixel that leaves (return false) stores the fresh path's tp, L and depth, not its
// last ones: every begin kernel rewrites them.  Between the loop's header and its back edge, outside the walk, the timed triangle
// build now has 39 v_mov_b32 (was 75 over all blocks, 62 on the hot path), 4 v_readlane_b32 and 4 v_writelane_b32 (8 and 4; all on
// the sincos vote's cold side now) and no s_load of a kernel argument: `tools/isa_digest.py loop` prints them.
template <bool BATCH, bool FRAME>
__device__ __forceinline__ bool shade_step_sweep(const FrameParams& fp, const TileMap& tm, const FrameBlock& fb, const float4* mats, PathRegs& p,
                                                 bool hit, float t, int k, int slot) {
    f3 n, bsdf, Le; int row;
    fetch_material<false>(MatSource{mats, nullptr, nullptr}, hit ? k : 0, n, bsdf, Le, row);
    const f3 hp = p.o + t * p.d;                                                  // triangle.h:90
    if (hit) p.L = p.L + p.tp * Le;                                               // integrator.h:204
    asm("" : "+v"(p.L.x), "+v"(p.L.y), "+v"(p.L.z), "+v"(p.tp.x), "+v"(p.tp.y), "+v"(p.tp.z));
    // integrator.h:207-212.  1 / rr_prob by the short reciprocal: see shade_step
    const bool deep = hit && p.depth > 2;
    const float rr_prob = fminf(fmaxf(p.tp.x, fmaxf(p.tp.y, p.tp.z)), 0.95f);
    const bool killed = deep && rng_uniform_if(p.rng, deep) > rr_prob;
    const float inv_rr = rcp_exact_normal(rr_prob);
    if (deep && !killed) p.tp = mk3(p.tp.x * inv_rr, p.tp.y * inv_rr, p.tp.z * inv_rr);
    bool end_sample = !hit || killed;                                             // integrator.h:198-201
    if (!end_sample) p.tp = p.tp * bsdf;                                          // integrator.h:215
    end_sample = end_sample || length_below_1em5(length_squared(p.tp));           // integrator.h:218, length(tp) < 1e-5f
    const f3 sn = dot(p.d, n) < 0 ? n : -n;                                       // integrator.h:221-222
    if (!end_sample) p.depth++;
    const bool go_on = !end_sample && p.depth < fp.max_depth;
    if (!end_sample && !go_on) {                                                  // loop bound: the reference has drawn u and v by now
        uint32_t x1, x2;                                                          // (integrator.h:63-64); the stream moves on, nothing reads them
        rng_next2(p.rng, x1, x2);
    }
    if (!go_on) {
        p.color = p.color + p.L;                                                  // integrator.h:390
        p.sample_idx++;
        // the next iteration of the spp loop starts from a fresh path.  Written here, in place, ahead of the pixel's exit: a pixel
        // that leaves below then holds what the lanes that go on hold, and no second copy of the state is kept for it
        p.tp = mk3(1.0f, 1.0f, 1.0f); p.L = mk3(0.0f, 0.0f, 0.0f); p.depth = 0;
        if (!BATCH) {
            if (p.sample_idx >= (unsigned int)fp.spp) return false;
        } else if ((p.sample_idx & fp.sample_mask) >= (unsigned int)fp.spp) {     // the spp loop of this frame is through
            const unsigned int frame = p.sample_idx >> 16;
            if (frame + 1u >= (unsigned int)fp.n_frames) return false;
            // frame batch: see shade_step
            fp.frame_color[frame * (unsigned int)fp.n_local + (unsigned int)slot] = make_float4(p.color.x, p.color.y, p.color.z, 0.0f);   // < 2^31 (host check)
            p.sample_idx = (frame + 1u) << 16;
            p.color = mk3(0.0f, 0.0f, 0.0f);
        }
    }
    // (u, v) of sampleCosineHemisphere where the path goes on, the pixel jitter of the next sample where it ended (shade_step)
    float r1, r2;
    rng_uniform2(p.rng, r1, r2);
    f3 w;
    if (go_on) {
        w = cosine_hemisphere<true>(sn, r1, r2);                                  // integrator.h:230
        p.o = hp + 1e-4f * sn;                                                    // integrator.h:266
    } else {
        w = FRAME ? camera_dir_block(fb, p.px, p.py, r1, r2, p.o)                 // next iteration of the spp loop
                  : camera_dir_raw<true>(fp, tm, p.px, p.py, r1, r2, p.o);
    }
    p.d = unit_vector_voted(w);                                                   // ray.h:9-12
    return true;
}

}  // namespace ptmi
