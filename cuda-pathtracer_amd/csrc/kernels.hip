// kernels.hip — the frame's own gfx950 kernels of the render path, and the launch of the bounce kernels.
//
// Compile with -ffp-contract=off: results must be bit-identical to the strict-IEEE
// evaluation of the reference's expressions (see include/ptmi_math.h, pt_vec.h).
//
// Kernels, by file (shared device functions: traversal.h the walks, shading.h the integrator's step, bounce.h the launch's
// head and tail)
//   kernels.hip        ptmi_render_init   render_init (integrator.h:274-280): XORWOW seeding + 2^67*pixel skip-ahead
//                      ptmi_frame_begin   sample 0's camera ray for every pixel (integrator.h:383-387)
//                      ptmi_resolve       integrator.h:393-407; the accumulation passes; the launch order by cost
//   bounce_sync.hip    ptmi_bounce        THE hot kernel (scenes up to 64 primitives, and deep-tree fallback): intersect (scene.h:50-110,
//                      triangle.h:64-96, quad.h:49-132) + integrator() body (integrator.h:189-268) + regeneration +
//                      queue compaction; segment-synchronous, wave-uniform SWEEP walk (or STACK / LANE)
//   bounce_phased.hip  ptmi_bounce_phased the same work for larger scenes: per-lane stackless walk with wave-scheduled NODE/PRIM/SHADE phases
//   bounce_wide.hip    ptmi_bounce_wide   the phased scheduling over the opt-in 8-wide tree, plain or certified
//   first_hit.hip      the Radiosity view, and
//                      ptmi_render_nee    opt-in next-event estimation with MIS (include/ptmi.h): one lane runs a pixel's samples to their end;
//                                         its ENV instantiation renders every frame of a context with an environment (ptmi_set_environment),
//                                         its SURF = 1 instantiation every frame of a scene with a mirror or glass primitive (ptmi_set_surfaces),
//                                         SURF = 2 with a rough-metal primitive as well (ptmi_set_surfaces_rough; rough.h),
//                                         its SMOOTH instantiation every frame of a scene with a smooth primitive (ptmi_set_vertex_normals;
//                                         vertex_normal.h), its TEX instantiation every frame of a scene with a textured primitive
//                                         (ptmi_set_albedo_texture; albedo_texture.h); every instantiation starts its samples on a thin
//                                         lens where the context has one (ptmi_set_lens; lens.h): an argument, not a parameter;
//                                         its MEDIUM instantiation every frame of a scene with a participating medium
//                                         (ptmi_set_medium; medium.h)
//   features.hip       ptmi_features      the feature pass; its SHADED instantiation where ptmi_set_feature_shading asks for a table the context has
//   debug_hooks.hip    the test hooks
#include "bounce.h"

namespace ptmi {

// One 160x160 GF(2) matrix at a time is staged in LDS (3200 B); rows are read as wave-wide broadcasts.
__global__ __launch_bounds__(kBlock) void ptmi_render_init(TileMap tm, PathState st, const uint32_t* __restrict__ jump,
                                                           unsigned long long seed_base) {
    __shared__ uint32_t M[160 * 5];
    const int n = tm.local_rows * tm.width;
    const int slot = blockIdx.x * kBlock + threadIdx.x;
    const bool live = slot < n;
    int x = 0, y = 0;
    const unsigned int pix = live ? (unsigned int)global_pixel(tm, slot, x, y) : 0u;
    const unsigned long long seed = seed_base + (unsigned long long)pix;
    const uint32_t s0 = ((uint32_t)seed) ^ 0xaad26b49u;
    const uint32_t s1 = (uint32_t)(seed >> 32) ^ 0xf7dcefddu;
    const uint32_t t0 = 1099087573u * s0;
    const uint32_t t1 = 2591861531u * s1;
    uint32_t v[5] = {123456789u + t0, 362436069u ^ t0, 521288629u + t1, 88675123u ^ t1, 5783321u + t0};
    const uint32_t d = 6615241u + t1 + t0;

    for (int k = 0; k < 32; k++) {
        const bool mine = live && ((pix >> k) & 1u);
        if (!__syncthreads_or(mine ? 1 : 0)) continue;     // block-uniform: nobody needs T^(2^67 * 2^k)
        for (int i = threadIdx.x; i < 160 * 5; i += kBlock) M[i] = jump[k * 160 * 5 + i];
        __syncthreads();
        if (mine) {
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
        __syncthreads();
    }
    if (!live) return;
    st.E[slot] = make_uint4(v[0], v[1], v[2], v[3]);
    st.F[slot] = make_uint2(v[4], d);
    st.A[slot] = make_float4(0, 0, 0, 1.0f);
    st.B[slot] = make_float4(0, 0, 1.0f, 1.0f);
    st.C[slot] = make_float4(0, 0, 0, 1.0f);
    st.D[slot] = make_float4(0, 0, 0, __uint_as_float(0u));
}

__global__ __launch_bounds__(kBlock) void ptmi_frame_begin(TileMap tm, PathState st, FrameParams fp) {
    const int n = tm.local_rows * tm.width;
    const int slot = blockIdx.x * kBlock + threadIdx.x;
    if (slot >= n) return;
    int x, y;
    global_pixel(tm, slot, x, y);
    const uint4 e = st.E[slot]; const uint2 f = st.F[slot];
    Rng rng = {e.x, e.y, e.z, e.w, f.x, f.y};
    f3 o, d;
    camera_ray(fp, tm, x, y, rng, o, d);
    st.A[slot] = make_float4(o.x, o.y, o.z, 1.0f);
    st.B[slot] = make_float4(d.x, d.y, d.z, 1.0f);
    st.C[slot] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    st.D[slot] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0u));
    st.E[slot] = make_uint4(rng.v0, rng.v1, rng.v2, rng.v3);
    st.F[slot] = make_uint2(rng.v4, rng.d);
}

size_t bounce_lds_bytes_wide(const DeviceScene& sc) { return (size_t)sc.w_top * kWideNodeDwords * 4 + (size_t)sc.w_depth * kBlock * sizeof(uint2); }
size_t bounce_lds_bytes(const DeviceScene& sc) {
    if (sc.traversal == TRAVERSAL_WIDE || sc.traversal == TRAVERSAL_CERTIFIED) return bounce_lds_bytes_wide(sc);
    size_t b = 0;
    const bool geom = sc.lds_resident || sc.traversal == TRAVERSAL_SWEEP;
    // the sweep: with the frame block, the larger of its two node images and the leaf image - which of them a build stages is its own matter (sweep_form)
    if (geom) b += (sc.traversal == TRAVERSAL_SWEEP ? ptmi_sweep_leaves_lds_vecs(sc.n_nodes, sc.prim_stride, sc.n_prims, sc.sweep_leaves)
                                                    : ptmi_scene_lds_vecs(sc.n_nodes, sc.prim_stride, sc.n_prims)) * sizeof(float4);   // what stage_scene lays out (bounce.h)
    if (sc.traversal == TRAVERSAL_STACK) b += (size_t)sc.stack_entries * kBlock * sizeof(int);
    return b;
}

// ---- kernel selection: the only place that knows which traversal belongs to which kernel family ---------------------------
static BounceKernel select_bounce_kernel(const BounceArgs& a, size_t* lds) {
    const DeviceScene& sc = a.sc;
    *lds = bounce_lds_bytes(sc);
    switch (sc.traversal) {
        case TRAVERSAL_PHASED: return select_bounce_phased(a);
        case TRAVERSAL_PACKED: *lds = (size_t)sc.n_top * 2 * sizeof(float4); return select_bounce_phased(a);     // the top of the packed tree
        case TRAVERSAL_WIDE:
        case TRAVERSAL_CERTIFIED: return select_bounce_wide(a);
        default: return select_bounce_sync(a);                  // TRAVERSAL_SWEEP, TRAVERSAL_LANE, TRAVERSAL_STACK
    }
}

void launch_bounce(const DeviceScene& sc, const TileMap& tm, const PathState& st, const FrameParams& fp,
                   const int* queue_in, int n_in, const int* count_in, int* queue_out, int* count_out, int segments,
                   StatCounters* stats, bool many_waves, hipStream_t s, const CountPublish& pub, const LaunchSchedule& sched) {
    if (n_in <= 0) return;
    BounceArgs a{sc, tm, st, fp, queue_in, n_in, count_in, queue_out, count_out, segments, stats, many_waves ? 1 : 0,
                 pub.done_count, pub.next_count, pub.host_count, nullptr, nullptr, nullptr};
    dim3 grid((n_in + kBlock - 1) / kBlock);
    const bool wide = sc.traversal == TRAVERSAL_WIDE || sc.traversal == TRAVERSAL_CERTIFIED;
    if (wide && sched.max_waves > 0 && sched.cursor) {      // fewer lanes than queue entries: the lanes take the rest through the cursor
        a.cursor = sched.cursor;
        grid.x = std::min<unsigned int>(grid.x, (unsigned int)(sched.max_waves + kBlock / 64 - 1) / (kBlock / 64));
    }
    if (wide) { a.cost = sched.cost; a.cost_max = sched.cost_max; }
    size_t lds = 0;
    const BounceKernel k = select_bounce_kernel(a, &lds);
    hipLaunchKernelGGL(k, grid, dim3(kBlock), lds, s, a);
}

// waves of the frame's bounce kernel that the device holds at once (0: unknown)
int bounce_resident_waves(const DeviceScene& sc, const FrameParams& fp, bool stats, int n_cus) {
    BounceArgs a{sc, TileMap(), PathState(), fp, nullptr, 0, nullptr, nullptr, nullptr, 0, stats ? reinterpret_cast<StatCounters*>(1) : nullptr, 0,
                 nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t lds = 0;
    const BounceKernel k = select_bounce_kernel(a, &lds);
    int blocks = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k, kBlock, lds) != hipSuccess) blocks = 0;
    return blocks * (kBlock / 64) * n_cus;
}

// ---- launch order by cost (device_scene.h: launch_order_by_cost) ---------------------------------------------------------------
// class 0 = the heaviest: (255 - floor(256 cost / (cost_max + 1))) >> shift, so ascending classes are descending costs
__device__ __forceinline__ int cost_class(unsigned int c, unsigned int cmax, int shift) {
    const unsigned long long k = ((unsigned long long)min(c, cmax) << 8) / ((unsigned long long)cmax + 1ull);
    return (255 - (int)k) >> shift;
}
__global__ __launch_bounds__(kBlock) void ptmi_cost_histogram(const int* __restrict__ queue_in, int n, const unsigned int* __restrict__ cost,
                                                              const unsigned int* __restrict__ cost_max, int* __restrict__ hist, int shift) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const unsigned int cmax = *cost_max;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
        atomicAdd(&h[cost_class(cost[queue_in ? queue_in[i] : i], cmax, shift)], 1);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}
// one workgroup: hist[256 + c] = first position of class c
__global__ __launch_bounds__(kBlock) void ptmi_cost_offsets(int* __restrict__ hist) {
    __shared__ int h[256];
    h[threadIdx.x] = hist[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) { int acc = 0; for (int c = 0; c < 256; c++) { const int v = h[c]; h[c] = acc; acc += v; } }
    __syncthreads();
    hist[256 + threadIdx.x] = h[threadIdx.x];
}
// every workgroup takes 256 consecutive entries, counts its classes, reserves one range per class and places its entries there
// in their order (so neighbours of one class stay neighbours)
__global__ __launch_bounds__(kBlock) void ptmi_cost_scatter(const int* __restrict__ queue_in, int n, const unsigned int* __restrict__ cost,
                                                            const unsigned int* __restrict__ cost_max, int* __restrict__ hist, int* __restrict__ queue, int shift) {
    __shared__ int h[256], base[256];
    __shared__ unsigned char cls[kBlock];
    h[threadIdx.x] = 0;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int entry = i < n ? (queue_in ? queue_in[i] : i) : 0;
    const int c = i < n ? cost_class(cost[entry], *cost_max, shift) : 255;
    cls[threadIdx.x] = (unsigned char)c;
    __syncthreads();
    if (i < n) atomicAdd(&h[c], 1);
    int local = 0;                                     // entries of my class before me in this workgroup
    for (int j = 0; j < (int)threadIdx.x; j++) local += cls[j] == c ? 1 : 0;
    __syncthreads();
    if (h[threadIdx.x]) base[threadIdx.x] = atomicAdd(&hist[256 + threadIdx.x], h[threadIdx.x]);
    __syncthreads();
    if (i < n) queue[base[c] + local] = entry;
}
void launch_order_by_cost(const int* queue_in, int n, const unsigned int* cost, const unsigned int* cost_max, int* hist, int* queue, int classes, hipStream_t s) {
    if (n <= 0) return;
    int shift = 0;
    while ((256 >> shift) > classes && shift < 7) shift++;
    (void)hipMemsetAsync(hist, 0, 512 * sizeof(int), s);
    const int blocks = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(ptmi_cost_histogram, dim3(std::min(blocks, 1024)), dim3(kBlock), 0, s, queue_in, n, cost, cost_max, hist, shift);
    hipLaunchKernelGGL(ptmi_cost_offsets, dim3(1), dim3(kBlock), 0, s, hist);
    hipLaunchKernelGGL(ptmi_cost_scatter, dim3(blocks), dim3(kBlock), 0, s, queue_in, n, cost, cost_max, hist, queue, shift);
}

void launch_render_init(const TileMap& tm, const PathState& st, const uint32_t* d_jump, uint64_t seed_base, hipStream_t s) {
    const int n = tm.local_rows * tm.width;
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_render_init, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, tm, st, d_jump,
                       (unsigned long long)seed_base);
}

void launch_frame_begin(const TileMap& tm, const PathState& st, const FrameParams& fp, hipStream_t s) {
    const int n = tm.local_rows * tm.width;
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_frame_begin, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, tm, st, fp);
}

// ---------------------------------------------------------------------------------------------
// resolve: color /= spp; Reinhard; gamma 1/2.2; 8-bit (integrator.h:393-407)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ptmi_resolve(TileMap tm, PathState st, int spp, unsigned char* __restrict__ rgb8,
                                                       float* __restrict__ radiance, const float4* __restrict__ color_src) {
    const int n = tm.local_rows * tm.width;
    const int slot = blockIdx.x * kBlock + threadIdx.x;
    if (slot >= n) return;
    const float4 D = color_src ? color_src[slot] : st.D[slot];
    int ox, olr;
    slot_to_local(tm, slot, ox, olr);
    const size_t out = (size_t)olr * (size_t)tm.width + (size_t)ox;      // images are local-row-major whatever the slot order
    const float k = rcp_rn((float)spp);                    // Vector::operator/=(T): T k = 1.0 / t (vector.h:90-94)
    resolve_pixel(D, k, out, rgb8, radiance);
}

void launch_resolve(const TileMap& tm, const PathState& st, int spp, unsigned char* rgb8, float* radiance, hipStream_t s,
                    const float4* color_src) {
    const int n = tm.local_rows * tm.width;
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_resolve, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, tm, st, spp, rgb8, radiance, color_src);
}

// ---------------------------------------------------------------------------------------------
// accumulation passes (include/ptmi.h: ptmi_accum_pass; device_scene.h: AccumBuffers)
// ---------------------------------------------------------------------------------------------
// ptmi_frame_begin for the queued pixels of a pass: the same draws, the same first camera ray; the sample index starts at 0
// again and the colour sum goes on (first pass: from zero)
__global__ __launch_bounds__(kBlock) void ptmi_pass_begin(TileMap tm, PathState st, FrameParams fp, const int* __restrict__ queue, int n, int first) {
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= n) return;
    const int slot = queue ? queue[idx] : idx;
    int x, y;
    global_pixel(tm, slot, x, y);
    const uint4 e = st.E[slot]; const uint2 f = st.F[slot];
    Rng rng = {e.x, e.y, e.z, e.w, f.x, f.y};
    f3 o, d;
    camera_ray(fp, tm, x, y, rng, o, d);
    const float4 D = first ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : st.D[slot];
    st.A[slot] = make_float4(o.x, o.y, o.z, 1.0f);
    st.B[slot] = make_float4(d.x, d.y, d.z, 1.0f);
    st.C[slot] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    st.D[slot] = make_float4(D.x, D.y, D.z, __uint_as_float(0u));
    st.E[slot] = make_uint4(rng.v0, rng.v1, rng.v2, rng.v3);
    st.F[slot] = make_uint2(rng.v4, rng.d);
}

// The stopping test of the pass's pixels (the rule of include/ptmi.h, float32 in the order written there) and the next pass's
// queue: the pixels that go on, in their input order inside a wave (ballot + prefix popcount, one atomic per wave)
__global__ __launch_bounds__(kBlock) void ptmi_adapt(PathState st, AccumBuffers ab, AdaptRule rule, const int* __restrict__ queue_in, int n,
                                                     int* __restrict__ queue_out, int* __restrict__ count_out) {
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    const bool active = idx < n;
    const int slot = active ? (queue_in ? queue_in[idx] : idx) : 0;
    bool more = false;
    if (active) {
        const float4 S = st.D[slot];
        const float4 prev = rule.first ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : ab.prev[slot];    // S_{k-1}.xyz, mean
        float M2 = rule.first ? 0.0f : ab.m2[slot];
        const unsigned int k = (rule.first ? 0u : ab.passes[slot]) + 1u;
        const float dx = S.x - prev.x, dy = S.y - prev.y, dz = S.z - prev.z;
        const float y = (0.2126f * dx + 0.7152f * dy + 0.0722f * dz) * rule.inv_spp;
        const float nf = (float)k;
        const float delta = y - prev.w;
        const float mean = prev.w + delta / nf;
        M2 = M2 + delta * (y - mean);
        const float a = rule.threshold * (mean + rule.floor_);
        const bool stop = rule.stopping && ((int)k >= rule.max_passes ||
                                            ((int)k >= rule.min_passes && M2 <= a * a * (float)(k * (k - 1u))));
        ab.prev[slot] = make_float4(S.x, S.y, S.z, mean);
        ab.m2[slot] = M2;
        ab.passes[slot] = k;
        more = !stop;
    }
    const unsigned long long mask = __ballot(more);
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0 && mask) base = atomicAdd(count_out, __popcll(mask));
    base = __shfl(base, 0);
    if (more) queue_out[base + __popcll(mask & ((1ull << lane) - 1ull))] = slot;
}

// ptmi_resolve with every pixel's own sample count (passes x spp), over all local pixels: the ones that stopped keep their
// image; also the count map, local row-major
__global__ __launch_bounds__(kBlock) void ptmi_resolve_counts(TileMap tm, PathState st, const unsigned int* __restrict__ passes, int spp,
                                                              unsigned char* __restrict__ rgb8, float* __restrict__ radiance,
                                                              unsigned int* __restrict__ counts) {
    const int n = tm.local_rows * tm.width;
    const int slot = blockIdx.x * kBlock + threadIdx.x;
    if (slot >= n) return;
    const float4 D = st.D[slot];
    int ox, olr;
    slot_to_local(tm, slot, ox, olr);
    const size_t out = (size_t)olr * (size_t)tm.width + (size_t)ox;
    const unsigned int samples = passes[slot] * (unsigned int)spp;          // < 2^24 (host check): exact as a float
    counts[out] = samples;
    resolve_pixel(D, rcp_rn((float)samples), out, rgb8, radiance);
}

void launch_pass_begin(const TileMap& tm, const PathState& st, const FrameParams& fp, const int* queue, int n, bool first, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_pass_begin, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, tm, st, fp, queue, n, first ? 1 : 0);
}
void launch_adapt(const PathState& st, const AccumBuffers& ab, const AdaptRule& rule, const int* queue_in, int n, int* queue_out,
                  int* count_out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_adapt, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, st, ab, rule, queue_in, n, queue_out, count_out);
}
void launch_resolve_counts(const TileMap& tm, const PathState& st, const unsigned int* passes, int spp, unsigned char* rgb8,
                           float* radiance, unsigned int* counts, hipStream_t s) {
    const int n = tm.local_rows * tm.width;
    if (n <= 0) return;
    hipLaunchKernelGGL(ptmi_resolve_counts, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, tm, st, passes, spp, rgb8, radiance, counts);
}

}  // namespace ptmi
