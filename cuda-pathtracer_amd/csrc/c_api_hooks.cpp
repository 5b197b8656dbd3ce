// c_api_hooks.cpp — the test hooks of libptmi.so: every ptmi_debug_* entry of include/ptmi.h, and nothing else.  A hook checks its
// arguments and the context's state first - a refused call touches no device - and then either sets state the product reads or
// runs one kernel on given inputs through HookRun.
#include "c_api_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

#include "shade_lean.h"

using namespace ptmi;

namespace {

// One launch on given inputs: upload, launch once, synchronise, download.  Constructing it is the hook's first HIP call: it binds
// the context's device and stream.  A buffer is asked for where the launcher takes it, inside run()'s launch, so every size is
// written once, beside the parameter it belongs to; run() downloads once the stream has drained.
class HookRun {
    struct Download { void* host; const void* dev; size_t bytes; };
    std::vector<void*> bufs_;
    std::vector<Download> downloads_;
    template <class T> T* alloc(size_t n) { bufs_.push_back(nullptr); return (T*)(bufs_.back() = hipMallocSafe(n * sizeof(T), "debug buffer")); }
public:
    const hipStream_t stream;
    explicit HookRun(ptmi_ctx* c) : stream(c->app.render.stream) { PTMI_HIP(hipSetDevice(c->app.device_id)); }
    HookRun(const HookRun&) = delete;
    ~HookRun() { for (void* p : bufs_) if (p) (void)hipFree(p); }
    // n elements of h on the device.  h == nullptr, an optional buffer left out: a dummy allocation, and nullptr for the kernel
    template <class T> const T* in(const T* h, size_t n) {
        T* d = alloc<T>(h ? n : 1);
        if (h) PTMI_HIP(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
        return h ? d : nullptr;
    }
    // n elements for the kernel to write, downloaded to h after the launch (h == nullptr: not downloaded); fill 0 or 0xff sets
    // every byte on the stream first, for the elements a kernel leaves alone
    template <class T> T* out(T* h, size_t n, int fill = -1) {
        T* d = alloc<T>(n);
        if (fill >= 0) PTMI_HIP(hipMemsetAsync(d, fill, n * sizeof(T), stream));
        if (h) downloads_.push_back({h, d, n * sizeof(T)});
        return d;
    }
    // n elements the kernel updates: h's values up, the kernel's back into h
    template <class T> T* inout(T* h, size_t n) {
        T* d = out(h, n);
        PTMI_HIP(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    template <class Launch> void run(Launch&& launch) {
        launch(stream);
        PTMI_HIP(hipGetLastError());
        PTMI_HIP(hipStreamSynchronize(stream));
        for (const Download& d : downloads_) PTMI_HIP(hipMemcpy(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost));
    }
};

// the wave-vote hooks: n cases of in_per floats in waves of 64, live[i] == 0 a lane that is not active; out_per floats per case
// back, zero where a lane was not active
template <class Launch>
void run_vote_hook(ptmi_ctx* c, int n, const float* in, int in_per, const int* live, float* out, int out_per, Launch launch) {
    need(c && in && live && out, "NULL argument");
    need(n > 0, "n must be positive");
    HookRun k(c);
    k.run([&](hipStream_t s) { launch(k.in(in, (size_t)in_per * n), k.in(live, n), k.out(out, (size_t)out_per * n, 0), s); });
}

// the bit-sweep checks: a kernel compares a short form with the IEEE one over count bit patterns and counts into two words,
// {mismatches, the smallest mismatching pattern}, preset to {0, ~0}
template <class Launch>
void run_bit_sweep(ptmi_ctx* c, uint64_t count, uint64_t* mismatches, uint32_t* first_bad_bits, Launch launch) {
    need(count > 0 && count <= (1ull << 32), "count must be in [1, 2^32]");
    HookRun k(c);
    unsigned long long h[2] = {0ull, ~0ull};
    k.run([&](hipStream_t s) { launch(k.inout(h, 2), s); });
    *mismatches = h[0]; *first_bad_bits = h[0] ? (uint32_t)h[1] : 0u;
}

// the intersect hooks take rays from anywhere: each origin is held to the bound the scene and the camera are held to
// (SceneState::upload)
void check_hook_rays(ptmi_ctx* c, int n, const float* o, const float* d) {
    const SceneState& s = c->app.scene;
    need(s.d_nodes != nullptr, "no scene loaded");
    need(n > 0, "n must be positive");
    for (int i = 0; i < n; i++) s.checkQuadOrigin(o + 3 * (size_t)i, d + 3 * (size_t)i, "ray");
}

// the table hooks (vertex normals, albedo) name primitives in load order
void check_hook_prims(ptmi_ctx* c, int n, const int* prim, const float* p, float* out) {
    need(c && prim && p && out, "NULL argument");
    need(n >= 0, "n must not be negative");
    need(c->app.scene.d_nodes != nullptr, "no scene loaded");
    const int n_prims = (int)c->app.scene.h_primitives.size();
    for (int i = 0; i < n; i++) need(prim[i] >= 0 && prim[i] < n_prims, "prim out of range");
}
// and their kernels take leaf-order slots: bvh_indices[slot] is the slot's primitive
std::vector<int> leaf_slots(const SceneState& sc, int n, const int* prim) {
    std::vector<int> slot_of(sc.h_primitives.size()), slots((size_t)n);
    for (size_t k = 0; k < slot_of.size(); k++) slot_of[sc.bvh_indices[k]] = (int)k;
    for (int i = 0; i < n; i++) slots[i] = slot_of[prim[i]];
    return slots;
}

}  // namespace

extern "C" {

// ---- state the product reads: which walk, which tree ----
int ptmi_debug_set_traversal(ptmi_ctx* c, int force_mode, int sweep_max_prims, int* out_mode) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        need(force_mode >= -1 && (force_mode <= 4 || force_mode == TRAVERSAL_CERTIFIED), "force_mode must be -1..4 or 6");
        need(sweep_max_prims >= 0, "sweep_max_prims must be >= 0");
        SceneState& s = c->app.scene;
        s.force_traversal = force_mode; s.sweep_max_prims = sweep_max_prims;
        if (force_mode == TRAVERSAL_CERTIFIED && s.d_nodes && !s.fastReady()) {
            PTMI_HIP(hipSetDevice(c->app.device_id));
            s.buildFast();
        }
        s.chooseTraversal();
        if (out_mode) *out_mode = s.d_nodes ? s.d_scene.traversal : -1;
    });
}

int ptmi_debug_get_traversal(const ptmi_ctx* c, int* out_mode) {
    return guarded([&] {
        need(c != nullptr && out_mode != nullptr, "ctx / out_mode is NULL");
        *out_mode = c->app.scene.d_nodes ? c->app.scene.d_scene.traversal : -1;
    });
}

int ptmi_debug_set_solver_walk(ptmi_ctx* c, int force_walk, int min_prims) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        need(force_walk == -1 || force_walk == 0 || (force_walk >= 2 && force_walk <= 4), "force_walk must be -1, 0, 2, 3 or 4");
        need(min_prims >= 0, "min_prims must be >= 0");
        c->app.radiosity.force_walk = force_walk; c->app.radiosity.cert_min_prims = min_prims;
    });
}

int ptmi_debug_set_packed_min_nodes(ptmi_ctx* c, int min_nodes, int* n_positions) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        need(min_nodes >= 0, "min_nodes must be >= 0");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        SceneState& s = c->app.scene;
        s.packed_min_nodes = min_nodes;
        if (s.d_nodes) { s.buildPacked(); s.chooseTraversal(); }
        if (n_positions) *n_positions = s.d_scene.n_pos;
    });
}

int ptmi_debug_set_packed_top(ptmi_ctx* c, int top_records, int* n_top, int* top_depth) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        need(top_records >= 0 && top_records <= 2048, "top_records must be in [0, 2048] (64 KB of LDS)");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        SceneState& s = c->app.scene;
        s.packed_top_records = top_records;
        if (s.d_nodes) { s.buildPacked(); s.chooseTraversal(); }
        if (n_top) *n_top = s.d_scene.n_top;
        if (top_depth) *top_depth = s.d_scene.top_depth;
    });
}

int ptmi_debug_set_fast_tree(ptmi_ctx* c, int max_leaf, float c_trav, float c_tri, int top_nodes, int* n_nodes, int* depth, int* n_top) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        need(max_leaf >= 1 && max_leaf <= kWideMaxLeaf, "max_leaf must be 1..3");
        need(c_trav >= 0.0f && c_tri > 0.0f, "c_trav must be >= 0 and c_tri > 0");
        need(top_nodes >= 0 && top_nodes <= 600, "top_nodes must be in [0, 600] (75 KB of LDS)");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        SceneState& s = c->app.scene;
        s.wide_params.max_leaf = max_leaf; s.wide_params.c_trav = c_trav; s.wide_params.c_tri = c_tri; s.wide_top_nodes = top_nodes;
        if (s.d_nodes) s.buildFast();
        if (n_nodes) *n_nodes = s.d_scene.w_nodes;
        if (depth) *depth = s.h_wide.depth;
        if (n_top) *n_top = s.d_scene.w_top;
    });
}

// ---- the walks, per ray ----
int ptmi_debug_intersect(ptmi_ctx* c, int n, const float* o, const float* d, float t_min, float t_max,
                         int* hit, int* prim, float* t, float* p, float* nrm) {
    return guarded([&] {
        need(c && o && d && hit && prim && t && p && nrm, "NULL argument");
        check_hook_rays(c, n, o, d);
        HookRun k(c);
        k.run([&](hipStream_t s) {
            launch_debug_intersect(c->app.scene.d_scene, n, k.in(o, 3 * (size_t)n), k.in(d, 3 * (size_t)n), t_min, t_max, k.out(hit, n), k.out(prim, n),
                                   k.out(t, n), k.out(p, 3 * (size_t)n), k.out(nrm, 3 * (size_t)n), s);
        });
    });
}

int ptmi_debug_intersect_fast(ptmi_ctx* c, int n, const float* o, const float* d, float t_min, float t_max,
                              int* hit, int* prim, float* t, uint64_t* counts) {
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the walk's counters are the caller's words");
    return guarded([&] {
        need(c && o && d && hit && prim && t, "NULL argument");
        check_hook_rays(c, n, o, d);
        HookRun k(c);
        if (!c->app.scene.fastReady()) c->app.scene.buildFast();
        k.run([&](hipStream_t s) {                     // the two counters start at zero; counts NULL: counted, not downloaded
            launch_debug_intersect_wide(c->app.scene.d_scene, n, k.in(o, 3 * (size_t)n), k.in(d, 3 * (size_t)n), t_min, t_max, k.out(hit, n),
                                        k.out(prim, n), k.out(t, n), k.out((unsigned long long*)counts, 2, 0), s);
        });
    });
}

int ptmi_debug_first_hit(ptmi_ctx* c, int n, const float* o, const float* d, float t_min, int* hit, int* prim, float* t) {
    return guarded([&] {
        need(c && o && d && hit && prim && t, "NULL argument");
        check_hook_rays(c, n, o, d);
        HookRun k(c);
        k.run([&](hipStream_t s) {
            launch_debug_first_hit(c->app.scene.d_scene, n, k.in(o, 3 * (size_t)n), k.in(d, 3 * (size_t)n), t_min, k.out(hit, n), k.out(prim, n), k.out(t, n), s);
        });
    });
}

// ---- the numerics contract and the shade step's short forms ----
int ptmi_debug_rng(ptmi_ctx* c, uint64_t seed_base, int n_pixels, const int* pixels, int count, float* out) {
    return guarded([&] {
        need(c && pixels && out, "NULL argument");
        need(n_pixels > 0 && count > 0, "n_pixels and count must be positive");
        HookRun k(c);
        k.run([&](hipStream_t s) {
            launch_debug_rng(c->app.render.d_jump, seed_base, n_pixels, k.in(pixels, n_pixels), count, k.out(out, (size_t)n_pixels * count), s);
        });
    });
}

int ptmi_debug_math(ptmi_ctx* c, int op, int n, const float* a, const float* b, double* out) {
    return guarded([&] {
        need(c && a && b && out, "NULL argument");
        need(n > 0, "n must be positive");
        need(op >= 0 && op < PTMI_MATH_OPS, "unknown op");
        HookRun k(c);
        k.run([&](hipStream_t s) { launch_debug_math(n, op, k.in(a, n), k.in(b, n), k.out(out, 2 * (size_t)n), s); });
    });
}

int ptmi_debug_rcp_check(ptmi_ctx* c, uint32_t first_bits, uint64_t count, uint64_t* mismatches, uint32_t* first_bad_bits) {
    return guarded([&] {
        need(c && mismatches && first_bad_bits, "NULL argument");
        run_bit_sweep(c, count, mismatches, first_bad_bits, [&](unsigned long long* d, hipStream_t s) { launch_debug_rcp(first_bits, count, d, s); });
    });
}

int ptmi_debug_sqrt_check(ptmi_ctx* c, uint32_t first_bits, uint64_t count, uint64_t* mismatches, uint32_t* first_bad_bits) {
    return guarded([&] {
        need(c && mismatches && first_bad_bits, "NULL argument");
        run_bit_sweep(c, count, mismatches, first_bad_bits, [&](unsigned long long* d, hipStream_t s) { launch_debug_sqrt(first_bits, count, d, s); });
    });
}

int ptmi_debug_size_div_check(ptmi_ctx* c, int size, uint32_t first_bits, uint64_t count, uint64_t* mismatches, uint32_t* first_bad_bits, int* lean) {
    return guarded([&] {
        need(c && mismatches && first_bad_bits && lean, "NULL argument");
        need(size >= 1, "size must be positive");
        const float inv = ptmi_size_reciprocal(size);                  // as RenderState::allocateBuffers takes TileMap's
        run_bit_sweep(c, count, mismatches, first_bad_bits,
                      [&](unsigned long long* d, hipStream_t s) { launch_debug_size_div((float)size, inv, first_bits, count, d, s); });
        *lean = inv != 0.0f ? 1 : 0;
    });
}

int ptmi_debug_sincos_lean_check(ptmi_ctx* c, uint32_t first_bits, uint64_t count, uint64_t* bad_sin, uint64_t* bad_cos,
                                 uint32_t* first_bad_bits, uint64_t* flagged, uint32_t* flagged_bits, int* n_flagged_bits) {
    return guarded([&] {
        need(c && bad_sin && bad_cos && first_bad_bits && flagged && flagged_bits && n_flagged_bits, "NULL argument");
        need(count > 0 && count <= (1ull << 32), "count must be in [1, 2^32]");
        HookRun k(c);
        unsigned long long h[13] = {0ull, 0ull, ~0ull};
        k.run([&](hipStream_t s) { launch_debug_sincos_lean_check(first_bits, count, k.inout(h, 13), s); });
        *bad_sin = h[0]; *bad_cos = h[1]; *first_bad_bits = (h[0] | h[1]) ? (uint32_t)h[2] : 0u; *flagged = h[3];
        *n_flagged_bits = (int)std::min<unsigned long long>(h[12], 8ull);
        for (int i = 0; i < 8; i++) flagged_bits[i] = i < *n_flagged_bits ? (uint32_t)h[4 + i] : 0u;
    });
}

int ptmi_debug_ray_inv(ptmi_ctx* c, int n, const float* d, const int* live, float* out_inv) {
    return guarded([&] {
        need(c && d && live && out_inv, "NULL argument");
        need(n > 0, "n must be positive");
        HookRun k(c);
        k.run([&](hipStream_t s) { launch_debug_ray_inv(n, k.in(d, 3 * (size_t)n), k.in(live, n), k.out(out_inv, 3 * (size_t)n), s); });
    });
}

int ptmi_debug_sincos_lean(ptmi_ctx* c, int n, const float* x, const int* live, float* out) {
    return guarded([&] {
        run_vote_hook(c, n, x, 1, live, out, 4, [&](const float* i, const int* l, float* o, hipStream_t s) { launch_debug_sincos_lean(n, i, l, o, s); });
    });
}
int ptmi_debug_unit_voted(ptmi_ctx* c, int n, const float* w, const int* live, float* out) {
    return guarded([&] {
        run_vote_hook(c, n, w, 3, live, out, 6, [&](const float* i, const int* l, float* o, hipStream_t s) { launch_debug_unit_voted(n, i, l, o, s); });
    });
}

// ---- the sampling functions, per call ----
int ptmi_debug_cosine_sample(ptmi_ctx* c, int n, const float* normals, const float* u, const float* v, float* out_dirs) {
    return guarded([&] {
        need(c && normals && u && v && out_dirs, "NULL argument");
        need(n > 0, "n must be positive");
        HookRun k(c);
        k.run([&](hipStream_t s) { launch_debug_cosine(n, k.in(normals, 3 * (size_t)n), k.in(u, n), k.in(v, n), k.out(out_dirs, 3 * (size_t)n), s); });
    });
}

int ptmi_debug_guided_sample(ptmi_ctx* c, int op, int n, int n_recs, const float* recs, const int* rec_idx, const float* normals,
                             const float* in3, const uint32_t* states, float* out, int* used) {
    return guarded([&] {
        need(c && normals && in3 && states && out && used, "NULL argument");
        need(n > 0, "n must be positive");
        need(op >= 0 && op <= 5, "op must be in [0, 5]");
        const bool grid = op >= 1 && op <= 3;
        if (grid) {
            need(recs && rec_idx && n_recs > 0, "ops 1-3 need CDF records and their indices");
            for (int i = 0; i < n; i++) need(rec_idx[i] >= 0 && rec_idx[i] < n_recs, "record index out of range");
        }
        HookRun k(c);
        k.run([&](hipStream_t s) {                     // the other ops read no record: nullptr for both
            launch_debug_guided(n, op, k.in(grid ? recs : nullptr, (size_t)n_recs * kCdfDwords), k.in(grid ? rec_idx : nullptr, n),
                                k.in(normals, 3 * (size_t)n), k.in(in3, 3 * (size_t)n), k.in(states, 6 * (size_t)n), k.out(out, 6 * (size_t)n), k.out(used, n), s);
        });
    });
}

int ptmi_debug_grid_index(ptmi_ctx* c, int n, const float* dirs, const float* normals, int* out) {
    return guarded([&] {
        need(c && dirs && normals && out, "NULL argument");
        need(n > 0, "n must be positive");
        HookRun k(c);
        k.run([&](hipStream_t s) { launch_debug_grid_index(n, k.in(dirs, 3 * (size_t)n), k.in(normals, 3 * (size_t)n), k.out(out, n), s); });
    });
}

int ptmi_debug_nee_call(ptmi_ctx* c, int op, int n, const float* in, float* out_f, int* out_i) {
    static_assert(kNeeCallIn == PTMI_NEE_CALL_IN && kNeeCallOutF == PTMI_NEE_CALL_OUT_F && kNeeCallOutI == PTMI_NEE_CALL_OUT_I, "ptmi.h and device_scene.h disagree");
    return guarded([&] {
        need(c && in && out_f && out_i, "NULL argument");
        need(n >= 0, "n must not be negative");
        need(op >= 0 && op < PTMI_NEE_CALL_OPS, "unknown op");
        const EnvTable ev = c->app.env.table(true, c->app.scene.d_emitters.n);
        if (op == PTMI_NEE_CALL_ENV_LOOKUP || op == PTMI_NEE_CALL_ENV_SAMPLE) need(ev.texel != nullptr, "the op needs an environment (ptmi_set_environment)");
        if (op == PTMI_NEE_CALL_EMITTER_SAMPLE) need(c->app.scene.d_emitters.n > 0, "the op needs a scene with an emitter");
        if (op == PTMI_NEE_CALL_ENV_LOOKUP)                   // (int)(NaN * w) is no column: the kernel never looks a non-finite direction up
            for (size_t i = 0; i < (size_t)n * kNeeCallIn; i += kNeeCallIn)
                need(std::isfinite(in[i]) && std::isfinite(in[i + 1]) && std::isfinite(in[i + 2]), "ENV_LOOKUP needs finite directions");
        if (n == 0) return;
        HookRun k(c);
        k.run([&](hipStream_t s) {
            launch_debug_nee_call(c->app.scene.d_scene.has_quads != 0, n, op, c->app.scene.d_emitters, ev, k.in(in, (size_t)n * kNeeCallIn),
                                  k.out(out_f, (size_t)n * kNeeCallOutF), k.out(out_i, (size_t)n * kNeeCallOutI), s);
        });
    });
}

// ---- the per-primitive tables, per call ----
int ptmi_debug_vertex_normal(ptmi_ctx* c, int n, const int* prim, const float* p, float* out) {
    return guarded([&] {
        check_hook_prims(c, n, prim, p, out);
        if (n == 0) return;
        const SceneState& sc = c->app.scene;
        if (!sc.hasVertexNormals()) {                         // no table: the kernel never calls the function
            for (int i = 0; i < n; i++) {
                const f3 s = sc.h_primitives[prim[i]].normal;
                out[4 * i] = s.x; out[4 * i + 1] = s.y; out[4 * i + 2] = s.z; out[4 * i + 3] = 0.0f;
            }
            return;
        }
        const std::vector<int> slots = leaf_slots(sc, n, prim);
        HookRun k(c);
        k.run([&](hipStream_t s) {
            launch_debug_vertex_normal(sc.d_scene, sc.vertexNormalTable(), n, k.in(slots.data(), n), k.in(p, 3 * (size_t)n), k.out(out, 4 * (size_t)n), s);
        });
    });
}

int ptmi_debug_albedo(ptmi_ctx* c, int n, const int* prim, const float* p, float* out) {
    return guarded([&] {
        check_hook_prims(c, n, prim, p, out);
        if (n == 0) return;
        const SceneState& sc = c->app.scene;
        if (!sc.hasAlbedoTexture()) {                         // no table: the kernel never calls the function
            for (int i = 0; i < n; i++) {
                out[6 * i] = out[6 * i + 1] = out[6 * i + 5] = 0.0f;
                out[6 * i + 2] = out[6 * i + 3] = out[6 * i + 4] = 1.0f;
            }
            return;
        }
        const std::vector<int> slots = leaf_slots(sc, n, prim);
        HookRun k(c);
        k.run([&](hipStream_t s) {
            launch_debug_albedo(sc.d_scene, sc.albedoTable(), n, k.in(slots.data(), n), k.in(p, 3 * (size_t)n), k.out(out, 6 * (size_t)n), s);
        });
    });
}

// ---- thin lens ----
int ptmi_debug_lens_block(ptmi_ctx* c, float* out24) {
    return guarded([&] {
        need(c && out24, "NULL argument");
        need(c->app.lens.on(), "no lens set (radius 0 is the pinhole)");
        need(c->app.render.tile.width > 0, "no resolution set");
        const float4* d = lensDeviceBlock(c->app);
        PTMI_HIP(hipMemcpy(out24, d, kLensBlockFloats * sizeof(float), hipMemcpyDeviceToHost));
    });
}
int ptmi_debug_lens_ray(ptmi_ctx* c, int n, const int* px, const int* py, const float* r, float* out) {
    return guarded([&] {
        need(c && px && py && r && out, "NULL argument");
        need(n >= 0, "n must not be negative");
        need(c->app.lens.on(), "no lens set (radius 0 is the pinhole)");
        need(c->app.render.tile.width > 0, "no resolution set");
        if (n == 0) return;
        HookRun k(c);
        const float4* lens = lensDeviceBlock(c->app);
        k.run([&](hipStream_t s) { launch_debug_lens_ray(lens, n, k.in(px, n), k.in(py, n), k.in(r, 4 * (size_t)n), k.out(out, 6 * (size_t)n), s); });
    });
}

// ---- participating medium ----
int ptmi_debug_medium_call(ptmi_ctx* c, int op, int n, const float* in, float* out) {
    static_assert(kMediumCallIn == PTMI_MEDIUM_CALL_IN && kMediumCallOut == PTMI_MEDIUM_CALL_OUT && kMediumBlockFloats == PTMI_MEDIUM_BLOCK_FLOATS,
                  "ptmi.h, device_scene.h and medium.h disagree");
    return guarded([&] {
        need(c && in && out, "NULL argument");
        need(op >= 0 && op <= 3, "op must be 0 .. 3");
        need(n >= 0, "n must not be negative");
        if (n == 0) return;
        HookRun k(c);
        k.run([&](hipStream_t s) { launch_debug_medium_call(n, op, k.in(in, (size_t)n * kMediumCallIn), k.out(out, (size_t)n * kMediumCallOut), s); });
    });
}

// ---- multi-GPU frame exchange: the placement of gathered tiles ----
int ptmi_debug_place_tiles(ptmi_ctx* c, int width, int height, int n_ranks, int row_block, const unsigned char* tiles_rgb8,
                           const float* tiles_radiance, unsigned char* out_rgb8, float* out_radiance) {
    return guarded([&] {
        need(c != nullptr, "ctx is NULL");
        PTMI_HIP(hipSetDevice(c->app.device_id));
        debugPlaceTiles(width, height, n_ranks, row_block, tiles_rgb8, tiles_radiance, out_rgb8, out_radiance, c->app.render.stream);
    });
}

// ---- the filters' inputs and the history's statistics, given instead of rendered or accumulated ----
int ptmi_debug_set_temporal_moments(ptmi_ctx* c, const float* mean, const float* variance, const float* frames) {
    return guarded([&] { need(c && mean && variance && frames, "NULL argument"); debugSetTemporalMoments(c->app, mean, variance, frames); });
}
int ptmi_debug_set_filter_inputs(ptmi_ctx* c, const float* radiance, const float* albedo, const float* normal, const float* position,
                                 const float* hit_fraction, int grid) {
    return guarded([&] {
        need(c && radiance && albedo && normal && position && hit_fraction, "NULL argument");
        debugSetFilterInputs(c->app, radiance, albedo, normal, position, hit_fraction, grid);
    });
}

// ---- the accumulation's stopping test and resolve, and the launch order by cost, on given state ----
int ptmi_debug_accum_step(ptmi_ctx* c, const float* sums, const float* prev, const float* m2, const uint32_t* passes, const int* queue,
                          int n_queue, const ptmi_adaptive_params* params, int first, int* queue_out, int* n_out) {
    return guarded([&] {
        need(c && sums && prev && m2 && passes && queue_out && n_out, "NULL argument");
        AdaptiveParams prm;
        if (params) { prm.min_passes = params->min_passes; prm.max_passes = params->max_passes; prm.threshold = params->threshold; prm.floor = params->floor; }
        *n_out = debugAccumStep(c->app, sums, prev, m2, passes, queue, n_queue, params ? &prm : nullptr, first != 0, queue_out);
    });
}
int ptmi_debug_order_by_cost(ptmi_ctx* c, int n, const int* queue_in, const uint32_t* cost, int n_cost, uint32_t cost_max, int classes,
                             int* queue_out, int* hist) {
    return guarded([&] {
        need(c && cost && queue_out && hist, "NULL argument");
        need(n > 0 && n_cost > 0, "n and n_cost must be positive");
        need(classes >= 1, "classes must be positive");
        need(queue_in != nullptr || n <= n_cost, "the identity queue needs n <= n_cost");
        if (queue_in) for (int i = 0; i < n; i++) need(queue_in[i] >= 0 && queue_in[i] < n_cost, "a queue entry lies outside cost[]");
        HookRun k(c);
        k.run([&](hipStream_t s) {                     // queue_in NULL: the identity queue; a position the pass does not write reads -1
            launch_order_by_cost(k.in(queue_in, n), n, k.in(cost, n_cost), k.in(&cost_max, 1), k.out(hist, 512), k.out(queue_out, n, 0xff), classes, s);
        });
    });
}

// ---- the guided-record kernels (csrc/radiosity.hip) on given grids and form factors ----
int ptmi_debug_cdf_records(ptmi_ctx* c, int n, int src_kind, const float* src, float* out) {
    return guarded([&] {
        need(c && src && out, "NULL argument");
        need(n >= 1, "n must be positive");
        need(src_kind >= 0 && src_kind <= 2, "src_kind must be 0, 1 or 2");
        HookRun k(c);
        const size_t per = (size_t)kGridSize * (src_kind == 0 ? 4 : src_kind == 1 ? 3 : 1);
        k.run([&](hipStream_t s) { launch_cdf_records(n, k.in(src, per * n), src_kind, k.out(out, (size_t)n * kCdfDwords), s); });
    });
}
int ptmi_debug_filter_pdfs(ptmi_ctx* c, int n, const float* rgb, const float* counts, int use_bilateral, float sigma_spatial,
                           float sigma_range, float* out_formfactor, float* out_radiosity) {
    return guarded([&] {
        need(c && rgb && out_formfactor && out_radiosity, "NULL argument");
        need(n >= 1, "n must be positive");
        HookRun k(c);
        const size_t cells = (size_t)n * kGridSize;
        k.run([&](hipStream_t s) {                     // counts NULL: no form-factor grids
            launch_filter_pdfs(n, k.in(rgb, 3 * cells), k.in(counts, cells), k.out(out_formfactor, cells), k.out(out_radiosity, cells), use_bilateral != 0,
                               sigma_spatial, sigma_range, s);
        });
    });
}
int ptmi_debug_radiosity_grid(ptmi_ctx* c, int n, const float* centre, const float* normal, const float* form_factors,
                              const float* radiosity, int enable_filtering, int use_bilateral, float sigma_spatial, float sigma_range,
                              float* out) {
    return guarded([&] {
        need(c && centre && normal && form_factors && radiosity && out, "NULL argument");
        need(n >= 1, "n must be positive");
        HookRun k(c);
        const size_t cells = (size_t)n * kGridSize;
        // geo: only the normal [4] and the centroid [5] of each primitive's six records are read by the kernel
        std::vector<float4> h_geo(6 * (size_t)n, make_float4(0.0f, 0.0f, 0.0f, 0.0f)), h_rad(n), h_grid(cells);
        for (int i = 0; i < n; i++) {
            h_geo[6 * (size_t)i + 4] = make_float4(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], 0.0f);
            h_geo[6 * (size_t)i + 5] = make_float4(centre[3 * i], centre[3 * i + 1], centre[3 * i + 2], 0.0f);
            h_rad[i] = make_float4(radiosity[3 * i], radiosity[3 * i + 1], radiosity[3 * i + 2], 0.0f);
        }
        RadiosityBuffers rb;                            // the solver's struct, which writes two of the buffers this kernel reads
        rb.geo = k.in(h_geo.data(), h_geo.size()); rb.radiosity = const_cast<float4*>(k.in(h_rad.data(), h_rad.size()));
        rb.form_factors = const_cast<float*>(k.in(form_factors, (size_t)n * n)); rb.rad_grid = k.out(h_grid.data(), cells); rb.n = n;
        RadiosityParams prm{};
        prm.enable_filtering = enable_filtering != 0; prm.use_bilateral = use_bilateral != 0;
        prm.filter_sigma_spatial = sigma_spatial; prm.filter_sigma_range = sigma_range;
        k.run([&](hipStream_t s) { launch_radiosity_grid(rb, prm, s); });
        for (size_t i = 0; i < cells; i++) { out[3 * i] = h_grid[i].x; out[3 * i + 1] = h_grid[i].y; out[3 * i + 2] = h_grid[i].z; }
    });
}

}  // extern "C"
