// render_state.cpp — what a context owns besides its scene: RenderState's buffers and chunks, the environment light, the
// XORWOW jump matrices, the tiling, and ApplicationState itself.  The launches are render_run.cpp's.
#include "application_state.h"
#include "../csrc/shade_lean.h"

#include <algorithm>
#include <cstring>

namespace ptmi {

void* hipMallocSafe(size_t bytes, const char* name) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e != hipSuccess) throw HipError(e, std::string("hipMalloc(") + name + ", " + std::to_string(bytes) + " B): " + hipGetErrorString(e));
    return p;
}

// ------------------------------------------------------------------------------------------------
// XORWOW skip-ahead matrices
// ------------------------------------------------------------------------------------------------
namespace {
using Mat = std::vector<uint32_t>;   // 160 rows x 5 words; row b = image of basis state bit b
void stepV(uint32_t v[5]) {
    const uint32_t t = v[0] ^ (v[0] >> 2);
    v[0] = v[1]; v[1] = v[2]; v[2] = v[3]; v[3] = v[4];
    v[4] = (v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1));
}
void apply(const Mat& m, const uint32_t* in, uint32_t* out) {
    uint32_t r[5] = {0, 0, 0, 0, 0};
    for (int b = 0; b < 160; b++)
        if ((in[b >> 5] >> (b & 31)) & 1u) for (int c = 0; c < 5; c++) r[c] ^= m[b * 5 + c];
    std::memcpy(out, r, sizeof r);
}
Mat square(const Mat& m) {
    Mat s(160 * 5);
    for (int b = 0; b < 160; b++) apply(m, &m[b * 5], &s[b * 5]);
    return s;
}
}  // namespace

std::vector<uint32_t> buildXorwowJumpMatrices() {
    Mat m(160 * 5);
    for (int b = 0; b < 160; b++) {
        uint32_t v[5] = {0, 0, 0, 0, 0};
        v[b >> 5] = 1u << (b & 31);
        stepV(v);
        std::memcpy(&m[b * 5], v, sizeof v);
    }
    for (int s = 0; s < 67; s++) m = square(m);          // one subsequence = 2^67 draws
    std::vector<uint32_t> all;
    all.reserve(kXorwowJumpWords);
    for (int k = 0; k < 32; k++) {
        all.insert(all.end(), m.begin(), m.end());
        if (k != 31) m = square(m);
    }
    return all;
}

// ------------------------------------------------------------------------------------------------
// tiling
// ------------------------------------------------------------------------------------------------
int countLocalRows(int height, int n_ranks, int rank, int row_block) {
    int rows = 0;
    for (int y0 = rank * row_block; y0 < height; y0 += n_ranks * row_block) rows += std::min(row_block, height - y0);
    return rows;
}
std::vector<int> localRowMap(const TileMap& tm) {
    std::vector<int> rows;
    for (int y0 = tm.rank * tm.row_block; y0 < tm.height; y0 += tm.n_ranks * tm.row_block)
        for (int y = y0; y < std::min(y0 + tm.row_block, tm.height); y++) rows.push_back(y);
    return rows;
}

// ------------------------------------------------------------------------------------------------
// RenderState
// ------------------------------------------------------------------------------------------------
void RenderState::freeBuffers() {
    void* ptrs[] = {d_state.A, d_state.B, d_state.C, d_state.D, d_state.E, d_state.F, d_image, d_radiance, d_stats, d_frame_color,
                    d_cost[0], d_cost[1], d_cost_max, d_cost_hist, d_queue_ordered};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    d_cost[0] = d_cost[1] = nullptr; d_cost_max = nullptr; d_cost_hist = nullptr; d_queue_ordered = nullptr; cost_valid = false; cost_frame = 0;
    d_frame_color = nullptr; frame_color_frames = 0; batch_frames = 1; batch_spp = 0;
    if (h_image) { (void)hipHostFree(h_image); h_image = nullptr; }
    freeChunks();
    freeAccum();
    freeDenoise();
    freeTemporal();
    d_state = PathState();
    d_image = nullptr; d_radiance = nullptr; d_stats = nullptr;
    n_local = 0;
}

void RenderState::freeChunks() {
    for (Chunk& c : chunk) c.release();
    n_chunks = 0;
}

// The device side of one queue: the two bounce queues of `capacity` entries, the count ring and its host slots; with
// own_init_queue the first queue too (a chunk of the frame; a pass's d_queue_init points at the pass's queue)
void RenderState::Chunk::allocate(size_t capacity, bool own_init_queue) {
    const size_t cap = std::max<size_t>(capacity, 1) * sizeof(int);
    const std::string who = own_init_queue ? "chunk" : "accum";      // the names hipMallocSafe reports
    owns_init_queue = own_init_queue;
    if (own_init_queue) d_queue_init = (int*)hipMallocSafe(cap, "chunk.queue_init");
    d_queue[0] = (int*)hipMallocSafe(cap, (who + ".queue0").c_str());
    d_queue[1] = (int*)hipMallocSafe(cap, (who + ".queue1").c_str());
    // per ring slot i: [4 i] the launch's output count, [4 i + 1] its refill cursor, [4 i + 2] its finished pixels; [4 kCountRing]: the launch's arrival counter
    d_count = (int*)hipMallocSafe((4 * kCountRing + 1) * sizeof(int), (who + ".count").c_str());
    PTMI_HIP(hipMemset(d_count, 0, (4 * kCountRing + 1) * sizeof(int)));
    // coherent (fine-grained) host memory: with count publishing the device stores into it while the kernel runs
    PTMI_HIP(hipHostMalloc((void**)&h_count, kCountRing * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
    PTMI_HIP(hipHostGetDevicePointer((void**)&d_hcount, h_count, 0));
}

void RenderState::Chunk::release() {                 // (the stream stays: it belongs to the context)
    void* cp[] = {owns_init_queue ? d_queue_init : nullptr, d_queue[0], d_queue[1], d_count};
    for (void* p : cp) if (p) (void)hipFree(p);
    if (h_count) (void)hipHostFree(h_count);
    d_queue_init = d_queue[0] = d_queue[1] = d_count = nullptr; h_count = nullptr; d_hcount = nullptr; n = 0;
}

// chunks: 256-slot blocks dealt round-robin, so a workgroup still reads 256 consecutive state records
void RenderState::setupChunks(int n) {
    freeChunks();
    n_chunks = std::max(1, std::min(n, (int)kMaxChunks));
    std::vector<std::vector<int>> slots(n_chunks);
    for (size_t b = 0; b * kBlock < n_local; b++) {
        std::vector<int>& v = slots[b % n_chunks];
        for (size_t i = b * kBlock; i < std::min(n_local, (b + 1) * (size_t)kBlock); i++) v.push_back((int)i);
    }
    for (int c = 0; c < n_chunks; c++) {
        Chunk& ch = chunk[c];
        ch.n = (int)slots[c].size();
        ch.allocate(slots[c].size(), true);
        if (ch.n) PTMI_HIP(hipMemcpy(ch.d_queue_init, slots[c].data(), slots[c].size() * sizeof(int), hipMemcpyHostToDevice));
    }
}

void RenderState::freeAccum() {
    Accum& a = accum;
    void* ptrs[] = {a.d_active[0], a.d_active[1], a.ab.prev, a.ab.m2, a.ab.passes, a.d_counts, a.d_out_count};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    a.chunk.release();
    a = Accum();
}

void RenderState::freeDenoise() {
    void* ptrs[] = {dn.fb.albedo, dn.fb.normal, dn.fb.position, dn.d_rgb8, dn.d_radiance, dn.d_buf, dn.d_var_in, dn.d_var_out, dn.d_owned};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    dn = Denoise();
}

void RenderState::freeTemporal() {
    void* ptrs[] = {tp.side[0].color, tp.side[0].normal, tp.side[0].position, tp.side[0].albedo, tp.side[1].color, tp.side[1].normal,
                    tp.side[1].position, tp.side[1].albedo, tp.d_rgb8, tp.d_radiance, tp.d_stats, tp.moments[0], tp.moments[1]};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    tp = Temporal();
}

void RenderState::allocateAccum() {
    freeAccum();
    Accum& a = accum;
    try {
        const size_t n = std::max<size_t>(n_local, 1);
        for (int k = 0; k < 2; k++) a.d_active[k] = (int*)hipMallocSafe(n * sizeof(int), "accum.active");
        a.ab.prev = (float4*)hipMallocSafe(n * sizeof(float4), "accum.prev");
        a.ab.m2 = (float*)hipMallocSafe(n * sizeof(float), "accum.m2");
        a.ab.passes = (unsigned int*)hipMallocSafe(n * sizeof(unsigned int), "accum.passes");
        a.d_out_count = (int*)hipMallocSafe(sizeof(int), "accum.out_count");
        a.chunk.allocate(n, false);
        a.d_counts = (unsigned int*)hipMallocSafe(n * sizeof(unsigned int), "accum.counts");   // last: allocated() means complete
    } catch (...) { freeAccum(); throw; }
}

void RenderState::allocateBuffers() {
    freeBuffers();
    tile.width = width; tile.height = height;
    tile.inv_width = ptmi_size_reciprocal(width); tile.inv_height = ptmi_size_reciprocal(height);
    if (tile.inv_width == 0.0f || tile.inv_height == 0.0f) tile.inv_width = tile.inv_height = 0.0f;      // one flag for both
    tile.local_rows = countLocalRows(height, tile.n_ranks, tile.rank, tile.row_block);
    n_local = (size_t)tile.local_rows * (size_t)width;
    tile.tile8 = (allow_tile8 && width % 8 == 0 && tile.local_rows % 8 == 0 && tile.row_block % 8 == 0) ? 1 : 0;
    const size_t n = std::max<size_t>(n_local, 1);
    d_state.A = (float4*)hipMallocSafe(n * sizeof(float4), "state.A");
    d_state.B = (float4*)hipMallocSafe(n * sizeof(float4), "state.B");
    d_state.C = (float4*)hipMallocSafe(n * sizeof(float4), "state.C");
    d_state.D = (float4*)hipMallocSafe(n * sizeof(float4), "state.D");
    d_state.E = (uint4*)hipMallocSafe(n * sizeof(uint4), "state.E");
    d_state.F = (uint2*)hipMallocSafe(n * sizeof(uint2), "state.F");
    d_image = (unsigned char*)hipMallocSafe(n * 3, "d_image");
    d_radiance = (float*)hipMallocSafe(n * 3 * sizeof(float), "d_radiance");
    d_stats = (StatCounters*)hipMallocSafe(sizeof(StatCounters), "d_stats");
    for (int k = 0; k < 2; k++) d_cost[k] = (unsigned int*)hipMallocSafe(n * sizeof(unsigned int), "d_cost");
    d_cost_max = (unsigned int*)hipMallocSafe(2 * sizeof(unsigned int), "d_cost_max");
    d_cost_hist = (int*)hipMallocSafe(512 * sizeof(int), "d_cost_hist");
    d_queue_ordered = (int*)hipMallocSafe(n * sizeof(int), "d_queue_ordered");
    PTMI_HIP(hipHostMalloc((void**)&h_image, n * 3));                     // h_image = new unsigned char[img_size], application_state.h:99
    setupChunks(want_chunks > 0 ? std::min(want_chunks, (int)kMaxChunks) : (n_local >= (size_t)(1 << 18) ? 2 : 1));

    // camera: image size + aspect, then updateCamera (application_state.h:106-109)
    h_camera.image_width = width; h_camera.image_height = height;
    h_camera.aspect = (float)width / (float)height;
    h_camera.updateCamera();

    // render_init (application_state.h:120-122): streams are re-seeded on every (re)allocation
    launch_render_init(tile, d_state, d_jump, seed_base, stream);
    PTMI_HIP(hipGetLastError());
    PTMI_HIP(hipStreamSynchronize(stream));
}

void RenderState::updateResolution(int w, int h, const TileMap* tiling) {
    if (w <= 0 || h <= 0) throw ArgError("width and height must be positive");
    if ((long long)w * h > (1ll << 31) - 1) throw ArgError("frame has more than 2^31-1 pixels");
    if (tiling) {
        if (tiling->n_ranks < 1 || tiling->rank < 0 || tiling->rank >= tiling->n_ranks || tiling->row_block < 1)
            throw ArgError("bad tiling (need n_ranks >= 1, 0 <= rank < n_ranks, row_block >= 1)");
        tile.n_ranks = tiling->n_ranks; tile.rank = tiling->rank; tile.row_block = tiling->row_block;
    } else { tile.n_ranks = 1; tile.rank = 0; tile.row_block = 8; }
    width = w; height = h;
    allocateBuffers();
}

// ------------------------------------------------------------------------------------------------
// ApplicationState
// ------------------------------------------------------------------------------------------------
ApplicationState::ApplicationState(int device) : device_id(device) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) throw HipError(e == hipSuccess ? hipErrorNoDevice : e, "no HIP device available (libptmi has no CPU fallback)");
    if (device < 0 || device >= count) throw ArgError("device_id out of range");
    PTMI_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    PTMI_HIP(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        throw HipError(hipErrorInvalidDevice, std::string("libptmi is built for gfx950 only; device is ") + prop.gcnArchName);
    n_cus = prop.multiProcessorCount;
    PTMI_HIP(hipStreamCreateWithFlags(&render.stream, hipStreamNonBlocking));
    for (RenderState::Chunk& c : render.chunk) PTMI_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    h_jump = buildXorwowJumpMatrices();
    render.d_jump = (uint32_t*)hipMallocSafe(h_jump.size() * sizeof(uint32_t), "d_jump");
    PTMI_HIP(hipMemcpy(render.d_jump, h_jump.data(), h_jump.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    render.h_camera = Sensor(config.camera_origin, config.look_at, config.up, config.fov, 1.0f);   // application.h:107-113
}

ApplicationState::~ApplicationState() {
    (void)hipSetDevice(device_id);
    render.resolve_gate = nullptr;
    dist.finalize();
    for (hipEvent_t ev : event_pool) (void)hipEventDestroy(ev);
    scene.cleanup();
    env.drop();
    render.freeBuffers();
    if (render.d_jump) (void)hipFree(render.d_jump);
    if (render.stream) (void)hipStreamDestroy(render.stream);
    for (RenderState::Chunk& c : render.chunk) if (c.stream) (void)hipStreamDestroy(c.stream);
}

// ---- environment lighting (include/ptmi.h: ptmi_set_environment) ----------------------------------------------------------
void EnvState::set(int width, int height, const float* rgb, const EnvParams& p) {
    EnvHostTable t;
    buildEnvTable(width, height, rgb, p, t);           // throws ArgError: nothing has changed yet
    const size_t n = (size_t)width * (size_t)height;
    float* nz = (float*)hipMallocSafe(t.z.size() * sizeof(float), "d_env_z");
    float* nm = nullptr; float* nc = nullptr; float4* nt = nullptr;
    try {
        nm = (float*)hipMallocSafe(t.marginal.size() * sizeof(float), "d_env_marginal");
        nc = (float*)hipMallocSafe(n * sizeof(float), "d_env_row_cdf");
        nt = (float4*)hipMallocSafe(n * sizeof(float4), "d_env_texel");
        PTMI_HIP(hipMemcpy(nz, t.z.data(), t.z.size() * sizeof(float), hipMemcpyHostToDevice));
        PTMI_HIP(hipMemcpy(nm, t.marginal.data(), t.marginal.size() * sizeof(float), hipMemcpyHostToDevice));
        PTMI_HIP(hipMemcpy(nc, t.row_cdf.data(), n * sizeof(float), hipMemcpyHostToDevice));
        PTMI_HIP(hipMemcpy(nt, t.texel.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    } catch (...) {
        (void)hipFree(nz); if (nm) (void)hipFree(nm); if (nc) (void)hipFree(nc); if (nt) (void)hipFree(nt);
        throw;
    }
    drop();
    d_z = nz; d_marginal = nm; d_row_cdf = nc; d_texel = nt;
    params = p;
    h = std::move(t);
}

void EnvState::drop() {
    if (d_z) (void)hipFree(d_z);
    if (d_marginal) (void)hipFree(d_marginal);
    if (d_row_cdf) (void)hipFree(d_row_cdf);
    if (d_texel) (void)hipFree(d_texel);
    d_z = d_marginal = d_row_cdf = nullptr; d_texel = nullptr;
    h = EnvHostTable(); params = EnvParams();
}

EnvTable EnvState::table(bool next_event, int n_emitters) const {
    EnvTable e;
    if (!present()) return e;
    e.z = d_z; e.marginal = d_marginal; e.row_cdf = d_row_cdf; e.texel = d_texel;
    e.w = h.width; e.h = h.height; e.rot = h.rot_turns;
    e.sampled = next_event && h.total > 0.0f ? 1 : 0;
    e.q = n_emitters == 0 ? 1.0f : params.select_fraction;     // (total == 0: not sampled, q is not read)
    return e;
}

// camera update (application.h:161-163) and the camera fields of the frame's parameters
void cameraFrameParams(ApplicationState& g, FrameParams& fp) {
    RenderState& r = g.render;
    if (g.config.orbit) r.h_camera.updateCameraOrbit(); else r.h_camera.updateCamera();
    const CameraFrame cf = r.h_camera.frame();
    const float eye[3] = {cf.origin.x, cf.origin.y, cf.origin.z};
    g.scene.checkQuadOrigin(eye, nullptr, "camera");             // the quad test's products must not overflow (SceneState::upload)
    const f3* src[4] = {&cf.origin, &cf.lower_left_corner, &cf.horizontal, &cf.vertical};
    float* dst[4] = {fp.cam_origin, fp.cam_llc, fp.cam_hor, fp.cam_ver};
    for (int i = 0; i < 4; i++) { dst[i][0] = src[i]->x; dst[i][1] = src[i]->y; dst[i][2] = src[i]->z; }
}


// ---- thin lens (include/ptmi.h: ptmi_set_lens) --------------------------------------------------------------------------------
LensState::~LensState() { if (d_block) (void)hipFree(d_block); }

float lensFocus(const ApplicationState& g) { return g.lens.focus > 0.0f ? g.lens.focus : g.render.h_camera.radius; }

const float4* lensDeviceBlock(ApplicationState& g) {
    LensState& l = g.lens;
    if (!l.on()) return nullptr;
    float frame[12], block[kLensBlockFloats];
    cameraFrame12(g.render.h_camera, g.config.orbit, frame);     // what cameraFrameParams derives
    lensBlock(frame, g.render.tile.width, g.render.tile.height, l.radius, lensFocus(g), block);
    PTMI_HIP(hipSetDevice(g.device_id));
    if (!l.d_block) { l.d_block = (float4*)hipMallocSafe(sizeof block, "d_lens"); l.uploaded = false; }
    if (!l.uploaded || std::memcmp(block, l.h_block, sizeof block) != 0) {
        PTMI_HIP(hipMemcpy(l.d_block, block, sizeof block, hipMemcpyHostToDevice));
        std::memcpy(l.h_block, block, sizeof block);
        l.uploaded = true;
    }
    return l.d_block;
}

// ---- participating medium (include/ptmi.h: ptmi_set_medium) ---------------------------------------------------------------------
MediumState::~MediumState() { if (d_block) (void)hipFree(d_block); }

const float4* mediumDeviceBlock(ApplicationState& g) {
    MediumState& s = g.scene.medium;
    if (!s.on()) return nullptr;
    float block[kMediumBlockFloats];
    mediumBlock(s.m, block);
    PTMI_HIP(hipSetDevice(g.device_id));
    if (!s.d_block) { s.d_block = (float4*)hipMallocSafe(sizeof block, "d_medium"); s.uploaded = false; }
    if (!s.uploaded || std::memcmp(block, s.h_block, sizeof block) != 0) {
        PTMI_HIP(hipMemcpy(s.d_block, block, sizeof block, hipMemcpyHostToDevice));
        std::memcpy(s.h_block, block, sizeof block);
        s.uploaded = true;
    }
    return s.d_block;
}

}  // namespace ptmi
