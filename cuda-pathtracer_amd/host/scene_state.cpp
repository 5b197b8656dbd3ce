// scene_state.cpp — SceneState: host loading, the emitter table, upload, and the packed / fast layouts
#include "application_state.h"
#include "../csrc/sweep_near_far.h"
#include "../csrc/sweep_leaves.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <limits>

namespace ptmi {

// ------------------------------------------------------------------------------------------------
// SceneState
// ------------------------------------------------------------------------------------------------
void SceneState::cleanup() {
    if (d_nodes) (void)hipFree(d_nodes);
    if (d_prims) (void)hipFree(d_prims);
    if (d_mats) (void)hipFree(d_mats);
    if (d_precomputed_cdfs) (void)hipFree(d_precomputed_cdfs);
    if (d_radiosity) (void)hipFree(d_radiosity);
    if (d_emit_rec) (void)hipFree(d_emit_rec);
    if (d_emit_cdf) (void)hipFree(d_emit_cdf);
    if (d_pdf_area) (void)hipFree(d_pdf_area);
    if (d_surfaces) (void)hipFree(d_surfaces);
    d_surfaces = nullptr; n_mirror = n_glass = 0;
    for (int& c : surface_counts) c = 0;
    if (d_vertex_normals) (void)hipFree(d_vertex_normals);
    d_vertex_normals = nullptr; n_smooth = 0;
    if (d_albedo_rec) (void)hipFree(d_albedo_rec);
    if (d_albedo_texels) (void)hipFree(d_albedo_texels);
    d_albedo_rec = d_albedo_texels = nullptr; n_textured = tex_width = tex_height = tex_filter = 0;
    medium.drop();
    d_emit_rec = d_pdf_area = nullptr; d_emit_cdf = nullptr; d_emitters = EmitterTable();
    h_emit_prim.clear(); h_emit_cdf.clear(); h_emit_normal.clear(); h_pdf_area.clear(); h_emit_total = 0.0f;
    freePacked();
    freeFast();
    fast_declined = false;
    d_nodes = d_prims = d_mats = nullptr; d_precomputed_cdfs = nullptr; d_radiosity = nullptr;
    h_precomputed_cdfs.clear(); h_radiosity_grids.clear(); h_count_grids.clear(); h_filtered_formfactor.clear(); h_filtered_radiosity.clear();
    d_scene = DeviceScene();
    h_primitives.clear(); bvh_nodes.clear(); bvh_indices.clear();
    num_tris = num_quads = 0; bvh_depth = 0;
}

void SceneState::loadScene(const std::string& filename, int subdivision_count, bool convert_quads) {
    loadSceneHost(filename, subdivision_count, convert_quads);
    upload();
}

void SceneState::loadSceneArrays(std::vector<Primitive> prims) {
    loadSceneArraysHost(std::move(prims));
    upload();
}

void SceneState::loadSceneHost(const std::string& filename, int subdivision_count, bool convert_quads) {
    cleanup();
    const size_t dot = filename.find_last_of('.');
    if (dot == std::string::npos) throw IoError("unsupported file format (no extension): " + filename);
    std::string ext = filename.substr(dot);
    std::transform(ext.begin(), ext.end(), ext.begin(), [](unsigned char c) { return (char)std::tolower(c); });
    std::vector<Primitive> prims;
    if (ext == ".obj") {
        if (!loadOBJ(filename, prims)) throw IoError("failed to load scene: " + filename);
    } else if (ext == ".pbrt") {                                                    // USE_PBRT_LOADER, application_state.h:385-388
        std::string why;
        if (!loadPBRT(filename, prims, &why)) throw IoError("failed to load scene: " + filename + " (" + why + ")");
    } else throw IoError("unsupported file format: " + ext);
    if (convert_quads) prims = convertQuadsToTriangles(prims);
    if (subdivision_count > 0) prims = subdivide_primitives(prims, subdivision_count);
    h_primitives.swap(prims);
    scene_file = filename;
    buildBVH();
    buildEmitters();
}

void SceneState::loadSceneArraysHost(std::vector<Primitive> prims) {
    cleanup();
    if (prims.empty()) throw ArgError("scene has no primitives");
    h_primitives.swap(prims);
    scene_file = "<arrays>";
    buildBVH();
    buildEmitters();
}

// The geometric normal of include/ptmi.h's emitter table: unit_vector(cross(e1, e2)) of the triangle's (v1 - v0, v2 - v0) or the
// quad's (v10 - v00, v01 - v00)
static f3 emitterNormal(const Primitive& p) {
    return unit_vector(cross(p.v[1] - p.v[0], (p.type == PRIM_QUAD ? p.v[3] : p.v[2]) - p.v[0]));
}

// The emitter table of next-event estimation in the order of include/ptmi.h.  Candidates: a finite geometric normal, a quad only
// if planar.  Float32: w = area * ((Le.x + Le.y) + Le.z) > 0, running sums c_j from +0 that skip a weight the sum absorbs
// (c + w == c), pdf_area = (w / total) / area.  Where a weight or the sum overflows float, the same in binary64, normalised to a
// total of 1, skipping the entries that round to the one before.
void SceneState::buildEmitters() {
    const int n = (int)h_primitives.size();
    h_emit_prim.clear(); h_emit_cdf.clear(); h_emit_normal.clear();
    h_pdf_area.assign((size_t)n, 0.0f);
    h_emit_total = 0.0f;
    std::vector<int> cand;
    for (int i = 0; i < n; i++) {
        const Primitive& p = h_primitives[i];
        const f3 ng = emitterNormal(p);
        if (!std::isfinite(ng.x) || !std::isfinite(ng.y) || !std::isfinite(ng.z)) continue;
        if (p.type == PRIM_QUAD) {                   // the walk splits a quad along v00-v11, sampleUniform along v10-v01
            const f3 diag = p.v[2] - p.v[0];
            if (!(fabsf(dot(ng, diag)) <= 1e-4f * length(diag))) continue;
        }
        cand.push_back(i);
    }
    std::vector<float> w_of;
    float c = 0.0f;
    bool overflow = false;
    for (int i : cand) {
        const Primitive& p = h_primitives[i];
        const float w = p.area() * ((p.Le.x + p.Le.y) + p.Le.z);
        if (!(w > 0.0f)) continue;
        if (!(w <= FLT_MAX) || !(c + w <= FLT_MAX)) { overflow = true; break; }
        if (!(c + w > c)) continue;                  // absorbed: select() could never return it
        c = c + w;
        h_emit_prim.push_back(i); h_emit_cdf.push_back(c); w_of.push_back(w);
    }
    if (!overflow) {
        h_emit_total = c;
        for (size_t j = 0; j < h_emit_prim.size(); j++) {
            const int i = h_emit_prim[j];
            h_pdf_area[i] = (w_of[j] / c) / h_primitives[i].area();
        }
    } else {
        h_emit_prim.clear(); h_emit_cdf.clear();
        std::vector<int> pos;
        std::vector<double> wd, cd;
        double t = 0.0;
        for (int i : cand) {
            const Primitive& p = h_primitives[i];
            const double w = (double)p.area() * (((double)p.Le.x + (double)p.Le.y) + (double)p.Le.z);
            if (!(w > 0.0) || !std::isfinite(w)) continue;
            t = t + w;
            pos.push_back(i); wd.push_back(w); cd.push_back(t);
        }
        float prev = 0.0f;
        for (size_t k = 0; k < pos.size(); k++) {
            const float cdf = (float)(cd[k] / t);
            if (!(cdf > prev)) continue;             // absorbed
            const int i = pos[k];
            h_pdf_area[i] = (float)((wd[k] / t) / (double)h_primitives[i].area());
            h_emit_prim.push_back(i); h_emit_cdf.push_back(cdf);
            prev = cdf;
        }
        h_emit_total = h_emit_prim.empty() ? 0.0f : 1.0f;     // the last entry is C / C = 1
    }
    for (int i : h_emit_prim) h_emit_normal.push_back(emitterNormal(h_primitives[i]));
}

void SceneState::buildBVH() {
    const int n = (int)h_primitives.size();
    BVHBuilder builder(h_primitives.data(), n);
    bvh_nodes = builder.nodes;
    bvh_indices = builder.primitive_indices;
    bvh_depth = builder.max_depth;
    num_tris = num_quads = 0;
    for (const Primitive& p : h_primitives) (p.type == PRIM_TRIANGLE ? num_tris : num_quads)++;
}

// What the device's arithmetic asks of a scene; throws ArgError.  Called by upload(), and by the host-only scene's check
// (ptmi_host_scene_check_extent), which needs no GPU.
void SceneState::checkExtent() {
    // The kernels' short reciprocal (pt_vec.h: rcp_exact_normal) equals the IEEE quotient while the Moller-Trumbore
    // determinant stays below 2^126; |a| <= 2 |e1| |e2| (|d| = 1), so edge components below 2^60 are always safe.
    for (const Primitive& p : h_primitives)
        for (int k = 0; k < (p.type == PRIM_QUAD ? 4 : 3); k++) {
            const f3 e = p.v[k] - p.v[0];
            const float m = fmaxf(fabsf(e.x), fmaxf(fabsf(e.y), fabsf(e.z)));
            const float c = fabsf(p.v[k].x) + fabsf(p.v[k].y) + fabsf(p.v[k].z);
            if (!(m < 1.0e18f) || !(c < 3.0e38f)) throw ArgError("scene coordinates must be finite and primitive edges shorter than 1e18");
        }
    // The quad halves (Quad::intersect: u >= 0 && u <= 1) reject a NaN u or v that the device's min chain ignores.  u, v are
    // f * dot(s, h) and f * dot(d, q) with |h_a| <= 2 |d| E, |q_a| <= 2 S E (E: a quad edge, S: |o - v0|, per component), so no
    // product and no partial sum exceeds 6 |d| S E: below 2^128 nothing overflows and, f being finite (|a| > 1e-8), u and v are
    // numbers.  S is at most the scene's extent plus the rounding of a hit point o + t d, below 2^-22 of the largest coordinate
    // (quadReach adds 2^-20 of it), and 6 * 2^124 < 2^127.  Triangles need no such bound: Triangle::intersect (u < 0 || u > 1)
    // lets a NaN through as the device does.
    quad_edge_max = 0.0f;
    bool first = true;
    for (const Primitive& p : h_primitives)
        for (int k = 0; k < (p.type == PRIM_QUAD ? 4 : 3); k++) {
            const float c[3] = {p.v[k].x, p.v[k].y, p.v[k].z};
            for (int a = 0; a < 3; a++) {
                coord_lo[a] = first ? c[a] : fminf(coord_lo[a], c[a]);
                coord_hi[a] = first ? c[a] : fmaxf(coord_hi[a], c[a]);
            }
            first = false;
            if (p.type == PRIM_QUAD) {
                const f3 e = p.v[k] - p.v[0];
                quad_edge_max = fmaxf(quad_edge_max, fmaxf(fabsf(e.x), fmaxf(fabsf(e.y), fabsf(e.z))));
            }
        }
    if (quad_edge_max > 0.0f) {
        const double reach = quadReach(coord_lo);          // from a corner of the scene's box: its extent
        if (!((double)quad_edge_max * reach <= kQuadReachBound))
            throw ArgError("scene with quads: the largest quad edge times the scene's extent must not exceed 2^124");
    }
}

void SceneState::upload() {
    const int n = (int)h_primitives.size();
    checkExtent();
    // ---- SoA re-layout (device_scene.h) ----
    const int stride = num_quads ? 4 : 3;
    auto bits = [](int i) { float f; std::memcpy(&f, &i, 4); return f; };
    std::vector<float4> nodes(2 * bvh_nodes.size()), prims((size_t)stride * n), mats((size_t)3 * n);
    // pre-order skip pointers: skip[i] = i + size of the subtree rooted at i
    std::vector<int> subtree(bvh_nodes.size(), 1);
    for (size_t i = bvh_nodes.size(); i-- > 0;)
        if (!bvh_nodes[i].isLeaf()) subtree[i] = 1 + subtree[bvh_nodes[i].left_child] + subtree[bvh_nodes[i].right_child];
    for (size_t i = 0; i < bvh_nodes.size(); i++) {
        const BVHNode& b = bvh_nodes[i];
        if (!b.isLeaf() && b.left_child != (int)i + 1) throw ArgError("internal: BVH is not in pre-order");
        nodes[2 * i] = make_float4(b.bbox.min.x, b.bbox.min.y, b.bbox.min.z, bits(b.isLeaf() ? b.left_child : (int)i + subtree[i]));
        nodes[2 * i + 1] = make_float4(b.bbox.max.x, b.bbox.max.y, b.bbox.max.z, bits(b.isLeaf() ? -b.prim_count : b.right_child));
    }
    for (int k = 0; k < n; k++) {                     // k = leaf-order slot
        const int src = bvh_indices[k];
        const Primitive& p = h_primitives[src];
        const f3 e1 = p.v[1] - p.v[0], e2 = p.v[2] - p.v[0];
        prims[(size_t)stride * k] = make_float4(p.v[0].x, p.v[0].y, p.v[0].z, bits(p.type == PRIM_QUAD ? 1 : 0));
        prims[(size_t)stride * k + 1] = make_float4(e1.x, e1.y, e1.z, 0.0f);
        prims[(size_t)stride * k + 2] = make_float4(e2.x, e2.y, e2.z, 0.0f);
        if (stride == 4) {
            const f3 e3 = p.type == PRIM_QUAD ? p.v[3] - p.v[0] : mk3(0, 0, 0);
            prims[(size_t)stride * k + 3] = make_float4(e3.x, e3.y, e3.z, 0.0f);
        }
        mats[(size_t)3 * k] = make_float4(p.normal.x, p.normal.y, p.normal.z, bits(src));
        mats[(size_t)3 * k + 1] = make_float4(p.bsdf.x, p.bsdf.y, p.bsdf.z, 0.0f);
        mats[(size_t)3 * k + 2] = make_float4(p.Le.x, p.Le.y, p.Le.z, 0.0f);
    }
    d_nodes = (float4*)hipMallocSafe(nodes.size() * sizeof(float4), "d_nodes");
    d_prims = (float4*)hipMallocSafe(prims.size() * sizeof(float4), "d_prims");
    d_mats = (float4*)hipMallocSafe(mats.size() * sizeof(float4), "d_mats");
    PTMI_HIP(hipMemcpy(d_nodes, nodes.data(), nodes.size() * sizeof(float4), hipMemcpyHostToDevice));
    PTMI_HIP(hipMemcpy(d_prims, prims.data(), prims.size() * sizeof(float4), hipMemcpyHostToDevice));
    PTMI_HIP(hipMemcpy(d_mats, mats.data(), mats.size() * sizeof(float4), hipMemcpyHostToDevice));

    // the emitter table (device_scene.h: EmitterTable): records in emitter order, pdf_area by leaf-order slot
    {
        const int ne = (int)h_emit_prim.size();
        std::vector<int> slot_of((size_t)n);
        for (int k = 0; k < n; k++) slot_of[bvh_indices[k]] = k;
        std::vector<float4> rec((size_t)kEmitterStride * ne);
        std::vector<float4> pdf_slot((size_t)n, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        for (int j = 0; j < ne; j++) {
            const int i = h_emit_prim[j];
            const Primitive& p = h_primitives[i];
            const f3 ng = h_emit_normal[j];
            float4* r = &rec[(size_t)kEmitterStride * j];
            r[0] = make_float4(p.v[0].x, p.v[0].y, p.v[0].z, bits(slot_of[i]));
            r[1] = make_float4(p.v[1].x, p.v[1].y, p.v[1].z, p.sampleAreaRatio());
            r[2] = make_float4(p.v[2].x, p.v[2].y, p.v[2].z, bits(p.type == PRIM_QUAD ? 1 : 0));
            r[3] = make_float4(p.v[3].x, p.v[3].y, p.v[3].z, h_pdf_area[i]);
            r[4] = make_float4(ng.x, ng.y, ng.z, 0.0f);
            r[5] = make_float4(p.Le.x, p.Le.y, p.Le.z, 0.0f);
            pdf_slot[slot_of[i]] = make_float4(ng.x, ng.y, ng.z, h_pdf_area[i]);
        }
        d_pdf_area = (float4*)hipMallocSafe((size_t)n * sizeof(float4), "d_pdf_area");
        PTMI_HIP(hipMemcpy(d_pdf_area, pdf_slot.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice));
        if (ne > 0) {
            d_emit_rec = (float4*)hipMallocSafe(rec.size() * sizeof(float4), "d_emit_rec");
            d_emit_cdf = (float*)hipMallocSafe((size_t)ne * sizeof(float), "d_emit_cdf");
            PTMI_HIP(hipMemcpy(d_emit_rec, rec.data(), rec.size() * sizeof(float4), hipMemcpyHostToDevice));
            PTMI_HIP(hipMemcpy(d_emit_cdf, h_emit_cdf.data(), (size_t)ne * sizeof(float), hipMemcpyHostToDevice));
        }
        d_emitters.cdf = d_emit_cdf; d_emitters.rec = d_emit_rec; d_emitters.pdf_area = d_pdf_area;
        d_emitters.n = ne; d_emitters.total = h_emit_total;
    }

    d_scene.nodes = d_nodes; d_scene.prims = d_prims; d_scene.mats = d_mats;
    d_scene.n_nodes = (int)bvh_nodes.size(); d_scene.n_prims = n;
    d_scene.prim_stride = stride; d_scene.has_quads = num_quads ? 1 : 0;
    d_scene.stack_entries = std::min(bvh_depth + 1, 64);
    // the sweep's leaf-only walk (csrc/traversal.h): taken only where the node array itself shows every box inside its parent's,
    // all planes finite - once per scene load; 0 leaves: the sweep walks every node
    {
        const ptmi_vec_bits* nb = reinterpret_cast<const ptmi_vec_bits*>(nodes.data());
        d_scene.sweep_leaves = ptmi_sweep_leaves_verdict(nb, d_scene.n_nodes, n) ? ptmi_sweep_leaf_count(nb, d_scene.n_nodes) : 0;
    }
    // LDS residency: the whole scene is staged per workgroup while it leaves room for >= 2 workgroups per CU
    const size_t scene_bytes = (nodes.size() + prims.size() + mats.size()) * sizeof(float4);
    d_scene.lds_resident = (scene_bytes + (size_t)d_scene.stack_entries * kBlock * sizeof(int)) <= 64 * 1024 ? 1 : 0;
    buildPacked();
    // Triangle scenes beyond the sweep's few dozen primitives: the 8-wide tree + the certificate data of TRAVERSAL_CERTIFIED - the
    // default walk there: the reference's hit for every ray, by proof or by its own walk, at 1.4 - 2.3 x the rate of the walk over
    // the reference's tree (128 ... 1 M triangles, planar scenes included; 1 M triangles: +1.3 s of loading, +145 MB)
    if (n > sweep_max_prims && bvh_depth <= 62 && certified_default) {
        try { buildFast(); }
        catch (const ArgError&) { freeFast(); }        // a scene the builder declines (tree too deep for the walk's LDS stack, coordinates of 1e9): the reference's tree is walked
        catch (const HipError&) { freeFast(); (void)hipGetLastError(); }      // no memory for the second tree: the scene still loads
    }
    chooseTraversal();
}

void SceneState::freePacked() {
    void* ptrs[] = {d_gnodes, d_gmats, d_mtab, d_gprims, d_load_index};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    d_gnodes = d_gmats = d_mtab = nullptr; d_gprims = nullptr; d_load_index = nullptr;
    d_scene.gnodes = nullptr; d_scene.n_pos = 0; d_scene.gprims = nullptr; d_scene.gmats = nullptr; d_scene.mtab = nullptr;
    d_scene.load_index = nullptr; d_scene.n_top = 0; d_scene.top_depth = 0;
}

// The node records of the packed layout (csrc/device_scene.h: PACKED LAYOUT): same tree, same visiting order, explicit links,
// sibling pairs adjacent, the nodes of depth <= D first (level by level) while they fit top_records positions.  false: a leaf
// holds more than 7 primitives (its count has 3 bits).
bool packBvhNodes(const std::vector<BVHNode>& bvh_nodes, int top_records, std::vector<float4>& g, int& n_pos_out, int& n_top_out, int& top_depth_out) {
    const int n = (int)bvh_nodes.size();
    for (const BVHNode& b : bvh_nodes) if (b.isLeaf() && b.prim_count > 7) return false;
    auto bits = [](int i) { float f; std::memcpy(&f, &i, 4); return f; };
    std::vector<int> pos((size_t)n, -1), subtree((size_t)n, 1), stack;
    for (int i = n; i-- > 0;)
        if (!bvh_nodes[i].isLeaf()) subtree[i] = 1 + subtree[bvh_nodes[i].left_child] + subtree[bvh_nodes[i].right_child];
    int n_pos = 2, top_depth = -1;                     // root at 0, position 1 pads it to a pair
    pos[0] = 0;
    {
        std::vector<int> level{0}, next_level;
        for (int d = 0; !level.empty(); d++) {
            int pairs = 0;
            for (int x : level) if (!bvh_nodes[x].isLeaf()) pairs++;
            if (n_pos + 2 * pairs > top_records) break;                   // the next level no longer fits the LDS top
            next_level.clear();
            for (int x : level) {
                if (bvh_nodes[x].isLeaf()) continue;
                const int l = bvh_nodes[x].left_child, r = bvh_nodes[x].right_child;
                pos[l] = n_pos; pos[r] = n_pos + 1; n_pos += 2;
                next_level.push_back(l); next_level.push_back(r);
            }
            top_depth = d + 1;
            level.swap(next_level);
        }
    }
    const int n_top = top_records >= 2 ? n_pos : 0;
    stack.push_back(0);
    while (!stack.empty()) {                           // the rest: pairs in pre-order of their parents
        const int x = stack.back(); stack.pop_back();
        if (bvh_nodes[x].isLeaf()) continue;
        const int l = bvh_nodes[x].left_child, r = bvh_nodes[x].right_child;
        if (pos[l] < 0) { pos[l] = n_pos; pos[r] = n_pos + 1; n_pos += 2; }
        stack.push_back(r); stack.push_back(l);
    }
    auto position_of = [&](int pre) { return pre >= n ? n_pos : pos[pre]; };
    const float inf = std::numeric_limits<float>::infinity();
    g.assign((size_t)2 * n_pos, make_float4(inf, inf, inf, 0.0f));
    g[2] = make_float4(inf, inf, inf, bits(0)); g[3] = make_float4(-inf, -inf, -inf, bits(~n_pos));   // padding: an empty leaf nobody links to
    for (int i = 0; i < n; i++) {
        const BVHNode& b = bvh_nodes[i];
        int a_, b_;
        if (b.isLeaf()) { a_ = (b.left_child << 3) | b.prim_count; b_ = ~position_of(i + 1); }
        else { a_ = position_of(i + subtree[i]); b_ = pos[b.left_child]; }
        g[2 * (size_t)pos[i]] = make_float4(b.bbox.min.x, b.bbox.min.y, b.bbox.min.z, bits(a_));
        g[2 * (size_t)pos[i] + 1] = make_float4(b.bbox.max.x, b.bbox.max.y, b.bbox.max.z, bits(b_));
    }
    n_pos_out = n_pos; n_top_out = n_top; top_depth_out = top_depth;
    return true;
}

// The packed layout of csrc/device_scene.h: same tree, same visiting order, records placed so that a ray touches fewer lines.
void SceneState::buildPacked() {
    freePacked();
    const int n = (int)bvh_nodes.size(), n_prims = (int)h_primitives.size();
    if (!d_nodes || d_scene.lds_resident || bvh_depth > 62 || n < packed_min_nodes || n_prims >= (1 << 28)) return;
    auto bits = [](int i) { float f; std::memcpy(&f, &i, 4); return f; };
    std::vector<float4> g;
    int n_pos = 0, n_top = 0, top_depth = -1;
    if (!packBvhNodes(bvh_nodes, packed_top_records, g, n_pos, n_top, top_depth)) return;
    // materials: (normal, table row) per slot + the distinct (Kd, Ke) pairs; load-order index on its own
    std::map<std::array<uint32_t, 6>, int> rows;
    std::vector<float4> gm((size_t)n_prims), tab;
    std::vector<int> load_index((size_t)n_prims);
    std::vector<float> gp;
    if (!num_quads) gp.resize((size_t)9 * n_prims);
    for (int k = 0; k < n_prims; k++) {
        const Primitive& p = h_primitives[bvh_indices[k]];
        std::array<uint32_t, 6> key;
        const float kv[6] = {p.bsdf.x, p.bsdf.y, p.bsdf.z, p.Le.x, p.Le.y, p.Le.z};
        std::memcpy(key.data(), kv, sizeof kv);
        auto it = rows.find(key);
        if (it == rows.end()) {
            it = rows.emplace(key, (int)rows.size()).first;
            tab.push_back(make_float4(p.bsdf.x, p.bsdf.y, p.bsdf.z, 0.0f)); tab.push_back(make_float4(p.Le.x, p.Le.y, p.Le.z, 0.0f));
        }
        gm[k] = make_float4(p.normal.x, p.normal.y, p.normal.z, bits(it->second));
        load_index[k] = bvh_indices[k];
        if (!num_quads) {
            const f3 e1 = p.v[1] - p.v[0], e2 = p.v[2] - p.v[0];         // the float subtraction the reference does per test
            const float rec[9] = {p.v[0].x, p.v[0].y, p.v[0].z, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z};
            std::memcpy(&gp[(size_t)9 * k], rec, sizeof rec);
        }
    }
    auto upload_vec = [&](const void* src, size_t bytes, const char* name) {
        void* d = hipMallocSafe(bytes, name);
        PTMI_HIP(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
        return d;
    };
    d_gnodes = (float4*)upload_vec(g.data(), g.size() * sizeof(float4), "d_gnodes");
    d_gmats = (float4*)upload_vec(gm.data(), gm.size() * sizeof(float4), "d_gmats");
    d_mtab = (float4*)upload_vec(tab.data(), tab.size() * sizeof(float4), "d_mtab");
    d_load_index = (int*)upload_vec(load_index.data(), load_index.size() * sizeof(int), "d_load_index");
    if (!num_quads) d_gprims = (float*)upload_vec(gp.data(), gp.size() * sizeof(float), "d_gprims");
    d_scene.gnodes = d_gnodes; d_scene.n_pos = n_pos; d_scene.gprims = d_gprims; d_scene.gmats = d_gmats; d_scene.mtab = d_mtab;
    d_scene.load_index = d_load_index; d_scene.n_top = n_top; d_scene.top_depth = top_depth;
}

void SceneState::freeFast() {
    void* ptrs[] = {d_wnodes, d_wprims, d_wmats, d_wmtab, d_wload_index, d_wref_slot, d_wanc, d_wcert, d_wfast_of_ref, d_wqprims};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    d_wqprims = nullptr; d_scene.wqprims = nullptr;
    d_wnodes = nullptr; d_wprims = nullptr; d_wmats = d_wmtab = nullptr; d_wload_index = d_wref_slot = nullptr;
    d_wanc = nullptr; d_wcert = nullptr; d_wfast_of_ref = nullptr;
    h_wide.clear();
    d_scene.wnodes = nullptr; d_scene.w_nodes = d_scene.w_top = d_scene.w_depth = 0; d_scene.wprims = nullptr; d_scene.wmats = nullptr;
    d_scene.wmtab = nullptr; d_scene.wload_index = nullptr; d_scene.wref_slot = nullptr;
    d_scene.wanc = nullptr; d_scene.wcert = nullptr; d_scene.wfast_of_ref = nullptr; d_scene.w_guard = 0.0f; d_scene.w_big = 0.0f;
}

// The opt-in fast tree (csrc/wide_bvh.h): same triangles, same hit arithmetic, own boxes.  Per-triangle arrays are re-ordered
// into the fast tree's leaf order; wref_slot keeps every triangle's reference leaf-order slot for the equal-t rule.
void SceneState::buildFast() {
    freeFast();
    if (!d_nodes) throw ArgError("fast tree: no scene loaded");
    fast_declined = true;                              // until the build has gone through
    try { buildWideBVH(h_primitives, wide_params, h_wide); }
    catch (const std::exception& e) { h_wide.clear(); throw ArgError(e.what()); }      // every builder failure: the callers' fallback catches ArgError
    // The walk's stack is (levels - 1) x 256 lanes x 8 bytes of the workgroup's LDS, next to the tree's top and - in the radiosity
    // pre-pass - 7 KB of static arrays; a launch may ask for 64 KB.  24 levels = 46 KB leaves room for both (an 8-wide tree of a
    // million triangles has 9 levels); a deeper tree is declined and the scene walks the reference's tree.
    if (h_wide.depth > kWideMaxLevels) { h_wide.clear(); throw ArgError("fast tree: deeper than " + std::to_string(kWideMaxLevels) + " levels"); }
    const int n = (int)h_primitives.size();
    auto bits = [](int i) { float f; std::memcpy(&f, &i, 4); return f; };
    std::vector<int> ref_slot_of_load((size_t)n), ref_slot((size_t)n);
    for (int k = 0; k < n; k++) ref_slot_of_load[bvh_indices[k]] = k;
    std::map<std::array<uint32_t, 6>, int> rows;
    std::vector<float4> wm((size_t)n), tab;
    std::vector<float> wp((size_t)9 * n);
    std::vector<float4> wq(num_quads ? (size_t)4 * n : 0);
    for (int k = 0; k < n; k++) {
        const int li = h_wide.tri_load_index[k];
        const Primitive& p = h_primitives[li];
        ref_slot[k] = ref_slot_of_load[li];
        std::array<uint32_t, 6> key;
        const float kv[6] = {p.bsdf.x, p.bsdf.y, p.bsdf.z, p.Le.x, p.Le.y, p.Le.z};
        std::memcpy(key.data(), kv, sizeof kv);
        auto it = rows.find(key);
        if (it == rows.end()) {
            it = rows.emplace(key, (int)rows.size()).first;
            tab.push_back(make_float4(p.bsdf.x, p.bsdf.y, p.bsdf.z, 0.0f)); tab.push_back(make_float4(p.Le.x, p.Le.y, p.Le.z, 0.0f));
        }
        wm[k] = make_float4(p.normal.x, p.normal.y, p.normal.z, bits(it->second));
        const f3 e1 = p.v[1] - p.v[0], e2 = p.v[2] - p.v[0];             // the float subtraction the reference does per test
        const float rec[9] = {p.v[0].x, p.v[0].y, p.v[0].z, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z};
        std::memcpy(&wp[(size_t)9 * k], rec, sizeof rec);
        if (num_quads) {                                                  // scenes with quads: the 64-byte records of d_prims, fast order
            const f3 e3 = p.type == PRIM_QUAD ? p.v[3] - p.v[0] : mk3(0, 0, 0);
            wq[(size_t)4 * k] = make_float4(p.v[0].x, p.v[0].y, p.v[0].z, bits(p.type == PRIM_QUAD ? 1 : 0));
            wq[(size_t)4 * k + 1] = make_float4(e1.x, e1.y, e1.z, 0.0f);
            wq[(size_t)4 * k + 2] = make_float4(e2.x, e2.y, e2.z, 0.0f);
            wq[(size_t)4 * k + 3] = make_float4(e3.x, e3.y, e3.z, 0.0f);
        }
    }
    auto upload_vec = [&](const void* src, size_t bytes, const char* name) {
        void* d = hipMallocSafe(bytes, name);
        PTMI_HIP(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
        return d;
    };
    d_wnodes = (uint4*)upload_vec(h_wide.nodes.data(), h_wide.nodes.size() * sizeof(uint32_t), "d_wnodes");
    d_wprims = (float*)upload_vec(wp.data(), wp.size() * sizeof(float), "d_wprims");
    if (num_quads) d_wqprims = (float4*)upload_vec(wq.data(), wq.size() * sizeof(float4), "d_wqprims");
    d_wmats = (float4*)upload_vec(wm.data(), wm.size() * sizeof(float4), "d_wmats");
    d_wmtab = (float4*)upload_vec(tab.data(), tab.size() * sizeof(float4), "d_wmtab");
    d_wload_index = (int*)upload_vec(h_wide.tri_load_index.data(), (size_t)n * sizeof(int), "d_wload_index");
    d_wref_slot = (int*)upload_vec(ref_slot.data(), (size_t)n * sizeof(int), "d_wref_slot");
    // TRAVERSAL_CERTIFIED: per reference leaf the pre-order indices of its ancestors (the leaf itself first, the root last) in chunks
    // of four, padded with 0xffffffff; per fast-order triangle where its leaf's list starts and how many chunks it has; and the
    // way back from a reference leaf-order slot to the fast order (for the rays that take the reference's walk)
    {
        const int nn = (int)bvh_nodes.size();
        std::vector<int> parent((size_t)nn, -1);
        for (int i = 0; i < nn; i++) if (!bvh_nodes[i].isLeaf()) { parent[bvh_nodes[i].left_child] = i; parent[bvh_nodes[i].right_child] = i; }
        std::vector<uint32_t> anc;                       // 4 per chunk
        std::vector<uint32_t> leaf_ref((size_t)nn, 0u);  // leaf node -> first chunk << 5 | chunks
        std::vector<int> path;
        bool fits = true;
        for (int i = 0; i < nn; i++) {
            if (!bvh_nodes[i].isLeaf()) continue;
            path.clear();
            for (int x = i; x >= 0; x = parent[x]) path.push_back(x);
            const size_t first_chunk = anc.size() / 4, chunks = (path.size() + 3) / 4;
            if (chunks == 0) throw std::logic_error("fast tree: an empty ancestor list");      // the list starts with the leaf itself
            if (chunks > 31 || first_chunk >= (1u << 27)) { fits = false; break; }
            for (size_t k = 0; k < path.size(); k++) anc.push_back((uint32_t)path[k]);      // the leaf first, the root last
            while (anc.size() % 4) anc.push_back(0xffffffffu);
            leaf_ref[i] = (uint32_t)(first_chunk << 5) | (uint32_t)chunks;
        }
        if (fits && bvh_depth <= 62) {
            std::vector<int> leaf_of_slot((size_t)n, 0), fast_of_ref((size_t)n, 0);
            for (int i = 0; i < nn; i++) if (bvh_nodes[i].isLeaf()) for (int k = 0; k < bvh_nodes[i].prim_count; k++) leaf_of_slot[bvh_nodes[i].left_child + k] = i;
            // one 64-byte record per fast-order triangle - ONE line of memory per hit: the leaf's box as the reference built it + where
            // its ancestor list is (the proof reads these), then what shading reads (wmats' entry: normal, row of the material table)
            std::vector<float4> cert((size_t)kWideCertStride * n);
            for (int k = 0; k < n; k++) {
                const int leaf = leaf_of_slot[ref_slot[k]];
                const AABB& bx = bvh_nodes[leaf].bbox;
                float ref_bits; std::memcpy(&ref_bits, &leaf_ref[leaf], 4);
                cert[(size_t)kWideCertStride * k] = make_float4(bx.min.x, bx.min.y, bx.min.z, ref_bits);
                cert[(size_t)kWideCertStride * k + 1] = make_float4(bx.max.x, bx.max.y, bx.max.z, 0.0f);
                cert[(size_t)kWideCertStride * k + 2] = wm[k];
                cert[(size_t)kWideCertStride * k + 3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                fast_of_ref[ref_slot[k]] = k;
            }
            d_wanc = (uint4*)upload_vec(anc.data(), anc.size() * sizeof(uint32_t), "d_wanc");
            d_wcert = (float4*)upload_vec(cert.data(), cert.size() * sizeof(float4), "d_wcert");
            d_wfast_of_ref = (int*)upload_vec(fast_of_ref.data(), fast_of_ref.size() * sizeof(int), "d_wfast_of_ref");
        }
    }
    // LDS of a workgroup: the walk's stack (one 8-byte entry per lane and tree level below the root: a group is pushed only
    // while a deeper one is entered) + the top of the tree, whole levels while they fit wide_top_nodes AND six workgroups
    // still share a CU's 160 KB (6 waves per SIMD, what the kernel's 80 registers allow; a 9-level tree with the 8-level
    // tree's top dropped to 5 waves: -6 %)
    const int stack_entries = std::max(h_wide.depth - 1, 1);
    const long long lds_budget = 160 * 1024 / 6 - (long long)stack_entries * kBlock * 8;
    int top = 0;
    for (size_t l = 1; l < h_wide.level_start.size(); l++)
        if (h_wide.level_start[l] <= wide_top_nodes && (long long)h_wide.level_start[l] * kWideNodeDwords * 4 <= lds_budget) top = h_wide.level_start[l];
    d_scene.wnodes = d_wnodes; d_scene.w_nodes = h_wide.n_nodes; d_scene.w_top = top; d_scene.w_depth = stack_entries;
    d_scene.wqprims = d_wqprims;
    d_scene.wprims = d_wprims; d_scene.wmats = d_wmats; d_scene.wmtab = d_wmtab; d_scene.wload_index = d_wload_index; d_scene.wref_slot = d_wref_slot;
    d_scene.wanc = d_wanc; d_scene.wcert = d_wcert; d_scene.wfast_of_ref = d_wfast_of_ref; d_scene.w_guard = h_wide.origin_guard; d_scene.w_big = h_wide.scale;
    if (bounce_lds_bytes_wide(d_scene) > 56 * 1024) { freeFast(); throw ArgError("fast tree: the walk's LDS does not fit a workgroup"); }
    fast_declined = false;
}

void SceneState::setRadiosity(const float* rgb) {
    if (!d_nodes) throw ArgError("setRadiosity: no scene loaded");
    if (d_radiosity) { (void)hipFree(d_radiosity); d_radiosity = nullptr; }
    d_scene.radiosity = nullptr;
    if (!rgb) return;
    const int n = (int)h_primitives.size();
    std::vector<float4> leaf_order((size_t)n);
    for (int k = 0; k < n; k++) {                    // same leaf-order slots as prims/mats
        const float* c = rgb + (size_t)bvh_indices[k] * 3;
        leaf_order[k] = make_float4(c[0], c[1], c[2], 0.0f);
    }
    d_radiosity = (float4*)hipMallocSafe(leaf_order.size() * sizeof(float4), "d_radiosity");
    PTMI_HIP(hipMemcpy(d_radiosity, leaf_order.data(), leaf_order.size() * sizeof(float4), hipMemcpyHostToDevice));
    d_scene.radiosity = d_radiosity;
}

// specular surfaces (include/ptmi.h: ptmi_set_surfaces): the table by leaf-order slot, as upload() lays out pdf_area
void SceneState::setSurfaces(const int* kind, const float* ior, const float* roughness) {
    if (!d_nodes) throw ArgError("setSurfaces: no scene loaded");
    const int n = (int)h_primitives.size();
    float2* nd = nullptr;
    int mirrors = 0, glasses = 0, roughs = 0;
    if (kind) {
        for (int i = 0; i < n; i++) { mirrors += kind[i] == kSurfaceMirror; glasses += kind[i] == kSurfaceGlass; roughs += kind[i] == kSurfaceRough; }
        if (mirrors + glasses + roughs > 0) {
            std::vector<float2> slot((size_t)n);
            for (int k = 0; k < n; k++) {                // same leaf-order slots as prims/mats
                const int src = bvh_indices[k];
                float bits; std::memcpy(&bits, &kind[src], 4);
                float param = ior ? ior[src] : kSurfaceDefaultIor;
                if (kind[src] == kSurfaceRough) {            // alpha = roughness * roughness, in float
                    const float r = roughness ? roughness[src] : kSurfaceDefaultRoughness;
                    param = r * r;
                }
                slot[k] = make_float2(bits, param);
            }
            nd = (float2*)hipMallocSafe((size_t)n * sizeof(float2), "d_surfaces");
            const hipError_t e = hipMemcpy(nd, slot.data(), (size_t)n * sizeof(float2), hipMemcpyHostToDevice);
            if (e != hipSuccess) { (void)hipFree(nd); PTMI_HIP(e); }
        }
    }
    if (d_surfaces) (void)hipFree(d_surfaces);         // nothing has changed before this line
    d_surfaces = nd; n_mirror = mirrors; n_glass = glasses;
    const bool table = nd != nullptr;
    surface_counts[0] = table ? n - mirrors - glasses - roughs : 0;
    surface_counts[1] = mirrors; surface_counts[2] = glasses; surface_counts[3] = roughs;
}

// vertex normals (include/ptmi.h: ptmi_set_vertex_normals): prim_stride entries per leaf-order slot, as upload() lays out prims
void SceneState::setVertexNormals(const float* normals, const std::vector<unsigned char>& smooth, int smooth_count) {
    if (!d_nodes) throw ArgError("setVertexNormals: no scene loaded");
    const int n = (int)h_primitives.size();
    const int stride = d_scene.prim_stride;
    float4* nd = nullptr;
    if (!normals) smooth_count = 0;
    else if (smooth.size() != (size_t)n) throw ArgError("setVertexNormals: the classification does not match the scene");
    if (smooth_count > 0) {
        auto bits = [](int i) { float f; std::memcpy(&f, &i, 4); return f; };
        std::vector<float4> slot((size_t)stride * n, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        for (int k = 0; k < n; k++) {                    // same leaf-order slots as prims/mats
            const int src = bvh_indices[k];
            const int read = h_primitives[src].type == PRIM_QUAD ? 4 : 3;
            for (int c = 0; c < read && c < stride; c++) {
                const float* v = normals + ((size_t)src * kVertexNormalCorners + (size_t)c) * 3;
                slot[(size_t)stride * k + c] = make_float4(v[0], v[1], v[2], c == 0 ? bits(smooth[src]) : 0.0f);
            }
        }
        nd = (float4*)hipMallocSafe(slot.size() * sizeof(float4), "d_vertex_normals");
        const hipError_t e = hipMemcpy(nd, slot.data(), slot.size() * sizeof(float4), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(nd); PTMI_HIP(e); }
    }
    if (d_vertex_normals) (void)hipFree(d_vertex_normals);   // nothing has changed before this line
    d_vertex_normals = nd; n_smooth = smooth_count;
}

// albedo texture (include/ptmi.h: ptmi_set_albedo_texture): two float4 per leaf-order slot and the image as float4 (rgb, 0)
void SceneState::setAlbedoTexture(int width, int height, const float* texels, int filter, const float* uv, const int* textured) {
    if (!d_nodes) throw ArgError("setAlbedoTexture: no scene loaded");
    const int n = (int)h_primitives.size();
    const int count = texels && uv ? countTextured(n, textured) : 0;
    float4 *rd = nullptr, *td = nullptr;
    if (count > 0) {
        const float untextured = std::numeric_limits<float>::quiet_NaN();
        std::vector<float4> rec(2 * (size_t)n, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        for (int k = 0; k < n; k++) {                    // same leaf-order slots as prims/mats
            const int src = bvh_indices[k];
            if (textured && textured[src] == 0) { rec[2 * (size_t)k].x = untextured; continue; }   // its UVs are never read
            const float* v = uv + (size_t)src * kAlbedoCorners * 2;
            const bool quad = h_primitives[src].type == PRIM_QUAD;
            rec[2 * (size_t)k] = make_float4(v[0], v[1], v[2], v[3]);
            rec[2 * (size_t)k + 1] = make_float4(v[4], v[5], quad ? v[6] : 0.0f, quad ? v[7] : 0.0f);
        }
        std::vector<float4> tex((size_t)width * (size_t)height);
        for (size_t t = 0; t < tex.size(); t++) tex[t] = make_float4(texels[3 * t], texels[3 * t + 1], texels[3 * t + 2], 0.0f);
        rd = (float4*)hipMallocSafe(rec.size() * sizeof(float4), "d_albedo_rec");
        hipError_t e = hipMemcpy(rd, rec.data(), rec.size() * sizeof(float4), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(rd); PTMI_HIP(e); }
        try {
            td = (float4*)hipMallocSafe(tex.size() * sizeof(float4), "d_albedo_texels");
        } catch (...) { (void)hipFree(rd); throw; }
        e = hipMemcpy(td, tex.data(), tex.size() * sizeof(float4), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(rd); (void)hipFree(td); PTMI_HIP(e); }
    }
    if (d_albedo_rec) (void)hipFree(d_albedo_rec);       // nothing has changed before this line
    if (d_albedo_texels) (void)hipFree(d_albedo_texels);
    d_albedo_rec = rd; d_albedo_texels = td; n_textured = count;
    tex_width = count > 0 ? width : 0; tex_height = count > 0 ? height : 0; tex_filter = count > 0 ? filter : 0;
}

// RadiosityState: host/radiosity_state.cpp

void SceneState::precomputeCDFsDevice(const void* d_src, int src_kind, hipStream_t stream) {
    if (!d_nodes) throw ArgError("precomputeCDFs: no scene loaded");
    if (d_precomputed_cdfs) { (void)hipFree(d_precomputed_cdfs); d_precomputed_cdfs = nullptr; }
    h_precomputed_cdfs.clear();
    d_scene.cdfs = nullptr;
    const int n = (int)h_primitives.size();
    d_precomputed_cdfs = (float*)hipMallocSafe((size_t)n * kCdfDwords * sizeof(float), "d_precomputed_cdfs");
    launch_cdf_records(n, d_src, src_kind, d_precomputed_cdfs, stream);
    PTMI_HIP(hipGetLastError());
    PTMI_HIP(hipStreamSynchronize(stream));
    d_scene.cdfs = d_precomputed_cdfs;
}

const std::vector<float>& SceneState::precomputedCdfsHost() {
    if (h_precomputed_cdfs.empty() && d_precomputed_cdfs) {
        h_precomputed_cdfs.resize(h_primitives.size() * (size_t)kCdfDwords);
        PTMI_HIP(hipMemcpy(h_precomputed_cdfs.data(), d_precomputed_cdfs, h_precomputed_cdfs.size() * sizeof(float), hipMemcpyDeviceToHost));
    }
    return h_precomputed_cdfs;
}

void SceneState::precomputeCDFs(const float* rgb) {
    if (!d_nodes) throw ArgError("precomputeCDFs: no scene loaded");
    if (d_precomputed_cdfs) { (void)hipFree(d_precomputed_cdfs); d_precomputed_cdfs = nullptr; }
    h_precomputed_cdfs.clear();
    d_scene.cdfs = nullptr;
    h_filtered_formfactor.clear(); h_filtered_radiosity.clear();
    if (!rgb) { h_radiosity_grids.clear(); return; }
    const size_t cells = h_primitives.size() * (size_t)kGridSize;
    if (rgb != h_radiosity_grids.data()) h_radiosity_grids.assign(rgb, rgb + cells * 3);
    struct Tmp { void* p = nullptr; ~Tmp() { if (p) (void)hipFree(p); } } d_rgb;
    d_rgb.p = hipMallocSafe(cells * 3 * sizeof(float), "d_radiosity_grids_rgb");
    PTMI_HIP(hipMemcpy(d_rgb.p, rgb, cells * 3 * sizeof(float), hipMemcpyHostToDevice));
    precomputeCDFsDevice(d_rgb.p, 1, nullptr);
}

void SceneState::precomputeCDFsFromFiltered(bool use_bilateral, float sigma_spatial, float sigma_range, hipStream_t stream) {
    if (!d_nodes) throw ArgError("precomputeCDFsFromFiltered: no scene loaded");
    if (h_radiosity_grids.empty()) throw ArgError("precomputeCDFsFromFiltered: the scene has no radiosity grids");
    const int n = (int)h_primitives.size();
    const size_t cells = (size_t)n * kGridSize;
    struct Tmp { void* p = nullptr; ~Tmp() { if (p) (void)hipFree(p); } } rgb, cnt, off, orad;
    rgb.p = hipMallocSafe(cells * 3 * sizeof(float), "d_filter_rgb");
    off.p = hipMallocSafe(cells * sizeof(float), "d_filtered_formfactor");
    orad.p = hipMallocSafe(cells * sizeof(float), "d_filtered_radiosity");
    PTMI_HIP(hipMemcpy(rgb.p, h_radiosity_grids.data(), cells * 3 * sizeof(float), hipMemcpyHostToDevice));
    if (!h_count_grids.empty()) {
        cnt.p = hipMallocSafe(cells * sizeof(float), "d_filter_counts");
        PTMI_HIP(hipMemcpy(cnt.p, h_count_grids.data(), cells * sizeof(float), hipMemcpyHostToDevice));
    }
    launch_filter_pdfs(n, (const float*)rgb.p, (const float*)cnt.p, (float*)off.p, (float*)orad.p, use_bilateral, sigma_spatial, sigma_range, stream);
    PTMI_HIP(hipGetLastError());
    PTMI_HIP(hipStreamSynchronize(stream));
    h_filtered_formfactor.resize(cells); h_filtered_radiosity.resize(cells);
    PTMI_HIP(hipMemcpy(h_filtered_formfactor.data(), off.p, cells * sizeof(float), hipMemcpyDeviceToHost));
    PTMI_HIP(hipMemcpy(h_filtered_radiosity.data(), orad.p, cells * sizeof(float), hipMemcpyDeviceToHost));
    precomputeCDFsDevice(orad.p, 2, stream);
}

double SceneState::quadReach(const float* o) const {
    double far = 0.0, coord = 0.0;
    for (int a = 0; a < 3; a++) {
        far = std::max(far, std::max(std::fabs((double)o[a] - (double)coord_lo[a]), std::fabs((double)o[a] - (double)coord_hi[a])));
        coord = std::max(coord, std::max(std::fabs((double)o[a]), std::max(std::fabs((double)coord_lo[a]), std::fabs((double)coord_hi[a]))));
    }
    return far + coord * 0x1p-20;
}

void SceneState::checkQuadOrigin(const float* o, const float* d, const char* who) const {
    if (!(quad_edge_max > 0.0f)) return;
    double dmax = d ? 0.0 : 1.0;                       // d == nullptr: a unit direction
    for (int a = 0; a < 3; a++) {
        if (!std::isfinite(o[a]) || (d && !std::isfinite(d[a]))) return;      // t comes out NaN or infinite: accepted by neither side
        if (d) dmax = std::max(dmax, std::fabs((double)d[a]));
    }
    if (!((double)quad_edge_max * quadReach(o) * dmax <= kQuadReachBound))
        throw ArgError(std::string(who) + ": with quads in the scene, the largest quad edge times the origin's distance from the scene must not exceed 2^124");
}

// traversal choice (results are identical in all three; see device_scene.h)
void SceneState::chooseTraversal() {
    if (!d_nodes) return;
    if (bvh_depth > 62) d_scene.traversal = TRAVERSAL_STACK;           // the reference's stack-overflow rule can trigger
    else if ((int)h_primitives.size() <= sweep_max_prims) d_scene.traversal = TRAVERSAL_SWEEP;
    else d_scene.traversal = certified_default && d_scene.certified_ready() ? TRAVERSAL_CERTIFIED : (d_scene.gnodes ? TRAVERSAL_PACKED : TRAVERSAL_PHASED);
    // PHASED: measured faster than the segment-synchronous LANE walk from 128 primitives up (LDS-resident or not); PACKED: the
    // phased walk over the packed layout of scenes too large for LDS; LANE stays available through the override
    if (force_traversal >= 0 && !(force_traversal != TRAVERSAL_STACK && bvh_depth > 62)) d_scene.traversal = force_traversal;
    // the sweep reads through LDS, and its image - near/far node records, frame block, leaf records (csrc/kernels.hip: bounce_lds_bytes) - is the larger one
    const bool sweep_fits = d_scene.lds_resident && ptmi_sweep_leaves_lds_vecs(d_scene.n_nodes, d_scene.prim_stride, d_scene.n_prims, d_scene.sweep_leaves) * sizeof(float4) <= 64 * 1024;
    if (d_scene.traversal == TRAVERSAL_SWEEP && !sweep_fits) d_scene.traversal = TRAVERSAL_LANE;
    if (d_scene.traversal == TRAVERSAL_PACKED && !d_scene.gnodes) d_scene.traversal = TRAVERSAL_PHASED;
    // CERTIFIED needs the fast tree and the ancestor lists (triangle scenes of depth <= 62); otherwise the exact walk it stands for
    if (d_scene.traversal == TRAVERSAL_CERTIFIED && !d_scene.certified_ready())
        d_scene.traversal = (int)h_primitives.size() <= sweep_max_prims && sweep_fits ? TRAVERSAL_SWEEP : (d_scene.gnodes ? TRAVERSAL_PACKED : TRAVERSAL_PHASED);
    // the sweep's kernels have the primitive stride as a constant of the instantiation (traversal.h: intersect_sweep)
    if (d_scene.traversal == TRAVERSAL_SWEEP && d_scene.prim_stride != (d_scene.has_quads ? 4 : 3))
        throw ArgError("internal: the sweep reads 3 float4 per primitive without quads and 4 with");
}

}  // namespace ptmi
