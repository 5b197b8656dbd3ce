// vertex_normal.h — the shading normal of a path vertex on a smooth primitive (include/ptmi.h: "vertex normals"; the table:
// device_scene.h VertexNormalTable).  ptmi_render_nee (first_hit.hip) calls it where it forms sn, the test hook
// (debug_hooks.hip: ptmi_debug_vertex_normal_k) once per case.  binary32, uncontracted (-ffp-contract=off), in the order the
// header writes; comparisons, not fminf / fmaxf, so that a NaN coordinate stays a NaN through the clamps.
#pragma once
#include <float.h>

#include "pt_device.h"

namespace ptmi {

// (den, r1, r2) of w over the edges (ea, eb): w = r1 ea + r2 eb in the least-squares sense; valid: den is a positive finite number
struct HalfCoords { float den, r1, r2; bool valid; };
__device__ __forceinline__ HalfCoords half_coords(f3 ea, f3 eb, f3 w) {
    const float d00 = dot(ea, ea), d01 = dot(ea, eb), d11 = dot(eb, eb), d20 = dot(w, ea), d21 = dot(w, eb);
    HalfCoords h;
    h.den = d00 * d11 - d01 * d01;
    h.valid = h.den > 0.0f && h.den <= FLT_MAX;
    h.r1 = (d11 * d20 - d01 * d21) / h.den;
    h.r2 = (d00 * d21 - d01 * d20) / h.den;
    return h;
}

// the clamped weights (b0, b1, b2) of h over (corner 0, corner a, corner b): by comparison, so a NaN stays a NaN.  The normals
// here and the texture coordinates of albedo_texture.h are blended with these
struct HalfWeights { float b0, b1, b2; };
__device__ __forceinline__ HalfWeights clamped_weights(const HalfCoords& h) {
    HalfWeights w;
    w.b1 = h.r1 < 0.0f ? 0.0f : (h.r1 > 1.0f ? 1.0f : h.r1);
    const float m = 1.0f - w.b1;
    w.b2 = h.r2 < 0.0f ? 0.0f : (h.r2 > m ? m : h.r2);
    w.b0 = m - w.b2;
    return w;
}

// the clamped weights of h and the normal they give over (n0, na, nb); false: the sum has no direction, nrm stays
__device__ __forceinline__ bool blend_normals(const HalfCoords& h, f3 n0, f3 na, f3 nb, f3& nrm) {
    const HalfWeights cw = clamped_weights(h);
    const float b0 = cw.b0, b1 = cw.b1, b2 = cw.b2;
    const f3 sum = mk3((b0 * n0.x + b1 * na.x) + b2 * nb.x, (b0 * n0.y + b1 * na.y) + b2 * nb.y, (b0 * n0.z + b1 * na.z) + b2 * nb.z);
    const float len2 = dot(sum, sum);
    if (!(len2 > 0.0f && len2 <= FLT_MAX)) return false;
    nrm = unit_vector(sum);
    return true;
}

// The normal of leaf-order slot k at the point hp: nrm comes in as the stored normal and stays it for a flat primitive and
// wherever the contract falls back; true: nrm is the interpolated unit normal.  One 16-byte read decides; the other corners and
// the primitive's record are read for a smooth slot only.
template <bool HAS_QUADS>
__device__ __forceinline__ bool vertex_normal(const DeviceScene& sc, const VertexNormalTable& vn, int k, f3 hp, f3& nrm) {
    const int S = HAS_QUADS ? 4 : 3;                          // DeviceScene::prim_stride
    const float4* __restrict__ rec = vn.rec + (size_t)S * (size_t)k;
    const float4 c0 = rec[0];
    if (__float_as_int(c0.w) == 0) return false;
    const float4 c1 = rec[1], c2 = rec[2];
    const float4* __restrict__ pr = sc.prims + (size_t)S * (size_t)k;
    const float4 p0 = pr[0], p1 = pr[1], p2 = pr[2];
    const f3 w = hp - xyz(p0);
    const HalfCoords h1 = half_coords(xyz(p1), xyz(p2), w);  // a triangle; a quad's (v00, v10, v11)
    if (HAS_QUADS && __float_as_int(p0.w) != 0) {
        if (h1.valid && h1.r1 >= 0.0f) return blend_normals(h1, xyz(c0), xyz(c1), xyz(c2), nrm);
        const float4 c3 = rec[3], p3 = pr[3];
        const HalfCoords h2 = half_coords(xyz(p2), xyz(p3), w);                           // (v00, v11, v01)
        if (!h2.valid) return false;
        return blend_normals(h2, xyz(c0), xyz(c2), xyz(c3), nrm);
    }
    if (!h1.valid) return false;
    return blend_normals(h1, xyz(c0), xyz(c1), xyz(c2), nrm);
}

}  // namespace ptmi
