// albedo_texture.h — the image's value at a path vertex on a textured primitive (include/ptmi.h: "albedo texture"; the table:
// device_scene.h AlbedoTable).  ptmi_render_nee (first_hit.hip) calls it directly before tp = tp * bsdf, the test hook
// (debug_hooks.hip: ptmi_debug_albedo_k) once per case.  binary32, uncontracted (-ffp-contract=off), in the order the header
// writes; the weights are vertex_normal.h's, and comparisons, not fminf / fmaxf, as there.
#pragma once
#include "vertex_normal.h"

namespace ptmi {

// the repeat: s = u - floorf(u) pinned into [0, 1); -1e-9f gives 1.0f and a NaN gives a NaN: both become 0
__device__ __forceinline__ float wrap_unit(float u) {
    const float s = u - floorf(u);
    return s >= 0.0f && s < 1.0f ? s : 0.0f;
}

// one coordinate blended with the weights of a half over (corner 0, corner a, corner b)
__device__ __forceinline__ float blend_coord(const HalfWeights& w, float c0, float ca, float cb) {
    return (w.b0 * c0 + w.b1 * ca) + w.b2 * cb;
}

// the image's value at (su, sv) in [0, 1)^2.  Every index below lies in 0 .. width - 1 / 0 .. height - 1 for such an argument.
__device__ __forceinline__ f3 albedo_texel(const AlbedoTable& at, float su, float sv) {
    const int W = at.width, H = at.height;
    const float4* __restrict__ tx = at.texel;
    if (at.filter == 0) {
        int i = (int)(su * (float)W), j = (int)(sv * (float)H);
        if (i > W - 1) i = W - 1;
        if (j > H - 1) j = H - 1;
        return xyz(tx[(size_t)j * (size_t)W + (size_t)i]);
    }
    const float x = su * (float)W - 0.5f, y = sv * (float)H - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    const float fx = x - x0, fy = y - y0;
    int i0 = (int)x0, j0 = (int)y0;
    int i1 = i0 + 1, j1 = j0 + 1;
    if (i0 < 0) i0 = W - 1;
    if (i1 > W - 1) i1 = 0;
    if (j0 < 0) j0 = H - 1;
    if (j1 > H - 1) j1 = 0;
    const f3 t00 = xyz(tx[(size_t)j0 * (size_t)W + (size_t)i0]), t01 = xyz(tx[(size_t)j0 * (size_t)W + (size_t)i1]);
    const f3 t10 = xyz(tx[(size_t)j1 * (size_t)W + (size_t)i0]), t11 = xyz(tx[(size_t)j1 * (size_t)W + (size_t)i1]);
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const f3 a = mk3(gx * t00.x + fx * t01.x, gx * t00.y + fx * t01.y, gx * t00.z + fx * t01.z);
    const f3 b = mk3(gx * t10.x + fx * t11.x, gx * t10.y + fx * t11.y, gx * t10.z + fx * t11.z);
    return mk3(gy * a.x + fy * b.x, gy * a.y + fy * b.y, gy * a.z + fy * b.z);
}

// what albedo_at found: the wrapped coordinates, the image's value there and whether the slot is textured
struct AlbedoLookup { float su, sv; f3 T; bool textured; };

// The lookup of leaf-order slot k at the point hp.  One 16-byte read decides an untextured slot; the second record, the
// primitive's vertices and the texels are read for a textured slot only.
template <bool HAS_QUADS>
__device__ __forceinline__ AlbedoLookup albedo_lookup(const DeviceScene& sc, const AlbedoTable& at, int k, f3 hp) {
    AlbedoLookup r = {0.0f, 0.0f, mk3(1.0f, 1.0f, 1.0f), false};
    const float4* __restrict__ rec = at.rec + 2 * (size_t)k;
    const float4 c01 = rec[0];                                // (u0, v0, u1, v1); u0 is a NaN for an untextured slot
    if (c01.x != c01.x) return r;
    const float4 c23 = rec[1];                                // (u2, v2, u3, v3)
    const int S = HAS_QUADS ? 4 : 3;                          // DeviceScene::prim_stride
    const float4* __restrict__ pr = sc.prims + (size_t)S * (size_t)k;
    const float4 p0 = pr[0], p1 = pr[1], p2 = pr[2];
    const f3 w = hp - xyz(p0);
    const HalfCoords h1 = half_coords(xyz(p1), xyz(p2), w);  // a triangle; a quad's (v00, v10, v11)
    float u = c01.x, v = c01.y;                               // no half with a valid den: the first corner's
    if (HAS_QUADS && __float_as_int(p0.w) != 0) {
        if (h1.valid && h1.r1 >= 0.0f) {
            const HalfWeights cw = clamped_weights(h1);
            u = blend_coord(cw, c01.x, c01.z, c23.x); v = blend_coord(cw, c01.y, c01.w, c23.y);
        } else {
            const HalfCoords h2 = half_coords(xyz(p2), xyz(pr[3]), w);                    // (v00, v11, v01)
            if (h2.valid) {
                const HalfWeights cw = clamped_weights(h2);
                u = blend_coord(cw, c01.x, c23.x, c23.z); v = blend_coord(cw, c01.y, c23.y, c23.w);
            }
        }
    } else if (h1.valid) {
        const HalfWeights cw = clamped_weights(h1);
        u = blend_coord(cw, c01.x, c01.z, c23.x); v = blend_coord(cw, c01.y, c01.w, c23.y);
    }
    r.su = wrap_unit(u); r.sv = wrap_unit(v);
    r.T = albedo_texel(at, r.su, r.sv);
    r.textured = true;
    return r;
}

// Kd(p) = Kd_k * T of leaf-order slot k at the point hp: kd comes in as Kd_k and stays it for an untextured slot
template <bool HAS_QUADS>
__device__ __forceinline__ void albedo_at(const DeviceScene& sc, const AlbedoTable& at, int k, f3 hp, f3& kd) {
    const AlbedoLookup r = albedo_lookup<HAS_QUADS>(sc, at, k, hp);
    if (r.textured) kd = kd * r.T;
}

}  // namespace ptmi
