// prim_sample.h — Primitive::sampleUniform (primitive.h:150-191) on the device, stated once for its two callers: the radiosity
// pre-pass's form factors (form_factors.hip) and the emitter samples of next-event estimation (first_hit.hip: ptmi_render_nee).
// Compile with -ffp-contract=off (see include/ptmi_math.h, pt_vec.h).
#pragma once
#include "pt_vec.h"

namespace ptmi {
namespace {

// A primitive as the samplers see it: the radiosity pre-pass's load-order geometry (form_factors.hip: load_geom) and the
// emitter records of next-event estimation (first_hit.hip: ptmi_render_nee).  Quads: v0..v3 = v00, v10, v11, v01.
struct Geom { f3 v0, v1, v2, v3; int type; float area, ratio; f3 normal, centroid; };

// primitive.h:153-157
__device__ __forceinline__ f3 bary_point(f3 a, f3 b, f3 c, float r1, float r2) {
    const float sqrt_r1 = sqrt_rn(r1);
    const float u = 1.0f - sqrt_r1;
    const float v = sqrt_r1 * (1.0f - r2);
    const float w = sqrt_r1 * r2;
    return u * a + v * b + w * c;
}
// Primitive::sampleUniform (primitive.h:150-191); the quad's area ratio comes precomputed from the host
template <bool HAS_QUADS>
__device__ __forceinline__ f3 sample_uniform(const Geom& g, float r1, float r2) {
    if (!HAS_QUADS || g.type == 0) return bary_point(g.v0, g.v1, g.v2, r1, r2);      // triangle-only scenes: v3 / ratio / type stay out of registers
    if (r1 < g.ratio) return bary_point(g.v0, g.v1, g.v3, r1 / g.ratio, r2);                     // (v00, v10, v01)
    return bary_point(g.v1, g.v2, g.v3, (r1 - g.ratio) / (1.0f - g.ratio), r2);                  // (v10, v11, v01)
}

}  // namespace
}  // namespace ptmi
