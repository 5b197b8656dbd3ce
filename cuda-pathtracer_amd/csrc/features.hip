// features.hip — the feature pass (include/ptmi.h: ptmi_render_features, "shaded features"), a translation unit of its own so that
// its instantiations compile beside first_hit.hip's.  Compile with -ffp-contract=off (kernels.hip).
#include "light_sample.h"
#include "vertex_normal.h"
#include "albedo_texture.h"

namespace ptmi {

// ---------------------------------------------------------------------------------------------
// feature pass (include/ptmi.h: ptmi_render_features): g x g camera rays per local pixel through the stratum centres, first
// hit by the walk of the Radiosity view (the reference's hit for every ray), no RNG.  One thread per local pixel, local
// row-major; sums in stratum order (row j of the strata outer, column i inner), then x rcp_rn((float)(g * g)).
// SHADED (include/ptmi.h: "shaded features"): the context asks for a shaded feature (ptmi_set_feature_shading) whose table it
// has.  flags bit 0 with at.rec: a hit on a textured slot adds Kd_k * T (albedo_texture.h); bit 1 with vn.rec: a hit on a smooth
// slot adds the interpolated normal (vertex_normal.h) - the functions the path kernel calls, at the point that is added to P.
// Both tests are wave-uniform.  The lookups index at.rec, vn.rec and sc.prims by k, so they stay inside `live && hit`: a lane
// that is not live walks along (the small-scene walks are wave-synchronous) and a miss leaves k = -1.
// ---------------------------------------------------------------------------------------------
template <int MODE, bool HAS_QUADS, bool SHADED>
__global__ __launch_bounds__(kBlock) void ptmi_features(DeviceScene sc, TileMap tm, FrameParams fp, int g, FeatureBuffers fb,
                                                        VertexNormalTable vn, AlbedoTable at, int flags) {
    extern __shared__ float4 smem[];
    const int n = tm.local_rows * tm.width;
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    const bool live = idx < n;
    const int lr = live ? idx / tm.width : 0;
    const int x = live ? idx - lr * tm.width : 0;
    const int y = ((lr / tm.row_block) * tm.n_ranks + tm.rank) * tm.row_block + (lr % tm.row_block);
    const float gf = (float)g;
    f3 alb = mk3(0.0f, 0.0f, 0.0f), nrm = mk3(0.0f, 0.0f, 0.0f), pos = mk3(0.0f, 0.0f, 0.0f);
    float hits = 0.0f;
    LaneCounters cn = {0, 0, 0, 0, 0, 0, 0};
    [[maybe_unused]] const bool tex_on = SHADED ? (flags & 1) && at.rec : false;
    [[maybe_unused]] const bool smooth_on = SHADED ? (flags & 2) && vn.rec : false;
    for (int j = 0; j < g; j++) {
        for (int i = 0; i < g; i++) {
            const float u = ((float)x + ((float)i + 0.5f) / gf) / (float)tm.width;
            const float v = ((float)y + ((float)j + 0.5f) / gf) / (float)tm.height;
            f3 o, d;
            camera_ray_uv(fp, u, v, o, d);
            float t = 0.0f; int k = -1;
            const bool hit = first_hit<MODE, HAS_QUADS>(sc, smem, live, o, d, 1e-4f, t, k, cn);
            if (live && hit) {
                const f3 p = o + t * d;                                                   // one float triple for P, the UV and the normal
                f3 kd = xyz(sc.mats[3 * k + 1]), ns = xyz(sc.mats[3 * k]);
                if constexpr (SHADED) {
                    if (tex_on) albedo_at<HAS_QUADS>(sc, at, k, p, kd);                   // Kd(p) = Kd_k * T
                    if (smooth_on) vertex_normal<HAS_QUADS>(sc, vn, k, p, ns);            // Ns(p); the stored normal where it falls back
                }
                alb = alb + kd;
                nrm = nrm + ns;
                pos = pos + p;
                hits = hits + 1.0f;
            }
        }
    }
    if (!live) return;
    const float kk = rcp_rn((float)(g * g));
    fb.albedo[idx] = make_float4(alb.x * kk, alb.y * kk, alb.z * kk, hits * kk);
    fb.normal[idx] = make_float4(nrm.x * kk, nrm.y * kk, nrm.z * kk, 0.0f);
    fb.position[idx] = make_float4(pos.x * kk, pos.y * kk, pos.z * kk, 0.0f);
}

void launch_features(const DeviceScene& sc, const TileMap& tm, const FrameParams& fp, int g, const FeatureBuffers& fb,
                     const VertexNormalTable& vn, const AlbedoTable& at, int flags, hipStream_t s) {
    const int n = tm.local_rows * tm.width;
    if (n <= 0) return;
    const bool shaded = ((flags & 1) && at.rec) || ((flags & 2) && vn.rec);   // a flag whose table is absent asks for nothing
    first_hit_walk(sc, [&](auto mode, auto quads, size_t lds) {
        with_bool(shaded, [&](auto sh) {
            hipLaunchKernelGGL((ptmi_features<decltype(mode)::value, decltype(quads)::value, decltype(sh)::value>), dim3((n + kBlock - 1) / kBlock),
                               dim3(kBlock), lds, s, sc, tm, fp, g, fb, vn, at, flags);
        });
    });
}

}  // namespace ptmi
