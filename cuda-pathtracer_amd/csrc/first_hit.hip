// first_hit.hip — the kernels that trace one ray at a time to its first hit (traversal.h: first_hit): the Radiosity view and
// next-event estimation (the feature pass: features.hip).  Compile with -ffp-contract=off (kernels.hip).
#include "light_sample.h"
#include "vertex_normal.h"
#include "albedo_texture.h"
#include "lens.h"
#include "medium.h"

namespace ptmi {

// ---------------------------------------------------------------------------------------------
// render_radiosity (integrator.h:460-504): a visualisation pass, one thread per pixel, not performance-critical; the walk: first_hit_walk
// ---------------------------------------------------------------------------------------------
template <int MODE, bool HAS_QUADS>
__global__ __launch_bounds__(kBlock) void ptmi_render_radiosity(DeviceScene sc, TileMap tm, PathState st, FrameParams fp,
                                                                unsigned char* __restrict__ rgb8, float* __restrict__ radiance) {
    extern __shared__ float4 smem[];
    const int n = tm.local_rows * tm.width;
    const int slot = blockIdx.x * kBlock + threadIdx.x;
    const bool live = slot < n;
    int x = 0, y = 0;
    Rng rng = {0, 0, 0, 0, 0, 0};
    if (live) {
        global_pixel(tm, slot, x, y);
        const uint4 e = st.E[slot]; const uint2 f = st.F[slot];
        rng = Rng{e.x, e.y, e.z, e.w, f.x, f.y};                                      // curandState local_rng = rand_state[pixel_index]
    }
    f3 color = mk3(0.0f, 0.0f, 0.0f);
    LaneCounters cn = {0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < fp.spp; s++) {
        f3 o = mk3(0, 0, 0), d = mk3(0, 0, 1);
        if (live) camera_ray(fp, tm, x, y, rng, o, d);
        float t = 0.0f; int k = -1;
        const bool hit = first_hit<MODE, HAS_QUADS>(sc, smem, live, o, d, 1e-4f, t, k, cn);
        if (live && hit) {
            color = color + xyz(sc.mats[3 * k + 2]);                                  // color += si.Le
            color = color + (sc.radiosity ? xyz(sc.radiosity[k]) : mk3(0.0f, 0.0f, 0.0f));   // color += prim->getRadiosity()
        }
    }
    if (!live) return;
    const float kk = rcp_rn((float)fp.spp);
    const float c[3] = {color.x * kk, color.y * kk, color.z * kk};
    int ox, olr;
    slot_to_local(tm, slot, ox, olr);
    const size_t out = (size_t)olr * (size_t)tm.width + (size_t)ox;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        if (radiance) radiance[out * 3 + ch] = c[ch];
        if (rgb8) rgb8[out * 3 + ch] = (unsigned char)(255.99f * sqrt_rn(fminf(c[ch], 1.0f)));
    }
    st.E[slot] = make_uint4(rng.v0, rng.v1, rng.v2, rng.v3);                          // rand_state[pixel_index] = local_rng
    st.F[slot] = make_uint2(rng.v4, rng.d);
}

void launch_render_radiosity(const DeviceScene& sc, const TileMap& tm, const PathState& st, const FrameParams& fp,
                             unsigned char* rgb8, float* radiance, hipStream_t s) {
    const int n = tm.local_rows * tm.width;
    if (n <= 0) return;
    first_hit_walk(sc, [&](auto mode, auto quads, size_t lds) {
        hipLaunchKernelGGL((ptmi_render_radiosity<decltype(mode)::value, decltype(quads)::value>), dim3((n + kBlock - 1) / kBlock), dim3(kBlock), lds, s,
                           sc, tm, st, fp, rgb8, radiance);
    });
}

// ---------------------------------------------------------------------------------------------
// next-event estimation with MIS (include/ptmi.h: ptmi_config.next_event; the contract, float for float, is written there).
// One lane per queued pixel runs n_frames x spp samples to their end, so a pixel's sums are added in sample order.  Path rays
// and shadow rays go through ONE call site of first_hit_walk's walk (the reference's hit for every ray): a lane alternates
// between its path ray and the shadow ray of the vertex it has just shaded, whose contribution is computed before the walk
// and added if the walk's closest hit is the sampled emitter.  Every RNG draw of a vertex - Russian roulette, u_sel, r1, r2,
// u, v - is made before its shadow ray is traced, in the contract's order, so visibility never moves a draw.
// ---------------------------------------------------------------------------------------------
// specular surfaces (include/ptmi.h: "specular surfaces"; the table: device_scene.h SurfaceTable).  SPEC: the context has a table
// with a mirror or glass primitive; a vertex on one makes no light sample and no cosine sample and goes on along the reflected or
// refracted direction, and what the next path ray finds (an emitter, the environment) counts in full.
// SURF (include/ptmi.h: "rough metal"): 0 no table; 1 a table of mirror and glass only (SPEC); 2 a table with a rough-metal
// primitive as well: such a vertex draws what a diffuse one draws, its light sample evaluates the GGX lobe and its BSDF sample
// comes from rough.h; both are computed here, before the shadow walk, so only `ended` joins the state that crosses a walk.
// SMOOTH (include/ptmi.h: "vertex normals"; the table: device_scene.h VertexNormalTable): the context has a table with a smooth
// primitive; a vertex on one takes the normal interpolated at the hit point (vertex_normal.h) where sn is formed, and everything
// below reads it from there.  The emitter pdf above keeps the geometric normal.
// TEX (include/ptmi.h: "albedo texture"; the table: device_scene.h AlbedoTable): the context has a table with a textured primitive;
// a vertex on one multiplies Kd by the image's value at the hit point (albedo_texture.h) directly before the throughput takes it,
// after the roulette.  at.filter is a wave-uniform runtime switch.
// lens (include/ptmi.h: "thin lens"; the block: host/lens.cpp) is a wave-uniform runtime switch too, not a template parameter: with
// a block the sample's primary ray comes from lens.h - two draws in front of the jitter's, an origin on the lens - and nothing
// below the camera ray changes.  nullptr: the pinhole.
// medium (include/ptmi.h: "participating medium"; the block: host/medium.cpp) is the third such switch: with a block every path ray
// makes the free-flight draw directly after its walk and may have a medium vertex (mv) in front of the hit or the miss; that vertex
// goes through the roulette, the light sample and the two draws of the surface vertex below, with the phase function in the place
// of the BSDF, and every visible shadow ray takes the transmittance of its own segment.  The records are read after the walk,
// where they are used (medium.h).  MEDIUM is a template parameter and not a fourth runtime switch: as one, it cost 39 of the 144
// instantiations a wave per SIMD; the MEDIUM = false instantiations keep the parent's registers and waves and
// give its frames bit for bit (their code differs by the one more kernel argument).
// the weight of a vertex's light sample of density p towards wi: light_weight of a surface vertex (whose cosine test the caller
// makes), or the phase function's at a medium vertex (medium.h), which has no such test
template <int SURF, bool MEDIUM>
__device__ __forceinline__ bool vertex_light_weight(const float4* __restrict__ medium, bool mv, const f3& d, bool rough, const RoughVertex& rv, const f3& wi,
                                                    float cos_s, float p, float& w) {
    if constexpr (MEDIUM) {
        if (mv) {
            w = medium_light_weight(medium[1].w, d, wi, p);
            return true;
        }
    }
    return light_weight<SURF>(rough, rv, wi, cos_s, p, w);
}

template <int MODE, bool HAS_QUADS, bool ENV, int SURF, bool SMOOTH, bool TEX, bool MEDIUM>
__global__ __launch_bounds__(kBlock) void ptmi_render_nee(DeviceScene sc, EmitterTable em, EnvTable ev, SurfaceTable sf, TileMap tm, PathState st, FrameParams fp,
                                                          const int* __restrict__ queue, int n, int first, int next_event, VertexNormalTable vn, AlbedoTable at,
                                                          const float4* __restrict__ lens, const float4* __restrict__ medium) {
    extern __shared__ float4 smem[];
    constexpr bool SPEC = SURF != 0;
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= n) return;                                    // the walks are per lane: no barrier below
    const int slot = queue ? queue[idx] : idx;
    int x, y;
    global_pixel(tm, slot, x, y);
    const uint4 e = st.E[slot]; const uint2 f = st.F[slot];
    Rng rng = {e.x, e.y, e.z, e.w, f.x, f.y};
    f3 color = first ? mk3(0.0f, 0.0f, 0.0f) : xyz(st.D[slot]);
    LaneCounters cn = {0, 0, 0, 0, 0, 0, 0};
    // wave-uniform switches of the ENV, SPEC, SMOOTH and TEX instantiations; without any of them they fold to the NEE kernel
    // (a lens or a medium brings next_event = 0 to the instantiation without any of them, which only next_event = 1 reached before)
    const bool nee_on = ENV || SPEC || SMOOTH || TEX || MEDIUM || lens ? next_event != 0 : true;   // light samples and MIS weights at all
    const bool env_on = ENV ? ev.sampled != 0 : false;       // the environment is one of the lights: five draws, selection by q
    const float q = ENV ? ev.q : 0.0f, omq = 1.0f - q;
    for (int frame = 0; frame < fp.n_frames; frame++) {
        if (frame > 0) {                                     // frame batch: bank the previous frame's sum, as shade_step does
            fp.frame_color[(unsigned int)(frame - 1) * (unsigned int)fp.n_local + (unsigned int)slot] = make_float4(color.x, color.y, color.z, 0.0f);
            color = mk3(0.0f, 0.0f, 0.0f);
        }
        for (int s = 0; s < fp.spp; s++) {
            f3 o, d;
            if (lens) lens_ray(lens, x, y, rng, o, d);       // the block is read in there, per sample
            else camera_ray(fp, tm, x, y, rng, o, d);
            f3 tp = mk3(1.0f, 1.0f, 1.0f), L = mk3(0.0f, 0.0f, 0.0f);
            float pb_prev = 0.0f;                            // pdf of the cosine sample that made the current path ray
            bool spec_prev = false;                          // SPEC: a mirror or glass vertex made the current path ray: no MIS weight
            int depth = 0;
            bool shadow = false;                             // the next walk is the shadow ray (so, sd) of the last vertex
            f3 so = o, sd = d, contrib = mk3(0.0f, 0.0f, 0.0f);
            int s_slot = -1;                                 // the sampled emitter's slot; -1: the environment (visible iff nothing is hit)
            bool ended = false;                              // SURF = 2: the rough vertex ended the path; its shadow ray is still to walk
            while (true) {
                const f3 ro = shadow ? so : o, rd = shadow ? sd : d;
                float t = 0.0f; int k = -1;
                const bool hit = first_hit<MODE, HAS_QUADS>(sc, smem, true, ro, rd, 1e-4f, t, k, cn);
                if (shadow) {                                // visible iff the closest hit is the sampled emitter
                    if (ENV && s_slot < 0 ? !hit : (hit && k == s_slot)) {
                        if constexpr (MEDIUM) {              // the transmittance of the shadow ray's own segment
                            const float T = medium_transmittance(medium, so, sd, ENV && s_slot < 0 ? INFINITY : t);
                            L = L + mk3(contrib.x * T, contrib.y * T, contrib.z * T);
                        } else L = L + contrib;
                    }
                    shadow = false;
                    if (SURF == 2 && ended) break;
                    continue;
                }
                [[maybe_unused]] bool mv = false;                                         // a medium vertex in front of the hit or the miss
                [[maybe_unused]] float tm = 0.0f;
                if constexpr (MEDIUM) {                                                          // one draw per path ray, whatever comes of it
                    const float u_m = rng_uniform(rng);
                    mv = medium_free_flight(medium, o, d, hit ? t : INFINITY, u_m, tm);
                }
                if (!hit && !mv) {                                                        // integrator.h:198-201
                    if constexpr (ENV) {                                                  // the path ray leaves the scene: E(d)
                        const float4 te = ev.texel[env_texel(ev, d)];
                        const f3 c = tp * xyz(te);
                        if (env_on && depth > 0 && !(SPEC && spec_prev)) {
                            const float w = mis_power_heuristic(pb_prev, q * te.w);
                            L = L + mk3(c.x * w, c.y * w, c.z * w);
                        } else L = L + c;
                    }
                    break;
                }
                if (MEDIUM && mv) k = 0;                                                          // nothing of primitive k is used: x emits nothing, albedo for Kd
                f3 nrm = xyz(sc.mats[3 * k]);
                f3 bsdf = MEDIUM && mv ? xyz(medium[2]) : xyz(sc.mats[3 * k + 1]);
                const f3 Le = xyz(sc.mats[3 * k + 2]);
                const f3 hp = o + (MEDIUM && mv ? tm : t) * d;                                     // triangle.h:90; the medium vertex x
                if (!mv) {
                    const float4 pe = depth > 0 && nee_on && !(SPEC && spec_prev) ? em.pdf_area[k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    const float pa = pe.w;
                    if (pa > 0.0f) {                                                      // an emitter found by the BSDF sample
                        float p_l = (pa * (t * t)) / fabsf(dot(xyz(pe), d));             // the geometric normal: area -> solid angle
                        if (env_on) p_l = omq * p_l;
                        const float w = mis_power_heuristic(pb_prev, p_l);
                        const f3 c = tp * Le;
                        L = L + mk3(c.x * w, c.y * w, c.z * w);
                    } else L = L + tp * Le;                                               // integrator.h:204
                }
                if (depth > 2) {                                                          // integrator.h:207-212
                    const float max_tp = fmaxf(tp.x, fmaxf(tp.y, tp.z));
                    const float rr_prob = fminf(max_tp, 0.95f);
                    if (rng_uniform(rng) > rr_prob) break;
                    tp = div_scalar(tp, rr_prob);
                }
                if constexpr (TEX) { if (!mv) albedo_at<HAS_QUADS>(sc, at, k, hp, bsdf); }   // Kd(p) = Kd_k * T, after the roulette
                tp = tp * bsdf;                                                           // integrator.h:215
                if (length(tp) < 1e-5f) break;                                            // integrator.h:218
                if constexpr (SMOOTH) { if (!mv) vertex_normal<HAS_QUADS>(sc, vn, k, hp, nrm); }   // after the throughput exit, not at the hit
                const f3 sn = dot(d, nrm) < 0 ? nrm : -nrm;                               // integrator.h:221-222
                const f3 o2 = MEDIUM && mv ? hp : hp + 1e-4f * sn;                            // integrator.h:266; a medium vertex has no offset
                [[maybe_unused]] bool rough = false;                                      // SURF = 2: this vertex is rough metal (rv)
                [[maybe_unused]] RoughVertex rv;
                if constexpr (SPEC) {
                    const float2 sr = sf.rec[k];
                    const int kind = mv ? 0 : __float_as_int(sr.x);
                    if (SURF == 2 ? kind == 1 || kind == 2 : kind != 0) {                 // no light sample, no cosine sample
                        float u = 1.0f;
                        if (kind == 2) u = rng_uniform(rng);                              // glass: one draw whatever comes of it
                        bool reflect;
                        [[maybe_unused]] float fr;
                        f3 next;
                        const bool walk = specular_vertex(d, nrm, sn, kind, sr.y, u, reflect, fr, next);
                        depth++;
                        if (depth >= fp.max_depth) break;
                        if (!walk) break;                                                 // no walk starts with a NaN direction
                        o = reflect ? o2 : hp - 1e-4f * sn;
                        d = unit_vector(next);
                        spec_prev = true;
                        continue;
                    }
                    spec_prev = false;
                    if constexpr (SURF == 2) {
                        rough = kind == 3;
                        if (rough) rv = rough_vertex(sn, d, sr.y);
                    }
                }
                if (nee_on && depth + 1 < fp.max_depth && (em.n > 0 || env_on)) {         // NEE: three draws (five with an environment) whatever comes of them
                    float u_sel = rng_uniform(rng);
                    const float r1 = rng_uniform(rng);
                    const float r2 = rng_uniform(rng);
                    bool to_env = false;
                    if (env_on) {
                        const float r3 = rng_uniform(rng);
                        const float r4 = rng_uniform(rng);
                        to_env = u_sel <= q;
                        if (to_env) {
                            int r, j;
                            f3 wi;
                            const float4 te = env_sample(ev, r1, r2, r3, r4, r, j, wi);
                            const float cos_s = dot(sn, wi);
                            const float p_e = q * te.w;
                            float w;
                            if (((MEDIUM && mv) || cos_s > 0.0f) && p_e > 0.0f && p_e <= FLT_MAX && vertex_light_weight<SURF, MEDIUM>(medium, mv, d, rough, rv, wi, cos_s, p_e, w)) {
                                const f3 c = tp * xyz(te);
                                contrib = mk3(c.x * w, c.y * w, c.z * w);
                                so = o2; sd = wi; s_slot = -1;
                                shadow = true;
                            }
                        } else u_sel = (u_sel - q) / omq;
                    }
                    if (!to_env) {
                        const EmitterSample es = emitter_sample<HAS_QUADS>(em, u_sel, r1, r2, o2, env_on, omq);
                        const f3 wi = es.wi;
                        const float cos_s = dot(sn, wi);
                        float w;
                        if (((MEDIUM && mv) || cos_s > 0.0f) && es.ok && vertex_light_weight<SURF, MEDIUM>(medium, mv, d, rough, rv, wi, cos_s, es.p_l, w)) {
                            const f3 c = tp * xyz(es.rec[5]);
                            contrib = mk3(c.x * w, c.y * w, c.z * w);
                            so = o2; sd = wi; s_slot = es.slot;
                            shadow = true;
                        }
                    }
                }
                const float u = rng_uniform(rng);                                         // integrator.h:63-64
                const float vv = rng_uniform(rng);
                depth++;
                if (depth >= fp.max_depth) break;                                         // (no shadow ray pending: NEE needs depth + 1 < max_depth)
                if (MEDIUM && mv) {                                                       // the phase sample: u is the cosine's draw, vv the azimuth's
                    const float g = medium[1].w;
                    const float c = hg_sample(g, u);
                    pb_prev = hg_value(g, c);                                             // of the sampled cosine itself
                    d = hg_direction(d, c, vv);
                    o = hp;
                    continue;
                }
                if constexpr (SURF == 2) {
                    if (rough) {                                                          // u, vv are the contract's u1, u2
                        f3 next;
                        float wgt = 0.0f, p_b = 0.0f;
                        bool on = rv.ok && rough_sample(rv, u, vv, next, wgt, p_b);       // the grazing exit; a sample below the horizon
                        if (on) {
                            const float len2 = dot(next, next);
                            on = len2 > 0.0f && len2 <= FLT_MAX;                          // no walk starts with a NaN direction
                        }
                        if (!on) {                                                        // the path ends; a light sample made above still counts
                            if (!shadow) break;
                            ended = true;
                            continue;
                        }
                        tp = mk3(tp.x * wgt, tp.y * wgt, tp.z * wgt);
                        pb_prev = p_b;
                        o = o2;
                        d = unit_vector(next);
                        continue;
                    }
                }
                const f3 next = cosine_hemisphere(sn, u, vv);                             // integrator.h:230
                pb_prev = cos_over_pi(fmaxf(dot(sn, next), 0.0f));
                o = o2;
                d = unit_vector(next);
            }
            color = color + L;                                                            // integrator.h:390
        }
    }
    st.D[slot] = make_float4(color.x, color.y, color.z, __uint_as_float(0u));
    st.E[slot] = make_uint4(rng.v0, rng.v1, rng.v2, rng.v3);
    st.F[slot] = make_uint2(rng.v4, rng.d);
}

void launch_render_nee(const DeviceScene& sc, const EmitterTable& em, const PerLaneTables& t, bool next_event, const TileMap& tm, const PathState& st,
                       const FrameParams& fp, const int* queue, int n, bool first, hipStream_t s) {
    if (n <= 0) return;
    first_hit_walk(sc, [&](auto mode, auto quads, size_t lds) {
        with_bool(t.env.texel != nullptr, [&](auto with_env) {
            auto launch = [&](auto surf_kinds) {
                with_bool(t.vn.rec != nullptr, [&](auto smooth) {
                    with_bool(t.at.rec != nullptr, [&](auto tex) {
                        with_bool(t.medium != nullptr, [&](auto with_medium) {
                            hipLaunchKernelGGL((ptmi_render_nee<decltype(mode)::value, decltype(quads)::value, decltype(with_env)::value,
                                                                decltype(surf_kinds)::value, decltype(smooth)::value, decltype(tex)::value,
                                                                decltype(with_medium)::value>),
                                               dim3((n + kBlock - 1) / kBlock), dim3(kBlock), lds, s, sc, em, t.env, t.surf, tm, st, fp, queue, n, first ? 1 : 0,
                                               next_event ? 1 : 0, t.vn, t.at, t.lens, t.medium);
                        });
                    });
                });
            };
            if (t.surf.rec == nullptr) launch(std::integral_constant<int, 0>{});
            else if (!t.rough) launch(std::integral_constant<int, 1>{});
            else launch(std::integral_constant<int, 2>{});
        });
    });
}

}  // namespace ptmi
