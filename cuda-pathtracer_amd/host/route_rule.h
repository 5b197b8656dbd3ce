// route_rule.h — which path-tracing runs take the per-lane kernel ptmi_render_nee instead of the bounce-kernel queue loop, and which
// configs the features that send them there refuse.  Pure: nothing of HIP is included, so the rule runs (and is tested,
// tests/test_route_rule.py) without a GPU.  csrc/c_api.cpp asks it for refusals, host/render_run.cpp for the route.
// Why each feature takes that kernel (ONE launch for the whole frame, batch or pass: no chunks, no refill, no launch order by cost): next_event
// is its estimator; it is the kernel that looks an environment up where a path ray misses (for both values of next_event), continues a path
// through mirror, glass and rough metal, shades a smooth primitive with the interpolated normal, multiplies a textured primitive's Kd by the image,
// starts a sample on a thin lens and samples a free flight through a medium.  It traces the reference's hits and samples the BSDF: hence the refusals.
#pragma once
#include <string>

namespace ptmi {
enum RouteFeature { kRouteNextEvent, kRouteEnvironment, kRouteSurfaces, kRouteVertexNormals, kRouteAlbedoTexture, kRouteLens, kRouteMedium, kRouteFeatures };
enum RouteField { kRouteIntegrator, kRouteSamplingMode, kRouteFastTree, kRouteFields };   // both in the order ptmi_set_config checks them

// One row per feature.  ptmi_set_config says "<is_set> <kNeeds[field]>: <why_config[field] or why_fast>", the feature's setter
// "<setter>: the config has <kHas[field]><why_setter[field] or why_fast>": each direction keeps its own wording.  A field without a
// why is allowed (the Radiosity view keeps the pinhole and sees vacuum); next_event is a config field and has no setter.
struct RouteRow { const char *is_set, *setter, *why_config[2], *why_setter[2], *why_fast; };
constexpr const char* kNeeds[kRouteFields] = {"integrator 0 (PathTracing)", "sampling_mode 0 (BSDF)", "fast_tree 0"};
constexpr const char* kHas[kRouteFields] = {"integrator 1 (Radiosity), ", "a guided sampling_mode, ", "fast_tree 1; "};
constexpr const char *kBounce = "the guided modes run through the bounce kernels", *kBounceWhich = "which runs through the bounce kernels";
constexpr RouteRow kRouteRows[kRouteFeatures] = {
    {"next_event needs", nullptr, {"the Radiosity view traces first hits only", "MIS against the guided modes' grid pdf is not implemented"}, {},
     "NEE frames always trace the reference's hits"},
    {"an environment is set: it needs", "environment", {"the Radiosity view traces first hits only", "the guided modes do not look the environment up"},
     {"which traces first hits only", "which does not look the environment up"}, "environment frames always trace the reference's hits"},
    {"specular surfaces are set: they need", "surfaces", {"the Radiosity view traces first hits only", "the guided modes sample a diffuse lobe at every vertex"},
     {"which traces first hits only", "which samples a diffuse lobe at every vertex"}, "specular frames always trace the reference's hits"},
    {"vertex normals are set: they need", "vertex normals", {"the Radiosity view shades nothing", "the guided modes' grids lie about the stored normal"},
     {"which shades nothing", "whose grids lie about the stored normal"}, "frames with vertex normals always trace the reference's hits"},
    {"an albedo texture is set: it needs", "albedo texture", {"the Radiosity view ignores the texture", kBounce},
     {"which ignores the texture", kBounceWhich}, "textured frames always trace the reference's hits"},
    {"a lens is set: it needs", "lens", {nullptr, kBounce}, {nullptr, kBounceWhich}, "frames through a lens always trace the reference's hits"},
    {"a medium is set: it needs", "medium", {nullptr, kBounce}, {nullptr, kBounceWhich}, "frames through a medium always trace the reference's hits"},
};
// the first refusal feature f meets under a config, in field order, in its setter's words (to_config: in ptmi_set_config's); empty: none
inline std::string featureRefusal(int f, int integrator, int sampling_mode, int fast_tree, bool to_config = false) {
    const RouteRow& r = kRouteRows[f];
    const bool offends[kRouteFields] = {integrator != 0, sampling_mode != 0, fast_tree != 0};
    for (int k = 0; k < kRouteFields; k++) {
        const char* why = k == kRouteFastTree ? r.why_fast : to_config ? r.why_config[k] : r.why_setter[k];
        if (offends[k] && why) return to_config ? std::string(r.is_set) + " " + kNeeds[k] + ": " + why : std::string(r.setter) + ": the config has " + kHas[k] + why;
    }
    return {};
}
// the first refusal a config meets under the features present (a mask of 1 << RouteFeature), in feature order; empty: none
inline std::string configRefusal(unsigned features, int integrator, int sampling_mode, int fast_tree) {
    std::string why;
    for (int f = 0; f < kRouteFeatures && why.empty(); f++)
        if (features >> f & 1) why = featureRefusal(f, integrator, sampling_mode, fast_tree, true);
    return why;
}
struct Route { bool per_lane, blocks; };   // the run is one launch of ptmi_render_nee; it is handed the lens and the medium blocks (path tracing only)
inline Route routeOf(unsigned features, int integrator) { return {features != 0 && integrator == 0, integrator == 0}; }
}  // namespace ptmi
