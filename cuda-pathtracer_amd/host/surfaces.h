// surfaces.h — host half of the specular surfaces (include/ptmi.h: "specular surfaces"): the kinds and the check of a caller's
// table.  No device involved; ptmi_check_surfaces exposes the check.
#pragma once

namespace ptmi {

constexpr int kSurfaceDiffuse = 0, kSurfaceMirror = 1, kSurfaceGlass = 2;   // PTMI_SURFACE_*
constexpr float kSurfaceDefaultIor = 1.5f;                                  // ior == NULL
constexpr float kSurfaceMaxIor = 8.0f;
constexpr int kSurfaceRough = 3;                                            // PTMI_SURFACE_ROUGH (include/ptmi.h: "rough metal")
constexpr float kSurfaceDefaultRoughness = 0.3f;                            // roughness == NULL
constexpr float kSurfaceMinRoughness = 0.05f, kSurfaceMaxRoughness = 1.0f;

// throws ArgError: n_prims < 1, kind NULL, a kind outside 0 .. 2, an ior (NULL: none to check) that is NaN, infinite or outside
// [1, 8] - every entry, whatever its kind
void checkSurfaces(int n_prims, const int* kind, const float* ior);

// the check of ptmi_set_surfaces_rough: as checkSurfaces with kinds 0 .. 3, and a roughness (NULL: none to check) that is NaN,
// infinite or outside [0.05, 1] - every entry, whatever its kind
void checkSurfacesRough(int n_prims, const int* kind, const float* ior, const float* roughness);

}  // namespace ptmi
