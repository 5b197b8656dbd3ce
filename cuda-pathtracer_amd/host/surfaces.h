// surfaces.h — host half of the specular surfaces (include/ptmi.h: "specular surfaces"): the kinds and the check of a caller's
// table.  No device involved; ptmi_check_surfaces exposes the check.
#pragma once

namespace ptmi {

constexpr int kSurfaceDiffuse = 0, kSurfaceMirror = 1, kSurfaceGlass = 2;   // PTMI_SURFACE_*
constexpr float kSurfaceDefaultIor = 1.5f;                                  // ior == NULL
constexpr float kSurfaceMaxIor = 8.0f;

// throws ArgError: n_prims < 1, kind NULL, a kind outside 0 .. 2, an ior (NULL: none to check) that is NaN, infinite or outside
// [1, 8] - every entry, whatever its kind
void checkSurfaces(int n_prims, const int* kind, const float* ior);

}  // namespace ptmi
