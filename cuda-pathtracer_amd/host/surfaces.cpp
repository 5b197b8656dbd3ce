// surfaces.cpp — the check of a specular-surface table, as include/ptmi.h ("specular surfaces") states it.
#include "surfaces.h"

#include <string>

#include "application_state.h"   // ArgError

namespace ptmi {

void checkSurfaces(int n_prims, const int* kind, const float* ior) {
    if (n_prims < 1) throw ArgError("surfaces: n_prims must be >= 1");
    if (!kind) throw ArgError("surfaces: kind is NULL");
    for (int i = 0; i < n_prims; i++)
        if (kind[i] != kSurfaceDiffuse && kind[i] != kSurfaceMirror && kind[i] != kSurfaceGlass)
            throw ArgError("surfaces: kind of primitive " + std::to_string(i) + " must be 0 (diffuse), 1 (mirror) or 2 (glass)");
    if (ior)
        for (int i = 0; i < n_prims; i++)
            if (!(ior[i] >= 1.0f && ior[i] <= kSurfaceMaxIor))       // NaN fails both comparisons
                throw ArgError("surfaces: ior of primitive " + std::to_string(i) + " must be finite and in [1, 8]");
}

void checkSurfacesRough(int n_prims, const int* kind, const float* ior, const float* roughness) {
    if (n_prims < 1) throw ArgError("surfaces: n_prims must be >= 1");
    if (!kind) throw ArgError("surfaces: kind is NULL");
    for (int i = 0; i < n_prims; i++)
        if (kind[i] < kSurfaceDiffuse || kind[i] > kSurfaceRough)
            throw ArgError("surfaces: kind of primitive " + std::to_string(i) + " must be 0 (diffuse), 1 (mirror), 2 (glass) or 3 (rough metal)");
    if (ior)
        for (int i = 0; i < n_prims; i++)
            if (!(ior[i] >= 1.0f && ior[i] <= kSurfaceMaxIor))       // NaN fails both comparisons
                throw ArgError("surfaces: ior of primitive " + std::to_string(i) + " must be finite and in [1, 8]");
    if (roughness)
        for (int i = 0; i < n_prims; i++)
            if (!(roughness[i] >= kSurfaceMinRoughness && roughness[i] <= kSurfaceMaxRoughness))
                throw ArgError("surfaces: roughness of primitive " + std::to_string(i) + " must be finite and in [0.05, 1]");
}

}  // namespace ptmi
