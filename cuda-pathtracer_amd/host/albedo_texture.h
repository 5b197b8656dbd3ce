// albedo_texture.h — host half of the albedo texture (include/ptmi.h: "albedo texture"): the check of a caller's image, UV table
// and mask, and the count of textured primitives.  No device involved; ptmi_check_albedo_texture exposes the check.
#pragma once
#include <vector>

#include "primitive.h"

namespace ptmi {

constexpr int kAlbedoCorners = 4;                             // the table has 4 x 2 floats per primitive; a triangle's 4th is ignored
constexpr int kAlbedoMaxSide = 4096;                          // width and height: 1 .. 4096
constexpr float kAlbedoMaxUV = 65536.0f;                      // |u|, |v| of a corner that is read

// the number of textured primitives: textured[i] != 0; textured NULL: all n_prims
int countTextured(int n_prims, const int* textured);

// throws ArgError: n_prims < 1, texels or uv NULL, width or height outside 1 .. 4096, filter not 0 or 1, a texel component that
// is not finite or is negative, and - for a textured primitive only - a UV component of corners 0 .. 2 (what is read whatever the
// primitive's type) that is not finite or whose magnitude exceeds 65536.  UVs of untextured primitives are not read.
void checkAlbedoTexture(int width, int height, const float* texels, int filter, int n_prims, const float* uv, const int* textured);
// the same against a scene's primitives (load order): n_prims equals their count, and a textured quad's 4th corner is checked too
void checkAlbedoTexture(const std::vector<Primitive>& prims, int width, int height, const float* texels, int filter, int n_prims,
                        const float* uv, const int* textured);

}  // namespace ptmi
