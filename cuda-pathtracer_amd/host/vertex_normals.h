// vertex_normals.h — host half of the vertex normals (include/ptmi.h: "vertex normals"): the check of a caller's table and the
// flat / smooth classification.  No device involved; ptmi_check_vertex_normals and ptmi_host_classify_vertex_normals expose them.
#pragma once
#include <vector>

#include "primitive.h"

namespace ptmi {

constexpr int kVertexNormalCorners = 4;                       // the table has 4 x 3 floats per primitive; a triangle's 4th is ignored

// throws ArgError: n_prims < 1, normals NULL, a NaN or infinite component in corners 0 .. 2 of any primitive (what is read
// whatever the primitive's type)
void checkVertexNormals(int n_prims, const float* normals);
// the same against a scene's primitives (load order): n_prims equals their count, and a quad's 4th corner is finite too
void checkVertexNormals(const std::vector<Primitive>& prims, int n_prims, const float* normals);

// flat: every corner normal that is read compares equal (==, component for component; -0.0 == 0.0) to the stored normal
bool vertexNormalsSmooth(PrimitiveType type, const f3& stored, const float* corners /* 4 x 3 */);
// smooth[i] = 1 where primitive i is smooth; returns their number
int classifyVertexNormals(const std::vector<Primitive>& prims, const float* normals, std::vector<unsigned char>& smooth);

}  // namespace ptmi
