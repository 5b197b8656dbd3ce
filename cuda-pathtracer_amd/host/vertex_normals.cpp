// vertex_normals.cpp — the check and the flat / smooth classification of a vertex-normal table, as include/ptmi.h ("vertex
// normals") states them.
#include "vertex_normals.h"

#include <cmath>
#include <string>

#include "application_state.h"   // ArgError

namespace ptmi {

static void checkCorner(const float* normals, int i, int c) {
    const float* v = normals + ((size_t)i * kVertexNormalCorners + (size_t)c) * 3;
    if (!(std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2])))
        throw ArgError("vertex normals: corner " + std::to_string(c) + " of primitive " + std::to_string(i) + " must be finite");
}

void checkVertexNormals(int n_prims, const float* normals) {
    if (n_prims < 1) throw ArgError("vertex normals: n_prims must be >= 1");
    if (!normals) throw ArgError("vertex normals: normals is NULL");
    for (int i = 0; i < n_prims; i++)
        for (int c = 0; c < 3; c++) checkCorner(normals, i, c);
}

void checkVertexNormals(const std::vector<Primitive>& prims, int n_prims, const float* normals) {
    if (n_prims != (int)prims.size()) throw ArgError("vertex normals: n_prims does not match the loaded scene");
    checkVertexNormals(n_prims, normals);
    for (int i = 0; i < n_prims; i++)
        if (prims[i].type == PRIM_QUAD) checkCorner(normals, i, 3);
}

bool vertexNormalsSmooth(PrimitiveType type, const f3& stored, const float* corners) {
    const int read = type == PRIM_QUAD ? 4 : 3;
    for (int c = 0; c < read; c++)
        if (!(corners[3 * c] == stored.x && corners[3 * c + 1] == stored.y && corners[3 * c + 2] == stored.z)) return true;
    return false;
}

int classifyVertexNormals(const std::vector<Primitive>& prims, const float* normals, std::vector<unsigned char>& smooth) {
    smooth.assign(prims.size(), 0);
    int n_smooth = 0;
    for (size_t i = 0; i < prims.size(); i++) {
        smooth[i] = vertexNormalsSmooth(prims[i].type, prims[i].normal, normals + i * kVertexNormalCorners * 3) ? 1 : 0;
        n_smooth += smooth[i];
    }
    return n_smooth;
}

}  // namespace ptmi
