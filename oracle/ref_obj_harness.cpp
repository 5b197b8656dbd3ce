// ref_obj_harness.cpp — thin C-ABI driver around the REFERENCE's own OBJ/MTL loader (utils/file_manager.h:39-79, 93-273).
//
// TEST INFRASTRUCTURE ONLY.  Built by oracle/Makefile into oracle/_ref/libptmi_ref_obj.so where /root/reference exists AND
// NVIDIA's own <cuda_runtime.h> is on the machine: file_manager.h includes that header (it uses cudaError_t and
// cudaDeviceReset in an error helper nothing calls).  This image ships the genuine header - with crt/ and
// device_launch_parameters.h - inside its Triton wheel (triton/backends/nvidia/include); oracle/Makefile locates that
// directory at make time and skips this target cleanly where it is absent.  Nothing is written in its place: no stand-in
// header, no edited copy.  The reference sources are included BY PATH from where they lie.
//
// What this pins: loadOBJ + loadMTL, end to end, on any .obj file - primitive type, vertices, stored normal, Kd ("bsdf"),
// Ke ("Le"), the accept/reject decision, and (through the returned count) every skipped-token and default-material rule.
// What it cannot pin: convertQuadsToTriangles lives in application_state.h (GL, GLFW and cuRAND headers) and stays pinned
// through the constructors it calls (ref_harness.cpp) and the survey's known answers.  subdivide_primitives (form_factors.h)
// is compiled and pinned in ref_solver_harness.cpp.
#include <cuda_runtime.h>

#include <cfloat>
#include <cstring>
#include <iostream>
#include <sstream>

#include "utils/file_manager.h"

namespace {
struct Silencer {   // the loader reports progress on std::cout and warnings on std::cerr
    std::streambuf *o, *e; std::ostringstream so, se;
    Silencer() : o(std::cout.rdbuf(so.rdbuf())), e(std::cerr.rdbuf(se.rdbuf())) {}
    ~Silencer() { std::cout.rdbuf(o); std::cerr.rdbuf(e); }
};
struct Loaded { Primitive* prims = nullptr; int n = 0; std::string warnings; };
}

extern "C" {

// returns 1 when loadOBJ accepted the file; *handle then owns the primitives (ref_obj_free)
int ref_obj_load(const char* path, int* n_out, void** handle) {
    Loaded* L = new Loaded;
    bool ok;
    {
        Silencer quiet;
        ok = loadOBJ(path, &L->prims, L->n);
        L->warnings = quiet.se.str();
    }
    *n_out = ok ? L->n : 0;
    *handle = L;
    return ok ? 1 : 0;
}
// number of "Warning" lines the loader printed (skipped face tokens, unknown materials, ...)
int ref_obj_warning_count(void* handle) {
    const std::string& w = ((Loaded*)handle)->warnings;
    int c = 0;
    for (size_t p = w.find("arning"); p != std::string::npos; p = w.find("arning", p + 1)) c++;
    return c;
}
void ref_obj_get(void* handle, int* type, float* verts /* n*4*3 */, float* normal, float* bsdf, float* Le) {
    Loaded* L = (Loaded*)handle;
    for (int i = 0; i < L->n; i++) {
        const Primitive& p = L->prims[i];
        type[i] = (int)p.type;
        float* v = verts + (size_t)i * 12;
        std::memset(v, 0, 12 * sizeof(float));
        if (p.type == PRIM_TRIANGLE) {
            for (int c = 0; c < 3; c++) {
                v[c] = p.tri.v0[c]; v[3 + c] = p.tri.v1[c]; v[6 + c] = p.tri.v2[c];
                normal[3 * i + c] = p.tri.normal[c]; bsdf[3 * i + c] = p.tri.bsdf[c]; Le[3 * i + c] = p.tri.Le[c];
            }
        } else {
            for (int c = 0; c < 3; c++) {
                v[c] = p.quad.v00[c]; v[3 + c] = p.quad.v10[c]; v[6 + c] = p.quad.v11[c]; v[9 + c] = p.quad.v01[c];
                normal[3 * i + c] = p.quad.normal[c]; bsdf[3 * i + c] = p.quad.bsdf[c]; Le[3 * i + c] = p.quad.Le[c];
            }
        }
    }
}
void ref_obj_free(void* handle) {
    Loaded* L = (Loaded*)handle;
    if (!L) return;
    delete[] L->prims;
    delete L;
}

}  // extern "C"
