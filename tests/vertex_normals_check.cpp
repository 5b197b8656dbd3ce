// vertex_normals_check.cpp — a stand-alone caller of host/vertex_normals.cpp (the check and the flat / smooth classification of a
// caller's corner-normal table), to be built with -fsanitize=address,undefined (tests/test_vertex_normals_sanitized.py): every
// table is a heap block of exactly n_prims * 4 * 3 floats, so a read past the caller's table is reported.  Prints one line per
// case and "ok <cases>" at the end; any other ending is a failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../cuda-pathtracer_amd/host/application_state.h"
#include "../cuda-pathtracer_amd/host/vertex_normals.h"

using namespace ptmi;

static int g_cases = 0, g_bad = 0;

static void expect(bool ok, const char* what) {
    g_cases++;
    if (!ok) { g_bad++; std::printf("FAILED %s\n", what); }
    else std::printf("pass %s\n", what);
}

// an exact-size heap copy of a table whose every corner is `n`
static std::unique_ptr<float[]> table(int n_prims, f3 n) {
    std::unique_ptr<float[]> t(new float[(size_t)n_prims * 12]);
    for (int i = 0; i < n_prims * 4; i++) { t[3 * i] = n.x; t[3 * i + 1] = n.y; t[3 * i + 2] = n.z; }
    return t;
}

template <typename F>
static bool rejects(F&& f, const char* needle) {
    try { f(); } catch (const ArgError& e) { return std::strstr(e.what(), needle) != nullptr; }
    return false;
}

int main() {
    const f3 up = mk3(0.0f, 0.0f, 1.0f);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (int n : {1, 2, 7, 64, 1000}) {
        std::vector<Primitive> prims((size_t)n);
        for (int i = 0; i < n; i++) { prims[i].type = i % 3 == 1 ? PRIM_QUAD : PRIM_TRIANGLE; prims[i].normal = up; }
        auto t = table(n, up);
        checkVertexNormals(n, t.get());
        checkVertexNormals(prims, n, t.get());
        std::vector<unsigned char> smooth;
        expect(classifyVertexNormals(prims, t.get(), smooth) == 0 && (int)smooth.size() == n, "an all-flat table");
        // the LAST primitive's last read corner: the far end of the caller's block
        const int last = n - 1, corner = prims[last].type == PRIM_QUAD ? 3 : 2;
        t[(size_t)last * 12 + corner * 3 + 2] = std::nextafter(1.0f, 2.0f);
        expect(classifyVertexNormals(prims, t.get(), smooth) == 1 && smooth[last] == 1, "one ulp in the last corner that is read");
        t[(size_t)last * 12 + corner * 3 + 2] = nan;
        expect(rejects([&] { checkVertexNormals(prims, n, t.get()); }, "must be finite"), "a NaN in the last corner that is read");
        t[(size_t)last * 12 + corner * 3 + 2] = 1.0f;
        if (prims[last].type == PRIM_TRIANGLE) {             // a triangle's 4th corner is neither checked nor compared
            t[(size_t)last * 12 + 9] = inf;
            checkVertexNormals(prims, n, t.get());
            expect(classifyVertexNormals(prims, t.get(), smooth) == 0, "a triangle's 4th corner is ignored");
        }
        expect(rejects([&] { checkVertexNormals(prims, n + 1, t.get()); }, "n_prims"), "a count that is not the scene's");
    }
    {
        auto t = table(3, mk3(-0.0f, 0.0f, 1.0f));
        std::vector<Primitive> prims(3);
        for (Primitive& p : prims) { p.type = PRIM_QUAD; p.normal = up; }
        std::vector<unsigned char> smooth;
        expect(classifyVertexNormals(prims, t.get(), smooth) == 0, "-0.0 == 0.0");
        prims[1].normal = mk3(nan, 0.0f, 1.0f);
        expect(classifyVertexNormals(prims, t.get(), smooth) == 1 && smooth[1] == 1, "a NaN stored normal equals nothing");
        auto z = table(3, mk3(0.0f, 0.0f, 0.0f));
        checkVertexNormals(prims, 3, z.get());
        expect(classifyVertexNormals(prims, z.get(), smooth) == 3, "zero-length corner normals are allowed, and smooth");
        for (float bad : {nan, inf, -inf})
            for (int c = 0; c < 3; c++) {
                auto b = table(3, up);
                b[(size_t)2 * 12 + c * 3 + c] = bad;
                expect(rejects([&] { checkVertexNormals(3, b.get()); }, ("corner " + std::to_string(c) + " of primitive 2").c_str()), "a non-finite component");
            }
        auto b = table(3, up);
        b[9] = nan;
        checkVertexNormals(3, b.get());                      // without types the 4th corner is not read
        expect(rejects([&] { checkVertexNormals(prims, 3, b.get()); }, "corner 3 of primitive 0"), "a quad's 4th corner is read");
    }
    expect(rejects([] { checkVertexNormals(0, nullptr); }, "n_prims"), "no primitive");
    expect(rejects([] { checkVertexNormals(-5, nullptr); }, "n_prims"), "a negative count");
    expect(rejects([] { checkVertexNormals(4, nullptr); }, "NULL"), "no table");
    if (g_bad) { std::printf("%d of %d cases failed\n", g_bad, g_cases); return 1; }
    std::printf("ok %d\n", g_cases);
    return 0;
}
