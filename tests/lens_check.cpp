// lens_check.cpp — a stand-alone caller of host/lens.cpp (the check of a thin lens's two numbers and the lens block), to be built
// with -fsanitize=address,undefined (tests/test_lens_host.py) together with that file alone: it needs no HIP header.  The frame
// and the block are heap blocks of exactly 12 and 24 floats, so a read or write past either is reported.  Prints one line per case
// and "ok <cases>" at the end; any other ending is a failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

#include "../cuda-pathtracer_amd/host/lens.h"

using namespace ptmi;

static int g_cases = 0, g_bad = 0;

static void expect(bool ok, const char* what) {
    g_cases++;
    if (!ok) { g_bad++; std::printf("FAILED %s\n", what); }
    else std::printf("pass %s\n", what);
}

template <typename F>
static bool rejects(F&& f, const char* needle) {
    try { f(); } catch (const LensError& e) { return std::strstr(e.what(), needle) != nullptr; }
    return false;
}

static std::unique_ptr<float[]> frame(float hx, float vy, float oz) {
    // a camera at (0, 0, oz) looking down -z: llc = org + (-hx / 2, -vy / 2, -1)
    std::unique_ptr<float[]> f(new float[12]);
    const float v[12] = {0.0f, 0.0f, oz, -hx / 2, -vy / 2, oz - 1.0f, hx, 0.0f, 0.0f, 0.0f, vy, 0.0f};
    std::memcpy(f.get(), v, sizeof v);
    return f;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float big = std::numeric_limits<float>::max(), tiny = std::numeric_limits<float>::denorm_min();
    // the two numbers
    checkLens(0.0f, 1.0f); checkLens(0.0f, tiny); checkLens(big, big); checkLens(-0.0f, 1.0f);
    expect(true, "the ends of both ranges pass");
    expect(rejects([&] { checkLens(nan, 1.0f); }, "radius is a NaN"), "a NaN radius");
    expect(rejects([&] { checkLens(1.0f, nan); }, "focus_distance is a NaN"), "a NaN focus distance");
    expect(rejects([&] { checkLens(nan, nan); }, "radius is a NaN"), "two NaNs name the radius");
    expect(rejects([&] { checkLens(inf, 1.0f); }, "radius must be finite"), "an infinite radius");
    expect(rejects([&] { checkLens(-inf, 1.0f); }, "radius must be finite"), "a negative infinite radius");
    expect(rejects([&] { checkLens(1.0f, inf); }, "focus_distance must be finite"), "an infinite focus distance");
    expect(rejects([&] { checkLens(1.0f, -inf); }, "focus_distance must be finite"), "a negative infinite focus distance");
    expect(rejects([&] { checkLens(-tiny, 1.0f); }, "radius must not be negative"), "the smallest negative radius");
    expect(rejects([&] { checkLens(1.0f, 0.0f); }, "focus_distance must be positive"), "focus distance 0");
    expect(rejects([&] { checkLens(1.0f, -0.0f); }, "focus_distance must be positive"), "focus distance -0");
    expect(rejects([&] { checkLens(1.0f, -3.0f); }, "focus_distance must be positive"), "a negative focus distance");
    // the block: every value at its place, exact where the arithmetic is
    for (int w : {1, 33, 1 << 23, (1 << 23) + 1}) {
        for (int h : {1, 19, 4096}) {
            auto f = frame(2.0f, 0.5f, 3.0f);
            std::unique_ptr<float[]> b(new float[kLensBlockFloats]);
            lensBlock(f.get(), w, h, 0.25f, 8.0f, b.get());
            const bool sizes = b[3] == (float)w && b[11] == (float)h && (w > (1 << 23) ? b[7] == 0.0f && b[15] == 0.0f : b[7] == 1.0f / (float)w && b[15] == 1.0f / (float)h);
            expect(sizes, "W, 1 / W, H, 1 / H");
            const bool vecs = b[0] == -8.0f && b[1] == -2.0f && b[2] == -5.0f && b[4] == 16.0f && b[5] == 0.0f && b[6] == 0.0f && b[8] == 0.0f && b[9] == 4.0f &&
                              b[10] == 0.0f && b[12] == 0.0f && b[13] == 0.0f && b[14] == 3.0f && b[16] == 0.25f && b[17] == 0.0f && b[18] == 0.0f &&
                              b[20] == 0.0f && b[21] == 0.25f && b[22] == 0.0f && b[19] == 0.0f && b[23] == 0.0f;
            expect(vecs, "llc_f, hor_f, ver_f, org, a, b");
        }
    }
    {
        auto f = frame(2.0f, 0.5f, 3.0f);
        std::unique_ptr<float[]> b(new float[kLensBlockFloats]);
        for (int i = 0; i < kLensBlockFloats; i++) b[i] = -7.0f;
        auto untouched = [&] { for (int i = 0; i < kLensBlockFloats; i++) if (b[i] != -7.0f && !std::isinf(b[i]) && !std::isnan(b[i])) return false; return true; };
        expect(rejects([&] { lensBlock(f.get(), 0, 4, 0.25f, 8.0f, b.get()); }, "width and height"), "width 0");
        expect(rejects([&] { lensBlock(f.get(), 4, -1, 0.25f, 8.0f, b.get()); }, "width and height"), "a negative height");
        expect(rejects([&] { lensBlock(f.get(), 4, 4, 0.0f, 8.0f, b.get()); }, "pinhole"), "radius 0 has no block");
        expect(rejects([&] { lensBlock(f.get(), 4, 4, 0.25f, 0.0f, b.get()); }, "focus_distance must be positive"), "the block makes the check");
        expect(rejects([&] { lensBlock(nullptr, 4, 4, 0.25f, 8.0f, b.get()); }, "NULL"), "no frame");
        expect(rejects([&] { lensBlock(f.get(), 4, 4, 0.25f, 8.0f, nullptr); }, "NULL"), "no block");
        expect(untouched(), "a call rejected before the arithmetic writes nothing");
        expect(rejects([&] { lensBlock(f.get(), 4, 4, 0.25f, big, b.get()); }, "not finite (record 1, component 0)"), "f * hor overflows before f * (llc - org)");
        auto wide = frame(4.0f, 0.5f, 0.0f);
        wide[3] = 0.0f; wide[4] = 0.0f; wide[5] = -0.25f;           // llc - org stays small: hor_f is the first to overflow
        expect(rejects([&] { lensBlock(wide.get(), 4, 4, 0.25f, big / 2.0f, b.get()); }, "not finite (record 1, component 0)"), "f * hor overflows alone");
        auto flat = frame(0.0f, 0.5f, 3.0f);
        expect(rejects([&] { lensBlock(flat.get(), 4, 4, 0.25f, 8.0f, b.get()); }, "not finite (record 4"), "a frame without width: R / 0");
        auto bad = frame(2.0f, nan, 3.0f);
        expect(rejects([&] { lensBlock(bad.get(), 4, 4, 0.25f, 8.0f, b.get()); }, "not finite"), "a NaN in the frame");
        auto small = frame(1e-30f, 1e-30f, 3.0f);                    // length^2 underflows to 0: R / 0
        expect(rejects([&] { lensBlock(small.get(), 4, 4, 0.25f, 8.0f, b.get()); }, "not finite (record 4"), "a frame whose squared length underflows");
        lensBlock(f.get(), 4, 4, big / 4.0f, tiny, b.get());
        expect(std::isfinite(b[16]) && b[4] == 2.0f * tiny, "the largest radius and the smallest focus distance that are finite");
    }
    if (g_bad) { std::printf("%d of %d cases failed\n", g_bad, g_cases); return 1; }
    std::printf("ok %d\n", g_cases);
    return 0;
}
