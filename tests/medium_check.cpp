// medium_check.cpp — a stand-alone caller of host/medium.cpp (the check of a participating medium's numbers, the medium block and
// the box's corners), to be built with -fsanitize=address,undefined (tests/test_medium_host.py) together with that file alone: it
// needs no HIP header.  The block and the corners are heap blocks of exactly 12 and 24 floats, so a read or write past either is
// reported.  Prints one line per case and "ok <cases>" at the end; any other ending is a failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

#include "../cuda-pathtracer_amd/host/medium.h"

using namespace ptmi;

static int g_cases = 0, g_bad = 0;

static void expect(bool ok, const char* what) {
    g_cases++;
    if (!ok) { g_bad++; std::printf("FAILED %s\n", what); }
    else std::printf("pass %s\n", what);
}

template <typename F>
static bool rejects(F&& f, const char* needle) {
    try { f(); } catch (const MediumError& e) { return std::strstr(e.what(), needle) != nullptr; }
    return false;
}

static Medium fog() {
    Medium m;
    const float lo[3] = {-1.0f, 0.0f, -3.0f}, hi[3] = {2.0f, 5.5f, 4.0f}, al[3] = {0.25f, 0.5f, 1.0f};
    std::memcpy(m.lo, lo, sizeof lo); std::memcpy(m.hi, hi, sizeof hi); std::memcpy(m.albedo, al, sizeof al);
    m.sigma_t = 0.75f; m.g = -0.5f;
    return m;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float big = std::numeric_limits<float>::max(), tiny = std::numeric_limits<float>::denorm_min();
    checkMedium(Medium());
    checkMedium(fog());
    { Medium m = fog(); m.sigma_t = 0.0f; m.g = 0.9f; checkMedium(m); m.g = -0.9f; m.sigma_t = big; checkMedium(m); }
    { Medium m = fog(); m.lo[0] = -big; m.hi[0] = big; m.albedo[0] = 0.0f; m.albedo[1] = -0.0f; checkMedium(m); }
    expect(true, "the ends of every range pass");
    for (int a = 0; a < 3; a++) {
        const char* lo_msg[3] = {"lo.x is not finite", "lo.y is not finite", "lo.z is not finite"};
        const char* hi_msg[3] = {"hi.x is not finite", "hi.y is not finite", "hi.z is not finite"};
        const char* al_msg[3] = {"albedo.r is not finite", "albedo.g is not finite", "albedo.b is not finite"};
        const char* box_msg[3] = {"lo.x must be below hi.x", "lo.y must be below hi.y", "lo.z must be below hi.z"};
        const char* rng_msg[3] = {"albedo.r must lie in [0, 1]", "albedo.g must lie in [0, 1]", "albedo.b must lie in [0, 1]"};
        expect(rejects([&] { Medium m = fog(); m.lo[a] = nan; checkMedium(m); }, lo_msg[a]), "a NaN lo");
        expect(rejects([&] { Medium m = fog(); m.lo[a] = -inf; checkMedium(m); }, lo_msg[a]), "an infinite lo");
        expect(rejects([&] { Medium m = fog(); m.hi[a] = nan; checkMedium(m); }, hi_msg[a]), "a NaN hi");
        expect(rejects([&] { Medium m = fog(); m.hi[a] = inf; checkMedium(m); }, hi_msg[a]), "an infinite hi");
        expect(rejects([&] { Medium m = fog(); m.albedo[a] = nan; checkMedium(m); }, al_msg[a]), "a NaN albedo");
        expect(rejects([&] { Medium m = fog(); m.albedo[a] = inf; checkMedium(m); }, al_msg[a]), "an infinite albedo");
        expect(rejects([&] { Medium m = fog(); m.hi[a] = m.lo[a]; checkMedium(m); }, box_msg[a]), "lo == hi");
        expect(rejects([&] { Medium m = fog(); m.hi[a] = m.lo[a] - 1.0f; checkMedium(m); }, box_msg[a]), "lo > hi");
        expect(rejects([&] { Medium m = fog(); m.albedo[a] = -tiny; checkMedium(m); }, rng_msg[a]), "the smallest negative albedo");
        expect(rejects([&] { Medium m = fog(); m.albedo[a] = std::nextafter(1.0f, 2.0f); checkMedium(m); }, rng_msg[a]), "the first albedo above 1");
    }
    expect(rejects([&] { Medium m = fog(); m.sigma_t = nan; checkMedium(m); }, "sigma_t is not finite"), "a NaN sigma_t");
    expect(rejects([&] { Medium m = fog(); m.sigma_t = inf; checkMedium(m); }, "sigma_t is not finite"), "an infinite sigma_t");
    expect(rejects([&] { Medium m = fog(); m.sigma_t = -tiny; checkMedium(m); }, "sigma_t must not be negative"), "the smallest negative sigma_t");
    expect(rejects([&] { Medium m = fog(); m.g = nan; checkMedium(m); }, "g is not finite"), "a NaN g");
    expect(rejects([&] { Medium m = fog(); m.g = -inf; checkMedium(m); }, "g is not finite"), "an infinite g");
    expect(rejects([&] { Medium m = fog(); m.g = std::nextafter(0.9f, 1.0f); checkMedium(m); }, "|g| must not exceed 0.9"), "the first g above 0.9");
    expect(rejects([&] { Medium m = fog(); m.g = -1.0f; checkMedium(m); }, "|g| must not exceed 0.9"), "g -1");
    expect(rejects([&] { Medium m = fog(); m.lo[1] = nan; m.g = 2.0f; checkMedium(m); }, "lo.y is not finite"), "the finiteness of every field comes first");
    {
        std::unique_ptr<float[]> b(new float[kMediumBlockFloats]);
        for (int i = 0; i < kMediumBlockFloats; i++) b[i] = -7.0f;
        expect(rejects([&] { Medium m = fog(); m.g = 1.0f; mediumBlock(m, b.get()); }, "|g|"), "the block makes the check");
        expect(rejects([&] { mediumBlock(fog(), nullptr); }, "NULL"), "no block");
        bool untouched = true;
        for (int i = 0; i < kMediumBlockFloats; i++) untouched = untouched && b[i] == -7.0f;
        expect(untouched, "a rejected call writes nothing");
        mediumBlock(fog(), b.get());
        const float want[kMediumBlockFloats] = {-1.0f, 0.0f, -3.0f, 0.75f, 2.0f, 5.5f, 4.0f, -0.5f, 0.25f, 0.5f, 1.0f, 0.0f};
        expect(std::memcmp(b.get(), want, sizeof want) == 0, "(lo, sigma_t) (hi, g) (albedo, 0)");
    }
    {
        std::unique_ptr<float[]> c(new float[24]);
        mediumCorners(fog(), c.get());
        bool ok = true;
        int seen = 0;
        for (int i = 0; i < 8; i++) {
            const float* p = c.get() + 3 * i;
            ok = ok && (p[0] == -1.0f || p[0] == 2.0f) && (p[1] == 0.0f || p[1] == 5.5f) && (p[2] == -3.0f || p[2] == 4.0f);
            seen |= 1 << ((p[0] == 2.0f) | (p[1] == 5.5f) << 1 | (p[2] == 4.0f) << 2);
        }
        expect(ok && seen == 0xff, "the eight corners, each once");
    }
    if (g_bad) { std::printf("%d of %d cases failed\n", g_bad, g_cases); return 1; }
    std::printf("ok %d\n", g_cases);
    return 0;
}
