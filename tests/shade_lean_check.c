/* shade_lean_check.c — csrc/shade_lean.h against the long forms, on the host (tests/test_shade_lean_forms_host.py builds and runs it).
 *   shade_lean_check sincos <first_bits> <count>   ptmi_sincos_2pi_fast against ptmi_sincosf over a range of bit patterns
 *       -> "sincos <bad_sin> <bad_cos> <flagged> <flagged_and_different> <first_bad_bits>", bad = different outside the flag
 *   shade_lean_check div <W> <first_bits> <count>  ptmi_div_by_size_lean against a / W
 *       -> "div <bad> <first_bad_bits> <lean>", lean = 0 if this size keeps the IEEE division (then nothing is compared)
 * Build with -ffp-contract=off. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../cuda-pathtracer_amd/csrc/shade_lean.h"

static float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "sincos")) {
        const uint32_t first = (uint32_t)strtoul(argv[2], 0, 0);
        const unsigned long long count = strtoull(argv[3], 0, 0);
        unsigned long long bad_s = 0, bad_c = 0, flagged = 0, flagged_diff = 0, first_bad = ~0ull;
        for (unsigned long long i = 0; i < count; i++) {
            const uint32_t bits = first + (uint32_t)i;
            float s, c, fs, fc;
            ptmi_sincosf(u2f(bits), &s, &c);
            const int flag = ptmi_sincos_2pi_fast(u2f(bits), &fs, &fc);
            const int ds = f2u(s) != f2u(fs), dc = f2u(c) != f2u(fc);
            if (flag) { flagged++; flagged_diff += ds | dc; continue; }
            bad_s += ds; bad_c += dc;
            if ((ds | dc) && first_bad == ~0ull) first_bad = bits;
        }
        printf("sincos %llu %llu %llu %llu %llu\n", bad_s, bad_c, flagged, flagged_diff, first_bad == ~0ull ? 0ull : first_bad);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "div")) {
        const int W = atoi(argv[2]);
        const uint32_t first = (uint32_t)strtoul(argv[3], 0, 0);
        const unsigned long long count = strtoull(argv[4], 0, 0);
        const float y = ptmi_size_reciprocal(W), Wf = (float)W;
        unsigned long long bad = 0, first_bad = ~0ull;
        for (unsigned long long i = 0; y != 0.0f && i < count; i++) {
            const uint32_t bits = first + (uint32_t)i;
            const float a = u2f(bits);
            if (f2u(a / Wf) != f2u(ptmi_div_by_size_lean(a, Wf, y))) { bad++; if (first_bad == ~0ull) first_bad = bits; }
        }
        printf("div %llu %llu %d\n", bad, first_bad == ~0ull ? 0ull : first_bad, y != 0.0f);
        return 0;
    }
    fprintf(stderr, "usage: shade_lean_check sincos <first_bits> <count> | div <W> <first_bits> <count>\n");
    return 2;
}
