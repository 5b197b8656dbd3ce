/* shade_lean.h — the arithmetic of two short forms of the shade step, free of HIP so that a plain C compiler can check it
 * (tests/test_shade_lean_forms_host.py) before the kernels use it (shading.h: sincos_2pi_lean, div_by_size).  Compile with
 * -ffp-contract=off like everything else: the fused operations below are written out, nothing else may fuse.
 *
 * Each form gives the bits of the form it stands for on the inputs stated with it; outside them the caller keeps the long form.
 */
#ifndef PTMI_SHADE_LEAN_H
#define PTMI_SHADE_LEAN_H

#include "../../include/ptmi_math.h"

/* (float)(2 pi): the largest phi = (float)(2 pi v) of a uniform v <= 1.  The arguments of ptmi_sincos_2pi_fast are the bit
 * patterns 0 .. PTMI_TWO_PI_F_BITS, 1 086 918 620 floats. */
#define PTMI_TWO_PI_F_BITS 0x40C90FDBu

/* A binary64 value rounds to binary32 by dropping the low 29 bits of its significand; the boundary is 0x10000000.  Two binary64
 * results a few ulp apart can round to different floats only if one of them lies next to that boundary: within +-256 here.
 * (For results below 2^-126 the boundary is elsewhere; sin and cos of a float in [0, 2 pi] come no closer to 0 than 4e-8, apart
 * from sin x = x for tiny x, which both forms return exactly.) */
PTMI_HD int ptmi_round_ambiguous(double v) {
    const uint32_t low = (uint32_t)ptmi_d2u(v) & 0x1FFFFFFFu;
    return low - (0x10000000u - 256u) <= 512u;
}

/* A coefficient of the polynomials below.  On the device it is pinned to a scalar register pair, which v_fma_f64 reads as its
 * addend; left to itself the compiler forms v_fmac_f64, whose addend is its destination, and keeps a copy of every coefficient in
 * a vector register pair for the length of the kernel: 20 VGPRs, and a wave per SIMD or more in every bounce kernel. */
#if defined(__HIP_DEVICE_COMPILE__)
#define PTMI_LEAN_COEF(name, value) double name = value; __asm__("" : "+s"(name))
#else
#define PTMI_LEAN_COEF(name, value) const double name = value
#endif

/* ptmi_sincosf for x in [0, (float)(2 pi)] in half the binary64 operations: ptmi_sincos_d's reduction constants and fdlibm
 * coefficients, every multiply-add one explicit fma, the quadrant by selects.  Both forms are within about 2^-50 of the true
 * value, so their float roundings differ only where ptmi_round_ambiguous says so: the return value is that flag for either
 * result, and the caller takes ptmi_sincosf then.  Over all 1 086 918 620 arguments: no difference outside the flag, 255 flagged. */
PTMI_HD int ptmi_sincos_2pi_fast(float x, float* s_out, float* c_out) {
    PTMI_LEAN_COEF(INV_PIO2, 6.36619772367581382433e-01);
    PTMI_LEAN_COEF(PIO2_1, 1.57079632673412561417e+00);
    PTMI_LEAN_COEF(PIO2_1T, 6.07710050650619224932e-11);
    PTMI_LEAN_COEF(S1, -1.66666666666666324348e-01); PTMI_LEAN_COEF(S2, 8.33333333332248946124e-03);
    PTMI_LEAN_COEF(S3, -1.98412698298579493134e-04); PTMI_LEAN_COEF(S4, 2.75573137070700676789e-06);
    PTMI_LEAN_COEF(S5, -2.50507602534068634195e-08); PTMI_LEAN_COEF(S6, 1.58969099521155010221e-10);
    PTMI_LEAN_COEF(C1, 4.16666666666666019037e-02); PTMI_LEAN_COEF(C2, -1.38888888888741095749e-03);
    PTMI_LEAN_COEF(C3, 2.48015872894767294178e-05); PTMI_LEAN_COEF(C4, -2.75573143513906633035e-07);
    PTMI_LEAN_COEF(C5, 2.08757232129817482790e-09); PTMI_LEAN_COEF(C6, -1.13596475577881948265e-11);
    const double xd = (double)x;
    const int k = (int)__builtin_fma(xd, INV_PIO2, 0.5);          /* x >= 0: truncation is floor */
    const double nk = -(double)k;
    double r = __builtin_fma(nk, PIO2_1, xd);
    r = __builtin_fma(nk, PIO2_1T, r);
    const double z = r * r;
    double ps = S6;
    ps = __builtin_fma(ps, z, S5); ps = __builtin_fma(ps, z, S4); ps = __builtin_fma(ps, z, S3);
    ps = __builtin_fma(ps, z, S2); ps = __builtin_fma(ps, z, S1);
    const double sr = __builtin_fma(r * z, ps, r);
    double pc = C6;
    pc = __builtin_fma(pc, z, C5); pc = __builtin_fma(pc, z, C4); pc = __builtin_fma(pc, z, C3);
    pc = __builtin_fma(pc, z, C2); pc = __builtin_fma(pc, z, C1);
    const double cr = __builtin_fma(z * z, pc, __builtin_fma(z, -0.5, 1.0));
    const double sm = (k & 1) ? cr : sr, cm = (k & 1) ? sr : cr;
    const double s = (k & 2) ? -sm : sm, c = ((k + 1) & 2) ? -cm : cm;
    *s_out = (float)s; *c_out = (float)c;
    return ptmi_round_ambiguous(s) | ptmi_round_ambiguous(c);
}

/* a / W for an image size W in three operations, with y = 1 / W the IEEE reciprocal taken once (ptmi_size_reciprocal).
 * Markstein's correction: q0 = a y is within an ulp of the quotient, r = a - q0 W is exact in one fma, and q0 + r y rounds to
 * the correctly rounded quotient when y is the correctly rounded reciprocal, nothing over- or underflows and W's significand is
 * not all ones (Markstein, "Computation of elementary functions on the IBM RISC System/6000 processor", 1990; for a divisor known
 * in advance: Brisebarre, Muller and Raina, "Accelerating correctly rounded floating-point division when the divisor is known in
 * advance", IEEE Trans. Computers 53(8), 2004).  Here a = (float)x + r1 lies in [2^-33, W] and W is an integer in [1, 2^23]: at
 * most 23 significant bits, so never all 24 ones, and a / W >= 2^-56 with a residual far above the denormals.  The tests add the
 * exhaustive comparison over a for sixteen sizes; the claim for the other sizes rests on the theorem. */
PTMI_HD float ptmi_div_by_size_lean(float a, float W, float y) {
    const float q0 = a * y;
    const float r = __builtin_fmaf(-q0, W, a);
    return __builtin_fmaf(r, y, q0);
}
/* y of ptmi_div_by_size_lean for image size W, or 0: this size keeps the IEEE division */
PTMI_HD float ptmi_size_reciprocal(int W) { return (W >= 1 && W <= (1 << 23)) ? 1.0f / (float)W : 0.0f; }

#endif /* PTMI_SHADE_LEAN_H */
