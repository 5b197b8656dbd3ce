// pt_vec.h — 3-float vector with the reference's rounding semantics, host + device.
//
// The reference's Vector<T,N> (include/core/vector.h) fixes the evaluation order
// of every expression on the path; the helpers below spell that order out so the
// same bits come out of the host code and the gfx950 kernels.  Everything here is
// compiled with -ffp-contract=off: a*b+c must stay two roundings.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define PT_HD __host__ __device__ __forceinline__

namespace ptmi {

struct f3 { float x, y, z; };

PT_HD f3 mk3(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
PT_HD f3 operator+(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }      // vector.h:148-153
PT_HD f3 operator-(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }      // vector.h:155-160
PT_HD f3 operator*(f3 a, f3 b) { return mk3(a.x * b.x, a.y * b.y, a.z * b.z); }      // vector.h:162-167
PT_HD f3 operator*(float t, f3 v) { return mk3(t * v.x, t * v.y, t * v.z); }         // vector.h:177-187
PT_HD f3 operator-(f3 a) { return mk3(-a.x, -a.y, -a.z); }                           // vector.h:56-60

// IEEE-correct 1/t.  The reference writes `T k = 1.0 / t` (vector.h:90-94,189-195):
// a binary64 quotient rounded to binary32, which equals the correctly rounded
// binary32 quotient (53 >= 2*24+2, double rounding is innocuous for division).
// On the device both rely on hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt (the build passes it
// explicitly): `/` and __builtin_sqrtf then lower to the IEEE-exact v_div_scale/fmas/fixup and scaled-sqrt
// sequences.  NOT __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS that is the 1-ulp v_sqrt_f32.
PT_HD float rcp_rn(float t) { return 1.0f / t; }

// Correctly rounded 1/a for the Moller-Trumbore determinant, in 1 v_rcp_f32 + 4 v_fma_f32 instead of the compiler's
// 10-instruction IEEE division (v_div_scale x2, v_rcp, 4 fma, mul, v_div_fmas, v_div_fixup; the scale/fmas/fixup
// ops are half-rate).  Two Newton steps on the <= 1 ulp hardware seed; without the scaling steps this is exact only
// while neither a nor 1/a leaves the normal range.  tests/test_gpu_parity.py::test_fast_reciprocal_is_exact checks
// ALL 2^32 bit patterns against the IEEE quotient on the device and pins the interval [2^-100, 2^100] used here;
// outside it the caller's result is either rejected anyway (|a| < 1e-8) or unreachable for scenes that pass the
// host's extent check.  Device only: the CPU oracle keeps the true division.
__device__ __forceinline__ float rcp_exact_normal(float a) {
    float r = __builtin_amdgcn_rcpf(a);
    float e = __builtin_fmaf(-a, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
    e = __builtin_fmaf(-a, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
    return r;
}
PT_HD float sqrt_rn(float x) { return __builtin_sqrtf(x); }
// sqrt_rn for an operand that is 0 or >= 2^-96 (+inf included): the compiler's own sequence - v_sqrt_f32 (<= 1 ulp), then the
// two neighbours of the seed tried with one residual fma each - without the scale-by-2^32 steps in front of and behind it, which
// act only below 2^-96, and without the class select for 0 and inf (a NaN residual picks neither neighbour, so both fall through
// unchanged).  9 instructions instead of 14.  tests/test_gpu_lean_numerics.py checks ALL 2^32 bit patterns against sqrt_rn on the
// device and pins the set {0} + [2^-96, +inf] used here.  Device only: the CPU oracle keeps the library's sqrtf.
__device__ __forceinline__ float sqrt_lean(float x) {
    float s = __builtin_amdgcn_sqrtf(x);
    const float down = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
    const float r_down = __builtin_fmaf(-down, s, x), r_up = __builtin_fmaf(-up, s, x);
    s = r_down <= 0.0f ? down : s;
    s = r_up > 0.0f ? up : s;
    return s;
}
// sqrt_rn(x) < 1e-5f without the square root.  sqrt_rn is correctly rounded, hence monotone, so the test is x < X0 with X0 the
// smallest float whose sqrt_rn reaches 1e-5f: sqrt_rn(0x1.b7cdf8p-34f) = 0x1.4f8b56p-17f < 1e-5f = 0x1.4f8b58p-17f =
// sqrt_rn(0x1.b7cdfap-34f).  Both forms are false for a NaN and for +inf.  tests/test_shade_numerics_host.py proves the boundary.
constexpr float kSqLenBelow1em5 = 0x1.b7cdfap-34f;
PT_HD bool length_below_1em5(float length_squared) { return length_squared < kSqLenBelow1em5; }
PT_HD f3 div_scalar(f3 v, float t) { float k = rcp_rn(t); return mk3(v.x * k, v.y * k, v.z * k); }
PT_HD float dot(f3 a, f3 b) { float s = a.x * b.x; s += a.y * b.y; s += a.z * b.z; return s; }   // vector.h:198-203 (0 + x is exact)
PT_HD float length_squared(f3 a) { return dot(a, a); }                               // vector.h:97-101
PT_HD float length(f3 a) { return sqrt_rn(length_squared(a)); }                      // vector.h:103-105
PT_HD f3 unit_vector(f3 v) { return div_scalar(v, length(v)); }                      // vector.h:205-208
// unit_vector for a vector whose squared length provably lies in [2^-96, 2^100]: its root is then inside [2^-48, 2^50], where
// rcp_exact_normal is the IEEE quotient.  The same bits as unit_vector, in 14 instructions less.
__device__ __forceinline__ f3 unit_vector_lean(f3 v) {
    const float k = rcp_exact_normal(sqrt_lean(length_squared(v)));
    return mk3(v.x * k, v.y * k, v.z * k);
}
// unit_vector for a vector nothing is known about, per wave: ONE vote decides.  If the squared length of every active lane lies
// in [2^-96, 2^100] the wave takes unit_vector_lean's operations, otherwise - a zero, a denormal, a huge, an infinite or a NaN
// squared length in any active lane - the whole wave takes unit_vector's.  Either way every lane gets unit_vector's bits.  Lanes
// that are not active at the call have no say.  tests/test_gpu_shade_lean_forms.py::test_unit_vector_vote pins it.
__device__ __forceinline__ f3 unit_vector_voted(f3 v) {
    const float l2 = length_squared(v);
    const bool in_range = (l2 >= 0x1p-96f) & (l2 <= 0x1p+100f);             // false for a NaN
    float k;
    if (__any(!in_range)) k = rcp_rn(sqrt_rn(l2));
    else k = rcp_exact_normal(sqrt_lean(l2));
    return mk3(v.x * k, v.y * k, v.z * k);
}
PT_HD f3 cross(f3 a, f3 b) {                                                         // vector.h:211-218
    return mk3(a.y * b.z - a.z * b.y, -(a.x * b.z - a.z * b.x), a.x * b.y - a.y * b.x);
}

}  // namespace ptmi
