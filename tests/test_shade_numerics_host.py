"""shade_step tests `length(tp) < 1e-5f` (integrator.h:218) on the squared length: `length_squared(tp) < X0` with
X0 = kSqLenBelow1em5 of csrc/pt_vec.h.  The two are the same predicate for every float, proved here on the host:

  sqrt_rn is the correctly rounded square root, so it is monotone: x <= y implies sqrt_rn(x) <= sqrt_rn(y).  If X0 is the
  smallest float with sqrt_rn(X0) >= 1e-5f, then x >= X0 gives sqrt_rn(x) >= sqrt_rn(X0) >= 1e-5f and x < X0, i.e.
  x <= pred(X0), gives sqrt_rn(x) <= sqrt_rn(pred(X0)) < 1e-5f.  So the boundary pair (pred(X0), X0) decides it.

The boundary pair is checked exactly; monotonicity is checked rather than assumed on every float of the three binades around
X0 and on every 128th positive pattern from 0 to +inf; NaN, +inf, zeros and negative values are compared one by one.
sqrt_rn here is float32(sqrt(float64(x))): a binary64 root rounded to binary32 is the correctly rounded binary32 root
(53 >= 2 * 24 + 2), whatever the host's float32 sqrt does.
"""
import os
import re

import numpy as np

F = np.float32
U = np.uint32
HERE = os.path.dirname(os.path.abspath(__file__))
PT_VEC = os.path.join(os.path.dirname(HERE), "cuda-pathtracer_amd", "csrc", "pt_vec.h")
T = F(1e-5)


def sqrt_rn(x):
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.asarray(x, F).astype(np.float64)).astype(F)


def source_constant():
    with open(PT_VEC) as f:
        m = re.search(r"constexpr float kSqLenBelow1em5 = (0x[0-9a-fA-F.]+p[-+]?\d+)f;", f.read())
    assert m, "kSqLenBelow1em5 not found in csrc/pt_vec.h"
    x = float.fromhex(m.group(1))
    assert float(F(x)) == x, "the constant is not a binary32 value"
    return F(x)


def both(x):
    """(the reference's predicate, the kernel's) for an array of floats"""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        return sqrt_rn(x) < T, x < source_constant()


def test_boundary_pair():
    x0 = source_constant()
    below = np.array([x0], F).view(U) - U(1)
    assert sqrt_rn(x0) >= T and sqrt_rn(below.view(F))[0] < T
    # the derivation: the first float at or above 1e-5f squared, searched among its neighbours
    near = (np.array([T * T], F).view(U)[0] + np.arange(-64, 65)).astype(U).view(F)
    first = near[np.argmax(sqrt_rn(near) >= T)]
    assert first.view(U) == x0.view(U), (float(first).hex(), float(x0).hex())


def test_same_predicate_around_the_boundary_and_over_the_range():
    x0 = source_constant()
    e = int(np.array([x0], F).view(U)[0] >> 23)
    binades = np.arange((e - 1) << 23, (e + 2) << 23, dtype=np.int64).astype(U).view(F)       # every float of three binades
    for x in (binades, np.arange(0, 0x7F800000 + 1, 128, dtype=np.int64).astype(U).view(F)):
        r = sqrt_rn(x)
        assert (np.diff(r) >= 0).all()                         # monotone where checked
        want, got = both(x)
        assert np.array_equal(want, got)
        assert want.any() and not want.all()


def test_special_values():
    x = np.array([np.nan, -np.nan, np.inf, 0.0, -0.0, 1e-45, -1e-45, -1.0, -np.inf, 3.4028235e38], F)
    want, got = both(x)
    assert not want[0] and not got[0] and not want[1] and not got[1]          # a NaN is below nothing, in either form
    assert not want[2] and not got[2]                                         # +inf (a squared length that overflowed)
    assert want[3] and got[3] and want[4] and got[4] and want[5] and got[5]   # zeros and the smallest denormal
    # a squared length is never negative; for the record the forms part there (sqrt of a negative is a NaN, below nothing)
    assert not want[7] and got[7]
