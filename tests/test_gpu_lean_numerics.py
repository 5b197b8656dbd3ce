"""The short forms of sqrt and 1 / x that the shading code and the walks' ray set-up use (csrc/pt_vec.h: sqrt_lean,
rcp_exact_normal; csrc/traversal.h: ray_inv) must give the bits of the IEEE operation wherever they are used.

sqrt_lean: all 2^32 bit patterns against sqrt_rn on the device.  Equality is asserted on the set the callers stay in,
{+0} and [2^-96, +inf]; what the rest of the patterns do is printed for the record (run with -s).  Recorded on an MI355X:
see RECORD below.

ray_inv: one wave votes.  Directions with components 0, -0, 2^-101, 2^-100, denormals, 1, 2^100 and beyond, inf and NaN, alone
in a wave of ordinary directions, in every component and at several lanes: every lane of every wave gets the IEEE quotient.
1 / 0 = inf is the case that tells: the short form alone gives a NaN there.
"""
import numpy as np
import pytest

import ptmi

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32

LO = (127 - 96) << 23            # 2^-96
INF = 0x7F800000

# mismatches of sqrt_lean against sqrt_rn outside the asserted set, as printed by test_lean_sqrt_all_patterns on an MI355X
RECORD = ("(0, 2^-96): 12 343 263 of 260 046 847 patterns differ, the first 0x00000001; NaN, -0 and negative patterns: "
          "8 388 607 of 2 155 872 255 differ, the first 0x80000001 - as many as there are negative denormals (2^23 - 1)")


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def test_lean_sqrt_all_patterns(R):
    bad, first = R.debug_sqrt_check(0, 1)                                   # +0
    assert bad == 0, hex(first)
    bad, first = R.debug_sqrt_check(LO, INF - LO + 1)                       # [2^-96, +inf], both ends included
    assert bad == 0, (bad, hex(first))
    # the rest of the 2^32 patterns, for the record: positive values below 2^-96 (denormals included), then NaNs, -0, negative
    # values and negative NaNs (a NaN on both sides counts as equal)
    below, first_below = R.debug_sqrt_check(1, LO - 1)
    rest, first_rest = R.debug_sqrt_check(INF + 1, (1 << 32) - (INF + 1))
    print(f"sqrt_lean != sqrt_rn: {below} of {LO - 1} patterns in (0, 2^-96), first {first_below:#010x}; "
          f"{rest} of {(1 << 32) - (INF + 1)} NaN / -0 / negative patterns, first {first_rest:#010x}")
    assert 1 + (INF - LO + 1) + (LO - 1) + ((1 << 32) - (INF + 1)) == 1 << 32


def f32(bits_):
    return np.array(bits_, U).view(F)


SPECIAL = np.concatenate([
    f32([0x00000000, 0x80000000]),                                           # 0, -0
    F(2.0) ** np.array([-101, -100, 100, 101], F),                          # the ends of the pinned interval and one binade beyond
    -(F(2.0) ** np.array([-101, -100], F)),
    f32([0x0D800000 - 1, 0x71800000 + 1]),                                  # the floats next to 2^-100 (below) and 2^100 (above)
    f32([0x00000001, 0x007FFFFF, 0x80000001, 0x00400000, 0x00800000]),       # denormals, and the smallest normal
    np.array([1.0, -1.0, np.inf, -np.inf, np.nan], F),
])


def ordinary(rng, n):
    """n directions whose components cover the pinned interval [2^-100, 2^100): random sign, exponent and mantissa"""
    e = rng.integers(127 - 100, 127 + 100, (n, 3)).astype(U)
    b = (rng.integers(0, 2, (n, 3)).astype(U) << U(31)) | (e << U(23)) | rng.integers(0, 1 << 23, (n, 3)).astype(U)
    return b.view(F)


def test_ray_inv_vote(R):
    rng = np.random.default_rng(5)
    waves, live = [], []
    waves.append(ordinary(rng, 64)); live.append(np.ones(64, np.int32))     # nothing to vote about: the short form
    unit = rng.normal(0, 1, (64, 3)); unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    waves.append(unit.astype(F)); live.append(np.ones(64, np.int32))        # ray directions as the kernels see them
    for s in SPECIAL:
        for c in range(3):
            for lane in (0, 37, 63):
                w = ordinary(rng, 64); w[lane, c] = s
                waves.append(w); live.append(np.ones(64, np.int32))
        w = ordinary(rng, 64); w[11] = s                                     # all three components at once
        waves.append(w); live.append(np.ones(64, np.int32))
        w = ordinary(rng, 64); w[5, 1] = s                                   # in a lane without a ray: no say in the vote
        l = np.ones(64, np.int32); l[5] = 0
        waves.append(w); live.append(l)
    w = ordinary(rng, 23); w[22, 2] = F(0.0)                                 # a partial last wave
    waves.append(w); live.append(np.ones(23, np.int32))
    d = np.concatenate(waves); live = np.concatenate(live)
    got = R.debug_ray_inv(d, live)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        want = (F(1.0) / d).astype(F)
    alive = live != 0
    same = (got.view(U) == want.view(U)) | (np.isnan(got) & np.isnan(want))
    bad = np.argwhere(~same & alive[:, None])
    assert len(bad) == 0, [(int(i), int(c), float(d[i, c]), got[i, c].view(U), want[i, c].view(U)) for i, c in bad[:5]]
    zeros = alive[:, None] & (d == 0)
    assert zeros.any() and np.isinf(got[zeros]).all()                        # 1 / 0 and 1 / -0: inf, never the short form's NaN
