"""The short forms of the shade step's direction tail (csrc/shade_lean.h, csrc/shading.h, csrc/pt_vec.h) must give the bits of
the forms they stand for wherever the sweep kernel uses them, on the device:

  sincos_2pi_lean    the cosine sample's sincos - explicit binary64 fmas behind one vote per wave - against ptmi_sincosf: all
                     1 086 918 620 arguments in [0, (float)(2 pi)], and the vote with every kind of argument that must turn it
  div_by_size        the pixel jitter's a / W in three operations against the IEEE division: every a in [2^-33, W] for sixteen
                     image sizes W, and a size above 2^23, which keeps the division
  unit_vector_voted  the Ray constructor's normalisation behind one vote per wave against unit_vector
  rcp_exact_normal   the roulette's 1 / rr_prob against the IEEE reciprocal: every float in [2^-33, 0.95]

Recorded on an MI355X (run with -s): sincos_2pi_lean: 255 of 1 086 918 620 arguments raise the ambiguity flag (2.3e-7), none of
them differs.
"""
import numpy as np
import pytest

import ptmi

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32

TWO_PI_BITS = 0x40C90FDB         # (float)(2 pi)
N_ARGS = TWO_PI_BITS + 1         # 1 086 918 620
LO33 = (127 - 33) << 23          # 2^-33, the smallest curand uniform
SIZES = [1, 3, 7, 683, 1024, 1080, 1365, 1920, 2047, 2048, 3840, 4095, 4096, 8191, 16383, 16384]


def bits(x):
    return int(np.array(x, F).view(U))


def f32(b):
    return np.array(b, U).view(F)


def same_bits(a, b):
    return (a.view(U) == b.view(U)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def exhaustive(R):
    """one pass over all arguments, shared: (bad sin, bad cos, first bad, flagged lanes, some flagged patterns)"""
    return R.debug_sincos_lean_check(0, N_ARGS)


def test_sincos_all_arguments(exhaustive):
    bad_sin, bad_cos, first, flagged, kept = exhaustive
    print(f"sincos_2pi_lean: {flagged} of {N_ARGS} arguments raise the ambiguity flag ({flagged / N_ARGS:.2e}); "
          f"some of them: {[hex(int(b)) for b in kept]}")
    assert bad_sin == 0, (bad_sin, hex(first))
    assert bad_cos == 0, (bad_cos, hex(first))
    assert flagged <= 1e-5 * N_ARGS, flagged          # a wave of 64 then goes the long way once in about 1 500 calls at the most


def ordinary_angles(rng, n):
    return (rng.random(n) * 2.0 * np.pi).astype(F).clip(0, f32(TWO_PI_BITS))


def test_sincos_vote(R, exhaustive):
    kept = exhaustive[4]
    assert len(kept) >= 4, kept                        # the exhaustive pass found flagged arguments to stand in a wave
    special = np.concatenate([f32([0x80000000]), np.array([-1.5], F), f32([TWO_PI_BITS + 1]), np.array([1e5, np.inf, np.nan], F),
                              f32(kept[:4])])
    rng = np.random.default_rng(11)
    waves, live = [ordinary_angles(rng, 64)], [np.ones(64, np.int32)]        # nothing to vote about: the short form
    for s in special:
        for lane in (0, 37, 63):
            w = ordinary_angles(rng, 64); w[lane] = s
            waves.append(w); live.append(np.ones(64, np.int32))
        w = ordinary_angles(rng, 64); w[5] = s                                # in a lane that is not active: no say in the vote
        l = np.ones(64, np.int32); l[5] = 0
        waves.append(w); live.append(l)
    w = ordinary_angles(rng, 23); w[22] = f32(0x80000000)                     # a partial last wave
    waves.append(w); live.append(np.ones(23, np.int32))
    x = np.concatenate(waves); live = np.concatenate(live)
    out = R.debug_sincos_lean(x, live)
    alive = live != 0
    ok = same_bits(out[:, 0], out[:, 2]) & same_bits(out[:, 1], out[:, 3])
    bad = np.flatnonzero(~ok & alive)
    assert len(bad) == 0, [(int(i), float(x[i]), out[i].view(U).tolist()) for i in bad[:5]]
    assert (out[~alive] == 0).all()                                           # a lane that is not active wrote nothing
    zero = np.flatnonzero(alive & (x.view(U) == 0x80000000))                  # the reference columns are ptmi_sincosf's: sin -0, cos -0
    assert len(zero) and (out[zero, 3] == 1).all() and (out[zero, 2] == 0).all()


@pytest.mark.parametrize("size", SIZES)
def test_division_by_image_size(R, size):
    hi = bits(size)
    bad, first, lean = R.debug_size_div_check(size, LO33, hi - LO33 + 1)      # every float in [2^-33, W]
    assert lean, size
    assert bad == 0, (size, bad, hex(first))


def test_division_keeps_ieee_above_2_23(R):
    size = (1 << 23) + 1
    bad, first, lean = R.debug_size_div_check(size, LO33, bits(size) - LO33 + 1)
    assert not lean
    assert bad == 0, (bad, hex(first))
    assert R.debug_size_div_check(1 << 23, LO33, 1 << 20)[2]                  # 2^23 itself still takes the short form


def ordinary_vectors(rng, n):
    """n vectors whose squared length lies well inside [2^-96, 2^100]: random sign and mantissa, exponents in [-40, 40)"""
    e = rng.integers(127 - 40, 127 + 40, (n, 3)).astype(U)
    b = (rng.integers(0, 2, (n, 3)).astype(U) << U(31)) | (e << U(23)) | rng.integers(0, 1 << 23, (n, 3)).astype(U)
    return b.view(F)


def squared_length(w):
    """length_squared (pt_vec.h) in numpy's binary32: the dot product in its order"""
    with np.errstate(all="ignore"):
        l2 = (w[:, 0] * w[:, 0]).astype(F)
        l2 = (l2 + (w[:, 1] * w[:, 1]).astype(F)).astype(F)
        return (l2 + (w[:, 2] * w[:, 2]).astype(F)).astype(F)


def unit_vector_host(w):
    """unit_vector (pt_vec.h) in numpy's binary32: the IEEE root and quotient of squared_length"""
    with np.errstate(all="ignore"):
        k = (F(1.0) / np.sqrt(squared_length(w)).astype(F)).astype(F)
        return (w * k[:, None]).astype(F)


def two_squares(target_bits):
    """(x, y, 0) whose squared length, as the kernel rounds it, is exactly the float with these bits"""
    t = float(f32(target_bits))
    x = F(np.sqrt(t * 0.5))
    y0 = bits(F(np.sqrt(t - float(F(x * x)))))
    for d in range(0, 65):
        for y in (f32(y0 + d), f32(y0 - d)):
            v = np.array([[x, y, 0]], F)
            if bits(squared_length(v)[0]) == target_bits:
                return v[0]
    raise AssertionError(f"no pair of squares adds up to {target_bits:#010x}")


LO96, HI100 = (127 - 96) << 23, (127 + 100) << 23      # 2^-96 and 2^100, the ends of the vote's interval
EDGES = [LO96 - 1, LO96, LO96 + 1, HI100 - 1, HI100, HI100 + 1]      # the floats next to both ends, on both sides, and the ends
DENORMAL_L2 = np.array([[2.0 ** -70, 0, 0], [2.0 ** -64, 0, 0], [1.37 * 2.0 ** -66, 2.0 ** -67, 0], [0, 2.0 ** -74, 1.9 * 2.0 ** -74]], F)


def test_unit_vector_vote(R):
    rng = np.random.default_rng(13)
    edge = np.array([two_squares(b) for b in EDGES], F)
    assert [bits(v) for v in squared_length(edge)] == EDGES                   # what the lanes are fed, as the kernel adds it up
    l2_den = squared_length(DENORMAL_L2)
    assert ((l2_den > 0) & (l2_den < F(2.0) ** -126)).all(), l2_den            # squared lengths that are denormals
    # these are the cases that tell whether the lower bound of the vote acts: the short root alone is wrong for each of them
    assert [R.debug_sqrt_check(bits(v), 1)[0] for v in l2_den] == [1] * len(l2_den)
    component = np.concatenate([
        f32([0x00000000, 0x80000000, 0x00000001, 0x007FFFFF]),                # squared length 0: a zero vector, denormal components
        F(2.0) ** np.array([-60, 60], F),                                      # far outside: 2^-120, and 2^120
        np.array([np.inf, -np.inf, np.nan], F),
    ])
    special = np.concatenate([edge, DENORMAL_L2, np.array([[s, 0, 0] for s in component], F),
                              np.array([[2.0 ** 64, 2.0 ** 64, 0]], F)])       # finite components, the squared length overflows
    waves, live = [], []
    waves.append(ordinary_vectors(rng, 64)); live.append(np.ones(64, np.int32))          # nothing to vote about: the short form
    unit = rng.normal(0, 1, (64, 3)); unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    waves.append(unit.astype(F)); live.append(np.ones(64, np.int32))                    # bounce directions: length 1 to rounding
    for v in special:
        for lane in (0, 37, 63):
            w = ordinary_vectors(rng, 64); w[lane] = v
            waves.append(w); live.append(np.ones(64, np.int32))
        w = ordinary_vectors(rng, 64); w[11] = np.roll(v, 1)                  # the same length through the other components
        waves.append(w); live.append(np.ones(64, np.int32))
        w = ordinary_vectors(rng, 64); w[5] = v                               # in a lane that is not active: no say in the vote
        l = np.ones(64, np.int32); l[5] = 0
        waves.append(w); live.append(l)
    w = ordinary_vectors(rng, 23); w[22] = (0, 0, 0)                          # a partial last wave
    waves.append(w); live.append(np.ones(23, np.int32))
    w = np.concatenate(waves); live = np.concatenate(live)
    out = R.debug_unit_voted(w, live)
    alive = live != 0
    got, want = out[:, :3], out[:, 3:]
    bad = np.argwhere(~same_bits(got, want) & alive[:, None])
    assert len(bad) == 0, [(int(i), int(c), w[i].tolist(), got[i, c].view(U), want[i, c].view(U)) for i, c in bad[:5]]
    host = unit_vector_host(w)
    bad = np.argwhere(~same_bits(got, host) & alive[:, None])
    assert len(bad) == 0, [(int(i), int(c), w[i].tolist(), got[i, c].view(U), host[i, c].view(U)) for i, c in bad[:5]]
    assert (out[~alive] == 0).all()
    zeros = alive & (w == 0).all(axis=1)
    assert zeros.any() and np.isnan(got[zeros]).all()                          # 0 * (1 / 0): a NaN, as unit_vector gives


def test_roulette_reciprocal(R):
    hi = bits(0.95)
    bad, first = R.debug_rcp_check(LO33, hi - LO33 + 1)                        # every float in [2^-33, 0.95f]
    assert bad == 0, (bad, hex(first))
