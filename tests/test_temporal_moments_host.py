"""CPU tests of the history's luminance statistics (include/ptmi.h: ptmi_set_temporal_moments): the float32 recurrence of
tests/temporal_moments_oracle.py against binary64, the raw-moment form it replaces, and the edges of the contract.  No GPU."""
import numpy as np
import pytest

import ptmi
import temporal_moments_oracle as TM
from filter_edge_sets import dn, up

F = np.float32
D = np.float64
PIXELS = 627                                                         # 33 x 19
FRAMES = [2, 4, 8, 32]
# (mean, sd) of the inputs' luminance
INPUTS = {"unit": (1.0, 0.2), "dark": (0.5, 0.5), "bright": (1e3, 1e-2)}
# The largest |s2 - np.var| / sd^2 over the 627 pixels, measured on the restatement (numpy 1.26, x86-64), and the bound, four
# times that (the precedent of DESIGN 4.18 and 4.22).  "bright" is the input's own quantisation: an ulp of 1e3 is 6e-5, 0.6 % of sd.
#   frames        2        4        8        32
#   unit      4.9e-07  7.1e-07  4.5e-07  8.2e-07       (the raw-moment form: 6.7e-06  7.7e-06  9.9e-06  2.2e-05)
#   dark      3.6e-07  9.7e-07  6.6e-07  4.3e-07       (                     1.2e-06  1.3e-06  6.5e-07  1.0e-06)
#   bright    0        5.5e-03  6.0e-03  7.9e-03       (                     1.3e+03  1.9e+03  2.5e+03  4.4e+03)
MEASURED = {"unit": 8.2e-7, "dark": 9.7e-7, "bright": 7.9e-3}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
# the capped history (max_history = 8, 32 frames) against the same recurrence in binary64: measured 7.2e-7, 3.1e-7, 7.2e-3
MEASURED_CAPPED = {"unit": 7.2e-7, "dark": 3.1e-7, "bright": 7.2e-3}


def draws(which, frames, seed=1):
    mean, sd = INPUTS[which]
    return np.random.default_rng(seed).normal(mean, sd, (frames, PIXELS)).astype(F)


def run(x, max_history, T=F, m=2.0):
    """the still camera's recurrence over the frames x (frames, pixels): restart, then BLEND with step 5's alpha"""
    x = x.astype(T)
    m = T(m)
    mu, s2, k, n = x[0].copy(), np.zeros(x.shape[1], T), np.ones(x.shape[1], T), np.full(x.shape[1], m, T)
    for l in x[1:]:
        n = np.fmin(n + m, T(max_history) * m)
        mu, s2, k = TM.blend(mu, s2, k, l, m / n, max_history, T)
    return mu, s2, k


def run_raw(x, max_history, m=2.0):
    m = F(m)
    m1, m2, n = x[0].copy(), x[0] * x[0], np.full(x.shape[1], m, F)
    var = np.zeros(x.shape[1], F)
    for l in x[1:]:
        n = np.fmin(n + m, F(max_history) * m)
        m1, m2, var = TM.raw_blend(m1, m2, l, m / n)
    return var


@pytest.mark.parametrize("which", list(INPUTS))
@pytest.mark.parametrize("frames", FRAMES)
def test_uncapped_recurrence_is_the_population_variance(which, frames):
    x = draws(which, frames)
    mu, s2, k = run(x, 65536)
    assert mu.dtype == F and s2.dtype == F and k.dtype == F
    ref = np.var(x.astype(D), axis=0)
    sd2 = INPUTS[which][1] ** 2
    err = float(np.abs(s2.astype(D) - ref).max() / sd2)
    print(f"{which} {frames}: blend {err:.2e}")
    assert err <= BOUND[which]
    assert np.array_equal(k, np.full(PIXELS, F(frames)))
    # the mean: one rounding of at most half an ulp of max |x| per frame
    assert np.abs(mu.astype(D) - x.astype(D).mean(0)).max() <= frames * 2.0 ** -24 * float(np.abs(x).max())


@pytest.mark.parametrize("which", list(INPUTS))
def test_raw_moment_form_fails_the_bound(which):
    """the reason for the contract: E[l^2] - E[l]^2 carried in float32 misses the bound the blend form keeps"""
    worst = 0.0
    for frames in FRAMES:
        x = draws(which, frames)
        ref = np.var(x.astype(D), axis=0)
        err = float(np.abs(run_raw(x, 65536).astype(D) - ref).max() / INPUTS[which][1] ** 2)
        print(f"{which} {frames}: raw {err:.2e}")
        worst = max(worst, err)
    if which == "dark":                                               # mean and spread of one size: nothing cancels, and the raw
        return                                                        # form is as good as the other (the figures beside MEASURED)
    assert worst > BOUND[which]


@pytest.mark.parametrize("which", list(INPUTS))
def test_capped_recurrence_against_binary64(which):
    x = draws(which, 32)
    mu, s2, k = run(x, 8)
    mu64, s264, k64 = run(x, 8, D)
    err = float(np.abs(s2.astype(D) - s264).max() / INPUTS[which][1] ** 2)
    print(f"{which} capped: {err:.2e}")
    assert err <= 4.0 * MEASURED_CAPPED[which]
    assert np.array_equal(k, np.full(PIXELS, F(8))) and np.array_equal(k64, np.full(PIXELS, 8.0))
    assert s2.min() > 0


def test_alpha_one():
    """max_history = 1: s2 = 0 * (...), which is 0, or NaN for a non-finite operand; mu goes through h + (l - h)"""
    one = F(1)
    with np.errstate(all="ignore"):
        mu, s2, k = TM.blend(F(0.3), F(0.7), F(1), F(1.9), one, 1)
        assert (mu, k) == (F(0.3) + (F(1.9) - F(0.3)), one) and s2 == 0 and not np.signbit(s2)
        for bad in (F(np.inf), F(np.nan)):
            assert np.isnan(TM.blend(F(0.3), bad, one, F(1.9), one, 1)[1])
            assert np.isnan(TM.blend(bad, F(0.7), one, F(1.9), one, 1)[1])
            assert np.isnan(TM.blend(F(0.3), F(0.7), one, bad, one, 1)[1])


def test_k_at_the_cap():
    alpha = F(0.25)
    for k_h, cap, want in ((F(7), 8, F(8)), (dn(7), 8, dn(7) + F(1)), (F(8), 8, F(8)), (up(7), 8, F(8)), (F(np.nan), 8, F(8)),
                           (F(1), 1, F(1)), (F(65535), 65536, F(65536))):
        with np.errstate(invalid="ignore"):
            got = TM.blend(F(1), F(0.1), k_h, F(1.1), alpha, cap)[2]
        assert got.dtype == F and got == want, (k_h, cap)


def test_variance_is_clamped_at_zero():
    c = np.full((1, 4, 3), F(0.5))
    s2 = np.array([[F(-1e-3), F(np.nan), F(0.3), F(-np.inf)]])
    k = np.full((1, 4), F(5))
    v = TM.temporal_variance(c, c, s2, k)
    assert np.array_equal(v.view(np.uint32), np.array([[0, 0, (F(0.3) / F(4)).view(np.uint32), 0]], np.uint32))
    scaled = TM.temporal_variance(c * F(2), c, s2, k)                  # a demodulated signal twice the history's
    s = TM.lum(c * F(2)) / TM.lum(c)
    assert np.array_equal(scaled[0, 2], ((F(0.3) / F(4)) * s[0, 2]) * s[0, 2])
    black = TM.temporal_variance(c, c * F(0), s2, k)                   # lr > 0 does not hold: no conversion
    assert black[0, 2] == F(0.3) / F(4)


def test_ownership_around_min_frames():
    k = np.array([dn(4), F(4), up(4), F(1), F(3), F(np.nan), F(np.inf)], F)
    assert TM.MIN_FRAMES == F(4)
    assert TM.owned(k).tolist() == [False, True, True, False, False, False, True]
    c = np.full((1, 3, 3), F(1))
    v = TM.temporal_variance(c, c, np.full((1, 3), F(0.6)), k[None, :3])
    assert np.array_equal(v[0], np.array([F(0.6) / (dn(4) - F(1)), F(0.6) / F(3), F(0.6) / (up(4) - F(1))], F))


def test_library_exports_the_new_entry_points():
    L = ptmi.lib()
    for name in ("ptmi_set_temporal_moments", "ptmi_get_temporal_moments", "ptmi_read_temporal_moments",
                 "ptmi_denoise_temporal_variance", "ptmi_debug_set_temporal_moments"):
        assert hasattr(L, name) and name in ptmi.EXPORTS, name
    assert L.ptmi_set_temporal_moments(None, 0) == -1                  # a NULL context is refused, not followed
