"""Host side of the variance-guided a-trous filter (include/ptmi.h: ptmi_denoise_variance) - no GPU needed: the parameter check
through the C ABI, and what the contract promises, shown on its numpy restatement (tests/variance_oracle.py), which
tests/test_gpu_variance.py holds the kernels to bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ptmi
import variance_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -24                                   # float32's unit roundoff


def gamma(n):
    """the bound (1 + d_1) .. (1 + d_n) = 1 + t, |t| <= gamma(n), of n roundings"""
    return n * U / (1 - n * U)


def uniform_features(h, w):
    """normals and positions that make wn = wx = 1 exactly"""
    nrm = np.zeros((h, w, 3), F); nrm[..., 2] = 1
    pos = np.full((h, w, 3), 0.5, F)
    return nrm, pos


# ------------------------------------------------------------------------------------------------
# 1. parameters
# ------------------------------------------------------------------------------------------------
def test_default_variance_params_and_struct_match_the_header():
    p = ptmi.default_variance_params()
    assert (p.iterations, p.normal_squarings, p.feature_grid, p.demodulate, p.source, p.spatial_radius) == (5, 7, 2, 1, 0, 3)
    assert (p.sigma_luminance, p.epsilon, p.sigma_position) == (2.0, F(1e-2), 0.0)
    q = ptmi.default_variance_params(iterations=3, source=1)
    assert (q.iterations, q.source, q.spatial_radius) == (3, 1, 3)
    with pytest.raises(TypeError):
        ptmi.default_variance_params(sigma_color=3.0)
    header = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*ptmi_variance_params;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"^\w+\s+", "", d.strip()) for d in body.split(";") if d.strip()]
    assert fields == [f for f, _ in ptmi.VarianceParams._fields_]
    assert C.sizeof(ptmi.VarianceParams) == 36


NAN = float("nan")
BAD = [("iterations", -1), ("iterations", 11),
       ("sigma_luminance", 9e-5), ("sigma_luminance", 2e4), ("sigma_luminance", NAN),
       ("epsilon", 9e-13), ("epsilon", 2e4), ("epsilon", NAN),
       ("sigma_position", 1e-9), ("sigma_position", 2e12), ("sigma_position", NAN),
       ("normal_squarings", -1), ("normal_squarings", 11),
       ("feature_grid", 0), ("feature_grid", 5),
       ("demodulate", -1), ("demodulate", 2),
       ("source", -1), ("source", 2),
       ("spatial_radius", 0), ("spatial_radius", 4)]


@pytest.mark.parametrize("field,value", BAD)
def test_variance_params_are_validated(field, value):
    L = ptmi.lib()
    p = ptmi.default_variance_params(**{field: value})
    assert L.ptmi_check_variance_params(C.byref(p)) == -1
    msg = L.ptmi_last_error().decode()
    assert msg.startswith("denoise: " + field + " must be"), msg


def test_valid_variance_params_pass_and_the_shared_messages_are_ptmi_denoises():
    L = ptmi.lib()
    for ok in (dict(), dict(iterations=0), dict(iterations=10), dict(sigma_luminance=1e-4), dict(sigma_luminance=1e4),
               dict(epsilon=1e-12), dict(epsilon=1e4), dict(sigma_position=-1.0), dict(sigma_position=1e-6), dict(normal_squarings=0),
               dict(normal_squarings=10), dict(feature_grid=1), dict(feature_grid=4), dict(demodulate=0), dict(source=1),
               dict(spatial_radius=1)):
        assert L.ptmi_check_variance_params(C.byref(ptmi.default_variance_params(**ok))) == 0, ok
    for bad in (dict(iterations=11), dict(sigma_position=1e-9), dict(normal_squarings=11), dict(feature_grid=0), dict(demodulate=2)):
        assert L.ptmi_check_variance_params(C.byref(ptmi.default_variance_params(**bad))) == -1
        mine = L.ptmi_last_error().decode()
        assert L.ptmi_check_denoise_params(C.byref(ptmi.default_denoise_params(**bad))) == -1
        assert L.ptmi_last_error().decode() == mine
    assert L.ptmi_check_variance_params(None) == -1 and L.ptmi_denoise_variance(None, None) == -1
    assert L.ptmi_read_variance(None, None, None) == -1 and L.ptmi_variance_timing(None, None, None) == -1
    assert L.ptmi_read_pass_moments(None, None, None, None) == -1
    L.ptmi_default_variance_params(None)


# ------------------------------------------------------------------------------------------------
# 2. a constant image with zero variance passes through exactly
# ------------------------------------------------------------------------------------------------
def test_constant_image_with_zero_variance_passes_through_bit_for_bit():
    # values of a few mantissa bits: every product h * c and every partial sum is exact, at the borders too, so S = c * W exactly
    h, w = 19, 23
    c = np.empty((h, w, 3), F); c[...] = (0.75, 1.5, 0.3125)
    nrm, pos = uniform_features(h, w)
    for iterations in (1, 3, 5):
        out, vo = VO.atrous(c, np.zeros((h, w), F), nrm, pos, iterations, 4.0, 1e-6, 0.1, 7)
        assert np.array_equal(out.view(np.uint32), c.view(np.uint32)) and not vo.any()
    # and through the whole filter: a constant albedo of 1/2 is divided out and multiplied in exactly, the spatial variance of a
    # constant luminance is exactly 0 where the window's sum of l is exact - l = 1 here
    rad = np.empty((h, w, 3), F); rad[...] = 0.5
    feat = dict(albedo=np.full((h, w, 3), 0.5, F), normal=nrm, position=pos)
    assert VO.lum(np.ones((1, 3), F))[0] == 1
    out, vin, vo = VO.denoise_variance(rad, feat, 5, 4.0, 1e-6, 0.1, 7)
    assert np.array_equal(out.view(np.uint32), rad.view(np.uint32)) and not vin.any() and not vo.any()


# ------------------------------------------------------------------------------------------------
# 3. uniform variance, no luminance edge-stop: the plain B3 convolution; the variance shrinks by (70/256)^2
# ------------------------------------------------------------------------------------------------
def test_uniform_variance_gives_the_b3_convolution_and_its_variance():
    h, w = 21, 17
    rng = np.random.default_rng(5)
    c = rng.uniform(0.0, 0.5, (h, w, 3)).astype(F)                # |dl| <= 1/2
    nrm, pos = uniform_features(h, w)
    v0 = F(0.37)
    # a = 1e8 * 0.37: dl^2 / a <= 6.8e-9 < 2^-25, so 1 + dl^2 / a rounds to 1 and wl = 1 exactly
    out, vo = VO.atrous(c, np.full((h, w), v0, F), nrm, pos, 1, 1e4, 1e-6, 0.1, 7)
    b = np.array([1, 4, 6, 4, 1], np.float64) / 16
    num = np.zeros((h, w, 3)); den = np.zeros((h, w)); den2 = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            for j in range(5):
                for i in range(5):
                    qy, qx = y + j - 2, x + i - 2
                    if 0 <= qy < h and 0 <= qx < w:
                        num[y, x] += b[j] * b[i] * c[qy, qx].astype(np.float64)
                        den[y, x] += b[j] * b[i]; den2[y, x] += (b[j] * b[i]) ** 2
    want = num / den[..., None]
    # S: 25 products (the weights are exact) and 24 additions of positive terms, then one division by the exact W: gamma(26)
    assert (np.abs(out - want) <= gamma(26) * want).all()
    assert np.abs(out - c).max() > 0.01
    # V: (w * w) exact, x v one rounding each, 24 additions, two divisions by the exact W: gamma(27)
    want_v = float(v0) * den2 / den ** 2
    assert (np.abs(vo - want_v) <= gamma(27) * want_v).all()
    inner = want_v[2:-2, 2:-2]
    assert np.allclose(inner, float(v0) * (70 / 256) ** 2, rtol=1e-15, atol=0)
    assert (np.abs(vo[2:-2, 2:-2] - float(v0) * (70 / 256) ** 2) <= gamma(27) * float(v0) * (70 / 256) ** 2).all()


# ------------------------------------------------------------------------------------------------
# 4. a luminance step survives: no pixel moves further than the closed form allows
# ------------------------------------------------------------------------------------------------
def test_luminance_step_is_preserved_to_the_closed_form():
    h, w, edge = 12, 16, 7                                        # columns >= edge are the bright side
    c = np.zeros((h, w, 3), F); c[:, edge:] = 1.0
    nrm, pos = uniform_features(h, w)
    L = VO.lum(c)
    D = float(L[0, edge]) - float(L[0, 0])
    sigma_l, v0, eps = 1.0, 5e-5, 1e-6
    a = sigma_l * sigma_l * v0 + eps
    assert D * D / a >= 1e4
    wlx = 1 / (1 + D * D / a)                                     # what a tap across the edge weighs, next to 1 on this side
    out, _ = VO.atrous(c, np.full((h, w), v0, F), nrm, pos, 1, sigma_l, eps, 0.1, 7)
    b = np.array([1, 4, 6, 4, 1], np.float64) / 16
    tight = 0
    for y in range(h):
        for x in range(w):
            same = cross = 0.0
            for j in range(5):
                for i in range(5):
                    qy, qx = y + j - 2, x + i - 2
                    if 0 <= qy < h and 0 <= qx < w:
                        if (qx >= edge) == (x >= edge): same += b[j] * b[i]
                        else: cross += b[j] * b[i]
            bound = wlx * cross / (same + wlx * cross)             # of the step's height 1, towards the other side
            moved = (out[y, x].astype(np.float64) - c[y, x]) * (-1 if x >= edge else 1)
            # a is formed in float32 from the prefiltered variance (<= 8 roundings, it enters wl with a factor below 1), the
            # sums take 26 more; a bright pixel also rounds at its own size 1
            slack = gamma(34) * bound + (gamma(26) if x >= edge else 0.0)
            assert (moved >= -slack).all() and (moved <= bound + slack).all(), (y, x, moved, bound)
            if cross and x < edge:
                assert (moved >= bound - slack).all()             # and the bound is reached: it is the closed form
                tight += 1
    assert tight == 2 * h                                         # the two columns whose taps reach over the edge
    # the column next to the edge has 5/16 of its (separable) weights across it: the step moves by wlx * 5/11 = 2.3e-5 at most,
    # against 5/16 through the plain convolution
    assert np.abs(out - c).max() <= wlx * 5 / 11 * (1 + gamma(34)) + gamma(26)


# ------------------------------------------------------------------------------------------------
# 5. why the contract takes two sweeps
# ------------------------------------------------------------------------------------------------
def test_two_sweep_variance_survives_a_bright_pixel():
    rng = np.random.default_rng(11)
    n, lum0, spread = 49, 1e3, 1e-2
    grey = (lum0 + spread * rng.standard_normal((7, 7))).astype(F)
    c = np.repeat(grey[..., None], 3, axis=2)
    nrm, pos = uniform_features(7, 7)
    l32 = VO.lum(c)                                               # the data: what both forms are given
    l64 = l32.astype(np.float64)
    true = float(((l64 - l64.mean()) ** 2).mean())
    assert 0.5 * spread ** 2 < true < 2 * spread ** 2
    got = float(VO.spatial_variance(c, nrm, pos, 3, 7, 0.1)[3, 3])
    # the mean carries at most gamma(n) * l of rounding (n - 1 additions and a division), which shifts the variance by its
    # square; l_q - m is exact (Sterbenz), and the second sweep adds n + 2 roundings of its own
    bound = (gamma(n) * lum0) ** 2 / true + gamma(n + 2)
    assert bound < 0.2                                            # it says something: the one-sweep form misses by a factor
    print(f"two-sweep: true {true:.6e} got {got:.6e} relative error {abs(got - true) / true:.3e} (bound {bound:.3e})")
    assert abs(got - true) <= bound * true
    # the one-sweep form in float32, E[l^2] - E[l]^2: both terms are 1e6 +- 0.06
    s1 = F(0); s2 = F(0)
    for x in l32.ravel():
        s1 = F(s1 + x); s2 = F(s2 + F(x * x))
    one = float(F(F(s2 / F(n)) - F(F(s1 / F(n)) * F(s1 / F(n)))))
    print(f"one-sweep: {one:.6e}")                                # -0.0625 here, a negative variance 860 times the true one in size (other seeds: 0, 0.0625)
    assert abs(one - true) > 100 * bound * true


# ------------------------------------------------------------------------------------------------
# 6. the float32 restatement against binary64
# ------------------------------------------------------------------------------------------------
def seeded_input(h=32, w=40, seed=2024):
    """a lit wall meeting a floor, with a noisy radiance: smooth albedo, two normals, positions on the two planes"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    floor = yy < h // 3
    nrm = np.zeros((h, w, 3), F); nrm[floor] = (0, 1, 0); nrm[~floor] = (0, 0, 1)
    pos = np.stack([xx * 0.05, np.where(floor, 0.0, (yy - h // 3) * 0.05), np.where(floor, (h // 3 - yy) * 0.05, 0.0)], -1).astype(F)
    alb = (0.3 + 0.6 * rng.random((1, 1, 3)) * (0.5 + 0.5 * np.sin(xx / 7.0))[..., None]).astype(F)
    clean = alb * (0.2 + 0.8 * (xx / w))[..., None]
    rad = (clean * rng.gamma(4.0, 0.25, (h, w, 1))).astype(F)
    return rad, dict(albedo=alb, normal=nrm, position=pos)


MEASURED = dict(radiance=6.473e-07, variance_in=5.835e-07, variance_out=1.779e-06)   # printed by the test below


def test_restatement_against_binary64():
    rad, feat = seeded_input()
    args = (5, 4.0, 1e-6, 0.1, 7)
    r32, vi32, vo32 = VO.denoise_variance(rad, feat, *args)
    r64, vi64, vo64 = VO.denoise_variance(rad, feat, *args, T=np.float64)
    assert r32.dtype == F and vi32.dtype == F and vo32.dtype == F and r64.dtype == np.float64
    worst = {}
    for name, a, b in (("radiance", r32, r64), ("variance_in", vi32, vi64), ("variance_out", vo32, vo64)):
        assert (b > 0).all()
        worst[name] = float((np.abs(a - b) / b).max())
    print("float32 against binary64, worst relative error: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for name in worst:
        assert worst[name] <= 4 * MEASURED[name], name            # four times the measured value, as test_nee_call_sets_host.py
    assert not np.array_equal(r32, rad) and (vo32 < vi32).mean() > 0.9
