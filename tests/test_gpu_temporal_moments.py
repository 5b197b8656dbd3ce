"""The history's luminance statistics (include/ptmi.h: ptmi_set_temporal_moments) and the variance-guided filter steered by them
(ptmi_denoise_temporal_variance) against their numpy float32 restatement (tests/temporal_moments_oracle.py), bit for bit, a NaN
counting as equal to a NaN; then the expected value of the variance on a constructed still camera, and what the filter buys.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ptmi
import denoise_oracle as DO
import filter_edge_sets as FS
import temporal_moments_oracle as TM
import temporal_oracle as TO
import variance_oracle as VO

from test_gpu_denoise import tone_map
from test_gpu_filter_edges import same, where_differs
from test_gpu_nee_expectation import Z_MAX
from test_gpu_temporal import CBOX, H, ORBIT, W, auto_sigma, bits, expect_error, load, view

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the two parameter sets of test_gpu_temporal.test_orbit_matches_numpy, by feature grid
ORBIT_PARAMS = {1: dict(feature_grid=1), 2: dict(feature_grid=2, max_history=3, normal_min=0.5, sigma_position=0.4, sigma_albedo=0.3)}


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def plain_step(R, hist, m, prm):
    """one step on the GPU and in the parent's restatement (temporal_oracle alone): output, counts, stats"""
    _, rad = R.read_image()
    cam = R.camera_frame()
    _, out, st = R.temporal_accumulate(**prm)
    p = ptmi.default_temporal_params(**prm)
    sx = p.sigma_position if p.sigma_position > 0 else auto_sigma(R)
    exp, hist, stats = TO.step(hist, rad, m, R.features(), cam, p.max_history, p.normal_min, sx, p.sigma_albedo)
    assert same(out, exp), where_differs(out, exp)
    assert same(R.history_counts(), hist.count)
    assert (st.accepted, st.rejected, st.missed) == stats
    return hist, st


def checked_step(R, hist, mom, m, prm, rad=None, feat=None, cam=None):
    """one step with the switch on, on the GPU and in numpy: output, counts, stats and (mu, s2, k); returns (the numpy history,
    its statistics, the stats, the output)"""
    rad = R.read_image()[1] if rad is None else rad
    cam = R.camera_frame() if cam is None else cam
    rgb, out, st = R.temporal_accumulate(**prm)
    feat = R.features() if feat is None else feat
    p = ptmi.default_temporal_params(**prm)
    sx = p.sigma_position if p.sigma_position > 0 else auto_sigma(R)
    exp, hist, stats, mom = TM.step(hist, mom, rad, m, feat, cam, p.max_history, p.normal_min, sx, p.sigma_albedo)
    assert same(out, exp), where_differs(out, exp)
    assert same(R.history_counts(), hist.count), where_differs(R.history_counts(), hist.count)
    assert (st.accepted, st.rejected, st.missed) == stats
    assert st.accepted + st.rejected + st.missed == out.shape[0] * out.shape[1]
    for name, got, want in zip(("mu", "s2", "k"), R.temporal_moments(), mom):
        assert same(got, want), (name, where_differs(got, want))
    assert np.array_equal(rgb, tone_map(exp))
    return hist, mom, st, out


# ------------------------------------------------------------------------------------------------
# 1. the step with the statistics against the restatement, along the orbit of test_gpu_temporal.py
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cbox", "cbox_quads", "soup"])
@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("w,h", [(W, H), (33, 19), (5, 3)])
def test_orbit_matches_numpy(R, which, g, w, h):
    """33 x 19: the last wave's lanes past the image are live in the ballots; 5 x 3: smaller than a workgroup"""
    load(R, which)
    view(R, *ORBIT[0])
    R.set_config(spp=2, max_depth=5)
    R.update_resolution(w, h)
    R.set_temporal_moments(1)
    R.temporal_reset()
    hist, mom, seen, spread = None, None, [], 0.0
    for yaw, pitch in ORBIT:
        view(R, yaw, pitch)
        R.render_frame()
        hist, mom, st, _ = checked_step(R, hist, mom, 2, ORBIT_PARAMS[g])
        seen.append(st)
        spread = max(spread, float(mom[1].max()))
    assert seen[0].accepted == 0 and seen[-1].accepted == w * h
    if (w, h) != (5, 3):
        assert seen[1].accepted > 0
        assert mom[2].max() > 1 and spread > 0                         # frames were counted and a variance was seen (the last
                                                                       # views look away from the box: black, and no variance)


def test_orbit_with_adaptive_passes_matches_numpy(R):
    """per-pixel m: alpha differs from pixel to pixel"""
    load(R, "cbox")
    R.set_config(spp=2, max_depth=5)
    R.update_resolution(W, H)
    R.set_temporal_moments(1)
    R.temporal_reset()
    hist, mom, varied = None, None, False
    for yaw, pitch in ORBIT[:3]:
        view(R, yaw, pitch)
        R.render_adaptive(min_passes=2, max_passes=8, threshold=0.1, floor=0.01)         # the runs of test_gpu_temporal.py
        m = R.sample_counts().astype(F)
        varied |= len(np.unique(m)) > 1
        hist, mom, _, _ = checked_step(R, hist, mom, m, dict(max_history=8))
    assert varied


# ------------------------------------------------------------------------------------------------
# 2. the switch
# ------------------------------------------------------------------------------------------------
def _three_plain_views(R, first_accepts_nothing=True):
    hist = None
    for i, (yaw, pitch) in enumerate(ORBIT[:3]):
        view(R, yaw, pitch)
        R.render_frame()
        hist, st = plain_step(R, hist, 2, dict(feature_grid=2))
        if i == 0 and first_accepts_nothing:
            assert st.accepted == 0
    assert st.accepted > 0


def test_switch_off_is_the_parents_step_on_a_fresh_context():
    r = ptmi.Renderer(0)
    try:
        assert r.get_temporal_moments() == 0
        load(r, "cbox")
        r.set_config(spp=2, max_depth=5)
        r.update_resolution(33, 19)
        _three_plain_views(r)
        expect_error(lambda: r.temporal_moments(), "temporal moments are off")
    finally:
        r.close()


def test_switch_off_after_on_and_what_the_switch_empties(R):
    load(R, "cbox")
    R.set_config(spp=2, max_depth=5)
    R.update_resolution(33, 19)
    R.set_temporal_moments(1)
    assert R.get_temporal_moments() == 1
    load(R, "cbox")                                                    # kept over scene loads
    assert R.get_temporal_moments() == 1
    R.set_config(spp=2, max_depth=5)
    view(R, *ORBIT[0])
    R.render_frame()
    image = R.read_image()
    R.temporal_accumulate()
    feats = R.features()
    assert R.history_counts().max() == 2
    R.set_temporal_moments(1)                                          # the current value: nothing happens
    assert R.history_counts().max() == 2
    R.set_temporal_moments(0)                                          # a new value empties the history and nothing else
    assert R.get_temporal_moments() == 0 and R.history_counts().max() == 0
    assert all(np.array_equal(a, b) for a, b in zip(image, R.read_image()))
    assert all(np.array_equal(bits(feats[k]), bits(v)) for k, v in R.features().items())
    _three_plain_views(R)                                              # its first step accepts nothing
    R.set_temporal_moments(1)
    assert R.history_counts().max() == 0
    R.render_frame()
    _, _, st = R.temporal_accumulate()
    assert st.accepted == 0
    for bad in (2, -1):
        expect_error(lambda: R.set_temporal_moments(bad), "on must be 0 or 1")
    assert R.get_temporal_moments() == 1 and R.history_counts().max() == 2


# ------------------------------------------------------------------------------------------------
# 3. constructed state through the two hooks
# ------------------------------------------------------------------------------------------------
def constructed_views(w, h):
    """Two views of one plane through filter_edge_sets' cameras: view A sees it through its pixel centres, view B's pixels hold
    the points that view A sees at (x + 0.37, y + 0.21) - every footprint mixes four taps with weights of their own; the last
    column and the top row lose taps to the image's edge."""
    cam_a, cam_b = FS.cameras()
    fa, fb = FS._frame(cam_a, w, h), FS._frame(cam_b, w, h)
    n0 = FS._axis_facing(fa, fb, w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    pos = {}
    for name, dx, dy in (("a", 0.0, 0.0), ("b", 0.37, 0.21)):
        pos[name] = np.array([[FS._point(fa, w, h, x + dx, y + dy, FS.DEPTH) for x in range(w)] for y in range(h)]).astype(F)
    feat = {k: dict(position=pos[k], normal=np.broadcast_to(n0, (h, w, 3)).copy(), albedo=np.full((h, w, 3), F(0.5)),
                    hit_fraction=np.ones((h, w), F)) for k in pos}
    rad = {k: (F(0.25) + F(2) * np.stack([FS.noise(xx, yy, c + s) for c in range(3)], -1)).astype(F) for k, s in (("a", 11), ("b", 23), ("c", 37))}
    return (cam_a, fa), (cam_b, fb), feat, rad


def ptmi_camera(yaw):
    c = ptmi.default_camera()
    c.yaw_deg = yaw
    return c


@pytest.mark.parametrize("w,h", [(8, 4), (33, 19)])
@pytest.mark.parametrize("cap", [8, 1])
def test_constructed_statistics(R, w, h, cap):
    (_, fa), (_, fb), feat, rad = constructed_views(w, h)
    prm = dict(max_history=cap, normal_min=0.9, sigma_position=100.0, sigma_albedo=0.125)
    load(R, "cbox")
    R.set_camera(ptmi_camera(FS.YAW_A))
    R.set_config(spp=FS.TEMPORAL_SPP, max_depth=5, integrator=0)
    R.update_resolution(w, h)
    R.set_temporal_moments(1)
    assert np.array_equal(bits(R.camera_frame()), bits(fa))
    m = FS.TEMPORAL_SPP
    # view A into an empty history: (l, 0, 1) everywhere
    R.debug_set_filter_inputs(rad["a"], feat["a"], grid=2)
    hist, mom, st, _ = checked_step(R, None, None, m, prm, rad["a"], feat["a"], fa)
    assert st.accepted == 0 and (mom[2] == 1).all() and (mom[1] == 0).all()
    # the history's statistics, constructed: k = 1, 3, 4 and the cap mixed within every footprint, a NaN and an Inf variance
    yy, xx = np.mgrid[0:h, 0:w]
    ks = np.array([1, 3, 4, cap], F)[(xx + 2 * yy) % 4]
    s2 = (F(0.01) + FS.noise(xx, yy, 5)).astype(F)
    s2[1, 2], s2[h - 2, w - 3] = F(np.nan), F(np.inf)
    mu = TM.lum(rad["a"]) + F(0.125)
    R.debug_set_temporal_moments(mu, s2, ks)
    for got, want in zip(R.temporal_moments(), (mu, s2, ks)):
        assert same(got, want)
    assert same(R.history_counts(), hist.count)                        # the hook touches nothing else
    # view B over it: the bilinear resampling of all three
    R.set_camera(ptmi_camera(FS.YAW_B))
    R.debug_set_filter_inputs(rad["b"], feat["b"], grid=2)
    hist, mom, st, _ = checked_step(R, hist, (mu, s2, ks), m, prm, rad["b"], feat["b"], fb)
    assert st.accepted >= (w - 1) * (h - 1)
    assert np.isnan(mom[1]).sum() >= 4                                 # the NaN reaches its four footprints
    if cap > 1:
        assert np.isinf(mom[1]).sum() >= 4                             # so does the Inf (with alpha = 1 it is 0 x Inf, a NaN)
        assert len(np.unique(mom[2])) > 4                              # fractional frame counts
    # the filter on this state: owned and spatial pixels side by side, a NaN variance among them
    for fprm in (dict(iterations=0), dict(iterations=2, spatial_radius=1)):
        check_filter(R, hist, mom, feat["b"], dict(fprm, sigma_position=FS.SIGMA_X))
    # the filter's own edges, injected: a negative and a NaN variance under fmaxf, k just below, at and just above 4
    s2e, ke = mom[1].copy(), mom[2].copy()
    s2e[0, :4] = [F(-0.5), F(np.nan), F(0.25), F(0.25)]
    ke[0, :4] = [F(4), F(5), FS.dn(4), FS.up(4)]
    R.debug_set_temporal_moments(mom[0], s2e, ke)
    vin, own = check_filter(R, hist, (mom[0], s2e, ke), feat["b"], dict(iterations=1, spatial_radius=1, sigma_position=FS.SIGMA_X))
    assert own[0, :4].tolist() == [True, True, False, True] and vin[0, 0] == 0 and vin[0, 1] == 0 and vin[0, 3] > 0
    mom = (mom[0], s2e, ke)
    # the still camera: k_h + 1 exactly at the cap, one below it, and at it already
    ks = np.array([cap - 1, cap - 2, cap, 1], F)[(xx + yy) % 4] if cap > 1 else np.ones((h, w), F)
    R.debug_set_temporal_moments(mom[0], mom[1], ks)
    R.debug_set_filter_inputs(rad["c"], feat["b"], grid=2)
    hist, mom, st, _ = checked_step(R, hist, (mom[0], mom[1], ks), m, prm, rad["c"], feat["b"], fb)
    assert st.accepted == w * h and mom[2].max() == cap
    if cap == 1:
        finite = np.isfinite(mom[1])
        assert (mom[1][finite] == 0).all() and (mom[2] == 1).all()


# ------------------------------------------------------------------------------------------------
# 4. the filter over the history
# ------------------------------------------------------------------------------------------------
def check_filter(R, hist, mom, feat, prm):
    """ptmi_denoise_temporal_variance(**prm) on the history (numpy's copy: hist, mom; feat: the history's features) against the
    restatement: radiance, rgb8, variance in and out.  Returns (variance_in, the owned mask)."""
    p = ptmi.default_variance_params(**prm)
    b = R.scene_bvh()
    sx = p.sigma_position if p.sigma_position > 0 else DO.auto_sigma_position(b["bmin"][0], b["bmax"][0])
    drgb, drad = R.denoise_temporal_variance(**prm)
    vin, vout = R.variance()
    erad, evin, evout = TM.denoise_temporal_variance(hist.color, feat, mom, p.iterations, p.sigma_luminance, p.epsilon, sx,
                                                     p.normal_squarings, bool(p.demodulate), p.spatial_radius, p.source)
    assert same(vin, evin), (prm, where_differs(vin, evin))
    assert same(vout, evout), (prm, where_differs(vout, evout))
    assert same(drad, erad), (prm, where_differs(drad, erad))
    assert np.array_equal(drgb, tone_map(erad)), prm
    assert all(np.array_equal(a, b_) for a, b_ in zip(R.read_denoised(), (drgb, drad)))
    return vin, TM.owned(mom[2])


FW, FH = 67, 45                  # more than one workgroup each way, no multiple of the 16 x 16 tile
FILTER_PARAMS = [dict(iterations=0, spatial_radius=1), dict(iterations=0, spatial_radius=3), dict(iterations=3, spatial_radius=1),
                 dict(iterations=3, spatial_radius=3), dict(iterations=3, demodulate=0), dict(iterations=3, source=1)]


def filter_orbit(R, views):
    load(R, "cbox")
    R.set_config(spp=2, max_depth=5)
    R.update_resolution(FW, FH)
    R.set_temporal_moments(1)
    R.temporal_reset()
    hist, mom = None, None
    for i in range(views):
        view(R, 90.0 + 1.5 * i)
        R.render_frame()
        hist, mom, _, _ = checked_step(R, hist, mom, 2, dict())
    return hist, mom


@pytest.mark.parametrize("views", [3, 6])
def test_denoise_temporal_variance_matches_numpy(R, views):
    hist, mom = filter_orbit(R, views)
    feat = R.features()                                                # the history's view's features (current, g = 2)
    own = TM.owned(mom[2])
    if views == 3:
        assert not own.any()                                           # k <= 3: the spatial estimate everywhere
    else:
        assert own.any() and (~own).any()                              # pixels on both sides of k >= PTMI_TEMPORAL_MIN_FRAMES
    for prm in FILTER_PARAMS:
        vin, _ = check_filter(R, hist, mom, feat, prm)
        b = R.scene_bvh()
        spatial = VO.denoise_variance(hist.color, feat, 0, 2.0, 0.01, DO.auto_sigma_position(b["bmin"][0], b["bmax"][0]), 7,
                                      bool(prm.get("demodulate", 1)), prm.get("spatial_radius", 3))[1]
        if prm.get("source") == 1 or views == 3:
            assert same(vin, spatial)                                  # the spatial route
        else:
            assert same(vin[~own], spatial[~own]) and not same(vin[own], spatial[own])
    view(R, 120.0)                                                     # a new view: the history still filters with its own features
    R.render_frame()
    R.render_features(1)
    check_filter(R, hist, mom, feat, FILTER_PARAMS[3])


def test_later_filters_are_what_they_are_without_the_feature(R):
    def sequence(on):
        load(R, "cbox")
        R.set_config(spp=2, max_depth=5)
        R.update_resolution(48, 40)
        R.set_temporal_moments(on)
        R.temporal_reset()
        for i in range(5):
            view(R, 90.0 + i)
            R.render_frame()
            R.temporal_accumulate()
        if on:
            R.denoise_temporal_variance(iterations=2)
        out = list(R.denoise_temporal(iterations=2)) + list(R.denoise_variance(iterations=2)) + list(R.variance())
        return out + list(R.denoise(iterations=1)) + list(R.read_image()) + list(R.read_temporal())
    plain, mixed = sequence(0), sequence(1)
    for a, b in zip(plain, mixed):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ------------------------------------------------------------------------------------------------
# 5. rejections
# ------------------------------------------------------------------------------------------------
def test_rejections(R):
    load(R, "cbox")
    view(R, 90.0)
    R.set_config(spp=2, max_depth=5, integrator=0)
    R.update_resolution(40, 32)
    zeros = np.zeros((32, 40), F)
    R.set_temporal_moments(0)
    R.render_frame()
    R.temporal_accumulate()
    for call in (R.temporal_moments, R.denoise_temporal_variance, lambda: R.debug_set_temporal_moments(zeros, zeros, zeros)):
        expect_error(call, "temporal moments are off")
    R.set_temporal_moments(1)
    for call in (R.temporal_moments, R.denoise_temporal_variance, lambda: R.debug_set_temporal_moments(zeros, zeros, zeros)):
        expect_error(call, "history is empty")
    R.temporal_accumulate(feature_grid=1)
    expect_error(lambda: R.denoise_temporal_variance(feature_grid=2), "feature_grid differs")
    for bad, needle in ((dict(iterations=11), "iterations"), (dict(sigma_luminance=0.0), "sigma_luminance"), (dict(epsilon=0.0), "epsilon"),
                        (dict(sigma_position=float("nan")), "sigma_position"), (dict(normal_squarings=11), "normal_squarings"),
                        (dict(feature_grid=5), "feature_grid"), (dict(demodulate=2), "demodulate"), (dict(source=2), "source"),
                        (dict(spatial_radius=4), "spatial_radius")):
        full = dict(dict(feature_grid=1), **bad)
        expect_error(lambda: R.denoise_temporal_variance(**full), needle)
        p = ptmi.default_variance_params(**full)                       # ptmi_check_variance_params's own message
        assert ptmi.lib().ptmi_check_variance_params(p) == -1
        message = ptmi.lib().ptmi_last_error().decode()
        with pytest.raises(ptmi.PtmiError) as e:
            R.denoise_temporal_variance(**full)
        assert message in str(e.value)
    assert R.L.ptmi_debug_set_temporal_moments(R.h, zeros.ctypes.data, None, zeros.ctypes.data) == -1
    expect_error(R.variance, "no current variance")                    # nothing has run since the resolution was set
    R.denoise_temporal_variance(feature_grid=1, iterations=1)
    assert all(a.shape == (32, 40) for a in R.temporal_moments())


# ------------------------------------------------------------------------------------------------
# 6. CLI
# ------------------------------------------------------------------------------------------------
def test_cli_orbit_writes_the_python_api_png(R, tmp_path):
    load(R, "cbox")
    view(R, 90.0)
    R.set_config(spp=4, max_depth=5, seed_base=2023)
    R.update_resolution(64, 48)
    R.set_temporal_moments(1)
    R.temporal_reset()
    for i in range(6):
        view(R, 90.0 + 1.0 * i)
        R.render_frame()
        R.temporal_accumulate()
        rgb, _ = R.denoise_temporal_variance(iterations=3)
    assert TM.owned(R.temporal_moments()[2]).any()
    api_png = str(tmp_path / "api.png"); cli_png = str(tmp_path / "cli.png"); sd_png = str(tmp_path / "sd.png")
    ptmi.write_png(api_png, rgb)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", CBOX, "--width", "64", "--height", "48",
                    "--spp", "4", "--max-depth", "5", "--orbit", "6", "--yaw-step", "1", "--temporal", "--denoise", "3",
                    "--variance-guided", "--variance-png", sd_png, "--out", cli_png], check=True, timeout=300)
    assert open(api_png, "rb").read() == open(cli_png, "rb").read()
    assert os.path.getsize(sd_png) > 0


# ------------------------------------------------------------------------------------------------
# 7. the expected value of the variance
# ------------------------------------------------------------------------------------------------
def test_still_camera_variance_is_unbiased(R):
    """8 injected frames of independent normal luminances (mean 1, sd 0.2): s2 x 8 / 7 is the unbiased sample variance, whose
    mean over the 627 pixels has the analytic standard error sigma^2 sqrt(2 / (7 x 627)) = 8.5e-4.  The restatement alone gives
    z = -0.22 for this seed (numpy's default_rng(1), x86-64); the GPU's numbers are the restatement's by bits."""
    w, h, n, sd = 33, 19, 8, 0.2
    x = np.random.default_rng(1).normal(1.0, sd, (n, h, w)).astype(F)
    (_, fa), _, feat, _ = constructed_views(w, h)
    load(R, "cbox")
    R.set_camera(ptmi_camera(FS.YAW_A))
    R.set_config(spp=FS.TEMPORAL_SPP, max_depth=5, integrator=0)
    R.update_resolution(w, h)
    R.set_temporal_moments(1)
    hist, mom = None, None
    prm = dict(max_history=64, sigma_position=100.0)
    for i in range(n):
        rad = np.repeat(x[i][..., None], 3, axis=2)
        R.debug_set_filter_inputs(rad, feat["a"], grid=2)
        hist, mom, st, _ = checked_step(R, hist, mom, FS.TEMPORAL_SPP, prm, rad, feat["a"], fa)
    assert st.accepted == w * h and (mom[2] == n).all()
    _, s2, k = R.temporal_moments()
    unbiased = s2.astype(np.float64) * n / (n - 1)
    se = sd * sd * np.sqrt(2.0 / ((n - 1) * w * h))
    z = (unbiased.mean() - sd * sd) / se
    print(f"variance: mean {unbiased.mean():.6f} expected {sd * sd:.6f} se {se:.2e} z {z:+.2f}")
    assert abs(z) <= Z_MAX
    R.denoise_temporal_variance(demodulate=0, iterations=0, sigma_position=FS.SIGMA_X)
    vin, vout = R.variance()
    assert np.array_equal(bits(vin), bits(np.fmax(F(0), s2 / (k - F(1))))) and np.array_equal(bits(vin), bits(vout))
    assert abs((vin.astype(np.float64).mean() * n - sd * sd) / se) <= Z_MAX


# ------------------------------------------------------------------------------------------------
# 8. quality
# ------------------------------------------------------------------------------------------------
# test_gpu_temporal.test_quality_guard's orbit: cbox 128 x 128 at 4 spp, 16 views 2 degrees apart, radiance RMSE at the last view
# against 4096 spp of seed 77; the filters at their defaults.  First measurement on an MI355X:
#   the history alone 0.2917   ptmi_denoise_temporal 0.3748   ptmi_denoise_temporal_variance 0.3350   (64 % of the pixels own
#   their variance);  new / heuristic 0.894, new / history 1.148.
# The filter that knows which pixels have converged beats the heuristic one on the same history, and still does not beat
# leaving the history alone: its bias floor (epsilon, the spatial estimate of the 36 % young pixels) is above 16 views' noise.
# The bound is the measured ratio x 1.2, QUALITY_TEMPORAL's own margin for other devices and compilers (0.54 measured, 0.65
# asserted); nothing is asserted against the history alone.
QUALITY_RATIO = 0.894 * 1.2


def test_quality_against_the_heuristic_filter(R):
    load(R, "cbox")
    view(R, 90.0 + 15 * 2.0)
    R.set_config(spp=4096, max_depth=5, seed_base=77)
    R.update_resolution(128, 128)
    R.render_frame()
    ref = R.read_image()[1].astype(np.float64)
    R.set_config(spp=4, max_depth=5, seed_base=2023)
    R.update_resolution(128, 128)
    R.set_temporal_moments(1)
    for i in range(16):
        view(R, 90.0 + 2.0 * i)
        R.render_frame()
        _, hist, _ = R.temporal_accumulate()
    _, heuristic = R.denoise_temporal()
    _, guided = R.denoise_temporal_variance()
    rmse = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - ref) ** 2)))
    owned = float(TM.owned(R.temporal_moments()[2]).mean())
    print(f"quality: history {rmse(hist):.4f} heuristic {rmse(heuristic):.4f} variance-guided {rmse(guided):.4f} "
          f"guided/heuristic {rmse(guided) / rmse(heuristic):.3f} guided/history {rmse(guided) / rmse(hist):.3f} owned {owned:.3f}")
    assert np.isfinite(guided).all()
    assert rmse(guided) / rmse(heuristic) <= QUALITY_RATIO
