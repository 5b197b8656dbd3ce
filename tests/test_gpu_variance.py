"""The variance-guided a-trous filter (include/ptmi.h: ptmi_denoise_variance) against its numpy float32 restatement
(tests/variance_oracle.py), bit for bit: the spatial variance estimate, the accumulation's moments restated from the oracle's
per-sample colours, the filter steered by either, and that nothing else moves.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ptmi
import variance_oracle as VO
from oracle_binding import OracleScene, default_camera

from test_gpu_adaptive import expected_counts, oracle_sample_colours
from test_gpu_denoise import CBOX, bits, expect_error, load, sigma_x_auto, tone_map

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 203, 77
# the adaptive run of this file: 64 x 40 pixels, 2 samples per pass, 2 .. 6 passes
AW, AH, SPP, MIN_P, MAX_P, THRESHOLD, FLOOR = 64, 40, 2, 2, 6, 0.1, 0.01


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def restated(R, rad, moments=None, **prm):
    """the restatement's (radiance, variance_in, variance_out) for the parameters denoise_variance(**prm) uses"""
    p = ptmi.default_variance_params(**prm)
    sx = p.sigma_position if p.sigma_position > 0 else sigma_x_auto(R)
    return VO.denoise_variance(rad, R.features(), p.iterations, p.sigma_luminance, p.epsilon, sx, p.normal_squarings, bool(p.demodulate),
                               p.spatial_radius, None if p.source == 1 else moments)


def assert_equals_restatement(R, rad, got, moments=None, **prm):
    drgb, drad = got
    vin, vout = R.variance()
    erad, evin, evout = restated(R, rad, moments, **prm)
    assert np.array_equal(bits(vin), bits(evin)), f"variance_in: {int((bits(vin) != bits(evin)).sum())} pixels differ"
    assert np.array_equal(bits(drad), bits(erad)), f"radiance: {int((bits(drad) != bits(erad)).any(-1).sum())} pixels differ"
    assert np.array_equal(bits(vout), bits(evout))
    assert np.array_equal(drgb, tone_map(erad))
    return erad, evin, evout


# ------------------------------------------------------------------------------------------------
# 1. the spatial source
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,width,height", [("cbox", 40, 32), ("cbox_quads", W, H), ("soup", W, H), ("soup", 5, 3)])
@pytest.mark.parametrize("iterations", [0, 1, 3, 5])
@pytest.mark.parametrize("radius", [1, 3])
def test_spatial_source_matches_numpy(R, which, width, height, iterations, radius):
    load(R, which)
    R.set_camera(ptmi.default_camera())
    R.set_config(spp=4, max_depth=5)
    R.update_resolution(width, height)
    if which == "soup":
        assert R.traversal() == ptmi.Renderer.CERTIFIED
    R.render_frame()
    rgb, rad = R.read_image()
    prm = dict(iterations=iterations, spatial_radius=radius, feature_grid=2)
    if which == "soup":
        prm.update(sigma_luminance=2.5, epsilon=1e-3, normal_squarings=3, sigma_position=0.3)
    got = R.denoise_variance(**prm)
    _, evin, evout = assert_equals_restatement(R, rad, got, **prm)
    if iterations == 0:
        assert np.array_equal(got[0], rgb) and np.array_equal(bits(got[1]), bits(rad)) and np.array_equal(bits(evin), bits(evout))
        return
    if (width, height) == (5, 3):
        return              # smaller than every window: what it checks is the clipping.  Its pixels lie further apart than sigma_x,
                            # each all but alone in its window: no variance, and nothing for either filter to do
    assert evin.max() > 0
    assert not np.array_equal(bits(got[1]), bits(rad))
    heuristic = R.denoise(iterations=iterations, feature_grid=2)[1]
    assert not np.array_equal(bits(got[1]), bits(heuristic))


@pytest.mark.parametrize("radius", [1, 3])
def test_spatial_source_matches_numpy_at_stride_512(R, radius):
    """iterations = 10 on 5 x 3: from stride 4 on every tap but the centre is outside the image"""
    test_spatial_source_matches_numpy(R, "soup", 5, 3, 10, radius)


# ------------------------------------------------------------------------------------------------
# 2. the accumulation source: the moments, then the filter on them
# ------------------------------------------------------------------------------------------------
def expected_moments(colours, spp, min_passes, max_passes, threshold, floor):
    """the loop of test_gpu_adaptive.expected_counts, returning the stopping rule's state: (mean, M2, passes)"""
    hh, ww = colours.shape[1:3]
    S = np.zeros((hh, ww, 3), F); prev = np.zeros_like(S)
    mean = np.zeros((hh, ww), F); M2 = np.zeros_like(mean)
    passes = np.zeros((hh, ww), np.uint32); active = np.ones((hh, ww), bool)
    inv_spp = F(1.0) / F(spp)
    for k in range(1, max_passes + 1):
        for j in range(spp):
            S = np.where(active[..., None], S + colours[(k - 1) * spp + j], S)
        d = S - prev
        y = (F(0.2126) * d[..., 0] + F(0.7152) * d[..., 1] + F(0.0722) * d[..., 2]) * inv_spp
        delta = y - mean
        m = mean + delta / F(k)
        m2 = M2 + delta * (y - m)
        a = F(threshold) * (m + F(floor))
        stop = (k >= max_passes) | ((k >= min_passes) & (m2 <= a * a * F(np.uint32(k * (k - 1)))))
        prev = np.where(active[..., None], S, prev)
        mean = np.where(active, m, mean); M2 = np.where(active, m2, M2)
        passes = np.where(active, np.uint32(k), passes)
        active &= ~stop
    return mean, M2, passes


_moments = {}


def adaptive_moments():
    if not _moments:
        colours = oracle_sample_colours(OracleScene.load(CBOX, 0), MAX_P * SPP, AW, AH, max_depth=5)
        _moments["v"] = expected_moments(colours, SPP, MIN_P, MAX_P, THRESHOLD, FLOOR)
        _moments["counts"] = expected_counts(colours, SPP, MIN_P, MAX_P, THRESHOLD, FLOOR)
    return _moments["v"]


def adaptive_run(R):
    load(R, "cbox")
    R.set_camera(ptmi.default_camera())
    R.set_config(spp=SPP, max_depth=5)
    R.update_resolution(AW, AH)
    R.render_adaptive(min_passes=MIN_P, max_passes=MAX_P, threshold=THRESHOLD, floor=FLOOR)
    return R.read_image()


def test_pass_moments_match_the_restated_stopping_rule(R):
    emean, em2, epasses = adaptive_moments()
    counts = _moments["counts"]                                        # test_gpu_adaptive's restatement of the stopping rule
    assert len(np.unique(counts)) >= 2, np.unique(counts)              # on the oracle, before anything else
    assert np.array_equal(counts, epasses * np.uint32(SPP))
    adaptive_run(R)
    mean, m2, passes = R.pass_moments()
    assert np.array_equal(passes, epasses) and np.array_equal(R.sample_counts(), epasses * np.uint32(SPP))
    assert np.array_equal(bits(mean), bits(emean)) and np.array_equal(bits(m2), bits(em2))
    R.set_config(wave_tiles=1)                                         # 8 x 8 slot tiles: another slot order, the same local arrays
    try:
        adaptive_run(R)
        mean, m2, passes = R.pass_moments()
        assert np.array_equal(passes, epasses) and np.array_equal(bits(mean), bits(emean)) and np.array_equal(bits(m2), bits(em2))
    finally:
        R.set_config(wave_tiles=0)


def test_accumulation_source_matches_numpy(R):
    _, em2, epasses = adaptive_moments()
    _, rad = adaptive_run(R)
    got = R.denoise_variance(iterations=3)
    _, evin, _ = assert_equals_restatement(R, rad, got, moments=(em2, epasses), iterations=3)
    # source = 1 on the same image: the spatial estimate everywhere, and another result
    spatial = R.denoise_variance(iterations=3, source=1)
    _, svin, _ = assert_equals_restatement(R, rad, spatial, iterations=3, source=1)
    assert not np.array_equal(bits(evin), bits(svin)) and not np.array_equal(bits(got[1]), bits(spatial[1]))
    # the moments under another slot order
    R.set_config(wave_tiles=1)
    try:
        _, rad8 = adaptive_run(R)
        assert np.array_equal(bits(rad8), bits(rad))
        again = R.denoise_variance(iterations=3)
        assert np.array_equal(bits(again[1]), bits(got[1])) and np.array_equal(bits(R.variance()[0]), bits(evin))
    finally:
        R.set_config(wave_tiles=0)
    # one progressive pass: no pixel has two pass means, source 0 is source 1
    R.update_resolution(AW, AH)
    R.accum_reset(); R.accum_pass(None)
    _, rad1 = R.read_image()
    auto = R.denoise_variance(iterations=2)
    vin_auto = R.variance()
    forced = R.denoise_variance(iterations=2, source=1)
    assert np.array_equal(bits(auto[1]), bits(forced[1])) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(vin_auto, R.variance()))
    assert_equals_restatement(R, rad1, forced, iterations=2, source=1)
    # a second plain pass: every pixel has k = 2 and takes the accumulation's variance
    R.accum_pass(None)
    _, rad2 = R.read_image()
    _, m2, passes = R.pass_moments()
    assert (passes == 2).all()
    assert_equals_restatement(R, rad2, R.denoise_variance(iterations=2), moments=(m2, passes), iterations=2)


# ------------------------------------------------------------------------------------------------
# 3. without demodulation, and a selected frame
# ------------------------------------------------------------------------------------------------
def test_without_demodulation_and_on_a_selected_frame(R):
    load(R, "cbox")
    R.set_camera(ptmi.default_camera())
    R.set_config(spp=4, max_depth=5)
    R.update_resolution(40, 32)
    R.render_frame()
    _, rad = R.read_image()
    prm = dict(iterations=5, demodulate=0, normal_squarings=0, sigma_position=0.5, spatial_radius=2)
    assert_equals_restatement(R, rad, R.denoise_variance(**prm), **prm)
    R.set_config(spp=2)
    R.update_resolution(40, 32)
    R.render_frames(3)
    R.select_frame(1)
    _, rad = R.read_image()
    assert_equals_restatement(R, rad, R.denoise_variance(iterations=2), iterations=2)


# ------------------------------------------------------------------------------------------------
# 4. nothing else moves
# ------------------------------------------------------------------------------------------------
def test_denoise_variance_leaves_frames_accumulations_and_denoise_alone(R):
    load(R, "cbox")
    R.set_camera(ptmi.default_camera())
    R.set_config(spp=2, max_depth=5)
    R.update_resolution(48, 40)
    R.render_frame()
    R.render_frame()
    plain = R.read_image()
    R.update_resolution(48, 40)
    R.render_frame()
    img1 = R.read_image()
    alone = R.denoise()
    R.update_resolution(48, 40)
    R.render_frame()
    R.render_features(2)
    R.denoise_variance()
    assert all(np.array_equal(a, b) for a, b in zip(R.read_image(), img1))         # the image is untouched
    after_variance = R.denoise()                                                   # ptmi_denoise gives what it gives alone
    assert np.array_equal(after_variance[0], alone[0]) and np.array_equal(bits(after_variance[1]), bits(alone[1]))
    R.denoise_variance(iterations=2)
    R.render_frame()
    after = R.read_image()
    assert np.array_equal(after[0], plain[0]) and np.array_equal(bits(after[1]), bits(plain[1]))
    # an accumulation goes on unchanged, its moments too
    R.update_resolution(48, 40)
    R.accum_reset(); R.accum_pass(None); R.accum_pass(None); R.accum_pass(None)
    acc = R.read_image(); mom = R.pass_moments()
    R.update_resolution(48, 40)
    R.accum_reset(); R.accum_pass(None); R.accum_pass(None)
    R.denoise_variance(iterations=3)
    R.denoise_variance(iterations=1, source=1)
    R.accum_pass(None)
    acc2 = R.read_image(); mom2 = R.pass_moments()
    assert np.array_equal(acc[0], acc2[0]) and np.array_equal(bits(acc[1]), bits(acc2[1]))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(mom, mom2))


# ------------------------------------------------------------------------------------------------
# 5. independent of the scheduling of the render, and of what the buffers held before
# ------------------------------------------------------------------------------------------------
def test_denoise_variance_is_independent_of_scheduling(R):
    load(R, "cbox")
    R.set_camera(ptmi.default_camera())
    R.set_config(spp=4, max_depth=5, wave_tiles=0, streams=0)
    R.update_resolution(72, 40)
    R.render_frame()
    base = R.denoise_variance(iterations=4)
    base_v = R.variance()
    try:
        for wave_tiles, streams in ((1, 1), (0, 2), (1, 3)):
            R.set_config(wave_tiles=wave_tiles, streams=streams)
            R.update_resolution(203, 77)                              # another size in between: the buffers are new
            R.render_frame()
            R.denoise_variance(iterations=1)
            R.update_resolution(72, 40)
            R.render_frame()
            got = R.denoise_variance(iterations=4)
            assert np.array_equal(got[0], base[0]) and np.array_equal(bits(got[1]), bits(base[1])), (wave_tiles, streams)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(R.variance(), base_v)), (wave_tiles, streams)
    finally:
        R.set_config(wave_tiles=0, streams=0)


# ------------------------------------------------------------------------------------------------
# 6. rejections
# ------------------------------------------------------------------------------------------------
def test_rejections(R):
    load(R, "cbox")
    R.set_camera(ptmi.default_camera())
    R.set_config(spp=2, max_depth=5, integrator=0)
    R.update_resolution(40, 32)
    expect_error(lambda: R.denoise_variance(), "no image rendered yet")
    expect_error(lambda: R.variance(), "no current variance")
    expect_error(lambda: R.pass_moments(), "no pass yet")
    R.render_frame()
    expect_error(lambda: R.pass_moments(), "no pass yet")                  # a frame is no accumulation
    for bad, needle in ((dict(iterations=11), "iterations"), (dict(iterations=-1), "iterations"), (dict(sigma_luminance=0.0), "sigma_luminance"),
                        (dict(sigma_luminance=float("nan")), "sigma_luminance"), (dict(epsilon=0.0), "epsilon"),
                        (dict(epsilon=float("nan")), "epsilon"), (dict(sigma_position=1e-9), "sigma_position"),
                        (dict(normal_squarings=11), "normal_squarings"), (dict(feature_grid=0), "feature_grid"), (dict(demodulate=2), "demodulate"),
                        (dict(source=2), "source"), (dict(spatial_radius=0), "spatial_radius"), (dict(spatial_radius=4), "spatial_radius")):
        expect_error(lambda: R.denoise_variance(**bad), needle)
    R.denoise_variance(iterations=1)
    R.variance()
    R.set_camera(ptmi.default_camera())                                    # stale, as the features are
    expect_error(lambda: R.variance(), "no current variance")
    expect_error(lambda: R.denoise_variance(), "no image rendered yet")
    R.set_config(integrator=1)
    R.render_frame()
    expect_error(lambda: R.denoise_variance(), "Radiosity integrator")
    R.set_config(integrator=0)
    R.update_resolution(40, 32, n_ranks=2, rank=0, row_block=8)
    R.render_frame()
    expect_error(lambda: R.denoise_variance(), "more than one rank")
    R.update_resolution(40, 32)


# ------------------------------------------------------------------------------------------------
# 7. CLI
# ------------------------------------------------------------------------------------------------
def test_cli_variance_guided_writes_the_python_api_png(R, tmp_path):
    load(R, "cbox")
    R.set_camera(ptmi.default_camera())
    R.set_config(spp=4, max_depth=5, seed_base=2023)
    R.update_resolution(64, 48)
    R.render_frame()
    rgb, _ = R.denoise_variance(iterations=4)
    assert not np.array_equal(rgb, R.denoise(iterations=4)[0])
    api_png = str(tmp_path / "api.png"); cli_png = str(tmp_path / "cli.png")
    ptmi.write_png(api_png, rgb)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", CBOX, "--width", "64", "--height", "48",
                    "--spp", "4", "--max-depth", "5", "--denoise", "4", "--variance-guided", "--out", cli_png,
                    "--variance-png", str(tmp_path / "sd.png")], check=True, timeout=300)
    assert open(api_png, "rb").read() == open(cli_png, "rb").read()
    assert os.path.getsize(str(tmp_path / "sd.png")) > 0


# ------------------------------------------------------------------------------------------------
# 8. quality, measured
# ------------------------------------------------------------------------------------------------
# cbox 128 x 128 against the 4096-spp frame of seed 77 (radiance RMSE), default parameters.  First measurement on an MI355X:
#   (a) a frame of 8 spp, the spatial source:               noisy 0.3677, filtered 0.2301 (ratio 0.626); ptmi_denoise on it 0.1393 (0.379)
#   (b) render_adaptive at 2 spp (17.6 spp on average), the
#       accumulation's statistics:                          noisy 0.1257, filtered 0.1164 (ratio 0.926); ptmi_denoise on it 0.1451 (1.154)
# The guards are those ratios plus the 20 % that QUALITY_RATIO of test_gpu_denoise.py took over its 0.379, capped at 1 (a filter
# that makes the image worse fails whatever was measured).  Where each filter wins and loses: DESIGN.md 4.18.
QUALITY_RATIO_SPATIAL = 0.751             # 0.626 x 1.2
QUALITY_RATIO_ACCUMULATION = 1.0          # 0.926 x 1.2 = 1.11, capped


def test_quality_guard(R):
    load(R, "cbox")
    R.set_camera(ptmi.default_camera())
    R.update_resolution(128, 128)
    R.set_config(spp=4096, max_depth=5, seed_base=77)
    R.render_frame()
    _, ref = R.read_image()
    rmse = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - ref) ** 2)))
    try:
        R.set_config(spp=8, max_depth=5, seed_base=2023)
        R.update_resolution(128, 128)
        R.render_frame()
        _, noisy = R.read_image()
        _, den = R.denoise_variance()
        _, heur = R.denoise()
        print(f"quality (a) spatial: noisy {rmse(noisy):.4f} filtered {rmse(den):.4f} ratio {rmse(den) / rmse(noisy):.3f}; "
              f"ptmi_denoise {rmse(heur):.4f} ratio {rmse(heur) / rmse(noisy):.3f}")
        assert rmse(den) < rmse(noisy)
        assert rmse(den) <= QUALITY_RATIO_SPATIAL * rmse(noisy)
        R.set_config(spp=2)
        R.update_resolution(128, 128)
        passes = R.render_adaptive(**{f: getattr(ptmi.default_adaptive_params(), f) for f in ("min_passes", "max_passes", "threshold", "floor")})
        _, noisy = R.read_image()
        _, den = R.denoise_variance()
        assert (R.pass_moments()[2] >= 2).all()                          # every pixel was steered by its own statistics
        _, heur = R.denoise()
        print(f"quality (b) accumulation: {len(passes)} passes, {R.sample_counts().mean():.1f} spp on average; noisy {rmse(noisy):.4f} "
              f"filtered {rmse(den):.4f} ratio {rmse(den) / rmse(noisy):.3f}; ptmi_denoise {rmse(heur):.4f} ratio {rmse(heur) / rmse(noisy):.3f}")
        assert rmse(den) < rmse(noisy)
        assert rmse(den) <= QUALITY_RATIO_ACCUMULATION * rmse(noisy)
    finally:
        R.set_config(spp=2, seed_base=2023)
