"""Temporal accumulation with reprojection (include/ptmi.h: ptmi_temporal_accumulate).

The step is restated in numpy float32 (tests/temporal_oracle.py) from the GPU's image, features, sample counts and camera
frames; history and output must match the GPU bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ptmi
import denoise_oracle as DO
import temporal_oracle as TO
from oracle_binding import SCENES

from test_gpu_adaptive import _soup
from test_gpu_denoise import tone_map

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CBOX = os.path.join(SCENES, "cbox.obj")
CBOX_QUADS = os.path.join(SCENES, "cbox_quads.obj")
W, H = 203, 77
# (yaw, pitch) of the orbit's views: steps of 1 and 5 degrees, a 90-degree jump, a pitch change, and a still camera
ORBIT = [(90.0, 0.0), (91.0, 0.0), (96.0, 0.0), (186.0, 0.0), (186.0, 10.0), (187.0, 10.0), (187.0, 10.0)]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def load(R, which):
    if which == "soup":
        R.load_scene_arrays(*_soup(11))
    else:
        R.load_scene(CBOX if which == "cbox" else CBOX_QUADS, 0)


def view(R, yaw, pitch=0.0):
    cam = ptmi.default_camera()
    cam.yaw_deg, cam.pitch_deg = yaw, pitch
    R.set_camera(cam)


def auto_sigma(R):
    b = R.scene_bvh()
    return TO.auto_sigma_position(b["bmin"][0], b["bmax"][0])


def checked_step(R, hist, m, prm):
    """one temporal step on the GPU and in numpy; asserts the output, the history counts and the stats; returns
    (the new numpy history, stats, radiance)"""
    _, rad = R.read_image()
    cam = R.camera_frame()
    rgb, out, st = R.temporal_accumulate(**prm)
    feat = R.features()
    p = ptmi.default_temporal_params(**prm)
    sx = p.sigma_position if p.sigma_position > 0 else auto_sigma(R)
    exp, hist, (acc, rej, mis) = TO.step(hist, rad, m, feat, cam, p.max_history, p.normal_min, sx, p.sigma_albedo)
    assert np.array_equal(bits(out), bits(exp))
    assert np.array_equal(bits(R.history_counts()), bits(hist.count))
    assert (st.accepted, st.rejected, st.missed) == (acc, rej, mis)
    assert st.accepted + st.rejected + st.missed == out.shape[0] * out.shape[1]
    return hist, st, rgb, out


# ------------------------------------------------------------------------------------------------
# 1. the step against its numpy restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cbox", "cbox_quads", "soup"])
@pytest.mark.parametrize("g", [1, 2])
def test_orbit_matches_numpy(R, which, g):
    load(R, which)
    view(R, *ORBIT[0])
    R.set_config(spp=2, max_depth=5)
    R.update_resolution(W, H)
    if which == "soup":
        assert R.traversal() == ptmi.Renderer.CERTIFIED
    prm = dict(feature_grid=g) if g == 1 else dict(feature_grid=g, max_history=3, normal_min=0.5, sigma_position=0.4, sigma_albedo=0.3)
    hist, seen = None, []
    for yaw, pitch in ORBIT:
        view(R, yaw, pitch)
        R.render_frame()
        hist, st, rgb, out = checked_step(R, hist, 2, prm)
        seen.append(st)
    assert seen[0].accepted == 0 and seen[1].accepted > 0 and seen[-1].accepted == W * H
    idx = np.random.default_rng(5).integers(0, W * H, 2000)
    assert np.array_equal(rgb.reshape(-1, 3)[idx], tone_map(out.reshape(-1, 3)[idx]))


def test_orbit_with_adaptive_passes_matches_numpy(R):
    """the input is an adaptive accumulation: m is every pixel's own count"""
    load(R, "cbox")
    R.set_config(spp=2, max_depth=5)
    R.update_resolution(W, H)
    hist, varied = None, False
    for i, (yaw, pitch) in enumerate(ORBIT[:5]):
        view(R, yaw, pitch)
        if i == 2:                                               # one plain frame in between
            R.render_frame()
            m = 2
        else:
            R.render_adaptive(min_passes=2, max_passes=8, threshold=0.1, floor=0.01)     # the runs of test_gpu_adaptive.py
            m = R.sample_counts().astype(F)
            varied |= len(np.unique(m)) > 1
        hist, _, _, _ = checked_step(R, hist, m, dict(max_history=8))
    assert varied


# ------------------------------------------------------------------------------------------------
# 2. a still camera: the running mean
# ------------------------------------------------------------------------------------------------
def test_still_camera_is_the_running_mean(R):
    load(R, "cbox")
    view(R, 90.0)
    R.set_config(spp=2, max_depth=5, seed_base=2023)
    R.update_resolution(64, 48)
    N = 8
    hist = None
    for _ in range(N):
        R.render_frame()
        hist, st, _, out = checked_step(R, hist, 2, dict(max_history=64))
    assert st.accepted == 64 * 48
    assert np.array_equal(R.history_counts(), np.full((48, 64), F(2 * N)))
    R.update_resolution(64, 48)                                   # the same streams again, as one accumulation of N passes
    R.accum_reset()
    for _ in range(N):
        R.accum_pass(None)
    _, acc = R.read_image()
    assert np.allclose(out, acc, rtol=1e-5, atol=1e-7)              # a running mean rounds differently from a sum


# ------------------------------------------------------------------------------------------------
# 3. statistics of camera motion
# ------------------------------------------------------------------------------------------------
def test_a_small_step_accepts_and_a_jump_rejects(R):
    load(R, "cbox")
    view(R, 90.0)
    R.set_config(spp=2, max_depth=5)
    R.update_resolution(128, 128)
    R.render_frame()
    _, _, st = R.temporal_accumulate()
    assert st.accepted == 0 and st.rejected + st.missed == 128 * 128
    view(R, 91.0)
    R.render_frame()
    _, _, small = R.temporal_accumulate()
    view(R, 181.0)
    R.render_frame()
    _, _, jump = R.temporal_accumulate()
    n = 128 * 128
    for s in (small, jump):
        assert s.accepted + s.rejected + s.missed == n
    hits = n - small.missed
    assert small.accepted > 0.9 * hits
    assert jump.accepted < 0.5 * (n - jump.missed)


# ------------------------------------------------------------------------------------------------
# 4. what keeps and what empties the history
# ------------------------------------------------------------------------------------------------
def test_invalidation(R):
    load(R, "cbox")
    view(R, 90.0)
    R.set_config(spp=2, max_depth=5)
    R.update_resolution(48, 40)
    R.render_frame()
    R.temporal_accumulate()
    view(R, 91.0)                                                  # the camera keeps the history
    R.render_frame()
    _, _, st = R.temporal_accumulate()
    assert st.accepted > 0 and R.history_counts().max() == 4
    emptying = [("temporal_reset", lambda: R.temporal_reset()), ("update_resolution", lambda: R.update_resolution(48, 40)),
                ("set_config", lambda: R.set_config(spp=2)), ("load_scene", lambda: load(R, "cbox")),
                ("set_radiosity", lambda: R.set_radiosity(None)), ("set_radiosity_grids", lambda: R.set_radiosity_grids(None)),
                ("run_radiosity_solver", lambda: R.run_radiosity_solver(num_iterations=1, mc_samples=4))]
    for name, change in emptying:
        R.temporal_reset()
        R.render_frame()
        R.temporal_accumulate()
        R.render_frame()
        R.temporal_accumulate()
        assert R.history_counts().max() == 4, name
        change()
        assert R.history_counts().max() == 0, name
        R.render_frame()
        _, _, st = R.temporal_accumulate()
        assert st.accepted == 0, name
        assert np.array_equal(R.history_counts(), np.full((40, 48), F(2))), name


# ------------------------------------------------------------------------------------------------
# 5. a temporal step changes nothing else
# ------------------------------------------------------------------------------------------------
def _sequence(R, temporal):
    load(R, "cbox")
    view(R, 90.0)
    R.set_config(spp=2, max_depth=5)
    R.update_resolution(48, 40)
    out = []
    def t():
        if temporal:
            R.temporal_accumulate(feature_grid=1)
            R.denoise_temporal(iterations=2, feature_grid=1)
    R.render_frame(); out += R.read_image(); t()
    view(R, 93.0)
    R.render_frame(); t(); R.render_frame(); out += R.read_image()
    out += R.denoise(iterations=3); t()
    R.accum_reset(); R.accum_pass(None); t(); R.accum_pass(None); out += R.read_image(); t()
    out += R.denoise(iterations=2); out.append(R.sample_counts())
    R.render_frame(); out += R.read_image()
    return out


def test_temporal_steps_leave_frames_passes_and_denoise_alone(R):
    plain = _sequence(R, False)
    mixed = _sequence(R, True)
    assert len(plain) == len(mixed)
    for a, b in zip(plain, mixed):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ------------------------------------------------------------------------------------------------
# 6. the result does not depend on the scheduling or the walk
# ------------------------------------------------------------------------------------------------
def _orbit3(R, mode=-1, wave_tiles=0, streams=0):
    load(R, "soup")
    view(R, 90.0)
    R.set_config(spp=2, max_depth=5, wave_tiles=wave_tiles, streams=streams)
    R.update_resolution(64, 40)
    R.set_traversal(mode)
    for yaw in (90.0, 92.0, 97.0):
        view(R, yaw)
        R.render_frame()
        _, rad, _ = R.temporal_accumulate()
    return rad, R.history_counts()


def test_independent_of_wave_tiles_streams_and_walk(R):
    base = _orbit3(R)
    for kw in (dict(wave_tiles=1, streams=1), dict(streams=3), dict(mode=1), dict(mode=6)):
        got = _orbit3(R, **kw)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(base, got)), kw
    R.set_traversal(-1)
    R.set_config(wave_tiles=0, streams=0)


# ------------------------------------------------------------------------------------------------
# 7. the filter over the history
# ------------------------------------------------------------------------------------------------
def test_denoise_temporal_matches_the_filter_of_the_history(R):
    load(R, "cbox")
    R.set_config(spp=2, max_depth=5)
    R.update_resolution(W, H)
    for yaw in (90.0, 92.0, 95.0):
        view(R, yaw)
        R.render_frame()
        _, hist, _ = R.temporal_accumulate()
    feat = R.features()                                             # the history's view's features (current, g = 2)
    drgb, drad = R.denoise_temporal(iterations=3)
    b = R.scene_bvh()
    exp = DO.denoise(hist, feat, 3, 4.0, 2.0, DO.auto_sigma_position(b["bmin"][0], b["bmax"][0]), 7)
    assert np.array_equal(bits(drad), bits(exp))
    assert np.array_equal(R.read_denoised()[0], drgb)
    view(R, 99.0)                                                   # a new view: the history still filters with its own features
    R.render_frame()
    R.render_features(1)
    _, drad2 = R.denoise_temporal(iterations=3)
    assert np.array_equal(bits(drad2), bits(exp))


# ------------------------------------------------------------------------------------------------
# 8. quality guard
# ------------------------------------------------------------------------------------------------
# cbox 128 x 128 at 4 spp, 16 views 2 degrees apart; radiance RMSE at the last view against 4096 spp of another seed.
# First measurement on an MI355X: frame 0.539, filtered 0.401, temporal 0.292 (ratio 0.54), temporal + filter 0.375 (ratio
# 0.93 of the filter alone); the first bound leaves a margin for other devices and compilers, the second asks for no more
# than a gain.
QUALITY_TEMPORAL = 0.65         # temporal / single frame
QUALITY_FILTERED = 1.0          # temporal + filter / filter alone


def test_quality_guard(R):
    load(R, "cbox")
    last = 90.0 + 15 * 2.0
    view(R, last)
    R.set_config(spp=4096, max_depth=5, seed_base=77)
    R.update_resolution(128, 128)
    R.render_frame()
    _, ref = R.read_image()
    ref = ref.astype(np.float64)
    R.set_config(spp=4, max_depth=5, seed_base=2023)
    R.update_resolution(128, 128)
    for i in range(16):
        view(R, 90.0 + 2.0 * i)
        R.render_frame()
        _, hist, _ = R.temporal_accumulate()
    _, frame = R.read_image()
    _, hist_f = R.denoise_temporal()
    _, frame_f = R.denoise()
    rmse = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - ref) ** 2)))
    print(f"quality: frame {rmse(frame):.4f} filtered {rmse(frame_f):.4f} temporal {rmse(hist):.4f} temporal+filter {rmse(hist_f):.4f}")
    assert rmse(hist) <= QUALITY_TEMPORAL * rmse(frame)
    assert rmse(hist_f) <= QUALITY_FILTERED * rmse(frame_f)


# ------------------------------------------------------------------------------------------------
# 9. rejections
# ------------------------------------------------------------------------------------------------
def expect_error(fn, needle):
    with pytest.raises(ptmi.PtmiError) as e:
        fn()
    assert e.value.code == -1 and needle in str(e.value), str(e.value)


def test_rejections(R):
    load(R, "cbox")
    view(R, 90.0)
    R.set_config(spp=2, max_depth=5, integrator=0)
    R.update_resolution(40, 32)
    expect_error(lambda: R.temporal_accumulate(), "no image rendered yet")
    expect_error(lambda: R.read_temporal(), "no temporal step yet")
    expect_error(lambda: R.denoise_temporal(), "history is empty")
    R.render_frame()
    for bad, needle in ((dict(max_history=0), "max_history"), (dict(max_history=65537), "max_history"),
                        (dict(normal_min=1.5), "normal_min"), (dict(normal_min=float("nan")), "normal_min"),
                        (dict(sigma_position=1e-9), "sigma_position"), (dict(sigma_position=float("nan")), "sigma_position"),
                        (dict(feature_grid=0), "feature_grid"), (dict(feature_grid=5), "feature_grid")):
        expect_error(lambda: R.temporal_accumulate(**bad), needle)
    expect_error(lambda: R.denoise_temporal(), "history is empty")     # a refused step leaves no history
    R.temporal_accumulate(feature_grid=1)
    expect_error(lambda: R.denoise_temporal(feature_grid=2), "feature_grid differs")
    R.denoise_temporal(feature_grid=1, iterations=1)
    view(R, 95.0)                                                     # an image older than the view
    expect_error(lambda: R.temporal_accumulate(), "no image rendered yet")
    R.set_config(integrator=1)
    R.render_frame()
    expect_error(lambda: R.temporal_accumulate(), "Radiosity integrator")
    R.set_config(integrator=0)
    R.update_resolution(40, 32, n_ranks=2, rank=0, row_block=8)
    R.render_frame()
    expect_error(lambda: R.temporal_accumulate(), "more than one rank")
    R.update_resolution(40, 32)


# ------------------------------------------------------------------------------------------------
# 10. CLI
# ------------------------------------------------------------------------------------------------
def test_cli_orbit_writes_the_python_api_png(R, tmp_path):
    load(R, "cbox")
    view(R, 90.0)
    R.set_config(spp=4, max_depth=5, seed_base=2023)
    R.update_resolution(64, 48)
    for i in range(4):
        view(R, 90.0 + 3.0 * i)
        R.render_frame()
        R.temporal_accumulate()
    rgb, _ = R.denoise_temporal(iterations=3)
    api_png = str(tmp_path / "api.png"); cli_png = str(tmp_path / "cli.png")
    ptmi.write_png(api_png, rgb)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", CBOX, "--width", "64", "--height", "48",
                    "--spp", "4", "--max-depth", "5", "--orbit", "4", "--yaw-step", "3", "--temporal", "--denoise", "3",
                    "--out", cli_png, "--out-prefix", str(tmp_path / "view_")], check=True, timeout=300)
    assert open(api_png, "rb").read() == open(cli_png, "rb").read()
    assert all(os.path.getsize(str(tmp_path / f"view_{i:03d}.png")) > 0 for i in range(4))
