"""Progressive and adaptive accumulation (include/ptmi.h: ptmi_accum_pass) against the CPU oracle, bit for bit.

A pixel's colour sum after k passes of spp samples is the sum a single frame of k * spp samples from the same stream position
forms, so every pixel must equal the oracle's fresh frame at that pixel's own sample count.  The adaptive runs are restated
independently: the oracle's frames of ONE sample with continuing streams give every sample's colour exactly (rcp_rn(1) = 1),
numpy float32 forms the running sums and the stopping rule of the header, and from them the expected count map.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ptmi
from oracle_binding import OracleScene, SCENES, default_camera

from guided_fixtures import synthetic_radiosity_grids

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CBOX = os.path.join(SCENES, "cbox.obj")
# the adaptive runs of this file: 40 x 32 pixels, 2 samples per pass, 2 .. 8 passes
W, H, SPP, MIN_P, MAX_P = 40, 32, 2, 2, 8
THRESHOLD, FLOOR = 0.1, 0.01


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def _soup(seed, n=3000):
    """triangles floating in front of the default camera, a tenth of them emitters (the certified walk: > 64 primitives)"""
    rng = np.random.default_rng(seed)
    centers = np.stack([rng.uniform(-3, 3, n), rng.uniform(0.2, 5.0, n), rng.uniform(-5.5, 0.5, n)], 1)[:, None, :]
    verts = (centers + rng.normal(0, 0.5, (n, 4, 3))).astype(F)
    normal = rng.normal(0, 1, (n, 3)); normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    bsdf = rng.uniform(0.1, 0.95, (n, 3)).astype(F)
    Le = (rng.uniform(0, 6, (n, 3)) * (rng.random((n, 1)) < 0.1)).astype(F)
    return np.zeros(n, np.int32), verts, normal.astype(F), bsdf, Le


def oracle_sample_colours(o, n, width=W, height=H, **kw):
    """(n, H, W, 3): the colour of each pixel's samples 0 .. n-1 - oracle frames of one sample with continuing streams"""
    state = np.zeros((height * width, 6), np.uint32)
    out = np.zeros((n, height, width, 3), F)
    for k in range(n):
        _, rad, _ = o.render(default_camera(), width, height, 1, rng_state=state, reset_rng=(k == 0), **kw)
        out[k] = rad
    return out


def expected_counts(colours, spp, min_passes, max_passes, threshold, floor):
    """the stopping rule of include/ptmi.h in numpy float32: samples per pixel at the end of the accumulation"""
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
    return passes * np.uint32(spp)


def assert_pixels_at_counts(rgb, rad, counts, o, what, **kw):
    """every pixel equals, in radiance bits and rgb8, the oracle's fresh frame at that pixel's count"""
    hh, ww = counts.shape
    for n in np.unique(counts):
        orgb, orad, _ = o.render(default_camera(), ww, hh, int(n), **kw)
        sel = counts == n
        bad = int((bits(rad[sel]) != bits(orad[sel])).any(axis=-1).sum())
        assert bad == 0, f"{what}: {bad} of {int(sel.sum())} pixels at {n} samples differ"
        assert (rgb[sel] == orgb[sel]).all(), f"{what}: rgb8 differs at {n} samples"


def adaptive_run(R, threshold=THRESHOLD):
    R.update_resolution(W, H)
    passes = R.render_adaptive(min_passes=MIN_P, max_passes=MAX_P, threshold=threshold, floor=FLOOR)
    rgb, rad = R.read_image()
    return passes, R.sample_counts(), rgb, rad


# ------------------------------------------------------------------------------------------------
# 1. progressive = one big frame
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sub,mode", [("cbox.obj", 0, 0), ("cbox_quads.obj", 0, 0), ("cbox.obj", 2, 0), ("cbox.obj", 2, 3)])
def test_progressive_passes_equal_one_big_frame(R, name, sub, mode):
    path = os.path.join(SCENES, name)
    R.load_scene(path, sub)
    o = OracleScene.load(path, sub)
    if mode:
        grids = synthetic_radiosity_grids(R.scene_info()["n_prims"], seed=3)
        R.set_radiosity_grids(grids); o.set_radiosity_grids(grids)
    w, h, spp, K = 48, 40, 3, 3
    try:
        R.set_config(spp=spp, max_depth=5, sampling_mode=mode, mis_bsdf_fraction=0.5)
        R.update_resolution(w, h)
        if sub == 2:
            assert R.traversal() == R.CERTIFIED
        for k in range(1, K + 1):
            st = R.accum_pass()
            assert (st.pass_, st.active_before, st.active_after, st.samples) == (k, w * h, w * h, w * h * spp)
            rgb, rad = R.read_image()
            assert (R.sample_counts() == k * spp).all()
            orgb, orad, _ = o.render(default_camera(), w, h, k * spp, max_depth=5, sampling_mode=mode)
            assert (bits(rad) == bits(orad)).all() and (rgb == orgb).all(), f"{name} sub {sub} mode {mode} pass {k}"
        # and the product's own frame of K * spp samples
        R.update_resolution(w, h)
        R.set_config(spp=K * spp)
        R.render_frame()
        frgb, frad = R.read_image()
        assert (bits(frad) == bits(rad)).all() and (frgb == rgb).all()
    finally:
        R.set_config(sampling_mode=0)
        if mode:
            R.set_radiosity_grids(None)


# ------------------------------------------------------------------------------------------------
# 2. adaptive = an independent restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["cbox", "soup"])
def test_adaptive_counts_and_pixels_match_restatement(R, scene):
    if scene == "cbox":
        R.load_scene(CBOX, 0); o = OracleScene.load(CBOX, 0)
    else:
        arrs = _soup(11)
        R.load_scene_arrays(*arrs); o = OracleScene.from_arrays(*arrs)
        assert R.traversal() == R.CERTIFIED
    R.set_config(spp=SPP, max_depth=5)
    passes, counts, rgb, rad = adaptive_run(R)
    want = expected_counts(oracle_sample_colours(o, MAX_P * SPP), SPP, MIN_P, MAX_P, THRESHOLD, FLOOR)
    assert (counts == want).all(), f"{scene}: {int((counts != want).sum())} pixels stop at another pass"
    early, full = float((want < MAX_P * SPP).mean()), float((want == MAX_P * SPP).mean())
    # the threshold leaves both kinds of pixel: >= 10 % each on the soup; the default view of cbox at this size is mostly black
    # (those pixels stop at min_passes), there both kinds must still be there
    assert (early >= 0.1 and full >= 0.1) if scene == "soup" else (early > 0.5 and full > 0.01), (early, full)
    assert passes[-1].active_after == 0 and len(passes) == int(want.max()) // SPP
    assert sum(p.samples for p in passes) == int(counts.sum())
    assert_pixels_at_counts(rgb, rad, counts, o, scene)


# ------------------------------------------------------------------------------------------------
# 3. independent of scheduling
# ------------------------------------------------------------------------------------------------
def test_adaptive_run_is_independent_of_scheduling(R):
    R.load_scene(CBOX, 2)
    R.set_config(spp=SPP, max_depth=5, segments_per_launch=0, wave_tiles=0, streams=0, collect_stats=False)
    _, counts0, rgb0, rad0 = adaptive_run(R)
    assert 0 < int((counts0 < MAX_P * SPP).sum()) < counts0.size

    def same(what):
        _, counts, rgb, rad = adaptive_run(R)
        assert (counts == counts0).all() and (bits(rad) == bits(rad0)).all() and (rgb == rgb0).all(), what
    try:
        for mode in (R.SWEEP, R.LANE, R.STACK, R.PHASED, R.PACKED, R.CERTIFIED):
            R.set_traversal(mode)
            same(f"traversal {mode}")
        R.set_traversal(-1)
        for seg in (1, 5, 0):
            R.set_config(segments_per_launch=seg)
            same(f"segments_per_launch {seg}")
        for tiles, streams in ((1, 1), (1, 2), (0, 2), (0, 1)):
            R.set_config(wave_tiles=tiles, streams=streams)
            same(f"wave_tiles {tiles} streams {streams}")
        R.set_config(wave_tiles=0, streams=0, collect_stats=True)
        same("collect_stats")
    finally:
        R.set_traversal(-1)
        R.set_config(segments_per_launch=0, wave_tiles=0, streams=0, collect_stats=False)


# ------------------------------------------------------------------------------------------------
# 4. tiles
# ------------------------------------------------------------------------------------------------
def test_adaptive_tile_union_is_the_single_gpu_run(R):
    R.load_scene(CBOX, 0)
    R.set_config(spp=SPP, max_depth=5)
    _, counts1, rgb1, rad1 = adaptive_run(R)
    for n_ranks, rb in ((2, 8), (3, 4), (4, 1)):
        rgb = np.zeros_like(rgb1); rad = np.full_like(rad1, -1); counts = np.zeros_like(counts1)
        for rank in range(n_ranks):
            R.update_resolution(W, H, n_ranks=n_ranks, rank=rank, row_block=rb)
            R.render_adaptive(min_passes=MIN_P, max_passes=MAX_P, threshold=THRESHOLD, floor=FLOOR)
            rows = R.local_rows()
            a, b = R.read_image()
            rgb[rows] = a; rad[rows] = b; counts[rows] = R.sample_counts()
        assert (counts == counts1).all() and (bits(rad) == bits(rad1)).all() and (rgb == rgb1).all(), (n_ranks, rb)


# ------------------------------------------------------------------------------------------------
# 5. state and errors
# ------------------------------------------------------------------------------------------------
def test_every_reset_trigger_restarts_the_accumulation(R):
    R.load_scene(CBOX, 0)
    R.set_config(spp=SPP, max_depth=5)
    R.update_resolution(W, H)
    n = R.scene_info()["n_prims"]
    grids = synthetic_radiosity_grids(n, seed=1)
    triggers = {
        "accum_reset": lambda: R.accum_reset(),
        "set_camera": lambda: R.set_camera(ptmi.default_camera()),
        "set_config": lambda: R.set_config(spp=SPP),
        "update_resolution": lambda: R.update_resolution(W, H),
        "load_scene": lambda: R.load_scene(CBOX, 0),
        "load_scene_arrays": lambda: R.load_scene_arrays(*_soup(2, 100)),
        "set_radiosity_grids": lambda: R.set_radiosity_grids(grids),
        "use_raw_cdfs": lambda: R.use_raw_cdfs(),
        "apply_grid_filter": lambda: R.apply_grid_filter(),
        "set_radiosity": lambda: R.set_radiosity(None),
        "run_radiosity_solver": lambda: R.run_radiosity_solver(num_iterations=1, mc_samples=4),
        "render_frame": lambda: R.render_frame(),
        "render_frames": lambda: R.render_frames(2),
    }
    for what, trigger in triggers.items():
        R.accum_reset(); R.accum_pass(); R.accum_pass()
        assert (R.sample_counts() == 2 * SPP).all(), what
        trigger()
        if what.startswith("render_frame"):
            assert (R.sample_counts() == 0).all(), what
        st = R.accum_pass()
        assert st.pass_ == 1 and (R.sample_counts() == SPP).all(), what
        if what == "load_scene_arrays":
            R.load_scene(CBOX, 0)
    # a rejected set_config is not a reset
    R.accum_pass()
    with pytest.raises(ptmi.PtmiError):
        R.set_config(spp=0)
    R.config.spp = SPP
    assert R.accum_pass().pass_ == 3


def test_frame_between_passes_continues_the_streams(R):
    R.load_scene(CBOX, 0)
    R.set_config(spp=3, max_depth=5)
    R.update_resolution(W, H)
    o = OracleScene.load(CBOX, 0)
    state = np.zeros((H * W, 6), np.uint32)
    R.accum_pass()
    o.render(default_camera(), W, H, 3, rng_state=state, reset_rng=True)
    R.render_frame()
    rgb, rad = R.read_image()
    orgb, orad, _ = o.render(default_camera(), W, H, 3, rng_state=state, reset_rng=False)
    assert (bits(rad) == bits(orad)).all() and (rgb == orgb).all()
    # and a pass after that frame: one more frame's worth of the same streams
    R.accum_pass()
    rgb, rad = R.read_image()
    orgb, orad, _ = o.render(default_camera(), W, H, 3, rng_state=state, reset_rng=False)
    assert (bits(rad) == bits(orad)).all() and (rgb == orgb).all()


def test_rejections_raise(R):
    R.load_scene(CBOX, 0)
    R.set_config(spp=SPP, max_depth=5)
    R.update_resolution(W, H)
    bad = [dict(min_passes=1), dict(min_passes=5, max_passes=4), dict(threshold=float("nan")), dict(threshold=-1.0),
           dict(floor=0.0), dict(floor=float("nan")), dict(floor=float("inf")), dict(max_passes=70000)]
    for p in bad:
        with pytest.raises(ptmi.PtmiError):
            R.accum_pass(p)
    R.set_config(spp=1 << 20)
    with pytest.raises(ptmi.PtmiError):
        R.accum_pass(dict(max_passes=16))              # 16 * 2^20 = 2^24 samples
    R.set_config(spp=SPP)
    # the Radiosity integrator
    R.set_config(integrator=1)
    with pytest.raises(ptmi.PtmiError):
        R.accum_pass()
    R.set_config(integrator=0)
    # select_frame after a pass
    R.render_frames(2)
    R.select_frame(0)
    R.accum_pass()
    with pytest.raises(ptmi.PtmiError):
        R.select_frame(0)
    # a pass after the accumulation has reached max_passes, or has finished
    R.accum_reset(); R.accum_pass(); R.accum_pass()
    with pytest.raises(ptmi.PtmiError):
        R.accum_pass(dict(min_passes=2, max_passes=2))
    R.accum_reset()
    passes = R.render_adaptive(min_passes=2, max_passes=3, threshold=1e30)
    assert len(passes) == 2 and passes[-1].active_after == 0 and (R.sample_counts() == 2 * SPP).all()
    with pytest.raises(ptmi.PtmiError):
        R.accum_pass(dict(min_passes=2, max_passes=3, threshold=1e30))
    with pytest.raises(ptmi.PtmiError):
        R.accum_pass()
    R.accum_reset()
    assert R.accum_pass().pass_ == 1


def test_pass_stats_agree_with_sample_counts(R):
    R.load_scene(CBOX, 0)
    R.set_config(spp=SPP, max_depth=5, collect_stats=True)
    try:
        passes, counts, _, _ = adaptive_run(R)
        assert sum(p.samples for p in passes) == int(counts.sum())
        assert sum(p.active_before for p in passes) * SPP == int(counts.sum())
        for k, p in enumerate(passes, 1):
            assert p.pass_ == k and p.active_before == (W * H if k == 1 else passes[k - 2].active_after)
            assert p.active_after == int((counts > k * SPP).sum())
            assert p.seconds > 0 and p.rays > 0 and p.bounce_launches > 0
    finally:
        R.set_config(collect_stats=False)


# ------------------------------------------------------------------------------------------------
# 6. CLI
# ------------------------------------------------------------------------------------------------
def test_cli_adaptive_writes_the_python_api_png(R, tmp_path):
    R.load_scene(CBOX, 0)
    R.set_camera(ptmi.default_camera())
    R.set_config(spp=SPP, max_depth=5)
    R.update_resolution(W, H)
    R.render_adaptive(min_passes=ptmi.default_adaptive_params().min_passes, max_passes=MAX_P, threshold=THRESHOLD)
    rgb, _ = R.read_image()
    api_png = str(tmp_path / "api.png"); cli_png = str(tmp_path / "cli.png")
    ptmi.write_png(api_png, rgb)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", CBOX, "--width", str(W), "--height", str(H),
                    "--spp", str(SPP), "--max-depth", "5", "--adaptive", str(THRESHOLD), "--passes", str(MAX_P), "--out", cli_png,
                    "--counts-png", str(tmp_path / "counts.png")], check=True, timeout=300)
    assert open(api_png, "rb").read() == open(cli_png, "rb").read()
    assert os.path.getsize(str(tmp_path / "counts.png")) > 0
