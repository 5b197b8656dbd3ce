"""Next-event estimation on the GPU against the analytic value of white furnaces (tests/furnace.py): closed scenes of one Le and
one Kd = rho, where every pixel's expected value is Le * (1 - rho^D) / (1 - rho) for both estimators.  Unlike the bit-exact tests
of tests/test_gpu_nee.py, these would also catch a contract that is itself biased.  Every pixel has its own RNG stream, so the
pixel-to-pixel spread gives the standard error directly."""
import numpy as np
import pytest

import furnace as FN
import ptmi

pytestmark = pytest.mark.gpu

W = H = 128
SPP = 1024
BLOCK = 16
DEPTHS = (1, 2, 3, 5, 8)
Z_MAX = 5.0
FLOOR = 0.005                 # 5 SE <= 0.5 % of the value: a test that cannot pass by being noisy


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    r.set_camera(ptmi.default_camera())
    yield r
    r.close()


def load(R, name, tmp_path):
    src, _ = FN.load_pair(name, tmp_path)
    if isinstance(src, str):
        R.load_scene(src, 0)
    else:
        R.load_scene_arrays(*src)
    R.set_camera(ptmi.default_camera())


def render(R, depth, next_event, spp=SPP):
    R.update_resolution(W, H)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    R.render_frame()
    rad = R.read_image(rgb8=False)[1].astype(np.float64)
    assert not np.isnan(rad).any()
    return rad


def zstats(diff, value):
    """(mean, SE, z) of the image mean of `diff` (pixel estimates minus the value they should average to) per channel, and the
    largest per-block |z|.  A floor of 2e-5 of the value on the SE absorbs float rounding where an estimator has no variance."""
    floor = 2e-5 * np.abs(value)
    px = diff.reshape(-1, 3)
    mean = px.mean(0)
    se = px.std(0, ddof=1) / np.sqrt(len(px))
    z = np.abs(mean) / np.maximum(se, floor)
    b = diff.reshape(H // BLOCK, BLOCK, W // BLOCK, BLOCK, 3).transpose(0, 2, 1, 3, 4).reshape(-1, BLOCK * BLOCK, 3)
    bse = b.std(1, ddof=1) / np.sqrt(BLOCK * BLOCK)
    bz = np.abs(b.mean(1)) / np.maximum(bse, floor)
    return mean, se, z, float(bz.max())


def check(tag, diff, value):
    mean, se, z, bz = zstats(diff, value)
    print(f"{tag}: mean - value {np.array2string(mean, precision=6)}, value {np.array2string(value, precision=5)}, "
          f"SE {np.array2string(se, precision=6)}, z {np.array2string(z, precision=2)}, block |z| max {bz:.2f}")
    assert (Z_MAX * se <= FLOOR * np.abs(value)).all(), (tag, "too noisy to see a bias of 0.5 %", se, value)
    assert (z < Z_MAX).all(), (tag, mean, se, z)
    assert bz < Z_MAX, (tag, bz)


WALK = {"tris_many": "CERTIFIED", "quads_many": "CERTIFIED", "emitters_4k": "CERTIFIED", "deep": "STACK", "deep_quads": "STACK"}


@pytest.mark.parametrize("name", [v for v in FN.VARIANTS if v not in FN.TILTED])
def test_both_estimators_reach_the_analytic_value(R, name, tmp_path):
    load(R, name, tmp_path)
    if name in WALK:
        assert R.traversal() == getattr(R, WALK[name]), name
    if name == "declined":
        assert R.traversal() in (R.PHASED, R.PACKED)             # the 8-wide builder declined: the reference's tree
    for depth in DEPTHS:
        value = FN.expected(depth)
        for nee in (False, True):
            check(f"{name} depth {depth} {'NEE' if nee else 'reference'}", render(R, depth, nee) - value, value)


@pytest.mark.parametrize("name", ["tilted", "tilted_mixed", "tilted_obj"])
def test_tilted_stored_normals(R, name, tmp_path):
    """Stored normals 10 - 40 degrees off the plane on every wall (all the power): the analytic value up to max_depth 2; beyond,
    the reference's estimator leaves the box after a self-hit, and NEE must equal its mean (per-pixel differences)."""
    load(R, name, tmp_path)
    for depth in DEPTHS:
        value = FN.expected(depth)
        ref, nee = render(R, depth, False), render(R, depth, True)
        if depth <= 2:
            check(f"{name} depth {depth} reference", ref - value, value)
            check(f"{name} depth {depth} NEE", nee - value, value)
        else:
            check(f"{name} depth {depth} NEE - reference", nee - ref, ref.reshape(-1, 3).mean(0))


@pytest.mark.parametrize("le", [1e30, 3e38])
def test_extreme_emission_stays_free_of_nan(R, le, tmp_path):
    """Le near float max: the emitter table stays finite (its weights overflow float), so no NaN reaches a pixel; at 1e30 the
    furnace's value is still checked"""
    s = FN.variant("tris")
    s.e = [(le, le, le)] * len(s)
    R.load_scene_arrays(*s.arrays())
    for depth in (2, 5):
        nee = render(R, depth, True, spp=64)
        if le == 1e30:
            value = FN.expected(depth, le=(le, le, le))
            assert np.isfinite(nee).all()
            mean = nee.reshape(-1, 3).mean(0)
            assert (np.abs(mean / value - 1.0) < 0.02).all(), (mean, value)
    # one emitter of 3e38 among ordinary ones, one of weight 1e-9 of the rest
    s = FN.variant("tris")
    s.e[20] = (3e38, 3e38, 3e38); s.e[21] = (1e-30, 0.0, 0.0)
    R.load_scene_arrays(*s.arrays())
    render(R, 5, True, spp=64)
