"""Environment lighting on the GPU against analytic values, with the method and the constants of tests/test_gpu_nee_expectation.py:
128 x 128 pixels, 1024 spp, the pixel-to-pixel standard error, |z| < 5 per channel and per 16 x 16 block, and 5 SE <= 0.5 % of
the value.  Unlike the bit-exact tests of tests/test_gpu_env.py these would also catch a contract that is itself biased - a
stored pdf that is not the sampler's density, a selection probability left out of a weight."""
import numpy as np
import pytest

import env_scenes as ES
import ptmi
from test_gpu_nee_expectation import BLOCK, FLOOR, H, SPP, W, Z_MAX, check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def render(R, depth, next_event, spp=SPP):
    R.update_resolution(W, H)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    R.render_frame()
    rad = R.read_image(rgb8=False)[1].astype(np.float64)
    assert not np.isnan(rad).any()
    return rad


def check_masked(tag, rad, mask, value):
    """check() over the pixels of `mask`: per channel over all of them, per 16 x 16 block over the blocks that lie inside it"""
    value = np.asarray(value, np.float64)
    px = rad[mask] - value
    floor = 2e-5 * np.abs(value)
    mean = px.mean(0)
    se = px.std(0, ddof=1) / np.sqrt(len(px))
    z = np.abs(mean) / np.maximum(se, floor)
    whole = mask.reshape(H // BLOCK, BLOCK, W // BLOCK, BLOCK).all(axis=(1, 3))
    b = (rad - value).reshape(H // BLOCK, BLOCK, W // BLOCK, BLOCK, 3).transpose(0, 2, 1, 3, 4)[whole].reshape(-1, BLOCK * BLOCK, 3)
    bz = np.abs(b.mean(1)) / np.maximum(b.std(1, ddof=1) / np.sqrt(BLOCK * BLOCK), floor)
    print(f"{tag}: {int(mask.sum())} pixels, {len(b)} whole blocks, mean - value {np.array2string(mean, precision=6)}, "
          f"SE {np.array2string(se, precision=6)}, z {np.array2string(z, precision=2)}, block |z| max {bz.max():.2f}")
    assert len(b) >= 4
    assert (Z_MAX * se <= FLOOR * np.abs(value)).all(), (tag, "too noisy to see a bias of 0.5 %", se, value)
    assert (z < Z_MAX).all(), (tag, mean, se, z)
    assert bz.max() < Z_MAX, (tag, bz.max())


def check_interval(tag, rad, lo, hi):
    """check() for an expectation that may lie anywhere in [lo, hi]: the distance of a mean to the interval, in its SE"""
    floor = 2e-5 * np.abs(hi)
    px = rad.reshape(-1, 3)
    mean = px.mean(0)
    se = px.std(0, ddof=1) / np.sqrt(len(px))
    z = np.maximum(np.maximum(mean - hi, lo - mean), 0.0) / np.maximum(se, floor)
    b = rad.reshape(H // BLOCK, BLOCK, W // BLOCK, BLOCK, 3).transpose(0, 2, 1, 3, 4).reshape(-1, BLOCK * BLOCK, 3)
    bm = b.mean(1)
    bz = np.maximum(np.maximum(bm - hi, lo - bm), 0.0) / np.maximum(b.std(1, ddof=1) / np.sqrt(BLOCK * BLOCK), floor)
    print(f"{tag}: mean {np.array2string(mean, precision=6)} in [{np.array2string(lo, precision=6)}, {np.array2string(hi, precision=6)}], "
          f"SE {np.array2string(se, precision=6)}, z {np.array2string(z, precision=2)}, block z max {bz.max():.2f}")
    assert (Z_MAX * se <= FLOOR * np.abs(hi)).all(), (tag, "too noisy to see a bias of 0.5 %", se, hi)
    assert (z < Z_MAX).all(), (tag, mean, se, z)
    assert bz.max() < Z_MAX, (tag, bz.max())


def shrink(mask):
    """the pixels all of whose eight neighbours are in the mask too: the feature pass samples 16 points of a pixel, and a
    silhouette can cut a corner between them"""
    m = np.pad(mask, 1, constant_values=False)
    out = mask.copy()
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out &= m[dy:dy + mask.shape[0], dx:dx + mask.shape[1]]
    return out


# ------------------------------------------------------------------------------------------------
# 1. a convex body under a constant map: a cosine sample from its outside never hits it again
# ------------------------------------------------------------------------------------------------
RHO = np.array((0.3, 0.5, 0.7)); L0 = np.array((0.5, 0.4, 0.3))
E = np.array((0.875, 0.75, 0.5))                          # few mantissa bits: a pixel's sum of n x E is exact in float


def test_convex_body_under_a_constant_map(R):
    R.load_scene_arrays(*ES.cube(RHO, L0, half=2.0).arrays())
    R.set_camera(ptmi.default_camera())
    R.set_environment(ES.constant_map(E))
    R.update_resolution(W, H)
    R.set_config(spp=1, max_depth=1, next_event=False)
    R.render_features(4)
    hf = R.features()["hit_fraction"]
    hit, missed = shrink(hf == 1.0), shrink(hf == 0.0)
    assert hit.sum() > 2000 and missed.sum() > 2000
    value = L0 + RHO * E
    for depth in (1, 2, 5):
        for nee in (False, True):
            rad = render(R, depth, nee, spp=SPP if (nee and depth > 1) else 16)
            tag = f"cube depth {depth} {'NEE' if nee else 'plain'}"
            assert (rad[missed] == E.astype(np.float32)).all(), tag          # the background, exactly
            if depth == 1:                                                   # Le alone, no light sample at the last vertex
                assert np.abs(rad[hit] / L0 - 1.0).max() < 1e-6, tag
            elif not nee:                                                    # exact per sample
                assert np.abs(rad[hit] / value - 1.0).max() < 1e-6, tag
            else:
                check_masked(tag, rad, hit, value)
    R.set_environment(None)


# ------------------------------------------------------------------------------------------------
# 2. a ground quad under a sun
# ------------------------------------------------------------------------------------------------
# The sun's radiance (env_scenes.sun_radiance_for_cap; the arithmetic is spelled out in
# tests/test_env_furnace_host.py::test_the_sun_arithmetic).  Per unit albedo, sky 1, sun texel a, F_s = 0.005979 (the largest
# form factor of a 32 x 16 texel):  V = 1 + (a - 1) F_s,  Var = (1 - F_s) + a^2 F_s - V^2 per sample of the plain estimator,
# N = 128^2 x 1024.  Half the irradiance (a = 168) would make 5 SE = 0.79 % of V; 5 sqrt(Var / N) = 0.9 x 0.5 % of V gives
# a = 67 (flat) and a = 59 (tilted 35 degrees, map turned 70): the sun carries 28 % and 30 % of the irradiance.
GROUND_RHO = np.array((0.3, 0.5, 0.7))


@pytest.mark.parametrize("tilt,rot", [(0.0, 0.0), (35.0, 70.0)])
def test_ground_quad_under_a_sun(R, tilt, rot):
    env, _, v, var = ES.sun_case(tilt, rot)
    R.load_scene_arrays(*ES.ground_quad(GROUND_RHO, tilt).arrays())
    R.set_camera(ES.top_down_camera(tilt))
    R.set_environment(env, rotation_deg=rot)
    value = GROUND_RHO * v
    out = {}
    for nee in (False, True):
        rad = render(R, 5, nee)
        check(f"ground tilt {tilt} {'NEE' if nee else 'plain'}", rad - value, value)
        out[nee] = rad.reshape(-1, 3).var(0, ddof=1)
    predicted = GROUND_RHO ** 2 * var / SPP
    print(f"ground tilt {tilt}: pixel variance plain {out[False]} (closed form {predicted}), NEE {out[True]}, "
          f"ratio {out[False] / out[True]}")
    assert (np.abs(out[False] / predicted - 1.0) < 0.1).all()                # the closed-form variance of the plain estimator
    assert (out[True] < out[False]).all()
    R.set_environment(None)
    R.set_camera(ptmi.default_camera())


# ------------------------------------------------------------------------------------------------
# 3. open furnaces: the split between the emitter table and the environment
# ------------------------------------------------------------------------------------------------
F_RHO = np.array((0.3, 0.4, 0.5)); F_E = np.array((1.0, 0.75, 0.5)); DEPTH = 12


@pytest.mark.parametrize("name", ["tris_many", "quads_many"])
@pytest.mark.parametrize("q", [0.25, 0.75])
def test_open_furnace(R, name, q):
    """Kd = rho, Le = (1 - rho) E on every primitive, a constant map E: every vertex adds (1 - rho) E and passes rho on, an
    escaping path adds E, so at depth D every pixel's expectation lies in [E (1 - rho^D), E] whatever the geometry and whichever
    mix of emitter and environment samples q gives.  rho^12 <= 2.5e-4: that one-sided allowance is added to the z-test."""
    assert (F_RHO ** DEPTH <= 2.5e-4).all()
    s = ES.without_box(name)
    s.b = [tuple(F_RHO)] * len(s); s.e = [tuple((1.0 - F_RHO) * F_E)] * len(s)
    R.load_scene_arrays(*s.arrays())
    assert R.traversal() == R.CERTIFIED
    R.set_camera(ptmi.default_camera())
    R.set_environment(ES.constant_map(F_E), select_fraction=q)
    rad = render(R, DEPTH, True)
    check_interval(f"{name} q {q}", rad, F_E * (1.0 - F_RHO ** DEPTH), F_E)
    R.set_environment(None)
