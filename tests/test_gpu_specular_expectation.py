"""Specular surfaces on the GPU against analytic values (include/ptmi.h: "specular surfaces"): a mirror that shows an emitter, a
glass slab's transmission series, a black furnace with mirrors and glass inside, and the agreement of both estimators on the
Cornell box.  The z statistic, Z_MAX and FLOOR are tests/test_gpu_nee_expectation.py's; unlike the bit-exact tests of
tests/test_gpu_specular.py, these would also catch a contract that is itself wrong."""
import os

import numpy as np
import pytest

import furnace as FN
import ptmi
import ptmi_scenes
import specular_scenes as SS
from oracle_binding import SCENES
from test_gpu_nee_expectation import FLOOR, Z_MAX

pytestmark = pytest.mark.gpu

BLOCK = 16
CBOX = os.path.join(SCENES, "cbox.obj")


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def render(R, w, h, spp, depth, next_event):
    R.update_resolution(w, h)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    st = R.render_frame()
    assert st.bounce_launches == 1                            # the per-lane kernel
    return R.read_image(rgb8=False)[1].astype(np.float64)


def zstats(diff, value):
    """test_gpu_nee_expectation.zstats for a frame of any size: (mean, SE, z) of the image mean of `diff` per channel and the
    largest |z| of the BLOCK x BLOCK block means; the same floor of 2e-5 of the value on the SE"""
    h, w = diff.shape[:2]
    floor = 2e-5 * np.abs(value)
    px = diff.reshape(-1, 3)
    mean = px.mean(0)
    se = px.std(0, ddof=1) / np.sqrt(len(px))
    z = np.abs(mean) / np.maximum(se, floor)
    b = diff.reshape(h // BLOCK, BLOCK, w // BLOCK, BLOCK, 3).transpose(0, 2, 1, 3, 4).reshape(-1, BLOCK * BLOCK, 3)
    bse = b.std(1, ddof=1) / np.sqrt(BLOCK * BLOCK)
    bz = np.abs(b.mean(1)) / np.maximum(bse, floor)
    return mean, se, z, float(bz.max())


def check(tag, diff, value):
    value = np.asarray(value, np.float64)
    mean, se, z, bz = zstats(diff, value)
    print(f"{tag}: mean - value {np.array2string(mean, precision=6)}, value {np.array2string(value, precision=5)}, "
          f"SE {np.array2string(se, precision=6)}, z {np.array2string(z, precision=2)}, block |z| max {bz:.2f}")
    assert (Z_MAX * se <= FLOOR * np.abs(value)).all(), (tag, "too noisy to see a bias of 0.5 %", se, value)
    assert (z < Z_MAX).all(), (tag, mean, se, z)
    assert bz < Z_MAX, (tag, bz)


def load(R, scene, kind, cam, ior=None):
    R.load_scene_arrays(*scene.arrays())
    R.set_camera(cam)
    R.set_config(sampling_mode=0, integrator=0, fast_tree=False)
    R.set_surfaces(kind, ior)


# ------------------------------------------------------------------------------------------------
# a mirror: exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_a_mirror_shows_the_emitter_exactly(R, next_event):
    w = h = 32
    tint, le = np.array([0.5, 0.25, 1.0]), np.array([1.0, 0.75, 0.5])
    cam = ptmi.default_camera()
    scene, kind = SS.mirror_and_emitter(cam, w, h, tint, le)
    load(R, scene, kind, cam)
    rad = render(R, w, h, 8, 2, next_event)
    print("max relative deviation from tint * Le:", np.abs(rad / (tint * le) - 1.0).max())
    assert np.abs(rad / (tint * le) - 1.0).max() <= 1e-6
    deeper = render(R, w, h, 8, 6, next_event)                # the emitter is black: nothing is added later
    assert np.abs(deeper / (tint * le) - 1.0).max() <= 1e-6
    assert (render(R, w, h, 8, 1, next_event) == 0).all()


# ------------------------------------------------------------------------------------------------
# a glass slab: E (1 - F) / (1 + F), the series (1 - F)^2 sum_j F^2j of the interreflections
# ------------------------------------------------------------------------------------------------
def fresnel(theta, n=1.5):
    """the unpolarised Fresnel reflectance of an interface 1 -> n at the angle theta, binary64"""
    tt = np.arcsin(np.sin(theta) / n)
    ci, ct = np.cos(theta), np.cos(tt)
    rs = (ci - n * ct) / (ci + n * ct)
    rp = (n * ci - ct) / (n * ci + ct)
    return 0.5 * (rs * rs + rp * rp)


SLAB_W = SLAB_H = 64
SLAB_SPP = 64
SLAB_DEPTH = 12            # the series is cut after j = 4: F^10 = 1e-14 of the value (F = 0.04)


@pytest.mark.parametrize("next_event", [False, True])
def test_a_glass_slab_transmits_the_interreflection_series(R, next_event):
    """A sample is E or 0, so its standard deviation is at most E / 2 and the image mean's standard error at most
    E / (2 sqrt(64 * 64 * 64)) = 9.8e-4 E; 5 SE = 4.9e-3 E, and the measured spread (E sqrt(T (1 - T)), T = 0.923: 0.267 E) gives
    5 SE = 2.6e-3 E <= FLOOR * 0.923 E = 4.6e-3 E.  check() asserts that on the measured spread."""
    assert fresnel(0.0) == pytest.approx(0.04) and (1 - 0.04) / (1 + 0.04) == pytest.approx(0.923077, abs=1e-6)
    E = np.array([1.0, 0.75, 0.5])
    cam = ptmi.default_camera()
    cam.vfov_deg = 10.0
    scene, kind = SS.glass_slab(cam, SLAB_W, SLAB_H, E)
    load(R, scene, kind, cam, 1.5)
    Fr = fresnel(SS.pixel_angles(cam, SLAB_W, SLAB_H))
    assert 0.04 <= Fr.min() and Fr.max() < 0.0401                 # a narrow view: the slab is seen almost head-on
    expected = ((1.0 - Fr) / (1.0 + Fr))[..., None] * E
    rad = render(R, SLAB_W, SLAB_H, SLAB_SPP, SLAB_DEPTH, next_event)
    check(f"slab next_event {int(next_event)}", rad - expected, expected.reshape(-1, 3).mean(0))


# ------------------------------------------------------------------------------------------------
# the black furnace: walls of Le = E and rho = 0 around tilted mirrors and a glass cuboid - every pixel's expectation is E
# ------------------------------------------------------------------------------------------------
FURNACE_W = FURNACE_H = 64
FURNACE_SPP = 64


@pytest.mark.parametrize("quads", [False, True])
@pytest.mark.parametrize("next_event", [False, True])
def test_black_furnace(R, quads, next_event):
    """Every sample that reaches a wall before Russian roulette starts (depth <= 2: a direct view, or up to two specular
    vertices) returns exactly E; the deeper ones return E / 0.95^k or 0.  The spread is whatever the roulette makes it, and
    check() asserts 5 SE <= FLOOR * E on the measured value (64 x 64 x 64 spp measures 5 SE = 4.5e-4 E).  The share of samples
    that max_depth cuts off is <= 1e-4 (tests/specular_scenes.py: BLACK_FURNACE_DEPTH, checked on the CPU)."""
    E = np.asarray(FN.LE, np.float64)
    scene, kind = SS.black_furnace(quads=quads)
    load(R, scene, kind, ptmi.default_camera())
    rad = render(R, FURNACE_W, FURNACE_H, FURNACE_SPP, SS.BLACK_FURNACE_DEPTH, next_event)
    assert not np.isnan(rad).any()
    check(f"black furnace quads {int(quads)} next_event {int(next_event)}", rad - E, E)


# ------------------------------------------------------------------------------------------------
# both estimators on the Cornell box with a mirror block and a glass block
# ------------------------------------------------------------------------------------------------
def test_both_estimators_agree_on_the_cornell_blocks(R):
    """next_event 0 and 1 count vertices alike, so their expectations are equal pixel by pixel; the per-pixel differences are
    tested as test_gpu_nee_expectation tests NEE - reference on the tilted furnaces.  Frame size: at 128 x 128 x 1024 spp the
    standard error of the mean difference measures (3.35, 2.46, 1.64)e-4 per channel against the FLOOR * value / Z_MAX =
    (2.15, 1.85, 1.47)e-4 that check() demands (value = the image mean (0.2149, 0.1852, 0.1470)); four times the pixels halve
    it to (1.7, 1.2, 0.8)e-4, so the frame is 256 x 256 x 1024 spp."""
    w = h = 256
    R.load_scene(CBOX, 0)
    R.set_camera(ptmi.default_camera())
    R.set_config(sampling_mode=0, integrator=0, fast_tree=False)
    R.set_surfaces(ptmi_scenes.cornell_blocks(R.scene_prims()))
    ref = render(R, w, h, 1024, 8, False)
    nee = render(R, w, h, 1024, 8, True)
    assert not np.isnan(ref).any() and not np.isnan(nee).any()
    check("cornell blocks NEE - reference", nee - ref, ref.reshape(-1, 3).mean(0))


# ------------------------------------------------------------------------------------------------
# extreme emission
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_extreme_emission_through_glass_stays_free_of_nan(R, next_event):
    cam = ptmi.default_camera()
    cam.vfov_deg = 10.0
    scene, kind = SS.glass_slab(cam, 32, 32, (1e30, 1e30, 1e30))
    load(R, scene, kind, cam, 1.5)
    rad = render(R, 32, 32, 64, SLAB_DEPTH, next_event)
    assert np.isfinite(rad).all()
    assert abs(rad.mean() / (1e30 * 0.923077) - 1.0) < 0.02
