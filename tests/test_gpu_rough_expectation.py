"""Rough metal on the GPU against analytic values (include/ptmi.h: "rough metal"): the directional albedo under a constant
environment, the agreement of both estimators on the Cornell box, the approach to the mirror at the smallest roughness, and
extreme emission.  The z statistic, Z_MAX and FLOOR are tests/test_gpu_nee_expectation.py's (through
tests/test_gpu_specular_expectation.py's check, which asserts the bias and that the frame is not too noisy to see one); the
analytic values are tests/rough_oracle.py's binary64 quadratures, which tests/test_rough_host.py holds to their own error."""
import os

import numpy as np
import pytest

import env_scenes as ES
import ptmi
import rough_oracle as RO
import rough_scenes as RS
from oracle_binding import SCENES
from test_gpu_nee_expectation import FLOOR, Z_MAX
from test_gpu_specular_expectation import check, render

pytestmark = pytest.mark.gpu

CBOX = os.path.join(SCENES, "cbox.obj")
E_SKY = np.array([1.0, 0.75, 0.5])
MARGIN = 0.8                   # a frame is sized so that 5 SE is at most about 0.8 of the cap FLOOR * value


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def load(R, scene, kind, cam, roughness, env=None):
    R.load_scene_arrays(*scene.arrays())
    R.set_camera(cam)
    R.set_config(sampling_mode=0, integrator=0, fast_tree=False)
    R.set_environment(env)
    R.set_surfaces(kind, None, roughness)


# ------------------------------------------------------------------------------------------------
# 1. the directional albedo: a rough ground quad (tint 1) under a constant sky E shows E * albedo(angle of incidence)
# ------------------------------------------------------------------------------------------------
ALB_SIDE = 64
ALB_FOV = 10.0
_albedo_tables = {}


def incidence_cosines(cam, side):
    """cos of the angle between every pixel centre's ray and the ground's normal +y, (side, side), row 0 = bottom"""
    f = ptmi.host_camera_frame(cam, side, side).astype(np.float64)
    origin, llc, hor, ver = f[0:3], f[3:6], f[6:9], f[9:12]
    t = (np.arange(side) + 0.5) / side
    d = llc[None, None] + t[None, :, None] * hor + t[:, None, None] * ver - origin
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    return -d[..., 1]


def albedo_table(alpha, lo, hi):
    """the albedo on eleven angles spanning [lo, hi] (radians) by the binary64 quadrature, for linear interpolation; the midpoints
    check the interpolation to 1e-4.  Shared by both estimators' cases."""
    key = (alpha, round(lo, 6), round(hi, 6))
    if key not in _albedo_tables:
        nodes = np.linspace(lo, hi, 11)
        values = np.array([RO.albedo64(alpha, th, 750, 1500) for th in nodes])
        mids = 0.5 * (nodes[:-1] + nodes[1:])
        at_mids = np.array([RO.albedo64(alpha, th, 750, 1500) for th in mids])
        worst = np.abs(np.interp(mids, nodes, values) - at_mids).max()
        assert worst <= 1e-4, (alpha, lo, hi, worst)
        _albedo_tables[key] = (nodes, values)
    return _albedo_tables[key]


def weight_spread(alpha, theta):
    """(mean, standard deviation) of the visible-normal sample's weight at the view angle, binary64, 400 000 samples"""
    rng = np.random.default_rng(17)
    _, w = RO.sample64(alpha, RO.wo64(theta), rng.uniform(0, 1, 400_000), rng.uniform(0, 1, 400_000))
    return float(w.mean()), float(w.std())


# samples per pixel of the 64 x 64 frames, per alpha: the smallest multiple of 32 at which 5 SE of the image mean is at most
# MARGIN * FLOOR of the value for the LARGEST relative spread std / albedo over the three view angles, which tests/test_rough_host.py
# prints: 0.271 / 0.858 (60 degrees), 0.388 / 0.689 (0), 0.365 / 0.308 (0)  ->  (5 * ratio / (0.8 * 0.005))^2 / 64^2 = 38, 121, 536.  The
# reference estimator (next_event 0) has exactly that spread (a sample is E * weight).  The spread of the next_event = 1 frames is
# not known in advance; they run at the same size and check() asserts that the frame is not too noisy.
ALB_SPP = {0.25: 64, 0.5: 128, 1.0: 576}


@pytest.mark.parametrize("next_event", [False, True])
@pytest.mark.parametrize("view_deg", [0.0, 30.0, 60.0])
@pytest.mark.parametrize("alpha", [0.25, 0.5, 1.0])
def test_directional_albedo(R, alpha, view_deg, next_event):
    """E * albedo(angle of incidence) per pixel, and 0 at max_depth 1.  Measured on the MI355X (first channel, value = E * albedo):
    alpha 0.25 at 0 / 30 / 60 degrees: next_event 0 mean - value -6.0e-5 / -9.6e-5 / -2.1e-4, SE 4.8e-4 / 4.9e-4 / 5.3e-4, z 0.13 /
    0.20 / 0.39; next_event 1 SE 7.1e-4 / 7.1e-4 / 7.2e-4 (5 SE = 0.78 of the cap), z 0.07 / 0.07 / 0.38.  alpha 0.5 at 0 / 30:
    next_event 0 SE 5.4e-4 / 5.3e-4, z 0.43 / 0.55; next_event 1 SE 5.4e-4 / 5.4e-4 (0.79 of the cap), z 1.13 / 0.99.  alpha 1 at
    0 / 30: next_event 0 SE 2.4e-4 / 2.4e-4 (0.77 of the cap), z 1.86 / 1.27; next_event 1 SE 1.6e-4 / 1.7e-4, z 0.85 / 0.86.
    At 60 degrees: alpha 0.5 SE 5.0e-4 / 5.3e-4, z 0.44 / 0.81; alpha 1 SE 2.5e-4 / 2.0e-4, z 1.26 / 0.01 (next_event 0 / 1)."""
    cam = ES.top_down_camera(view_deg)
    cam.vfov_deg = ALB_FOV
    scene, kind = RS.ground()
    load(R, scene, kind, cam, float(np.sqrt(alpha)), ES.constant_map(E_SKY))
    cos_i = incidence_cosines(cam, ALB_SIDE)
    th = np.arccos(np.clip(cos_i, -1.0, 1.0))
    assert abs(th.mean() - np.radians(view_deg)) < np.radians(4.0) and th.max() - th.min() < np.radians(15.0)
    nodes, values = albedo_table(alpha, float(th.min()), float(th.max()))
    expected = np.interp(th, nodes, values)[..., None] * E_SKY
    spp = ALB_SPP[alpha]
    mean_w, std_w = weight_spread(alpha, np.radians(view_deg))
    assert 5.0 * std_w / np.sqrt(ALB_SIDE * ALB_SIDE * spp) <= MARGIN * FLOOR * mean_w * 1.02      # the sizing above, re-derived
    assert (render(R, ALB_SIDE, ALB_SIDE, 4, 1, next_event) == 0).all()                             # max_depth 1: nothing arrives
    rad = render(R, ALB_SIDE, ALB_SIDE, spp, 2, next_event)
    assert np.isfinite(rad).all()
    check(f"albedo alpha {alpha} view {view_deg} next_event {int(next_event)}", rad - expected, expected.reshape(-1, 3).mean(0))


# ------------------------------------------------------------------------------------------------
# 2. both estimators on the Cornell box with a glass block and a rough block
# ------------------------------------------------------------------------------------------------
AGREE_SIDE, AGREE_SPP = 256, 1024


def test_both_estimators_agree_on_the_cornell_box_with_a_rough_block(R):
    """next_event 0 and 1 count vertices alike, so their expectations are equal pixel by pixel: a wrong p_b, a wrong g or MIS
    weights that do not sum to 1 show here.  The size is that of the Cornell test of tests/test_gpu_specular_expectation.py.
    Measured on the MI355X: mean difference (-9.1e-5, 1.2e-5, -6.7e-6) on a mean of (0.2252, 0.1903, 0.1487), SE (1.70, 1.21,
    0.74)e-4 - 5 SE at 0.76 of the cap, so the size stands -, z (0.53, 0.10, 0.09), largest block |z| 3.38."""
    R.load_scene(CBOX, 0)
    R.set_camera(ptmi.default_camera())
    R.set_config(sampling_mode=0, integrator=0, fast_tree=False)
    R.set_environment(None)
    R.set_surfaces(RS.blocks(R.scene_prims()), None, 0.3)
    ref = render(R, AGREE_SIDE, AGREE_SIDE, AGREE_SPP, 8, False)
    nee = render(R, AGREE_SIDE, AGREE_SIDE, AGREE_SPP, 8, True)
    assert np.isfinite(ref).all() and np.isfinite(nee).all()
    check("cornell rough block NEE - reference", nee - ref, ref.reshape(-1, 3).mean(0))


# ------------------------------------------------------------------------------------------------
# 3. towards the mirror: roughness 0.05 (alpha 0.0025) at 45 degrees shows the emitter almost in full
# ------------------------------------------------------------------------------------------------
PANEL_SIDE, PANEL_SPP = 32, 64
TINT, LE = np.array([0.5, 0.25, 1.0]), np.array([1.0, 0.75, 0.5])
_panel = {}


def panel_albedo():
    """(albedo, the weight's standard deviation) at 45 degrees and alpha 0.0025: the half-vector quadrature, which shows its own
    error by a run at half the resolution, and the binary64 sampler"""
    if not _panel:
        fine = RO.albedo_half_vector64(0.0025, np.radians(45.0), 2000, 1000)
        coarse = RO.albedo_half_vector64(0.0025, np.radians(45.0), 1000, 500)
        assert abs(fine - coarse) <= 1e-4
        _panel["v"] = (fine, weight_spread(0.0025, np.radians(45.0))[1])
    return _panel["v"]


def test_roughness_at_its_smallest_approaches_the_mirror(R):
    """the reference estimator: a sample is tint * Le * weight with weight <= 1, so no pixel exceeds tint * Le, and a pixel's mean
    of PANEL_SPP samples stays within 5 standard errors of the albedo.  Measured on the MI355X: pixel / (tint Le) between 0.999992 and 0.99999994."""
    albedo, std_w = panel_albedo()
    print(f"albedo at 45 degrees, alpha 0.0025: {albedo:.6f}; weight standard deviation {std_w:.4f}")
    assert 0.99 < albedo <= 1.0
    cam = ptmi.default_camera()
    scene, kind = RS.panel_and_emitter(cam, PANEL_SIDE, PANEL_SIDE, TINT, LE)
    load(R, scene, kind, cam, 0.05)
    rad = render(R, PANEL_SIDE, PANEL_SIDE, PANEL_SPP, 2, False) / (TINT * LE)
    print(f"pixel / (tint Le): min {rad.min():.6f}, mean {rad.mean():.6f}, max {rad.max():.8f}")
    assert rad.max() <= 1.0 + 1e-5
    assert rad.min() >= albedo - 5.0 * std_w / np.sqrt(PANEL_SPP)
    assert (render(R, PANEL_SIDE, PANEL_SIDE, 4, 1, False) == 0).all()


# ------------------------------------------------------------------------------------------------
# 4. extreme emission
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_extreme_emission_in_a_rough_panel_stays_finite(R, next_event):
    albedo, _ = panel_albedo()
    cam = ptmi.default_camera()
    scene, kind = RS.panel_and_emitter(cam, PANEL_SIDE, PANEL_SIDE, TINT, (1e30, 1e30, 1e30))
    load(R, scene, kind, cam, 0.05)
    rad = render(R, PANEL_SIDE, PANEL_SIDE, PANEL_SPP, 2, next_event)
    assert np.isfinite(rad).all()
    value = rad.reshape(-1, 3).mean(0) / (TINT * 1e30)
    print(f"next_event {int(next_event)}: image mean / (tint 1e30) {value}, albedo {albedo:.6f}")
    assert np.abs(value / albedo - 1.0).max() < 0.02
