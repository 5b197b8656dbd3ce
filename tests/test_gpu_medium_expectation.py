"""The participating medium on the GPU against analytic values (include/ptmi.h: "participating medium"): an absorber in front of an
emitter, where a pixel expects Le times its average transmittance, and two furnaces - emitting walls around a medium of albedo 1,
and a constant sky over a white plane - where every pixel expects the one radiance there is, whatever the medium scatters.  Unlike
the bit-exact tests of tests/test_gpu_medium.py, these would also catch a contract that is itself biased.

Both furnaces are biased low by the share of samples max_depth cuts.  tests/medium_walk.py estimates that share on the CPU before
any GPU run, over 3 x 10^5 samples per configuration; it must be at most 1e-5 (DESIGN.md 4.24 records the estimates)."""
import numpy as np
import pytest

import furnace as FN
import medium_walk as MW
import ptmi
from test_gpu_nee_expectation import BLOCK, FLOOR, SPP, W, Z_MAX, check, zstats

pytestmark = pytest.mark.gpu

H = W
MAX_DEPTH = 64
CUT_SAMPLES = 300000
CUT_MAX = 1e-5
ROOM = ((-10.0, -10.0, -10.0), (10.0, 10.0, 10.0))            # contains the default camera (0.5, 3, 8.5)
FRONT = ((-10.0, -10.0, -10.0), (10.0, 10.0, 5.0))            # does not
SIGMA = 0.1
E_SKY = (1.0, 0.75, 0.5)
SKY_BOX = ((-3.0, 0.5, -3.0), (3.0, 4.5, 3.0))
SKY_SIGMA = 0.3


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    r.set_camera(ptmi.default_camera())
    yield r
    r.close()


def render(R, depth, next_event, spp=SPP):
    R.update_resolution(W, H)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    st = R.render_frame()
    assert st.bounce_launches == 1
    rad = R.read_image(rgb8=False)[1].astype(np.float64)
    assert not np.isnan(rad).any()
    return rad


def assert_few_cut(kind, frame, box, sigma, g):
    o, d = MW.camera_rays(frame, CUT_SAMPLES)
    cut, n = MW.cut_share(kind, o, d, box[0], box[1], sigma, g, MAX_DEPTH)
    print(f"{kind} g {g}: {cut} of {n} samples cut by max_depth {MAX_DEPTH}")
    assert n >= CUT_SAMPLES and cut / n <= CUT_MAX, (kind, g, cut, n)


# ------------------------------------------------------------------------------------------------
# the absorber
# ------------------------------------------------------------------------------------------------
ABS_LE = (1.0, 0.75, 0.5)
ABS_BOX = ((-2.0, -4.0, 2.0), (2.0, 4.0, 6.0))                # two faces perpendicular to the optical axis (z); the side faces at
ABS_SIGMA = 0.25                                               # x = +-2 cut through the view, so some columns leave through them


def absorber_scene():
    s = FN.Scene(rho=(0.0, 0.0, 0.0), le=ABS_LE)
    s.quad((-10, -10, 0), (10, -10, 0), (10, 10, 0), (-10, 10, 0))
    return s.arrays()


def absorber_camera():
    cam = ptmi.default_camera()
    cam.orbit = 0
    cam.origin[:] = (0.0, 0.0, 10.0); cam.lookat[:] = (0.0, 0.0, 0.0); cam.vup[:] = (0.0, 1.0, 0.0)
    return cam


def mean_transmittance(frame12, box, sigma, nodes=8):
    """the pixel-average of exp(-sigma l), l the binary64 length of the camera ray inside the box, by a nodes x nodes Gauss-Legendre
    rule over each pixel: (H, W), row 0 at the bottom"""
    org, llc, hor, ver = np.asarray(frame12, np.float64).reshape(4, 3)
    gx, gw = np.polynomial.legendre.leggauss(nodes)
    gx, gw = 0.5 * (gx + 1.0), 0.5 * gw
    u = (np.arange(W)[:, None] + gx[None, :]).reshape(-1) / W                     # (W * nodes,)
    v = (np.arange(H)[:, None] + gx[None, :]).reshape(-1) / H
    d = llc[None, None, :] + u[None, :, None] * hor[None, None, :] + v[:, None, None] * ver[None, None, :] - org[None, None, :]
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    lo, hi = np.asarray(box[0], np.float64), np.asarray(box[1], np.float64)
    with np.errstate(all="ignore"):
        ta, tb = (lo - org) / d, (hi - org) / d
    t0 = np.maximum(np.minimum(ta, tb).max(2), 0.0); t1 = np.maximum(ta, tb).min(2)
    T = np.exp(-sigma * np.maximum(t1 - t0, 0.0))                                 # (H * nodes, W * nodes)
    T = T.reshape(H, nodes, W, nodes)
    return np.einsum("ynxm,n,m->yx", T, gw, gw)


def binomial_z(diff, var, value):
    """|z| of the mean of diff (pixels x 3) against the binomial standard error sqrt(sum var) / n, over the siblings' floor"""
    n = diff.shape[0]
    se = np.sqrt(var.sum(0)) / n
    return np.abs(diff.mean(0)) / np.maximum(se, 2e-5 * np.abs(value)), se


@pytest.mark.parametrize("next_event", [False, True])
def test_an_absorber_dims_the_emitter_behind_it_by_its_transmittance(R, next_event):
    R.load_scene_arrays(*absorber_scene())
    R.set_camera(absorber_camera())
    R.update_resolution(W, H)
    R.set_medium(ABS_BOX[0], ABS_BOX[1], ABS_SIGMA, albedo=0.0, g=0.0)
    T = mean_transmittance(R.camera_frame(), ABS_BOX, ABS_SIGMA)
    assert 0.2 < T.min() < T.max() <= 1.0 and np.ptp(T[:, W // 2]) > 0 and np.ptp(T[H // 2]) > 0.05
    le = np.array(ABS_LE, np.float64)
    rad = render(R, 5, next_event)
    expect = T[:, :, None] * le
    diff = rad - expect
    # a sample is Le with probability T(its ray) and 0 otherwise: a pixel's mean has the variance Le^2 T (1 - T) / spp, T the pixel's average
    var = (T * (1.0 - T))[:, :, None] * le * le / SPP
    value = expect.reshape(-1, 3).mean(0)
    z, se = binomial_z(diff.reshape(-1, 3), var.reshape(-1, 3), value)
    print(f"absorber {'NEE' if next_event else 'reference'}: mean {rad.reshape(-1, 3).mean(0)}, expected {value}, SE {se}, z {z}")
    assert (Z_MAX * se <= FLOOR * value).all()
    assert (z < Z_MAX).all(), z
    blocks = lambda a: a.reshape(H // BLOCK, BLOCK, W // BLOCK, BLOCK, 3).transpose(0, 2, 1, 3, 4).reshape(-1, BLOCK * BLOCK, 3)
    bz = max(binomial_z(b, v, value)[0].max() for b, v in zip(blocks(diff), blocks(var)))
    cz = max(binomial_z(diff[:, x], var[:, x], value)[0].max() for x in range(W))
    print(f"  block |z| max {bz:.2f}, column |z| max {cz:.2f}")
    assert bz < Z_MAX and cz < Z_MAX, (bz, cz)
    R.set_camera(ptmi.default_camera())


# ------------------------------------------------------------------------------------------------
# the emitter furnace
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", [ROOM, FRONT], ids=["camera_inside", "camera_outside"])
@pytest.mark.parametrize("quads", [True, False], ids=["quads", "triangles"])
def test_emitting_walls_around_a_scattering_medium(R, quads, box):
    s = FN.box(FN.Scene(rho=(0.0, 0.0, 0.0)), quads=quads)
    R.load_scene_arrays(*s.arrays())
    R.set_camera(ptmi.default_camera())
    R.update_resolution(W, H)
    value = np.array(FN.LE, np.float64)
    for g in (0.0, 0.6):
        assert_few_cut("furnace", R.camera_frame(), box, SIGMA, g)
        R.set_medium(box[0], box[1], SIGMA, albedo=1.0, g=g)
        for nee in (False, True):
            check(f"emitter furnace {'quads' if quads else 'tris'} g {g} {'NEE' if nee else 'reference'}", render(R, MAX_DEPTH, nee) - value, value)


# ------------------------------------------------------------------------------------------------
# the sky furnace
# ------------------------------------------------------------------------------------------------
def test_a_constant_sky_over_a_white_plane(R):
    s = FN.Scene(rho=(1.0, 1.0, 1.0), le=(0.0, 0.0, 0.0))
    s.quad((-500, 0, -500), (-500, 0, 500), (500, 0, 500), (500, 0, -500))
    R.load_scene_arrays(*s.arrays())
    R.set_camera(ptmi.default_camera())
    R.update_resolution(W, H)
    R.set_environment(np.broadcast_to(np.array(E_SKY, np.float32), (4, 8, 3)).copy())
    value = np.array(E_SKY, np.float64)
    try:
        for g in (0.0, 0.6):
            assert_few_cut("sky", R.camera_frame(), SKY_BOX, SKY_SIGMA, g)
            R.set_medium(SKY_BOX[0], SKY_BOX[1], SKY_SIGMA, albedo=1.0, g=g)
            for nee in (False, True):
                check(f"sky furnace g {g} {'NEE' if nee else 'reference'}", render(R, MAX_DEPTH, nee) - value, value)
    finally:
        R.set_environment(None)
