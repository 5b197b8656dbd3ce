"""Vertex normals on the GPU against analytic values (include/ptmi.h: "vertex normals"): furnaces around a smooth-shaded sphere
(tests/smooth_scenes.py).  The scene is closed and every primitive a ray can reach has the same Le and Kd, so a direction sampled
about a shading normal on the wrong side of the surface - it hits the sphere from inside, or the box - finds what every other
direction finds: every pixel expects furnace.expected(depth) for both estimators, whatever the interpolated normals are.  Sizes,
depths, the z statistic, Z_MAX and FLOOR are tests/test_gpu_nee_expectation.py's; unlike the bit-exact tests of
tests/test_gpu_smooth.py these would also catch a contract that is itself biased.

Measured on the MI355X (128 x 128 x 1024 spp; DESIGN.md 4.19 has the table): the white furnace's z statistic stays below 1.9 at every
depth for both estimators (largest block |z| 3.76); the black furnaces lack 4.4e-5 of E (z 2.2 for the glass sphere, 2.25 for the
mirror): the share max_depth 32 cuts, times the 4.4 a cut sample weighs after 29 roulette steps."""
import numpy as np
import pytest

import furnace as FN
import ptmi
import smooth_scenes as SS
from test_gpu_nee_expectation import DEPTHS, H, SPP, W, check

pytestmark = pytest.mark.gpu

MIRROR, GLASS = 1, 2


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def load(R, scene, table, kind=None):
    R.load_scene_arrays(*scene.arrays())
    R.set_camera(ptmi.default_camera())
    R.set_config(sampling_mode=0, integrator=0, fast_tree=False)
    if kind is not None:
        R.set_surfaces(kind)
    R.set_vertex_normals(table)


def render(R, depth, next_event, spp=SPP):
    R.update_resolution(W, H)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    st = R.render_frame()
    assert st.bounce_launches == 1                            # the per-lane kernel
    rad = R.read_image(rgb8=False)[1].astype(np.float64)
    assert not np.isnan(rad).any()
    return rad


def sphere_share(R):
    """the share of the pixels whose centre ray hits the sphere, from the feature pass (the sphere's triangles are the scene's
    only primitives that are no walls: their feature position lies inside the box)"""
    R.update_resolution(W, H)
    R.render_features(1)
    pos = R.features()["position"]
    return float((np.abs(pos).max(2) < FN.HALF - 1.0).mean())


@pytest.mark.parametrize("quads", [False, True])
def test_white_furnace_around_a_smooth_sphere(R, quads):
    scene, table, sphere = SS.white_sphere(quads=quads)
    load(R, scene, table)
    assert R.vertex_normals_info() == dict(n_smooth=len(sphere)) and len(sphere) == 20 * 4 ** SS.SPHERE_LEVEL
    share = sphere_share(R)
    print(f"the sphere covers {share:.3f} of the pixels")
    assert share >= 0.25
    for depth in DEPTHS:
        value = FN.expected(depth)
        for nee in (False, True):
            check(f"white sphere quads {int(quads)} depth {depth} {'NEE' if nee else 'reference'}", render(R, depth, nee) - value, value)


@pytest.mark.parametrize("kind", [GLASS, MIRROR])
@pytest.mark.parametrize("next_event", [False, True])
def test_black_furnace_around_a_specular_smooth_sphere(R, kind, next_event):
    """rho = 0, Le = E walls around a glass or mirror sphere with tint 1: every path ends on a wall with throughput 1, so every
    pixel expects E.  The share of samples that max_depth cuts off is <= 1e-4 (tests/smooth_scenes.py: BLACK_FURNACE_DEPTH,
    checked on the CPU with SmoothRenderer.cut)."""
    E = np.asarray(FN.LE, np.float64)
    scene, table, kinds = SS.black_sphere(kind)
    load(R, scene, table, kinds)
    assert R.vertex_normals_info() == dict(n_smooth=20 * 4 ** SS.SPHERE_LEVEL)
    assert sphere_share(R) >= 0.25
    rad = render(R, SS.BLACK_FURNACE_DEPTH, next_event)
    check(f"black furnace kind {kind} next_event {int(next_event)}", rad - E, E)
