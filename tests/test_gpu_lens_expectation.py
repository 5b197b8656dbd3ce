"""The thin lens on the GPU against analytic values (include/ptmi.h: "thin lens"): the blurred image of a straight edge in front
of and behind the plane of focus (tests/lens_edge.py has the derivation), the same edge in that plane, which must stay sharp, and
a white furnace seen through the lens.  Sizes, the z statistic, Z_MAX and FLOOR are tests/test_gpu_nee_expectation.py's; unlike
the bit-exact tests of tests/test_gpu_lens.py these would also catch a contract that is itself wrong - a disc that is not
uniformly covered, a focal plane at another depth, a lens of another size."""
import numpy as np
import pytest

import furnace as FN
import lens_edge as LE
import ptmi
from test_gpu_nee_expectation import H, SPP, W, check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def render(R, depth, next_event, lens, spp=SPP, launches=1):
    R.set_lens(*lens)
    R.update_resolution(W, H)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    st = R.render_frame()
    if launches is not None:
        assert st.bounce_launches == launches
    rad = R.read_image(rgb8=False)[1].astype(np.float64)
    assert not np.isnan(rad).any()
    return rad


@pytest.mark.parametrize("quad", [True, False])
@pytest.mark.parametrize("z0", [5.0, 20.0])
def test_a_blurred_edge(R, z0, quad):
    R.load_scene_arrays(*LE.scene(z0, quad))
    R.set_camera(LE.camera())
    le = np.asarray(LE.LE, np.float64)
    for next_event in (False, True):
        tag = f"edge at z0 {z0:g} {'quad' if quad else 'triangles'} {'NEE' if next_event else 'reference'}"
        rad = render(R, 1, next_event, (LE.RADIUS, LE.FOCUS))
        prob = LE.check_edge(tag, rad, z0, SPP)
        expected = prob[None, :, None] * le[None, None, :]
        check(tag + ", the image", rad - expected, prob.mean() * le)
        assert 30 <= ((prob > 1e-3) & (prob < 1 - 1e-3)).sum() <= 40 if z0 == 5.0 else 14 <= ((prob > 1e-3) & (prob < 1 - 1e-3)).sum() <= 22
    # the test's power: the pinhole's frame of the same scene misses those values
    pin = render(R, 1, False, (0.0, None), launches=None)
    missed = (np.abs(pin.mean(0) - prob[:, None] * le[None]) > 0.05 * le[None]).all(1)
    print(f"edge at z0 {z0:g}: the pinhole misses the expected value by more than 5 % of Le in {int(missed.sum())} columns")
    assert missed.sum() >= 10
    LE.check_edge("the pinhole against its own step", pin, z0, SPP, radius=0.0)


@pytest.mark.parametrize("quad", [True, False])
def test_the_focal_plane_is_sharp(R, quad):
    """The edge in the plane of focus: every lens point sees a focal-plane point at the same (u, v), so a pixel whose footprint,
    widened by one pixel, lies wholly on one side of x = 0 is Le or 0 exactly.  Columns 63 and 64 are left out."""
    R.load_scene_arrays(*LE.scene(LE.FOCUS, quad))
    R.set_camera(LE.camera())
    le = np.asarray(LE.LE, np.float32)
    checked = np.array([(x + 2) / W <= 0.5 or (x - 1) / W >= 0.5 for x in range(W)])
    assert (~checked).sum() <= 3
    for next_event in (False, True):
        render(R, 1, next_event, (LE.RADIUS, LE.FOCUS))
        rad = R.read_image(rgb8=False)[1]                        # binary32: the comparison is exact
        lit = np.arange(W) < W // 2
        assert np.array_equal(rad[:, checked & lit], np.broadcast_to(le, rad[:, checked & lit].shape))
        assert (rad[:, checked & ~lit] == 0).all()
    R.set_lens(0.0)


@pytest.mark.parametrize("quads", [False, True])
def test_furnace_through_a_lens(R, quads):
    """furnace.box around the lens: the lens moves where a path starts and nothing else, so every pixel expects the furnace's value"""
    R.load_scene_arrays(*FN.box(FN.Scene(), quads=quads).arrays())
    R.set_camera(ptmi.default_camera())
    for depth in (2, 5, 8):
        value = FN.expected(depth)
        for nee in (False, True):
            check(f"furnace quads {int(quads)} depth {depth} {'NEE' if nee else 'reference'}", render(R, depth, nee, (0.5, None)) - value, value)
    R.set_lens(0.0)
