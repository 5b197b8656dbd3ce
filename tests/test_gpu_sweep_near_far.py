"""The sweep's node pass over the near/far records (csrc/sweep_near_far.h, csrc/traversal.h: intersect_sweep with SWEEP_NEAR_FAR):
each lane reads (near, far) of an axis at an address its ray's sign chose, where box_hit swaps two products.  The read must put the
very plane into each place that the swap would have, for every sign of 1 / d - so every comparison here is of bits, with no
tolerance: hit, primitive and t per ray against the CPU oracle, radiance and the 8-bit image per frame against the oracle and
against the LANE walk, which reads the two-vector records.

  scenes   1 triangle (the root is a leaf, a single record), 3 triangles, a 64-triangle soup (the last skip entries name the
           record one past the end), cbox.obj - built by tests/test_gpu_sweep_passes.py's scene() as tri1, tri3, tri64 and cbox.
           Triangles only: a scene with a quad runs the quad builds, which keep the two-vector records
  rays     debug_intersect, which stages and walks as the timed build does, on 32 waves of 64 rays per scene:
             8 waves with all eight sign octants mixed, lane by lane;
             16 waves of one octant each, two per octant;
             4 waves whose lanes have one or two components exactly +0 or -0 (1 / d = +-inf; -0 reads (hi, lo), +0 (lo, hi)),
               all 18 patterns in every wave;
             2 waves with a denormal component: in every lane, and in one lane only (the whole wave takes ray_inv's long form);
             2 waves with the origin on a plane of the root's box and of a leaf's, the direction's component along that axis
               +0, -0 or not zero (0 * inf in the slab test)
  frames   cbox and the 3-triangle soup at 72x56 and 70x50 (3 500 pixels: a ragged last workgroup with a partial wave), 4 spp,
           max_depth 8, collect_stats off (the builds that take the form): two successive frames and a batch of 3 against the
           oracle, then the same frames through LANE against the sweep's
"""
import numpy as np
import pytest

import ptmi
from test_gpu_sweep_passes import SIZES, SPP, assert_frame, bits, cameras, oracle_frames, scene

pytestmark = pytest.mark.gpu
F = np.float32
RAY_SCENES = ["tri1", "tri3", "tri64", "cbox"]
FRAME_SCENES = ["cbox", "tri3"]
DEPTH = 8
OCTANTS = np.array([[1.0 if (k >> a) & 1 == 0 else -1.0 for a in range(3)] for k in range(8)])
# one or two components of a direction set to a signed zero: (axis, zero) pairs
ZEROS = [((a,), (z,)) for a in range(3) for z in (0.0, -0.0)] + \
        [((a, b), (za, zb)) for a, b in ((0, 1), (0, 2), (1, 2)) for za in (0.0, -0.0) for zb in (0.0, -0.0)]


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


@pytest.fixture
def loaded(R, request):
    """the scene of the test's `name` parameter on the device, walked by the sweep"""
    name = request.node.callspec.params["name"]
    arrs, _, cam, max_prims = scene(name)
    R.load_scene_arrays(*arrs)
    R.set_camera(cameras(cam)[1])
    assert R.set_traversal(-1, sweep_max_prims=max_prims) == R.SWEEP
    yield R
    R.set_traversal(-1)
    R.set_camera(ptmi.default_camera())
    R.set_config(segments_per_launch=0, collect_stats=False)


def rays(name):
    """(origins, unit directions) of 32 waves of 64, and the lane ranges of the constructed kinds"""
    arrs = scene(name)[0]
    rng = np.random.default_rng(1000 + len(arrs[0]))
    b = ptmi.HostScene.from_arrays(*arrs).bvh()
    n = 32 * 64
    target = arrs[1][rng.integers(0, len(arrs[0]), n)][:, :3].mean(axis=1) + rng.normal(0, 0.3, (n, 3))
    d = np.abs(rng.normal(0, 1, (n, 3))) + 0.05
    octant = np.empty(n, np.int64)
    octant[:512] = rng.permuted(np.tile(np.arange(8), (8, 8)), axis=1).ravel()       # mixed: every wave holds each octant 8 times
    octant[512:1536] = np.repeat(np.arange(8), 128)                                  # one octant per wave
    octant[1536:] = rng.integers(0, 8, n - 1536)
    d *= OCTANTS[octant]
    for i in range(1536, 1792):                                                      # signed zeros
        axes, zeros = ZEROS[i % len(ZEROS)]
        d[i, list(axes)] = zeros
    tiny = np.array([1e-40, -1e-40, 3e-39, -4e-45])
    for i in list(range(1792, 1856)) + [1856 + 37]:                                  # a denormal: in every lane, in one lane
        d[i, i % 3] = tiny[i % 4]
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    org = target - d * rng.uniform(1.0, 9.0, (n, 1))
    # origins on a box plane: of the root (first wave) and of a leaf (second), direction component along that axis 0, -0 or not
    leaves = np.flatnonzero(b["count"] > 0)
    for i in range(1920, 2048):
        node = 0 if i < 1984 else int(leaves[i % len(leaves)])
        a = i % 3
        lo, hi = b["bmin"][node].astype(np.float64), b["bmax"][node].astype(np.float64)
        org[i] = lo + (hi - lo) * rng.uniform(-0.2, 1.2, 3)
        org[i, a] = (lo, hi)[(i // 3) % 2][a]
        if (i // 6) % 3 < 2:
            d[i, a] = (0.0, -0.0)[(i // 6) % 3]
            d[i] /= np.linalg.norm(d[i])
    return org.astype(F), d.astype(F)


def test_the_rays_are_what_they_claim():
    for name in RAY_SCENES:
        org, d = rays(name)
        assert org.shape == d.shape == (2048, 3)
        neg = np.signbit(d)
        code = neg[:, 0] + 2 * neg[:, 1] + 4 * neg[:, 2]
        for w in range(8):
            assert np.array_equal(np.bincount(code[64 * w:64 * w + 64], minlength=8), np.full(8, 8)), name
        for w in range(8, 24):
            assert (code[64 * w:64 * w + 64] == (w - 8) // 2).all(), name
        z = d[1536:1792]
        assert ((z == 0).sum(axis=1) >= 1).all() and ((z == 0).sum(axis=1) == 2).any()
        assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
        den = (d != 0) & (np.abs(d) < np.finfo(F).tiny)
        assert (den[1792:1856].sum(axis=1) == 1).all() and den[1856:1920].sum() == 1
        on = d[1920:]
        assert ((on == 0) & np.signbit(on)).any() and ((on == 0) & ~np.signbit(on)).any() and (on != 0).all(axis=1).any()
        assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert [len(scene(n)[0][0]) for n in ("tri1", "tri3", "tri64")] == [1, 3, 64]
    for n in RAY_SCENES + FRAME_SCENES:                      # no quad anywhere: every scene runs the builds that take the form
        assert not scene(n)[0][0].any(), n
    b = ptmi.HostScene.from_arrays(*scene("tri1")[0]).bvh()
    assert len(b["left"]) == 1 and b["count"][0] == 1        # the root is a leaf: one record


@pytest.mark.parametrize("name", RAY_SCENES)
def test_rays_match_oracle(loaded, name):
    R = loaded
    o = scene(name)[1]
    org, d = rays(name)
    got = R.debug_intersect(org, d)
    want = [o.intersect(org[i], d[i]) for i in range(len(org))]
    whit = np.array([h.hit for h in want], np.int32)
    bad = np.flatnonzero((got["hit"] != 0) != (whit != 0))
    assert bad.size == 0, f"{name}: hit differs for rays {bad[:8]}"
    on = whit != 0
    assert on.any() and not on.all()
    assert on[:1536].reshape(24, 64).any(axis=1).all()                                         # every octant wave does meet the scene
    assert np.array_equal(got["prim"][on], np.array([h.prim for h in want], np.int32)[on])
    tb = bits(got["t"][on]) != bits(np.array([h.t for h in want], F)[on])
    assert not tb.any(), f"{name}: t differs in bits for rays {np.flatnonzero(on)[tb][:8]}"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", FRAME_SCENES)
def test_frames_match_oracle_and_lane(loaded, name, size):
    R = loaded
    W, H = size
    want = oracle_frames(name, W, H, DEPTH, 3)

    def render(what):
        out = []
        R.update_resolution(W, H)                            # re-seeds the streams
        R.set_config(spp=SPP, max_depth=DEPTH, segments_per_launch=0, collect_stats=False, sampling_mode=0)
        for k in range(2):
            R.render_frame()
            assert_frame(R, want[k], f"{name} {W}x{H} {what} frame {k}")
            out.append(R.read_image())
        R.update_resolution(W, H)
        st = R.render_frames(3)
        assert st.samples == W * H * SPP * 3
        for k in range(3):
            R.select_frame(k)
            assert_frame(R, want[k], f"{name} {W}x{H} {what} frame {k} of the batch")
            out.append(R.read_image())
        return out

    swept = render("sweep")
    assert R.set_traversal(R.LANE) == R.LANE
    for k, ((rgb, rad), (lrgb, lrad)) in enumerate(zip(swept, render("LANE"))):
        assert np.array_equal(bits(rad), bits(lrad)) and np.array_equal(rgb, lrgb), f"{name} {W}x{H}: LANE and the sweep differ in image {k}"
