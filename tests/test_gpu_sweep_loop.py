"""The segment loop of ptmi_bounce<SWEEP> (csrc/bounce_sync.hip) after its restructuring: the frame block in LDS that the camera
branch reads (csrc/frame_block.h, staged by stage_scene), shade_step_sweep's late commit of the path state and the RNG's two-step
tail (csrc/shading.h, csrc/pt_device.h).  None of it may change a bit: every frame here is compared with the CPU oracle bit for bit
- radiance as uint32, the 8-bit image and, with collect_stats, samples, rays, node_visits, prim_tests and hits.  No tolerance.

Each frame runs with collect_stats off AND on: those are different instantiations, and only the first takes the new shade step (the
second still stages the block, behind the primitives, and must not notice it).

  images    1x1 (one lane), 3x5 (a partial wave), 64x1 (exactly one wave), 65x1 (a wave and a lane), 257x3 (more than a workgroup)
  scenes    cbox.obj, and one triangle (the root is a leaf; most paths leave after one bounce)
  spp       1 and 5
  max_depth 1 (no bounce), 3 (the last depth without roulette), 4 (the first with it), 8 (the depth limit's two skipped draws)
  segments_per_launch 1, 2 and 33: the state crosses a launch boundary in the middle of a sample, so what is committed late must be
            in the stored record; two successive frames, so a finished pixel's stored stream must be the one the oracle carries over
  batch     2 frames through render_frames (the BATCH instantiation) against two single frames and the oracle
  camera    one whose hor holds a -0.0 and a denormal component: the block must hand both to the kernel as they are
  sizes     a frame 2^23 + 1 rows high, of which this rank renders nine (eight from the middle, and the last): inv_height is 0 and the
            row jitter takes the IEEE division, inv_width is set and the column jitter the short one.  A frame that wide has no
            cheap oracle (one row is 8.4 M pixels), so the width's IEEE side runs through the device hook of
            test_gpu_shade_lean_forms.py::test_division_by_image_size, over the same arguments: the hook and the camera branch
            share div_by_size's four-argument form
  rays      debug_intersect, which stages through the same stage_scene (with an empty block), on 256 random rays through cbox.obj:
            hit, primitive and the bits of t
"""
import functools
import os

import numpy as np
import pytest

import ptmi
from oracle_binding import Camera, OracleScene, SCENES, default_camera

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
IMAGES = ((1, 1), (3, 5), (64, 1), (65, 1), (257, 3))
SPPS = (1, 5)
DEPTHS = (1, 3, 4, 8)
SEGMENTS = (1, 2, 33)
SCENE_NAMES = ("cbox", "tri1")
ODD_CAMERA = ((0.0, 2.5, 9.0), (1e-39, 2.5, 0.0), (0.0, 1.0, 0.0), 40.0, 0.0, 0.0, 0)       # hor = (47.3, -0.0, 5.3e-39) at 65x1
TALL = (1 << 23) + 1
TALL_CAMERA = ((0.0, 2.5, 9.0), (0.0, 2.5, 0.0), (0.0, 1.0, 0.0), 30.0, 0.0, 0.0, 0)        # the middle rows look at the back wall
LO33 = 0x2F000000                                                                             # 2^-33, the smallest curand uniform


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(arrays, oracle scene)"""
    if name == "cbox":
        p = OracleScene.load(os.path.join(SCENES, "cbox.obj")).prims()
        arrs = (p["type"], p["verts"], p["normal"], p["bsdf"], p["Le"])
    else:                                                        # one large triangle across the default camera's view, glowing
        verts = np.zeros((1, 4, 3), F)
        verts[0, :3] = [(-4.0, -1.0, -1.0), (4.5, 0.0, -1.5), (0.5, 7.0, 0.5)]
        arrs = (np.zeros(1, np.int32), verts, np.array([[0.0, 0.0, 1.0]], F), np.array([[0.7, 0.5, 0.3]], F), np.array([[0.5, 1.0, 2.0]], F))
    return arrs, OracleScene.from_arrays(*arrs)


def frame_camera(W, H):
    """camera fields for a W x H frame: the default camera, or for the wide strips one that looks into the box from the front with
    a horizontal field of 40 degrees (at the default's vertical 40 degrees nearly every pixel of a 65x1 strip looks past the scene)"""
    if W <= 2 * H:
        return None
    return ((0.0, 2.5, 9.0), (0.0, 2.5, 0.0), (0.0, 1.0, 0.0), float(np.degrees(2.0 * np.arctan(np.tan(np.radians(20.0)) * H / W))), 0.0, 0.0, 0)


def cameras(fields):
    if fields is None:
        return default_camera(), ptmi.default_camera()
    return Camera(*fields), ptmi.Camera(*fields)


@functools.lru_cache(maxsize=None)
def oracle_frames(name, W, H, spp, depth, n, cam=None):
    """the oracle's first n frames, streams carried over: [(rgb8, radiance, counters)], shared and read-only"""
    o = scene(name)[1]
    state = np.zeros((H * W, 6), U)
    out = []
    for k in range(n):
        rgb, rad, st = o.render(cameras(cam)[0], W, H, spp, max_depth=depth, rng_state=state, reset_rng=(k == 0))
        rgb.setflags(write=False); rad.setflags(write=False)
        out.append((rgb, rad, (st.samples, st.rays, st.node_visits, st.prim_tests, st.hits)))
    return out


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


@pytest.fixture
def sweep(R):
    """load(name, camera fields) puts a scene on the device, walked by the sweep"""
    def load(name, cam=None):
        R.load_scene_arrays(*scene(name)[0])
        R.set_camera(cameras(cam)[1])
        assert R.set_traversal(-1) == R.SWEEP
        return R
    yield load
    R.set_traversal(-1)
    R.set_camera(ptmi.default_camera())
    R.set_config(segments_per_launch=0, collect_stats=False)


def assert_frame(R, want, what, st=None):
    rgb, rad = R.read_image()
    orgb, orad, ocount = want
    nd = int((bits(rad) != bits(orad)).any(axis=-1).sum())
    assert nd == 0, f"{what}: radiance differs in {nd} pixels"
    assert np.array_equal(rgb, orgb), f"{what}: rgb8 differs in {int((rgb != orgb).any(axis=-1).sum())} pixels"
    if st is not None:
        assert (st.samples, st.rays, st.node_visits, st.prim_tests, st.hits) == ocount, what


def test_the_cases_are_what_they_claim():
    assert len(scene("tri1")[0][0]) == 1 and len(scene("cbox")[0][0]) <= 64
    hor = ptmi.host_camera_frame(cameras(ODD_CAMERA)[1], 65, 1)[6:9].view(U)
    assert hor[1] == 0x80000000 and 0 < hor[2] < 0x00800000                 # a -0.0 and a denormal
    rows = ptmi.host_local_row_map(TALL, 1 << 20, 1 << 19, 8)
    assert list(rows) == list(range(1 << 22, (1 << 22) + 8))
    assert list(ptmi.host_local_row_map(TALL, 1 << 20, 0, 8)) == list(range(8)) + [1 << 23]
    # the frames do see the box, and its paths go deep: some 3 segments per sample at max_depth 8, more than at 4
    for W, H in IMAGES:
        deep, mid = (oracle_frames("cbox", W, H, 5, d, 1, frame_camera(W, H))[0][2] for d in (8, 4))
        assert 2 * deep[1] > 5 * deep[0] and deep[1] > mid[1], (W, H, deep, mid)
        assert oracle_frames("tri1", W, H, 5, 8, 1, frame_camera(W, H))[0][2][4] > 0, (W, H)


@pytest.mark.parametrize("size", IMAGES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_frames_match_oracle(R, sweep, name, size):
    W, H = size
    sweep(name, frame_camera(W, H))
    for spp in SPPS:
        for depth in DEPTHS:
            want = oracle_frames(name, W, H, spp, depth, 2, frame_camera(W, H))
            for seg in SEGMENTS:
                for stats in (False, True):
                    R.update_resolution(W, H)                    # re-seeds the streams
                    R.set_config(spp=spp, max_depth=depth, segments_per_launch=seg, collect_stats=stats, sampling_mode=0)
                    for k in range(2):
                        st = R.render_frame()
                        assert_frame(R, want[k], f"{name} {W}x{H} spp {spp} depth {depth} seg {seg} stats {stats} frame {k}", st if stats else None)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_batch_of_two_is_two_single_frames(R, sweep, name):
    for W, H in ((65, 1), (257, 3)):
        sweep(name, frame_camera(W, H))
        for depth in (4, 8):
            want = oracle_frames(name, W, H, 5, depth, 2, frame_camera(W, H))
            for seg in (2, 33):
                for stats in (False, True):
                    R.update_resolution(W, H)
                    R.set_config(spp=5, max_depth=depth, segments_per_launch=seg, collect_stats=stats, sampling_mode=0)
                    single = []
                    for k in range(2):
                        R.render_frame()
                        single.append(R.read_image())
                    R.update_resolution(W, H)
                    st = R.render_frames(2)
                    assert st.samples == W * H * 5 * 2
                    if stats:
                        assert (st.rays, st.node_visits, st.prim_tests, st.hits) == tuple(sum(w[2][c] for w in want) for c in (1, 2, 3, 4))
                    for k in range(2):
                        R.select_frame(k)
                        what = f"{name} {W}x{H} depth {depth} seg {seg} stats {stats} frame {k} of the batch"
                        assert_frame(R, want[k], what)
                        rgb, rad = R.read_image()
                        assert np.array_equal(bits(rad), bits(single[k][1])) and np.array_equal(rgb, single[k][0]), what


@pytest.mark.parametrize("size", ((65, 1), (3, 5)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_signed_zero_and_denormal_in_the_camera(R, sweep, size):
    sweep("cbox", ODD_CAMERA)
    W, H = size
    for depth in (1, 8):
        want = oracle_frames("cbox", W, H, 5, depth, 2, ODD_CAMERA)
        for seg in (1, 33):
            for stats in (False, True):
                R.update_resolution(W, H)
                R.set_config(spp=5, max_depth=depth, segments_per_launch=seg, collect_stats=stats, sampling_mode=0)
                if (W, H) == (65, 1):
                    hor = R.camera_frame()[6:9].view(U)
                    assert hor[1] == 0x80000000 and 0 < hor[2] < 0x00800000
                for k in range(2):
                    st = R.render_frame()
                    assert_frame(R, want[k], f"odd camera {W}x{H} depth {depth} seg {seg} stats {stats} frame {k}", st if stats else None)


@pytest.mark.parametrize("rank", (1 << 19, 0), ids=("middle_rows", "first_and_last_rows"))
def test_a_frame_higher_than_2_23_rows(R, sweep, rank):
    sweep("cbox", TALL_CAMERA)
    W, spp, depth = 3, 5, 4
    o = scene("cbox")[1]
    spans = ((1 << 22, (1 << 22) + 8, 0),) if rank else ((0, 8, 0), (1 << 23, TALL, 8))       # (first row, one past the last, local row)
    want = []
    for y0, y1, at in spans:
        orgb, orad, ost = o.render(cameras(TALL_CAMERA)[0], W, TALL, spp, max_depth=depth, y0=y0, y1=y1)
        want.append((orgb[y0:y1].copy(), orad[y0:y1].copy(), ost.hits))
    for seg in (1, 33):
        R.update_resolution(W, TALL, n_ranks=1 << 20, rank=rank, row_block=8)
        R.set_config(spp=spp, max_depth=depth, segments_per_launch=seg, collect_stats=False, sampling_mode=0)
        rows = R.local_rows()
        assert list(rows) == (list(range(1 << 22, (1 << 22) + 8)) if rank else list(range(8)) + [1 << 23])
        R.render_frame()
        rgb, rad = R.read_image()
        assert rad.shape[:2] == (len(rows), W)
        for (y0, y1, at), (orgb, orad, hits) in zip(spans, want):
            assert np.array_equal(bits(rad[at:at + y1 - y0]), bits(orad)), (rank, seg, y0)
            assert np.array_equal(rgb[at:at + y1 - y0], orgb), (rank, seg, y0)
        if rank:
            assert want[0][2] > 0 and rad.any()                  # the middle rows see the box: the quotient reaches the radiance


def test_the_width_above_2_23_keeps_the_ieee_division(R):
    size = TALL
    bad, first, lean = R.debug_size_div_check(size, LO33, int(bits(size)[0]) - LO33 + 1)      # every float in [2^-33, W]
    assert not lean
    assert bad == 0, (bad, hex(first))
    bad, first, lean = R.debug_size_div_check(1 << 23, LO33, 1 << 20)
    assert lean and bad == 0, (bad, hex(first))


def test_intersect_hook_stages_through_the_same_function(R, sweep):
    sweep("cbox")
    arrs, o = scene("cbox")
    rng = np.random.default_rng(256)
    n = 256
    org = np.where(rng.random((n, 1)) < 0.5, rng.uniform(-2, 2, (n, 3)) + np.array([0, 2.5, 0]), np.array([0.5, 3.0, 8.5])).astype(F)
    target = arrs[1][rng.integers(0, len(arrs[0]), n)][:, :3].mean(axis=1) + rng.normal(0, 0.4, (n, 3))
    d = target - org
    d[-32:] = rng.normal(0, 0.2, (32, 3)) + np.array([0.0, 0.0, 1.0])       # out through the open front, or away from the box: no hit
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    got = R.debug_intersect(org, d)
    want = [o.intersect(org[i], d[i]) for i in range(n)]
    whit = np.array([h.hit for h in want], np.int32)
    assert np.array_equal(got["hit"] != 0, whit != 0)
    on = whit != 0
    assert on.any() and not on.all()
    assert np.array_equal(got["prim"][on], np.array([h.prim for h in want], np.int32)[on])
    assert np.array_equal(bits(got["t"][on]), bits(np.array([h.t for h in want], F)[on]))
