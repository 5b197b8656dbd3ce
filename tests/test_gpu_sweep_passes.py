"""The sweep walk's node and triangle passes (csrc/traversal.h: intersect_sweep over the records of csrc/sweep_records.h): the cursor
is the LDS address of a node record, a miss selects the record's prepared skip lane, the hit update sits behind the (a, u) vote and
takes the slot from the record's slot lane, a leaf's primitives are read from one address.  None of it may change a bit: every
frame here is compared with the CPU oracle bit for bit - radiance, the 8-bit image and, with collect_stats, all five workload
counters (node_visits and prim_tests count the passes themselves).  No tolerance.

Each scene runs with collect_stats off AND on: those are different instantiations of the kernel, and only the first is timed.

  scenes   1, 2, 3 primitives (the root is a leaf; the smallest trees); 64 primitives (the most nodes the default sweep takes, and
           the last skip entries name the record one past the end); 300 triangles through the sweep with sweep_max_prims raised,
           still LDS-resident (node records past 4 KB, primitive records past 16 KB); triangles only (stride 3), quads only and
           mixed soups (triangle records in the stride-4 layout); both Cornell files; a camera turned away from the scene (every
           ray misses the root box: the cursor goes from the first record straight to the end)
  frames   72x56 and 70x50 (3 500 pixels: a ragged last workgroup with a partial wave), 4 spp, max_depth 1 and 8,
           segments_per_launch 1 and 32, two successive frames; a batch of 3 through render_frames (the BATCH instantiation);
           the same frames through LANE and STACK
  rays     debug_intersect - which stages and walks as the kernel does - on 3 000 rays per scene against OracleScene.intersect:
           hit, primitive and the bits of t
"""
import functools
import os

import numpy as np
import pytest

import ptmi
from oracle_binding import Camera, OracleScene, SCENES, default_camera

pytestmark = pytest.mark.gpu
F = np.float32
SPP = 4
SIZES = ((72, 56), (70, 50))
DEPTHS = (1, 8)
SEGMENTS = (1, 32)
AWAY = ((0.5, 3.0, 8.5), (0.5, 3.0, 20.0), (0.0, 1.0, 0.0), 40.0, 90.0, 0.0, 0)      # looks along +z; every scene lies at z < 4
SCENE_NAMES = ["soup1", "soup2", "soup3", "soup64", "tri64", "quad64", "quad5", "tri300", "cbox", "cbox_quads", "soup20_away"]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def soup(n, seed, quads):
    """n random primitives; quads: None mixed, False triangles only, True quads only"""
    rng = np.random.default_rng(seed)
    types = (rng.random(n) < 0.4).astype(np.int32) if quads is None else np.full(n, int(quads), np.int32)
    if quads is None and n > 1:
        types[0], types[1] = 0, 1                                # a mixed soup holds both kinds
    centers = rng.uniform(-2.5, 2.5, (n, 1, 3)) + np.array([0, 2.5, 0])
    verts = (centers + rng.normal(0, 1.5 if n < 10 else 0.6 if n < 100 else 0.3, (n, 4, 3))).astype(F)
    q = types == 1
    verts[q, 2] = verts[q, 1] + (verts[q, 3] - verts[q, 0])
    normal = rng.normal(0, 1, (n, 3)); normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    bsdf = rng.uniform(0.2, 0.9, (n, 3)); Le = rng.uniform(0, 4, (n, 3)) * (rng.random((n, 1)) < 0.3)
    Le[0] = 3.0                                                  # an emitter in every scene
    return types, verts, normal.astype(F), bsdf.astype(F), Le.astype(F)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(arrays, oracle scene, camera fields, sweep_max_prims)"""
    cam = AWAY if name.endswith("_away") else None
    base = name.split("_away")[0]
    if base.startswith("cbox"):
        p = OracleScene.load(os.path.join(SCENES, base + ".obj")).prims()
        arrs = (p["type"], p["verts"], p["normal"], p["bsdf"], p["Le"])
    else:
        kind = {"soup": None, "tri": False, "quad": True}[base.rstrip("0123456789")]
        n = int(base.lstrip("abcdefghijklmnopqrstuvwxyz"))
        arrs = soup(n, 31 * n + 5, kind)
    return arrs, OracleScene.from_arrays(*arrs), cam, max(64, len(arrs[0]))


def cameras(fields):
    if fields is None:
        return default_camera(), ptmi.default_camera()
    return Camera(*fields), ptmi.Camera(*fields)


@functools.lru_cache(maxsize=None)
def oracle_frames(name, W, H, depth, n):
    """the oracle's first n frames, streams carried over: [(rgb8, radiance, counters)], shared and read-only"""
    _, o, cam, _ = scene(name)
    state = np.zeros((H * W, 6), np.uint32)
    out = []
    for k in range(n):
        rgb, rad, st = o.render(cameras(cam)[0], W, H, SPP, max_depth=depth, rng_state=state, reset_rng=(k == 0))
        rgb.setflags(write=False); rad.setflags(write=False)
        out.append((rgb, rad, (st.samples, st.rays, st.node_visits, st.prim_tests, st.hits)))
    return out


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


def assert_frame(R, want, what, st=None):
    rgb, rad = R.read_image()
    orgb, orad, ocount = want
    nd = int((bits(rad) != bits(orad)).any(axis=-1).sum())
    assert nd == 0, f"{what}: radiance differs in {nd} pixels"
    assert np.array_equal(rgb, orgb), f"{what}: rgb8 differs in {int((rgb != orgb).any(axis=-1).sum())} pixels"
    if st is not None:
        assert (st.samples, st.rays, st.node_visits, st.prim_tests, st.hits) == ocount, what


def test_the_scenes_are_what_they_claim():
    assert [len(scene(n)[0][0]) for n in ("soup1", "soup2", "soup3", "soup64", "tri300")] == [1, 2, 3, 64, 300]
    assert not scene("tri64")[0][0].any() and scene("quad64")[0][0].all() and scene("quad5")[0][0].all()
    for n in ("soup2", "soup3", "soup64", "soup20_away"):
        t = scene(n)[0][0]
        assert t.any() and not t.all(), n
    for n in SCENE_NAMES:
        assert scene(n)[0][1][..., 2].max() < 4.0, n                       # AWAY looks along +z from z = 8.5


@pytest.mark.parametrize("stats", [False, True], ids=["timed", "stats"])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_sweep_frames_match_oracle(loaded, name, stats):
    R = loaded
    info = R.scene_info()
    if name == "tri300":                                     # record addresses past 4 KB (nodes) and 16 KB (primitives)
        assert 32 * info["n_bvh_nodes"] > 4096 and 32 * info["n_bvh_nodes"] + 48 * info["n_prims"] > 16384
    for W, H in SIZES:
        for depth in DEPTHS:
            want = oracle_frames(name, W, H, depth, 2)
            if name.endswith("_away"):
                assert all(w[2][1] == w[2][0] and w[2][4] == 0 for w in want)   # one ray per sample and no hit: the camera does look away
            for seg in SEGMENTS:
                R.update_resolution(W, H)                    # re-seeds the streams
                R.set_config(spp=SPP, max_depth=depth, segments_per_launch=seg, collect_stats=stats, sampling_mode=0)
                for k in range(2):
                    st = R.render_frame()
                    assert_frame(R, want[k], f"{name} {W}x{H} depth {depth} seg {seg} frame {k}", st if stats else None)


@pytest.mark.parametrize("stats", [False, True], ids=["timed", "stats"])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_sweep_batch_of_three(loaded, name, stats):
    R = loaded
    W, H = SIZES[1]
    for depth in DEPTHS:
        want = oracle_frames(name, W, H, depth, 3)
        for seg in SEGMENTS:
            R.update_resolution(W, H)
            R.set_config(spp=SPP, max_depth=depth, segments_per_launch=seg, collect_stats=stats, sampling_mode=0)
            st = R.render_frames(3)
            assert st.samples == W * H * SPP * 3
            if stats:
                assert (st.rays, st.node_visits, st.prim_tests, st.hits) == tuple(sum(w[2][c] for w in want) for c in (1, 2, 3, 4))
            for k in range(3):
                R.select_frame(k)
                assert_frame(R, want[k], f"{name} frame {k} of the batch, depth {depth} seg {seg}")


@pytest.mark.parametrize("walk", ["LANE", "STACK"])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_lane_and_stack_render_the_sweeps_frames(loaded, name, walk):
    R = loaded
    assert R.set_traversal(getattr(R, walk)) == getattr(R, walk)
    W, H = SIZES[1]
    for depth in DEPTHS:
        want = oracle_frames(name, W, H, depth, 2)
        for stats in (False, True):
            R.update_resolution(W, H)
            R.set_config(spp=SPP, max_depth=depth, segments_per_launch=32, collect_stats=stats, sampling_mode=0)
            for k in range(2):
                st = R.render_frame()
                assert_frame(R, want[k], f"{name} {walk} depth {depth} frame {k}", st if stats else None)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_debug_intersect_walks_the_sweeps_records(loaded, name):
    R = loaded
    arrs, o, _, _ = scene(name)
    rng = np.random.default_rng(len(arrs[0]))
    n = 3000
    org = np.where(rng.random((n, 1)) < 0.5, rng.uniform(-3, 3, (n, 3)) + np.array([0, 2.5, 0]), np.array([0.5, 3.0, 8.5])).astype(F)
    target = arrs[1][rng.integers(0, len(arrs[0]), n)].mean(axis=1) + rng.normal(0, 0.4, (n, 3))
    d = target - org
    d[:100] = np.eye(3)[rng.integers(0, 3, 100)] * rng.choice([-1.0, 1.0], (100, 1))       # axis-parallel: 1 / d by the division
    d[100:200, 1] = 0.0
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    got = R.debug_intersect(org, d)
    hit, prim, t = got["hit"], got["prim"], got["t"]
    want = [o.intersect(org[i], d[i]) for i in range(n)]
    whit = np.array([h.hit for h in want], np.int32)
    assert np.array_equal(hit != 0, whit != 0)
    on = whit != 0
    assert on.any() and not on.all()
    assert np.array_equal(prim[on], np.array([h.prim for h in want], np.int32)[on])
    assert np.array_equal(bits(t[on]), bits(np.array([h.t for h in want], F)[on]))
