"""shade_step's shared direction tail (csrc/shading.h): in plain BSDF sampling the lanes that go on with their path and the lanes
that start the next sample draw, build and normalise their next direction in one pass.  Nothing may change: every frame here is
compared with the CPU oracle bit for bit - radiance and the 8-bit image, with collect_stats the five workload counters too - in
every state a pixel can be in when a launch ends.

  max_depth 1, 2, 3: every path runs into the depth limit, i.e. the two draws that are consumed and thrown away; 8 reaches
  Russian roulette (depth > 2) and its one extra draw
  segments_per_launch 1, 3, 32: a pixel crosses launch boundaries after a bounce, after the end of a sample, in mid path
  96x64 = 6 144 pixels = 24 workgroups, 70x50 = 3 500 pixels: a ragged last workgroup with a partial wave
  a second frame after the first: the streams stand where the oracle's stand - a miscounted draw shows here at the latest
"""
import functools
import os

import numpy as np
import pytest

import ptmi
from guided_fixtures import synthetic_radiosity_grids
from oracle_binding import OracleScene, SCENES, default_camera

pytestmark = pytest.mark.gpu
F = np.float32
SPP = 6
SEGMENTS = (1, 3, 32)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.set_traversal(-1)
    r.close()


@functools.lru_cache(maxsize=None)
def oracle_frames(name, sub, W, H, spp, depth, n, mode=0):
    """the oracle's first n frames (streams carried over from frame to frame): [(rgb8, radiance, stats)], shared and read-only"""
    o = OracleScene.load(os.path.join(SCENES, name), sub)
    if mode:
        grids = synthetic_radiosity_grids(o.n_prims, seed=mode)
        o.set_radiosity_grids(grids); o.set_mis_fraction(0.5)
    state = np.zeros((H * W, 6), np.uint32)
    out = []
    for k in range(n):
        rgb, rad, st = o.render(default_camera(), W, H, spp, max_depth=depth, rng_state=state, reset_rng=(k == 0), sampling_mode=mode)
        rgb.setflags(write=False); rad.setflags(write=False)
        out.append((rgb, rad, (st.samples, st.rays, st.node_visits, st.prim_tests, st.hits)))
    return out


def assert_frame(R, want, what, st=None, reference_tree=True):
    rgb, rad = R.read_image()
    orgb, orad, ocount = want
    nd = int((bits(rad) != bits(orad)).any(axis=-1).sum())
    assert nd == 0, f"{what}: radiance differs in {nd} pixels"
    assert np.array_equal(rgb, orgb), f"{what}: rgb8 differs in {int((rgb != orgb).any(axis=-1).sum())} pixels"
    if st is not None:
        if reference_tree:
            assert (st.samples, st.rays, st.node_visits, st.prim_tests, st.hits) == ocount, what
        else:                                    # the certified walk visits its own tree; samples, rays and hits are still the oracle's
            assert (st.samples, st.rays, st.hits) == (ocount[0], ocount[1], ocount[4]), what


def two_frames(R, name, sub, W, H, depth, stats, what, reference_tree=True):
    """frame 0 and frame 1 of the loaded scene against the oracle's, for every segments_per_launch"""
    want = oracle_frames(name, sub, W, H, SPP, depth, 2)
    for seg in SEGMENTS:
        R.update_resolution(W, H)                                   # re-seeds the streams
        R.set_config(spp=SPP, max_depth=depth, segments_per_launch=seg, collect_stats=stats, sampling_mode=0)
        for k in range(2):
            st = R.render_frame()
            assert_frame(R, want[k], f"{what} depth {depth} seg {seg} frame {k}", st if stats else None, reference_tree)


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("depth", [1, 2, 3, 8])
@pytest.mark.parametrize("name,W,H", [("cbox.obj", 96, 64), ("cbox.obj", 70, 50), ("cbox_quads.obj", 96, 64)])
def test_sweep_frames_and_counters_match_oracle(R, name, W, H, depth, stats):
    R.load_scene(os.path.join(SCENES, name))
    assert R.set_traversal(-1) == R.SWEEP
    try:
        two_frames(R, name, 0, W, H, depth, stats, f"{name} {W}x{H}")
    finally:
        R.set_config(segments_per_launch=0, collect_stats=False)


@pytest.mark.parametrize("depth", [2, 8])
@pytest.mark.parametrize("name,W,H", [("cbox.obj", 70, 50), ("cbox_quads.obj", 96, 64)])
def test_frame_batch_banks_each_frame(R, name, W, H, depth):
    """render_frames(3) - the batch branch of the end of a sample: the colour sum is banked and the pixel goes straight on with
    the next frame - against three render_frame calls and the oracle's three frames; a fourth frame continues the streams."""
    n = 3
    want = oracle_frames(name, 0, W, H, SPP, depth, n + 1)
    R.load_scene(os.path.join(SCENES, name))
    try:
        for seg in SEGMENTS:
            R.update_resolution(W, H)
            R.set_config(spp=SPP, max_depth=depth, segments_per_launch=seg, collect_stats=False, sampling_mode=0)
            single = []
            for k in range(n):
                R.render_frame()
                assert_frame(R, want[k], f"{name} single frame {k} seg {seg}")
                single.append(R.read_image()[1].copy())
            R.update_resolution(W, H)
            st = R.render_frames(n)
            assert st.samples == W * H * SPP * n
            for k in range(n):
                R.select_frame(k)
                assert_frame(R, want[k], f"{name} frame {k} of the batch, depth {depth} seg {seg}")
                assert np.array_equal(bits(R.read_image()[1]), bits(single[k]))
            R.render_frame()
            assert_frame(R, want[n], f"{name} frame after the batch, depth {depth} seg {seg}")
    finally:
        R.set_config(segments_per_launch=0)


@pytest.mark.parametrize("depth", [2, 8])
@pytest.mark.parametrize("walk", ["LANE", "STACK", "PHASED", "PACKED", "CERTIFIED"])
def test_other_walks_share_the_tail(R, walk, depth):
    """cbox.obj subdivided twice, 512 triangles: above the sweep's 64 primitives, so every other walk - and with it the other
    bounce kernels that call shade_step, and the vote in front of the LANE and STACK walks' 1 / d - renders the same small frames"""
    name, sub, W, H = "cbox.obj", 2, 64, 40
    R.load_scene(os.path.join(SCENES, name), sub)
    try:
        if walk == "PACKED":
            assert R.set_packed_min_nodes(16) > 0
        if walk == "CERTIFIED":
            assert R.set_traversal(-1) == R.CERTIFIED
        else:
            mode = getattr(R, walk)
            assert R.set_traversal(mode) == mode
        two_frames(R, name, sub, W, H, depth, True, f"{name}/{sub} {walk}", reference_tree=(walk != "CERTIFIED"))
    finally:
        R.set_traversal(-1); R.set_packed_min_nodes(8192)
        R.set_config(segments_per_launch=0, collect_stats=False)


def test_guided_frame_is_still_the_old_frame(R):
    """sampling_mode 3 (MIS) over CDF records: the instantiation whose end of a sample was not rewritten"""
    name, W, H, spp, depth, mode = "cbox.obj", 64, 64, 4, 5, 3
    want = oracle_frames(name, 0, W, H, spp, depth, 2, mode)
    R.load_scene(os.path.join(SCENES, name))
    R.set_radiosity_grids(synthetic_radiosity_grids(R.scene_info()["n_prims"], seed=mode))
    try:
        for seg in (0, 3):
            R.update_resolution(W, H)
            R.set_config(spp=spp, max_depth=depth, sampling_mode=mode, mis_bsdf_fraction=0.5, segments_per_launch=seg, collect_stats=True)
            for k in range(2):
                st = R.render_frame()
                assert_frame(R, want[k], f"guided seg {seg} frame {k}", st)
    finally:
        R.set_config(sampling_mode=0, segments_per_launch=0, collect_stats=False)
        R.set_radiosity_grids(None)
