"""Rough metal on the GPU (include/ptmi.h: "rough metal") against the CPU restatement of the header's contract
(tests/path_oracle.py), bit for bit, and through every way a context renders: frames, batches, passes, tiles, the denoiser and
the temporal step."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_oracle as DO
import env_scenes as ES
import ptmi
import ptmi_scenes
import rough_scenes as RS
import temporal_oracle as TO
from gpu_frames import CBOX, CBOX_QUADS, ROOT, bits, check_frames, hidden_mirror, ocam, small_sky
from oracle_binding import OracleScene, default_camera
from path_oracle import RoughRenderer
from test_gpu_denoise import sigma_x_auto, tone_map

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 17, 13
SPP = 4
GLASS, ROUGH = RS.GLASS, RS.ROUGH


@pytest.fixture()
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def configure(R, depth, next_event, w=W, h=H, spp=SPP, cam=None):
    R.set_camera(cam if cam is not None else ptmi.default_camera())
    R.update_resolution(w, h)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)


def cornell(R, which, depth, next_event, w=W, h=H, spp=SPP, roughness=0.3, env=None):
    """cbox / cbox_quads with the tall block rough and the short block glass: (the oracle's copy, kind)"""
    path = CBOX if which == "cbox" else CBOX_QUADS
    R.load_scene(path, 0)
    kind = RS.blocks(R.scene_prims())
    configure(R, depth, next_event, w, h, spp)
    if env is not None:
        R.set_environment(env)
    R.set_surfaces(kind, None, roughness)
    return OracleScene.load(path), kind


def arrays_scene(R, arrays, kind, roughness, depth, next_event, w=W, h=H, spp=SPP, cam=None, env=None):
    R.load_scene_arrays(*arrays)
    configure(R, depth, next_event, w, h, spp, cam)
    if env is not None:
        R.set_environment(env)
    R.set_surfaces(kind, None, roughness)
    return OracleScene.from_arrays(*arrays)


def reference(o, kind, next_event, w=W, h=H, roughness=0.3, env=None, cam=None):
    return RoughRenderer(o, default_camera() if cam is None else ocam(cam), w, h, kind, None, roughness, env, next_event)


# ------------------------------------------------------------------------------------------------
# bit for bit against the restatement, first and second frame (the streams carry over)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sky", [False, True])
@pytest.mark.parametrize("next_event", [False, True])
@pytest.mark.parametrize("depth", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("which", ["cbox", "cbox_quads"])
def test_cornell_rough_block_17x13(R, which, depth, next_event, sky):
    env = small_sky() if sky else None
    o, kind = cornell(R, which, depth, next_event, env=env)
    n_block = int((kind == ROUGH).sum())
    assert n_block in (5, 10) and R.surface_counts() == [len(kind) - 2 * n_block, 0, n_block, n_block]
    assert R.surfaces_info() == dict(n_mirror=0, n_glass=n_block)
    _, rad, _ = check_frames(R, reference(o, kind, next_event, env=env), SPP, depth)
    assert rad.max() > 0


@pytest.mark.parametrize("next_event", [False, True])
def test_cornell_rough_block_32x32(R, next_event):
    env = small_sky()
    o, kind = cornell(R, "cbox", 8, next_event, 32, 32, env=env)
    check_frames(R, reference(o, kind, next_event, 32, 32, env=env), SPP, 8)


def test_the_rough_block_shows_and_is_met(R):
    o, kind = cornell(R, "cbox", 8, True)
    R.render_frame()
    rough = R.read_image()[1]
    R.set_surfaces(None)
    R.update_resolution(W, H)
    R.render_frame()
    assert not np.array_equal(bits(rough), bits(R.read_image()[1]))
    ref = RoughRenderer(o, default_camera(), W, H, kind, next_event=True)
    ref.trace = []
    ref.sums(1, 8)
    assert {k for k, _, _ in ref.trace} == {0, 2, 3}


@pytest.mark.parametrize("which,walk", [("soup", "CERTIFIED"), ("soup_quads", "CERTIFIED"), ("deep", "STACK"), ("deep_quads", "STACK")])
@pytest.mark.parametrize("next_event", [False, True])
def test_the_other_walks(R, which, walk, next_event):
    """the certified walk on a soup of triangles and of quads (mirror, glass and rough metal among them, a roughness per
    primitive), the stack walk on the deep chain; the Cornell box goes through the LANE walk"""
    if which.startswith("soup"):
        arrays = ES.soup() if which == "soup" else ES.without_box("quads_many").arrays()
        kind, rough = RS.soup_table(len(arrays[0]))
    else:
        arrays, kind = RS.rough_furnace(quads=which == "deep_quads", chain=True)
        rough = 0.4
    env = small_sky() if which.startswith("soup") else None
    o = arrays_scene(R, arrays, kind, rough, 5, next_event, spp=3, env=env)
    assert R.traversal() == getattr(R, walk) and R.surface_counts()[3] > 0
    check_frames(R, reference(o, kind, next_event, roughness=rough, env=env), 3, 5)


@pytest.mark.parametrize("roughness", [0.05, 1.0])
@pytest.mark.parametrize("next_event", [False, True])
def test_roughness_at_its_ends(R, roughness, next_event):
    o, kind = cornell(R, "cbox", 5, next_event, roughness=roughness)
    check_frames(R, reference(o, kind, next_event, roughness=roughness), SPP, 5)


def test_per_primitive_roughness(R):
    R.load_scene(CBOX_QUADS, 0)
    kind = RS.blocks(R.scene_prims())
    rough = np.linspace(0.05, 1.0, len(kind)).astype(F)
    configure(R, 8, True)
    R.set_surfaces(kind, None, rough)
    check_frames(R, reference(OracleScene.load(CBOX_QUADS), kind, True, roughness=rough), SPP, 8)


@pytest.mark.parametrize("next_event", [False, True])
def test_a_rough_emitter(R, next_event):
    """the light of the Cornell box made of rough metal: Le is added as on any surface, a light sample may pick it, and a path that
    reaches it goes on through the lobe"""
    R.load_scene(CBOX, 0)
    le = R.scene_prims()["Le"]
    kind = RS.blocks(R.scene_prims())
    kind[le.any(1)] = ROUGH
    assert le.any(1).sum() == 2
    configure(R, 5, next_event)
    R.set_surfaces(kind, None, 0.5)
    _, rad, _ = check_frames(R, reference(OracleScene.load(CBOX), kind, next_event, roughness=0.5), SPP, 5)
    assert rad.max() > 0


@pytest.mark.parametrize("next_event", [False, True])
def test_tilted_and_non_unit_stored_normals(R, next_event):
    arrays, kind = RS.rough_furnace(scale_normals=True)
    o = arrays_scene(R, arrays, kind, 0.3, 8, next_event)
    check_frames(R, reference(o, kind, next_event), SPP, 8)


def test_a_zero_stored_normal_ends_the_path(R):
    """un is NaN: the grazing test fails, the path ends and the frame stays free of NaN"""
    arrays, kind = RS.rough_furnace(zero_normals=3)
    o = arrays_scene(R, arrays, kind, 0.3, 8, True)
    _, rad, _ = check_frames(R, reference(o, kind, True), SPP, 8)
    assert np.isfinite(rad).all()


@pytest.mark.parametrize("next_event", [False, True])
def test_a_camera_skimming_a_rough_quad(R, next_event):
    cam = ptmi.default_camera()
    cam.vfov_deg = 0.05                                      # every row within 5e-4 rad of the axis, which meets the quad at 1e-4 rad
    scene, kind = RS.skimming_quad(cam, W, H)
    env = small_sky()
    for roughness in (0.05, 0.6):
        o = arrays_scene(R, scene.arrays(), kind, roughness, 4, next_event, cam=cam, env=env)
        ref = reference(o, kind, next_event, roughness=roughness, env=env, cam=cam)
        _, rad, _ = check_frames(R, ref, SPP, 4, frames=1)
        assert np.isfinite(rad).all()
    ref.trace = []
    ref.sums(1, 4)
    assert sum(1 for k, d, _ in ref.trace if k == ROUGH and d == 0) > W * H // 4            # (one sample per pixel) the camera does meet the quad


# ------------------------------------------------------------------------------------------------
# a rough primitive that no ray can reach: SURF = 2 against SURF = 0 (and the bounce kernels) and against SURF = 1
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cbox", "cbox_sub"])
@pytest.mark.parametrize("table", ["diffuse", "blocks"])
@pytest.mark.parametrize("next_event", [False, True])
def test_an_unreachable_rough_primitive_changes_no_bit(R, which, table, next_event):
    """cbox: the sweep-sized scene (the LANE walk of the per-lane kernel); cbox_sub (513 primitives): the certified walk"""
    arrays, hidden = hidden_mirror(which)
    R.load_scene_arrays(*arrays)
    configure(R, 5, next_event, 32, 24)
    kind = np.zeros(hidden + 1, np.int32)
    if table == "blocks":
        kind[:hidden] = ptmi_scenes.cornell_blocks({k: v[:hidden] for k, v in R.scene_prims().items()})
    R.set_surfaces(kind, None, 0.3)
    assert R.surface_counts()[3] == 0 and (R.surface_counts()[1] > 0) == (table == "blocks")
    plain = []
    for _ in range(2):
        R.render_frame()
        plain.append(R.read_image())
    kind[hidden] = ROUGH
    R.set_surfaces(kind, None, 0.3)
    assert R.surface_counts()[3] == 1
    R.update_resolution(32, 24)
    for k in range(2):
        st = R.render_frame()
        rgb, rad = R.read_image()
        assert st.bounce_launches == 1                        # ptmi_render_nee
        assert np.array_equal(bits(rad), bits(plain[k][1])), k
        assert np.array_equal(rgb, plain[k][0])


# ------------------------------------------------------------------------------------------------
# tiling, batches, passes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_union_of_three_ranks_is_the_single_gpu_frame(R, next_event):
    w, h = 40, 37
    cornell(R, "cbox", 5, next_event, w, h, spp=3)
    R.render_frame()
    rgb_whole, whole = R.read_image()
    seen = np.zeros(h, int)
    for rank in range(3):
        R.update_resolution(w, h, n_ranks=3, rank=rank, row_block=8)
        R.render_frame()
        rgb, rad = R.read_image()
        rows = R.local_rows()
        seen[rows] += 1
        assert np.array_equal(bits(rad), bits(whole[rows]))
        assert np.array_equal(rgb, rgb_whole[rows])
    assert (seen == 1).all()


@pytest.mark.parametrize("next_event", [False, True])
def test_batch_equals_separate_frames(R, next_event):
    w, h = 32, 24
    cornell(R, "cbox_quads", 5, next_event, w, h, spp=3)
    singles = []
    for _ in range(4):
        R.render_frame()
        singles.append(R.read_image())
    R.update_resolution(w, h)
    st = R.render_frames(4)
    assert st.samples == 4 * w * h * 3
    for k in range(4):
        R.select_frame(k)
        rgb, rad = R.read_image()
        assert np.array_equal(bits(rad), bits(singles[k][1])), k
        assert np.array_equal(rgb, singles[k][0])


@pytest.mark.parametrize("next_event", [False, True])
def test_passes_equal_a_frame_of_their_samples(R, next_event):
    spp, k, w, h = 2, 3, 32, 24
    o, kind = cornell(R, "cbox", 5, next_event, w, h, spp=spp * k)
    R.render_frame()
    rgb_f, rad_f = R.read_image()
    R.update_resolution(w, h)
    R.set_config(spp=spp)
    for _ in range(k):
        R.accum_pass()
    rgb, rad = R.read_image()
    assert np.array_equal(bits(rad), bits(rad_f))
    assert np.array_equal(rgb, rgb_f)
    R.set_surfaces(kind, None, 0.6)                          # a new table restarts the accumulation
    R.accum_pass()
    assert (R.sample_counts() == spp).all()


def test_adaptive_pixels_equal_the_frame_at_their_count(R):
    spp, w, h = 2, 32, 24
    cornell(R, "cbox", 5, True, w, h, spp=spp)
    R.render_adaptive(min_passes=2, max_passes=6, threshold=0.3, floor=0.05)
    counts = R.sample_counts()
    rgb, rad = R.read_image()
    assert len(np.unique(counts)) > 1
    for c in np.unique(counts):
        R.update_resolution(w, h)
        R.set_config(spp=int(c))
        R.render_frame()
        frgb, frad = R.read_image()
        m = counts == c
        assert np.array_equal(bits(rad[m]), bits(frad[m])), c
        assert np.array_equal(rgb[m], frgb[m])


# ------------------------------------------------------------------------------------------------
# the denoiser and the temporal step take a rough frame as any other
# ------------------------------------------------------------------------------------------------
def test_denoise_on_a_rough_frame(R):
    w, h = 48, 40
    o, kind = cornell(R, "cbox", 5, True, w, h)
    with pytest.raises(ptmi.PtmiError):                      # the new table made the image stale
        R.denoise()
    R.render_frame()
    _, rad = R.read_image()
    drgb, drad = R.denoise()
    p = ptmi.default_denoise_params()
    f = R.features()
    exp = DO.denoise(rad, f, p.iterations, p.sigma_color, p.color_floor, sigma_x_auto(R), p.normal_squarings, bool(p.demodulate))
    assert np.array_equal(bits(drad), bits(exp))
    assert np.array_equal(drgb, tone_map(exp))


def test_temporal_step_on_a_rough_frame(R):
    w, h = 48, 40
    o, kind = cornell(R, "cbox", 5, True, w, h)
    cam = ptmi.default_camera()
    p = ptmi.default_temporal_params()
    b = R.scene_bvh()
    sx = TO.auto_sigma_position(b["bmin"][0], b["bmax"][0])
    hist = None
    for view in range(3):
        cam.yaw_deg = 90.0 + 2.0 * view
        R.set_camera(cam)
        R.render_frame()
        _, rad = R.read_image()
        frame = R.camera_frame()
        _, out, st = R.temporal_accumulate()
        exp, hist, (acc, rej, mis) = TO.step(hist, rad, SPP, R.features(), frame, p.max_history, p.normal_min, sx, p.sigma_albedo)
        assert np.array_equal(bits(out), bits(exp)), view
        assert (st.accepted, st.rejected, st.missed) == (acc, rej, mis)
    assert st.accepted > 0
    R.set_surfaces(kind, None, 0.8)                          # other materials: the history empties
    assert (R.history_counts() == 0).all()


# ------------------------------------------------------------------------------------------------
# state and rejections
# ------------------------------------------------------------------------------------------------
def test_invalid_combinations_in_both_call_orders(R):
    w, h = 32, 24
    o, kind = cornell(R, "cbox", 5, False, w, h, spp=2)
    kind[kind == GLASS] = 0                                   # rough metal alone must bring the restrictions
    R.set_surfaces(kind, None, 0.3)
    base = ptmi.default_config()
    base.spp, base.max_depth = 2, 5
    R.render_frame()
    _, before = R.read_image()
    for field, value in (("integrator", 1), ("sampling_mode", 3), ("sampling_mode", 1), ("fast_tree", 1)):
        bad = ptmi.Config.from_buffer_copy(base)
        setattr(bad, field, value)
        assert R.L.ptmi_set_config(R.h, C.byref(bad)) == -1, field
        assert "surfaces" in R.L.ptmi_last_error().decode()
    R.update_resolution(w, h)                                # nothing changed: the same first frame again
    R.render_frame()
    assert np.array_equal(bits(R.read_image()[1]), bits(before))
    R.set_surfaces(None)
    assert R.surface_counts() == [0, 0, 0, 0]
    k = np.ascontiguousarray(kind)
    zero = np.zeros_like(k)
    rough = np.full(len(k), 0.3, F)
    for field, value in (("integrator", 1), ("sampling_mode", 3), ("fast_tree", 1)):
        cfg = ptmi.Config.from_buffer_copy(base)
        setattr(cfg, field, value)
        assert R.L.ptmi_set_config(R.h, C.byref(cfg)) == 0
        assert R.L.ptmi_set_surfaces_rough(R.h, len(k), k.ctypes.data, None, rough.ctypes.data) == -1, field
        assert "surfaces" in R.L.ptmi_last_error().decode()
        assert R.surface_counts() == [0, 0, 0, 0]
        assert R.L.ptmi_set_surfaces_rough(R.h, len(k), zero.ctypes.data, None, rough.ctypes.data) == 0      # all diffuse: no table
        assert R.surface_counts() == [0, 0, 0, 0]
    assert R.L.ptmi_set_config(R.h, C.byref(base)) == 0
    # bad tables leave the table that is set alone; the old entry point still refuses kind 3
    R.set_surfaces(kind, None, 0.3)
    counts = R.surface_counts()
    assert counts[3] == 10 and counts[0] == len(k) - 10
    bad_kind = k.copy(); bad_kind[0] = 4
    bad_rough = rough.copy(); bad_rough[0] = 0.049            # on a diffuse entry
    assert R.L.ptmi_set_surfaces_rough(R.h, len(k), bad_kind.ctypes.data, None, rough.ctypes.data) == -1
    assert R.L.ptmi_set_surfaces_rough(R.h, len(k), k.ctypes.data, None, bad_rough.ctypes.data) == -1
    assert "roughness" in R.L.ptmi_last_error().decode()
    assert R.L.ptmi_set_surfaces_rough(R.h, len(k) - 1, k.ctypes.data, None, rough.ctypes.data) == -1
    assert R.L.ptmi_set_surfaces(R.h, len(k), k.ctypes.data, None) == -1
    assert "kind" in R.L.ptmi_last_error().decode()
    with pytest.raises(ptmi.PtmiError):
        R.set_surfaces(kind)                                 # no roughness: the old entry point
    assert R.surface_counts() == counts
    R.update_resolution(w, h)
    R.render_frame()
    assert np.array_equal(bits(R.read_image()[1]), bits(before))
    # roughness NULL is 0.3 everywhere
    assert R.L.ptmi_set_surfaces_rough(R.h, len(k), k.ctypes.data, None, None) == 0
    R.update_resolution(w, h)
    R.render_frame()
    assert np.array_equal(bits(R.read_image()[1]), bits(before))
    fresh = ptmi.Renderer(0)
    try:
        assert fresh.L.ptmi_set_surfaces_rough(fresh.h, len(k), k.ctypes.data, None, None) == -1      # no scene loaded
    finally:
        fresh.close()


def test_a_scene_load_drops_the_table(R):
    o, kind = cornell(R, "cbox", 5, True)
    assert R.surface_counts()[3] == 10
    R.render_frame()
    R.load_scene(CBOX, 0)
    assert R.surface_counts() == [0, 0, 0, 0] and R.surfaces_info() == dict(n_mirror=0, n_glass=0)
    R.update_resolution(W, H)
    check_frames(R, reference(o, np.zeros_like(kind), True), SPP, 5, frames=1)
    R.set_config(fast_tree=False, next_event=False)
    R.set_config(sampling_mode=3)                             # and nothing is left that would refuse a guided mode
    R.set_config(sampling_mode=0)


def test_command_line_writes_a_png_with_rough_metal(tmp_path):
    out = tmp_path / "metal.png"
    kind = RS.blocks(ptmi.HostScene.load(CBOX).prims())
    run = lambda idx: f"{idx.min()}-{idx.max()}"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", CBOX, "--width", "32", "--height", "24",
                          "--spp", "4", "--max-depth", "8", "--next-event", "--glass", run(np.flatnonzero(kind == GLASS)),
                          "--rough", run(np.flatnonzero(kind == ROUGH)), "--roughness", "0.3", "--out", str(out)],
                         check=True, timeout=300, capture_output=True, text=True)
    assert "0 mirror, 10 glass" in res.stdout and "10 rough-metal primitives, roughness 0.3" in res.stdout
    assert out.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
