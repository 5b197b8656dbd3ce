"""Specular surfaces on the GPU (include/ptmi.h: "specular surfaces") against the CPU restatement of the header's contract
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
import specular_scenes as SS
import temporal_oracle as TO
from gpu_frames import check_frames, hidden_mirror, small_sky
from oracle_binding import OracleScene, SCENES, default_camera
from path_oracle import SpecRenderer
from specular_oracle import GLASS, MIRROR
from test_gpu_denoise import sigma_x_auto, tone_map

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CBOX = os.path.join(SCENES, "cbox.obj")
CBOX_QUADS = os.path.join(SCENES, "cbox_quads.obj")
W, H = 32, 24
SPP = 4


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture()
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def load(R, which):
    """loads `which` into the renderer and returns (the oracle's copy, the kind array)"""
    if which in ("cbox", "cbox_quads"):
        path = CBOX if which == "cbox" else CBOX_QUADS
        R.load_scene(path, 0)
        kind = ptmi_scenes.cornell_blocks(R.scene_prims())
        return OracleScene.load(path), kind
    if which in ("soup", "soup_quads"):                      # above 64 primitives: the certified walk
        if which == "soup":
            arrays = ES.soup()
        else:
            arrays = ES.without_box("quads_many").arrays()
        kind = np.zeros(len(arrays[0]), np.int32)
        kind[::5] = MIRROR; kind[2::5] = GLASS               # two fifths of the soup, emitters among them
    else:                                                    # "deep", "deep_quads": a tree deeper than 62 levels, the stack walk
        s, kind = SS.black_furnace(quads=which == "deep_quads", chain=True)
        s.b[:FN_BOX[which]] = [(0.6, 0.5, 0.4)] * FN_BOX[which]    # walls that scatter, so that light samples are made too
        arrays = s.arrays()
    R.load_scene_arrays(*arrays)
    return OracleScene.from_arrays(*arrays), kind


FN_BOX = {"deep": 12, "deep_quads": 6}


def setup(R, which, depth, next_event, w=W, h=H, spp=SPP, ior=None, env=None, surfaces=True):
    o, kind = load(R, which)
    R.set_camera(ptmi.default_camera())
    R.update_resolution(w, h)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    if env is not None:
        R.set_environment(env)
    if surfaces:
        R.set_surfaces(kind, ior)
    return o, kind


def reference(o, kind, next_event, w=W, h=H, ior=None, env=None):
    return SpecRenderer(o, default_camera(), w, h, kind, ior, env, next_event)


# ------------------------------------------------------------------------------------------------
# bit for bit against the restatement, first and second frame (the streams carry over)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sky", [False, True])
@pytest.mark.parametrize("next_event", [False, True])
@pytest.mark.parametrize("depth", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("which", ["cbox", "cbox_quads"])
def test_cornell_blocks_17x13(R, which, depth, next_event, sky):
    env = small_sky() if sky else None
    o, kind = setup(R, which, depth, next_event, 17, 13, env=env)
    assert R.surfaces_info() == dict(n_mirror=int((kind == 1).sum()), n_glass=int((kind == 2).sum()))
    _, rad, _ = check_frames(R, reference(o, kind, next_event, 17, 13, env=env), SPP, depth)
    assert rad.max() > 0


@pytest.mark.parametrize("sky", [False, True])
@pytest.mark.parametrize("next_event", [False, True])
@pytest.mark.parametrize("depth", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("which", ["cbox", "cbox_quads"])
def test_cornell_blocks_32x32(R, which, depth, next_event, sky):
    env = small_sky() if sky else None
    o, kind = setup(R, which, depth, next_event, 32, 32, env=env)
    check_frames(R, reference(o, kind, next_event, 32, 32, env=env), SPP, depth)


def test_the_blocks_show(R):
    """the frame differs from the diffuse one where the blocks are, and both specular kinds were met"""
    o, kind = setup(R, "cbox", 8, True)
    R.render_frame()
    spec = R.read_image()[1]
    R.set_surfaces(None)
    R.update_resolution(W, H)
    R.render_frame()
    assert not np.array_equal(bits(spec), bits(R.read_image()[1]))
    ref = SpecRenderer(o, default_camera(), W, H, kind, next_event=True)
    ref.trace = []
    ref.sums(1, 8)
    assert {k for k, _, _ in ref.trace} == {0, 1, 2}


@pytest.mark.parametrize("which,walk", [("soup", "CERTIFIED"), ("soup_quads", "CERTIFIED"), ("deep", "STACK"), ("deep_quads", "STACK")])
@pytest.mark.parametrize("next_event", [False, True])
def test_the_other_walks(R, which, walk, next_event):
    """(the Cornell box, a scene of the sweep's size, goes through ptmi_render_nee's LANE walk)"""
    o, kind = setup(R, which, 5, next_event, spp=3)
    assert R.traversal() == getattr(R, walk)
    check_frames(R, reference(o, kind, next_event), 3, 5)


@pytest.mark.parametrize("next_event", [False, True])
def test_a_glass_emitter(R, next_event):
    """the light of the Cornell box made of glass: Le is added as on any surface, and a light sample may pick it"""
    o, kind = load(R, "cbox")
    le = R.scene_prims()["Le"]
    kind[le.any(1)] = GLASS
    assert (kind[le.any(1)] == GLASS).all() and le.any(1).sum() == 2
    R.set_camera(ptmi.default_camera()); R.update_resolution(W, H)
    R.set_config(spp=SPP, max_depth=5, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    R.set_surfaces(kind)
    _, rad, _ = check_frames(R, reference(o, kind, next_event), SPP, 5)
    assert rad.max() > 0


@pytest.mark.parametrize("ior", [1.0, 8.0])
def test_ior_at_its_ends(R, ior):
    o, kind = setup(R, "cbox", 8, True, ior=ior)
    check_frames(R, reference(o, kind, True, ior=ior), SPP, 8)


def test_per_primitive_ior(R):
    o, kind = load(R, "cbox_quads")
    ior = np.linspace(1.0, 8.0, len(kind)).astype(F)
    R.set_camera(ptmi.default_camera()); R.update_resolution(W, H)
    R.set_config(spp=SPP, max_depth=8, sampling_mode=0, integrator=0, fast_tree=False, next_event=False)
    R.set_surfaces(kind, ior)
    check_frames(R, reference(o, kind, False, ior=ior), SPP, 8)


@pytest.mark.parametrize("next_event", [False, True])
def test_a_tilted_stored_normal_on_a_mirror(R, next_event):
    """tests/specular_scenes.py's furnace: four mirror panels with stored normals 19 degrees off their planes, and the cuboid"""
    s, kind = SS.black_furnace()
    s.b[:12] = [(0.6, 0.5, 0.4)] * 12
    for k in (12, 13, 20, 21):                                # and a panel and a face of the cuboid with stored normals not of unit length
        s.n[k] = tuple((5.0 if k < 20 else 0.25) * np.asarray(s.n[k]))
    assert kind[12] == MIRROR and kind[20] == GLASS
    arrays = s.arrays()
    R.load_scene_arrays(*arrays)
    R.set_camera(ptmi.default_camera()); R.update_resolution(W, H)
    R.set_config(spp=SPP, max_depth=8, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    R.set_surfaces(kind)
    check_frames(R, reference(OracleScene.from_arrays(*arrays), kind, next_event), SPP, 8)


def test_a_zero_stored_normal_ends_the_path(R):
    """un is NaN: the path ends before anything is traced with it, and the frame stays free of NaN"""
    s, kind = SS.black_furnace()
    arrays = list(s.arrays())
    arrays[2][np.flatnonzero(kind == MIRROR)[:2]] = 0.0
    arrays[2][np.flatnonzero(kind == GLASS)[:4]] = 0.0
    R.load_scene_arrays(*arrays)
    R.set_camera(ptmi.default_camera()); R.update_resolution(W, H)
    R.set_config(spp=SPP, max_depth=8, sampling_mode=0, integrator=0, fast_tree=False, next_event=True)
    R.set_surfaces(kind)
    _, rad, _ = check_frames(R, reference(OracleScene.from_arrays(*arrays), kind, True), SPP, 8)
    assert np.isfinite(rad).all()


# ------------------------------------------------------------------------------------------------
# a specular primitive that no ray can reach: the SPEC kernel against the kernels this change does not touch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cbox", "cbox_quads", "cbox_sub"])
@pytest.mark.parametrize("next_event", [False, True])
def test_an_unreachable_mirror_changes_no_bit(R, which, next_event):
    """cbox / cbox_quads: the sweep, cbox_sub (513 primitives): the certified walk of the phased kernels"""
    arrays, hidden = hidden_mirror(which)
    R.load_scene_arrays(*arrays)
    R.set_camera(ptmi.default_camera()); R.update_resolution(W, H)
    R.set_config(spp=SPP, max_depth=5, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    kind = np.zeros(hidden + 1, np.int32)
    R.set_surfaces(kind)
    assert R.surfaces_info() == dict(n_mirror=0, n_glass=0)
    plain = []
    for _ in range(2):
        R.render_frame()
        plain.append(R.read_image())
    assert R.traversal() == (R.CERTIFIED if which == "cbox_sub" else R.SWEEP)      # next_event 0: the bounce kernels rendered these
    kind[hidden] = MIRROR
    R.set_surfaces(kind)
    assert R.surfaces_info() == dict(n_mirror=1, n_glass=0)
    R.update_resolution(W, H)
    for k in range(2):
        st = R.render_frame()
        rgb, rad = R.read_image()
        assert st.bounce_launches == 1                        # ptmi_render_nee
        assert np.array_equal(bits(rad), bits(plain[k][1])), k
        assert np.array_equal(rgb, plain[k][0])


# ------------------------------------------------------------------------------------------------
# no table, an all-diffuse table, a scene load
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_all_diffuse_and_dropped_tables_give_the_frame_without_one(R, next_event):
    o, kind = setup(R, "cbox", 5, next_event, surfaces=False)
    plain = []
    for _ in range(2):
        R.render_frame()
        plain.append(R.read_image())
    assert R.surfaces_info() == dict(n_mirror=0, n_glass=0)

    def same_as_plain(tag):
        R.update_resolution(W, H)                            # freshly seeded streams
        for k in range(2):
            st = R.render_frame()
            rgb, rad = R.read_image()
            assert np.array_equal(bits(rad), bits(plain[k][1])), (tag, k)
            assert np.array_equal(rgb, plain[k][0])
        return st

    R.set_surfaces(np.zeros(len(kind), np.int32), 2.0)
    same_as_plain("all diffuse")
    R.set_surfaces(kind)
    R.render_frame()
    assert not np.array_equal(bits(R.read_image()[1]), bits(plain[0][1]))
    R.set_surfaces(None)
    assert R.surfaces_info() == dict(n_mirror=0, n_glass=0)
    same_as_plain("dropped")


def test_a_scene_load_drops_the_table(R):
    o, kind = setup(R, "cbox", 5, True)
    R.set_environment(small_sky())
    assert R.surfaces_info()["n_glass"] == 10
    R.render_frame()
    R.load_scene(CBOX, 0)
    assert R.surfaces_info() == dict(n_mirror=0, n_glass=0)
    assert R.environment_info()["width"] == 7                 # the environment belongs to the context and stays
    R.update_resolution(W, H)
    check_frames(R, reference(o, np.zeros_like(kind), True, env=small_sky()), SPP, 5, frames=1)
    R.set_config(fast_tree=False, next_event=False)
    R.set_environment(None)
    R.set_config(sampling_mode=3)                             # and nothing is left that would refuse a guided mode
    R.set_config(sampling_mode=0)


# ------------------------------------------------------------------------------------------------
# tiling, batches, passes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_union_of_three_ranks_is_the_single_gpu_frame(R, next_event):
    w, h = 40, 37
    setup(R, "cbox", 5, next_event, w, h, spp=3)
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
    setup(R, "cbox_quads", 5, next_event, spp=3)
    singles = []
    for _ in range(4):
        R.render_frame()
        singles.append(R.read_image())
    R.update_resolution(W, H)
    st = R.render_frames(4)
    assert st.samples == 4 * W * H * 3
    for k in range(4):
        R.select_frame(k)
        rgb, rad = R.read_image()
        assert np.array_equal(bits(rad), bits(singles[k][1])), k
        assert np.array_equal(rgb, singles[k][0])


@pytest.mark.parametrize("next_event", [False, True])
def test_passes_equal_a_frame_of_their_samples(R, next_event):
    spp, k = 2, 3
    o, kind = setup(R, "cbox", 5, next_event, spp=spp * k)
    R.render_frame()
    rgb_f, rad_f = R.read_image()
    R.update_resolution(W, H)
    R.set_config(spp=spp)
    for _ in range(k):
        R.accum_pass()
    rgb, rad = R.read_image()
    assert np.array_equal(bits(rad), bits(rad_f))
    assert np.array_equal(rgb, rgb_f)
    R.set_surfaces(kind, 1.33)                               # a new table restarts the accumulation
    R.accum_pass()
    assert (R.sample_counts() == spp).all()


def test_adaptive_pixels_equal_the_frame_at_their_count(R):
    spp = 2
    setup(R, "cbox", 5, True, spp=spp)
    R.render_adaptive(min_passes=2, max_passes=6, threshold=0.3, floor=0.05)
    counts = R.sample_counts()
    rgb, rad = R.read_image()
    assert len(np.unique(counts)) > 1
    for c in np.unique(counts):
        R.update_resolution(W, H)
        R.set_config(spp=int(c))
        R.render_frame()
        frgb, frad = R.read_image()
        m = counts == c
        assert np.array_equal(bits(rad[m]), bits(frad[m])), c
        assert np.array_equal(rgb[m], frgb[m])


# ------------------------------------------------------------------------------------------------
# the denoiser and the temporal step take a specular frame as any other; the features ignore the table
# ------------------------------------------------------------------------------------------------
def test_denoise_on_a_specular_frame(R):
    w, h = 48, 40
    o, kind = setup(R, "cbox", 5, True, w, h)
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
    R.set_surfaces(None)
    R.render_features(p.feature_grid)
    g = R.features()
    for key in ("albedo", "normal", "position", "hit_fraction"):     # bsdf stays the albedo of a mirror and of glass
        assert np.array_equal(bits(f[key]), bits(g[key])), key


def test_temporal_step_on_a_specular_frame(R):
    w, h = 48, 40
    o, kind = setup(R, "cbox", 5, True, w, h)
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
    R.set_surfaces(kind, 2.0)                                # other materials: the history empties
    assert (R.history_counts() == 0).all()


# ------------------------------------------------------------------------------------------------
# configuration
# ------------------------------------------------------------------------------------------------
def test_invalid_combinations_in_both_call_orders(R):
    o, kind = setup(R, "cbox", 5, False, spp=2)
    base = ptmi.default_config()
    base.spp, base.max_depth = 2, 5
    R.render_frame()
    _, before = R.read_image()
    # a table first: the config is rejected and names the surfaces
    for field, value in (("integrator", 1), ("sampling_mode", 3), ("sampling_mode", 1), ("fast_tree", 1)):
        bad = ptmi.Config.from_buffer_copy(base)
        setattr(bad, field, value)
        assert R.L.ptmi_set_config(R.h, C.byref(bad)) == -1, field
        assert "specular surfaces" in R.L.ptmi_last_error().decode()
    R.update_resolution(W, H)                                # nothing changed: the same first frame again
    R.render_frame()
    assert np.array_equal(bits(R.read_image()[1]), bits(before))
    # the config first: the table is rejected, names itself, and none is set; an all-diffuse table is no table and passes
    R.set_surfaces(None)
    k = np.ascontiguousarray(kind)
    zero = np.zeros_like(k)
    for field, value in (("integrator", 1), ("sampling_mode", 3), ("fast_tree", 1)):
        cfg = ptmi.Config.from_buffer_copy(base)
        setattr(cfg, field, value)
        assert R.L.ptmi_set_config(R.h, C.byref(cfg)) == 0
        assert R.L.ptmi_set_surfaces(R.h, len(k), k.ctypes.data, None) == -1, field
        assert "surfaces" in R.L.ptmi_last_error().decode()
        assert R.surfaces_info() == dict(n_mirror=0, n_glass=0)
        assert R.L.ptmi_set_surfaces(R.h, len(k), zero.ctypes.data, None) == 0
    assert R.L.ptmi_set_config(R.h, C.byref(base)) == 0
    # bad tables leave the table that is set alone
    R.set_surfaces(kind)
    bad_kind = k.copy(); bad_kind[3] = 3
    ior = np.full(len(k), 1.5, F); bad_ior = ior.copy(); bad_ior[-1] = np.nan
    assert R.L.ptmi_set_surfaces(R.h, len(k), bad_kind.ctypes.data, None) == -1
    assert R.L.ptmi_set_surfaces(R.h, len(k), k.ctypes.data, bad_ior.ctypes.data) == -1
    bad_ior[-1] = 9.0
    assert R.L.ptmi_set_surfaces(R.h, len(k), k.ctypes.data, bad_ior.ctypes.data) == -1
    assert R.L.ptmi_set_surfaces(R.h, len(k) - 1, k.ctypes.data, None) == -1
    assert "n_prims" in R.L.ptmi_last_error().decode()
    assert R.L.ptmi_set_surfaces(R.h, len(k) + 1, k.ctypes.data, None) == -1
    assert R.surfaces_info() == dict(n_mirror=10, n_glass=10)
    R.update_resolution(W, H)
    R.render_frame()
    assert np.array_equal(bits(R.read_image()[1]), bits(before))
    fresh = ptmi.Renderer(0)
    try:
        assert fresh.L.ptmi_set_surfaces(fresh.h, len(k), k.ctypes.data, None) == -1      # no scene loaded
    finally:
        fresh.close()


def test_command_line_writes_a_png_with_mirror_and_glass(tmp_path):
    out = tmp_path / "blocks.png"
    kind = ptmi_scenes.cornell_blocks(ptmi.HostScene.load(CBOX).prims())
    run = lambda idx: f"{idx.min()}-{idx.max()}"
    mirror, glass = np.flatnonzero(kind == 1), np.flatnonzero(kind == 2)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", CBOX, "--width", "32", "--height", "24",
                          "--spp", "4", "--max-depth", "8", "--next-event", "--mirror", run(mirror[:-1]) + f",{mirror[-1]}", "--glass", run(glass),
                          "--ior", "1.5", "--out", str(out)], check=True, timeout=300, capture_output=True, text=True)
    assert "10 mirror, 10 glass" in res.stdout
    assert out.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
