"""Environment lighting on the GPU (include/ptmi.h: "environment lighting") against the CPU restatement of the header's contract
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
import temporal_oracle as TO
from gpu_frames import check_frames
from oracle_binding import OracleScene, SCENES, default_camera
from path_oracle import EnvRenderer
from test_gpu_denoise import sigma_x_auto, tone_map

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CBOX = os.path.join(SCENES, "cbox.obj")
CBOX_QUADS = os.path.join(SCENES, "cbox_quads.obj")
W, H = 32, 24


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture()
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def load(R, which):
    """loads `which` into the renderer and returns the oracle's copy"""
    if which in ("cbox", "cbox_quads"):
        path = CBOX if which == "cbox" else CBOX_QUADS
        R.load_scene(path, 0)
        return OracleScene.load(path)
    arrays = {"soup": lambda: ES.soup(), "soup_dark": lambda: ES.soup(emitters=False),
              "deep_open": lambda: ES.without_box("deep").arrays()}[which]()
    R.load_scene_arrays(*arrays)
    return OracleScene.from_arrays(*arrays)


def setup(R, which, spp, depth, next_event, w=W, h=H):
    o = load(R, which)
    R.set_camera(ptmi.default_camera())
    R.update_resolution(w, h)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    return o


def reference(o, env, next_event, **prm):
    return EnvRenderer(o, default_camera(), W, H, env, next_event, **prm)


# ------------------------------------------------------------------------------------------------
# bit for bit against the restatement, first and second frame (the streams carry over)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
@pytest.mark.parametrize("depth", [1, 2, 5, 8])
def test_cbox_under_the_sky(R, next_event, depth):
    env = ES.sky_32x16()
    o = setup(R, "cbox", 3, depth, next_event)
    R.set_environment(env)
    info = R.environment_info()
    assert (info["width"], info["height"]) == (32, 16) and info["total"] == ptmi.host_env_table(env)["total"]
    _, rad, _ = check_frames(R, reference(o, env, next_event), 3, depth)
    assert rad.max() > 0


@pytest.mark.parametrize("next_event", [False, True])
def test_cbox_quads_with_a_turned_map(R, next_event):
    env = ES.random_map(7, 5, 12)
    o = setup(R, "cbox_quads", 3, 5, next_event)
    R.set_environment(env, rotation_deg=70.0, scale=1.5)
    check_frames(R, reference(o, env, next_event, rotation_deg=70.0, scale=1.5), 3, 5)


@pytest.mark.parametrize("which,walk,next_event", [("soup", "CERTIFIED", False), ("soup", "CERTIFIED", True),
                                                   ("deep_open", "STACK", False), ("deep_open", "STACK", True)])
def test_the_other_walks(R, which, walk, next_event):
    env = ES.sky_32x16()
    o = setup(R, which, 3, 5, next_event)
    assert R.traversal() == getattr(R, walk)
    R.set_environment(env)
    check_frames(R, reference(o, env, next_event), 3, 5)


def test_a_scene_without_emitters_samples_the_environment_only(R):
    """q = 1 whatever select_fraction says; without the map this scene renders black"""
    env = ES.sky_32x16()
    o = setup(R, "soup_dark", 4, 5, True)
    assert len(ptmi.HostScene.from_arrays(*ES.soup(emitters=False)).emitters()["prim"]) == 0
    R.render_frame()
    assert R.read_image()[1].max() == 0
    R.update_resolution(W, H)
    R.set_environment(env, select_fraction=0.25)
    _, rad, _ = check_frames(R, reference(o, env, True, select_fraction=0.25), 4, 5)
    assert rad.max() > 0


@pytest.mark.parametrize("fraction", [0.0, 1.0])
def test_select_fraction_at_its_ends(R, fraction):
    env = ES.sky_32x16()
    o = setup(R, "cbox", 4, 5, True)
    R.set_environment(env, select_fraction=fraction)
    check_frames(R, reference(o, env, True, select_fraction=fraction), 4, 5)


# ------------------------------------------------------------------------------------------------
# nothing to add: the frame without a map
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_black_maps_and_a_dropped_map_give_the_frame_without_one(R, next_event):
    setup(R, "cbox", 3, 5, next_event)
    plain = []
    for _ in range(2):
        R.render_frame()
        plain.append(R.read_image())
    assert R.environment_info() == dict(width=0, height=0, total=0)

    def same_as_plain(tag):
        R.update_resolution(W, H)                          # freshly seeded streams
        for k in range(2):
            R.render_frame()
            rgb, rad = R.read_image()
            assert np.array_equal(bits(rad), bits(plain[k][1])), (tag, k)
            assert np.array_equal(rgb, plain[k][0])

    R.set_environment(np.zeros((5, 7, 3), F))
    assert R.environment_info()["total"] == 0 and R.environment_info()["width"] == 7
    same_as_plain("all-zero map")
    R.set_environment(ES.sky_32x16(), scale=0.0)
    assert R.environment_info()["total"] == 0
    same_as_plain("scale 0")
    R.set_environment(ES.sky_32x16())
    R.render_frame()
    assert not np.array_equal(bits(R.read_image()[1]), bits(plain[0][1]))
    R.set_environment(None)
    assert R.environment_info() == dict(width=0, height=0, total=0)
    same_as_plain("dropped")


def test_the_map_survives_a_scene_load(R):
    env = ES.sky_32x16()
    setup(R, "soup", 3, 5, True)
    R.set_environment(env, rotation_deg=30.0)
    R.render_frame()
    o = load(R, "cbox")
    assert R.environment_info()["width"] == 32
    R.update_resolution(W, H)
    check_frames(R, reference(o, env, True, rotation_deg=30.0), 3, 5, frames=1)


# ------------------------------------------------------------------------------------------------
# tiling, batches, passes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_union_of_three_ranks_is_the_single_gpu_frame(R, next_event):
    w, h = 40, 37
    setup(R, "cbox", 3, 5, next_event, w, h)
    R.set_environment(ES.sky_32x16())
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
    setup(R, "cbox_quads", 3, 5, next_event)
    R.set_environment(ES.sky_32x16())
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
    setup(R, "soup", spp * k, 5, next_event)
    R.set_environment(ES.sky_32x16())
    R.render_frame()
    rgb_f, rad_f = R.read_image()
    R.update_resolution(W, H)
    R.set_config(spp=spp)
    for _ in range(k):
        R.accum_pass()
    rgb, rad = R.read_image()
    assert np.array_equal(bits(rad), bits(rad_f))
    assert np.array_equal(rgb, rgb_f)
    R.set_environment(ES.sky_32x16(), scale=2.0)          # a new map restarts the accumulation
    R.accum_pass()
    assert (R.sample_counts() == spp).all()


def test_adaptive_pixels_equal_the_frame_at_their_count(R):
    spp = 2
    setup(R, "cbox", spp, 5, True)
    R.set_environment(ES.sky_32x16())
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
# the denoiser and the temporal step take an environment frame as any other
# ------------------------------------------------------------------------------------------------
def test_denoise_and_the_pixels_that_see_only_sky(R):
    w, h = 48, 40
    setup(R, "soup", 4, 5, True, w, h)
    R.set_environment(ES.sky_32x16())
    with pytest.raises(ptmi.PtmiError):                    # the new map made the image stale
        R.denoise()
    R.render_frame()
    _, rad = R.read_image()
    drgb, drad = R.denoise()
    p = ptmi.default_denoise_params()
    f = R.features()
    exp = DO.denoise(rad, f, p.iterations, p.sigma_color, p.color_floor, sigma_x_auto(R), p.normal_squarings, bool(p.demodulate))
    assert np.array_equal(bits(drad), bits(exp))
    assert np.array_equal(drgb, tone_map(exp))
    missed = f["hit_fraction"] == 0
    assert missed.sum() > 20 and (rad[missed] > 0).all()   # the background shows there
    assert np.array_equal(bits(drad[missed]), bits(rad[missed]))   # every tap weighs 0: the pixel keeps its input


def test_temporal_step_on_an_environment_frame(R):
    w, h = 48, 40
    setup(R, "soup", 4, 5, True, w, h)
    R.set_environment(ES.sky_32x16())
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
        exp, hist, (acc, rej, mis) = TO.step(hist, rad, 4, R.features(), frame, p.max_history, p.normal_min, sx, p.sigma_albedo)
        assert np.array_equal(bits(out), bits(exp)), view
        assert (st.accepted, st.rejected, st.missed) == (acc, rej, mis)
    assert st.accepted > 0 and st.missed > 0               # pixels that see only sky restart with the current frame
    missed = R.features()["hit_fraction"] == 0
    assert np.array_equal(bits(out[missed]), bits(rad[missed]))
    R.set_environment(ES.sky_32x16(), scale=0.5)          # another light: the history empties
    assert (R.history_counts() == 0).all()


# ------------------------------------------------------------------------------------------------
# configuration
# ------------------------------------------------------------------------------------------------
def test_invalid_combinations_in_both_call_orders(R):
    env = ES.sky_32x16()
    setup(R, "cbox", 2, 5, False)
    base = ptmi.default_config()
    base.spp, base.max_depth = 2, 5
    # an environment first: the config is rejected and names the environment
    R.set_environment(env)
    R.render_frame()
    _, before = R.read_image()
    for field, value in (("integrator", 1), ("sampling_mode", 3), ("sampling_mode", 1), ("fast_tree", 1)):
        bad = ptmi.Config.from_buffer_copy(base)
        setattr(bad, field, value)
        assert R.L.ptmi_set_config(R.h, C.byref(bad)) == -1, field
        assert "environment" in R.L.ptmi_last_error().decode()
    R.update_resolution(W, H)                              # nothing changed: the same first frame again
    R.render_frame()
    assert np.array_equal(bits(R.read_image()[1]), bits(before))
    # the config first: the environment is rejected, names itself, and none is set
    R.set_environment(None)
    e = np.ascontiguousarray(env)
    for field, value in (("integrator", 1), ("sampling_mode", 3), ("fast_tree", 1)):
        cfg = ptmi.Config.from_buffer_copy(base)
        setattr(cfg, field, value)
        assert R.L.ptmi_set_config(R.h, C.byref(cfg)) == 0
        assert R.L.ptmi_set_environment(R.h, 32, 16, e.ctypes.data, None) == -1, field
        assert "environment" in R.L.ptmi_last_error().decode()
        assert R.environment_info()["width"] == 0
    assert R.L.ptmi_set_config(R.h, C.byref(base)) == 0
    # bad maps and parameters leave the map that is set alone
    R.set_environment(env)
    bad_map = e.copy(); bad_map[3, 4, 1] = np.nan
    assert R.L.ptmi_set_environment(R.h, 32, 16, bad_map.ctypes.data, None) == -1
    bad_map[3, 4, 1] = -1.0
    assert R.L.ptmi_set_environment(R.h, 32, 16, bad_map.ctypes.data, None) == -1
    assert R.L.ptmi_set_environment(R.h, 0, 16, e.ctypes.data, None) == -1
    assert R.L.ptmi_set_environment(R.h, 1 << 13, (1 << 12) + 1, e.ctypes.data, None) == -1
    assert R.L.ptmi_set_environment(R.h, 32, 16, e.ctypes.data, C.byref(ptmi.default_env_params(select_fraction=2.0))) == -1
    R.update_resolution(W, H)
    R.render_frame()
    assert np.array_equal(bits(R.read_image()[1]), bits(before))


def test_command_line_writes_a_png_with_a_sky(tmp_path):
    out = tmp_path / "sky.png"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", CBOX, "--width", "32", "--height", "24",
                    "--spp", "4", "--next-event", "--sky", "--env-rotation", "40", "--out", str(out)], check=True, timeout=300)
    assert out.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
