"""The thin lens on the GPU (include/ptmi.h: "thin lens") against the CPU restatement of the header's contract
(tests/lens_oracle.py), bit for bit: the kernel's function per call, frames through every way a context renders, what the lens
leaves alone, and what setting it drops."""
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_oracle as DO
import lens_oracle as LO
import ptmi
import temporal_oracle as TO
import texture_cases as TC
from gpu_frames import check_frames, ocam, small_sky
from oracle_binding import OracleScene, default_camera
from test_gpu_denoise import sigma_x_auto, tone_map
from test_gpu_smooth import spheres

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 33, 19                                                  # 627 pixels: not a multiple of the block, the idx >= n exit is live
SPP = 3
MIRROR, GLASS, ROUGH = 1, 2, 3
LENSES = [(0.05, 3.0), (1.0, 8.5), (0.05, 8.5), (1.0, 3.0)]    # R in {0.05, 1} x f in {3, 8.5}
TINY = F(2.0 ** -33)
EDGE_R3 = (TINY, F(1.0))
EDGE_R4 = (TINY, F(0.25), F(0.5), F(1.0))
PIXELS = ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture()
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def setup(R, arrays, depth, next_event, w=W, h=H, spp=SPP, kind=None, rough=False, env=None, normals=None, cam=None):
    R.load_scene_arrays(*arrays)
    R.set_camera(cam or ptmi.default_camera())
    R.update_resolution(w, h)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    if env is not None:
        R.set_environment(env)
    if kind is not None and kind.any():
        R.set_surfaces(kind, 1.5, 0.3 if rough else None)
    if normals is not None:
        R.set_vertex_normals(normals)


def reference(arrays, lens, next_event, w=W, h=H, kind=None, env=None, cam=None):
    return LO.LensRenderer(OracleScene.from_arrays(*arrays), cam or default_camera(), w, h, kind=kind, env_rgb=env, next_event=next_event,
                           radius=lens[0], focus_distance=lens[1])


def frames(R, n=2, w=W, h=H):
    """n consecutive frames of the context as it is, from freshly seeded streams: [(rgb, radiance, stats)]"""
    R.update_resolution(w, h)
    out = []
    for _ in range(n):
        st = R.render_frame()
        out.append(R.read_image() + (st,))
    return out


def curand_uniforms(rng, shape):
    """uniforms as the stream makes them: x * 2^-32 + 2^-33 of a 32-bit x, in binary32"""
    x = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(F)
    return (x * F(2.3283064e-10) + F(2.3283064e-10 / 2.0)).astype(F)


# ------------------------------------------------------------------------------------------------
# a. the kernel's function, per call
# ------------------------------------------------------------------------------------------------
def per_call(R, block, px, py, r):
    got = R.debug_lens_ray(px, py, r)
    for i in range(len(px)):
        o, d = LO.lens_ray(block, int(px[i]), int(py[i]), *r[i])
        exp = np.concatenate([o, d]).astype(F)
        assert np.array_equal(bits(got[i]), bits(exp)), (i, px[i], py[i], r[i], got[i], exp)
    return got


@pytest.mark.parametrize("lens", LENSES)
def test_lens_ray_at_the_edges_of_its_inputs(R, lens):
    cam = ptmi.default_camera()
    R.set_camera(cam)
    R.update_resolution(W, H)
    with pytest.raises(ptmi.PtmiError, match="no lens"):
        R.debug_lens_ray(np.zeros(1, np.int32), np.zeros(1, np.int32), np.ones((1, 4), F))
    R.set_lens(*lens)
    block = R.debug_lens_block()
    assert np.array_equal(bits(block), bits(ptmi.host_lens_block(cam, W, H, *lens)))
    assert np.array_equal(bits(block), bits(LO.lens_block(LO.frame_of(ocam(cam), W, H), W, H, *lens)))
    cases = [(x, y, r3, r4, r1, r2) for (x, y) in PIXELS for r3 in EDGE_R3 for r4 in EDGE_R4 for (r1, r2) in ((TINY, F(1.0)), (F(1.0), TINY), (F(0.5), F(0.5)))]
    px = np.array([c[0] for c in cases], np.int32); py = np.array([c[1] for c in cases], np.int32)
    r = np.array([c[2:] for c in cases], F)
    got = per_call(R, block, px, py, r)
    assert np.isfinite(got).all()
    assert np.allclose(np.linalg.norm(got[:, 3:].astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_lens_ray_on_random_draws(R):
    cam = ptmi.default_camera()
    cam.yaw_deg, cam.pitch_deg = 60.0, 20.0
    R.set_camera(cam)
    R.update_resolution(W, H)
    R.set_lens(0.3, 5.0)
    block = R.debug_lens_block()
    rng = np.random.default_rng(11)
    n = 4096
    px = rng.integers(0, W, n).astype(np.int32); py = rng.integers(0, H, n).astype(np.int32)
    got = per_call(R, block, px, py, curand_uniforms(rng, (n, 4)))
    off = np.linalg.norm(got[:, :3].astype(np.float64) - block[3, :3].astype(np.float64), axis=1)
    assert off.max() <= 0.3 * (1 + 2.0 ** -22) and off.max() > 0.29


# ------------------------------------------------------------------------------------------------
# b. frames, bit for bit against the restatement, first and second frame (the streams carry over)
# ------------------------------------------------------------------------------------------------
def surface_kinds(parts, n, surfaces):
    kind = np.zeros(n, np.int32)
    if surfaces == "mirror_glass":
        kind[parts["short"]] = MIRROR; kind[parts["tall"]] = GLASS
    elif surfaces == "rough_glass":
        kind[parts["short"]] = ROUGH; kind[parts["tall"]] = GLASS
    return kind


VARIANTS = ["plain", "sky", "mirror_glass", "rough_glass"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("next_event", [False, True])
@pytest.mark.parametrize("depth", [1, 3, 8])
@pytest.mark.parametrize("which", ["cbox", "cbox_quads"])
def test_cornell_box_through_a_lens_33x19(R, which, depth, next_event, variant):
    arrays, parts = TC.cornell(which)
    n = len(arrays[0])
    # every (R, f) pair meets every value of every other parameter
    lens = LENSES[(VARIANTS.index(variant) + [1, 3, 8].index(depth) + int(next_event) + int(which == "cbox_quads")) % 4]
    kind = surface_kinds(parts, n, variant)
    env = small_sky() if variant == "sky" else None
    setup(R, arrays, depth, next_event, kind=kind, rough=variant == "rough_glass", env=env)
    R.set_lens(*lens)
    assert R.lens() == (F(lens[0]), F(lens[1]))
    _, rad, _ = check_frames(R, reference(arrays, lens, next_event, kind=kind, env=env), SPP, depth)
    assert rad.max() > 0


@pytest.mark.parametrize("next_event", [False, True])
def test_vertex_normals_and_a_texture_through_a_lens(R, next_event):
    arrays, normals, ranges = spheres("cbox_quads")
    n = len(arrays[0])
    img, uv = TC.image(), TC.random_uvs(n)
    kind = np.zeros(n, np.int32)
    kind[slice(*ranges["short"])] = ROUGH; kind[slice(*ranges["tall"])] = GLASS
    setup(R, arrays, 5, next_event, 17, 13, kind=kind, rough=True, normals=normals)
    R.set_albedo_texture(img, uv, None, "bilinear")
    R.set_lens(0.3, 8.5)
    ref = LO.LensTexturedSmoothRenderer(OracleScene.from_arrays(*arrays), default_camera(), 17, 13, normals, kind=kind, next_event=next_event,
                                        image=img, uv=uv, filter="bilinear", radius=0.3, focus_distance=8.5)
    check_frames(R, ref, SPP, 5)


_walk_ref = {}


@pytest.mark.parametrize("walk", ["LANE", "CERTIFIED", "STACK"])
@pytest.mark.parametrize("next_event", [False, True])
def test_the_three_walks(R, walk, next_event):
    """ptmi_render_nee's three walks, forced on one scene of 512 triangles: one restatement for all three"""
    arrays, _ = TC.cornell("cbox_sub")
    lens = (0.3, 6.0)
    setup(R, arrays, 5, next_event, 17, 13)
    R.set_lens(*lens)
    mode = getattr(R, walk)
    try:
        assert R.set_traversal(mode) == mode
        if next_event not in _walk_ref:
            ref = reference(arrays, lens, next_event, 17, 13)
            _walk_ref[next_event] = [ref.frame(SPP, 5) for _ in range(2)]
        for k in range(2):
            st = R.render_frame()
            rgb, rad = R.read_image()
            assert np.array_equal(bits(rad), bits(_walk_ref[next_event][k][1])), (walk, k)
            assert np.array_equal(rgb, _walk_ref[next_event][k][0])
            assert st.bounce_launches == 1
    finally:
        R.set_traversal(-1)


# ------------------------------------------------------------------------------------------------
# c. radius 0 is no lens; the route of a lens; what keeps the lens and what re-derives the block
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_radius_0_after_a_lens_is_the_fresh_context(R, next_event):
    arrays, _ = TC.cornell("cbox")
    setup(R, arrays, 5, next_event)
    plain = frames(R)
    launches = plain[0][2].bounce_launches
    assert launches == 1 if next_event else launches > 1      # the sweep's launches for the reference's estimator
    R.set_lens(0.5, 4.0)
    through = frames(R)
    assert through[0][2].bounce_launches == 1                  # both estimators: the per-lane kernel
    assert not np.array_equal(bits(through[0][1]), bits(plain[0][1]))
    for off in ((0.0, None), (0.0, 4.0), (0.0, -1.0)):
        R.set_lens(0.5, 4.0)
        R.set_lens(*off)
        assert R.lens()[0] == 0.0
        again = frames(R)
        for k in range(2):
            assert np.array_equal(bits(again[k][1]), bits(plain[k][1])), (off, k)
            assert np.array_equal(again[k][0], plain[k][0])
            assert again[k][2].bounce_launches == plain[k][2].bounce_launches, off
    with pytest.raises(ptmi.PtmiError, match="no lens"):
        R.debug_lens_block()


def test_a_scene_load_keeps_the_lens(R):
    arrays, _ = TC.cornell("cbox")
    quads, _ = TC.cornell("cbox_quads")
    setup(R, quads, 3, True)
    R.set_lens(1.0, 8.5)
    R.render_frame()
    R.load_scene_arrays(*arrays)
    assert R.lens() == (1.0, 8.5)
    R.update_resolution(W, H)
    check_frames(R, reference(arrays, (1.0, 8.5), True), SPP, 3, frames=1)


def test_the_default_focus_distance_follows_the_camera(R):
    cam = ptmi.default_camera()
    assert R.lens() == (0.0, F(ptmi.default_focus_distance(cam)))
    cam.origin[2] = 4.0
    R.set_camera(cam)
    assert R.lens() == (0.0, F(ptmi.default_focus_distance(cam)))
    R.set_lens(0.25)                                           # the camera's distance, now the context's own
    cam.origin[2] = 6.0
    R.set_camera(cam)
    assert R.lens()[0] == 0.25 and R.lens()[1] != F(ptmi.default_focus_distance(cam))
    R.set_lens(0.0)                                            # no lens: the default again
    assert R.lens() == (0.0, F(ptmi.default_focus_distance(cam)))


def test_camera_and_resolution_re_derive_the_block(R):
    arrays, _ = TC.cornell("cbox")
    setup(R, arrays, 3, True)
    lens = (0.3, 5.0)
    R.set_lens(*lens)
    cam = ptmi.default_camera()
    assert np.array_equal(bits(R.debug_lens_block()), bits(ptmi.host_lens_block(cam, W, H, *lens)))
    R.render_frame()
    cam.yaw_deg, cam.pitch_deg, cam.vfov_deg = 70.0, 10.0, 55.0
    R.set_camera(cam)
    assert R.lens() == (F(0.3), 5.0)
    assert np.array_equal(bits(R.debug_lens_block()), bits(ptmi.host_lens_block(cam, W, H, *lens)))
    R.update_resolution(W, H)                                  # freshly seeded streams, as the restatement's
    check_frames(R, reference(arrays, lens, True, cam=ocam(cam)), SPP, 3, frames=1)     # and the frame after it uses that block
    R.update_resolution(40, 24)
    assert R.lens() == (F(0.3), 5.0)
    assert np.array_equal(bits(R.debug_lens_block()), bits(ptmi.host_lens_block(cam, 40, 24, *lens)))
    fixed = ptmi.default_camera(); fixed.orbit = 0
    R.set_camera(fixed)
    assert np.array_equal(bits(R.debug_lens_block()), bits(ptmi.host_lens_block(fixed, 40, 24, *lens)))
    R.set_lens(0.3, 7.0)
    assert np.array_equal(bits(R.debug_lens_block()), bits(ptmi.host_lens_block(fixed, 40, 24, 0.3, 7.0)))


# ------------------------------------------------------------------------------------------------
# d. every way a context renders gives the plain frame of the same sample count
# ------------------------------------------------------------------------------------------------
def lens_cbox(R, next_event, w=W, h=H, spp=SPP, which="cbox", lens=(0.4, 6.0)):
    arrays, _ = TC.cornell(which)
    setup(R, arrays, 5, next_event, w, h, spp=spp)
    R.set_lens(*lens)
    return arrays


@pytest.mark.parametrize("next_event", [False, True])
def test_union_of_three_ranks_is_the_single_gpu_frame(R, next_event):
    w, h = 40, 37
    lens_cbox(R, next_event, w, h)
    R.render_frame()
    rgb_whole, whole = R.read_image()
    seen = np.zeros(h, int)
    for rank in range(3):
        R.update_resolution(w, h, n_ranks=3, rank=rank, row_block=8)
        st = R.render_frame()
        assert st.bounce_launches == 1
        rgb, rad = R.read_image()
        rows = R.local_rows()
        seen[rows] += 1
        assert np.array_equal(bits(rad), bits(whole[rows]))
        assert np.array_equal(rgb, rgb_whole[rows])
    assert (seen == 1).all()


@pytest.mark.parametrize("next_event", [False, True])
def test_a_batch_of_three_equals_separate_frames(R, next_event):
    lens_cbox(R, next_event, which="cbox_quads")
    singles = [f[:2] for f in frames(R, 3)]
    R.update_resolution(W, H)
    st = R.render_frames(3)
    assert st.samples == 3 * W * H * SPP and st.bounce_launches == 1
    for k in (1, 0, 2):
        R.select_frame(k)
        rgb, rad = R.read_image()
        assert np.array_equal(bits(rad), bits(singles[k][1])), k
        assert np.array_equal(rgb, singles[k][0])


@pytest.mark.parametrize("next_event", [False, True])
def test_two_passes_equal_a_frame_of_their_samples(R, next_event):
    lens_cbox(R, next_event, spp=2 * SPP)
    R.render_frame()
    rgb_f, rad_f = R.read_image()
    R.update_resolution(W, H)
    R.set_config(spp=SPP)
    for _ in range(2):
        R.accum_pass()
    rgb, rad = R.read_image()
    assert np.array_equal(bits(rad), bits(rad_f))
    assert np.array_equal(rgb, rgb_f)


# ------------------------------------------------------------------------------------------------
# e. what the lens does not touch, and what setting it drops
# ------------------------------------------------------------------------------------------------
def test_the_guides_stay_the_pinhole_s_and_the_filters_run(R):
    w, h = 48, 40
    arrays, _ = TC.cornell("cbox")
    setup(R, arrays, 5, True, w, h, spp=4)
    p = ptmi.default_denoise_params()
    R.render_features(p.feature_grid)
    pinhole = R.features()
    R.set_config(integrator=1, next_event=False)
    R.render_frame()
    view = R.read_image()[1]
    R.set_config(integrator=0, next_event=True)
    R.set_lens(0.5, 6.0)
    with pytest.raises(ptmi.PtmiError):                        # the lens made the image stale
        R.denoise()
    R.render_frame()
    _, rad = R.read_image()
    drgb, drad = R.denoise()
    f = R.features()
    for key in ("albedo", "normal", "position", "hit_fraction"):
        assert np.array_equal(bits(f[key]), bits(pinhole[key])), key
    exp = DO.denoise(rad, f, p.iterations, p.sigma_color, p.color_floor, sigma_x_auto(R), p.normal_squarings, bool(p.demodulate))
    assert np.array_equal(bits(drad), bits(exp))
    assert np.array_equal(drgb, tone_map(exp))
    R.denoise_variance()
    # the temporal step on those guides: the restatement's, from an empty history
    tp = ptmi.default_temporal_params()
    b = R.scene_bvh()
    sx = TO.auto_sigma_position(b["bmin"][0], b["bmax"][0])
    hist = None
    for _ in range(2):
        R.render_frame()
        _, rad = R.read_image()
        _, out, st = R.temporal_accumulate()
        g = R.features()
        for key in ("albedo", "normal", "position", "hit_fraction"):
            assert np.array_equal(bits(g[key]), bits(pinhole[key])), key
        exp, hist, (acc, rej, mis) = TO.step(hist, rad, 4, g, R.camera_frame(), tp.max_history, tp.normal_min, sx, tp.sigma_albedo)
        assert np.array_equal(bits(out), bits(exp))
        assert (st.accepted, st.rejected, st.missed) == (acc, rej, mis)
    assert st.accepted > 0
    R.set_config(integrator=1, next_event=False)               # the Radiosity view keeps the pinhole
    R.update_resolution(w, h)                                  # (the streams it had before the lens)
    R.render_frame()
    assert np.array_equal(bits(R.read_image()[1]), bits(view))


def test_setting_the_lens_drops_what_setting_the_camera_drops(R):
    arrays, _ = TC.cornell("cbox")

    def state_after(change):
        setup(R, arrays, 5, True, spp=2)
        R.set_lens(0.2, 5.0)
        R.accum_pass(); R.accum_pass()
        assert (R.sample_counts() == 4).all()
        R.denoise_variance(iterations=1)
        R.temporal_accumulate()
        history = R.history_counts().copy()
        assert history.max() > 0
        change()
        dropped = {}
        for name, call in (("features", R.features), ("variance", R.variance), ("denoise", R.denoise)):
            try:
                call(); dropped[name] = False
            except ptmi.PtmiError:
                dropped[name] = True
        dropped["history"] = not np.array_equal(R.history_counts(), history)
        R.accum_pass()
        dropped["accumulation"] = bool((R.sample_counts() == 2).all())
        return dropped
    camera = state_after(lambda: R.set_camera(ptmi.default_camera()))
    assert camera["accumulation"] and camera["features"]
    assert state_after(lambda: R.set_lens(0.2, 5.5)) == camera
    assert state_after(lambda: R.set_lens(0.0)) == camera
    same = state_after(lambda: R.set_lens(0.2, 5.0))           # the values it has: nothing is dropped
    assert not any(same.values()), same


def test_rejections_change_nothing(R):
    arrays, _ = TC.cornell("cbox")
    setup(R, arrays, 3, False, spp=2)
    R.set_lens(0.3, 5.0)
    before = frames(R, 1)[0][1]
    L = R.L
    for r, f, msg in ((np.nan, 1.0, "radius is a NaN"), (1.0, np.nan, "focus_distance is a NaN"), (0.0, np.nan, "focus_distance is a NaN"),
                      (np.inf, 1.0, "radius must be finite"), (1.0, np.inf, "focus_distance must be finite"), (-0.5, 1.0, "radius must not be negative"),
                      (0.5, 0.0, "focus_distance must be positive"), (0.5, -1.0, "focus_distance must be positive"), (0.5, 3e38, "not finite"),
                      (3e38, 1.0, "not finite")):
        assert L.ptmi_set_lens(R.h, r, f) == -1, (r, f)
        assert msg in L.ptmi_last_error().decode(), (r, f, L.ptmi_last_error())
        assert R.lens() == (F(0.3), 5.0)
    assert np.array_equal(bits(frames(R, 1)[0][1]), bits(before))
    # a lens first: the config is rejected and names the lens; the Radiosity view is allowed
    for field, value in (("sampling_mode", 3), ("fast_tree", 1)):
        with pytest.raises(ptmi.PtmiError, match="a lens is set"):
            R.set_config(**{field: value})
        R.config = ptmi.Config.from_buffer_copy(R.config); setattr(R.config, field, 0)
    R.set_config(integrator=1); R.set_config(integrator=0)
    # the config first: the lens is rejected and none is set
    R.set_lens(0.0)
    for field, value in (("sampling_mode", 3), ("fast_tree", 1)):
        R.set_config(**{field: value})
        with pytest.raises(ptmi.PtmiError, match="lens: the config has"):
            R.set_lens(0.3, 5.0)
        assert R.lens()[0] == 0.0
        R.set_config(**{field: 0})
    # a camera that makes the block overflow fails the render with the block's message
    R.set_lens(0.3, 1e37)
    wide = ptmi.default_camera(); wide.vfov_deg = 179.9
    R.set_camera(wide)
    with pytest.raises(ptmi.PtmiError, match="not finite"):
        R.render_frame()
    R.set_camera(ptmi.default_camera())
    R.render_frame()


def test_focus_distance_at_a_pixel(R):
    arrays, _ = TC.cornell("cbox")
    setup(R, arrays, 3, True)
    frame = R.camera_frame()
    for px, py in ((16, 9), (10, 9)):                          # the pixel on the axis, where the depth is the distance, and another
        o, d = ptmi.pinhole_centre_ray(frame, W, H, px, py)
        t = R.debug_first_hit(o[None], d[None])["t"][0]
        f = R.focus_distance_at(px, py)
        assert f == ptmi.depth_along_axis(frame, d, t) and 0 < f <= float(t) * (1 + 1e-6)
    assert f < 0.99 * float(t)
    with pytest.raises(ValueError):
        R.focus_distance_at(W, 0)
    cam = ptmi.default_camera(); cam.orbit = 0
    cam.origin[:] = (0.5, 3.0, 8.5); cam.lookat[:] = (0.5, 3.0, 20.0)       # looking away from the box
    R.set_camera(cam)
    with pytest.raises(ValueError, match="nothing to focus on"):
        R.focus_distance_at(16, 9)


def test_command_line_writes_a_png_focused_at_a_pixel(tmp_path):
    out = tmp_path / "lens.png"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", TC.CBOX, "--width", "33", "--height", "19",
                          "--spp", "4", "--max-depth", "5", "--aperture", "0.3", "--focus-at", "16,9", "--out", str(out)],
                         check=True, timeout=300, capture_output=True, text=True)
    assert "lens: radius 0.3, focus distance" in res.stdout, res.stdout
    assert out.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
