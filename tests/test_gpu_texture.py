"""The albedo texture on the GPU (include/ptmi.h: "albedo texture") against the CPU restatement of the header's contract
(tests/texture_oracle.py), bit for bit: the kernel's function per call, frames through every way a context renders, and
identities against the kernels this feature does not touch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_oracle as DO
import env_scenes as ES
import furnace as FN
import ptmi
import ptmi_scenes
import smooth_cases as SC
import temporal_oracle as TO
import texture_cases as TC
import texture_oracle as TX
from gpu_frames import check_frames, hidden_mirror, small_sky
from oracle_binding import OracleScene, default_camera
from test_gpu_denoise import sigma_x_auto, tone_map
from test_gpu_smooth import spheres

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 32, 24
SPP = 4
MIRROR, GLASS, ROUGH = 1, 2, 3
FILTERS = ("nearest", "bilinear")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture()
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def surface_kinds(parts, n, surfaces):
    kind = np.zeros(n, np.int32)
    if surfaces == "mirror_glass":
        kind[parts["short"]] = MIRROR; kind[parts["tall"]] = GLASS
    elif surfaces == "rough_glass":
        kind[parts["short"]] = ROUGH; kind[parts["tall"]] = GLASS
    return kind


def setup(R, arrays, depth, next_event, w=W, h=H, spp=SPP, kind=None, rough=False, env=None, normals=None):
    R.load_scene_arrays(*arrays)
    R.set_camera(ptmi.default_camera())
    R.update_resolution(w, h)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    if env is not None:
        R.set_environment(env)
    if kind is not None and kind.any():
        R.set_surfaces(kind, 1.5, 0.3 if rough else None)
    if normals is not None:
        R.set_vertex_normals(normals)


def reference(arrays, image, uv, filt, next_event, w=W, h=H, kind=None, env=None, textured=None, normals=None):
    scene = OracleScene.from_arrays(*arrays)
    tex = dict(image=image, uv=uv, textured=textured, filter=filt)
    if normals is not None:
        return TX.TexturedSmoothRenderer(scene, default_camera(), w, h, normals, kind=kind, env_rgb=env, next_event=next_event, **tex)
    return TX.TexturedRenderer(scene, default_camera(), w, h, kind=kind, env_rgb=env, next_event=next_event, **tex)


def plain_frames(R, w=W, h=H, n=2):
    """n consecutive frames of the context as it is, from freshly seeded streams"""
    R.update_resolution(w, h)
    out = []
    for _ in range(n):
        st = R.render_frame()
        out.append(R.read_image() + (st,))
    return out


def same_frames(R, plain, tag, launches=None, w=W, h=H):
    R.update_resolution(w, h)
    for k in range(len(plain)):
        st = R.render_frame()
        rgb, rad = R.read_image()
        assert np.array_equal(bits(rad), bits(plain[k][1])), (tag, k, int((bits(rad) != bits(plain[k][1])).sum()))
        assert np.array_equal(rgb, plain[k][0]), (tag, k)
        if launches is not None:
            assert st.bounce_launches == launches, (tag, st.bounce_launches)


# ------------------------------------------------------------------------------------------------
# a. the kernel's function, per call
# ------------------------------------------------------------------------------------------------
def per_call(R, arrays, table, prim, p):
    prims = TC.as_prims(arrays)
    got = R.debug_albedo(prim, p)
    for i in range(len(prim)):
        s_u, s_v, T, tex = TX.lookup(prims, table, int(prim[i]), p[i])
        exp = np.array([s_u, s_v, T[0], T[1], T[2], 1.0 if tex else 0.0], F)
        assert np.array_equal(bits(got[i]), bits(exp)), (i, int(prim[i]), p[i], got[i], exp)
    return got


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("quads", [False, True])
def test_albedo_per_call_on_the_edge_case_mesh(R, quads, filt):
    arrays, uv, textured, index = TC.mesh(quads)
    img = TC.image()
    R.load_scene_arrays(*arrays)
    none = R.debug_albedo(np.zeros(3, np.int32), np.zeros((3, 3), F))     # no table: zeros, ones, flag 0
    assert np.array_equal(none, np.tile(np.array([0, 0, 1, 1, 1, 0], F), (3, 1)))
    R.set_albedo_texture(img, uv, textured, filt)
    assert R.albedo_texture_info() == dict(n_textured=len(uv) - 1, width=5, height=3, filter=TX.FILTERS[filt])
    table = TX.make_table(img, uv, textured, filt)
    prim, p = TC.cases(arrays, index)
    got = per_call(R, arrays, table, prim, p)
    m = prim == index[TC.UNTEXTURED]
    assert m.any() and np.array_equal(got[m], np.tile(np.array([0, 0, 1, 1, 1, 0], F), (m.sum(), 1)))
    assert got[~m, 5].all() and (got[:, :2] >= 0).all() and (got[:, :2] < 1).all()
    for name in (SC.SLIVER, SC.HUGE):                          # no valid den: the first corner's UV
        k = index[name]
        s = np.array([TX.wrap(uv[k, 0, 0]), TX.wrap(uv[k, 0, 1])], F)
        assert np.array_equal(bits(got[prim == k, :2]), bits(np.tile(s, ((prim == k).sum(), 1)))), name
    # named points: zero area, the overflowing den, a NaN point (texel 0), corners with UVs of +-65536 (s = 0)
    k = index[TC.EDGE_UVS]
    extra_prim = np.array([index[SC.SLIVER], index[SC.HUGE], index[SC.TRI], k, k], np.int32)
    extra_p = np.array([(1.5, 4.0, 0.0), (4.5e17, 4.5e17, 0.0), (np.nan, 0.0, 0.0), arrays[1][k, 0], arrays[1][k, 1]], F)
    got = per_call(R, arrays, table, extra_prim, extra_p)
    assert (got[2:, :2] == 0).all()
    if filt == "nearest":
        assert np.array_equal(bits(got[2, 2:5]), bits(img[0, 0]))
    R.set_albedo_texture(None, None)
    assert R.albedo_texture_info() == dict(n_textured=0, width=0, height=0, filter=0)
    assert np.array_equal(R.debug_albedo(prim[:5], p[:5]), np.tile(np.array([0, 0, 1, 1, 1, 0], F), (5, 1)))
    for bad in (len(arrays[0]), -1):
        with pytest.raises(ptmi.PtmiError, match="prim out of range"):
            R.debug_albedo(np.array([bad], np.int32), np.zeros((1, 3), F))


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("which", ["cbox", "cbox_quads"])
def test_albedo_per_call_on_random_points_of_the_cornell_box(R, which, filt):
    arrays, parts = TC.cornell(which)
    n_prims = len(arrays[0])
    img, uv = TC.image(), TC.random_uvs(n_prims)
    textured = np.ones(n_prims, bool); textured[parts["emitters"]] = False
    R.load_scene_arrays(*arrays)
    R.set_albedo_texture(img, uv, textured, filt)
    rng = np.random.default_rng(2)
    n = 4096
    prim = rng.integers(0, n_prims, n).astype(np.int32)
    w = rng.uniform(-0.2, 1.2, (n, 4)); w[arrays[0][prim] == 0, 3] = 0.0
    p = np.einsum("ij,ijk->ik", w / w.sum(1, keepdims=True), arrays[1][prim].astype(np.float64)).astype(F)
    got = per_call(R, arrays, TX.make_table(img, uv, textured, filt), prim, p)
    assert np.array_equal(got[:, 5] == 1, textured[prim])


# ------------------------------------------------------------------------------------------------
# b. frames, bit for bit against the restatement, first and second frame (the streams carry over)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sky", [False, True])
@pytest.mark.parametrize("surfaces", ["diffuse", "mirror_glass", "rough_glass"])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("next_event", [False, True])
@pytest.mark.parametrize("depth", [1, 3, 8])
@pytest.mark.parametrize("which", ["cbox", "cbox_quads"])
def test_textured_cornell_box_17x13(R, which, depth, next_event, filt, surfaces, sky):
    arrays, parts = TC.cornell(which)
    n = len(arrays[0])
    img, uv = TC.image(), TC.random_uvs(n)
    kind = surface_kinds(parts, n, surfaces)
    env = small_sky() if sky else None
    setup(R, arrays, depth, next_event, 17, 13, kind=kind, rough=surfaces == "rough_glass", env=env)
    R.set_albedo_texture(img, uv, None, filt)
    assert R.albedo_texture_info() == dict(n_textured=n, width=5, height=3, filter=TX.FILTERS[filt])
    _, rad, _ = check_frames(R, reference(arrays, img, uv, filt, next_event, 17, 13, kind=kind, env=env), SPP, depth)
    assert rad.max() > 0


@pytest.mark.parametrize("which,depth,next_event,filt,surfaces,sky", [("cbox", 8, True, "bilinear", "rough_glass", True),
                                                                       ("cbox", 3, False, "nearest", "diffuse", False),
                                                                       ("cbox_quads", 8, True, "nearest", "mirror_glass", False),
                                                                       ("cbox_quads", 3, False, "bilinear", "rough_glass", True)])
def test_textured_cornell_spheres_with_corner_normals_17x13(R, which, depth, next_event, filt, surfaces, sky):
    """SMOOTH and TEX together: cornell_spheres with its corner-normal table and a texture on every primitive"""
    arrays, normals, ranges = spheres(which)
    n = len(arrays[0])
    img, uv = TC.image(), TC.random_uvs(n)
    kind = np.zeros(n, np.int32)
    if surfaces != "diffuse":
        kind[slice(*ranges["short"])] = MIRROR if surfaces == "mirror_glass" else ROUGH
        kind[slice(*ranges["tall"])] = GLASS
    env = small_sky() if sky else None
    setup(R, arrays, depth, next_event, 17, 13, kind=kind, rough=surfaces == "rough_glass", env=env, normals=normals)
    R.set_albedo_texture(img, uv, None, filt)
    assert R.vertex_normals_info() == dict(n_smooth=160) and R.albedo_texture_info()["n_textured"] == n
    check_frames(R, reference(arrays, img, uv, filt, next_event, 17, 13, kind=kind, env=env, normals=normals), SPP, depth)


@pytest.mark.parametrize("which,walk", [("small", "SWEEP"), ("small_quads", "SWEEP"), ("soup", "CERTIFIED"), ("soup_quads", "CERTIFIED"),
                                        ("deep", "STACK"), ("deep_quads", "STACK")])
@pytest.mark.parametrize("next_event", [False, True])
def test_the_other_walks(R, which, walk, next_event):
    """ptmi_render_nee's LANE walk (a scene of the sweep's size: at most 64 primitives), the certified walk on soups and the
    stack walk of a deep tree.  Half of the primitives are textured, by turns with both filters."""
    if which.startswith("small"):
        arrays, _, _ = spheres("cbox_quads" if which.endswith("quads") else "cbox", 0)
        assert len(arrays[0]) <= 64
    elif which == "soup":
        arrays = ES.soup()
    elif which == "soup_quads":
        arrays = ES.without_box("quads_many").arrays()
    else:
        s = FN.variant(which); s.b[:12] = [(0.6, 0.5, 0.4)] * 12
        arrays = s.arrays()
    n = len(arrays[0])
    img, uv = TC.image(), TC.random_uvs(n)
    textured = np.arange(n) % 2 == 0
    uv[~textured] = np.nan                                     # never read
    filt = FILTERS[int(next_event)] if which.endswith("quads") else FILTERS[1 - int(next_event)]
    setup(R, arrays, 5, next_event, spp=3)
    R.set_albedo_texture(img, uv, textured, filt)
    assert R.traversal() == getattr(R, walk)
    assert R.albedo_texture_info()["n_textured"] == int(textured.sum())
    check_frames(R, reference(arrays, img, uv, filt, next_event, textured=textured), 3, 5)


# ------------------------------------------------------------------------------------------------
# c. identities against kernels this feature does not touch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("next_event", [False, True])
@pytest.mark.parametrize("which", ["cbox", "cbox_sub"])
def test_an_image_of_all_ones_gives_the_frame_without_a_texture(R, which, next_event, filt):
    """T = 1 exactly under both filters ((1 - f) + f == 1), so Kd(p) = Kd_k bit for bit: the TEX kernel - one launch - against
    the route the context takes without a texture (the bounce kernels for the reference's estimator)"""
    arrays, _ = TC.cornell(which)
    setup(R, arrays, 5, next_event)
    plain = plain_frames(R)
    assert R.traversal() == (R.CERTIFIED if which == "cbox_sub" else R.SWEEP)
    for w, h in ((5, 3), (1, 1)):
        R.set_albedo_texture(np.ones((h, w, 3), F), TC.random_uvs(len(arrays[0])), None, filt)
        assert R.albedo_texture_info()["n_textured"] == len(arrays[0])
        same_frames(R, plain, (which, filt, w), launches=1)


@pytest.mark.parametrize("which", ["cbox", "cbox_quads", "cbox_sub"])
@pytest.mark.parametrize("next_event", [False, True])
def test_a_texture_on_an_unreachable_triangle_changes_no_bit(R, which, next_event):
    arrays, hidden = hidden_mirror(which)
    setup(R, arrays, 5, next_event)
    plain = plain_frames(R)
    n = len(arrays[0])
    textured = np.zeros(n, bool); textured[hidden] = True
    uv = np.full((n, 4, 2), np.nan, F); uv[hidden] = TC.random_uvs(1)[0]
    for filt in FILTERS:
        R.set_albedo_texture(TC.image(), uv, textured, filt)
        assert R.albedo_texture_info()["n_textured"] == 1
        same_frames(R, plain, (which, filt), launches=1)       # ptmi_render_nee paying only the 16-byte decision


@pytest.mark.parametrize("next_event", [False, True])
def test_dropped_and_all_untextured_tables_give_the_plain_frame(R, next_event):
    arrays, _ = TC.cornell("cbox")
    n = len(arrays[0])
    setup(R, arrays, 5, next_event)
    plain = plain_frames(R)
    launches = plain[0][2].bounce_launches
    img, uv = TC.image(), TC.random_uvs(n)
    R.set_albedo_texture(img, np.full((n, 4, 2), np.nan, F), np.zeros(n, bool))
    assert R.albedo_texture_info() == dict(n_textured=0, width=0, height=0, filter=0)
    same_frames(R, plain, "all untextured", launches=launches)          # the route it takes without one
    R.set_albedo_texture(img, uv)
    R.update_resolution(W, H)
    R.render_frame()
    assert not np.array_equal(bits(R.read_image()[1]), bits(plain[0][1]))
    R.set_albedo_texture(None, None)
    assert R.albedo_texture_info() == dict(n_textured=0, width=0, height=0, filter=0)
    same_frames(R, plain, "dropped", launches=launches)


# ------------------------------------------------------------------------------------------------
# d. the feature shows: a test that fails without it
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_a_checkered_floor_shows_and_nothing_else_moves(R, next_event):
    """A checker on the floor only.  At max_depth = 2 a path reads a colour only at its first vertex (the second only adds what it
    emits), so the texture may change a pixel only where a camera ray can hit the floor, and it changes some of those.  At
    max_depth = 1 a sample ends after its first vertex's emission: no bit moves.  At max_depth = 8 most floor pixels differ; that
    frame takes 64 samples per pixel, because without light samples few of a Cornell-box pixel's first four paths find the light
    at all, and a pixel that is black in both frames cannot differ.  Both checker colours are below 1, so every floor vertex
    changes its path's throughput."""
    arrays, parts = TC.cornell("cbox")
    prims = TC.as_prims(arrays)
    n = len(arrays[0])
    w, h = 48, 40
    setup(R, arrays, 2, next_event, w, h)
    R.render_features(1)
    fp = R.features()["position"]
    fn = R.features()["normal"]
    floor_normal = arrays[2][parts["floor"][0]]
    floor_y = arrays[1][parts["floor"], :3, 1]
    # the pixels whose centre ray hits the floor (the floor's stored normal at the floor's height), widened by one pixel: the
    # frame's jittered rays stay inside their pixel
    on = (bits(fn) == bits(floor_normal)).all(2) & (fp[..., 1] < floor_y.max() + 1e-3)
    near = on.copy()
    near[1:] |= on[:-1]; near[:-1] |= on[1:]; near[:, 1:] |= on[:, :-1]; near[:, :-1] |= on[:, 1:]
    near[1:, 1:] |= on[:-1, :-1]; near[:-1, :-1] |= on[1:, 1:]; near[1:, :-1] |= on[:-1, 1:]; near[:-1, 1:] |= on[1:, :-1]
    assert on.sum() > 100 and (~near).sum() > 500
    textured = np.zeros(n, bool); textured[parts["floor"]] = True
    img = ptmi_scenes.checker(4, (0.9, 0.9, 0.9), (0.2, 0.2, 0.2))
    uv = ptmi_scenes.box_uvs(prims, scale=2.0)

    def pair(depth, spp=SPP):
        """the frame without and with the texture: which pixels differ"""
        frames = []
        for on_off in (False, True):
            if on_off:
                R.set_albedo_texture(img, uv, textured, "nearest")
            else:
                R.set_albedo_texture(None, None)
            R.set_config(spp=spp, max_depth=depth, next_event=next_event)
            R.update_resolution(w, h)                        # freshly seeded streams
            st = R.render_frame()
            frames.append(R.read_image()[1])
        assert st.bounce_launches == 1 and R.albedo_texture_info()["n_textured"] == len(parts["floor"])
        return (bits(frames[0]) != bits(frames[1])).any(2)

    changed = pair(2)
    assert not changed[~near].any()
    assert changed[on].any()
    assert not pair(1).any()
    changed = pair(8, spp=64)
    assert changed[on].mean() > 0.5


# ------------------------------------------------------------------------------------------------
# e. a scene load, tiling, batches, passes, the denoiser and the temporal step
# ------------------------------------------------------------------------------------------------
def textured_cbox(R, next_event, w=W, h=H, spp=SPP, which="cbox", filt="bilinear"):
    arrays, parts = TC.cornell(which)
    n = len(arrays[0])
    img, uv = TC.image(), TC.random_uvs(n)
    textured = np.ones(n, bool); textured[parts["emitters"]] = False
    setup(R, arrays, 5, next_event, w, h, spp=spp)
    R.set_albedo_texture(img, uv, textured, filt)
    return arrays, img, uv, textured


def test_a_scene_load_drops_the_texture(R):
    arrays, img, uv, textured = textured_cbox(R, True)
    assert R.albedo_texture_info()["n_textured"] == int(textured.sum())
    R.render_frame()
    R.load_scene_arrays(*arrays)
    assert R.albedo_texture_info() == dict(n_textured=0, width=0, height=0, filter=0)
    R.update_resolution(W, H)
    check_frames(R, reference(arrays, img, uv, "nearest", True, textured=np.zeros(len(uv), bool)), SPP, 5, frames=1)
    R.set_config(fast_tree=False, next_event=False)
    R.set_config(sampling_mode=3)                             # and nothing is left that would refuse a guided mode
    R.set_config(sampling_mode=0)


@pytest.mark.parametrize("next_event", [False, True])
def test_union_of_three_ranks_is_the_single_gpu_frame(R, next_event):
    w, h = 40, 37
    arrays, img, uv, textured = textured_cbox(R, next_event, w, h, spp=3)
    check_frames(R, reference(arrays, img, uv, "bilinear", next_event, w, h, textured=textured), 3, 5, frames=1)
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
    textured_cbox(R, next_event, spp=3, which="cbox_quads", filt="nearest")
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
    arrays, img, uv, textured = textured_cbox(R, next_event, spp=spp * k)
    R.render_frame()
    rgb_f, rad_f = R.read_image()
    R.update_resolution(W, H)
    R.set_config(spp=spp)
    for _ in range(k):
        R.accum_pass()
    rgb, rad = R.read_image()
    assert np.array_equal(bits(rad), bits(rad_f))
    assert np.array_equal(rgb, rgb_f)
    R.set_albedo_texture(img, uv, textured)                   # a new texture restarts the accumulation
    R.accum_pass()
    assert (R.sample_counts() == spp).all()


def test_denoise_on_a_textured_frame(R):
    w, h = 48, 40
    arrays, img, uv, textured = textured_cbox(R, True, w, h)
    with pytest.raises(ptmi.PtmiError):                      # the new texture made the image stale
        R.denoise()
    R.render_frame()
    _, rad = R.read_image()
    drgb, drad = R.denoise()
    p = ptmi.default_denoise_params()
    f = R.features()
    exp = DO.denoise(rad, f, p.iterations, p.sigma_color, p.color_floor, sigma_x_auto(R), p.normal_squarings, bool(p.demodulate))
    assert np.array_equal(bits(drad), bits(exp))
    assert np.array_equal(drgb, tone_map(exp))
    R.set_albedo_texture(None, None)
    R.render_features(p.feature_grid)
    g = R.features()
    for key in ("albedo", "normal", "position", "hit_fraction"):     # the feature albedo stays Kd_k
        assert np.array_equal(bits(f[key]), bits(g[key])), key


def test_temporal_step_on_a_textured_frame(R):
    w, h = 48, 40
    arrays, img, uv, textured = textured_cbox(R, True, w, h)
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
    R.set_albedo_texture(img, uv, textured)                   # other colours: the history empties
    assert (R.history_counts() == 0).all()


# ------------------------------------------------------------------------------------------------
# f. configuration, the command line
# ------------------------------------------------------------------------------------------------
def test_invalid_combinations_in_both_call_orders(R):
    arrays, img, uv, textured = textured_cbox(R, False, spp=2)
    n = len(uv)
    base = ptmi.default_config()
    base.spp, base.max_depth = 2, 5
    R.render_frame()
    _, before = R.read_image()
    # a texture first: the config is rejected and names the texture
    for field, value in (("integrator", 1), ("sampling_mode", 3), ("sampling_mode", 1), ("fast_tree", 1)):
        bad = ptmi.Config.from_buffer_copy(base)
        setattr(bad, field, value)
        assert R.L.ptmi_set_config(R.h, C.byref(bad)) == -1, field
        assert "albedo texture" in R.L.ptmi_last_error().decode()
    R.update_resolution(W, H)                                # nothing changed: the same first frame again
    R.render_frame()
    assert np.array_equal(bits(R.read_image()[1]), bits(before))
    # the config first: the texture is rejected, names itself, and none is set; an all-untextured mask is no table and passes
    R.set_albedo_texture(None, None)
    mask = np.ascontiguousarray(textured, np.int32); none = np.zeros(n, np.int32)

    def set_texture(image=img, table=uv, m=mask, filt=1, count=n, w=5, h=3):
        return R.L.ptmi_set_albedo_texture(R.h, w, h, image.ctypes.data, filt, count, table.ctypes.data, m.ctypes.data)
    for field, value in (("integrator", 1), ("sampling_mode", 3), ("fast_tree", 1)):
        cfg = ptmi.Config.from_buffer_copy(base)
        setattr(cfg, field, value)
        assert R.L.ptmi_set_config(R.h, C.byref(cfg)) == 0
        assert set_texture() == -1, field
        assert "albedo texture" in R.L.ptmi_last_error().decode()
        assert R.albedo_texture_info()["n_textured"] == 0
        assert set_texture(m=none) == 0
    assert R.L.ptmi_set_config(R.h, C.byref(base)) == 0
    # a rejected texture changes nothing
    R.set_albedo_texture(img, uv, textured)
    for bad_value in (np.nan, np.inf, 65537.0):
        bad = uv.copy(); bad[-1, 2, 1] = bad_value
        assert set_texture(table=bad) == -1
    for bad_value in (np.nan, np.inf, -0.5):
        bad = img.copy(); bad[2, 4, 1] = bad_value
        assert set_texture(image=bad) == -1
    for kw in (dict(w=0), dict(w=4097), dict(h=0), dict(h=4097), dict(filt=2), dict(filt=-1)):
        assert set_texture(**kw) == -1, kw
    assert set_texture(count=n - 1) == -1 and "n_prims" in R.L.ptmi_last_error().decode()
    assert set_texture(count=n + 1) == -1
    assert R.albedo_texture_info() == dict(n_textured=int(textured.sum()), width=5, height=3, filter=1)
    R.update_resolution(W, H)
    R.render_frame()
    assert np.array_equal(bits(R.read_image()[1]), bits(before))
    # a textured quad's 4th corner is read; a triangle's is not, nor is anything of an untextured primitive
    fourth = uv.copy(); fourth[:, 3] = np.nan; fourth[~textured] = np.nan
    assert set_texture(table=fourth) == 0
    quads, _ = TC.cornell("cbox_quads")
    R.load_scene_arrays(*quads)
    q = TC.random_uvs(len(quads[0])); q[-1, 3, 0] = np.inf
    assert R.L.ptmi_set_albedo_texture(R.h, 5, 3, img.ctypes.data, 0, len(q), q.ctypes.data, None) == -1
    assert "corner 3 of primitive %d" % (len(q) - 1) in R.L.ptmi_last_error().decode()
    fresh = ptmi.Renderer(0)
    try:
        assert fresh.L.ptmi_set_albedo_texture(fresh.h, 5, 3, img.ctypes.data, 0, n, uv.ctypes.data, None) == -1      # no scene loaded
        assert "no scene loaded" in fresh.L.ptmi_last_error().decode()
    finally:
        fresh.close()


def test_command_line_writes_a_png_with_a_checker(tmp_path):
    out = tmp_path / "checker.png"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", TC.CBOX, "--width", "32", "--height", "24",
                          "--spp", "4", "--max-depth", "5", "--next-event", "--texture", "checker:4", "--texture-scale", "2",
                          "--texture-filter", "nearest", "--out", str(out)], check=True, timeout=300, capture_output=True, text=True)
    assert "albedo texture: 4 x 4, nearest, 30 textured primitives" in res.stdout, res.stdout
    assert out.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
