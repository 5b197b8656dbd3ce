"""Vertex normals on the GPU (include/ptmi.h: "vertex normals") against the CPU restatement of the header's contract
(tests/smooth_oracle.py), bit for bit: the kernel's function per call, and frames through every way a context renders."""
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
import smooth_oracle as SM
import temporal_oracle as TO
from gpu_frames import check_frames, hidden_mirror, small_sky
from oracle_binding import OracleScene, SCENES, default_camera
from test_gpu_denoise import sigma_x_auto, tone_map

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CBOX = os.path.join(SCENES, "cbox.obj")
CBOX_QUADS = os.path.join(SCENES, "cbox_quads.obj")
W, H = 32, 24
SPP = 4
MIRROR, GLASS, ROUGH = 1, 2, 3


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture()
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


_SPHERES = {}


def spheres(which, level=1):
    """(arrays, table, ranges) of cornell_spheres on cbox / cbox_quads, built once"""
    if (which, level) not in _SPHERES:
        prims = ptmi.HostScene.load(CBOX if which == "cbox" else CBOX_QUADS).prims()
        _SPHERES[which, level] = ptmi_scenes.cornell_spheres(prims, level=level)
    return _SPHERES[which, level]


def random_table(arrays, seed=11, tilt=0.5):
    """corner normals tilted at random against the stored ones, every primitive smooth"""
    rng = np.random.default_rng(seed)
    stored = arrays[2].astype(np.float64)
    t = stored[:, None, :] + tilt * rng.normal(0, 1, (len(stored), 4, 3))
    return (t / np.linalg.norm(t, axis=2, keepdims=True)).astype(F)


def surface_kinds(ranges, n, surfaces):
    kind = np.zeros(n, np.int32)
    if surfaces == "mirror_glass":
        kind[slice(*ranges["short"])] = MIRROR; kind[slice(*ranges["tall"])] = GLASS
    elif surfaces == "rough_glass":
        kind[slice(*ranges["short"])] = ROUGH; kind[slice(*ranges["tall"])] = GLASS
    return kind


def setup(R, arrays, table, depth, next_event, w=W, h=H, spp=SPP, kind=None, rough=False, env=None):
    R.load_scene_arrays(*arrays)
    R.set_camera(ptmi.default_camera())
    R.update_resolution(w, h)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    if env is not None:
        R.set_environment(env)
    if kind is not None and kind.any():
        R.set_surfaces(kind, 1.5, 0.3 if rough else None)
    if table is not None:
        R.set_vertex_normals(table)


def reference(arrays, table, next_event, w=W, h=H, kind=None, env=None):
    return SM.SmoothRenderer(OracleScene.from_arrays(*arrays), default_camera(), w, h, table, kind=kind, env_rgb=env, next_event=next_event)


# ------------------------------------------------------------------------------------------------
# the kernel's function, per call
# ------------------------------------------------------------------------------------------------
def per_call(R, arrays, table, prim, p):
    prims = dict(type=arrays[0], verts=arrays[1], normal=arrays[2])
    got = R.debug_vertex_normal(prim, p)
    for i in range(len(prim)):
        n, smooth = SM.vertex_normal(prims, table, int(prim[i]), p[i])
        assert np.array_equal(bits(got[i, :3]), bits(n)) and got[i, 3] == (1.0 if smooth else 0.0), (i, int(prim[i]), p[i], got[i], n, smooth)
    return got


@pytest.mark.parametrize("quads", [False, True])
def test_vertex_normal_per_call_on_the_cpu_cases(R, quads):
    arrays, table, index = SC.mesh(quads)
    R.load_scene_arrays(*arrays)
    R.set_vertex_normals(table)
    assert R.vertex_normals_info() == dict(n_smooth=len(SC.smooth_names(quads)))
    prim, p = SC.cases(arrays, index)
    got = per_call(R, arrays, table, prim, p)
    for name in (SC.SLIVER, SC.ZEROS, SC.HUGE, SC.FLAT_TRI, SC.FLAT_4TH):      # fallbacks and flat primitives: the stored normal, flag 0
        m = prim == index[name]
        assert (got[m, 3] == 0).all() and np.array_equal(bits(got[m, :3]), bits(np.repeat(arrays[2][index[name]][None], m.sum(), 0))), name
    assert got[prim == index[SC.TRI], 3].all()
    # the two named fallback points, and a NaN point
    extra_prim = np.array([index[SC.CANCEL], index[SC.SLIVER], index[SC.TRI]], np.int32)
    extra_p = np.array([(1.0, 6.0, 0.0), (1.5, 4.0, 0.0), (np.nan, 0.0, 0.0)], F)
    assert (per_call(R, arrays, table, extra_prim, extra_p)[:, 3] == 0).all()
    R.set_vertex_normals(None)                                # no table: the stored normal, flag 0
    got = R.debug_vertex_normal(prim, p)
    assert (got[:, 3] == 0).all() and np.array_equal(bits(got[:, :3]), bits(arrays[2][prim]))
    with pytest.raises(ptmi.PtmiError):
        R.debug_vertex_normal(np.array([len(arrays[0])], np.int32), np.zeros((1, 3), F))


@pytest.mark.parametrize("which", ["cbox", "cbox_quads"])
def test_vertex_normal_per_call_on_random_points_of_the_spheres(R, which):
    arrays, table, ranges = spheres(which)
    R.load_scene_arrays(*arrays)
    R.set_vertex_normals(table)
    rng = np.random.default_rng(2)
    n = 4096
    prim = rng.integers(0, len(arrays[0]), n).astype(np.int32)
    w = rng.uniform(-0.2, 1.2, (n, 4)); w[arrays[0][prim] == 0, 3] = 0.0
    p = np.einsum("ij,ijk->ik", w / w.sum(1, keepdims=True), arrays[1][prim].astype(np.float64)).astype(F)
    got = per_call(R, arrays, table, prim, p)
    first = ranges["short"][0]
    assert got[prim >= first, 3].all() and not got[prim < first, 3].any()


# ------------------------------------------------------------------------------------------------
# frames, bit for bit against the restatement, first and second frame (the streams carry over)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sky", [False, True])
@pytest.mark.parametrize("surfaces", ["diffuse", "mirror_glass", "rough_glass"])
@pytest.mark.parametrize("next_event", [False, True])
@pytest.mark.parametrize("depth", [1, 3, 8])
@pytest.mark.parametrize("which", ["cbox", "cbox_quads"])
def test_cornell_spheres_17x13(R, which, depth, next_event, surfaces, sky):
    arrays, table, ranges = spheres(which)
    kind = surface_kinds(ranges, len(arrays[0]), surfaces)
    env = small_sky() if sky else None
    setup(R, arrays, table, depth, next_event, 17, 13, kind=kind, rough=surfaces == "rough_glass", env=env)
    assert R.vertex_normals_info() == dict(n_smooth=160)
    _, rad, _ = check_frames(R, reference(arrays, table, next_event, 17, 13, kind=kind, env=env), SPP, depth)
    assert rad.max() > 0


@pytest.mark.parametrize("which,walk", [("spheres0", "SWEEP"), ("spheres0_quads", "SWEEP"), ("soup", "CERTIFIED"), ("soup_quads", "CERTIFIED"),
                                        ("spheres2", "CERTIFIED"), ("deep", "STACK"), ("deep_quads", "STACK")])
@pytest.mark.parametrize("next_event", [False, True])
def test_the_other_walks(R, which, walk, next_event):
    """The Cornell box with level-1 spheres has more than 64 primitives: the certified walk.  Here are ptmi_render_nee's LANE
    walk (level-0 spheres: a scene of the sweep's size), the certified walk on soups and on level-2 spheres among quads, and the
    stack walk of a deep tree.  furnace's soups share no corner, so smooth_normals(crease_deg=180) leaves them flat - asserted
    here - and their tables are random tilts instead."""
    if which.startswith("spheres0"):
        arrays, table, _ = spheres("cbox_quads" if which.endswith("quads") else "cbox", 0)
    elif which == "soup":
        arrays = ES.soup()
    elif which == "soup_quads":
        arrays = ES.without_box("quads_many").arrays()
    elif which == "spheres2":
        arrays, table, _ = spheres("cbox_quads", 2)
    else:
        s = FN.variant(which); s.b[:12] = [(0.6, 0.5, 0.4)] * 12
        arrays = s.arrays()
    if not which.startswith("spheres"):
        prims = dict(type=arrays[0], verts=arrays[1], normal=arrays[2])
        if which.startswith("soup"):
            assert not SM.classify(prims, ptmi_scenes.smooth_normals(prims, crease_deg=180.0)).any()
        table = random_table(arrays)
    setup(R, arrays, table, 5, next_event, spp=3)
    assert R.traversal() == getattr(R, walk)
    assert R.vertex_normals_info()["n_smooth"] > 0
    check_frames(R, reference(arrays, table, next_event), 3, 5)


@pytest.mark.parametrize("next_event", [False, True])
def test_fallbacks_in_a_frame(R, next_event):
    """a box whose walls carry corner normals that cancel on one facet's edge, all-zero corner normals on another, and a
    degenerate facet in front of the camera: those vertices take the stored normal and the frame stays free of NaN"""
    s = FN.Scene(rho=(0.6, 0.5, 0.4), le=(0.0, 0.0, 0.0))
    FN.box(s, half=12.0)
    for k in (2, 3):
        s.e[k] = (4.0, 4.0, 4.0)
    s.tri((-1.0, 2.0, 0.0), (0.0, 2.0, 0.0), (2.0, 2.0, 0.0), normal=(0.0, 0.0, 1.0))       # zero area
    s.tri((-2.0, 1.0, -1.0), (3.0, 1.0, -1.0), (0.5, 5.0, -1.0))
    arrays = s.arrays()
    table = random_table(arrays)
    table[0, 0], table[0, 1], table[0, 2] = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0)     # n0 + n1 = 0 along edge 0 - 1
    table[1] = 0.0
    table[4] = 0.0; table[4, 0] = (1.0, 0.0, 0.0); table[4, 1] = (-1.0, 0.0, 0.0)                  # cancels in the middle of edge 0 - 1
    setup(R, arrays, table, 5, next_event)
    _, rad, _ = check_frames(R, reference(arrays, table, next_event), SPP, 5)
    assert np.isfinite(rad).all() and rad.max() > 0


# ------------------------------------------------------------------------------------------------
# the feature shows: a test that fails without it
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_the_spheres_show_and_nothing_else_moves(R, next_event):
    """The test that fails without the feature.  A path that can meet a sphere only at its first vertex: max_depth = 2 - the
    first vertex makes its light sample (next_event) and its BSDF sample with the normal, the second only adds what it emits.
    So the table may change a pixel only where a camera ray can hit a sphere, and it changes some of those.
    (At max_depth = 1 a sample ends after its first vertex's emission and no normal is read: no bit moves.)  At max_depth = 8
    the spheres' pixels differ for both estimators."""
    arrays, table, ranges = spheres("cbox")
    w, h = 48, 40
    setup(R, arrays, None, 2, next_event, w, h)
    R.render_features(1)
    fn = R.features()["normal"]
    # the pixels whose centre ray hits a sphere (the feature normal is a sphere facet's stored normal), widened by one pixel: the
    # frame's jittered rays stay inside their pixel
    sphere_normals = arrays[2][ranges["short"][0]:]
    on = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            on[y, x] = bool((bits(sphere_normals) == bits(fn[y, x])).all(1).any())
    near = on.copy()
    near[1:] |= on[:-1]; near[:-1] |= on[1:]; near[:, 1:] |= on[:, :-1]; near[:, :-1] |= on[:, 1:]
    near[1:, 1:] |= on[:-1, :-1]; near[:-1, :-1] |= on[1:, 1:]; near[1:, :-1] |= on[:-1, 1:]; near[:-1, 1:] |= on[1:, :-1]
    assert on.sum() > 50 and (~near).sum() > 500

    def pair(depth):
        """the frame without and with the table: which pixels differ"""
        frames = []
        for t in (None, table):
            R.set_vertex_normals(t)
            R.set_config(max_depth=depth)
            R.update_resolution(w, h)                        # freshly seeded streams
            st = R.render_frame()
            frames.append(R.read_image()[1])
        assert st.bounce_launches == 1 and R.vertex_normals_info() == dict(n_smooth=160)
        return (bits(frames[0]) != bits(frames[1])).any(2)

    changed = pair(2)
    assert not changed[~near].any()
    assert changed[on].any()                                  # (where the first vertex's light or BSDF sample found the light)
    assert not pair(1).any()
    changed = pair(8)
    assert changed[on].mean() > 0.5 if next_event else changed[on].any()


# ------------------------------------------------------------------------------------------------
# a smooth primitive that no ray can reach: the SMOOTH kernel against the kernels this change does not touch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cbox", "cbox_quads", "cbox_sub"])
@pytest.mark.parametrize("next_event", [False, True])
def test_an_unreachable_smooth_triangle_changes_no_bit(R, which, next_event):
    arrays, hidden = hidden_mirror(which)
    R.load_scene_arrays(*arrays)
    R.set_camera(ptmi.default_camera()); R.update_resolution(W, H)
    R.set_config(spp=SPP, max_depth=5, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    table = np.repeat(arrays[2][:, None, :], 4, axis=1).astype(F)
    R.set_vertex_normals(table)
    assert R.vertex_normals_info() == dict(n_smooth=0)
    plain = []
    for _ in range(2):
        R.render_frame()
        plain.append(R.read_image())
    assert R.traversal() == (R.CERTIFIED if which == "cbox_sub" else R.SWEEP)
    table[hidden, :3] = [(0.6, 0.0, 0.8), (0.0, 0.6, 0.8), (-0.6, 0.0, 0.8)]
    R.set_vertex_normals(table)
    assert R.vertex_normals_info() == dict(n_smooth=1)
    R.update_resolution(W, H)
    for k in range(2):
        st = R.render_frame()
        rgb, rad = R.read_image()
        assert st.bounce_launches == 1                        # ptmi_render_nee
        assert np.array_equal(bits(rad), bits(plain[k][1])), k
        assert np.array_equal(rgb, plain[k][0])


# ------------------------------------------------------------------------------------------------
# no table, an all-flat table, a scene load
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_all_flat_and_dropped_tables_give_the_frame_without_one(R, next_event):
    arrays, table, _ = spheres("cbox")
    setup(R, arrays, None, 5, next_event)
    plain = []
    for _ in range(2):
        R.render_frame()
        plain.append(R.read_image())
    assert R.vertex_normals_info() == dict(n_smooth=0)

    def same_as_plain(tag):
        R.update_resolution(W, H)                            # freshly seeded streams
        for k in range(2):
            R.render_frame()
            rgb, rad = R.read_image()
            assert np.array_equal(bits(rad), bits(plain[k][1])), (tag, k)
            assert np.array_equal(rgb, plain[k][0])

    flat = np.repeat(arrays[2][:, None, :], 4, axis=1).astype(F)
    flat[:, :, :][flat == 0] = -0.0                           # -0.0 == 0.0: still flat
    R.set_vertex_normals(flat)
    assert R.vertex_normals_info() == dict(n_smooth=0)
    same_as_plain("all flat")
    R.set_vertex_normals(table)
    R.render_frame()
    assert not np.array_equal(bits(R.read_image()[1]), bits(plain[0][1]))
    R.set_vertex_normals(None)
    assert R.vertex_normals_info() == dict(n_smooth=0)
    same_as_plain("dropped")


def test_a_scene_load_drops_the_table(R):
    arrays, table, _ = spheres("cbox")
    setup(R, arrays, table, 5, True)
    assert R.vertex_normals_info() == dict(n_smooth=160)
    R.render_frame()
    R.load_scene_arrays(*arrays)
    assert R.vertex_normals_info() == dict(n_smooth=0)
    R.update_resolution(W, H)
    check_frames(R, reference(arrays, np.repeat(arrays[2][:, None, :], 4, axis=1), True), SPP, 5, frames=1)
    R.set_config(fast_tree=False, next_event=False)
    R.set_config(sampling_mode=3)                             # and nothing is left that would refuse a guided mode
    R.set_config(sampling_mode=0)


# ------------------------------------------------------------------------------------------------
# tiling, batches, passes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_union_of_three_ranks_is_the_single_gpu_frame(R, next_event):
    w, h = 40, 37
    arrays, table, _ = spheres("cbox")
    setup(R, arrays, table, 5, next_event, w, h, spp=3)
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
    arrays, table, _ = spheres("cbox_quads")
    setup(R, arrays, table, 5, next_event, spp=3)
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
    arrays, table, _ = spheres("cbox")
    setup(R, arrays, table, 5, next_event, spp=spp * k)
    R.render_frame()
    rgb_f, rad_f = R.read_image()
    R.update_resolution(W, H)
    R.set_config(spp=spp)
    for _ in range(k):
        R.accum_pass()
    rgb, rad = R.read_image()
    assert np.array_equal(bits(rad), bits(rad_f))
    assert np.array_equal(rgb, rgb_f)
    R.set_vertex_normals(table)                               # a new table restarts the accumulation
    R.accum_pass()
    assert (R.sample_counts() == spp).all()


# ------------------------------------------------------------------------------------------------
# the denoiser and the temporal step take a smooth frame as any other; the features keep the stored normal
# ------------------------------------------------------------------------------------------------
def test_denoise_on_a_smooth_frame(R):
    w, h = 48, 40
    arrays, table, _ = spheres("cbox")
    setup(R, arrays, table, 5, True, w, h)
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
    R.set_vertex_normals(None)
    R.render_features(p.feature_grid)
    g = R.features()
    for key in ("albedo", "normal", "position", "hit_fraction"):     # the feature normal stays the stored one
        assert np.array_equal(bits(f[key]), bits(g[key])), key


def test_temporal_step_on_a_smooth_frame(R):
    w, h = 48, 40
    arrays, table, _ = spheres("cbox")
    setup(R, arrays, table, 5, True, w, h)
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
    R.set_vertex_normals(table)                               # other shading: the history empties
    assert (R.history_counts() == 0).all()


# ------------------------------------------------------------------------------------------------
# configuration
# ------------------------------------------------------------------------------------------------
def test_invalid_combinations_in_both_call_orders(R):
    arrays, table, _ = spheres("cbox")
    setup(R, arrays, table, 5, False, spp=2)
    base = ptmi.default_config()
    base.spp, base.max_depth = 2, 5
    R.render_frame()
    _, before = R.read_image()
    # a table first: the config is rejected and names the vertex normals
    for field, value in (("integrator", 1), ("sampling_mode", 3), ("sampling_mode", 1), ("fast_tree", 1)):
        bad = ptmi.Config.from_buffer_copy(base)
        setattr(bad, field, value)
        assert R.L.ptmi_set_config(R.h, C.byref(bad)) == -1, field
        assert "vertex normals" in R.L.ptmi_last_error().decode()
    R.update_resolution(W, H)                                # nothing changed: the same first frame again
    R.render_frame()
    assert np.array_equal(bits(R.read_image()[1]), bits(before))
    # the config first: the table is rejected, names itself, and none is set; an all-flat table is no table and passes
    R.set_vertex_normals(None)
    t = np.ascontiguousarray(table)
    flat = np.ascontiguousarray(np.repeat(arrays[2][:, None, :], 4, axis=1), F)
    for field, value in (("integrator", 1), ("sampling_mode", 3), ("fast_tree", 1)):
        cfg = ptmi.Config.from_buffer_copy(base)
        setattr(cfg, field, value)
        assert R.L.ptmi_set_config(R.h, C.byref(cfg)) == 0
        assert R.L.ptmi_set_vertex_normals(R.h, len(t), t.ctypes.data) == -1, field
        assert "vertex normals" in R.L.ptmi_last_error().decode()
        assert R.vertex_normals_info() == dict(n_smooth=0)
        assert R.L.ptmi_set_vertex_normals(R.h, len(t), flat.ctypes.data) == 0
    assert R.L.ptmi_set_config(R.h, C.byref(base)) == 0
    # a rejected table changes nothing
    R.set_vertex_normals(table)
    for bad_value in (np.nan, np.inf):
        bad = t.copy(); bad[-1, 2, 1] = bad_value
        assert R.L.ptmi_set_vertex_normals(R.h, len(t), bad.ctypes.data) == -1
    quad_scene = spheres("cbox_quads")
    assert R.L.ptmi_set_vertex_normals(R.h, len(t) - 1, t.ctypes.data) == -1
    assert "n_prims" in R.L.ptmi_last_error().decode()
    assert R.L.ptmi_set_vertex_normals(R.h, len(t) + 1, t.ctypes.data) == -1
    assert R.vertex_normals_info() == dict(n_smooth=160)
    R.update_resolution(W, H)
    R.render_frame()
    assert np.array_equal(bits(R.read_image()[1]), bits(before))
    # a quad's 4th corner is read, a triangle's is not
    fourth = t.copy(); fourth[-1, 3] = np.nan
    assert R.L.ptmi_set_vertex_normals(R.h, len(t), fourth.ctypes.data) == 0
    R.load_scene_arrays(*quad_scene[0])
    q = np.ascontiguousarray(quad_scene[1]).copy()
    assert quad_scene[0][0][0] == 1
    q[0, 3, 0] = np.inf
    assert R.L.ptmi_set_vertex_normals(R.h, len(q), q.ctypes.data) == -1
    assert "corner 3 of primitive 0" in R.L.ptmi_last_error().decode()
    fresh = ptmi.Renderer(0)
    try:
        assert fresh.L.ptmi_set_vertex_normals(fresh.h, len(t), t.ctypes.data) == -1      # no scene loaded
    finally:
        fresh.close()


def test_command_line_writes_a_png_with_a_glass_sphere(tmp_path):
    out = tmp_path / "spheres.png"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", CBOX, "--width", "32", "--height", "24",
                          "--spp", "4", "--max-depth", "8", "--next-event", "--spheres", "1", "--glass", "tall", "--out", str(out)],
                         check=True, timeout=300, capture_output=True, text=True)
    assert "0 mirror, 80 glass" in res.stdout and "vertex normals: 160 smooth primitives" in res.stdout
    assert out.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"


def test_command_line_spheres_needs_the_cornell_box():
    scene = os.path.join(ROOT, "tests", "golden", "pbrt", "01_trianglemesh.pbrt")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", scene, "--width", "16", "--height", "16",
                          "--spheres"], timeout=300, capture_output=True, text=True)
    assert res.returncode == 2 and "--spheres needs the Cornell box" in res.stderr and "Traceback" not in res.stderr
