"""The participating medium on the GPU (include/ptmi.h: "participating medium") against the CPU restatement of the header's contract
(tests/medium_oracle.py), bit for bit: the kernel's functions per call, frames through every way a context renders, what the
medium leaves alone, and what drops it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import medium_edge as ME
import medium_oracle as MO
import ptmi
import texture_cases as TC
from gpu_frames import check_frames, small_sky
from oracle_binding import OracleScene, default_camera
from test_gpu_smooth import spheres

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 33, 19                                                  # 627 pixels: not a multiple of the block, the idx >= n exit is live
SPP = 3
MIRROR, GLASS, ROUGH = 1, 2, 3
ROOM = ((-10.0, -10.0, -10.0), (10.0, 10.0, 10.0))            # holds the camera and the whole Cornell box
INNER = ((-2.0, 0.5, -2.0), (2.0, 4.5, 2.0))                  # inside the room, in front of the camera: camera rays enter it from outside
# (lo, hi, sigma_t, albedo, g): the camera inside and outside the box, g in {0, 0.6, -0.6}, a coloured albedo
MEDIA = [ROOM + (0.15, (1.0, 1.0, 1.0), 0.0), INNER + (0.6, (0.9, 0.6, 0.3), 0.6), ROOM + (0.2, (0.8, 0.8, 0.8), -0.6), INNER + (0.5, (0.3, 0.6, 0.9), 0.0),
         ROOM + (0.1, (0.5, 0.9, 0.7), 0.6), INNER + (0.8, (1.0, 1.0, 1.0), -0.6)]


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


def reference(arrays, medium, next_event, w=W, h=H, kind=None, env=None):
    return MO.MediumRenderer(OracleScene.from_arrays(*arrays), default_camera(), w, h, kind=kind, env_rgb=env, next_event=next_event, medium=medium)


def frames(R, n=2, w=W, h=H):
    """n consecutive frames of the context as it is, from freshly seeded streams: [(rgb, radiance, stats)]"""
    R.update_resolution(w, h)
    out = []
    for _ in range(n):
        st = R.render_frame()
        out.append(R.read_image() + (st,))
    return out


# ------------------------------------------------------------------------------------------------
# a. the kernel's functions, per call
# ------------------------------------------------------------------------------------------------
def expected_call(op, blk, o, d, t_end, u):
    out = np.zeros(ptmi.MEDIUM_CALL_OUT, F)
    g = blk[1, 3]
    if op == ptmi.MEDIUM_SEGMENT:
        ok, t0, t1 = MO.segment(blk, o, d, t_end)
        out[:4] = [ok, t0, t1, MO.transmittance(blk, o, d, t_end)]
    elif op == ptmi.MEDIUM_FREE_FLIGHT:
        v, tm = MO.free_flight(blk, o, d, t_end, u)
        with np.errstate(all="ignore"):
            out[0], out[1], out[2:5] = v, tm, (o + (tm * d).astype(F)).astype(F)
    elif op == ptmi.MEDIUM_HG_VALUE:
        out[0] = MO.hg(g, u)
    else:
        c = MO.hg_cosine(g, u)
        out[0], out[1], out[2:5] = c, MO.hg(g, c), MO.hg_direction(d, c, t_end)
    return out


def per_call(R, op, cases):
    got = R.debug_medium_call(op, np.array([ME.call_inputs(*c) for c in cases], F))
    for i, (blk, o, d, t_end, u) in enumerate(cases):
        exp = expected_call(op, blk, np.asarray(o, F), np.asarray(d, F), F(t_end), F(u))
        assert np.array_equal(bits(got[i]), bits(exp)), (op, i, o, d, t_end, u, got[i], exp)
    return got


def edge_cases():
    out = []
    for sigma in ME.SIGMAS:
        for g in ME.G_VALUES:
            blk = ME.block(sigma, g)
            for k, (_, o, d, t_end, _) in enumerate(ME.SEGMENTS):
                out.append((blk, o, d, t_end, ME.EDGE_U[k % 3]))
    return out


def phase_cases(cases):
    """the same cases with what ops 2 and 3 read: a unit d, the azimuth's draw in the t_end slot"""
    rng = np.random.default_rng(9)
    out = []
    for k, (blk, o, d, t_end, u) in enumerate(cases):
        v = float(ME.curand_uniforms(rng, 1)[0]) if k % 4 else (ME.TINY, 1.0)[k % 8 == 0]
        out.append((blk, o, d, v, u))
    return out


@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_medium_functions_at_the_edges_of_their_inputs(R, op):
    cases = edge_cases()
    if op >= 2:
        cases = phase_cases(cases) + [(ME.block(0.75, g), (0, 0, 0), (0.0, 0.0, -1.0), v, c) for g in ME.G_VALUES for v in (ME.TINY, 0.25, 1.0)
                                      for c in (-1.0, 1.0, -2.0, 2.0, 0.0, ME.TINY)]
    got = per_call(R, op, cases)
    assert np.isfinite(got[:, 0]).all()
    if op == 0:
        assert set(got[:, 0]) == {0.0, 1.0} and ((got[:, 3] >= 0) & (got[:, 3] <= 1)).all()
    if op == 3:
        assert np.allclose(np.linalg.norm(got[:, 2:5].astype(np.float64), axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_medium_functions_on_random_cases(R, op):
    cases = ME.random_cases(4096)
    if op >= 2:
        cases = phase_cases(cases)
    got = per_call(R, op, cases)
    if op < 2:
        assert 1000 < got[:, 0].sum() < 4000 if op == 0 else 100 < got[:, 0].sum() < 4000


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
def test_cornell_box_in_fog_33x19(R, which, depth, next_event, variant):
    arrays, parts = TC.cornell(which)
    n = len(arrays[0])
    # every medium meets every value of every other parameter
    medium = MEDIA[(VARIANTS.index(variant) + 2 * [1, 3, 8].index(depth) + 3 * int(next_event) + int(which == "cbox_quads")) % len(MEDIA)]
    kind = surface_kinds(parts, n, variant)
    env = small_sky() if variant == "sky" else None
    setup(R, arrays, depth, next_event, kind=kind, rough=variant == "rough_glass", env=env)
    R.set_medium(*medium)
    m = R.medium()
    assert m is not None and m.sigma_t == F(medium[2]) and tuple(m.albedo) == tuple(F(x) for x in medium[3])
    ref = reference(arrays, medium, next_event, kind=kind, env=env)
    ref.trace = []
    _, rad, _ = check_frames(R, ref, SPP, depth)
    assert rad.max() > 0 or depth == 1 and not next_event and variant != "sky"
    assert any(t[0] == MO.MEDIUM for t in ref.trace)          # the case has medium vertices


@pytest.mark.parametrize("next_event", [False, True])
def test_vertex_normals_and_a_texture_in_fog(R, next_event):
    arrays, normals, ranges = spheres("cbox_quads")
    n = len(arrays[0])
    img, uv = TC.image(), TC.random_uvs(n)
    kind = np.zeros(n, np.int32)
    kind[slice(*ranges["short"])] = ROUGH; kind[slice(*ranges["tall"])] = GLASS
    setup(R, arrays, 5, next_event, 17, 13, kind=kind, rough=True, normals=normals)
    R.set_albedo_texture(img, uv, None, "bilinear")
    R.set_medium(*MEDIA[1])
    ref = MO.MediumTexturedSmoothRenderer(OracleScene.from_arrays(*arrays), default_camera(), 17, 13, normals, kind=kind, next_event=next_event,
                                          image=img, uv=uv, filter="bilinear", medium=MEDIA[1])
    check_frames(R, ref, SPP, 5)


@pytest.mark.parametrize("next_event", [False, True])
def test_fog_through_a_lens(R, next_event):
    arrays, _ = TC.cornell("cbox")
    setup(R, arrays, 5, next_event, 17, 13)
    R.set_lens(0.3, 6.0)
    R.set_medium(*MEDIA[4])
    ref = MO.MediumLensRenderer(OracleScene.from_arrays(*arrays), default_camera(), 17, 13, next_event=next_event, medium=MEDIA[4],
                                radius=0.3, focus_distance=6.0)
    check_frames(R, ref, SPP, 5)


_walk_ref = {}


@pytest.mark.parametrize("walk", ["LANE", "CERTIFIED", "STACK"])
@pytest.mark.parametrize("next_event", [False, True])
def test_the_three_walks(R, walk, next_event):
    """ptmi_render_nee's three walks, forced on one scene of 512 triangles: one restatement for all three"""
    arrays, _ = TC.cornell("cbox_sub")
    setup(R, arrays, 5, next_event, 17, 13)
    R.set_medium(*MEDIA[0])
    mode = getattr(R, walk)
    try:
        assert R.set_traversal(mode) == mode
        if next_event not in _walk_ref:
            ref = reference(arrays, MEDIA[0], next_event, 17, 13)
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
# c. sigma_t 0 is no medium; a scene load drops it
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_sigma_0_after_a_medium_is_the_fresh_context(R, next_event):
    arrays, _ = TC.cornell("cbox")
    setup(R, arrays, 5, next_event)
    assert R.medium() is None
    plain = frames(R)
    launches = plain[0][2].bounce_launches
    assert launches == 1 if next_event else launches > 1      # the sweep's launches for the reference's estimator
    R.set_medium(*MEDIA[0])
    through = frames(R)
    assert through[0][2].bounce_launches == 1                  # both estimators: the per-lane kernel
    assert not np.array_equal(bits(through[0][1]), bits(plain[0][1]))
    for off in ((None,), ROOM + (0.0, (0.5, 0.5, 0.5), 0.6), (ptmi.make_medium(INNER[0], INNER[1], 0.0),)):
        R.set_medium(*MEDIA[0])
        R.set_medium(*off)
        assert R.medium() is None
        again = frames(R)
        for k in range(2):
            assert np.array_equal(bits(again[k][1]), bits(plain[k][1])), (off, k)
            assert np.array_equal(again[k][0], plain[k][0])
            assert again[k][2].bounce_launches == plain[k][2].bounce_launches, off


def test_a_scene_load_drops_the_medium(R):
    arrays, _ = TC.cornell("cbox")
    quads, _ = TC.cornell("cbox_quads")
    setup(R, quads, 3, True)
    R.set_medium(*MEDIA[1])
    R.render_frame()
    R.load_scene_arrays(*arrays)
    assert R.medium() is None
    R.update_resolution(W, H)
    check_frames(R, reference(arrays, None, True), SPP, 3, frames=1)


# ------------------------------------------------------------------------------------------------
# d. every way a context renders gives the plain frame of the same sample count
# ------------------------------------------------------------------------------------------------
def fog_cbox(R, next_event, w=W, h=H, spp=SPP, which="cbox", medium=MEDIA[2]):
    arrays, _ = TC.cornell(which)
    setup(R, arrays, 5, next_event, w, h, spp=spp)
    R.set_medium(*medium)
    return arrays


@pytest.mark.parametrize("next_event", [False, True])
def test_union_of_three_ranks_is_the_single_gpu_frame(R, next_event):
    w, h = 40, 37
    fog_cbox(R, next_event, w, h)
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
    fog_cbox(R, next_event, which="cbox_quads", medium=MEDIA[1])
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
    fog_cbox(R, next_event, spp=2 * SPP)
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
# e. what the medium does not touch, what setting it resets, and what is refused
# ------------------------------------------------------------------------------------------------
def test_features_denoiser_and_radiosity_view_do_not_see_the_medium(R):
    w, h = 48, 40
    arrays, _ = TC.cornell("cbox")
    setup(R, arrays, 5, True, w, h, spp=4)
    p = ptmi.default_denoise_params()
    R.set_config(integrator=1, next_event=False)
    R.render_frame()
    view = R.read_image()[1]
    R.set_config(integrator=0, next_event=True)
    R.update_resolution(w, h)
    R.render_features(p.feature_grid)
    clear = R.features()
    R.render_frame()
    _, rad_clear = R.read_image()
    _, drad_clear = R.denoise()                                # the no-medium context's result
    R.set_medium(*MEDIA[0])
    f = R.features()                                           # setting the medium leaves the feature buffers alone
    for key in ("albedo", "normal", "position", "hit_fraction"):
        assert np.array_equal(bits(f[key]), bits(clear[key])), key
    with pytest.raises(ptmi.PtmiError):                        # but the image shows the scene without it
        R.denoise()
    R.render_features(p.feature_grid)                          # a new feature pass gives the same buffers
    f = R.features()
    for key in ("albedo", "normal", "position", "hit_fraction"):
        assert np.array_equal(bits(f[key]), bits(clear[key])), key
    R.render_frame()
    _, rad = R.read_image()
    assert not np.array_equal(bits(rad), bits(rad_clear))
    _, drad_fog = R.denoise()
    assert not np.array_equal(bits(drad_fog), bits(drad_clear))
    # the denoiser is the no-medium context's: on the clear image and these guides it gives the clear result
    R.debug_set_filter_inputs(rad_clear, f, p.feature_grid)
    _, drad = R.denoise()
    assert np.array_equal(bits(drad), bits(drad_clear))
    R.set_medium(*MEDIA[0])
    R.set_config(integrator=1, next_event=False)               # the Radiosity view sees vacuum
    R.update_resolution(w, h)
    R.render_frame()
    assert np.array_equal(bits(R.read_image()[1]), bits(view))


def test_setting_the_medium_restarts_an_accumulation_and_keeps_the_history(R):
    arrays, _ = TC.cornell("cbox")
    setup(R, arrays, 5, True, spp=2)
    R.set_medium(*MEDIA[0])
    R.accum_pass(); R.accum_pass()
    assert (R.sample_counts() == 4).all()
    R.temporal_accumulate()
    history = R.history_counts().copy()
    assert history.max() > 0
    feats = R.features()
    R.set_medium(*MEDIA[0])                                    # the medium it has: nothing happens
    R.accum_pass()
    assert (R.sample_counts() == 6).all()
    R.set_medium(*MEDIA[2])
    assert np.array_equal(R.history_counts(), history)
    assert np.array_equal(bits(R.features()["position"]), bits(feats["position"]))
    R.accum_pass()
    assert (R.sample_counts() == 2).all()


def test_rejections_change_nothing(R):
    arrays, _ = TC.cornell("cbox")
    fresh = ptmi.Renderer(0)
    try:
        with pytest.raises(ptmi.PtmiError, match="no scene loaded"):
            fresh.set_medium(*MEDIA[0])
        fresh.set_medium(None)
    finally:
        fresh.close()
    setup(R, arrays, 3, False, spp=2)
    R.set_medium(*MEDIA[3])
    before = frames(R, 1)[0][1]
    nan = float("nan")
    for kw, msg in ((dict(sigma_t=nan), "sigma_t is not finite"), (dict(sigma_t=-1.0), "sigma_t must not be negative"), (dict(g=0.95), r"\|g\| must not exceed 0.9"),
                    (dict(albedo=(0.5, 1.5, 0.5)), r"albedo.g must lie in \[0, 1\]"), (dict(hi=(2.0, 0.5, 2.0)), "lo.y must be below hi.y"),
                    (dict(lo=(nan, 0.5, -2.0)), "lo.x is not finite")):
        args = dict(lo=INNER[0], hi=INNER[1], sigma_t=0.5, albedo=(0.3, 0.6, 0.9), g=0.0)
        args.update(kw)
        with pytest.raises(ptmi.PtmiError, match=msg):
            R.set_medium(**args)
        assert R.medium().sigma_t == 0.5
    assert np.array_equal(bits(frames(R, 1)[0][1]), bits(before))
    # a medium first: the config is rejected and names the medium; the Radiosity view is allowed
    for field, value in (("sampling_mode", 3), ("fast_tree", 1)):
        with pytest.raises(ptmi.PtmiError, match="a medium is set"):
            R.set_config(**{field: value})
        R.config = ptmi.Config.from_buffer_copy(R.config); setattr(R.config, field, 0)
    R.set_config(integrator=1); R.set_config(integrator=0)
    # the config first: the medium is rejected and none is set
    R.set_medium(None)
    for field, value in (("sampling_mode", 3), ("fast_tree", 1)):
        R.set_config(**{field: value})
        with pytest.raises(ptmi.PtmiError, match="medium: the config has"):
            R.set_medium(*MEDIA[0])
        assert R.medium() is None
        R.set_config(**{field: 0})
    # rays now start inside the box: with quads in the scene its corners are held to the bound on ray origins
    quads, _ = TC.cornell("cbox_quads")
    setup(R, quads, 3, False, spp=2)
    with pytest.raises(ptmi.PtmiError, match="medium: with quads in the scene"):
        R.set_medium((-3e38, -1.0, -1.0), (3e38, 1.0, 1.0), 0.5)
    assert R.medium() is None
    setup(R, arrays, 3, False, spp=2)                          # triangles need no such bound
    R.set_medium((-3e38, -1.0, -1.0), (3e38, 1.0, 1.0), 0.5)


def test_command_line_renders_fog(tmp_path):
    out = tmp_path / "fog.png"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", TC.CBOX, "--width", "33", "--height", "19",
                          "--spp", "4", "--max-depth", "5", "--next-event", "--fog", "0.15", "--fog-albedo", "0.9,0.8,0.7", "--fog-g", "0.6",
                          "--out", str(out)], check=True, timeout=300, capture_output=True, text=True)
    assert "fog: sigma_t 0.15, albedo (0.9, 0.8, 0.7), g 0.6, box (" in res.stdout, res.stdout
    assert out.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", TC.CBOX, "--width", "8", "--height", "8",
                          "--spp", "1", "--fog", "0.5", "--fog-box=-1,0,-1,1,2,1", "--fog-g", "0.95"], timeout=300, capture_output=True, text=True)
    assert res.returncode != 0 and "|g| must not exceed 0.9" in res.stderr, res.stderr
