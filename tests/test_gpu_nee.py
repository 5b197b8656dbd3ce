"""Next-event estimation with MIS on the GPU (include/ptmi.h: ptmi_config.next_event) against the CPU restatement of the header's
contract (tests/path_oracle.py), bit for bit, and against the reference's estimator in expectation."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ptmi
import denoise_oracle as DO
from gpu_frames import check_frames
from oracle_binding import OracleScene, SCENES, default_camera
from path_oracle import NeeRenderer
from test_gpu_denoise import sigma_x_auto, tone_map

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CBOX = os.path.join(SCENES, "cbox.obj")
CBOX_QUADS = os.path.join(SCENES, "cbox_quads.obj")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def soup(seed=5, n=200):
    """about 200 triangles in front of the default camera, three emitters of very different Le (the certified walk)"""
    rng = np.random.default_rng(seed)
    centers = np.stack([rng.uniform(-3, 3, n), rng.uniform(0.2, 5.0, n), rng.uniform(-5.5, 0.5, n)], 1)[:, None, :]
    verts = (centers + rng.normal(0, 0.6, (n, 4, 3))).astype(F)
    e1 = verts[:, 1] - verts[:, 0]; e2 = verts[:, 2] - verts[:, 0]
    normal = np.cross(e1, e2); normal /= np.linalg.norm(normal, axis=1, keepdims=True)   # stored normal = plane normal
    bsdf = rng.uniform(0.2, 0.9, (n, 3)).astype(F)
    Le = np.zeros((n, 3), F)
    Le[7] = (12.0, 12.0, 12.0); Le[60] = (0.0, 3.0, 0.5); Le[150] = (40.0, 10.0, 2.0)
    return np.zeros(n, np.int32), verts, normal.astype(F), bsdf, Le


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def load(R, which):
    if which == "soup":
        arrays = soup()
        R.load_scene_arrays(*arrays)
        return OracleScene.from_arrays(*arrays)
    path = CBOX if which == "cbox" else CBOX_QUADS
    R.load_scene(path, 0)
    return OracleScene.load(path)


def setup(R, which, w, h, spp, depth, next_event=True):
    o = load(R, which)
    R.set_camera(ptmi.default_camera())
    R.update_resolution(w, h)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)
    return o


# ------------------------------------------------------------------------------------------------
# bit for bit against the restatement, first and second frame (the streams carry over)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,w,h,spp,depth", [("cbox", 32, 24, 4, 5), ("cbox_quads", 24, 24, 3, 8), ("cbox", 16, 12, 3, 1),
                                                  ("cbox", 16, 12, 3, 2), ("soup", 24, 16, 2, 5)])
def test_frames_match_the_restatement(R, which, w, h, spp, depth):
    o = setup(R, which, w, h, spp, depth)
    if which == "soup":
        assert R.traversal() == ptmi.Renderer.CERTIFIED
    ref = NeeRenderer(o, default_camera(), w, h)
    for frame in range(2):
        _, rad, st = check_frames(R, ref, spp, depth, frames=1)
        assert st.rays == 0
    assert rad.max() > 0


@pytest.mark.parametrize("name,walk", [("deep", "STACK"), ("deep_quads", "STACK"), ("quads_many", "CERTIFIED"),
                                       ("declined", None), ("emitters_4k", "CERTIFIED"), ("tilted", None), ("warped", None)])
def test_furnace_frames_match_the_restatement(R, name, walk):
    """The walks the Cornell scenes do not reach (tests/furnace.py): the stack walk with triangles and quads, the certified walk
    with quads, the reference's tree where the 8-wide builder declines, > 1000 emitters; tilted stored normals and a non-planar
    emitter quad (the geometric normal, the table's planarity rule)"""
    import furnace as FN
    w, h, spp, depth = 12, 10, 2, 5
    arrays = FN.variant(name).arrays()
    R.load_scene_arrays(*arrays)
    o = OracleScene.from_arrays(*arrays)
    R.set_camera(ptmi.default_camera())
    R.update_resolution(w, h)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=True)
    if walk:
        assert R.traversal() == getattr(R, walk)
    else:
        assert R.traversal() not in (R.STACK, R.CERTIFIED)
    if name == "emitters_4k":
        assert len(ptmi.HostScene.from_arrays(*arrays).emitters()["prim"]) >= 1000
    _, rad, _ = check_frames(R, NeeRenderer(o, default_camera(), w, h), spp, depth)
    assert rad.max() > 0


def test_without_emitters_the_frame_is_the_references(R):
    """Le whose channels sum to 0 is no emitter (w = 0) but still shines: NEE draws nothing and both frames are the reference's"""
    types, verts, normal, bsdf, Le = soup()
    Le[0::2] = (2.0, -1.0, -1.0); Le[1::2] = (0.5, 0.5, -1.0)
    arrays = (types, verts, normal, bsdf, Le)
    R.load_scene_arrays(*arrays)
    o = OracleScene.from_arrays(*arrays)
    assert len(ptmi.HostScene.from_arrays(*arrays).emitters()["prim"]) == 0
    w, h, spp, depth = 16, 12, 3, 5
    R.set_camera(ptmi.default_camera())
    R.update_resolution(w, h)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=True)
    ref = NeeRenderer(o, default_camera(), w, h)
    frames = [check_frames(R, ref, spp, depth, frames=1)[:2] for frame in range(2)]
    orgb, orad, _ = o.render(default_camera(), w, h, spp, max_depth=depth)
    assert np.array_equal(bits(frames[0][1]), bits(orad)) and np.array_equal(frames[0][0], orgb)
    R.update_resolution(w, h)                              # freshly seeded streams: the reference's estimator, two frames
    R.set_config(next_event=False)
    for frame in range(2):
        R.render_frame()
        rgb, rad = R.read_image()
        assert np.array_equal(bits(rad), bits(frames[frame][1])), frame
        assert np.array_equal(rgb, frames[frame][0])
    assert np.abs(frames[1][1]).max() > 0


def test_nee_changes_the_estimate_and_off_is_the_reference(R):
    o = setup(R, "cbox", 16, 12, 4, 5, next_event=False)
    R.render_frame()
    _, rad_pt = R.read_image()
    _, orad, _ = o.render(default_camera(), 16, 12, 4, max_depth=5)
    assert np.array_equal(bits(rad_pt), bits(orad))
    R.update_resolution(16, 12)
    R.set_config(next_event=True)
    R.render_frame()
    _, rad_nee = R.read_image()
    assert not np.array_equal(bits(rad_pt), bits(rad_nee))


# ------------------------------------------------------------------------------------------------
# tiling, batches, passes
# ------------------------------------------------------------------------------------------------
def test_union_of_three_ranks_is_the_single_gpu_frame(R):
    W, H = 40, 37
    setup(R, "cbox", W, H, 3, 5)
    R.render_frame()
    _, whole = R.read_image()
    rgb_whole, _ = R.read_image()
    seen = np.zeros(H, int)
    for rank in range(3):
        R.update_resolution(W, H, n_ranks=3, rank=rank, row_block=8)
        R.render_frame()
        rgb, rad = R.read_image()
        rows = R.local_rows()
        seen[rows] += 1
        assert np.array_equal(bits(rad), bits(whole[rows]))
        assert np.array_equal(rgb, rgb_whole[rows])
    assert (seen == 1).all()


def test_batch_equals_separate_frames(R):
    W, H = 32, 24
    setup(R, "cbox_quads", W, H, 3, 5)
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


def test_passes_equal_a_frame_of_their_samples(R):
    W, H, spp, k = 24, 20, 2, 3
    setup(R, "soup", W, H, spp * k, 5)
    R.render_frame()
    rgb_f, rad_f = R.read_image()
    R.update_resolution(W, H)                              # freshly seeded streams
    R.set_config(spp=spp)
    for _ in range(k):
        R.accum_pass()
    rgb, rad = R.read_image()
    assert np.array_equal(bits(rad), bits(rad_f))
    assert np.array_equal(rgb, rgb_f)


def test_adaptive_pixels_equal_the_frame_at_their_count(R):
    W, H, spp = 24, 20, 2
    setup(R, "cbox", W, H, spp, 5)
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


def test_denoise_of_an_nee_frame(R):
    W, H = 48, 40
    setup(R, "cbox", W, H, 4, 5)
    R.render_frame()
    _, rad = R.read_image()
    drgb, drad = R.denoise()
    p = ptmi.default_denoise_params()
    exp = DO.denoise(rad, R.features(), p.iterations, p.sigma_color, p.color_floor, sigma_x_auto(R), p.normal_squarings, bool(p.demodulate))
    assert np.array_equal(bits(drad), bits(exp))
    assert np.array_equal(drgb, tone_map(exp))


# ------------------------------------------------------------------------------------------------
# configuration
# ------------------------------------------------------------------------------------------------
def test_set_config_rejects_what_nee_does_not_cover(R):
    W, H = 16, 12
    setup(R, "cbox", W, H, 2, 5)
    R.render_frame()
    _, before = R.read_image()
    base = ptmi.default_config()
    base.spp, base.max_depth, base.next_event = 2, 5, 1
    for field, value in (("integrator", 1), ("sampling_mode", 3), ("sampling_mode", 1), ("fast_tree", 1), ("next_event", 2)):
        bad = ptmi.Config.from_buffer_copy(base)
        setattr(bad, field, value)
        assert R.L.ptmi_set_config(R.h, C.byref(bad)) == -1, field
        assert "next_event" in R.L.ptmi_last_error().decode()
    R.update_resolution(W, H)                              # the NEE config still holds: the same first frame again
    R.render_frame()
    _, after = R.read_image()
    assert np.array_equal(bits(before), bits(after))


def test_command_line_writes_a_png(tmp_path):
    out = tmp_path / "nee.png"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", CBOX, "--width", "32", "--height", "24",
                    "--spp", "4", "--next-event", "--out", str(out)], check=True, timeout=300)
    assert out.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"


# ------------------------------------------------------------------------------------------------
# unbiased, and less noisy
# ------------------------------------------------------------------------------------------------
def frame_stack(R, next_event, frames=16, spp=512, size=32):
    setup(R, "cbox", size, size, spp, 5, next_event=next_event)
    out = []
    for _ in range(frames):
        R.render_frame()
        out.append(R.read_image()[1].astype(np.float64))
    return np.stack(out)                                   # (frames, H, W, 3)


def emitter_pixels(R, size=32):
    """pixels some camera ray of which hits an emitter: their depth-0 term (identical in both estimators) dominates their noise"""
    setup(R, "cbox", size, size, 64, 1, next_event=False)
    R.render_frame()
    return (R.read_image()[1] > 0).any(axis=2)


def nee_statistics(R):
    """(max over 8x8 blocks and channels of |mean difference| / standard error, frame-to-frame variance ratio reference / NEE over
    the image, the same over the pixels that see no emitter directly)"""
    pt, nee = frame_stack(R, False), frame_stack(R, True)
    n = pt.shape[0]
    blk = lambda a: a.reshape(n, 4, 8, 4, 8, 3).mean(axis=(2, 4))            # (frames, 4, 4, 3) block means per frame
    bp, bn = blk(pt), blk(nee)
    se = np.sqrt(bp.var(axis=0, ddof=1) / n + bn.var(axis=0, ddof=1) / n)
    z = np.abs(bp.mean(0) - bn.mean(0)) / np.maximum(se, 1e-12)
    vp, vn = pt.var(axis=0, ddof=1), nee.var(axis=0, ddof=1)
    m = ~emitter_pixels(R)
    return float(z.max()), float(vp.sum() / vn.sum()), float(vp[m].sum() / vn[m].sum())


def test_unbiased_and_less_noisy(R):
    z, ratio, ratio_lit = nee_statistics(R)
    print(f"NEE vs reference estimator, cbox 32x32 depth 5, 16 x 512 spp: max block |z| {z:.2f}, variance ratio {ratio:.2f} "
          f"(pixels that see no emitter: {ratio_lit:.2f})")
    assert z < 5.0
    # Over the whole image the few pixels that cover the light's edge dominate the summed variance, and their noise is the
    # depth-0 term both estimators share (measured 1.54); where no camera ray sees an emitter, NEE's gain shows.
    assert ratio >= 1.3
    assert ratio_lit >= 2.0
