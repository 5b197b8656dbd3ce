"""Shaded features on the GPU (include/ptmi.h: "shaded features") against the CPU restatement of the header's section
(tests/shaded_features_oracle.py), bit for bit; what must not move when nothing is asked; the state rules of
ptmi_set_feature_shading; the filters and the temporal step fed the shaded buffers; a quality guard on a checkered floor; the
command line."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import denoise_oracle as DO
import ptmi
import ptmi_scenes
import shaded_features_oracle as SF
import temporal_oracle as TO
import texture_cases as TC
import texture_oracle as TX
import variance_oracle as VO
from oracle_binding import OracleScene, camera_frame, camera_ray, default_camera
from test_gpu_adaptive import _soup
from test_gpu_denoise import sigma_x_auto, tone_map
from test_gpu_smooth import random_table, spheres

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("albedo", "normal", "position", "hit_fraction")
FILTERS = ("nearest", "bilinear")
ROUGH = 3
CHECKER = ((0.9, 0.9, 0.9), (0.2, 0.2, 0.2))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b, tag=None):
    for k in KEYS:
        assert np.array_equal(bits(a[k]), bits(b[k])), (tag, k, int((bits(a[k]) != bits(b[k])).sum()))


@pytest.fixture()
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def setup(R, arrays, w, h, spp=4, depth=5, next_event=True):
    R.load_scene_arrays(*arrays)
    R.set_camera(ptmi.default_camera())
    R.update_resolution(w, h)
    R.set_config(spp=spp, max_depth=depth, sampling_mode=0, integrator=0, fast_tree=False, next_event=next_event)


def shaded(R, g, flags):
    R.set_feature_shading(flags=flags)
    R.render_features(g)
    return R.features()


# ------------------------------------------------------------------------------------------------
# the scenes of (a): arrays, the texture's table (or None) and the corner normals (or None)
# ------------------------------------------------------------------------------------------------
_SCENES, _EXPECTED = {}, {}


def scene(which, filt="bilinear"):
    """cbox / cbox_quads: textured over every non-emitter with the 5 x 3 random image and random UVs; `+normals`: corner normals
    tilted at random as well, every primitive smooth.  spheres: cornell_spheres of level 2 with its corner normals and the
    texture over everything but the emitters.  soup: 3000 floating triangles, textured with random UVs (hits and misses)."""
    if (which, filt) not in _SCENES:
        base = which.split("+")[0]
        normals = None
        if base in ("cbox", "cbox_quads"):
            arrays, _ = TC.cornell(base)
            if which.endswith("+normals"):
                normals = random_table(arrays)
        elif base == "spheres":
            arrays, normals, _ = spheres("cbox", 2)
        else:
            arrays = _soup(11)
        n = len(arrays[0])
        textured = np.asarray(arrays[4]).max(1) <= 0
        table = TX.make_table(TC.image(), TC.random_uvs(n), textured, filt)
        _SCENES[which, filt] = (arrays, table, normals, OracleScene.from_arrays(*arrays))
    return _SCENES[which, filt]


def load(R, which, filt, w, h, tables=True, **kw):
    arrays, table, normals, _ = scene(which, filt)
    setup(R, arrays, w, h, **kw)
    if tables:
        R.set_albedo_texture(table["image"], table["uv"], table["textured"], filt)
        if normals is not None:
            R.set_vertex_normals(normals)
    return arrays, table, normals


def expected(which, filt, w, h, g, flags, rows=None):
    """the restatement, computed once per case and never written to"""
    key = (which, filt if flags & 1 else None, w, h, g, flags)
    if key not in _EXPECTED:
        _, table, normals, oscene = scene(which, filt)
        _EXPECTED[key] = SF.features(oscene, default_camera(), w, h, g, flags, table, normals)
        for v in _EXPECTED[key].values():
            v.setflags(write=False)
    e = _EXPECTED[key]
    return e if rows is None else {k: v[rows] for k, v in e.items()}


# ------------------------------------------------------------------------------------------------
# a. bit-exact against the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("g", [1, 3])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("which", ["cbox", "cbox_quads", "cbox+normals", "cbox_quads+normals"])
def test_cornell_box_17x13_matches_the_restatement(R, which, filt, g, flags):
    """221 pixels: one partial workgroup, whose lanes past the image walk along.  The sweep's scenes; the quads' second half."""
    load(R, which, filt, 17, 13)
    assert R.traversal() == R.SWEEP
    got = shaded(R, g, flags)
    exp = expected(which, filt, 17, 13, g, flags)
    same(got, exp, (which, filt, g, flags))
    assert exp["hit_fraction"].min() < 1 and exp["hit_fraction"].max() == 1
    plain = expected(which, filt, 17, 13, g, 0)
    assert (flags & 1 != 0) == (not np.array_equal(bits(exp["albedo"]), bits(plain["albedo"])))
    assert (flags & 2 != 0 and which.endswith("+normals")) == (not np.array_equal(bits(exp["normal"]), bits(plain["normal"])))


@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("g", [1, 3])
@pytest.mark.parametrize("w,h", [(48, 40), (5, 3)])
def test_cornell_spheres_match_the_restatement(R, w, h, g, flags):
    """1920 pixels: 7.5 workgroups, through the certified walk; and 15 pixels"""
    _, _, normals = load(R, "spheres", "bilinear", w, h)
    assert R.traversal() == R.CERTIFIED
    assert R.vertex_normals_info()["n_smooth"] == 640
    got = shaded(R, g, flags)
    exp = expected("spheres", "bilinear", w, h, g, flags)
    same(got, exp, (w, h, g, flags))
    if (w, h) == (48, 40):
        assert exp["hit_fraction"].min() < 1 and exp["hit_fraction"].max() == 1      # hits and misses both present
        plain = expected("spheres", "bilinear", w, h, g, 0)
        assert (flags & 1 != 0) == (not np.array_equal(bits(exp["albedo"]), bits(plain["albedo"])))
        assert (flags & 2 != 0) == (not np.array_equal(bits(exp["normal"]), bits(plain["normal"])))


@pytest.mark.parametrize("filt", FILTERS)
def test_soup_with_misses_matches_the_restatement(R, filt):
    load(R, "soup", filt, 17, 13)
    assert R.traversal() == R.CERTIFIED
    exp = expected("soup", filt, 17, 13, 2, 1)
    same(shaded(R, 2, 3), exp, filt)                          # bit 1 names a table that is not there
    assert 0 < exp["hit_fraction"].mean() < 1


# ------------------------------------------------------------------------------------------------
# b. nothing moves when nothing is asked
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cbox_quads+normals", "spheres"])
def test_nothing_moves_when_nothing_is_asked(R, which):
    w, h = 17, 13
    arrays, _, _ = load(R, which, "bilinear", w, h, tables=False)
    assert R.feature_shading() == dict(albedo=False, normal=False, flags=0)
    R.render_features(2)
    bare = R.features()
    same(shaded(R, 2, 3), bare, "flags 3, no tables")
    assert R.feature_shading() == dict(albedo=True, normal=True, flags=3)
    R.set_feature_shading()
    load(R, which, "bilinear", w, h)
    assert R.albedo_texture_info()["n_textured"] > 0 and R.vertex_normals_info()["n_smooth"] > 0
    plain = shaded(R, 2, 0)
    same(plain, bare, "flags 0, both tables")
    one, two, three = shaded(R, 2, 1), shaded(R, 2, 2), shaded(R, 2, 3)
    for k in ("normal", "position", "hit_fraction"):
        assert np.array_equal(bits(one[k]), bits(plain[k])), k
    for k in ("albedo", "position", "hit_fraction"):
        assert np.array_equal(bits(two[k]), bits(plain[k])), k
    assert not np.array_equal(bits(one["albedo"]), bits(plain["albedo"]))
    assert not np.array_equal(bits(two["normal"]), bits(plain["normal"]))
    assert np.array_equal(bits(three["albedo"]), bits(one["albedo"])) and np.array_equal(bits(three["normal"]), bits(two["normal"]))


def test_frames_do_not_depend_on_the_flag(R):
    load(R, "cbox+normals", "bilinear", 17, 13)
    frames = []
    for flags in (0, 3, 0):
        R.set_feature_shading(flags=flags)
        R.update_resolution(17, 13)                            # freshly seeded streams
        st = R.render_frame()
        frames.append(R.read_image() + (st.bounce_launches,))
    for rgb, rad, launches in frames[1:]:
        assert np.array_equal(bits(rad), bits(frames[0][1])) and np.array_equal(rgb, frames[0][0])
        assert launches == frames[0][2]
    R.set_feature_shading(flags=3)                            # between two frames of one stream: the second is what it would be
    R.update_resolution(17, 13)
    R.render_frame()
    R.set_feature_shading(flags=1)
    R.render_frame()
    second = R.read_image()[1]
    R.update_resolution(17, 13)
    R.render_frame(); R.render_frame()
    assert np.array_equal(bits(R.read_image()[1]), bits(second))


# ------------------------------------------------------------------------------------------------
# c. the feature shows: these fail without it
# ------------------------------------------------------------------------------------------------
def floor_pixels(R, arrays, parts):
    """the pixels whose centre ray hits the floor (test_gpu_texture.py: test_a_checkered_floor_shows_and_nothing_else_moves), from
    the context's plain features at g = 1"""
    R.set_feature_shading()
    R.render_features(1)
    f = R.features()
    floor_normal = arrays[2][parts["floor"][0]]
    floor_y = arrays[1][parts["floor"], :3, 1]
    return (bits(f["normal"]) == bits(floor_normal)).all(2) & (f["position"][..., 1] < floor_y.max() + 1e-3), f


def checkered_floor(R, w, h, **kw):
    arrays, parts = TC.cornell("cbox")
    n = len(arrays[0])
    setup(R, arrays, w, h, **kw)
    textured = np.zeros(n, bool); textured[parts["floor"]] = True
    R.set_albedo_texture(ptmi_scenes.checker(4, *CHECKER), ptmi_scenes.box_uvs(TC.as_prims(arrays), scale=2.0), textured, "nearest")
    return arrays, parts


def test_a_checkered_floor_shows_in_the_albedo_and_nowhere_else(R):
    arrays, parts = checkered_floor(R, 48, 40)
    on, plain = floor_pixels(R, arrays, parts)
    assert on.sum() > 100 and (~on).sum() > 500
    kd = np.asarray(arrays[3], F)[parts["floor"][0]]
    got = shaded(R, 1, 1)
    light, dark = (kd * F(0.9)).astype(F), (kd * F(0.2)).astype(F)
    assert {tuple(v) for v in bits(got["albedo"][on])} == {tuple(bits(light)), tuple(bits(dark))}
    assert {tuple(v) for v in bits(plain["albedo"][on])} == {tuple(bits(kd))}
    assert np.array_equal(bits(got["albedo"][~on]), bits(plain["albedo"][~on]))
    for k in ("normal", "position", "hit_fraction"):
        assert np.array_equal(bits(got[k]), bits(plain[k])), k


def centre_prims(oscene, w, h):
    """the load-order primitive each pixel's centre ray hits, -1 for a miss (g = 1's one stratum)"""
    cf = camera_frame(default_camera(), w, h)
    out = np.full((h, w), -1, int)
    for y in range(h):
        for x in range(w):
            o, d = camera_ray(cf, (F(x) + F(0.5)) / F(w), (F(y) + F(0.5)) / F(h))
            hit = oscene.intersect(o, d, 1e-4)
            if hit.hit:
                out[y, x] = hit.prim
    return out


def test_a_ball_shows_interpolated_normals(R):
    w, h = 48, 40
    arrays, _, _, oscene = scene("spheres")
    _, _, ranges = spheres("cbox", 2)
    load(R, "spheres", "bilinear", w, h)
    prim = centre_prims(oscene, w, h)
    stored = {tuple(v) for v in bits(arrays[2])}
    for name in ("short", "tall"):
        ball = (prim >= ranges[name][0]) & (prim < ranges[name][1])
        facets = len(np.unique(prim[ball]))
        assert ball.sum() > 60 and facets > 20
        flat = shaded(R, 1, 0)["normal"][ball]
        assert all(tuple(v) in stored for v in bits(flat))
        assert len({tuple(v) for v in bits(flat)}) <= facets
        smooth = shaded(R, 1, 2)["normal"][ball]
        len2 = (smooth.astype(np.float64) ** 2).sum(1)
        assert np.abs(len2 - 1.0).max() <= 2 * 2.0 ** -23, np.abs(len2 - 1.0).max()       # 2 ulp of 1
        assert len({tuple(v) for v in bits(smooth)}) > facets


# ------------------------------------------------------------------------------------------------
# d. tiling
# ------------------------------------------------------------------------------------------------
def test_union_of_three_ranks_is_the_single_gpu_pass(R):
    w, h = 40, 37
    load(R, "spheres", "bilinear", w, h)
    whole = shaded(R, 2, 3)
    R.set_feature_shading()
    R.render_features(2)
    assert not np.array_equal(bits(whole["albedo"]), bits(R.features()["albedo"]))
    R.set_feature_shading(flags=3)
    seen = np.zeros(h, int)
    for rank in range(3):
        R.update_resolution(w, h, n_ranks=3, rank=rank, row_block=8)
        assert R.feature_shading()["flags"] == 3
        rows = R.local_rows()
        seen[rows] += 1
        R.render_features(2)
        same(R.features(), {k: v[rows] for k, v in whole.items()}, rank)
    assert (seen == 1).all()


# ------------------------------------------------------------------------------------------------
# e. the state rules
# ------------------------------------------------------------------------------------------------
def restated_denoise(R, rad):
    p = ptmi.default_denoise_params()
    return DO.denoise(rad, R.features(), p.iterations, p.sigma_color, p.color_floor, sigma_x_auto(R), p.normal_squarings, bool(p.demodulate))


def test_a_new_value_keeps_the_image_and_drops_the_features(R):
    load(R, "cbox+normals", "bilinear", 40, 32)
    R.render_frame()
    _, rad = R.read_image()
    _, first = R.denoise()
    f0 = R.features()
    assert np.array_equal(bits(first), bits(restated_denoise(R, rad)))
    R.set_feature_shading(albedo=True)
    with pytest.raises(ptmi.PtmiError, match="no current feature buffers"):
        R.features()
    _, second = R.denoise()                                   # no render in between: the image is still current
    f1 = R.features()
    assert not np.array_equal(bits(f0["albedo"]), bits(f1["albedo"]))
    assert np.array_equal(bits(f0["normal"]), bits(f1["normal"]))
    assert np.array_equal(bits(second), bits(restated_denoise(R, rad)))
    assert not np.array_equal(bits(first), bits(second))
    assert np.array_equal(bits(R.read_image()[1]), bits(rad))
    R.set_feature_shading(albedo=True)                        # the same value twice: nothing changes
    same(R.features(), f1)
    R.denoise_variance()
    R.variance()
    R.set_feature_shading(albedo=True)
    R.variance()
    R.set_feature_shading(albedo=True, normal=True)           # a new value: the variance buffers go as well
    with pytest.raises(ptmi.PtmiError, match="no current variance"):
        R.variance()


def test_a_new_value_empties_the_history_and_leaves_an_accumulation(R):
    load(R, "cbox+normals", "bilinear", 40, 32, spp=2)
    R.accum_pass(); R.accum_pass()
    counts = R.sample_counts()
    assert (counts == 4).all()
    R.temporal_accumulate()
    assert (R.history_counts() > 0).any()
    R.set_feature_shading(normal=True)
    assert (R.history_counts() == 0).all()
    assert np.array_equal(R.sample_counts(), counts)
    R.accum_pass()                                            # and the accumulation goes on
    assert (R.sample_counts() == 6).all()
    R.temporal_accumulate()
    R.set_feature_shading(normal=True)                        # the same value: the history stays
    assert (R.history_counts() > 0).any()


def test_the_flag_survives_a_scene_load_and_a_bad_flag_changes_nothing(R):
    arrays, table, normals = load(R, "cbox_quads+normals", "nearest", 17, 13)
    R.set_feature_shading(albedo=True, normal=True)
    R.render_features(1)
    before = R.features()
    for bad in (-1, 4, 8):
        with pytest.raises(ptmi.PtmiError, match="flags must be in"):
            R.set_feature_shading(flags=bad)
        assert R.feature_shading()["flags"] == 3
        same(R.features(), before, bad)                       # still readable: nothing was invalidated
    R.load_scene_arrays(*arrays)                              # drops both tables, keeps the flags
    assert R.feature_shading() == dict(albedo=True, normal=True, flags=3)
    assert R.albedo_texture_info()["n_textured"] == 0 and R.vertex_normals_info()["n_smooth"] == 0
    R.update_resolution(17, 13)
    R.render_features(1)
    same(R.features(), expected("cbox_quads+normals", "nearest", 17, 13, 1, 0), "no tables")
    R.set_albedo_texture(table["image"], table["uv"], table["textured"], "nearest")     # and they take effect with the tables
    R.set_vertex_normals(normals)
    R.render_features(1)
    same(R.features(), before, "tables back")


# ------------------------------------------------------------------------------------------------
# f. the consumers read the shaded buffers
# ------------------------------------------------------------------------------------------------
def test_denoise_and_denoise_variance_on_shaded_features(R):
    load(R, "spheres", "bilinear", 48, 40)
    R.set_feature_shading(albedo=True, normal=True)
    R.render_frame()
    _, rad = R.read_image()
    drgb, drad = R.denoise()
    f = R.features()
    same(f, expected("spheres", "bilinear", 48, 40, ptmi.default_denoise_params().feature_grid, 3))
    exp = restated_denoise(R, rad)
    assert np.array_equal(bits(drad), bits(exp))
    assert np.array_equal(drgb, tone_map(exp))
    _, vrad = R.denoise_variance()
    p = ptmi.default_variance_params()
    erad, evin, evout = VO.denoise_variance(rad, f, p.iterations, p.sigma_luminance, p.epsilon, sigma_x_auto(R), p.normal_squarings,
                                            bool(p.demodulate), p.spatial_radius, None)
    vin, vout = R.variance()
    assert np.array_equal(bits(vrad), bits(erad))
    assert np.array_equal(bits(vin), bits(evin)) and np.array_equal(bits(vout), bits(evout))


def test_temporal_steps_on_shaded_features(R):
    load(R, "spheres", "bilinear", 48, 40)
    R.set_feature_shading(albedo=True, normal=True)
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
        f = R.features()
        if view == 0:
            same(f, expected("spheres", "bilinear", 48, 40, p.feature_grid, 3))
        exp, hist, (acc, rej, mis) = TO.step(hist, rad, 4, f, frame, p.max_history, p.normal_min, sx, p.sigma_albedo)
        assert np.array_equal(bits(out), bits(exp)), view
        assert (st.accepted, st.rejected, st.missed) == (acc, rej, mis)
    assert st.accepted > 0


# ------------------------------------------------------------------------------------------------
# g. quality guard
# ------------------------------------------------------------------------------------------------
# cbox 128 x 128 with the checker of (c) on its floor, next_event, depth 5; 8 spp denoised against a 4096-spp frame of another
# seed, radiance RMSE over the floor pixels.  Measured on an MI355X: noisy 0.02091, denoised with flags 0 0.03528 (the filter
# smears the checker: worse than its input), with flag 1 0.01656, ratio 0.4694; the bound is the geometric mean of that ratio and 1.
FLOOR_RATIO = 0.685


def test_quality_guard_on_a_checkered_floor(R):
    arrays, parts = checkered_floor(R, 128, 128)
    on, _ = floor_pixels(R, arrays, parts)
    assert on.sum() > 1000
    R.set_config(spp=4096, max_depth=5, seed_base=77, next_event=True)
    R.update_resolution(128, 128)
    R.render_frame()
    _, ref = R.read_image()
    R.set_config(spp=8, max_depth=5, seed_base=2023, next_event=True)
    R.update_resolution(128, 128)
    R.render_frame()
    _, noisy = R.read_image()
    rmse = lambda a: float(np.sqrt(np.mean((a[on].astype(np.float64) - ref[on]) ** 2)))
    R.set_feature_shading()
    _, plain = R.denoise()
    R.set_feature_shading(albedo=True)
    _, textured = R.denoise()
    print(f"floor quality: noisy {rmse(noisy):.5f} flags 0 {rmse(plain):.5f} flag 1 {rmse(textured):.5f} ratio {rmse(textured) / rmse(plain):.4f}")
    assert rmse(textured) <= FLOOR_RATIO * rmse(plain)


# ------------------------------------------------------------------------------------------------
# h. the command line
# ------------------------------------------------------------------------------------------------
def read_png(path):
    """(h, w, 3) uint8 of an 8-bit RGB PNG without interlace, top row first"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            w, h, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", body)
            assert (depth, colour, interlace) == (8, 2, 0)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    out = np.zeros((h, 3 * w), np.int64)
    for y in range(h):
        kind, line = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        up = out[y - 1] if y else np.zeros(3 * w, np.int64)
        if kind == 0:
            out[y] = line
        elif kind == 2:
            out[y] = (line + up) & 255
        else:
            for i in range(3 * w):
                a = out[y, i - 3] if i >= 3 else 0
                c = up[i - 3] if i >= 3 else 0
                if kind == 1:
                    pred = a
                elif kind == 3:
                    pred = (a + up[i]) // 2
                else:
                    pa, pb, pc = abs(up[i] - c), abs(a - c), abs(a + up[i] - 2 * c)
                    pred = a if pa <= pb and pa <= pc else (up[i] if pb <= pc else c)
                out[y, i] = (line[i] + pred) & 255
    return out.astype(np.uint8).reshape(h, w, 3)


def test_command_line_writes_a_checkered_albedo(R, tmp_path):
    w, h = 48, 40
    arrays, parts = TC.cornell("cbox")
    setup(R, arrays, w, h)
    R.render_features(ptmi.default_denoise_params().feature_grid)
    f = R.features()
    floor_normal = arrays[2][parts["floor"][0]]                # pixels all of whose feature rays hit the floor
    on = (bits(f["normal"]) == bits(floor_normal)).all(2) & (f["position"][..., 1] < arrays[1][parts["floor"], :3, 1].max() + 1e-3)
    assert on.sum() > 50
    colours = {}
    for tag, extra in (("shaded", ["--shaded-features"]), ("plain", [])):
        prefix = str(tmp_path / tag)
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ptmi_render.py"), "--scene", TC.CBOX, "--width", str(w), "--height", str(h),
                              "--spp", "4", "--max-depth", "5", "--next-event", "--texture", "checker:4", "--texture-prims",
                              ",".join(str(k) for k in parts["floor"]), "--texture-filter", "nearest", "--denoise", "--aov-png", prefix,
                              "--out", prefix + ".png"] + extra, check=True, timeout=300, capture_output=True, text=True)
        assert ("shaded features: albedo on, normal on" in res.stdout) == bool(extra), res.stdout
        png = read_png(prefix + "_albedo.png")[::-1]           # the file has the top row first
        assert png.shape == (h, w, 3)
        colours[tag] = {tuple(v) for v in png[on]}
    assert len(colours["plain"]) == 1 and len(colours["shaded"]) > 1
