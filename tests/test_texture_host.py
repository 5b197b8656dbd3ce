"""Host half of the albedo texture (include/ptmi.h, "albedo texture"): ptmi_check_albedo_texture's rejections, the restatement
(tests/texture_oracle.py) against a binary64 evaluation of the same formulas, its exact cases - corners, the wrap, the seam, a
1 x 1 image, the largest s times every width, an image of all ones - and ptmi_scenes' checker and box_uvs.  No GPU."""
import numpy as np
import pytest

import ptmi
import ptmi_scenes
import smooth_cases as SC
import texture_cases as TC
import texture_oracle as TX

F = np.float32
# float32 restatement against binary64 on this file's own inputs (test_restatement_against_binary64 prints them): the largest
# absolute error of the interpolated (u, v), UVs in [-2, 3], and of the bilinear T, texels below 1.  The test holds four times these.
MEASURED = {"uv": 4.5e-6, "texel": 2.1e-7}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# the check
# ------------------------------------------------------------------------------------------------
def good(n=3):
    return np.full((3, 5, 3), 0.5, F), np.full((n, 4, 2), 0.25, F)


def test_check_accepts_the_ends_of_every_range():
    img, uv = good()
    ptmi.check_albedo_texture(img, uv)
    for filt in ("nearest", "bilinear", 0, 1):
        ptmi.check_albedo_texture(img, uv, filter=filt)
    for h, w in ((1, 1), (1, 4096), (4096, 1)):
        ptmi.check_albedo_texture(np.zeros((h, w, 3), F), uv)
    for value in (65536.0, -65536.0, 0.0, -0.0):
        t = uv.copy(); t[2, 2, 1] = value
        ptmi.check_albedo_texture(img, t)
    big = img.copy(); big[2, 4, 2] = np.finfo(F).max
    ptmi.check_albedo_texture(big, uv)                         # a texel has no upper limit but finiteness
    fourth = uv.copy(); fourth[0, 3] = np.nan
    ptmi.check_albedo_texture(img, fourth)                     # the 4th corner is not read without a type


def test_check_rejects_by_message():
    img, uv = good()
    L = ptmi.lib()

    def call(w, h, texels, filt, n, table, mask=None):
        return L.ptmi_check_albedo_texture(w, h, None if texels is None else texels.ctypes.data, filt, n,
                                           None if table is None else table.ctypes.data, None if mask is None else mask.ctypes.data)
    assert call(5, 3, img, 0, 3, uv) == 0
    for n in (0, -1):
        assert call(5, 3, img, 0, n, uv) != 0 and b"n_prims" in L.ptmi_last_error()
    assert call(5, 3, None, 0, 3, uv) != 0 and b"texels is NULL" in L.ptmi_last_error()
    assert call(5, 3, img, 0, 3, None) != 0 and b"uv is NULL" in L.ptmi_last_error()
    huge = np.zeros((1, 4097, 3), F)
    for w in (0, -1, 4097):
        assert call(w, 1, huge, 0, 3, uv) != 0 and b"width must be 1 .. 4096" in L.ptmi_last_error()
        assert call(1, w, huge, 0, 3, uv) != 0 and b"height must be 1 .. 4096" in L.ptmi_last_error()
    for filt in (-1, 2):
        assert call(5, 3, img, filt, 3, uv) != 0 and b"filter must be 0 (nearest) or 1 (bilinear)" in L.ptmi_last_error()
    with pytest.raises(ValueError):
        ptmi.check_albedo_texture(img, uv, filter="cubic")
    for bad, msg in ((np.nan, "must be finite"), (np.inf, "must be finite"), (-np.inf, "must be finite"), (-1e-30, "must not be negative")):
        for at in ((0, 0, 0), (2, 4, 2)):                      # the first and the last component
            t = img.copy(); t[at] = bad
            with pytest.raises(ptmi.PtmiError, match="albedo texture: texel component %d %s" % (0 if at == (0, 0, 0) else 44, msg)):
                ptmi.check_albedo_texture(t, uv)
    for bad, msg in ((np.nan, "must be finite"), (np.inf, "must be finite"), (-np.inf, "must be finite"),
                     (np.nextafter(F(65536.0), F(1e9)), "exceeds 65536"), (-np.nextafter(F(65536.0), F(1e9)), "exceeds 65536")):
        for corner in range(3):
            for comp in range(2):
                t = uv.copy(); t[2, corner, comp] = bad
                with pytest.raises(ptmi.PtmiError, match="albedo texture: uv of corner %d of primitive 2 %s" % (corner, msg)):
                    ptmi.check_albedo_texture(img, t)
                ptmi.check_albedo_texture(img, t, textured=[1, 1, 0])      # of an untextured primitive: never read
    for shape in ((3, 5), (3, 5, 4)):
        with pytest.raises(ValueError):
            ptmi.check_albedo_texture(np.zeros(shape, F), uv)
    with pytest.raises(ValueError):
        ptmi.check_albedo_texture(img, np.zeros((3, 3, 2), F))
    with pytest.raises(ValueError):
        ptmi.check_albedo_texture(img, uv, textured=[1, 0])


def test_nan_uvs_on_untextured_primitives_are_accepted():
    img, uv = good(4)
    uv[1] = np.nan; uv[3] = np.inf
    ptmi.check_albedo_texture(img, uv, textured=[True, False, True, False])
    ptmi.check_albedo_texture(img, uv, textured=[5, 0, -1, 0])            # nonzero: textured
    with pytest.raises(ptmi.PtmiError, match="primitive 1"):
        ptmi.check_albedo_texture(img, uv, textured=[True, True, True, False])
    with pytest.raises(ptmi.PtmiError, match="primitive 1"):
        ptmi.check_albedo_texture(img, uv)                                  # no mask: all are textured


# ------------------------------------------------------------------------------------------------
# the restatement against binary64
# ------------------------------------------------------------------------------------------------
def uv64(v, c, ids, p):
    """binary64: the barycentric weights of p over the corners ids of v, and the UV they give"""
    v0, ea, eb = v[ids[0]], v[ids[1]] - v[ids[0]], v[ids[2]] - v[ids[0]]
    w = p - v0
    d00, d01, d11, d20, d21 = ea @ ea, ea @ eb, eb @ eb, w @ ea, w @ eb
    den = d00 * d11 - d01 * d01
    r1 = (d11 * d20 - d01 * d21) / den; r2 = (d00 * d21 - d01 * d20) / den
    return (1.0 - r1 - r2) * c[ids[0]] + r1 * c[ids[1]] + r2 * c[ids[2]]


def texel64(img, s_u, s_v):
    h, w = img.shape[:2]
    x = s_u * w - 0.5; y = s_v * h - 0.5
    x0 = np.floor(x); y0 = np.floor(y)
    fx, fy = x - x0, y - y0
    i0, j0 = int(x0) % w, int(y0) % h
    i1, j1 = (int(x0) + 1) % w, (int(y0) + 1) % h
    a = (1 - fx) * img[j0, i0] + fx * img[j0, i1]
    b = (1 - fx) * img[j1, i0] + fx * img[j1, i1]
    return (1 - fy) * a + fy * b


def test_restatement_against_binary64():
    arrays, uv, textured, index = TC.mesh()
    prims = TC.as_prims(arrays)
    rng = np.random.default_rng(21)
    worst = {"uv": 0.0, "texel": 0.0}
    for name, ids in ((SC.TRI, (0, 1, 2)), (SC.QUAD, (0, 1, 2)), (SC.QUAD, (0, 2, 3))):
        k = index[name]
        v = prims["verts"][k].astype(np.float64); c = uv[k].astype(np.float64)
        for _ in range(400):
            b = rng.dirichlet((1.0, 1.0, 1.0)) * 0.94 + 0.02                      # strictly inside the half
            p = (b[0] * v[ids[0]] + b[1] * v[ids[1]] + b[2] * v[ids[2]]).astype(F)
            got = np.array(TX.raw_uv(prims, uv, k, p), np.float64)
            worst["uv"] = max(worst["uv"], float(np.abs(got - uv64(v, c, ids, p.astype(np.float64))).max()))
    img = TC.image()
    for _ in range(2000):
        s_u, s_v = F(rng.uniform(0, 1)), F(rng.uniform(0, 1))
        got = TX.texel(img, "bilinear", s_u, s_v).astype(np.float64)
        worst["texel"] = max(worst["texel"], float(np.abs(got - texel64(img.astype(np.float64), float(s_u), float(s_v))).max()))
    print("float32 against binary64, worst absolute error: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for name in worst:
        assert 0 < worst[name] <= 4 * MEASURED[name], name


# ------------------------------------------------------------------------------------------------
# exact cases
# ------------------------------------------------------------------------------------------------
def test_a_corner_returns_the_corners_uv():
    """within the restatement's own rounding: r1, r2 at a corner are 0 or 1 up to a few ulps of the dot products, so the UV is
    the corner's up to a few ulps of the largest UV of the primitive (|uv| <= 3: 16 ulps of 4 = 4e-6)"""
    arrays, uv, textured, index = TC.mesh()
    prims = TC.as_prims(arrays)
    for name in (SC.TRI, SC.QUAD, SC.WARPED):
        k = index[name]
        for c in range(4 if prims["type"][k] == 1 else 3):
            got = np.array(TX.raw_uv(prims, uv, k, prims["verts"][k][c]), np.float64)
            assert np.abs(got - uv[k][c]).max() <= 16 * np.spacing(F(4.0)), (name, c, got, uv[k][c])
    got = TX.raw_uv(prims, uv, index[SC.TRI], prims["verts"][index[SC.TRI]][0])   # corner 0 itself: w = 0, r = 0, exact
    assert np.array_equal(bits(got), bits(uv[index[SC.TRI]][0]))


def test_degenerate_primitives_take_the_first_corners_uv():
    arrays, uv, textured, index = TC.mesh()
    prims = TC.as_prims(arrays)
    for name, p in ((SC.SLIVER, (1.5, 4.0, 0.0)), (SC.HUGE, (4.5e17, 4.5e17, 0.0))):
        k = index[name]
        assert np.array_equal(bits(TX.raw_uv(prims, uv, k, np.array(p, F))), bits(uv[k][0])), name
        s_u, s_v = TX.uv_at(prims, uv, k, np.array(p, F))
        assert 0 <= s_u < 1 and 0 <= s_v < 1


def test_the_wrap_pins_one_and_nan_to_zero():
    assert TX.wrap(F(-1e-9)) == 0 and F(-1e-9) - np.floor(F(-1e-9)) == F(1.0)        # the difference IS 1.0f
    with np.errstate(all="ignore"):
        assert TX.wrap(F(np.nan)) == 0 and TX.wrap(F(np.inf)) == 0
    assert TX.wrap(F(-0.25)) == F(0.75) and TX.wrap(F(2.5)) == F(0.5) and TX.wrap(F(65536.0)) == 0 and TX.wrap(F(-65536.0)) == 0
    assert bits(TX.wrap(F(-0.0))) == 0
    img = TC.image()
    for filt in ("nearest", "bilinear"):
        assert np.array_equal(bits(TX.texel(img, filt, TX.wrap(F(-1e-9)), TX.wrap(F(-1e-9)))), bits(TX.texel(img, filt, F(0), F(0))))
    assert np.array_equal(bits(TX.texel(img, "nearest", F(0), F(0))), bits(img[0, 0]))
    # a NaN point on a textured triangle: the weights stay NaN through the clamps, u is a NaN, s is 0: texel 0
    arrays, uv, textured, index = TC.mesh()
    prims = TC.as_prims(arrays)
    table = TX.make_table(img, uv, textured, "nearest")
    for name in (SC.TRI, SC.QUAD):
        s_u, s_v, T, tex = TX.lookup(prims, table, index[name], np.array((np.nan, 0.0, 0.0), F))
        assert tex and s_u == 0 and s_v == 0 and np.array_equal(bits(T), bits(img[0, 0])), name


def test_nearest_axes_and_rows():
    """row 0 is v in [0, 1 / height); u runs along a row: the image is 5 wide and 3 high"""
    img = TC.image()
    for j in range(3):
        for i in range(5):
            T = TX.texel(img, "nearest", F((i + 0.5) / 5), F((j + 0.5) / 3))
            assert np.array_equal(bits(T), bits(img[j, i])), (j, i)
            Tb = TX.texel(img, "bilinear", F((i + 0.5) / 5), F((j + 0.5) / 3))      # a texel centre: fx = fy = 0 up to rounding
            assert np.abs(Tb - img[j, i]).max() < 1e-6


def test_the_seam_blends_the_last_column_with_the_first():
    img = TC.image()
    s = np.nextafter(F(1.0), F(0.0))                           # just below 1
    i0, i1, fx = TX._axis_bilinear(s, 5)
    assert (i0, i1) == (4, 0) and abs(float(fx) - 0.5) < 1e-6
    j0, j1, fy = TX._axis_bilinear(F(0.5), 3)                  # the centre of row 1: fy = 0
    assert (j0, j1) == (1, 2) and fy == 0
    T = TX.texel(img, "bilinear", s, F(0.5))
    gx = F(1.0) - fx
    assert np.array_equal(bits(T), bits(F(1.0) * ((gx * img[1, 4]).astype(F) + (fx * img[1, 0]).astype(F)).astype(F) + F(0.0) * img[2, 0]))
    i0, i1, fx = TX._axis_bilinear(F(0.0), 5)                  # and just above 0: column 4 with column 0 again
    assert (i0, i1) == (4, 0) and fx == F(0.5)


def test_a_one_by_one_image():
    img = np.array([[[0.25, 0.5, 0.75]]], F)
    for filt in ("nearest", "bilinear"):
        for s_u, s_v in ((0.0, 0.0), (0.3, 0.9), (float(np.nextafter(F(1.0), F(0.0))),) * 2, (0.5, 0.5)):
            T = TX.texel(img, filt, F(s_u), F(s_v))
            if filt == "nearest":
                assert np.array_equal(bits(T), bits(img[0, 0]))
            else:
                assert np.abs(T - img[0, 0]).max() <= np.spacing(F(0.75))     # (1 - f) * t + f * t rounds


def test_no_width_at_which_s_times_width_rounds_up_to_width():
    """The largest s the wrap lets through is 1 - 2^-24.  s * width = width - width * 2^-24 lies more than half an ulp below width
    for every width that is no power of two (width * 2^-24 > 2^(k - 24) for 2^k < width < 2^(k + 1), the ulp below width being
    2^(k - 23)) and is exact for a power of two, so the rounded product stays below width for EVERY width 1 .. 4096 - checked
    here exhaustively - and the index is width - 1 before the clamp.  The clamp `i > width - 1` is a guard that this range of s
    never reaches; it is exercised with s = 1.0f, which the wrap pins to 0 and never passes on."""
    s = np.nextafter(F(1.0), F(0.0))
    widths = np.arange(1, 4097).astype(F)
    prod = (s * widths).astype(F)
    assert (prod < widths).all() and (prod.astype(np.int32) == np.arange(0, 4096)).all()
    for width in (1, 3, 5, 7, 1000, 4095, 4096):
        assert TX._axis_nearest(s, width) == width - 1
        assert TX._axis_nearest(F(1.0), width) == width - 1   # the clamp itself
        i0, i1, fx = TX._axis_bilinear(s, width)
        assert (i0, i1) == (width - 1, 0) and abs(float(fx) - 0.5) < 1e-3
    img = TC.image(width=7, height=3)
    assert np.array_equal(bits(TX.texel(img, "nearest", s, s)), bits(img[2, 6]))


def test_an_image_of_all_ones_gives_kd_bit_for_bit():
    """(1 - f) + f == 1 in binary32 for every f in [0, 1): sampled here, and the restatement's Kd(p) on random points"""
    rng = np.random.default_rng(8)
    f = np.concatenate([rng.uniform(0, 1, 1 << 20), 10.0 ** rng.uniform(-40, 0, 1 << 20), np.linspace(0.5, 1, 1 << 16, endpoint=False)]).astype(F)
    f = f[f < 1]
    assert ((F(1.0) - f) + f == F(1.0)).all()
    arrays, uv, textured, index = TC.mesh()
    prims = TC.as_prims(arrays)
    prims["bsdf"] = rng.uniform(0.0, 1.0, prims["bsdf"].shape).astype(F)
    prim, p = TC.cases(arrays, index)
    for filt in ("nearest", "bilinear"):
        for w, h in ((5, 3), (1, 1), (4, 4)):
            table = TX.make_table(np.ones((h, w, 3), F), uv, textured, filt)
            for i in range(0, len(prim), 3):
                assert np.array_equal(bits(TX.albedo(prims, table, int(prim[i]), p[i])), bits(prims["bsdf"][prim[i]])), (filt, i)


def test_an_untextured_primitive_keeps_kd():
    arrays, uv, textured, index = TC.mesh()
    prims = TC.as_prims(arrays)
    table = TX.make_table(TC.image(), uv, textured)
    k = index[TC.UNTEXTURED]
    assert np.array_equal(bits(TX.albedo(prims, table, k, prims["verts"][k][0])), bits(prims["bsdf"][k]))
    s_u, s_v, T, tex = TX.lookup(prims, table, k, prims["verts"][k][0])
    assert (s_u, s_v, tex) == (0, 0, False) and (T == 1).all()
    k = index[SC.TRI]
    assert not np.array_equal(bits(TX.albedo(prims, table, k, prims["verts"][k][0])), bits(prims["bsdf"][k]))


# ------------------------------------------------------------------------------------------------
# ptmi_scenes: checker and box_uvs
# ------------------------------------------------------------------------------------------------
def test_checker():
    a, b = (0.9, 0.8, 0.7), (0.1, 0.2, 0.3)
    img = ptmi_scenes.checker(4, a, b)
    assert img.shape == (4, 4, 3) and img.dtype == F
    for j in range(4):
        for i in range(4):
            assert np.array_equal(img[j, i], np.array(a if (i + j) % 2 == 0 else b, F))
    assert ptmi_scenes.checker(1, a, b).shape == (1, 1, 3)
    ptmi.check_albedo_texture(img, np.zeros((1, 4, 2), F))
    for bad in (0, -2):
        with pytest.raises(ValueError):
            ptmi_scenes.checker(bad, a, b)
    with pytest.raises(ValueError):
        ptmi_scenes.checker(2, (1, 2), b)


def test_box_uvs_coplanar_triangles_agree_at_shared_corners():
    arrays, parts = TC.cornell("cbox")
    prims = TC.as_prims(arrays)
    uv = ptmi_scenes.box_uvs(prims, scale=0.37, origin=(-3.0, 0.0, -6.0))
    assert uv.shape == (len(arrays[0]), 4, 2) and uv.dtype == F and np.isfinite(uv).all()
    a, b = parts["floor"]                                      # two coplanar triangles that share an edge
    shared = 0
    for ca in range(3):
        for cb in range(3):
            if np.array_equal(arrays[1][a, ca], arrays[1][b, cb]):
                shared += 1
                assert np.array_equal(bits(uv[a, ca]), bits(uv[b, cb]))
    assert shared == 2
    # the floor's normal is y: u from x, v from z
    v = arrays[1][a, 0]
    assert np.array_equal(bits(uv[a, 0]), bits(((v[[0, 2]] - np.array((-3.0, -6.0), F)) / F(0.37)).astype(F)))
    assert (uv[arrays[0] == 0, 3] == 0).all()                  # a triangle's 4th entry
    # a wall of any tessellation gets one continuous map: the subdivided box agrees with the plain one wherever a corner is shared
    sub, _ = TC.cornell("cbox_sub")
    uvs = ptmi_scenes.box_uvs(TC.as_prims(sub), scale=0.37, origin=(-3.0, 0.0, -6.0))
    corner = {tuple(arrays[1][a, c]): uv[a, c] for c in range(3)}
    seen = 0
    for k in TC.cornell("cbox_sub")[1]["floor"]:
        for c in range(3):
            key = tuple(sub[1][k, c])
            if key in corner:
                seen += 1
                assert np.array_equal(bits(uvs[k, c]), bits(corner[key]))
    assert seen >= 3
    quads, qparts = TC.cornell("cbox_quads")
    uq = ptmi_scenes.box_uvs(TC.as_prims(quads))
    assert np.array_equal(uq[qparts["floor"][0]], quads[1][qparts["floor"][0]][:, [0, 2]])
    ptmi.check_albedo_texture(ptmi_scenes.checker(2, (1, 1, 1), (0, 0, 0)), uq)
    with pytest.raises(ValueError):
        ptmi_scenes.box_uvs(prims, scale=0.0)
