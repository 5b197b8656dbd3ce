"""The post-processing kernels (csrc/denoise.hip, denoise_variance.hip, temporal.hip) on the constructed inputs of
tests/filter_edge_sets.py, given to the context through ptmi_debug_set_filter_inputs and run through the product's own drivers.

Every comparison is bit for bit against the float32 numpy restatements (denoise_oracle, variance_oracle, temporal_oracle), a NaN
counting as equal to a NaN whatever its payload.  tests/test_filter_edge_sets_host.py proves, without a GPU, that the labelled
pixels of the sets take the branches they name.
"""
import os

import numpy as np
import pytest

import ptmi
import denoise_oracle as DO
import filter_edge_sets as FS
import temporal_oracle as TO
import variance_oracle as VO
from oracle_binding import SCENES

from test_gpu_denoise import tone_map

pytestmark = pytest.mark.gpu
F = np.float32
CBOX = os.path.join(SCENES, "cbox.obj")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    """bit for bit, NaN payloads masked to "is NaN\""""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def where_differs(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return np.argwhere(~((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))[:8].tolist()


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    r.load_scene(CBOX, 0)
    yield r
    r.close()


def fresh(R, w, h, spp=2):
    R.set_camera(ptmi.default_camera())
    R.set_config(spp=spp, max_depth=5, integrator=0)
    R.update_resolution(w, h)


def inject(R, s):
    R.debug_set_filter_inputs(s["radiance"], s["feat"], grid=2)


def check_denoise(R, s, prm):
    """ptmi_denoise on the injected set s against the restatement: radiance and rgb8"""
    full = dict(FS.DENOISE_DEFAULTS, **prm)
    drgb, drad = R.denoise(**full)
    exp = FS.restate_denoise(DO, s, prm)
    assert same(drad, exp), (prm, where_differs(drad, exp))
    assert np.array_equal(drgb, tone_map(exp)), prm
    return drad


def check_variance(R, s, prm):
    """ptmi_denoise_variance (source = 1) on the injected set s against the restatement: radiance, rgb8, variance_in, variance_out"""
    full = dict(FS.VARIANCE_DEFAULTS, source=1, **prm)
    drgb, drad = R.denoise_variance(**full)
    vin, vout = R.variance()
    erad, evin, evout = FS.restate_variance(VO, s, prm)
    assert same(vin, evin), (prm, where_differs(vin, evin))
    assert same(vout, evout), (prm, where_differs(vout, evout))
    assert same(drad, erad), (prm, where_differs(drad, erad))
    assert np.array_equal(drgb, tone_map(erad)), prm
    return drad, vin, vout


def test_the_sets_defaults_are_the_products():
    d, v = ptmi.default_denoise_params(), ptmi.default_variance_params()
    for k, x in FS.DENOISE_DEFAULTS.items():
        assert k == "sigma_position" or getattr(d, k) == x
    for k, x in FS.VARIANCE_DEFAULTS.items():
        assert k == "sigma_position" or getattr(v, k) == F(x)
    assert d.feature_grid == 2 and v.feature_grid == 2 and ptmi.default_temporal_params().feature_grid == 2


# ------------------------------------------------------------------------------------------------
# a. the a-trous family on the finite sets, every size its own launch geometry
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", FS.ATROUS_SIZES)
def test_atrous_sets_through_denoise(R, w, h):
    s = FS.atrous_set(w, h)
    fresh(R, w, h)
    inject(R, s)
    rgb, rad = R.read_image()
    assert same(rad, s["radiance"]) and np.array_equal(rgb, tone_map(s["radiance"]))
    for prm in FS.DENOISE_PARAMS:
        drad = check_denoise(R, s, prm)
        if prm.get("iterations") == 0:
            assert same(drad, s["radiance"])
    for p in s["labels"].get("miss", []):                        # the misses keep their input through the defaults' five iterations
        assert same(check_denoise(R, s, {})[p], s["radiance"][p])


@pytest.mark.parametrize("w,h", FS.ATROUS_SIZES)
def test_atrous_sets_through_denoise_variance(R, w, h):
    s = FS.atrous_set(w, h)
    fresh(R, w, h)
    inject(R, s)
    for prm in FS.VARIANCE_PARAMS:
        drad, vin, vout = check_variance(R, s, prm)
        if prm.get("iterations") == 0:
            assert same(drad, s["radiance"]) and same(vin, vout)


def test_atrous_set_with_the_scenes_own_sigma(R):
    """sigma_position = 0: 2 % of the loaded scene's diagonal"""
    s = FS.atrous_set(33, 19)
    fresh(R, 33, 19)
    inject(R, s)
    b = R.scene_bvh()
    sx = DO.auto_sigma_position(b["bmin"][0], b["bmax"][0])
    _, drad = R.denoise()
    assert same(drad, FS.restate_denoise(DO, s, dict(sigma_position=sx)))
    _, vrad = R.denoise_variance(source=1)
    assert same(vrad, FS.restate_variance(VO, s, dict(sigma_position=sx))[0])


def test_launch_geometry_the_set_in_other_workgroups(R):
    """The 15 x 17 set inside a 33 x 19 image of misses: other workgroups, other lanes, partly filled tiles.  Taps cross the
    crop's border, so each run is held against the restatement of its own image, not against the small run."""
    s = FS.pad_into(FS.atrous_set(15, 17), 33, 19, 17, 1)
    fresh(R, 33, 19)
    inject(R, s)
    for prm in ({}, dict(iterations=2), dict(normal_squarings=0)):
        check_denoise(R, s, prm)
        check_variance(R, s, prm)


@pytest.mark.parametrize("w,h", FS.WIDE_SIZES)
def test_wide_sets_through_both_filters(R, w, h):
    """16k - 1 and 16k + 1 wide: more than a thousand workgroups in x, the last one ragged, ptmi_variance_spatial's staged tile at the
    far right edge"""
    s = FS.atrous_set(w, h)
    fresh(R, w, h)
    inject(R, s)
    rgb, rad = R.read_image()
    assert same(rad, s["radiance"])
    right = (slice(None), slice(w - 40, w))                      # the tone map where the last tiles are (a Python loop per value)
    assert np.array_equal(rgb[right], tone_map(s["radiance"][right]))
    for prm in FS.WIDE_DENOISE_PARAMS:
        drgb, drad = R.denoise(**dict(FS.DENOISE_DEFAULTS, **prm))
        exp = FS.restate_denoise(DO, s, prm)
        assert same(drad, exp), (prm, where_differs(drad, exp))
        assert np.array_equal(drgb[right], tone_map(exp[right]))
    for prm in FS.WIDE_VARIANCE_PARAMS:
        drgb, drad = R.denoise_variance(**dict(FS.VARIANCE_DEFAULTS, source=1, **prm))
        vin, vout = R.variance()
        erad, evin, evout = FS.restate_variance(VO, s, prm)
        assert same(vin, evin) and same(vout, evout) and same(drad, erad), (prm, where_differs(vin, evin), where_differs(drad, erad))
        assert np.array_equal(drgb[right], tone_map(erad[right]))


# ------------------------------------------------------------------------------------------------
# b. 0 < W and W * W == 0
# ------------------------------------------------------------------------------------------------
def test_underflow_set_takes_the_two_divisions(R):
    s = FS.underflow_set()
    (p,) = s["labels"]["w_squared_underflows"]
    fresh(R, s["width"], s["height"])
    inject(R, s)
    drad, vin, vout = check_variance(R, s, FS.UNDERFLOW_PARAMS)
    assert np.isfinite(vout).all() and np.isfinite(drad).all()       # V / (W * W) would be 0 / 0 at p
    check_denoise(R, s, dict(iterations=2, normal_squarings=10, sigma_position=1e-6))


# ------------------------------------------------------------------------------------------------
# c. non-finite pixels
# ------------------------------------------------------------------------------------------------
def test_nonfinite_set(R):
    s, clean = FS.nonfinite_set()
    fresh(R, 33, 19)
    inject(R, s)
    rgb, rad = R.read_image()
    assert same(rad, s["radiance"]) and np.array_equal(rgb, tone_map(s["radiance"]))
    feat = R.features()
    assert all(same(feat[k], s["feat"][k]) for k in feat)
    drad = check_denoise(R, s, FS.NONFINITE_DENOISE)
    vrad, vin, vout = check_variance(R, s, FS.NONFINITE_VARIANCE)
    control = tuple(np.array(s["labels"]["control"]).T)
    inject(R, clean)
    crad = check_denoise(R, clean, FS.NONFINITE_DENOISE)
    cvrad, cvin, cvout = check_variance(R, clean, FS.NONFINITE_VARIANCE)
    for a, b in ((drad, crad), (vrad, cvrad), (vin, cvin), (vout, cvout)):
        assert np.isfinite(a[control]).all() and np.array_equal(bits(a[control]), bits(b[control]))
    for prm in ({}, dict(iterations=10), dict(demodulate=0)):        # and through the whole depth of the filters
        inject(R, s)
        check_denoise(R, s, prm)
        check_variance(R, s, prm)


def test_mixed_infinity_pixel(R):
    """(+Inf, -Inf, .) radiance: a NaN luminance beside a colour distance that is Inf - where the colour weight's min is fminf"""
    s = FS.mixed_infinity_set()
    (p,) = s["labels"]["plus_minus_inf_radiance"]
    fresh(R, 33, 19)
    inject(R, s)
    drad = check_denoise(R, s, dict(iterations=1))
    q = (p[0], p[1] + 1)
    assert np.isnan(drad[q][0]) and np.isnan(drad[q][1]) and np.isfinite(drad[q][2])
    for prm in ({}, dict(iterations=2), dict(demodulate=0)):
        check_denoise(R, s, prm)
        check_variance(R, s, prm)


# ------------------------------------------------------------------------------------------------
# d. the temporal step
# ------------------------------------------------------------------------------------------------
def camera(yaw):
    c = ptmi.default_camera()
    c.yaw_deg = yaw
    return c


def temporal_script(R, d, prm, rgb_too=True):
    """View A into an empty history, view B over it, view B again (still), view A over view B's history, view B into an emptied
    history: every step on the GPU and in numpy.  Returns the numpy history and the output after the second step."""
    w, h = d["width"], d["height"]
    n = w * h
    cam_a, cam_b = camera(FS.YAW_A), camera(FS.YAW_B)
    R.set_camera(cam_a)
    R.set_config(spp=FS.TEMPORAL_SPP, max_depth=5, integrator=0)
    R.update_resolution(w, h)
    kw = dict(max_history=prm["max_history"], normal_min=prm["normal_min"], sigma_x=F(prm["sigma_position"]), sigma_albedo=prm["sigma_albedo"])
    hist, second = None, None
    steps = [(cam_a, d["feat_a"], d["rad_a"], d["frame_a"]), (cam_b, d["feat_b"], d["rad_b"], d["frame_b"]), (cam_b, d["feat_b"], d["rad_c"], d["frame_b"]),
             (cam_a, d["feat_a"], d["rad_b"], d["frame_a"]), None, (cam_b, d["feat_b"], d["rad_a"], d["frame_b"])]
    for i, step in enumerate(steps):
        if step is None:
            R.update_resolution(w, h)                            # the same size: the history empties
            hist = None
            continue
        cam, feat, rad, frame = step
        R.set_camera(cam)                                        # keeps the history
        assert np.array_equal(bits(R.camera_frame()), bits(frame))          # the frames the set was aimed through
        R.debug_set_filter_inputs(rad, feat, grid=2)
        rgb, out, st = R.temporal_accumulate(**prm)
        exp, hist, stats = TO.step(hist, rad, FS.TEMPORAL_SPP, feat, frame, **kw)
        assert same(out, exp), (i, where_differs(out, exp))
        assert same(R.history_counts(), hist.count), (i, where_differs(R.history_counts(), hist.count))
        assert (st.accepted, st.rejected, st.missed) == stats, i
        assert st.accepted + st.rejected + st.missed == n        # the ballots of a last wave that is not full
        if rgb_too:
            assert np.array_equal(rgb, tone_map(exp)), i
        if i == 1:
            second = (hist, exp, stats)
            for it in (1, 3):                                    # the a-trous filter over the constructed history
                _, drad = R.denoise_temporal(iterations=it, sigma_position=FS.SIGMA_X)
                e = DO.denoise(exp, feat, it, 4.0, 2.0, F(FS.SIGMA_X), 7, True)
                assert same(drad, e), (it, where_differs(drad, e))
    return second


@pytest.mark.parametrize("w,h", FS.TEMPORAL_SIZES[1:])
@pytest.mark.parametrize("prm", [FS.TEMPORAL_PARAMS, FS.TEMPORAL_PARAMS_ZERO_ALBEDO], ids=["thresholds", "zero_albedo_history_1"])
def test_temporal_set(R, w, h, prm):
    d = FS.temporal_set(w, h)
    hist, out, stats = temporal_script(R, d, prm)
    assert min(stats) > 0                                        # accepted, rejected and missed all occur
    if prm["max_history"] == 1:
        assert (hist.count == F(FS.TEMPORAL_SPP)).all()


@pytest.mark.parametrize("prm", [FS.TEMPORAL_PARAMS, FS.TEMPORAL_PARAMS_ZERO_ALBEDO], ids=["thresholds", "zero_albedo_history_1"])
def test_temporal_set_with_nonfinite_values(R, prm):
    """a NaN and an Inf colour in the history, a NaN position and an Inf normal among the current features, a NaN current colour"""
    d = FS.temporal_nonfinite_set()
    hist, out, stats = temporal_script(R, d, prm)
    assert np.isnan(out[d["labels"]["corner_top_right"][0]][0]) and np.isfinite(hist.count).all()


@pytest.mark.parametrize("w,h", FS.WIDE_SIZES)
def test_temporal_wide(R, w, h):
    """16k - 1 and 16k + 1 wide: the outcome counts of 32766 and 32770 pixels, a last wave of 62 and of 2 lanes"""
    hist, out, stats = temporal_script(R, FS.temporal_wide_set(w, h), FS.TEMPORAL_PARAMS, rgb_too=False)
    assert sum(stats) == w * h and min(stats) > 1000


@pytest.mark.parametrize("variant", ["corner_bottom_left", "corner_top_right", "inside", "px_on_minus1", "py_on_minus1", "px_on_0", "py_on_0",
                                     "px_on_size", "py_on_size", "missed"])
def test_temporal_one_pixel(R, variant):
    temporal_script(R, FS.temporal_set(1, 1, variant), FS.TEMPORAL_PARAMS)


# ------------------------------------------------------------------------------------------------
# the hook itself
# ------------------------------------------------------------------------------------------------
def raw_hook(r, s, grid=2, **null):
    """ptmi_debug_set_filter_inputs on the C ABI: (return code, message); null=...: arguments passed as NULL"""
    a = {"radiance": np.ascontiguousarray(s["radiance"], F), "hit_fraction": np.ascontiguousarray(s["feat"]["hit_fraction"], F)}
    a.update({k: np.ascontiguousarray(s["feat"][k], F) for k in ("albedo", "normal", "position")})
    p = lambda k: None if null.get(k) else a[k].ctypes.data
    rc = r.L.ptmi_debug_set_filter_inputs(r.h, p("radiance"), p("albedo"), p("normal"), p("position"), p("hit_fraction"), int(grid))
    return rc, r.L.ptmi_last_error().decode()


def test_hook_rejections_leave_the_context_alone(R):
    W, H = 24, 16
    s = FS.atrous_set(W, H)
    fresh(R, W, H)
    R.render_frame(); R.render_frame()
    plain = R.read_image()
    fresh(R, W, H)
    R.render_frame()
    first = R.read_image()
    R.render_features(2)
    feat = R.features()
    for k in ("radiance", "albedo", "normal", "position", "hit_fraction"):
        rc, msg = raw_hook(R, s, **{k: True})
        assert rc == -1 and "NULL" in msg, k
    for grid in (0, 5, -1):
        rc, msg = raw_hook(R, s, grid=grid)
        assert rc == -1 and "grid" in msg
    assert R.L.ptmi_debug_set_filter_inputs(None, None, None, None, None, None, 2) == -1
    now = R.read_image()
    assert np.array_equal(now[0], first[0]) and np.array_equal(bits(now[1]), bits(first[1]))
    assert all(np.array_equal(bits(feat[k]), bits(v)) for k, v in R.features().items())
    R.denoise(iterations=1)                                      # the image is still current
    R.render_frame()
    after = R.read_image()
    assert np.array_equal(after[0], plain[0]) and np.array_equal(bits(after[1]), bits(plain[1]))
    # the contexts the hook refuses: the Radiosity integrator, more than one rank - and what they hold stays
    R.set_config(integrator=1)
    rc, msg = raw_hook(R, s)
    assert rc == -1 and "Radiosity" in msg
    R.set_config(integrator=0)
    R.update_resolution(W, H, n_ranks=2, rank=0, row_block=8)
    half = dict(radiance=s["radiance"][:8], feat={k: v[:8] for k, v in s["feat"].items()})
    rc, msg = raw_hook(R, half)
    assert rc == -1 and "more than one rank" in msg
    R.update_resolution(W, H)
    with pytest.raises(ptmi.PtmiError, match="no image rendered yet"):
        R.denoise()
    # no scene, then no resolution
    r2 = ptmi.Renderer(0)
    try:
        rc, msg = raw_hook(r2, s)
        assert rc == -1 and "no scene" in msg
        r2.load_scene(CBOX, 0)
        rc, msg = raw_hook(r2, s)
        assert rc == -1 and "not allocated" in msg
        r2.set_config(spp=2, max_depth=5, integrator=0)
        r2.update_resolution(W, H)
        r2.render_frame(); r2.render_frame()
        again = r2.read_image()
        assert np.array_equal(again[0], plain[0]) and np.array_equal(bits(again[1]), bits(plain[1]))
    finally:
        r2.close()


def test_hook_touches_the_image_and_the_features_alone(R):
    W, H = 24, 16
    s = FS.atrous_set(W, H)
    fresh(R, W, H)
    R.render_frame(); R.render_frame()
    plain = R.read_image()
    fresh(R, W, H)
    R.render_frame()
    inject(R, s)
    feat = R.features()                                          # what was injected is what the context holds
    assert all(np.array_equal(bits(feat[k]), bits(s["feat"][k])) for k in feat)
    rgb, rad = R.read_image()
    assert np.array_equal(bits(rad), bits(s["radiance"])) and np.array_equal(rgb, tone_map(s["radiance"]))
    with pytest.raises(ptmi.PtmiError, match="nothing denoised yet"):
        R.read_denoised()
    with pytest.raises(ptmi.PtmiError, match="no current variance"):
        R.variance()
    check_denoise(R, s, {})
    assert np.array_equal(R.history_counts(), np.zeros((H, W), F))           # no history appeared
    R.render_frame()                                             # the next frame overwrites the injected image: streams and sums untouched
    after = R.read_image()
    assert np.array_equal(after[0], plain[0]) and np.array_equal(bits(after[1]), bits(plain[1]))


def test_hook_inputs_go_stale_like_rendered_ones(R):
    W, H = 24, 16
    s = FS.atrous_set(W, H)
    fresh(R, W, H)
    inject(R, s)
    R.denoise(iterations=1)
    R.set_camera(camera(80.0))
    with pytest.raises(ptmi.PtmiError, match="no image rendered yet"):
        R.denoise(iterations=1)
    with pytest.raises(ptmi.PtmiError, match="no current feature buffers"):
        R.features()
    R.render_features(2)                                         # recomputed from the scene, not what was injected
    traced = R.features()
    assert not np.array_equal(bits(traced["position"]), bits(s["feat"]["position"]))
    R.update_resolution(W, H)
    R.set_camera(camera(80.0))
    R.render_features(2)
    assert all(np.array_equal(bits(traced[k]), bits(v)) for k, v in R.features().items())


def test_hook_with_the_products_own_frame_reproduces_its_denoise(R):
    fresh(R, 40, 32, spp=4)
    R.render_frame()
    rgb, rad = R.read_image()
    drgb, drad = R.denoise()
    feat = R.features()
    vrgb, vrad = R.denoise_variance(source=1)
    vin, vout = R.variance()
    R.update_resolution(40, 32)                                  # image and features gone
    R.debug_set_filter_inputs(rad, feat, grid=2)
    rgb2, rad2 = R.read_image()
    assert np.array_equal(rgb2, rgb) and np.array_equal(bits(rad2), bits(rad))            # the hook's rgb8 is the resolve's
    drgb2, drad2 = R.denoise()
    assert np.array_equal(drgb2, drgb) and np.array_equal(bits(drad2), bits(drad))
    vrgb2, vrad2 = R.denoise_variance(source=1)
    vin2, vout2 = R.variance()
    assert np.array_equal(vrgb2, vrgb) and np.array_equal(bits(vrad2), bits(vrad))
    assert np.array_equal(bits(vin2), bits(vin)) and np.array_equal(bits(vout2), bits(vout))
