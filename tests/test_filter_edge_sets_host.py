"""The constructed filter inputs (tests/filter_edge_sets.py) proved on the numpy restatements alone, without a GPU: every label is
there as often as declared, its pixel takes the branch the label names (the intermediate - W, px, a dot product - is recomputed
and compared with == or np.nextafter), the two sides of a threshold get different verdicts, and in the temporal set no branch
of include/ptmi.h's ptmi_temporal_accumulate is left without a pixel.  On the finite sets the float32 restatements are also
held against their binary64 evaluation."""
import numpy as np
import pytest

import denoise_oracle as DO
import filter_edge_sets as FS
import temporal_oracle as TO
import variance_oracle as VO
from filter_edge_sets import dn, up

F = np.float32
TINY = np.finfo(F).tiny
DENORM_MIN = F(1.401298464324817e-45)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# a. the a-trous sets: labels and branches
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", FS.ATROUS_SIZES)
def test_atrous_labels_take_their_branches(w, h):
    s = FS.atrous_set(w, h)
    rad, feat, L = s["radiance"], s["feat"], s["labels"]
    assert rad.shape == (h, w, 3) and np.isfinite(rad).all() and all(np.isfinite(v).all() for v in feat.values())
    assert s["declared"] == {k: len(v) for k, v in L.items()} and all(len(set(v)) == len(v) for v in L.values())
    if (w, h) in FS.ATROUS_FULL:
        assert set(FS.ATROUS_LABELS) <= set(L) and len(L["miss"]) == 24
    tr_d, tr_v = [], []
    out = FS.restate_denoise(DO, s, dict(iterations=1), trace=tr_d)
    vout = FS.restate_variance(VO, s, dict(iterations=1), trace=tr_v)
    Wd, Wv = tr_d[0], tr_v[0][0]
    c = VO.demodulated(rad, feat["albedo"], True)
    for p in L.get("miss", []):                                  # W > 0 fails: the pixel keeps its input, in both filters
        assert Wd[p] == 0 and Wv[p] == 0 and feat["hit_fraction"][p] == 0
        assert (bits(out[p]) == bits(rad[p])).all() and (bits(vout[0][p]) == bits(rad[p])).all() and vout[1][p] == 0
    for p in L.get("hit_among_misses", []):                      # every tap but its own weighs 0: W is the centre tap's h = 9/64
        assert Wd[p] == F(0.140625) and Wv[p] == F(0.140625)
        assert (bits(out[p]) == bits((((Wd[p] * c[p]) / Wd[p]) * feat["albedo"][p]).astype(F))).all()    # S / W of the one tap
    for p in L.get("zero", []):
        assert (bits(rad[p]) == 0).all()
    for p in L.get("denormal", []):
        assert (rad[p] > 0).all() and (rad[p] < TINY).all()
    for p in L.get("albedo_zero_channel", []):                   # the zero channel is not divided; the others are
        a = feat["albedo"][p]
        assert a[1] == 0 and a[0] != 0 and a[2] != 0
        assert bits(c[p][1]) == bits(rad[p][1]) and c[p][0] == rad[p][0] / a[0]
    for p in L.get("albedo_tiny", []):
        assert (feat["albedo"][p] == F(1e-30)).all() and (c[p] > 1e7).all() and np.isfinite(c[p] * c[p]).all()
    for p in L.get("spike", []):
        y, x = p
        nb = [rad[q] for q in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)) if 0 <= q[0] < h and 0 <= q[1] < w]
        assert all((rad[p] > F(1e5) * q).all() for q in nb) and nb
    for p in L.get("partial_hit", []):
        n = feat["normal"][p]
        assert feat["hit_fraction"][p] == F(0.5) and TO.dot(n, n) == F(0.25)
    for y, x in L.get("seam", []):                               # wn = 0 and wn = 1 among the taps of one pixel
        n = feat["normal"]
        dots = {float(TO.dot(n[y, x], n[y + dj, x])) for dj in (-2, -1, 1, 2) if 0 <= y + dj < h}
        assert 0.0 in dots and 1.0 in dots
    if (w, h) in FS.ATROUS_FULL:                                 # the side wall: a normal weight that is neither 0 nor 1
        n = feat["normal"]
        d = TO.dot(n[:, 1:], n[:, :-1])
        assert ((d > 0) & (d < 1)).any()


# ------------------------------------------------------------------------------------------------
# a. float32 against binary64
# ------------------------------------------------------------------------------------------------
# The largest relative difference |float32 - binary64| / max(|binary64|, FLT_MIN) between the two evaluations of the restatements
# over set (a) - every size, every parameter set - measured on the CPU, never on a GPU.  Excluded: pixels within 4 ulp of a W > 0
# decision (an iteration where W > 0 holds in one evaluation and not in the other, or 0 < W <= 4 denormal steps), and for the
# variance-guided filter pixels with 0 < W < 1e-18, where W * W and every w * w leave float32's range (set (b), the header's
# (V / W) / W clause: the quotient of two underflowed sums has no digits to compare).  The test allows 4 x the measurement.
MEASURED = {"denoise": 1.53e-5, "variance_radiance": 1.15e-3, "variance_in": 1.80e-5, "variance_out": 2.04e-2}


def _rel(a32, b64, exclude):
    rel = np.abs(a32.astype(np.float64) - b64) / np.maximum(np.abs(b64), TINY)
    rel[exclude] = 0
    return float(rel.max())


@pytest.mark.parametrize("w,h", FS.ATROUS_SIZES)
def test_float32_restatements_agree_with_binary64(w, h):
    s = FS.atrous_set(w, h)
    worst = dict.fromkeys(MEASURED, 0.0)
    for prm in FS.DENOISE_PARAMS:
        t32, t64 = [], []
        a = FS.restate_denoise(DO, s, prm, trace=t32)
        b = FS.restate_denoise(DO, s, prm, T=np.float64, trace=t64)
        assert a.dtype == F and b.dtype == np.float64 and np.isfinite(a).all()
        ex = np.zeros((h, w), bool)
        for w32, w64 in zip(t32, t64):
            ex |= ((w32 > 0) != (w64 > 0)) | ((w32 > 0) & (w32 <= 4 * DENORM_MIN))
        worst["denoise"] = max(worst["denoise"], _rel(a, b, ex))
    for prm in FS.VARIANCE_PARAMS:
        t32, t64 = [], []
        a = FS.restate_variance(VO, s, prm, trace=t32)
        b = FS.restate_variance(VO, s, prm, T=np.float64, trace=t64)
        assert all(np.isfinite(x).all() for x in a)
        ex = np.zeros((h, w), bool)
        for (w32, _, _), (w64, _, _) in zip(t32, t64):
            ex |= ((w32 > 0) != (w64 > 0)) | ((w32 > 0) & (w32 < F(1e-18)))
        for key, x, y in zip(("variance_radiance", "variance_in", "variance_out"), a, b):
            worst[key] = max(worst[key], _rel(x, y, ex))
    print(f"float32 vs binary64 at {w} x {h}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 4 * MEASURED[k], (k, v)


# ------------------------------------------------------------------------------------------------
# b. 0 < W, W * W == 0
# ------------------------------------------------------------------------------------------------
def test_underflow_pixel_takes_the_two_division_clause():
    s = FS.underflow_set()
    (p,) = s["labels"]["w_squared_underflows"]
    tr = []
    rad, vin, vout = FS.restate_variance(VO, s, FS.UNDERFLOW_PARAMS, trace=tr)
    W, V, _ = tr[0]
    assert W[p] > 0 and W[p] * W[p] == 0 and W.dtype == F
    with np.errstate(all="ignore"):
        assert np.isfinite((V[p] / W[p]) / W[p]) and not np.isfinite(V[p] / (W[p] * W[p]))     # what the one-division form would give
    others = np.ones(W.shape, bool); others[p] = False
    assert (W[others] * W[others] > 0).all()
    assert np.isfinite(rad).all() and np.isfinite(vout).all() and vin[p] >= 0


# ------------------------------------------------------------------------------------------------
# c. non-finite pixels
# ------------------------------------------------------------------------------------------------
def test_nonfinite_pixels_stay_inside_their_reach():
    s, clean = FS.nonfinite_set()
    L = s["labels"]
    assert s["declared"] == {k: len(v) for k, v in L.items()} and all(len(L[k]) == 1 for k in s["reach"])
    reaches = list(s["reach"].values())
    for i in range(4):
        for j in range(i):
            assert not (reaches[i] & reaches[j]).any()                               # the four reaches do not overlap
    control = np.zeros((19, 33), bool)
    for p in L["control"]:
        control[p] = True
    assert control.sum() > 100 and not (control & np.any(reaches, axis=0)).any()
    assert 2 * (2 ** FS.NONFINITE_DENOISE["iterations"] - 1) <= FS.NONFINITE_REACH
    assert FS.NONFINITE_VARIANCE["spatial_radius"] + 2 * (2 ** FS.NONFINITE_VARIANCE["iterations"] - 1) == FS.NONFINITE_REACH
    runs = {"denoise": [(FS.restate_denoise(DO, x, FS.NONFINITE_DENOISE),) for x in (s, clean)],
            "variance": [FS.restate_variance(VO, x, FS.NONFINITE_VARIANCE) for x in (s, clean)]}
    for name, (got, ref) in runs.items():
        assert all(np.isfinite(r).all() for r in ref)
        for g, r in zip(got, ref):
            g2 = g.reshape(19, 33, -1); r2 = r.reshape(19, 33, -1)
            assert np.isfinite(g2[control]).all() and (bits(g2[control]) == bits(r2[control])).all(), name
            outside = ~np.any(reaches, axis=0)
            assert (bits(g2[outside]) == bits(r2[outside])).all(), name                # nothing escapes the stated reach
        rad_g, rad_r = got[0], ref[0]
        for label in ("nan_radiance", "inf_radiance"):                                # a non-finite colour shows inside its reach
            assert not np.isfinite(rad_g[s["reach"][label]]).all(), (name, label)
        for label in ("nan_normal", "inf_position"):
            # a non-finite FEATURE weighs its taps 0 (max(0, NaN) = 0; wx = 0) or fails W > 0: the rule of include/ptmi.h leaves every
            # colour in its reach finite - and changed, since the pixel no longer takes part
            m = s["reach"][label]
            assert np.isfinite(rad_g[m]).all(), (name, label)
            assert (bits(rad_g[m]) != bits(rad_r[m])).any(), (name, label)
            q = L[label][0]                                                            # the pixel itself keeps its input (demodulated and back)
            assert (bits(rad_g[q]) == bits(VO.demodulated(s["radiance"], s["feat"]["albedo"], True)[q] * s["feat"]["albedo"][q])).all()
    # the NaN pixel stays NaN and does not spread in ptmi_denoise; the Inf pixel turns the pixels that tap it into NaN
    den = runs["denoise"][0][0]
    nan_p, inf_p = L["nan_radiance"][0], L["inf_radiance"][0]
    m = s["reach"]["nan_radiance"].copy(); m[nan_p] = False
    assert np.isnan(den[nan_p][0]) and np.isfinite(den[m]).all()
    assert np.isnan(den[inf_p[0], inf_p[1] - 1][1]) and np.isfinite(den[inf_p[0], inf_p[1] - 1][0])


def test_mixed_infinity_pixel_reaches_the_min_of_the_colour_weight():
    s = FS.mixed_infinity_set()
    (p,) = s["labels"]["plus_minus_inf_radiance"]
    q = (p[0], p[1] + 1)
    c = VO.demodulated(s["radiance"], s["feat"]["albedo"], True)
    with np.errstate(all="ignore"):
        L = DO.lum(c)
        d = c[q] - c[p]
        assert np.isnan(L[p]) and np.isfinite(L[q]) and TO.dot(d, d) == np.inf               # a NaN luminance, a distance that is not NaN
        assert np.fmin(L[p], L[q]) == L[q] and np.isnan(np.minimum(L[p], L[q]))             # the two readings of min part here
    tr = []
    out = FS.restate_denoise(DO, s, dict(iterations=1), trace=tr)
    assert np.isfinite(tr[0][q]) and tr[0][q] > 0 and np.isnan(tr[0][p])
    assert np.isnan(out[q][0]) and np.isnan(out[q][1]) and np.isfinite(out[q][2])            # 0 * Inf in two channels, 0 * 0.25 in the third
    assert (bits(out[p]) == bits((c[p] * s["feat"]["albedo"][p]).astype(F))).all()           # the pixel itself: W is NaN, it keeps its value


@pytest.mark.parametrize("w,h", FS.WIDE_SIZES)
def test_wide_sets_are_finite_and_whole(w, h):
    s = FS.atrous_set(w, h)
    assert s["radiance"].shape == (h, w, 3) and set(s["labels"]) >= {"miss", "hit_among_misses", "spike", "albedo_tiny"}
    for prm in FS.WIDE_DENOISE_PARAMS:
        assert np.isfinite(FS.restate_denoise(DO, s, prm)).all()
    for prm in FS.WIDE_VARIANCE_PARAMS:
        assert all(np.isfinite(x).all() for x in FS.restate_variance(VO, s, prm))
    d = FS.temporal_wide_set(w, h)
    st = run_steps(d, FS.TEMPORAL_PARAMS)[1][2]
    assert sum(st) == w * h and min(st) > 1000 and (w * h) % 64 != 0                         # a last wave that is not full


# ------------------------------------------------------------------------------------------------
# d. the temporal set
# ------------------------------------------------------------------------------------------------
_sets = {}


def temporal(w, h, variant=None):
    if (w, h, variant) not in _sets:
        _sets[(w, h, variant)] = FS.temporal_set(w, h, variant)
    return _sets[(w, h, variant)]


def run_steps(d, prm, m=FS.TEMPORAL_SPP):
    """the script of tests/test_gpu_filter_edges.py on the restatement: view A into an empty history, view B over it, view B again
    (still), view A over that, and view B into an emptied history.  Returns per step (radiance, history, stats, trace)."""
    kw = dict(max_history=prm["max_history"], normal_min=prm["normal_min"], sigma_x=F(prm["sigma_position"]), sigma_albedo=prm["sigma_albedo"])
    out, hist = [], None
    for feat, rad, frame in ((d["feat_a"], d["rad_a"], d["frame_a"]), (d["feat_b"], d["rad_b"], d["frame_b"]), (d["feat_b"], d["rad_c"], d["frame_b"]),
                             (d["feat_a"], d["rad_b"], d["frame_a"]), (None, None, None), (d["feat_b"], d["rad_a"], d["frame_b"])):
        if feat is None:
            hist = None
            continue
        tr = {}
        r, hist, st = TO.step(hist, rad, m, feat, frame, trace=tr, **kw)
        out.append((r, hist, st, tr))
    return out


@pytest.mark.parametrize("w,h", FS.TEMPORAL_SIZES[1:])
def test_temporal_labels_take_their_branches(w, h):
    d = temporal(w, h)
    L, tap, exact = d["labels"], d["tap"], d["exact"]
    assert d["declared"] == {k: len(v) for k, v in L.items()}
    used = [p for v in L.values() for p in v]
    assert len(used) == len(set(used)) + 8 and len(set(used)) == w * h           # every pixel of view B has a job; 4 carry 2 - 4 labels
    # COVERAGE: no branch of the step is without a pixel
    assert set(FS.TEMPORAL_VERDICTS) <= set(L) and all(len(L[k]) == 1 for k in FS.TEMPORAL_VERDICTS)
    steps = run_steps(d, FS.TEMPORAL_PARAMS)
    n = w * h
    assert steps[0][2] == (0, n - 3, 3)                                          # an empty history: all restart; the W block's two misses and the hf = 0 tap
    _, hist, st, t = steps[1]
    assert sum(st) == n and min(st) > 0
    one = lambda k: L[k][0]
    for k, (has_taps, reused) in FS.TEMPORAL_VERDICTS.items():
        assert bool(t["ok"][one(k)]) == has_taps and bool(t["reuse"][one(k)]) == reused, k
    for k, kept in FS.TEMPORAL_TAP_KEPT.items():
        assert bool(t["keep"][tap[k]][one(k)]) == kept, k
    # px and py against -1, 0 and the size: the value is on the named side, and where the label says so it is the float itself
    for key, size in (("px", w), ("py", h)):
        v = lambda k: t[key][one(f"{key}_{k}")]
        e = lambda k: exact[f"{key}_{k}"]
        for thr, name in ((-1, "minus1"), (size, "size")):
            assert v("on_" + name) >= F(thr) and (v("on_" + name) == F(thr)) == e("on_" + name)
            assert v("below_" + name) < F(thr) and (v("below_" + name) == dn(F(thr))) == e("below_" + name)
        assert v("on_minus1") < v("above_minus1") < F(-0.99) and v("below_0") < 0 <= v("on_0") and (v("on_0") == 0) == e("on_0")
        assert v("on_size") - v("below_size") < 1e-4 and v("on_minus1") - v("below_minus1") < 1e-4      # neighbours, verdicts differ (above)
        assert -1 < v("between_minus1_and_0") < 0 and size - 1 < v("between_last_and_size") < size
        assert e("on_size") and e("below_size")
        # the taps outside the image: the low border loses taps 0 and 2 (px) / 0 and 1 (py), the high border the other two
        lo, hi = ((0, 2), (1, 3)) if key == "px" else ((0, 1), (2, 3))
        c0 = "x0" if key == "px" else "y0"
        for k in ("on_minus1", "above_minus1", "between_minus1_and_0", "below_0"):
            assert t[c0][one(f"{key}_{k}")] == -1 and not t["keep"][list(lo), one(f"{key}_{k}")[0], one(f"{key}_{k}")[1]].any()
        for k in ("between_last_and_size", "below_size"):
            assert t[c0][one(f"{key}_{k}")] == size - 1 and not t["keep"][list(hi), one(f"{key}_{k}")[0], one(f"{key}_{k}")[1]].any()
        assert t["keep"][list(hi), one(f"{key}_between_minus1_and_0")[0], one(f"{key}_between_minus1_and_0")[1]].all()
        assert t["keep"][list(lo), one(f"{key}_between_last_and_size")[0], one(f"{key}_between_last_and_size")[1]].all()
    # (which of -1, 0 and the size float32 reaches itself depends on the size: the sizes are always reached, 17 x 13 also reaches
    # px == -1; px == 0, py == 0 and py == -1 are reached by neither size and are held exactly by the 1 x 1 variants below)
    assert not (exact["px_on_0"] or exact["py_on_0"] or exact["py_on_minus1"]) and exact["px_on_minus1"] == ((w, h) == (17, 13))
    for k in ("corner_bottom_left", "corner_bottom_right", "corner_top_left", "corner_top_right"):
        kept = t["keep"][:, one(k)[0], one(k)[1]]
        assert kept.sum() == 1 and kept[tap[k]] and t["W"][one(k)] > F(0.01)
    p = one("fx_on_0")
    assert t["px"][p] >= 7 and t["x0"][p] == 7 and t["fx"][p] < 1e-5 and (t["fx"][p] == 0) == exact["fx_on_0"]
    # W on 0.01f and its float neighbours, one tap kept
    for k, val in (("W_eq_min", FS.W_MIN), ("W_below_min", dn(FS.W_MIN)), ("W_above_min", up(FS.W_MIN))):
        kept = t["keep"][:, one(k)[0], one(k)[1]]
        assert kept.tolist() == [False, False, False, True] and bits(t["W"][one(k)]) == bits(val), k
    # the acceptance thresholds: the dot product of the named tap is the parameter's float, or its neighbour
    at = lambda arr, k: arr[tap[k]][one(k)]
    nmin = F(FS.TEMPORAL_PARAMS["normal_min"]); sx2 = F(1); sa2 = F(0.125) * F(0.125)
    assert at(t["nn"], "normal_eq_min") == nmin and at(t["nn"], "normal_below_min") == dn(nmin) and at(t["nn"], "normal_above_min") == up(nmin)
    assert at(t["ee"], "position_eq_sigma") == sx2 and at(t["ee"], "position_below_sigma") == dn(sx2) and at(t["ee"], "position_above_sigma") == up(sx2)
    assert at(t["aa"], "albedo_eq_sigma") == sa2 and at(t["aa"], "albedo_below_sigma") == dn(sa2) and at(t["aa"], "albedo_above_sigma") == up(sa2)
    assert at(t["aa"], "albedo_equal") == 0 and exact["position_eq_sigma"] and exact["albedo_eq_sigma"]
    assert hist.hf[one("both_hf_quarter")] == F(0.25) and hist.hf[one("current_hf_quarter")] == F(0.25)
    ha = steps[0][1]                                                              # view A's history: the taps' hit fractions
    p = one("tap_hf_eq_0")
    y0, x0 = int(t["y0"][p]), int(t["x0"][p])
    assert [float(ha.hf[y0 + (k >> 1), x0 + (k & 1)]) for k in range(4)] == [0.0, 0.25, 0.25, 1.0]
    # the geometry: the signs of (fn, den) and of (sp, sc)
    sign = lambda a: (a > 0).astype(int) - (a < 0).astype(int)
    live = -1 if d["live_branch"] == "fn<0,den<0" else 1
    for frame in (d["frame_a"], d["frame_b"]):                                    # the handedness of every frame used: the other pair is dead
        assert sign(TO.dot(frame[3:6] - frame[0:3], TO.cross(frame[6:9], frame[9:12]))) == live
    assert d["dead_branch"] == ("fn>0,den>0" if live < 0 else "fn<0,den<0") and sign(t["fn"]) == live
    assert (sign(t["den"][t["ok"]]) == live).all() and sign(t["den"][one("behind_previous_camera")]) == -live
    p = one("back_in_one_view")
    assert sign(t["den"][p]) == live and sign(t["sp"][p]) * sign(t["sc"][p]) == -1
    p = one("back_in_both_views")
    assert t["sp"][p] < 0 and t["sc"][p] < 0 and t["reuse"][p]
    p = one("px_on_0")
    assert t["sp"][p] > 0 and t["sc"][p] > 0
    assert t["ok"][tuple(np.array(L["filler"]).T)].any() and not t["ok"][tuple(np.array(L["filler_outside"]).T)].any()
    # the blend: max_history = 65536 does not cap; the counts of the second step are m, 2 m or what the taps gave
    assert abs(hist.count[one("corner_top_right")] - F(2 * FS.TEMPORAL_SPP)) < 1e-5 and hist.count[one("missed")] == F(FS.TEMPORAL_SPP)
    # the still step: every pixel reuses its own history; then view A over view B's history, and an emptied history
    assert steps[2][2] == (n, 0, 0) and len(np.unique(steps[2][1].count)) > 1
    assert sum(steps[3][2]) == n and steps[3][2][0] > 0
    assert steps[4][2][0] == 0 and sum(steps[4][2]) == n


@pytest.mark.parametrize("w,h", FS.TEMPORAL_SIZES[1:])
def test_temporal_zero_sigma_albedo_and_max_history_one(w, h):
    d = temporal(w, h)
    L, tap = d["labels"], d["tap"]
    steps = run_steps(d, FS.TEMPORAL_PARAMS_ZERO_ALBEDO)
    r, hist, st, t = steps[1]
    p = L["albedo_equal"][0]
    assert t["keep"][:, p[0], p[1]].tolist() == [False, False, False, True]       # only equal albedos pass sigma_albedo = 0
    assert t["aa"][3][p] == 0
    # max_history = 1: n' = m and alpha = 1, the blend h + 1 * (c_cur - h) all the same
    assert (hist.count == F(FS.TEMPORAL_SPP)).all() and st[0] > 0
    q = L["corner_top_right"][0]
    assert t["reuse"][q] and np.allclose(r[q], d["rad_b"][q], rtol=1e-5)


@pytest.mark.parametrize("variant,has_taps,reused", [("corner_bottom_left", True, True), ("corner_top_right", True, True), ("inside", True, True),
                                                     ("px_on_minus1", True, False), ("py_on_minus1", True, False), ("px_on_0", True, True),
                                                     ("py_on_0", True, True), ("px_on_size", False, False), ("py_on_size", False, False),
                                                     ("missed", False, False)])
def test_temporal_one_pixel(variant, has_taps, reused):
    d = temporal(1, 1, variant)
    steps = run_steps(d, FS.TEMPORAL_PARAMS)
    t = steps[1][3]
    assert bool(t["ok"][0, 0]) == has_taps and bool(t["reuse"][0, 0]) == reused
    assert sum(steps[1][2]) == 1 and d["exact"][variant]
    exactly = {"px_on_minus1": ("px", -1), "py_on_minus1": ("py", -1), "px_on_0": ("px", 0), "py_on_0": ("py", 0), "px_on_size": ("px", 1),
               "py_on_size": ("py", 1)}
    if variant in exactly:                                       # float32 reaches every one of these itself at 1 x 1
        key, val = exactly[variant]
        assert bits(t[key][0, 0]) == bits(F(val))
    if variant.endswith("_on_minus1"):
        assert t["W"][0, 0] == 0                                 # the bound admits the pixel; its only inside taps weigh f = 0
    if variant.endswith("_on_0"):
        assert t["x0"][0, 0] == 0 and t["y0"][0, 0] == 0 and (t["fx"][0, 0] == 0 or t["fy"][0, 0] == 0)
    if variant.startswith("corner"):
        assert t["keep"][:, 0, 0].sum() == 1 and abs(t["W"][0, 0] - F(0.25)) < 1e-5


def test_temporal_nonfinite_values_follow_the_header():
    d = FS.temporal_nonfinite_set()
    L = d["labels"]
    for prm in (FS.TEMPORAL_PARAMS, FS.TEMPORAL_PARAMS_ZERO_ALBEDO):
        steps = run_steps(d, prm)
        r, hist, st, t = steps[1]
        assert sum(st) == 17 * 13
        for p in d["nonfinite"].values():                        # a non-finite feature: the tests fail at p or at every tap, a restart with the input as it is
            assert not t["reuse"][p] and (bits(r[p]) == bits(d["rad_b"][p])).all() and hist.count[p] == F(FS.TEMPORAL_SPP)
        p = L["corner_top_right"][0]                             # the NaN colour travels with the kept tap - at alpha = 1 as well
        assert t["reuse"][p] and np.isnan(r[p][0]) and np.isfinite(r[p][1:]).all()
        p = L["corner_top_left"][0]
        assert t["reuse"][p] and not np.isfinite(r[p][1]) and np.isfinite(r[p][0])
        p = L["corner_bottom_right"][0]                          # a NaN input colour: the pixel's own output, its count as ever
        assert np.isnan(r[p][1]) and np.isfinite(r[p][0]) and np.isfinite(hist.count).all()
        reads = np.zeros((13, 17), bool)                         # and nobody but the pixels a kept tap of which reads one of the two
        for k in range(4):
            ty, tx = t["y0"] + (k >> 1), t["x0"] + (k & 1)
            reads |= t["keep"][k] & t["reuse"] & (ty == 12) & ((tx == 16) | (tx == 0))
        reads[p] = True
        assert np.array_equal(~np.isfinite(r).all(axis=-1), reads) and reads.sum() >= 3
