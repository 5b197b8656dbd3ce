"""The kernels around an accumulation pass (csrc/kernels.hip: ptmi_adapt, ptmi_resolve_counts; csrc/denoise_variance.hip:
ptmi_pass_moments, ptmi_variance_moments) and the launch order by cost (ptmi_cost_histogram, ptmi_cost_offsets, ptmi_cost_scatter)
on the constructed state of tests/accum_edge_sets.py, given through ptmi_debug_accum_step and ptmi_debug_order_by_cost - which
launch the product's own kernels - and read back through the product: ptmi_read_pass_moments, ptmi_read_sample_counts,
ptmi_read_image, ptmi_denoise_variance (source = 0) and a following ptmi_accum_pass.

Every comparison is bit for bit against the numpy float32 / Python-integer restatements, a NaN counting as equal to a NaN whatever
its payload.  The two freedoms the kernels document - the order of the waves in the compacted queue, the order of the 256-entry
blocks inside a cost class - are asserted as the contract states them (check_compaction, check_order), not sorted away.
tests/test_accum_edge_sets_host.py proves, without a GPU, that every labelled case sits on its edge.
"""
import os

import numpy as np
import pytest

import ptmi
import accum_edge_sets as AS
import filter_edge_sets as FS
import variance_oracle as VO
from accum_edge_sets import F, U, bits, same
from oracle_binding import SCENES

from test_gpu_denoise import tone_map

pytestmark = pytest.mark.gpu
CBOX = os.path.join(SCENES, "cbox.obj")

# name: width, height, wave_tiles asked for, tiling, the slot order that must result (tile8), local rows
LAYOUTS = {
    "rows_24x16": dict(w=24, h=16, wave_tiles=0, tiling={}, tile8=False, rows=16),
    "tiles_24x16": dict(w=24, h=16, wave_tiles=1, tiling={}, tile8=True, rows=16),
    "rows_21x13": dict(w=21, h=13, wave_tiles=1, tiling={}, tile8=False, rows=13),             # no 8 x 8 tiling of 21 x 13 exists
    "ranks2_block8": dict(w=24, h=32, wave_tiles=1, tiling=dict(n_ranks=2, rank=1, row_block=8), tile8=True, rows=16),
    "ranks2_block4": dict(w=24, h=32, wave_tiles=1, tiling=dict(n_ranks=2, rank=0, row_block=4), tile8=False, rows=16),   # tile8 switches itself off
}


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    r.load_scene(CBOX, 0)
    yield r
    r.close()


def setup(R, name, spp=1):
    lay = LAYOUTS[name]
    R.set_camera(ptmi.default_camera())
    R.set_config(spp=spp, max_depth=5, integrator=0, wave_tiles=lay["wave_tiles"], streams=0)
    R.update_resolution(lay["w"], lay["h"], **lay["tiling"])
    assert len(R.local_rows()) == lay["rows"]
    return lay


def tone(rad):
    with np.errstate(all="ignore"):
        return tone_map(rad)


def read_state(R):
    mean, m2, passes = R.pass_moments()
    rgb, rad = R.read_image()
    return dict(mean=mean, m2=m2, passes=passes, counts=R.sample_counts(), rgb=rgb, rad=rad)


def step(R, lay, L):
    """one ptmi_debug_accum_step on launch L: the queue against the compaction's contract, every pixel of the moments, the count
    map, the radiance and the rgb8 against the restatement.  Returns (the queue, what was read back)"""
    out = R.debug_accum_step(L["sums"], L["prev"], L["m2"], L["passes"], queue=L["queue"], n_queue=L["n_queue"], params=L["params"], first=L["first"])
    r = AS.restate(L)
    q = AS.queue_of(L)
    AS.check_compaction(q, r["more"][q], out)
    px = lambda a: AS.to_pixels(a, lay["w"], lay["rows"], lay["tile8"])
    got = read_state(R)
    assert np.array_equal(got["passes"], px(r["passes"])), np.argwhere(got["passes"] != px(r["passes"]))[:8].tolist()
    assert same(got["mean"], px(r["prev"][:, 3])) and same(got["m2"], px(r["m2"]))
    assert np.array_equal(got["counts"], px(r["counts"]))
    assert same(got["rad"], px(r["radiance"])), np.argwhere(bits(got["rad"]) != bits(px(r["radiance"])))[:8].tolist()
    assert np.array_equal(got["rgb"], tone(px(r["radiance"])))
    return out, got


def fresh(R, name="rows_24x16", spp=1):
    lay = setup(R, name, spp)
    return lay, lay["w"] * lay["rows"]


# ------------------------------------------------------------------------------------------------
# the stopping rule at 24 x 16 = 384 slots, 1.5 workgroups
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,threshold,floor", AS.TIE_TRIPLES)
def test_ties_stop_and_their_nextafter_upwards_goes_on(R, k, threshold, floor):
    lay, n = fresh(R)
    L = AS.tie_launch(n, k, threshold, floor)
    out, _ = step(R, lay, L)
    assert set(L["labels"]["tie_up"]) <= set(out.tolist()) and not (set(L["labels"]["tie"]) | set(L["labels"]["tie_dn"])) & set(out.tolist())


def test_pass_counts_from_min_passes_to_65536_in_one_launch(R):
    lay, n = fresh(R)
    L = AS.pass_count_launch(n)
    out, got = step(R, lay, L)
    lab = {k: v[0] for k, v in L["labels"].items()}
    goes_on = {"k_min_minus_1", "k_50000_up", "k_below_max_nan", "k_2", "k_1"}
    for label, s in lab.items():
        assert (s in out.tolist()) == (label in goes_on), label
    assert got["counts"].max() == 65536
    step(R, lay, AS.beyond_launch(n))


def test_a_first_pass_with_a_queue_reads_no_stale_state(R):
    lay, n = fresh(R)
    L = AS.first_launch(n)
    out, got = step(R, lay, L)
    assert sorted(out.tolist()) == sorted(AS.queue_of(L).tolist())
    assert np.isfinite(got["mean"]).all() and np.isfinite(got["m2"]).all()


def test_nonfinite_and_signed_values_touch_no_other_pixel(R):
    """what NON-FINITE VALUES under THE STOPPING RULE (include/ptmi.h) says: a NaN M2 fails the comparison - the pixel goes on until
    max_passes stops it - and every other pixel of the launch is what it is without the case"""
    lay, n = fresh(R)
    plain = AS.nonfinite_launch(n, False)
    out0, got0 = step(R, lay, plain)
    full = AS.nonfinite_launch(n, True)
    launches = [("all", full, [s for v in full["labels"].values() for s in v])]
    launches += [(label, AS.nonfinite_single(n, label), full["labels"][label]) for label in AS.NONFINITE_LABELS]
    for what, L, slots in launches:
        out, got = step(R, lay, L)
        keep = np.ones(n, bool); keep[slots] = False
        keep_px = AS.to_pixels(keep, lay["w"], lay["rows"], lay["tile8"])
        for key in ("mean", "m2", "rad"):
            assert same(got[key][keep_px], got0[key][keep_px]), (what, key)
        for key in ("passes", "counts", "rgb"):
            assert np.array_equal(got[key][keep_px], got0[key][keep_px]), (what, key)
        assert set(out.tolist()) - set(slots) == set(out0.tolist()) - set(slots), what
    out, _ = step(R, lay, full)
    lab = {k: v[0] for k, v in full["labels"].items()}
    for label in ("sum_nan", "sum_pinf", "sum_ninf", "prev_inf", "prev_inf_sum_inf", "m2_nan", "m2_pinf"):
        assert lab[label] in out.tolist(), label
    assert lab["m2_nan_at_max"] not in out.tolist() and lab["m2_negative"] not in out.tolist()
    step(R, lay, AS.threshold_zero_launch(n))


def test_a_progressive_step_stops_nothing(R):
    lay, n = fresh(R)
    L = AS.progressive_launch(n)
    out, _ = step(R, lay, L)
    assert len(out) == L["n_queue"]


# ------------------------------------------------------------------------------------------------
# the compaction
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scattered", [False, True])
@pytest.mark.parametrize("length", AS.QUEUE_LENGTHS)
def test_compaction_of_ragged_queues(R, length, scattered):
    lay, n = fresh(R)
    for pattern in AS.PATTERNS:
        L = AS.compaction_launch(n, length, pattern, scattered)
        out, _ = step(R, lay, L)
        assert len(out) == AS.claimed_count(pattern, L["n_queue"]), pattern


# ------------------------------------------------------------------------------------------------
# resolve at counts, and every slot order
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [1, 3])
def test_every_pixel_is_resolved_at_its_own_count(R, spp):
    lay, n = fresh(R, "tiles_24x16", spp)
    L = AS.resolve_launch(n, spp)
    _, got = step(R, lay, L)
    assert len(np.unique(got["counts"])) >= 8 and (got["counts"] == 0).any() and (got["counts"] == spp).any()


def probe_slot_order(R, lay):
    """the slot order the context really has, through ptmi_read_pass_moments: slot s carries m2 = s"""
    n = lay["w"] * lay["rows"]
    R.debug_accum_step(np.ones((n, 3), F), np.zeros((n, 4), F), np.arange(n, dtype=F), np.arange(n, dtype=U), queue=None, n_queue=0, params=None)
    _, m2, passes = R.pass_moments()
    assert np.array_equal(m2.astype(np.int64), passes.astype(np.int64))
    rows_major = AS.to_pixels(np.arange(n), lay["w"], lay["rows"], False)
    if np.array_equal(passes, rows_major):
        return False
    assert np.array_equal(passes, AS.to_pixels(np.arange(n), lay["w"], lay["rows"], True))
    return True


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_step_under_every_slot_order(R, name):
    lay = setup(R, name)
    n = lay["w"] * lay["rows"]
    assert probe_slot_order(R, lay) == lay["tile8"]
    if name == "ranks2_block8":
        assert R.local_rows().tolist() == list(range(8, 16)) + list(range(24, 32))
    for L in (AS.tie_launch(n, *AS.TIE_TRIPLES[0]), AS.pass_count_launch(n), AS.first_launch(n), AS.nonfinite_launch(n), AS.resolve_launch(n, 1),
              AS.compaction_launch(n, None, "random_half", True), AS.compaction_launch(n, 257, "lane_63", False)):
        step(R, lay, L)
    R.set_config(wave_tiles=0)


# ------------------------------------------------------------------------------------------------
# read-back through ptmi_denoise_variance, source = 0
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rows_24x16", "tiles_24x16"])
def test_the_accumulation_source_of_the_variance_on_constructed_moments(R, name):
    """ptmi_debug_set_filter_inputs composes: it gives the features (and an image the step then overwrites); the step marks the
    image as a pass, so source = 0 reads the constructed M2 and passes"""
    lay = setup(R, name, spp=2)
    w, h = lay["w"], lay["rows"]
    s = FS.atrous_set(w, h)
    R.debug_set_filter_inputs(s["radiance"], s["feat"], grid=2)
    Lp = AS.variance_launch(w, h)                                       # by pixel
    L = dict(Lp, **{key: AS.to_slots(Lp[key].reshape((h, w) + Lp[key].shape[1:]), lay["tile8"]) for key in ("sums", "prev", "m2", "passes")})
    _, got = step(R, lay, L)
    r = AS.restate(Lp)
    rad = r["radiance"].reshape(h, w, 3)
    assert same(got["rad"], rad)
    moments = (r["m2"].reshape(h, w), r["passes"].reshape(h, w))
    for iterations in (0, 1):
        prm = dict(iterations=iterations, sigma_position=FS.SIGMA_X, feature_grid=2)
        drgb, drad = R.denoise_variance(source=0, **prm)
        vin, vout = R.variance()
        p = dict(FS.VARIANCE_DEFAULTS, **prm)
        erad, evin, evout = VO.denoise_variance(rad, s["feat"], p["iterations"], p["sigma_luminance"], p["epsilon"], F(p["sigma_position"]),
                                                p["normal_squarings"], bool(p["demodulate"]), p["spatial_radius"], moments=moments)
        assert same(vin, evin), np.argwhere(bits(vin) != bits(evin))[:8].tolist()
        assert same(vout, evout) and same(drad, erad) and np.array_equal(drgb, tone(erad))
        lab = {k: divmod(v[0], w) for k, v in Lp["labels"].items() if len(v) == 1}
        assert vin[lab["m2_negative"]] == 0 and vin[lab["m2_nan"]] == 0     # max(0, M2 / ...): fmaxf of a negative, and of a NaN, and 0
        # the hand-over: a pixel with two passes or more carries the moments' variance, the others the spatial estimate
        _, svin, _ = VO.denoise_variance(rad, s["feat"], 0, p["sigma_luminance"], p["epsilon"], F(p["sigma_position"]), p["normal_squarings"],
                                         bool(p["demodulate"]), p["spatial_radius"], moments=None)
        low = moments[1] < 2
        assert same(vin[low], svin[low]) and not same(vin[~low], svin[~low])
    R.set_config(wave_tiles=0)


# ------------------------------------------------------------------------------------------------
# continuation: a real pass goes on from the constructed state
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
@pytest.mark.parametrize("name", ["rows_24x16", "tiles_24x16"])
def test_a_real_pass_continues_from_the_step(R, name, next_event):
    """next_event: the same pass through the per-lane kernel, which takes the pass's queue itself - and lights far more of this
    view's pixels at one sample than the queue loop's paths, of which only a few reach the emitter"""
    lay = setup(R, name, spp=1)
    try:
        R.set_config(next_event=next_event)
        R.update_resolution(lay["w"], lay["h"])
        continuation(R, name, lay)
    finally:
        R.set_config(next_event=False, wave_tiles=0)


def continuation(R, name, lay):
    w, h, n = lay["w"], lay["rows"], lay["w"] * lay["rows"]
    prm = dict(min_passes=2, max_passes=8, threshold=0.05, floor=0.01)
    R.accum_reset()
    R.accum_pass(prm); R.accum_pass(prm)                               # the product alone: two passes
    two = read_state(R)
    R.update_resolution(w, h)                                          # streams re-seeded: the same first pass again
    st1 = R.accum_pass(prm)
    one = read_state(R)
    assert st1.active_after == n and (one["counts"] == 1).all()
    # the state after pass 1 by slot (spp = 1, one pass: the radiance is the colour sum, rcp_rn(1) = 1), given back through the
    # hook as a first pass of a chosen third of the slots: they go on (k = 1 < min_passes), the others are out of the accumulation
    sums = AS.to_slots(one["rad"], lay["tile8"])
    # the chosen third, in no order: every other slot whose two-sample sum is not black (most of this view is, at one sample), then
    # black ones - so both the pixels that go on and the ones left behind hold pixels a wrong sum would show in
    lit = np.flatnonzero(AS.to_slots(two["rad"], lay["tile8"]).any(-1))
    print(f"{name}: {len(lit)} of {n} slots lit after two samples, {int(sums.any(-1).sum())} after one")
    assert len(lit) >= 2                                               # one for the pixels that go on, one for those left behind
    dark = np.setdiff1d(np.arange(n), lit)
    take = lit[::2][:n // 3]
    chosen = np.random.default_rng(61).permutation(np.concatenate([take, dark[:n // 3 - len(take)]])).astype(np.int32)
    assert len(chosen) == n // 3 and len(set(chosen.tolist())) == n // 3
    L = dict(sums=sums, prev=np.concatenate([sums, AS.to_slots(one["mean"], lay["tile8"])[:, None]], 1), m2=AS.to_slots(one["m2"], lay["tile8"]),
             passes=AS.to_slots(one["passes"], lay["tile8"]), queue=chosen, n_queue=len(chosen), params=prm, first=True, spp=1, labels={})
    out, after = step(R, lay, L)
    assert sorted(out.tolist()) == sorted(chosen.tolist())
    for key in ("mean", "m2", "rad"):
        assert same(after[key], one[key]), key                         # the step restated pass 1's own test: nothing moved
    assert np.array_equal(after["rgb"], one["rgb"]) and np.array_equal(after["counts"], one["counts"])
    st2 = R.accum_pass(prm)
    assert (st2.pass_, st2.active_before, st2.samples) == (3, len(out), len(out))          # the step counted as the accumulation's pass 2
    got = read_state(R)
    sel = AS.to_pixels(np.isin(np.arange(n), chosen), w, h, lay["tile8"])
    assert np.array_equal(got["counts"], np.where(sel, 2, 1))          # exactly those pixels gained spp samples
    for key in ("mean", "m2", "rad"):
        assert same(got[key][~sel], one[key][~sel]) and same(got[key][sel], two[key][sel]), key
    for key in ("rgb", "passes"):
        assert np.array_equal(got[key][~sel], one[key][~sel]) and np.array_equal(got[key][sel], two[key][sel]), key
    assert not same(two["rad"][sel], one["rad"][sel]) and not same(two["rad"][~sel], one["rad"][~sel])     # either way would show


# ------------------------------------------------------------------------------------------------
# the launch order by cost
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", AS.ORDER_CLASSES)
def test_launch_order_by_cost(R, classes):
    for case in AS.order_cases():
        out, hist = R.debug_order_by_cost(case["n"], case["cost"], case["cost_max"], classes, queue_in=case["queue"])
        try:
            AS.check_order(case, classes, out, hist)
        except AssertionError as e:
            raise AssertionError(f"{case['label']}, classes {classes}: {e}") from e


def test_the_order_hook_leaves_the_context_alone(R):
    lay, n = fresh(R)
    R.accum_reset(); R.accum_pass(None)
    before = read_state(R)
    case = AS.order_cases()[0]
    R.debug_order_by_cost(case["n"], case["cost"], case["cost_max"], 32, queue_in=case["queue"])
    after = read_state(R)
    assert all(np.array_equal(bits(before[k]) if before[k].dtype == F else before[k], bits(after[k]) if after[k].dtype == F else after[k]) for k in before)
    assert R.accum_pass(None).pass_ == 2


# ------------------------------------------------------------------------------------------------
# rejections
# ------------------------------------------------------------------------------------------------
def expect_invalid(fn):
    with pytest.raises(ptmi.PtmiError) as e:
        fn()
    assert e.value.code == -1, str(e.value)


def test_rejections(R):
    lay, n = fresh(R)
    L = AS.progressive_launch(n)
    args = lambda **kw: {**dict(sums=L["sums"], prev=L["prev"], m2=L["m2"], passes=L["passes"]), **kw}
    for bad in ([n], [-1], [3, 3], [0, 5, n + 7]):
        expect_invalid(lambda: R.debug_accum_step(**args(queue=np.array(bad, np.int32))))
    expect_invalid(lambda: R.debug_accum_step(**args(queue=None, n_queue=n + 1)))
    expect_invalid(lambda: R.debug_accum_step(**args(queue=None, n_queue=-1)))
    p = lambda a: a.ctypes.data
    q = np.zeros(n, np.int32); cnt = ptmi.C.c_int(0)
    ok = [R.h, p(L["sums"]), p(L["prev"]), p(L["m2"]), p(L["passes"]), None, n, None, 0, p(q), ptmi.C.byref(cnt)]
    for null in (0, 1, 2, 3, 4, 9, 10):
        a = list(ok); a[null] = None
        assert R.L.ptmi_debug_accum_step(*a) == -1, null
    R.set_config(integrator=1)
    expect_invalid(lambda: R.debug_accum_step(**args()))
    R.set_config(integrator=0)
    fresh_ctx = ptmi.Renderer(0)
    try:
        assert fresh_ctx.L.ptmi_debug_accum_step(fresh_ctx.h, *ok[1:]) == -1       # no scene, no resolution
    finally:
        fresh_ctx.close()
    assert len(R.debug_accum_step(**args())) == n                                  # and the arguments were good
    cost = np.arange(10, dtype=U)
    for bad in (dict(n=0), dict(n=11), dict(classes=0), dict(queue_in=np.array([0, 10, 1], np.int32), n=3), dict(queue_in=np.array([-1], np.int32), n=1)):
        kw = dict(dict(n=10, cost=cost, cost_max=9, classes=16), **bad)
        expect_invalid(lambda: R.debug_order_by_cost(**kw))
    out, hist = np.zeros(10, np.int32), np.zeros(512, np.int32)
    for null in (0, 3, 7, 8):
        a = [R.h, 10, None, p(cost), 10, 9, 16, p(out), p(hist)]; a[null] = None
        assert R.L.ptmi_debug_order_by_cost(*a) == -1, null
