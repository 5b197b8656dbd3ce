"""The constructed accumulation state and cost tables (tests/accum_edge_sets.py) proved on the restatement alone, without a GPU:
every labelled slot sits on the edge its label names - the tie stops, its nextafter upwards goes on, the int32 product of
k * (k - 1) would be negative, each survivor pattern has the count it claims - and the two contract checkers accept every order the
contracts allow and refuse the ones they forbid.  So tests/test_gpu_accum_edges.py cannot pass vacuously."""
import numpy as np
import pytest

import accum_edge_sets as AS
from accum_edge_sets import F, U, bits, dn, up

N = 384                                                           # 24 x 16
SIZES = [384, 273]


def only(L, label):
    (s,) = L["labels"][label]
    return s


# ------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------
def test_slot_orders_are_bijections_and_differ():
    for w, h in ((24, 16), (24, 32), (8, 8)):
        for tile8 in (False, True):
            lr, x = AS.slot_pixels(w, h, tile8)
            assert len(set(zip(lr.tolist(), x.tolist()))) == w * h and lr.max() == h - 1 and x.max() == w - 1
            img = np.arange(w * h).reshape(h, w)
            assert np.array_equal(AS.to_pixels(AS.to_slots(img, tile8), w, h, tile8), img)
    a, b = AS.slot_pixels(24, 16, False), AS.slot_pixels(24, 16, True)
    assert (a[0] != b[0]).any() and (a[1] != b[1]).any()
    lr, x = b                                                     # the header's words: slot 9 is pixel (1, 1) of tile 0, slot 64 starts tile 1
    assert (lr[9], x[9]) == (1, 1) and (lr[64], x[64]) == (0, 8) and (lr[192], x[192]) == (8, 0)


# ------------------------------------------------------------------------------------------------
# the stopping rule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k,threshold,floor", AS.TIE_TRIPLES)
def test_ties_sit_on_the_comparison(n, k, threshold, floor):
    assert len(AS.TIE_TRIPLES) >= 3
    L = AS.tie_launch(n, k, threshold, floor)
    r = AS.restate(L)
    assert L["params"]["min_passes"] <= k < L["params"]["max_passes"]
    for label in ("tie", "tie_up", "tie_dn"):
        assert len(L["labels"][label]) >= 3
        for s in L["labels"][label]:
            assert r["k"][s] == k and r["queued"][s]
            assert bits(r["prev"][s, 3]) == bits(r["y"][s]) == bits(L["prev"][s, 3])          # delta == 0: the mean is the pass mean
            assert bits(r["m2"][s]) == bits(L["m2"][s])                                       # M2 is the injected one
            a = F(threshold) * (r["y"][s] + F(floor))
            bound = F(F(a * a) * F(U(k * (k - 1))))
            assert bits(bound) == bits(r["bound"][s]) and bound > 0 and np.isfinite(bound)
            want = dict(tie=bound, tie_up=up(bound), tie_dn=dn(bound))[label]
            assert bits(L["m2"][s]) == bits(want)
            assert bool(r["stop"][s]) == (label != "tie_up") and bool(r["more"][s]) == (label == "tie_up")
    bg = r["queued"].copy(); bg[[s for v in L["labels"].values() for s in v]] = False
    assert r["stop"][bg].any() and r["more"][bg].any()            # the background decides both ways


@pytest.mark.parametrize("n", SIZES)
def test_pass_counts_sit_on_their_edges(n):
    L = AS.pass_count_launch(n)
    r = AS.restate(L)
    prm = L["params"]
    assert L["spp"] == 1 and (prm["min_passes"], prm["max_passes"]) == (4, 65536)
    s = only(L, "k_min_minus_1")
    assert r["k"][s] == prm["min_passes"] - 1 and r["m2"][s] == 0 and r["m2"][s] <= r["bound"][s] and r["more"][s]
    s = only(L, "k_min")
    assert r["k"][s] == prm["min_passes"] and r["m2"][s] == 0 and r["stop"][s]
    for label in ("k_max_nan", "k_max_inf", "k_max_huge", "k_max_zero"):
        s = only(L, label)
        assert r["k"][s] == prm["max_passes"] == 65536 and L["passes"][s] == 65535 and r["stop"][s]
        assert not (r["m2"][s] <= r["bound"][s]) or label == "k_max_zero"          # it is the pass count that stops them
        assert r["counts"][s] == 65536
    assert np.isnan(r["m2"][only(L, "k_max_nan")])
    s = only(L, "k_below_max_nan")
    assert r["k"][s] == prm["max_passes"] - 1 and np.isnan(r["m2"][s]) and r["more"][s]
    # k * (k - 1) above 2^31: exact enough as uint32 -> float, negative as an int32
    for k in (50000, 65536):
        prod = (k * (k - 1)) & 0xFFFFFFFF
        assert prod >= 1 << 31 and np.int64(prod).astype(np.int32) < 0
        assert AS.kk_float(k) == F(prod) and AS.kk_float(k) > 0
    assert 65536 * 65535 == 0xFFFF0000 and int(AS.kk_float(65536)) == 0xFFFF0000            # exact as a float
    for label, stops in (("k_50000_tie", True), ("k_50000_up", False), ("k_50000_dn", True)):
        s = only(L, label)
        assert r["k"][s] == 50000 < prm["max_passes"] and bits(r["m2"][s]) == bits(L["m2"][s]) and r["m2"][s] > 0
        assert bool(r["stop"][s]) == stops
        assert not (r["m2"][s] <= F(np.int64((50000 * 49999) & 0xFFFFFFFF).astype(np.int32)))      # the int32 product would let all three go on
    assert bits(L["m2"][only(L, "k_50000_tie")]) == bits(r["bound"][only(L, "k_50000_tie")])
    assert r["k"][only(L, "k_2")] == 2 and r["more"][only(L, "k_2")] and r["k"][only(L, "k_1")] == 1 and r["more"][only(L, "k_1")]
    assert len(np.unique(r["k"][r["queued"]])) >= 8               # one launch mixes the pass counts


def test_k_65536_reaches_the_comparison_beyond_the_api_range():
    L = AS.beyond_launch(N)
    r = AS.restate(L)
    assert L["params"]["max_passes"] == 65537
    for label, stops in (("k_65536_tie", True), ("k_65536_up", False), ("k_65536_dn", True)):
        s = only(L, label)
        assert r["k"][s] == 65536 and bool(r["stop"][s]) == stops and r["m2"][s] > 0
        a = F(0.05) * (r["y"][s] + F(0.01))
        assert bits(r["bound"][s]) == bits(F(F(a * a) * F(0xFFFF0000)))


@pytest.mark.parametrize("n", SIZES)
def test_a_first_pass_ignores_the_stale_state(n):
    L = AS.first_launch(n)
    r = AS.restate(L)
    q = AS.queue_of(L)
    assert L["first"] and L["queue"] is not None and 0 < len(q) < n and not np.array_equal(q, np.sort(q))
    assert np.isnan(L["prev"][q]).any() and np.isnan(L["m2"][q]).any() and (L["passes"][q] == 0xFFFFFFFF).any()
    clean = dict(L, prev=L["prev"].copy(), m2=L["m2"].copy(), passes=L["passes"].copy())
    clean["prev"][q] = 0; clean["m2"][q] = 0; clean["passes"][q] = 0
    c = AS.restate(clean)
    for key in ("prev", "m2", "passes", "more", "counts", "radiance"):
        assert AS.same(r[key], c[key]) if r[key].dtype == F else np.array_equal(r[key], c[key]), key
    assert (r["passes"][q] == 1).all() and r["more"][q].all() and np.isfinite(r["prev"][q]).all() and (r["m2"][q] == 0).all()
    rest = L["labels"]["not_queued"]
    assert np.array_equal(r["passes"][rest], L["passes"][rest]) and set(L["passes"][rest].tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_cases_do_what_their_labels_say(n):
    L = AS.nonfinite_launch(n)
    r = AS.restate(L)
    assert set(L["labels"]) == set(AS.NONFINITE_LABELS)
    s = {label: only(L, label) for label in AS.NONFINITE_LABELS}
    assert all(r["queued"][v] for v in s.values())
    for label in ("sum_nan", "sum_pinf", "sum_ninf", "prev_inf", "prev_inf_sum_inf", "m2_nan"):           # M2 becomes a NaN: the comparison fails
        assert np.isnan(r["m2"][s[label]]) and r["k"][s[label]] == 4 and r["more"][s[label]], label
    assert np.isnan(L["sums"][s["sum_nan"]]).any() and np.isposinf(L["sums"][s["sum_pinf"]]).any() and np.isneginf(L["sums"][s["sum_ninf"]]).any()
    assert np.isneginf(r["y"][s["prev_inf"]]) and np.isnan(r["y"][s["prev_inf_sum_inf"]])                  # finite - Inf, Inf - Inf
    assert np.isposinf(r["m2"][s["m2_pinf"]]) and r["more"][s["m2_pinf"]]
    assert r["m2"][s["m2_negative"]] < 0 and bits(r["m2"][s["m2_negative"]]) == bits(-up(F(0), 3)) and r["stop"][s["m2_negative"]]
    assert r["y"][s["sum_equals_prev"]] == 0 and np.isfinite(r["m2"][s["sum_equals_prev"]])
    z = s["sum_negative_zero"]
    assert (bits(L["sums"][z]) == 0x80000000).all() and (bits(r["radiance"][z]) == 0x80000000).all() and bits(r["y"][z]) == 0
    assert np.isnan(r["m2"][s["m2_nan_at_max"]]) and r["k"][s["m2_nan_at_max"]] == L["params"]["max_passes"] and r["stop"][s["m2_nan_at_max"]]
    # the launch without them, and with one at a time: the same slots, plain values
    plain = AS.nonfinite_launch(n, False)
    assert all(np.isfinite(plain[key]).all() for key in ("sums", "prev", "m2")) and np.array_equal(AS.queue_of(plain), AS.queue_of(L))
    others = np.ones(n, bool); others[list(s.values())] = False
    for key in ("sums", "prev", "m2", "passes"):
        assert np.array_equal(plain[key][others], L[key][others])
    for label in AS.NONFINITE_LABELS:
        one = AS.nonfinite_single(n, label)
        keep = np.ones(n, bool); keep[s[label]] = False
        assert all(AS.same(one[key][keep].astype(F), plain[key][keep].astype(F)) for key in ("sums", "prev", "m2", "passes"))
        assert AS.same(one["sums"][s[label]], L["sums"][s[label]]) and AS.same(one["m2"][s[label]], L["m2"][s[label]])


def test_threshold_zero_stops_only_m2_at_most_zero():
    L = AS.threshold_zero_launch(N)
    r = AS.restate(L)
    for label, stops in (("t0_zero", True), ("t0_negative_zero", True), ("t0_negative", True), ("t0_positive", False)):
        s = only(L, label)
        assert r["bound"][s] == 0 and r["m2"][s] == L["m2"][s] and bool(r["stop"][s]) == stops, label      # (-0 + 0 * 0 is +0: equal, not the same bits)
    assert L["m2"][only(L, "t0_positive")] == AS.DENORM_MIN and L["m2"][only(L, "t0_negative")] == -AS.DENORM_MIN


def test_a_progressive_pass_stops_nothing_and_advances_the_moments():
    L = AS.progressive_launch(N)
    r = AS.restate(L)
    q = AS.queue_of(L)
    assert L["params"] is None and not r["stop"].any() and r["more"][q].all() and int(r["more"].sum()) == len(q) < N
    assert np.array_equal(r["passes"][q], L["passes"][q] + 1) and not np.array_equal(bits(r["m2"][q]), bits(L["m2"][q]))
    assert (AS.restate(dict(L, params=AS.PARAMS))["stop"]).any()  # the same state under a rule would stop some


# ------------------------------------------------------------------------------------------------
# the compaction
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scattered", [False, True])
@pytest.mark.parametrize("length", AS.QUEUE_LENGTHS)
@pytest.mark.parametrize("pattern", AS.PATTERNS)
def test_survivor_patterns_have_the_counts_they_claim(pattern, length, scattered):
    L = AS.compaction_launch(N, length, pattern, scattered)
    n_q = N if length is None else length
    q = AS.queue_of(L)
    r = AS.restate(L)
    assert len(q) == n_q and (L["queue"] is None) == (not scattered)
    if scattered and n_q > 2:
        assert not np.array_equal(q, np.sort(q)) and (n_q == N or len(np.setdiff1d(np.arange(q.max()), q)))   # not sorted, and it skips slots
    more = r["more"][q]
    assert np.array_equal(more, AS.survivors(pattern, n_q)) and int(more.sum()) == AS.claimed_count(pattern, n_q)
    assert not r["more"][~r["queued"]].any()
    if pattern == "random_half" and n_q >= 63:
        assert n_q / 4 < more.sum() < 3 * n_q / 4
    if pattern == "lane_63":
        assert int(more.sum()) == n_q // 64 and all(p % 64 == 63 for p in np.flatnonzero(more))
    if pattern == "lane_0":
        assert all(p % 64 == 0 for p in np.flatnonzero(more)) and more[0]
    AS.check_compaction(q, more, q[more])


def test_the_compaction_check_accepts_the_contract_and_nothing_else():
    L = AS.compaction_launch(N, 257, "random_half", True)
    q = AS.queue_of(L); more = AS.restate(L)["more"][q]
    waves = [list(q[w:w + 64][more[w:w + 64]]) for w in range(0, len(q), 64)]
    assert sum(len(w) > 1 for w in waves) >= 4
    AS.check_compaction(q, more, sum(waves, []))
    AS.check_compaction(q, more, sum(reversed(waves), []))                       # the order of the waves is free
    AS.check_compaction(q, more, sum(waves[1:] + waves[:1], []))
    swapped = [list(w) for w in waves]; swapped[1][0], swapped[1][1] = swapped[1][1], swapped[1][0]
    interleaved = sum(waves[2:], []) + [v for pair in zip(waves[0], waves[1]) for v in pair]
    interleaved += waves[0][len(waves[1]):] + waves[1][len(waves[0]):]
    flat = sum(waves, [])
    for bad in (sum(swapped, []), interleaved, flat[:-1], flat + [int(q[~more][0])], flat[:-1] + flat[:1], sorted(flat)):
        with pytest.raises(AssertionError):
            AS.check_compaction(q, more, bad)


# ------------------------------------------------------------------------------------------------
# resolve at counts, and the variance hand-over
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [1, 3])
def test_resolve_launch_has_counts_that_differ_per_pixel(spp):
    L = AS.resolve_launch(N, spp)
    r = AS.restate(L)
    lab = L["labels"]
    assert len(lab["not_queued"]) == N - N // 2 and lab["passes_0"] and lab["passes_1"]
    assert (r["counts"][lab["passes_0"]] == 0).all() and (r["counts"][lab["passes_1"]] == spp).all()
    assert np.array_equal(r["passes"][lab["not_queued"]], L["passes"][lab["not_queued"]])
    assert np.array_equal(r["counts"], r["passes"] * U(spp)) and len(np.unique(r["counts"])) >= 8
    assert (np.diff(r["counts"].astype(np.int64)) != 0).mean() > 0.8           # neighbours differ: a count read at another index shows
    assert not np.isfinite(r["radiance"][lab["passes_0"]]).any()               # a sum times rcp(0)


def test_variance_launch_has_the_hand_over_and_the_signed_cases():
    w, h = 24, 16
    L = AS.variance_launch(w, h)
    r = AS.restate(L)
    assert set(AS.VARIANCE_LABELS) == set(L["labels"]) and len(AS.queue_of(L)) == 0
    assert np.array_equal(r["passes"], L["passes"]) and AS.same(r["m2"], L["m2"])
    p = r["passes"].reshape(h, w)
    low = p < 2
    beside = np.zeros_like(low); beside[:, 1:] |= p[:, :-1] >= 2; beside[:, :-1] |= p[:, 1:] >= 2
    assert (low & beside).sum() > 50 and {0, 1, 2} <= set(np.unique(p).tolist())
    lum = lambda c: F(0.2126) * c[0] + F(0.7152) * c[1] + F(0.0722) * c[2]
    assert np.isnan(r["m2"][only(L, "m2_nan")]) and r["m2"][only(L, "m2_negative")] < 0
    assert lum(r["radiance"][only(L, "luminance_zero")]) == 0 and lum(r["radiance"][only(L, "luminance_negative")]) < 0
    assert all(r["passes"][only(L, label)] >= 2 for label in ("m2_nan", "m2_negative", "luminance_zero", "luminance_negative"))


# ------------------------------------------------------------------------------------------------
# the launch order by cost
# ------------------------------------------------------------------------------------------------
def reference_order(case, classes):
    q = np.arange(case["n"]) if case["queue"] is None else case["queue"]
    cls, hist, ends = AS.restate_order(case, classes)
    return q, cls, [int(e) for e in q[np.argsort(cls, kind="stable")]], np.concatenate([hist, ends])


def test_order_shift_and_class_arithmetic():
    assert [AS.order_shift(c) for c in AS.ORDER_CLASSES] == [7, 7, 4, 3, 0, 0] and AS.order_shift(255) == 1 and AS.order_shift(128) == 1
    assert AS.cost_class(0, 0, 0) == 255 and AS.cost_class(7, 0, 0) == 255 and AS.cost_class(7, 0, 7) == 1            # cost_max = 0: the last class
    assert AS.cost_class(100, 100, 0) == AS.cost_class(101, 100, 0) == AS.cost_class(0xFFFFFFFF, 100, 0) == 2          # 255 - floor(25600 / 101)
    assert AS.cost_class(0xFFFFFFFF, 0xFFFFFFFF, 0) == 0 and AS.cost_class(1 << 31, 0xFFFFFFFF, 0) == 127 and AS.cost_class(1 << 24, 0xFFFFFFFF, 0) == 254
    for c in (1 << 24, 1 << 31, 0xFFFFFFFF):                      # a 32-bit c << 8 loses the bits that decide
        assert 255 - (((c << 8) & 0xFFFFFFFF) // (1 << 32)) != AS.cost_class(c, 0xFFFFFFFF, 0)
    for cmax in (9, 1000003, 0xFFFFFFFF):
        steps = AS.class_steps(cmax)
        seen = {AS.cost_class(c, cmax, 0) for c in steps}
        assert seen == (set(range(256)) if cmax >= 255 else seen) and len(seen) >= min(cmax + 1, 256)
        jumps = sum(AS.cost_class(c, cmax, 0) != AS.cost_class(c - 1, cmax, 0) for c in steps if c >= 1 and c - 1 in steps)
        assert jumps >= min(cmax, 255)                            # both sides of every step are in the set


@pytest.mark.parametrize("classes", AS.ORDER_CLASSES)
def test_order_cases_and_the_order_check(classes):
    cases = AS.order_cases()
    labels = [c["label"] for c in cases]
    assert len(set(labels)) == len(labels) and {c["n"] for c in cases} >= set(AS.ORDER_LENGTHS)
    assert any(c["queue"] is None for c in cases) and any(c["queue"] is not None for c in cases)
    n_classes = 256 >> AS.order_shift(classes)
    for case in cases:
        q, cls, ref, hist = reference_order(case, classes)
        assert cls.min() >= 0 and cls.max() < n_classes and hist[256 + 255] == case["n"]
        AS.check_order(case, classes, ref, hist)
        if case["label"] == "cost_max_zero":
            assert (cls == n_classes - 1).all() and case["cost"].max() > 0
        if case["label"] == "at_and_above_cost_max":
            assert (case["cost"] > case["cost_max"]).any() and (case["cost"] == case["cost_max"]).any() and cls.min() == AS.cost_class(100, 100, AS.order_shift(classes))
        if case["queue"] is not None and case["n"] > 1:           # scattered: not sorted, distinct entries
            assert not np.array_equal(q, np.sort(q)) and len(set(q.tolist())) == len(q)
    # what the check refuses, on a case with several classes in several blocks
    case = next(c for c in cases if c["label"] == "random_1000_scattered")
    q, cls, ref, hist = reference_order(case, classes)
    blocks = [[[int(e) for e in q[b:b + 256][cls[b:b + 256] == c]] for b in range(0, len(q), 256)] for c in range(256)]
    free = sum((sum(reversed(runs), []) for runs in blocks), [])  # the blocks of a class in another order: allowed
    AS.check_order(case, classes, free, hist)
    assert len(np.unique(cls)) >= 2
    descending = sum((sum(runs, []) for runs in reversed(blocks)), [])
    with pytest.raises(AssertionError):
        AS.check_order(case, classes, descending, hist)
    run = next(r for runs in blocks for r in runs if len(r) >= 2)
    i, j = ref.index(run[0]), ref.index(run[1])
    swapped = list(ref); swapped[i], swapped[j] = swapped[j], swapped[i]
    starts = np.concatenate([hist[256:257] * 0, hist[256:511]])   # the offsets before the scatter, not the ends after it
    for bad_out, bad_hist in ((swapped, hist), (ref[:-1] + ref[:1], hist), (ref, np.concatenate([hist[:256], starts]))):
        with pytest.raises(AssertionError):
            AS.check_order(case, classes, bad_out, bad_hist)
