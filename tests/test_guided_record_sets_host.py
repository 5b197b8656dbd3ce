"""The constructed sets of tests/guided_record_sets.py, proved on the host: every label sits on the edge it names, the oracle's
C (oracle/ptmi_oracle.c) equals the REFERENCE's own Grid::initFromRadiosity / initFromFormFactor + buildCDFs (compiled into
oracle/_ref/libptmi_ref_integrator.so; its answers are recorded in tests/golden/ref_grid_records.npz) on every record case, the
oracle's C equals the numpy restatement on every filter and grid-update case (two independent restatements; the reference's own
filter and grid update, compiled, answer the same worlds and a subset of the filter cases in tests/test_solver_vs_ref.py), the float32 restatements stay
within a measured bound of the same formulas in binary64, and each mutant of the kernels' arithmetic changes a named case.

Re-record (where oracle/_ref is built):  python tests/golden/make_golden.py --ref-only
"""
import ctypes as C
import os

import numpy as np
import pytest

import guided_record_sets as S
from guided_record_sets import D, EPS_SUM, EPS_TOTAL, F, bits, same
from oracle_binding import (OracleScene, oracle_cdf_records, oracle_filter_pdfs, oracle_lib, oracle_radiosity_grid,
                            recorded_reference, ref_int_available, ref_int_lib, sha)
from test_integrator_vs_ref import (MIS_FRACTIONS, ask_grid_pdf, ask_grid_sample, ask_sample_mis, flat_cases, grid_scripts, mis_scripts,
                                    normal_cases, pdf_cases, po_grid_sample, po_sample_mis)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_grid_records.npz")
UPPER = np.r_[0:272 + 128, 528:530]          # the words buildCDFs fills: pdf, row_sums, marginal, rows 0 .. 7, total, is_valid
UNIFORM = (np.arange(1, 17).astype(F) * F(1.0 / 16)).astype(F)


@pytest.fixture(scope="module")
def ref():
    yield from recorded_reference(GOLDEN, ref_int_available() and hasattr(ref_int_lib(), "ref_grid_record"))


@pytest.fixture(scope="module")
def rs():
    return S.record_set()


@pytest.fixture(scope="module")
def restated(rs):
    return S.restate_records(rs["pdf"])


def rec_of(rs, restated, label):
    return restated[rs["labels"].index(label)]


# ---- 1. records: the labels -------------------------------------------------------------------------------------------------
def test_record_labels_sit_on_their_edges(rs, restated):
    r = lambda l: rec_of(rs, restated, l)
    valid = lambda l: int(r(l)[529:530].view(np.int32)[0])
    # total_weight: the float below 1e-6f, 1e-6f itself (invalid: the test is >), the float above (valid)
    assert r("total_below")[528] == S.dn(EPS_TOTAL) and r("total_at")[528] == EPS_TOTAL and r("total_above")[528] == S.up(EPS_TOTAL)
    assert (valid("total_below"), valid("total_at"), valid("total_above")) == (0, 0, 1)
    assert (r("total_at")[264:271] == 0).all() and r("total_at")[271] == 1          # inv_total = 0, the last entry forced
    # row_sum: below 1e-6f the row is uniform, at and above it (the test is <) it is the row's own
    assert r("row_sum_below")[258] == S.dn(EPS_TOTAL) and r("row_sum_at")[258] == EPS_TOTAL and r("row_sum_above")[258] == S.up(EPS_TOTAL)
    row2 = lambda l: r(l)[272 + 32:272 + 48]
    assert same(row2("row_sum_below"), UNIFORM) and not same(row2("row_sum_at"), UNIFORM) and not same(row2("row_sum_above"), UNIFORM)
    assert valid("row_sum_below") == 1
    # the order of a sum: 2^24 + 1 + ... stays 2^24, 1 + ... + 2^24 does not; the marginal likewise over the row sums
    assert r("row_order")[257] == F(2.0 ** 24) and r("row_order")[261] == F(2.0 ** 24 + 16)
    assert r("marginal_order_head")[528] == F(2.0 ** 24) and r("marginal_order_tail")[528] == F(2.0 ** 24 + 8)
    # running * (1 / row_sum) is not running / row_sum in every upper row
    g = rs["pdf"][rs["labels"].index("inverse_not_quotient")].reshape(16, 16)
    with np.errstate(all="ignore"):
        quot = np.array([np.cumsum(g[v], dtype=F) / np.cumsum(g[v], dtype=F)[-1] for v in range(8)], F)
    assert (bits(quot) != bits(r("inverse_not_quotient")[272:400].reshape(8, 16)))[:, :15].any(axis=1).all()
    # the entry before the forced 1.0f lies above it
    rows = r("penultimate_above_one")[272:400].reshape(8, 16)
    assert rows[3, 14] > 1 and rows[6, 14] > 1 and rows[3, 15] == 1 and rows[6, 15] == 1
    for k in range(8):
        h = r(f"one_hot_row{k}")
        assert valid(f"one_hot_row{k}") == 1 and (h[264:264 + k] == 0).all() and (h[264 + k:272] == 1).all()
        assert all(same(h[272 + 16 * v:288 + 16 * v], UNIFORM) for v in range(8) if v != k)
    for l in ("one_hot_lower", "zero", "denormal"):
        assert valid(l) == 0 and same(r(l)[272:528].reshape(16, 16), np.tile(UNIFORM, (16, 1))), l
    assert (r("denormal")[:256] > 0).all() and (r("denormal")[:256] < F(1.2e-38)).all() and r("denormal")[528] > 0
    # a row of 3e38: the row sum is inf, 1 / inf = 0, and the row is 0 (finite * 0) and then NaN (inf * 0) up to the forced 1
    h = r("row_3e38")
    assert np.isinf(h[260]) and np.isinf(h[528]) and valid("row_3e38") == 1
    row4 = h[272 + 64:272 + 80]
    assert row4[0] == 0 and np.isnan(row4[4:15]).all() and row4[15] == 1
    assert np.isnan(h[268:271]).all() and h[271] == 1 and (h[264:268] == 0).all()   # the marginal: finite * 0, then inf * 0
    # a NaN cell: every comparison with the NaN total fails - the record is INVALID, its row and the marginal are NaN
    h = r("nan_cell")
    assert np.isnan(h[528]) and valid("nan_cell") == 0 and np.isnan(h[258]) and np.isnan(h[272 + 32 + 11:272 + 47]).all() and h[272 + 47] == 1
    # an inf cell: VALID, inv_total = 0, the marginal is 0 up to the inf row sum and NaN (inf * 0) from it on
    h = r("inf_cell")
    assert np.isinf(h[528]) and valid("inf_cell") == 1 and (h[264:269] == 0).all() and np.isnan(h[269:271]).all() and h[271] == 1
    # negative cells: rows that go down
    rows = r("negative_rows")[272:400].reshape(8, 16)
    assert valid("negative_rows") == 1 and (np.diff(rows[1]) < 0).any() and (np.diff(rows[6]) < 0).any()
    p = r("decades_24")[:256]
    assert p.max() / p.min() > 1e23 and valid("decades_24") == 1
    assert all(valid(l) == 1 for l in S.SAMPLED)


def test_nan_marginal_of_a_nan_cell(rs, restated):
    """the NaN cell's marginal, spelled out: running is NaN from row 2 on and NaN * 0 is NaN"""
    h = rec_of(rs, restated, "nan_cell")
    assert (h[264:266] == 0).all() and np.isnan(h[266:271]).all() and h[271] == 1


def test_lower_hemisphere_rows_are_uniform(restated):
    """application_state.h:560-565: row_cdfs[128 .. 255] = (u + 1) * (1 / 16), whatever the grid holds"""
    assert same(restated[:, 272 + 128:528].reshape(-1, 8, 16), np.broadcast_to(UNIFORM, (len(restated), 8, 16)))


def test_fused_luminance_changes_a_bit(rs):
    """the random grids hold rgb triples for which a contracted 0.2126f * r + 0.7152f * g + 0.0722f * b rounds differently: a
    build of the kernel that fuses it would be seen.  A handful of the differing cells is confirmed in exact arithmetic."""
    rgb = rs["rgb"][rs["n_edges"]:]
    plain, fused = S.luminance(rgb), S.luminance_fused(rgb)
    differ = np.argwhere(bits(plain) != bits(fused))
    assert len(differ) > 100
    exact = [S.fused_differs_exactly(rgb[i, c]) for i, c in differ[:8]]
    assert all(exact)
    assert not same(S.restate_records(fused), S.restate_records(plain))


# ---- 2. records: the oracle against the compiled reference ------------------------------------------------------------------------
def ask_records(kind, src):
    L = ref_int_lib()
    out = np.zeros((len(src), 530), F)
    for k in range(len(src)):
        g = np.ascontiguousarray(src[k], F)
        assert L.ref_grid_record(kind, g.ctypes.data, out[k].ctypes.data) == 0
    return out


def ref_records(ref, rs, kind):
    """the compiled reference's records of the set for kind 1 (rgb) or 2 (pdf): the edge grids whole, the random ones as SHA-256"""
    src = rs["rgb"] if kind == 1 else rs["pdf"]
    ne = rs["n_edges"]

    def ask():
        out = ask_records(kind, src)
        return dict(in_edges=src[:ne], edges=out[:ne], in_random_sha=np.array([sha(g) for g in src[ne:]]),
                    random_sha=np.array([sha(r[UPPER]) for r in out[ne:]]))
    r = ref(f"records/kind{kind}", ask)
    assert same(r["in_edges"], src[:ne]) and np.array_equal(r["in_random_sha"], np.array([sha(g) for g in src[ne:]])), \
        "the record cases differ from the recorded ones - re-record"
    return r


def oracle_kind1(rgb):
    """the oracle's precomputeCDFs of rgb grids: a soup of as many triangles, po_scene_set_radiosity_grids, po_scene_get_cdfs"""
    n = len(rgb)
    verts = np.zeros((n, 4, 3), F); verts[:, 1, 0] = 1; verts[:, 2, 1] = 1; verts[:, :, 2] = np.arange(n)[:, None]
    s = OracleScene.from_arrays(np.zeros(n, np.int32), verts, np.tile([0, 0, 1], (n, 1)), np.full((n, 3), 0.5, F), np.zeros((n, 3), F))
    s.set_radiosity_grids(rgb)
    return s.cdfs()


@pytest.mark.parametrize("kind", [1, 2])
def test_oracle_records_are_the_references(ref, rs, restated, kind):
    r = ref_records(ref, rs, kind)
    got = oracle_kind1(rs["rgb"]) if kind == 1 else oracle_cdf_records(rs["pdf"])
    ne = rs["n_edges"]
    for k in range(ne):
        assert same(got[k, UPPER], r["edges"][k, UPPER]), (rs["labels"][k], kind)
    bad = [rs["labels"][ne + k] for k in range(len(got) - ne) if not np.array_equal(sha(got[ne + k, UPPER]), r["random_sha"][k])]
    assert not bad, bad[:5]
    assert same(got[:, 400:528].reshape(-1, 8, 16), np.broadcast_to(UNIFORM, (len(got), 8, 16)))
    assert same(got, restated)                         # and the numpy restatement is the oracle's, all 530 words


def test_record_fixture_is_small(ref):
    if not ref.record:                                 # while recording, the file is written when the module is done
        assert os.path.getsize(GOLDEN) < 400 * 1024


# ---- sampling on the valid edge records -----------------------------------------------------------------------------------------------
def sampling_cases(rec):
    """the thinned script lists of tests/test_integrator_vs_ref.py for one record"""
    normals = normal_cases()
    gs = flat_cases(normals[::3], grid_scripts(rec)[::3])
    pd = pdf_cases(normals[::3])
    mis = {frac: flat_cases(normals[::6], mis_scripts(rec, frac)[::2]) for frac in MIS_FRACTIONS}
    return gs, pd, mis


def recorded_for(ref, key, ask, inp):
    r = ref(key, lambda: ask(inp))
    for k, v in inp.items():
        v = np.asarray(v)
        ok = same(r[k], v) if v.dtype == F else np.array_equal(np.asarray(r[k]), v)
        assert ok, f"{key}: the cases' {k} differ from the recorded ones - re-record"
    return r


@pytest.mark.parametrize("label", S.SAMPLED)
def test_sampling_the_edge_records_vs_ref(ref, rs, restated, label):
    """Grid::sample, computePDF and sampleMIS of the compiled reference over the valid edge records - NaN CDF entries, rows that go
    down, a total one ulp above 1e-6f - against the oracle's: directions, pdfs, weights bit for bit (NaN = NaN), verdicts and
    draw counts exactly."""
    rec = np.ascontiguousarray(rec_of(rs, restated, label))
    gs, pd, mis = sampling_cases(rec)
    L = oracle_lib()
    nn, ww = gs
    r = recorded_for(ref, f"grid_sample/{label}", ask_grid_sample, dict(in_rec=rec, in_normal=nn, in_words=ww.astype(np.uint32)))
    assert int(np.asarray(r["valid"]).reshape(-1)[0]) == 1
    for k in range(len(nn)):
        d, pdf, used = po_grid_sample(rec, nn[k], ww[k])
        assert used == r["used"][k] == 4, (label, k)
        assert same(d, r["dir"][k]) and same(pdf, r["pdf"][k]), (label, nn[k], ww[k], d, r["dir"][k], pdf, r["pdf"][k])
    nn, dd = pd
    r = recorded_for(ref, f"grid_pdf/{label}", ask_grid_pdf, dict(in_rec=rec, in_normal=nn, in_dir=dd))
    got = [L.po_grid_pdf(rec.ctypes.data, np.ascontiguousarray(d).ctypes.data, np.ascontiguousarray(n).ctypes.data) for n, d in zip(nn, dd)]
    assert same(np.array(got, F), r["pdf"]), label
    for frac, (nn, ww) in mis.items():
        r = recorded_for(ref, f"sample_mis/{label}/{frac}", ask_sample_mis,
                         dict(in_rec=rec, in_frac=np.array([frac], F), in_normal=nn, in_words=ww.astype(np.uint32)))
        for k in range(len(nn)):
            d, wt, ub, used = po_sample_mis(rec, nn[k], frac, ww[k])
            assert (ub, used) == (r["used_bsdf"][k], r["used"][k]), (label, frac, nn[k], ww[k])
            assert same(d, r["dir"][k]) and same(wt, r["weight"][k]), (label, frac, nn[k], ww[k], wt, r["weight"][k])


def test_inf_cell_always_samples_row_7(ref, rs, restated):
    """a valid record with a NaN marginal: xi < NaN is never true, so the search falls through to the forced last entry"""
    rec = np.ascontiguousarray(rec_of(rs, restated, "inf_cell"))
    nn, ww = sampling_cases(rec)[0]
    r = recorded_for(ref, "grid_sample/inf_cell", ask_grid_sample, dict(in_rec=rec, in_normal=nn, in_words=ww.astype(np.uint32)))
    assert np.isnan(rec[269:271]).all()
    # pdf = cell / max(total, 1e-6f) / solid angle = finite / inf = 0 for every cell of row 7
    assert (r["pdf"] == 0).all() and np.isfinite(r["dir"]).all()
    z = np.einsum("ij,ij->i", r["dir"].astype(D), r["in_normal"].astype(D))
    assert ((z >= np.cos(np.pi / 2 - 0.01) - 1e-3) & (z <= np.cos(7 * np.pi / 16) + 1e-3)).all()   # theta in [7 pi / 16, pi / 2 - 0.01]; 1e-3: the frame at n.z = -0.9999999


# ---- 3. filter ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fs():
    return S.filter_set()


def filter_runs(fs):
    """(indices, rgb, counts, bilateral, ss, sr) of every launch: the cases of one sigma pair, Gaussian and bilateral"""
    for (ss, sr), idx in S.filter_groups(fs).items():
        rgb = np.array([fs[k]["rgb"] for k in idx], F); cnt = np.array([fs[k]["grid"] for k in idx], F)
        for bil in (0, 1):
            yield idx, rgb, cnt, bil, F(ss), F(sr)


@pytest.fixture(scope="module")
def filtered(fs):
    """the float32 restatement of every case: {bilateral: (formfactor (n, 256), radiosity (n, 256))}"""
    out = {b: [np.zeros((len(fs), 256), F), np.zeros((len(fs), 256), F)] for b in (0, 1)}
    for idx, rgb, cnt, bil, ss, sr in filter_runs(fs):
        ff, rad = S.restate_filter_pdfs(rgb, cnt, bil, ss, sr)
        out[bil][0][idx] = ff; out[bil][1][idx] = rad
    return out


def fcase(fs, label):
    return next(k for k, c in enumerate(fs) if c["label"] == label)


def test_filter_grids_are_the_luminance_of_their_rgb(fs):
    for c in fs:
        assert same(S.luminance(c["rgb"]), c["grid"]), c["label"]


def test_filter_oracle_is_the_restatement(fs, filtered):
    """oracle/ptmi_oracle.c's filter (the code inside po_scene_apply_grid_filter) against the numpy restatement, bit for bit, on
    every case, as counts and as rgb, Gaussian and bilateral"""
    for idx, rgb, cnt, bil, ss, sr in filter_runs(fs):
        off, orad = oracle_filter_pdfs(rgb, cnt, bil, ss, sr)
        for j, k in enumerate(idx):
            assert same(off[j], filtered[bil][0][k]) and same(orad[j], filtered[bil][1][k]), (fs[k]["label"], bil)
            assert same(filtered[bil][0][k], filtered[bil][1][k]), fs[k]["label"]     # the same 256 floats either way
        zff, _ = oracle_filter_pdfs(rgb, None, bil, ss, sr)
        assert (bits(zff) == 0).all()                                                  # counts = NULL: +0 everywhere


def test_filter_labels_sit_on_their_edges(fs, filtered):
    raw = lambda label, bil: S.restate_filter_float(fs[fcase(fs, label)]["grid"].reshape(1, 256), bil, fs[fcase(fs, label)]["sigma_spatial"],
                                                    fs[fcase(fs, label)]["sigma_range"])[0]
    # an impulse's footprint: rows i - 2 .. i + 2 clipped, columns j - 2 .. j + 2 wrapped
    ii, jj = np.mgrid[0:16, 0:16]
    for c in range(256):
        i, j = divmod(c, 16)
        want = (np.abs(ii - i) <= 2) & (np.minimum((jj - j) % 16, (j - jj) % 16) <= 2)
        for bil in (0, 1):
            got = filtered[bil][0][fcase(fs, f"impulse{c}")].reshape(16, 16)
            assert np.array_equal(got > 0, want) and np.array_equal(got != 0, want), (c, bil)
    # the range weight at ptmi_expf's cut-off
    w = lambda l: S.gaussian_weight(fs[fcase(fs, l)]["step"], S.SIGMA_R)
    a = lambda l: S.range_argument(fs[fcase(fs, l)]["step"])
    assert w("range_last_nonzero") == F(1e-45) and w("range_first_zero") == 0
    assert a("range_cut_at") >= F(-104) and a("range_cut_below") < F(-104) and a("range_cut_at") > a("range_cut_below")
    assert S.up(fs[fcase(fs, "range_cut_at")]["rgb"][8, 1]) == fs[fcase(fs, "range_cut_below")]["rgb"][8, 1]
    # an inf neighbour: the Gaussian's footprint is inf (inf * w / total); the bilateral's is NaN (the range weight is 0 and
    # inf * 0 is NaN) except at the inf cell itself, whose own range distance inf - inf makes the total weight NaN: it keeps inf
    k = fcase(fs, "inf_neighbour")
    fp = (np.abs(ii - 6) <= 2) & (np.abs(jj - 6) <= 2)
    assert np.isinf(raw("inf_neighbour", 0).reshape(16, 16)[fp]).all() and np.isfinite(raw("inf_neighbour", 0).reshape(16, 16)[~fp]).all()
    b1 = raw("inf_neighbour", 1).reshape(16, 16); ring = fp.copy(); ring[6, 6] = False
    assert np.isnan(b1[ring]).all() and np.isinf(b1[6, 6]) and np.isfinite(b1[~fp]).all()
    g0 = filtered[0][0][k].reshape(16, 16)                                               # the Gaussian's sum is inf: x / inf = 0, inf / inf = NaN
    assert np.isnan(g0[fp]).all() and (g0[~fp] == 0).all() and np.isnan(filtered[1][0][k]).all()   # the bilateral's sum is NaN
    # a NaN cell: outside its footprint the filtered grid is that of the grid without it, bit for bit.  Inside, the Gaussian
    # gives NaN; under the bilateral filter the NaN range weight makes the total NaN and each cell keeps its centre value.
    # Either way the sum is NaN, a NaN sum is not <= 1e-12f, and every normalised value is NaN
    for bil in (0, 1):
        a_, b_ = raw("nan_cell", bil).reshape(16, 16), raw("nan_cell_control", bil).reshape(16, 16)
        assert same(a_[~fp], b_[~fp]) and np.isfinite(b_).all() and np.isnan(a_[6, 6])
        assert np.isnan(a_[fp]).all() if bil == 0 else same(a_[fp], fs[fcase(fs, "nan_cell")]["grid"].reshape(16, 16)[fp])
        assert np.isnan(filtered[bil][0][fcase(fs, "nan_cell")]).all()
    # sigmas: 2 * sigma * sigma is 0 at 1e-23f - the centre weight is exp(-0 / 0) = NaN, the total NaN, and every cell keeps its
    # centre value; the smallest sigma with a nonzero 2 * sigma * sigma gives weights 1 (centre) and 0: again the centre value
    tiny = S.smallest_sigma()
    assert F(2) * F(1e-23) * F(1e-23) == 0 and F(2) * tiny * tiny > 0 and F(2) * S.dn(tiny) * S.dn(tiny) == 0
    assert np.isnan(S.gaussian_weight(F(0), F(1e-23))) and S.gaussian_weight(F(1), F(1e-23)) == 0
    for l in ("sigma_spatial_1e-23", "sigma_both_1e-23", "sigma_spatial_smallest"):
        for bil in (0, 1):
            assert same(raw(l, bil), fs[fcase(fs, l)]["grid"]), (l, bil)
    assert same(raw("sigma_range_1e-23", 1), fs[fcase(fs, "sigma_range_1e-23")]["grid"])     # NaN at the centre, 0 elsewhere
    assert not same(raw("sigma_range_1e-23", 0), fs[fcase(fs, "sigma_range_1e-23")]["grid"])
    assert S.gaussian_weight(np.sqrt(F(8)), F(1e18)) == 1                                      # every weight 1: a box filter
    # the sum of the filtered values at 1e-12f: below and AT it the values stay as they are (the test is <=)
    for bil, tag in ((0, "g"), (1, "b")):
        for name, want_sum, divided in (("below", S.dn(EPS_SUM), False), ("at", EPS_SUM, False), ("above", S.up(EPS_SUM), True)):
            k = fcase(fs, f"sum_{name}_{tag}")
            f, s = S.restate_normalize(raw(f"sum_{name}_{tag}", bil).reshape(1, 256))
            assert s[0] == want_sum, (name, tag, s[0])
            assert same(filtered[bil][0][k], f[0]) and (same(f[0], raw(f"sum_{name}_{tag}", bil)) != divided)
    # a sum whose order matters
    _, s = S.restate_normalize(raw("sum_order", 0).reshape(1, 256))
    _, sp = S.restate_normalize(raw("sum_order", 0).reshape(1, 256), pairwise=True)
    assert s[0] == F(0.7152) * F(2.0 ** 24) and sp[0] > s[0]


# ---- 4. grid update --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worlds():
    return S.grid_worlds()


@pytest.fixture(scope="module")
def grids(worlds):
    return {w["label"]: S.restate_grid_update(w) for w in worlds}


def world(worlds, label):
    return next(w for w in worlds if w["label"] == label)


def oracle_world(w):
    f = w["filtering"] or (0, S.SIGMA_S, S.SIGMA_R)
    return oracle_radiosity_grid(w["centre"], w["normal"], w["ff"], w["rad"], w["filtering"] is not None, f[0], F(f[1]), F(f[2]))


def test_grid_oracle_is_the_restatement(worlds, grids):
    """oracle/ptmi_oracle.c's grid update (the code inside po_radiosity_solve) against the numpy restatement, bit for bit"""
    for w in worlds:
        assert same(oracle_world(w), grids[w["label"]]), w["label"]


def test_grid_labels_sit_on_their_edges(worlds, grids):
    assert sorted(len(w["centre"]) for w in worlds)[:4] == [1, 2, 2, 2] and {len(w["centre"]) for w in worlds} >= set(range(1, 6)) | {40, 2050}
    assert (bits(grids["n1"]) == 0).all()                                              # the diagonal alone: skipped
    for w in worlds:
        assert np.isfinite(w["centre"]).all() and np.isfinite(w["normal"]).all() and (np.abs(w["normal"]).sum(axis=1) > 0).all()
    # every kind of form factor: +0, -0 and a negative are skipped, a denormal, an inf and a NaN are taken
    w = world(worlds, "ff_kinds"); g = grids["ff_kinds"][0]
    cell = dict(zip(w["kinds"], w["cells"]))
    for k in ("plus_zero", "minus_zero", "negative"):
        assert (bits(g[cell[k]]) == 0).all(), k
    assert (g[cell["denormal"]] > 0).all() and np.isinf(g[cell["inf"]]).all() and np.isnan(g[cell["nan"]]).all()
    assert same(g[cell["ordinary"]], F(0.125) * w["rad"][w["kinds"].index("ordinary")])
    assert int(np.count_nonzero(bits(g).any(axis=1))) == 4                              # and the diagonal 0.9 is nowhere
    for j, c in zip(range(1, len(w["cells"])), w["cells"][1:]):
        assert S.grid_index(S.world_geometry(w, 0)[1][j], w["normal"][0]) == c
    # centres that coincide, and distances below, at and above 1e-6f as the restatement computes them
    w = world(worlds, "near"); r, dirs = S.world_geometry(w, 0)
    nr = w["near"]
    assert r[nr["coincide"]] == 0 and r[nr["below"]] == S.dn(EPS_TOTAL) and r[nr["at"]] == EPS_TOTAL and r[nr["above"]] == S.up(EPS_TOTAL)
    want = np.zeros(3, F)
    for j in (nr["at"], nr["above"]):                                                  # r < 1e-6f skips; at 1e-6f it does not
        assert S.grid_index(dirs[j], w["normal"][0]) == 8 * 16
        want = want + F(0.25) * w["rad"][j]
    assert same(grids["near"][0][8 * 16], want)
    # a source through the centre of each of the 256 cells: the float32 direction lands in the labelled cell
    for label in ("cells_z", "cells_tilted"):
        w = world(worlds, label); _, dirs = S.world_geometry(w, 0)
        for c in range(256):
            assert S.grid_index(dirs[1 + c], w["normal"][0]) == c, (label, c)
            assert same(grids[label][0][c], w["ff"][0, 1 + c] * w["rad"][1 + c])
    # several sources in one cell: ascending j gives 2^24, any other order more
    for label in ("order_n9", "order_n2050"):
        w = world(worlds, label); first, c = w["group"]; _, dirs = S.world_geometry(w, 0)
        assert all(S.grid_index(dirs[first + k], w["normal"][0]) == c for k in range(4))
        assert (grids[label][0][c] == F(2.0 ** 24)).all()
    assert world(worlds, "order_n2050")["group"][0] == 2046                            # j = 2046 .. 2049: across the 2048-entry chunk
    # a NaN cell under the rgb filter: outside its footprint the control world's bits; inside NaN (Gaussian) or, the total
    # weight being NaN, the unfiltered centre value (bilateral)
    ii, jj = np.mgrid[0:16, 0:16]
    fp = (np.abs(ii - 5) <= 2) & (np.minimum(jj % 16, (-jj) % 16) <= 2)
    for kind in ("gaussian", "bilateral"):
        a_, b_ = grids[f"filtered_nan_{kind}"][0].reshape(16, 16, 3), grids[f"filtered_nan_control_{kind}"][0].reshape(16, 16, 3)
        assert same(a_[~fp], b_[~fp]) and np.isfinite(b_).all() and np.isnan(a_[5, 0]).all()
        unfiltered = S.restate_grid_update(dict(world(worlds, f"filtered_nan_{kind}"), filtering=None))[0].reshape(16, 16, 3)
        assert np.isnan(a_[fp]).all() if kind == "gaussian" else same(a_[fp], unfiltered[fp])
    for label in ("single_source_gaussian", "single_source_bilateral"):
        g = grids[label][0].reshape(16, 16, 3)
        assert np.count_nonzero(g.any(axis=2)) == 25 and g[2, 15].all() and g[2, 1].all() and g[0, 0].all()   # the wrap to columns 0, 1


# ---- 5. binary64 ---------------------------------------------------------------------------------------------------------------------
def rel_err(a32, a64):
    a32 = np.asarray(a32, D); a64 = np.asarray(a64, D)
    with np.errstate(all="ignore"):
        e = np.abs(a32 - a64) / np.abs(a64)
    e[(a64 == 0) & (a32 == 0)] = 0
    return e


def test_float32_restatements_stay_near_binary64(rs, restated, fs, filtered, worlds, grids, capsys):
    """The float32 restatements against the same formulas in binary64 over the ORDINARY cases.  The bounds are four times the
    largest relative error measured here (guided_record_sets.py: RECORD_BOUND, FILTER_BOUND, GRID_BOUND); a case is left out
    only with its reason - a non-finite input, a threshold binary64 takes the other way, negative cells that cancel - and the
    left-out cases are fewer than a quarter of each set."""
    # records: every CDF entry, row sum and the total
    ordinary = [k for k, l in enumerate(rs["labels"]) if l not in S.RECORD_NOT_ORDINARY]
    assert len(rs["labels"]) - len(ordinary) < len(rs["labels"]) / 4 and set(S.RECORD_NOT_ORDINARY) <= set(rs["labels"])
    r64 = S.restate_records(rs["pdf"].astype(D), D)
    assert np.array_equal(restated[ordinary, 529].view(np.int32), r64[ordinary, 529].astype(np.int32))
    e_rec = rel_err(restated[ordinary, 256:529], r64[ordinary, 256:529]).max()
    # filter: every normalised value
    ordinary = [k for k, c in enumerate(fs) if S.filter_not_ordinary(c["label"]) is None]
    assert len(fs) - len(ordinary) < len(fs) / 4
    e_fil = 0.0
    for idx, rgb, cnt, bil, ss, sr in filter_runs(fs):
        keep = [j for j, k in enumerate(idx) if k in set(ordinary)]
        if keep:
            ff64, _ = S.restate_filter_pdfs(rgb[keep].astype(D), cnt[keep].astype(D), bil, ss, sr, D)
            e_fil = max(e_fil, rel_err(filtered[bil][0][[idx[j] for j in keep]], ff64).max())
    # grid update: every cell
    ordinary = [w for w in worlds if w["label"] not in S.GRID_NOT_ORDINARY]
    assert len(worlds) - len(ordinary) < len(worlds) / 4
    e_grid = max(rel_err(grids[w["label"]], S.restate_grid_update(w, D)).max() for w in ordinary)
    with capsys.disabled():
        print(f"\n[guided record sets] float32 vs binary64: records {e_rec:.3g}, filter {e_fil:.3g}, grid update {e_grid:.3g}")
    assert e_rec <= S.RECORD_BOUND and e_fil <= S.FILTER_BOUND and e_grid <= S.GRID_BOUND
    assert e_rec >= S.RECORD_BOUND / 8 and e_fil >= S.FILTER_BOUND / 8 and e_grid >= S.GRID_BOUND / 8   # the bounds are the measured ones


# ---- 6. the mutants, on the restatement ----------------------------------------------------------------------------------------------
def changed(rs, a, b):
    return {l for l, x, y in zip(rs["labels"], a, b) if not same(x, y)}


def test_record_sets_tell_the_mutants(rs, restated):
    edges = lambda s: {l for l in s if not l.startswith("random")}
    assert edges(changed(rs, restated, S.restate_records(rs["pdf"], row_sum_lt="le"))) == {"row_sum_at"}
    assert edges(changed(rs, restated, S.restate_records(rs["pdf"], valid_gt="ge"))) == {"total_at"}
    assert "inverse_not_quotient" in changed(rs, restated, S.restate_records(rs["pdf"], divide=True))
    dropped = changed(rs, restated, S.restate_records(rs["pdf"], force_last=False))
    assert {"total_at", "total_below", "zero", "inf_cell", "row_3e38", "one_hot_lower"} <= dropped
    assert {"row_order"} <= changed(rs, restated, S.restate_records(rs["pdf"], descending=True))
    assert len(changed(rs, restated, S.restate_records(S.luminance_fused(rs["rgb"])))) > 50


def test_filter_sets_tell_the_mutants(fs, filtered):
    hit = {m: set() for m in ("clamp_phi", "le", "pairwise")}
    for idx, rgb, cnt, bil, ss, sr in filter_runs(fs):
        for m, kw in (("clamp_phi", dict(clamp_phi=True)), ("le", dict(le=False)), ("pairwise", dict(pairwise=True))):
            ff, _ = S.restate_filter_pdfs(rgb, cnt, bil, ss, sr, **kw)
            hit[m] |= {(fs[k]["label"], bil) for j, k in enumerate(idx) if not same(ff[j], filtered[bil][0][k])}
    wrap = {f"impulse{16 * i + j}" for i in range(16) for j in (0, 1, 14, 15)}
    assert {l for l, _ in hit["clamp_phi"]} >= wrap
    # at these magnitudes every range weight is exactly 1, so the bilateral sum is the Gaussian's and both searches agree
    assert hit["le"] == {(l, b) for l in ("sum_at_g", "sum_at_b") for b in (0, 1)}
    assert ("sum_order", 0) in hit["pairwise"] and ("sum_order", 1) in hit["pairwise"]


def test_grid_sets_tell_the_mutants(worlds, grids):
    def hit(**kw):
        return {w["label"] for w in worlds if len(w["centre"]) < 100 and not same(S.restate_grid_update(w, **kw), grids[w["label"]])}
    assert hit(take="gt") == {"ff_kinds"}                                               # the line before this change: the NaN form factor
    assert hit(r_skip="le") == {"near"}
    assert "order_n9" in hit(descending=True)
    # EQUIVALENT: without the `j != i` test the diagonal entry has r = 0 exactly and is skipped by `r < 1e-6f`
    assert hit(skip_self=False) == set() and all((np.diag(w["ff"]) != 0).any() for w in worlds if w["label"].startswith("random"))
    w = world(worlds, "order_n2050")
    rows = dict(w, ff=w["ff"] * (np.arange(2050) == 0)[:, None])                        # receiver 0 alone: the other rows are one term each
    assert not same(S.restate_grid_update(rows, descending=True)[0], grids["order_n2050"][0])


# ---- 7. the hooks' argument checks that need no GPU -------------------------------------------------------------------------------------
def test_hooks_reject_a_null_context():
    import ptmi
    L = ptmi.lib()
    a = np.zeros(1024, F); out = np.zeros(1024, F)
    p = lambda x: x.ctypes.data
    assert L.ptmi_debug_cdf_records(None, 1, 2, p(a), p(out)) == -1 and b"NULL" in L.ptmi_last_error()
    assert L.ptmi_debug_filter_pdfs(None, 1, p(a), None, 1, 1.5, 0.3, p(out), p(out)) == -1
    assert L.ptmi_debug_radiosity_grid(None, 1, p(a), p(a), p(a), p(a), 0, 1, 1.5, 0.3, p(out)) == -1
    r = ptmi.Renderer.__new__(ptmi.Renderer)                                            # the wrappers' shape checks, before any call
    r.L, r.h = L, C.c_void_p()
    with pytest.raises(ValueError):
        r.debug_cdf_records(1, np.zeros((1, 256, 4), F))
    with pytest.raises(ValueError):
        r.debug_filter_pdfs(np.zeros((1, 256, 3), F), counts=np.zeros((2, 256), F))
    with pytest.raises(ValueError):
        r.debug_radiosity_grid(np.zeros((2, 3), F), np.zeros((2, 3), F), np.zeros((2, 3), F), np.zeros((2, 3), F))
