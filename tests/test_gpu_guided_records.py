"""The kernels that turn a radiosity solution into the records guided sampling reads (csrc/radiosity.hip: ptmi_cdf_records<0|1|2>,
ptmi_filter_pdfs, ptmi_radiosity_grid) on the constructed grids, filter cases and worlds of tests/guided_record_sets.py, given
through ptmi_debug_cdf_records, ptmi_debug_filter_pdfs and ptmi_debug_radiosity_grid - which launch the product's own kernels.
Bit for bit (NaN counted equal to NaN: its sign and payload are the hardware's) against the numpy restatements, which
tests/test_guided_record_sets_host.py ties to the oracle's C and to the compiled reference; the records also against the compiled
reference's own answers in tests/golden/ref_grid_records.npz.  The public route (ptmi_set_radiosity_grids -> records ->
ptmi_apply_grid_filter -> records -> ptmi_use_raw_cdfs) must give the hooks' bits, the valid edge records are sampled through
ptmi_debug_guided_sample against the reference's recorded draws, and one guided frame over them ends the chain in pixels.
Reads only the record: no reference tree is needed here.  The whole file (40 tests) takes 1.8 s on an MI355X.
"""
import numpy as np
import pytest

import guided_record_sets as S
import ptmi
from guided_record_sets import F, bits, same
from oracle_binding import OracleScene, default_camera, sha
from test_gpu_integrator_vs_ref import keys, states_of
from test_guided_record_sets_host import GOLDEN, UNIFORM, UPPER, filter_runs
from test_integrator_vs_ref import random_soup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def rs():
    return S.record_set()


@pytest.fixture(scope="module")
def restated(rs):
    return S.restate_records(rs["pdf"])


def differing(labels, a, b):
    return [l for l, x, y in zip(labels, a, b) if not same(x, y)]


# ---- records ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_records(R, rs):
    """the three kinds on the whole set: kind 0's fourth float is NaN - it must not be read"""
    rgba = np.concatenate([rs["rgb"], np.full(rs["rgb"].shape[:2] + (1,), np.nan, F)], axis=2)
    return {0: R.debug_cdf_records(0, rgba), 1: R.debug_cdf_records(1, rs["rgb"]), 2: R.debug_cdf_records(2, rs["pdf"])}


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_gpu_records_are_the_restatement(rs, restated, device_records, kind):
    assert rs["has_rgb"].all()
    bad = differing(rs["labels"], device_records[kind], restated)
    assert not bad, bad[:8]


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_gpu_records_are_the_references(rs, recorded, device_records, kind):
    """the compiled reference's Grid::initFromRadiosity (kinds 0 and 1) / initFromFormFactor (kind 2) + buildCDFs on the same grids;
    the lower hemisphere's rows, which buildCDFs leaves out, by application_state.h:560-565"""
    got = device_records[kind]; ne = rs["n_edges"]; r = "records/kind%d/" % (2 if kind == 2 else 1)
    src = rs["pdf"] if kind == 2 else rs["rgb"]
    assert same(recorded[r + "in_edges"], src[:ne]) and np.array_equal(recorded[r + "in_random_sha"], np.array([sha(g) for g in src[ne:]]))
    bad = [rs["labels"][k] for k in range(ne) if not same(got[k, UPPER], recorded[r + "edges"][k, UPPER])]
    bad += [rs["labels"][ne + k] for k in range(len(got) - ne) if not np.array_equal(sha(got[ne + k, UPPER]), recorded[r + "random_sha"][k])]
    assert not bad, bad[:8]
    assert same(got[:, 400:528].reshape(-1, 8, 16), np.broadcast_to(UNIFORM, (len(got), 8, 16)))


def test_gpu_kind0_is_kind1(device_records):
    assert same(device_records[0], device_records[1])


# ---- filter -------------------------------------------------------------------------------------------------------------------------
def test_gpu_filter_is_the_restatement(R):
    fs = S.filter_set()
    bad = []
    for idx, rgb, cnt, bil, ss, sr in filter_runs(fs):
        want_ff, want_rad = S.restate_filter_pdfs(rgb, cnt, bil, ss, sr)
        ff, rad = R.debug_filter_pdfs(rgb, cnt, bil, ss, sr)
        bad += [(fs[k]["label"], bil, "counts") for j, k in enumerate(idx) if not same(ff[j], want_ff[j])]
        bad += [(fs[k]["label"], bil, "rgb") for j, k in enumerate(idx) if not same(rad[j], want_rad[j])]
        none_ff, none_rad = R.debug_filter_pdfs(rgb, None, bil, ss, sr)               # counts = NULL against an all-zero count grid
        zero_ff, zero_rad = R.debug_filter_pdfs(rgb, np.zeros_like(cnt), bil, ss, sr)
        assert (bits(none_ff) == 0).all() and (bits(zero_ff) == 0).all() and same(none_rad, rad) and same(zero_rad, rad)
    assert not bad, bad[:8]


# ---- grid update ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", S.grid_worlds(), ids=lambda w: w["label"])
def test_gpu_grid_update_is_the_restatement(R, w):
    f = w["filtering"] or (0, S.SIGMA_S, S.SIGMA_R)
    got = R.debug_radiosity_grid(w["centre"], w["normal"], w["ff"], w["rad"], w["filtering"] is not None, f[0], f[1], f[2])
    want = S.restate_grid_update(w)
    bad = [(i, c) for i, c in np.argwhere(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(axis=2))]
    assert not bad, bad[:8]


# ---- the public route -----------------------------------------------------------------------------------------------------------------
def soup_for(n):
    """n small triangles in a row: the geometry is irrelevant to the records"""
    verts = np.zeros((n, 4, 3), F); verts[:, 1, 0] = 1; verts[:, 2, 1] = 1; verts[:, :, 2] += np.arange(n)[:, None]
    return np.zeros(n, np.int32), verts, np.tile(np.array([0, 0, 1], F), (n, 1)), np.full((n, 3), 0.5, F), np.zeros((n, 3), F)


@pytest.mark.parametrize("bilateral,ss,sr", [(1, 1.5, 0.3), (0, 0.6, 0.3), (1, 1e-23, 0.3)])
def test_gpu_public_route_gives_the_hooks_bits(R, rs, bilateral, ss, sr):
    """ptmi_set_radiosity_grids -> records (kind 1) -> ptmi_apply_grid_filter -> pdfs and records (kind 2) -> ptmi_use_raw_cdfs ->
    records (kind 1 again) on a soup that carries the edge grids and a few random ones: the host plumbing (precomputeCDFs,
    precomputeCDFsFromFiltered, the zero count grid after host-supplied grids) adds nothing to the hooks' bits"""
    pick = list(range(rs["n_edges"])) + list(range(rs["n_edges"], rs["n_edges"] + 6))
    rgb = rs["rgb"][pick]
    R.load_scene_arrays(*soup_for(len(pick)))
    try:
        R.set_radiosity_grids(rgb)
        raw = R.debug_cdf_records(1, rgb)
        assert same(R.precomputed_cdfs(), raw)
        ff, rad = R.apply_grid_filter(bilateral, ss, sr)
        hook_ff, hook_rad = R.debug_filter_pdfs(rgb, None, bilateral, ss, sr)
        assert (bits(ff) == 0).all() and same(ff, hook_ff) and same(rad, hook_rad)
        assert same(R.precomputed_cdfs(), R.debug_cdf_records(2, hook_rad))
        R.use_raw_cdfs()
        assert same(R.precomputed_cdfs(), raw)
    finally:
        R.set_radiosity_grids(None)


# ---- sampling the valid edge records --------------------------------------------------------------------------------------------------
def test_gpu_replays_the_edge_records(R, recorded):
    """Grid::sample, computePDF and sampleMIS of the compiled reference on the valid edge records (an inf cell's NaN marginal,
    rows that go down, a total one ulp above 1e-6f, a uniform row inside a valid grid, an overflowing row), replayed through the
    bounce kernels' own device functions: values bit for bit with NaN = NaN, verdicts and draw counts exactly"""
    n = 0
    for key in keys(recorded, "grid_sample"):
        r = {k: recorded[f"{key}/{k}"] for k in ("in_rec", "in_normal", "in_words", "dir", "pdf", "used", "valid")}
        assert int(np.asarray(r["valid"]).reshape(-1)[0]) == 1
        m = len(r["in_normal"])
        out, used = R.debug_guided_sample(R.GUIDED_GRID_SAMPLE, r["in_normal"], np.zeros((m, 3), F), states_of(r["in_words"]),
                                          recs=r["in_rec"][None], rec_idx=np.zeros(m, np.int32))
        assert (used == r["used"]).all(), key
        want = np.concatenate([r["dir"], r["pdf"][:, None]], axis=1)
        bad = [k for k in range(m) if not same(out[k, :4], want[k])]
        assert not bad, (key, [(r["in_normal"][k], r["in_words"][k]) for k in bad[:5]])
        n += 1
    for key in keys(recorded, "grid_pdf"):
        r = {k: recorded[f"{key}/{k}"] for k in ("in_rec", "in_normal", "in_dir", "pdf")}
        m = len(r["in_normal"])
        out, _ = R.debug_guided_sample(R.GUIDED_GRID_PDF, r["in_normal"], r["in_dir"], np.zeros((m, 6), np.uint32),
                                       recs=r["in_rec"][None], rec_idx=np.zeros(m, np.int32))
        bad = [k for k in range(m) if not same(out[k, 3], r["pdf"][k])]
        assert not bad, (key, [(r["in_normal"][k], r["in_dir"][k]) for k in bad[:5]])
        n += 1
    for key in keys(recorded, "sample_mis"):
        r = {k: recorded[f"{key}/{k}"] for k in ("in_rec", "in_frac", "in_normal", "in_words", "dir", "weight", "used_bsdf", "used")}
        m = len(r["in_normal"])
        in3 = np.zeros((m, 3), F); in3[:, 0] = r["in_frac"][0]
        out, used = R.debug_guided_sample(R.GUIDED_MIS, r["in_normal"], in3, states_of(r["in_words"]),
                                          recs=r["in_rec"][None], rec_idx=np.zeros(m, np.int32))
        assert (used == r["used"]).all() and ((used == 3) == (r["used_bsdf"] != 0)).all(), key
        want = np.concatenate([r["dir"], r["weight"][:, None]], axis=1)
        bad = [k for k in range(m) if not same(out[k, :4], want[k])]
        assert not bad, (key, [(r["in_normal"][k], r["in_words"][k]) for k in bad[:5]])
        n += 1
    assert n == len(S.SAMPLED) * (2 + 5)                # every sampled record: sample, pdf, and MIS at five fractions


# ---- one frame ------------------------------------------------------------------------------------------------------------------------
def test_gpu_guided_frame_over_the_edge_records(R, rs):
    """a 32 x 32 frame, 3 spp, MIS sampling, on a soup whose primitives carry the valid edge records in turn, against the oracle:
    the chain constructed grid -> record -> sample -> estimator ends in pixels once"""
    arrs = random_soup(65, 65)
    grids = rs["rgb"][[S.record_index(l) for l in S.SAMPLED]][np.arange(65) % len(S.SAMPLED)]
    o = OracleScene.from_arrays(*arrs)
    o.set_radiosity_grids(grids)
    want_rgb, want_rad, _ = o.render(default_camera(), 32, 32, 3, max_depth=5, sampling_mode=3, seed_base=2023)
    R.load_scene_arrays(*arrs)
    try:
        R.set_radiosity_grids(grids)
        assert same(R.precomputed_cdfs(), o.cdfs())
        R.update_resolution(32, 32)
        R.set_config(spp=3, max_depth=5, seed_base=2023, sampling_mode=3, mis_bsdf_fraction=0.5, integrator=0)
        R.render_frame()
        rgb, rad = R.read_image()
    finally:
        R.set_config(sampling_mode=0)
        R.set_radiosity_grids(None)
    assert same(rad, want_rad) and np.array_equal(rgb, want_rgb)
    assert (want_rad > 0).any()


# ---- the hooks' argument checks -------------------------------------------------------------------------------------------------------
def test_gpu_hooks_reject_bad_arguments(R):
    L, h = R.L, R.h
    a = np.zeros(256 * 4, F); out = np.zeros(1024, F)
    p = lambda x: x.ctypes.data
    for n, kind in ((0, 0), (-1, 2), (1, 3), (1, -1)):
        assert L.ptmi_debug_cdf_records(h, n, kind, p(a), p(out)) == -1
    assert L.ptmi_debug_cdf_records(h, 1, 0, None, p(out)) == -1 and L.ptmi_debug_cdf_records(h, 1, 0, p(a), None) == -1
    assert L.ptmi_debug_filter_pdfs(h, 0, p(a), None, 1, 1.5, 0.3, p(out), p(out)) == -1
    assert L.ptmi_debug_filter_pdfs(h, 1, None, None, 1, 1.5, 0.3, p(out), p(out)) == -1
    assert L.ptmi_debug_filter_pdfs(h, 1, p(a), None, 1, 1.5, 0.3, None, p(out)) == -1
    assert L.ptmi_debug_filter_pdfs(h, 1, p(a), None, 1, 1.5, 0.3, p(out), None) == -1
    g = [p(a)] * 4
    assert L.ptmi_debug_radiosity_grid(h, 0, *g, 0, 1, 1.5, 0.3, p(out)) == -1
    for k in range(4):
        assert L.ptmi_debug_radiosity_grid(h, 1, *[None if j == k else g[j] for j in range(4)], 0, 1, 1.5, 0.3, p(out)) == -1
    assert L.ptmi_debug_radiosity_grid(h, 1, *g, 0, 1, 1.5, 0.3, None) == -1
