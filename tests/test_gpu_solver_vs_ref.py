"""The HIP radiosity solver against the compiled REFERENCE's recorded answers (tests/golden/ref_solver.npz), directly: not
through the oracle.  The cases are those of tests/test_solver_vs_ref.py (tests/solver_ref_sets.py); the record keeps a hash of
each case's inputs, so an answer is never compared with a case it was not recorded for.  Reads only the record: neither the
reference tree nor oracle/_ref is needed here.

run_radiosity_solver on the same scenes and parameters (form-factor rows of both kernels with num_iterations = 0, whole solves
with 0, 1 and 3 iterations, unfiltered, bilateral and Gaussian, and with an infinite emitter); the n = 257 scene through the
solver's walk 0 and its certified walk; debug_grid_index, debug_radiosity_grid, debug_filter_pdfs and apply_grid_filter (whose
result is what filtered_pdfs returns) on the recorded inputs.  Bit for bit, NaN counted equal to NaN (its sign and payload are
the hardware's).  Nothing is larger than 257 primitives with 8 samples; the file takes a few seconds on an MI355X.

One answer is not a function of its inputs in the reference itself: with num_iterations = 0 the radiosity grid is what the
Monte-Carlo kernel's float atomics left, in whatever order the threads came.  The record holds the harness's order (ascending
j), the device has its own, and neither is the reference's.  What both must be is A sum of the same terms - every term is
non-negative and is computed by the same arithmetic, and the reference's count grid says how many, m, fell into a cell.  Any
order of adding m non-negative floats is within (m - 1) 2^-24 (1 + (m - 1) 2^-24) of their exact sum, relative; two orders
therefore within twice that of each other.  sum_of_same_terms() requires this per cell and channel, on the rows the record
keeps whole, and bit equality wherever m <= 1.
"""
import numpy as np
import pytest

import ptmi
import solver_ref_sets as S
from oracle_binding import OracleScene

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def rec():
    return dict(np.load(S.GOLDEN))


def sub(rec, key, name):
    return dict(sha=rec[f"{key}/{name}_sha"][0], sha_nan=rec[f"{key}/{name}_sha"][1], head=rec[f"{key}/{name}_head"])


def recorded_inputs(rec, key, in_sha):
    assert np.array_equal(rec[f"{key}/in_sha"], in_sha), f"{key}: the case's inputs differ from the recorded ones - re-record"


def same(a, b):
    return S.canon(np.ascontiguousarray(a, F)).tobytes() == S.canon(np.ascontiguousarray(b, F)).tobytes()


def sum_of_same_terms(got, rec_head, counts_head):
    """got, rec_head: (rows, 256, 3) sums of the same m = counts_head (rows, 256) non-negative terms in two orders (docstring)"""
    got = np.asarray(got, np.float64)[:len(rec_head)]; want = np.asarray(rec_head, np.float64)
    m1 = np.maximum(np.asarray(counts_head, np.float64) - 1, 0)[..., None]
    bound = 2 * m1 * 2.0 ** -24 * (1 + m1 * 2.0 ** -24) * np.abs(want)
    return bool((np.abs(got - want) <= bound).all())


def solve(R, scene, walk=-1, **params):
    R.load_scene_arrays(*S.scene_arrays(scene))
    R.set_solver_walk(walk)
    try:
        st = R.run_radiosity_solver(**params)
    finally:
        R.set_solver_walk(-1)
    assert walk < 0 or st.walk == walk, (scene, walk, st.walk)
    return R.radiosity_solution()


def test_gpu_grid_index_is_the_references(R, rec):
    dirs, nrms = S.grid_index_cases()
    recorded_inputs(rec, "grid_index", S.inputs_sha(dirs, nrms))
    got = R.debug_grid_index(dirs, nrms)
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != rec["grid_index/index"])
    assert len(bad) == 0, (len(bad), dirs[bad[:3]], nrms[bad[:3]])


# the n = 257 scene through the reference's tree (walk 0) and through the certified walk (2), which must give the same rows
FF_GPU_CASES = [(c, -1) for c in S.FF_ROW_CASES if c[0] != "soup257"] + [(c, w) for c in S.FF_ROW_CASES if c[0] == "soup257" for w in (0, 2)]


@pytest.mark.parametrize("case,walk", FF_GPU_CASES, ids=lambda v: S.ff_key(v) if isinstance(v, tuple) else f"walk{v}")
def test_gpu_form_factor_rows_are_the_references(case, walk, R, rec):
    scene, mc, m = case
    key = S.ff_key(case); rows = S.ff_rows(scene)
    recorded_inputs(rec, key, S.inputs_sha(S.scene_sha(scene), rows))
    sol = solve(R, scene, walk, num_iterations=0, mc_samples=m, use_monte_carlo=mc)
    assert S.same_bulky(sol["form_factors"][rows], sub(rec, key, "ff"), True), "form factors"
    assert S.same_bulky(sol["grid"][rows], sub(rec, key, "grid"), True), "count grid"
    assert sum_of_same_terms(sol["radiosity_grid"][rows], rec[f"{key}/rad_grid_head"], rec[f"{key}/grid_head"]), "radiosity grid of the form-factor kernel"
    if not mc:
        assert not sol["radiosity_grid"].any()


@pytest.mark.parametrize("case", S.SOLVE_CASES, ids=S.solve_key)
def test_gpu_whole_solve_is_the_references(case, R, rec):
    key = S.solve_key(case)
    recorded_inputs(rec, key, S.scene_sha(case[0]))
    sol = solve(R, case[0], **S.solve_params(case))
    for k in ("radiosity", "unshot"):
        assert same(sol[k], rec[f"{key}/{k}"]), (k, np.argwhere(S.canon(sol[k]) != S.canon(rec[f"{key}/{k}"]))[:5])
    for k in ("form_factors", "grid"):
        assert S.same_bulky(sol[k], sub(rec, key, k), True), k
    if case[1] == 0 and case[3]:                         # the Monte-Carlo kernel's own grid: a sum in the device's order
        assert sum_of_same_terms(sol["radiosity_grid"], rec[f"{key}/radiosity_grid_head"], rec[f"{key}/grid_head"]), "radiosity_grid"
    else:
        assert S.same_bulky(sol["radiosity_grid"], sub(rec, key, "radiosity_grid"), True), "radiosity_grid"


def filter_group(rec, ss, sr, idx, bil, with_counts):
    from test_solver_vs_ref import filter_group_key
    cases = S.filter_cases()
    rgb = np.array([cases[k]["rgb"] for k in idx], F); counts = np.array([cases[k]["counts"] for k in idx], F) if with_counts else None
    key = filter_group_key(ss, sr, bil, with_counts)
    recorded_inputs(rec, key, S.inputs_sha(rgb, counts if with_counts else np.zeros(0, F)))
    return key, rgb, counts


@pytest.mark.parametrize("bil", [1, 0], ids=["bilateral", "gaussian"])
@pytest.mark.parametrize("with_counts", [1, 0], ids=["counts", "no_counts"])
def test_gpu_filter_pdfs_are_the_references(bil, with_counts, R, rec):
    for (ss, sr), idx in S.filter_groups().items():
        key, rgb, counts = filter_group(rec, ss, sr, idx, bil, with_counts)
        ff, rad = R.debug_filter_pdfs(rgb, counts, bool(bil), ss, sr)
        assert S.same_bulky(ff, sub(rec, key, "formfactor"), True), (ss, sr, "formfactor")
        assert S.same_bulky(rad, sub(rec, key, "radiosity"), True), (ss, sr, "radiosity")


@pytest.mark.parametrize("bil", [1, 0], ids=["bilateral", "gaussian"])
def test_gpu_apply_grid_filter_is_the_references(bil, R, rec):
    """the public route: the grids set on a loaded scene, "Apply Filter & Rebuild CDFs", and the pdfs it leaves (no solve has
    run, so there are no counts)"""
    (ss, sr), idx = next(iter(S.filter_groups().items()))
    key, rgb, _ = filter_group(rec, ss, sr, idx, bil, 0)
    R.load_scene_arrays(*S.random_scene(len(idx)))
    R.set_radiosity_grids(rgb)
    ff, rad = R.apply_grid_filter(bool(bil), ss, sr)
    assert S.same_bulky(ff, sub(rec, key, "formfactor"), True) and S.same_bulky(rad, sub(rec, key, "radiosity"), True)


def test_gpu_radiosity_grid_on_worlds_is_the_references(R, rec):
    for w in S.grid_worlds():
        key = f"world/{w['label']}"
        recorded_inputs(rec, key, S.inputs_sha(w["centre"], w["normal"], w["ff"], w["rad"]))
        kw = {}
        if w["filtering"] is not None:
            bil, ss, sr = w["filtering"]
            kw = dict(enable_filtering=True, use_bilateral=bool(bil), sigma_spatial=float(ss), sigma_range=float(sr))
        got = R.debug_radiosity_grid(w["centre"], w["normal"], w["ff"], w["rad"], **kw)
        assert S.same_bulky(got, sub(rec, key, "grid"), True), w["label"]


@pytest.mark.parametrize("name", ["cbox_quads", "soup65"])
def test_gpu_radiosity_grid_on_scenes_is_the_references(name, R, rec):
    """update_radiosity_grid and the two rgb filter wrappers on real primitives; the centroids are the oracle's, which
    tests/test_oracle_vs_ref.py ties to the reference's"""
    from test_solver_vs_ref import stage_inputs
    ff, rad, _ = stage_inputs(name)
    key = f"update_grid/{name}"
    recorded_inputs(rec, key, S.inputs_sha(S.scene_sha(name), ff, rad))
    arrs = S.scene_arrays(name)
    o = OracleScene.from_arrays(*arrs)
    c = np.array([o.prim_geometry(i)[1] for i in range(o.n_prims)], F)
    assert S.same_bulky(R.debug_radiosity_grid(c, arrs[2], ff, rad), sub(rec, key, "plain"), True)
    assert S.same_bulky(R.debug_radiosity_grid(c, arrs[2], ff, rad, True, True, 1.5, 0.3), sub(rec, key, "bilateral"), True)
    assert S.same_bulky(R.debug_radiosity_grid(c, arrs[2], ff, rad, True, False, 0.7, 0.3), sub(rec, key, "gaussian"), True)
