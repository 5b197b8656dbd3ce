"""The radiosity solver's kernels (csrc/radiosity.hip, csrc/form_factors.hip) at the sizes where they change their code path, against the oracle bit
for bit.  The kernels choose by n: the tiled Jacobi kernel iff n % 4 == 0 and n >= 64 (256-column tiles, groups of 8 rows,
a zeroed diagonal entry per row, a slower loop for tiles that hold a non-finite unshot value), the lane-per-row kernel
otherwise (1024-entry LDS chunks, dead lanes in the last workgroup), ptmi_radiosity_grid in 2048-entry chunks, the
form-factor kernel in 256-column blocks with a queue that carries over, the certified visibility walk from 256 primitives
up.  tests/ragged_scenes.py has the scenes (n random primitives for any n) and the table of cases:

    n                   Jacobi kernel   what the size is for
    1, 2, 3             lane-per-row    n - 1 clamps; one nearly empty workgroup; n = 1: no pair at all
    63 / 65             lane-per-row    below the rule / a second workgroup with one live lane
    64 / 68             tiled           one 64-column tile, exactly 8 row groups / a last group of 4 live rows
    252, 256, 260       tiled           one tile, exactly one, two (the second of 4 columns)
    255, 257            lane-per-row    either side of the certified walk's threshold; 1 live lane in the second column block
    516                 tiled           three tiles, the last of 4 columns, 4 live rows in the last group
    1025 / 1028         row / tiled     a second LDS chunk of one entry / five tiles
    2049 / 2052         row / tiled     ptmi_radiosity_grid's chunk border with 1 and 4 entries left
    68, 196, 1028, 2052 by environment  PTMI_RADIOSITY_ROWS (the lane-per-row kernel's 16-byte path: one odd group; a pair and
                                        an odd group; a vector part that ends on an LDS chunk; one that ends inside a chunk)
                                        and PTMI_RADIOSITY_TILE_ROWS=16, each in a child process

The CPU tests at the top assert on the oracle's own output that no comparison below can pass on an empty sum."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ragged_scenes as rs
from oracle_binding import OracleScene

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("form_factors", "radiosity", "unshot", "grid", "radiosity_grid")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def differing(got, exp):
    """entries whose bits differ, two NaNs counting as equal"""
    got = np.ascontiguousarray(got, F); exp = np.ascontiguousarray(exp, F)
    return (bits(got) != bits(exp)) & ~(np.isnan(got) & np.isnan(exp))


def compare_solution(got, exp, what):
    """tests/test_radiosity_solver.py's compare_solution with the radiosity grid exact; names the first rows that differ"""
    for k in KEYS:
        bad = differing(got[k], exp[k])
        rows = np.unique(np.nonzero(bad)[0])
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} entries, first rows {rows[:8].tolist()} of {got[k].shape[0]}"


def binary64_step(ff, bsdf, Le):
    """One Jacobi step from the documented rule alone (radiosity_iteration_kernel): incident = sum over j != i with
    F_ij > 0 of F_ij * Le_j; reflected = min(Kd * incident, incident); radiosity = Le + reflected; unshot = reflected."""
    Fp = np.where(ff > 0, ff, 0).astype(np.float64)
    np.fill_diagonal(Fp, 0.0)
    inc = Fp @ Le.astype(np.float64)
    refl = np.minimum(bsdf.astype(np.float64) * inc, inc)
    return inc, refl, Le.astype(np.float64) + refl


def assert_within_step_bound(radiosity, unshot, ff, bsdf, Le, what):
    n = ff.shape[0]
    inc, refl, rad = binary64_step(ff, bsdf, Le)
    bound = (n + 2) * 2.0 ** -24 * inc * np.maximum(bsdf.astype(np.float64), 1.0) + 2.0 ** -23 * np.abs(rad)
    for name, got, want in (("radiosity", radiosity, rad), ("unshot", unshot, refl)):
        err = np.abs(got.astype(np.float64) - want)
        worst = np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)
        print(f"{what}: {name} max error {err.max():.3e} ({err.max() / np.abs(want).max():.2e} of the largest value), closest to its bound at "
              f"receiver {worst[0]} channel {worst[1]}: error {err[worst]:.3e}, bound {bound[worst]:.3e}")
        assert (err <= bound).all(), f"{what}: {name} off the binary64 step at receiver {worst[0]} channel {worst[1]}: {err[worst]:.3e} > {bound[worst]:.3e}"
    assert (inc > 0).mean() > 0.5                                        # the sums are not empty


# ------------------------------------------------------------------------------------------------------------------
# CPU: the scenes give the comparisons something to compare
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(rs.CASES) + list(rs.NONFINITE_CASES))
def test_oracle_solution_is_not_trivial(case):
    """positive form factors: at least 5 % of the matrix, in every 256-column tile, in the last row and the last column, in
    the rows of the partial last group of 8; unshot not all zero after the last step.  n = 1 has no pair: its solution is Le."""
    o, sol, _ = rs.oracle_case(case)
    types, _, _, bsdf, Le = rs.case_scene(case)
    ff = sol["form_factors"]; n = ff.shape[0]
    assert n == len(types) and sol["radiosity"].shape == (n, 3)
    assert (np.diag(ff) == 0).all()              # a pair (i, i) is never sampled: the Jacobi kernels' own skip of j == i has nothing to skip
    if n == 1:
        assert (ff == 0).all() and sol["rays"] == 0 and (sol["radiosity"] == Le).all() and (sol["unshot"] == 0).all() and Le.any()
        return
    pos = ff > 0
    assert pos.mean() >= 0.05
    for a in range(0, n, 256):
        assert pos[:, a:a + 256].any(), f"no positive form factor in columns {a}.."
    assert pos[-1].any() and pos[:, -1].any()
    assert n % 8 == 0 or pos[n - n % 8:].any()
    assert (sol["unshot"] != 0).any() and sol["rays"] > 0 and sol["radiosity_grid"].any()
    if case in rs.NONFINITE_CASES:
        # the result holds finite and non-finite values (else the two loops of the tiled kernel could not be told apart); the
        # receiver without red reflectance sees the infinite emitter; the emitter's column holds zeros as well as positive entries
        _, e, _ = rs.NONFINITE_CASES[case]
        _, rcv = rs.nonfinite_scene(n, e)
        rad = sol["radiosity"]
        assert np.isinf(rad).sum() >= 50 and np.isfinite(rad).sum() >= 50
        assert bsdf[rcv, 0] == 0 and ff[rcv, e] > 0 and e % 4 == 3 and rs.tiled(n)
        assert pos[:, e].sum() >= 10 and (~pos[:, e]).sum() >= 10
    else:
        assert np.isfinite(sol["radiosity"]).all()


def test_cases_cover_both_kernels_with_both_primitive_mixes():
    seen = set()
    for case in rs.SIZE_CASES:
        n, quads, prm = rs.CASES[case]
        types = rs.case_scene(case)[0]
        assert len(types) == n and prm["num_iterations"] in (1, 3)
        if n >= 63:
            assert bool(quads) == bool((types == 1).any()) and (types == 0).any()
            seen.add((rs.tiled(n), bool(quads)))
    assert seen == {(True, True), (True, False), (False, True), (False, False)}


@pytest.mark.parametrize("case", ["n1025_step", "n1028_step", "n65"])
def test_binary64_step_agrees_with_the_oracle(case):
    """the restatement and its bound (test_gpu_one_step_against_binary64) hold for the oracle's own step"""
    _, sol, _ = rs.oracle_case(case)
    _, _, _, bsdf, Le = rs.case_scene(case)
    assert_within_step_bound(sol["radiosity"], sol["unshot"], sol["form_factors"], bsdf, Le, case)


@pytest.mark.parametrize("scene", list(rs.FF_SCENES))
def test_oracle_form_factor_kernel_scenes_are_not_trivial(scene):
    """the scenes of test_gpu_every_form_factor_kernel_is_the_oracles: positive form factors in every mode, and a radiosity grid
    that is not all zero where only the Monte-Carlo kernel writes it (num_iterations = 0) - a dropped RAD0 would pass otherwise"""
    assert len(rs.FF_KERNEL_CASES) == len(set(rs.FF_KERNEL_CASES)) == 24
    types = rs.ff_scene(scene)[0]
    assert bool((types == 1).any()) == (scene in ("mixed68", "deep_mixed")) and (types == 0).any()
    for mode in rs.FF_MODES:
        sol = rs.ff_oracle(scene, mode)
        assert (sol["form_factors"] > 0).any() and sol["rays"] > 0, (scene, mode)
    assert rs.ff_oracle(scene, "mc_it0")["radiosity_grid"].any() and rs.ff_oracle(scene, "mc_it0")["grid"].any()


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def R():
    import ptmi
    r = ptmi.Renderer(0)
    yield r
    r.close()


def solve(R, case, **override):
    R.load_scene_arrays(*rs.case_scene(case))
    st = R.run_radiosity_solver(**dict(rs.case_params(case), **override))
    return st, R.radiosity_solution()


@pytest.mark.gpu
@pytest.mark.parametrize("case", rs.SIZE_CASES)
def test_gpu_ragged_size_matches_oracle(R, case):
    n = rs.CASES[case][0]
    st, got = solve(R, case)
    _, exp, cdfs = rs.oracle_case(case)
    compare_solution(got, exp, case)
    assert st.rays == exp["rays"] and st.pairs == n * n
    assert (R.precomputed_cdfs().view(np.uint32) == cdfs.view(np.uint32)).all()
    assert st.walk == (2 if n >= 256 else 0)                            # the certified visibility walk's threshold
    if n == 1:
        assert (got["radiosity"] == rs.case_scene(case)[4]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["n260", "n257"])                      # tiled, lane-per-row
def test_gpu_visibility_walks_agree_at_ragged_sizes(R, case):
    """the reference's walk (0), the automatic choice (-1: certified from 256 up), every blocked ray through the ancestor chain
    (3) and through the reference's walk (4): one solution, the oracle's; the counters as in
    test_radiosity_solver_certified_walk_is_the_references"""
    _, exp, _ = rs.oracle_case(case)
    try:
        R.set_solver_walk(0)
        st0, want = solve(R, case)
        assert st0.walk == 0 and st0.cert_chain == 0 and st0.rays == exp["rays"]
        compare_solution(want, exp, f"{case} walk 0")
        for walk in (-1, 3, 4):
            R.set_solver_walk(walk)
            st = R.run_radiosity_solver(**rs.case_params(case))
            got = R.radiosity_solution()
            print(f"{case} walk {walk}: {st.rays} rays, {st.cert_chain} chains, {st.cert_fallback} fallbacks")
            assert st.walk == 2 and st.rays == st0.rays
            compare_solution(got, want, f"{case} walk {walk}")
            if walk == 3: assert st.cert_chain > 0 and st.cert_fallback == 0
            if walk == 4: assert st.cert_fallback == st.cert_chain > 0
            if walk == -1: assert st.cert_fallback <= st.cert_chain < st.rays // 10
    finally:
        R.set_solver_walk(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("bilateral,ss,sr", [(True, 1.5, 0.3), (False, 0.8, 0.3)])
def test_gpu_grid_filter_at_a_ragged_size(R, bilateral, ss, sr):
    """"Apply Filter & Rebuild CDFs" after a solve of 257 primitives: the filtered pdfs and the rebuilt CDF records"""
    case = "n257"
    solve(R, case)
    o = OracleScene.from_arrays(*rs.case_scene(case))
    o.radiosity_solve(**rs.case_params(case))
    ff, rad = R.apply_grid_filter(bilateral, ss, sr)
    off, orad = o.apply_grid_filter(bilateral, ss, sr)
    assert orad.any() and off.any()
    assert (bits(ff) == bits(off)).all() and (bits(rad) == bits(orad)).all()
    assert (R.precomputed_cdfs().view(np.uint32) == o.cdfs().view(np.uint32)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["n1025_step", "n1028_step"])          # lane-per-row, tiled
def test_gpu_one_step_against_binary64(R, case):
    """One Jacobi step against a numpy binary64 restatement of the documented rule, from the GPU's own form factors - a check
    that shares nothing with the oracle's source.

    The bound.  Every term of a row's sum is non-negative (F_ij > 0, Le >= 0), so no cancellation: a float32 chain of n
    products and n additions carries at most (n + 1) roundings per term, the product Kd * incident one more, each of relative
    size 2^-24: |reflected - exact| <= (n + 2) 2^-24 incident max(Kd, 1) (the min picks either Kd * incident or incident
    itself).  radiosity = Le + reflected adds one rounding of 2^-24 |radiosity|; 2^-23 |radiosity| covers it and the second-order
    terms.  Required per receiver and channel: |gpu - f64| <= (n + 2) 2^-24 incident_f64 max(Kd, 1) + 2^-23 |radiosity_f64|."""
    st, got = solve(R, case)
    _, _, _, bsdf, Le = rs.case_scene(case)
    assert_within_step_bound(got["radiosity"], got["unshot"], got["form_factors"], bsdf, Le, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(rs.NONFINITE_CASES))
def test_gpu_tiled_kernel_nonfinite_unshot(R, case):
    """An emitter with Le = (inf, 0, 3e38) and a receiver whose red Kd is exactly 0: tiles that hold the infinite value take the
    tiled kernel's compare / select loop, the others the multiply-add loop, in one launch.  The expectation is what the oracle's
    plain sequential loop gives, bit for bit (two NaNs count as equal)."""
    n = rs.NONFINITE_CASES[case][0]
    st, got = solve(R, case)
    _, exp, cdfs = rs.oracle_case(case)
    compare_solution(got, exp, case)
    assert st.rays == exp["rays"] and st.pairs == n * n
    assert not differing(R.precomputed_cdfs(), cdfs).any()


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["PTMI_RADIOSITY_ROWS=1", "PTMI_RADIOSITY_TILE_ROWS=16"])
def test_gpu_kernels_selected_by_environment(tmp_path, setting):
    """the lane-per-row kernel at sizes that are multiples of 4 (its 16-byte loads) and the tiled kernel with 16 rows per
    workgroup: read from the environment once per process, so each runs in a child process of its own"""
    env = {k: v for k, v in os.environ.items() if k not in ("PTMI_RADIOSITY_ROWS", "PTMI_RADIOSITY_TILE_ROWS")}
    name, value = setting.split("=")
    env[name] = value
    subprocess.run([sys.executable, os.path.join(HERE, "radiosity_env_worker.py"), str(tmp_path)], env=env, check=True, timeout=120)
    for case in rs.ENV_CASES:
        got = np.load(tmp_path / (case + ".npz"))
        _, exp, cdfs = rs.oracle_case(case)
        compare_solution(got, exp, f"{setting} {case}")
        assert int(got["rays"]) == exp["rays"] and int(got["pairs"]) == rs.CASES[case][0] ** 2
        assert (got["cdfs"].view(np.uint32) == cdfs.view(np.uint32)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("scene,walk,mode", rs.FF_KERNEL_CASES)
def test_gpu_every_form_factor_kernel_is_the_oracles(R, scene, walk, mode):
    """launch_form_factors turns (Monte-Carlo, quads, deep tree, num_iterations == 0, walk) into one of 24 instantiations of
    ptmi_form_factors; the other tests launch a few of them.  Each once, at the smallest scenes that reach it: the reference's
    walk (0), the opt-in fast tree (1: fast_tree) and the certified walk (2: asked for by name from 65 primitives up) on 68
    triangles and on 68 mixed primitives; a tree deeper than 31 levels, where every request ends at walk 0.  Everything is the
    oracle's bit for bit, except the radiosity grid of num_iterations = 0, which the reference itself sums with unordered
    float atomics: 2e-5 relative, as in test_gpu_solver_zero_iterations."""
    exp = rs.ff_oracle(scene, mode)
    deep = scene.startswith("deep")
    try:
        R.load_scene_arrays(*rs.ff_scene(scene))
        assert (R.scene_info()["bvh_depth"] > 31) == deep
        if walk == 1: R.set_config(fast_tree=True)
        if walk == 2 or deep: R.set_solver_walk(2, 65 if not deep else 1)
        st = R.run_radiosity_solver(**rs.FF_MODES[mode])
        got = R.radiosity_solution()
    finally:
        R.set_solver_walk(-1)
        R.set_config(fast_tree=False)
    what = f"{scene} walk {walk} {mode}"
    assert st.walk == walk, what
    for k in ("form_factors", "radiosity", "unshot", "grid"):
        bad = differing(got[k], exp[k])
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} entries"
    assert st.rays == exp["rays"], what
    if mode == "mc_it0":
        err = np.abs(got["radiosity_grid"].astype(np.float64) - exp["radiosity_grid"])
        print(f"{what}: radiosity grid max error {err.max():.3e}, largest value {np.abs(exp['radiosity_grid']).max():.3e}")
        assert np.allclose(got["radiosity_grid"], exp["radiosity_grid"], rtol=2e-5, atol=1e-7), what
    else:
        assert not differing(got["radiosity_grid"], exp["radiosity_grid"]).any(), f"{what}: radiosity_grid"
