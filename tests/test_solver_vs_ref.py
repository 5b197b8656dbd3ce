"""oracle/ptmi_oracle.c against the REFERENCE's own radiosity pre-pass - rendering/form_factors.h and rendering/grid_filter.h
compiled into oracle/_ref/libptmi_ref_solver.so (oracle/ref_solver_harness.cpp, only where the reference tree exists).  Bit-exact.

Per call: direction_to_grid_indices_local, visibility_test_anyhit (over the reference's BVHBuilder tree, and through its own
linear search), formfactor_rand_init, one Monte-Carlo pair on scripted raw words.  Per stage: rows of both form-factor
kernels (F, count grid), update_radiosity_grid, radiosity_iteration_kernel, the three filter wrappers of grid_filter.h run as
written, subdivide_primitives.  Whole solves: the launch sequence of RadiosityState::runSolver (restated in the harness, the
only restated code) around the reference's kernels, with 0, 1 and 3 iterations, unfiltered, bilateral and Gaussian.

Where the reference is not a function of its inputs the harness fixes the rules the oracle documents (the Jacobi step reads
the state before the launch; a receiver's pairs add to its radiosity grid in ascending j): agreement there pins the arithmetic,
not the rule.  The cases are in tests/solver_ref_sets.py.

Every answer of the compiled reference is recorded in tests/golden/ref_solver.npz, bulky ones as a hash and their first rows.
Where oracle/_ref is built the tests ask it live and also require the recorded bits; everywhere else they compare the oracle
with the record.  No case is skipped.
Re-record (where oracle/_ref is built):  python tests/golden/make_golden.py --ref-only
"""
import ctypes as C
import os

import numpy as np
import pytest

import solver_ref_sets as S
from oracle_binding import (OracleScene, SCENES, oracle_filter_pdfs, oracle_lib, oracle_radiosity_grid, recorded_reference, ref_sol_available,
                            sha)

F = np.float32
U32 = np.uint32


@pytest.fixture(scope="module")
def ref():
    yield from recorded_reference(S.GOLDEN, ref_sol_available())


def bits(a):
    return np.ascontiguousarray(a, F).view(U32)


def same_bits(a, b):
    a, b = bits(a), bits(np.asarray(b))
    return a.shape == b.shape and np.array_equal(a, b)


def recorded_for(ref, key, ask, in_sha):
    """ref(key, ...); the record must have been made from exactly these inputs (else the cases changed: re-record)"""
    r = ref(key, lambda: dict(ask(), in_sha=in_sha))
    assert np.array_equal(np.asarray(r["in_sha"]), in_sha), f"{key}: the case's inputs differ from the recorded ones - re-record"
    return r


def sub(r, name):
    """the bulky answer `name` of record r: dict(sha, head)"""
    return dict(sha=r[name + "_sha"][0], sha_nan=r[name + "_sha"][1], head=r[name + "_head"])


def put(d, name, a, rows=4):
    b = S.bulky(a, rows)
    d[name + "_sha"] = np.stack([b["sha"], b["sha_nan"]]); d[name + "_head"] = b["head"]      # exact bits; NaNs made one NaN
    return d


def ref_scene(name_or_arrays):
    from oracle_binding import RefSolverScene
    arrs = S.scene_arrays(name_or_arrays) if isinstance(name_or_arrays, str) else name_or_arrays
    return RefSolverScene(*arrs)


def oracle_scene(name_or_arrays):
    arrs = S.scene_arrays(name_or_arrays) if isinstance(name_or_arrays, str) else name_or_arrays
    return OracleScene.from_arrays(*arrs)


def centroids(o):
    return np.array([o.prim_geometry(i)[1] for i in range(o.n_prims)], F)


def _p(a):
    return a.ctypes.data


# ---- grid index and visibility --------------------------------------------------------------------------------------------------
def ref_grid_index(ref):
    from oracle_binding import ref_sol_grid_index
    dirs, nrms = S.grid_index_cases()
    return recorded_for(ref, "grid_index", lambda: dict(index=ref_sol_grid_index(dirs, nrms)), S.inputs_sha(dirs, nrms))


def test_grid_index_vs_ref(ref):
    dirs, nrms = S.grid_index_cases()
    r = ref_grid_index(ref)
    L = oracle_lib()
    got = np.array([L.po_direction_to_grid_index(_p(np.ascontiguousarray(d)), _p(np.ascontiguousarray(n))) for d, n in zip(dirs, nrms)], np.int32)
    bad = np.flatnonzero(got != r["index"])
    assert len(bad) == 0, (len(bad), dirs[bad[:3]], nrms[bad[:3]], got[bad[:3]], r["index"][bad[:3]])


def ref_anyhit(ref):
    rays = S.anyhit_rays()

    def ask():
        return dict(blocked=np.array([ref_scene(arrs).visibility(o, d, md, 0, 1)[0] for _, _, arrs, o, d, md, _ in rays], np.int32))
    return recorded_for(ref, "visibility/anyhit_edges", ask, S.inputs_sha(*[a for c in rays for a in (c[2][1], c[3], c[4], np.asarray(c[5], F))]))


def test_visibility_edges_vs_ref(ref):
    """tests/anyhit_edge_sets.py's families, one blocker on one edge of the question: the reference's verdict is the one the
    family states, and the oracle's is the reference's."""
    rays = S.anyhit_rays()
    r = ref_anyhit(ref)
    for k, (case, member, arrs, o, d, md, want) in enumerate(rays):
        sc = oracle_scene(arrs)                          # held: the handle dies with the object
        got = oracle_lib().po_visibility_blocked(sc.h, _p(o), _p(d), F(md), 0, 1)
        assert got == r["blocked"][k] == int(want), (case, member, got, r["blocked"][k], want)


def ref_chain(ref, name):
    arrs = S.scene_arrays(name)
    O, D, M, src, tgt = S.chain_rays(arrs, centroids(oracle_scene(name)))

    def ask():
        rs = ref_scene(name)
        return dict(blocked=rs.visibility(O, D, M, src, tgt), blocked_linear=rs.visibility(O, D, M, src, tgt, use_bvh=False))
    return (O, D, M, src, tgt), recorded_for(ref, f"visibility/{name}", ask, S.inputs_sha(S.scene_sha(name), O, D, M, src, tgt))


@pytest.mark.parametrize("name", S.CHAINS)
def test_visibility_deep_chain_vs_ref(name, ref):
    """A tree deeper than 31 levels: from 30 stack entries on the reference drops children, blockers under them included - in
    the mirrored chains, where the stack grows by one entry per level (tests/solver_ref_sets.py: scene_arrays)."""
    (O, D, M, src, tgt), r = ref_chain(ref, name)
    o = oracle_scene(name); L = oracle_lib()
    got = np.array([L.po_visibility_blocked(o.h, _p(O[k]), _p(D[k]), M[k], int(src[k]), int(tgt[k])) for k in range(len(O))], np.int32)
    bad = np.flatnonzero(got != r["blocked"])
    assert len(bad) == 0, (len(bad), src[bad[:5]], tgt[bad[:5]])


def test_rand_init_vs_ref(ref):
    """formfactor_rand_init: curand_init(12345 + idx, idx, 0) - seed and subsequence both move with the pair's index"""
    from oracle_binding import ref_sol_rand_init
    idx = np.array([0, 1, 2, 63, 64, 255, 256, 4224, 66048], np.int32)          # 66048 = 257 * 257 - 1
    r = recorded_for(ref, "rand_init", lambda: dict(state=ref_sol_rand_init(257 * 257, idx)), S.inputs_sha(idx))
    for k, i in enumerate(idx):
        st = np.zeros(6, U32)                            # a typed pointer: accepted whichever argtypes another module has set
        oracle_lib().po_rng_init(12345 + int(i), int(i), st.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert np.array_equal(st, r["state"][k]), i


# ---- scripted pairs --------------------------------------------------------------------------------------------------------------
def ref_scripted(ref):
    cases = S.scripted_cases()

    def ask():
        rs = ref_scene("scripted")
        res = [rs.mc_pair_words(i, j, ns, words) for _, i, j, ns, words in cases]
        return {k: np.array([c[k] for c in res]) for k in ("F", "grid", "rad_grid", "used", "overrun")}      # one row per case
    sh = S.inputs_sha(S.scene_sha("scripted"), *[np.array([i, j, ns] + list(w), np.int64) for _, i, j, ns, w in cases])
    return recorded_for(ref, "scripted", ask, sh)


def test_scripted_pairs_vs_ref(ref):
    r = ref_scripted(ref)
    o = oracle_scene("scripted")
    for c, (label, i, j, ns, words) in enumerate(S.scripted_cases()):
        got = o.mc_pair_words(i, j, ns, words)
        assert got["used"] == r["used"][c] and got["overrun"] == r["overrun"][c], (label, got["used"], r["used"][c], got["overrun"], r["overrun"][c])
        for k in ("F", "grid", "rad_grid"):
            assert same_bits(got[k], r[k][c]), (label, k, got[k][np.nonzero(got[k])] if k != "F" else got[k], r[k][c].sum())


def ref_tiers(ref):
    """every ordered pair of the Cornell box through the scripted entry at 8 samples: the words each pair draws say which tier
    it took (0: returned before sampling, 8 = 4 * max(1, 8 / 4), 16 = 4 * max(2, 8 / 2), 32 = 4 * 8)"""
    n = len(S.scene_arrays("cbox")[0])
    words = np.random.default_rng(8).integers(0, 2 ** 32, 32).astype(U32)

    def ask():
        rs = ref_scene("cbox")
        res = [[rs.mc_pair_words(i, j, 8, words) for j in range(n)] for i in range(n)]
        return dict(used=np.array([[int(c["used"]) for c in row] for row in res], np.int32), F=np.array([[c["F"] for c in row] for row in res], F),
                    counts=np.array([[c["grid"].sum() for c in row] for row in res], F))
    return words, recorded_for(ref, "tiers/cbox", ask, S.inputs_sha(S.scene_sha("cbox"), words))


def test_sample_tiers_vs_ref(ref):
    words, r = ref_tiers(ref)
    o = oracle_scene("cbox"); n = o.n_prims
    for i in range(n):
        for j in range(n):
            got = o.mc_pair_words(i, j, 8, words)
            assert int(got["used"]) == r["used"][i, j] and same_bits(got["F"], r["F"][i, j]) and float(got["grid"].sum()) == r["counts"][i, j], (i, j)


# ---- form-factor rows -----------------------------------------------------------------------------------------------------------
def ref_ff_rows(ref, case):
    scene, mc, m = case
    rows = S.ff_rows(scene)

    def ask():
        ff, grid, rad_grid = ref_scene(scene).ff_rows(rows, use_monte_carlo=bool(mc), mc_samples=m)
        return put(put(put(dict(), "ff", ff), "grid", grid), "rad_grid", rad_grid)
    return rows, recorded_for(ref, S.ff_key(case), ask, S.inputs_sha(S.scene_sha(scene), rows))


@pytest.mark.parametrize("case", S.FF_ROW_CASES, ids=S.ff_key)
def test_form_factor_rows_vs_ref(case, ref):
    scene, mc, m = case
    rows, r = ref_ff_rows(ref, case)
    ff, grid = oracle_scene(scene).form_factor_rows(rows, use_monte_carlo=bool(mc), mc_samples=m)
    assert S.same_bulky(ff, sub(r, "ff")), ("form factors", np.argwhere(bits(ff[:4]) != bits(r["ff_head"]))[:5])
    assert S.same_bulky(grid, sub(r, "grid")), "count grid"


# ---- stages ------------------------------------------------------------------------------------------------------------------------
STAGE_SCENES = ("cbox_quads", "soup65")


def stage_inputs(name):
    """random form factors (a fifth of them zero, some negative) and radiosity for the stage entries"""
    n = len(S.scene_arrays(name)[0])
    rng = np.random.default_rng(n)
    ff = (rng.uniform(-0.02, 0.2, (n, n)) * (rng.random((n, n)) < 0.8)).astype(F)
    return ff, rng.uniform(0, 3, (n, 3)).astype(F), rng.uniform(0, 2, (n, 3)).astype(F)


@pytest.mark.parametrize("name", STAGE_SCENES)
def test_update_radiosity_grid_on_scenes_vs_ref(name, ref):
    """update_radiosity_grid over real primitives (centroids and normals as the kernel takes them), then the two rgb filter
    wrappers on its result"""
    from oracle_binding import ref_sol_filter_grids
    ff, rad, _ = stage_inputs(name)

    def ask():
        g = ref_scene(name).update_grid(ff, rad)
        out = put(dict(), "plain", g)
        put(out, "bilateral", ref_sol_filter_grids(g, True, 1.5, 0.3)); put(out, "gaussian", ref_sol_filter_grids(g, False, 0.7, 0.3))
        return out
    r = recorded_for(ref, f"update_grid/{name}", ask, S.inputs_sha(S.scene_sha(name), ff, rad))
    o = oracle_scene(name); arrs = S.scene_arrays(name)
    c = centroids(o)
    assert S.same_bulky(oracle_radiosity_grid(c, arrs[2], ff, rad), sub(r, "plain"))
    assert S.same_bulky(oracle_radiosity_grid(c, arrs[2], ff, rad, True, True, 1.5, 0.3), sub(r, "bilateral"))
    assert S.same_bulky(oracle_radiosity_grid(c, arrs[2], ff, rad, True, False, 0.7, 0.3), sub(r, "gaussian"))


def ref_world(ref, w):
    def ask():
        from oracle_binding import ref_sol_filter_grids
        g = ref_scene(S.world_as_scene(w)).update_grid(w["ff"], w["rad"])
        if w["filtering"] is not None:
            bil, ss, sr = w["filtering"]
            g = ref_sol_filter_grids(g, bool(bil), float(ss), float(sr))
        return put(dict(), "grid", g, rows=2)
    return recorded_for(ref, f"world/{w['label']}", ask, S.inputs_sha(w["centre"], w["normal"], w["ff"], w["rad"]))


def test_update_radiosity_grid_on_worlds_vs_ref(ref):
    """tests/guided_record_sets.py's constructed worlds (every kind of form factor, coinciding centres and centres 1e-6f apart,
    a source in every cell, sums whose order matters, NaN under the filters)"""
    for w in S.grid_worlds():
        r = ref_world(ref, w)
        kw = {}
        if w["filtering"] is not None:
            bil, ss, sr = w["filtering"]
            kw = dict(enable_filtering=True, use_bilateral=bool(bil), sigma_spatial=float(ss), sigma_range=float(sr))
        got = oracle_radiosity_grid(w["centre"], w["normal"], w["ff"], w["rad"], **kw)
        assert S.same_bulky(got, sub(r, "grid")), w["label"]


@pytest.mark.parametrize("name", STAGE_SCENES)
def test_radiosity_iteration_vs_ref(name, ref):
    """radiosity_iteration_kernel, one launch from a given state.  The oracle has no entry for one step from a given state; its
    steps are compared through the whole solves below.  Here the reference's step is held to the formula's plain restatement in
    float32 (F_ij > 0 only, ascending j, min(Kd * E, E) per channel), so that the record of the step is itself checked."""
    ff, rad, unshot = stage_inputs(name)
    r = recorded_for(ref, f"iterate/{name}", lambda: dict(zip(("radiosity", "unshot"), ref_scene(name).iterate(ff, rad, unshot))),
                     S.inputs_sha(S.scene_sha(name), ff, rad, unshot))
    bsdf = S.scene_arrays(name)[3]
    n = len(ff)
    for i in range(n):
        e = np.zeros(3, F)
        for j in range(n):
            if i != j and ff[i, j] > 0:
                e = (e + unshot[j] * ff[i, j]).astype(F)
        refl = np.minimum((bsdf[i] * e).astype(F), e)
        assert same_bits(refl, r["unshot"][i]) and same_bits((rad[i] + refl).astype(F), r["radiosity"][i]), i


# ---- whole solves ----------------------------------------------------------------------------------------------------------------
def ref_solve(ref, case):
    scene = case[0]

    def ask():
        sol = ref_scene(scene).solve(**S.solve_params(case))
        out = dict(radiosity=sol["radiosity"], unshot=sol["unshot"])
        for k, rows in (("form_factors", 4), ("grid", 4), ("radiosity_grid", 4)):
            put(out, k, sol[k], rows)
        return out
    return recorded_for(ref, S.solve_key(case), ask, S.scene_sha(scene))


@pytest.mark.parametrize("case", S.SOLVE_CASES, ids=S.solve_key)
def test_whole_solve_vs_ref(case, ref):
    r = ref_solve(ref, case)
    sol = oracle_scene(case[0]).radiosity_solve(**S.solve_params(case))
    for k in ("radiosity", "unshot"):
        assert same_bits(sol[k], r[k]), (k, np.argwhere(bits(sol[k]) != bits(r[k]))[:5])
    for k in ("form_factors", "grid", "radiosity_grid"):
        assert S.same_bulky(sol[k], sub(r, k)), k


# ---- "Apply Filter & Rebuild CDFs" -------------------------------------------------------------------------------------------------
def filter_group_key(ss, sr, bil, with_counts):
    return f"filter_pdfs/{ss!r}/{sr!r}/{'bilateral' if bil else 'gaussian'}/{'counts' if with_counts else 'no_counts'}"


def ref_filter_group(ref, ss, sr, idx, bil, with_counts):
    from oracle_binding import ref_sol_filter_pdfs
    cases = S.filter_cases()
    rgb = np.array([cases[k]["rgb"] for k in idx], F); counts = np.array([cases[k]["counts"] for k in idx], F) if with_counts else None

    def ask():
        ff, rad = ref_sol_filter_pdfs(rgb, counts, bil, ss, sr)
        return put(put(dict(), "formfactor", ff, rows=4), "radiosity", rad, rows=4)
    return rgb, counts, recorded_for(ref, filter_group_key(ss, sr, bil, with_counts), ask, S.inputs_sha(rgb, counts if with_counts else np.zeros(0, F)))


@pytest.mark.parametrize("bil", [1, 0], ids=["bilateral", "gaussian"])
@pytest.mark.parametrize("with_counts", [1, 0], ids=["counts", "no_counts"])
def test_filter_pdfs_vs_ref(bil, with_counts, ref):
    """filter_pdfs_for_primitives as written - copy, luminance, filter, memcpy back, normalise - on one-hot, all-zero and
    huge-range grids and on the constructed grids of tests/guided_record_sets.py, one wrapper call per pair of sigmas"""
    for (ss, sr), idx in S.filter_groups().items():
        rgb, counts, r = ref_filter_group(ref, ss, sr, idx, bil, with_counts)
        ff, rad = oracle_filter_pdfs(rgb, counts, bil, ss, sr)
        labels = [S.filter_cases()[k]["label"] for k in idx]
        assert S.same_bulky(ff, sub(r, "formfactor")), (ss, sr, labels)
        assert S.same_bulky(rad, sub(r, "radiosity")), (ss, sr, labels)


# ---- subdivide_primitives ------------------------------------------------------------------------------------------------------------
def ref_subdivide(ref, case):
    scene, level = case
    path = os.path.join(SCENES, scene + ".obj")
    p = OracleScene.load(path).prims()                   # level 0 of the oracle's loader is the reference's loadOBJ (test_host_logic.py)
    base = (p["type"], p["verts"], p["normal"], p["bsdf"], p["Le"])

    def ask():
        q = ref_scene(base).subdivide(level).prims()
        return {k: q[k] for k in ("type", "verts", "normal", "bsdf", "Le")}
    return recorded_for(ref, f"subdivide/{scene}/{level}", ask, S.inputs_sha(np.asarray(base[0], np.int32), *base[1:]))


def assert_same_prims(got, r, what):
    assert np.array_equal(got["type"], r["type"]), what
    tri = got["type"] == 0
    assert same_bits(got["verts"][tri][:, :3], r["verts"][tri][:, :3]) and same_bits(got["verts"][~tri], r["verts"][~tri]), (what, "verts")
    for k in ("normal", "bsdf", "Le"):
        assert same_bits(got[k], r[k]), (what, k)


@pytest.mark.parametrize("case", S.SUBDIVIDE_CASES, ids=lambda c: f"{c[0]}_{c[1]}")
def test_subdivide_vs_ref(case, ref):
    """subdivide_primitives, levels 0 to 2, on triangles, quads and a mix: vertices, normals, bsdf and Le in order, for the
    oracle's loader and for the product's (ptmi_host_scene_load)"""
    import ptmi
    scene, level = case
    r = ref_subdivide(ref, case)
    path = os.path.join(SCENES, scene + ".obj")
    assert_same_prims(OracleScene.load(path, subdivision=level).prims(), r, "oracle")
    assert_same_prims(ptmi.HostScene.load(path, level, False).prims(), r, "product")


# ---- the cases are what they claim ---------------------------------------------------------------------------------------------------
def test_the_cases_are_what_they_claim(ref):
    """On the REFERENCE's own answers: every branch the cases name is taken."""
    # grid index: every one of the 256 cells is answered
    assert set(np.unique(ref_grid_index(ref)["index"])) == set(range(256))
    # visibility: blocked and open rays, on the edge families and on the chains
    b = ref_anyhit(ref)["blocked"]
    assert 0 < b.sum() < len(b)
    for name in S.CHAINS:
        (_, _, M, _, _), r = ref_chain(ref, name)
        assert 0 < r["blocked"].sum() < len(r["blocked"])
        aimed, aimed_linear = r["blocked"][-60:], r["blocked_linear"][-60:]
        assert aimed_linear[:49].all() and 0 < aimed.sum() < 49, aimed             # each aimed ray has its blocker; the walk loses some
        # The drop rule is live in the reference itself: its own linear search, which drops nothing, finds blockers that its
        # tree walk never reaches, and never the other way round.  Rays no longer than 1e5 only: beyond 4e5 the walk also loses
        # boxes to the slope 1e8 of a zero direction component.
        short = M < 1e5
        lost = (r["blocked_linear"] == 1) & (r["blocked"] == 0) & short
        assert not ((r["blocked"] == 1) & (r["blocked_linear"] == 0)).any()
        assert (lost.sum() >= 1) == name.endswith("_mirror"), (name, lost.sum())
    # the sample tiers: culled pairs draw nothing, and each of the three tiers is taken by some pair of the Cornell box
    _, t = ref_tiers(ref)
    assert set(np.unique(t["used"])) == {0, 8, 16, 32}, np.unique(t["used"])
    off = ~np.eye(len(t["used"]), dtype=bool)
    assert (t["used"][off] == 0).any() and (t["used"][off] > 0).any()
    assert ((t["used"] > 0) & (t["counts"] * 4 < t["used"])).any()                 # some samples are rejected or blocked
    # scripted pairs
    s = ref_scripted(ref)
    at = {c[0]: k for k, c in enumerate(S.scripted_cases())}
    g = lambda label, k: np.asarray(s[k][at[label]])
    assert g("coincide", "used") == 4 and g("coincide", "grid").sum() == 0 and g("coincide", "F") == 0      # p_i on p_j: r < 1e-6
    assert g("coincide_then_live", "grid").sum() >= 1 and g("coincide_then_live", "F") > 0                   # ... and the loop goes on
    assert g("overrun", "overrun") == 1 and g("coincide", "overrun") == 0
    assert g("cos_negative", "grid").sum() == 0 and g("cos_live", "grid").sum() == 1                         # nothing can block in that group
    assert g("cos_negative_then_live", "grid").sum() == 1 and 0 < g("cos_negative_then_live", "F") < g("cos_live", "F")   # visibility 1 / 2
    for label in ("blocked_1", "blocked_8", "blocked_back"):
        assert g(label, "used") > 0 and g(label, "grid").sum() == 0 and g(label, "F") == 0                    # valid_samples == 0
    assert g("clamped", "F") == 1 and g("clamped_8", "F") == 1 and 0 < g("unclamped_back", "F") < 1
    assert g("window", "grid").sum() == 1 and g("window_8", "grid").sum() == 8 and g("window_back", "grid").sum() == 8   # open, all of them
    assert g("self", "used") == 0 and g("other_group", "used") == 4 * 16                                      # i == j; the far tier of 64
    # form-factor rows: the coincident centroids give 0 both ways although the ceiling sees both; the floor lies behind both (back-facing)
    rows, r = ref_ff_rows(ref, ("coincident", 1, 8))
    ff = np.asarray(r["ff_head"])
    assert ff[0, 1] == 0 and ff[1, 0] == 0 and ff[0, 2] > 0 and ff[1, 2] > 0 and ff[2, 0] > 0 and (ff[3, :2] == 0).all() and (ff[:2, 3] == 0).all()
    # the filters change cells: the rgb wrappers on a scene's grids, the float wrappers on a one-hot grid
    (ss, sr), idx = next(iter(S.filter_groups().items()))
    assert [S.filter_cases()[k]["label"] for k in idx[:4]] == ["one_hot", "all_zero", "huge_range", "random"]
    plain = S.filter_cases()[idx[3]]["counts"].astype(np.float64); plain /= plain.sum()
    for bil in (1, 0):
        _, _, r = ref_filter_group(ref, ss, sr, idx, bil, 1)
        for k in ("formfactor_head", "radiosity_head"):
            head = np.asarray(r[k])
            # a lone cell spreads over its 5 x 5 taps - except the count of 7 under the bilateral filter, whose range weight
            # exp(-7 * 7 / 0.18) is 0 in float32 (the luminance of 1.9 still leaves exp(-19)); all-zero stays all-zero
            alone = bil and k == "formfactor_head"
            assert (head[0] > 0).sum() == (1 if alone else 25) and not head[1].any(), (bil, k, (head[0] > 0).sum())
        assert not np.allclose(np.asarray(r["formfactor_head"])[3], plain, rtol=1e-3, atol=0), bil      # the random counts are changed by both
    for case in S.SOLVE_CASES:
        if case[1] > 0 and case[3] == 1 and case[2] != "off":
            plain = ref_solve(ref, (case[0], case[1], "off", 1))
            assert not np.array_equal(ref_solve(ref, case)["radiosity_grid_sha"][0], plain["radiosity_grid_sha"][0]), case
            assert np.array_equal(ref_solve(ref, case)["form_factors_sha"][0], plain["form_factors_sha"][0]), case
    # num_iterations == 0 keeps the Monte-Carlo kernel's own radiosity grid: not all zero, and not the grid of one iteration
    nf = ref_solve(ref, ("nf65", 1, "off", 1))
    assert np.isinf(nf["radiosity"][0, 0]) and np.isfinite(nf["radiosity"][:, 0]).sum() > 32 and np.isinf(nf["radiosity"][1:, 0]).any()
    for scene in ("cbox", "soup65"):
        r0, r1 = ref_solve(ref, (scene, 0, "off", 1)), ref_solve(ref, (scene, 1, "off", 1))
        empty = sha(np.zeros((len(S.scene_arrays(scene)[0]), 256, 3), F))
        assert not np.array_equal(r0["radiosity_grid_sha"][0], empty) and not np.array_equal(r0["radiosity_grid_sha"][0], r1["radiosity_grid_sha"][0])
        assert same_bits(r0["radiosity"], S.scene_arrays(scene)[4]) and not same_bits(r1["radiosity"], r0["radiosity"])
    # subdivision quadruples the count per level
    for scene in ("cbox", "cbox_quads", "mixed"):
        n0 = len(ref_subdivide(ref, (scene, 0))["type"])
        assert [len(ref_subdivide(ref, (scene, lv))["type"]) for lv in (1, 2)] == [4 * n0, 16 * n0]
    t = ref_subdivide(ref, ("mixed", 1))["type"]
    assert (t == 0).any() and (t == 1).any()
