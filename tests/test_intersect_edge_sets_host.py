"""The edge sets of the closest-hit tests (tests/intersect_edge_sets.py), proven on the CPU - no GPU.

For every label the float32 restatement of the reference's formulas confirms that, per primitive kind, at least one ray sits exactly
on the edge with its neighbours on either side, and that the two sides get different verdicts where the reference's contract says
so.  Then the restatement against the oracle (the verdict on the primitive a ray is aimed at IS the scene's answer), the oracle's
tree against its linear pass (they differ only where a label says that the tree matters, and there by visiting order), and the
oracle against the compiled reference on every ray of every set: hit, primitive and the bits of t.  The reference's answers are
recorded in tests/golden/ref_intersect_edges.npz as those of tests/test_oracle_vs_ref.py are (live where oracle/_ref is built,
and then equal to the record; re-record with tests/golden/make_golden.py --ref-only).
"""
import os

import numpy as np
import pytest

import intersect_edge_sets as S
import ptmi
from intersect_edge_sets import F, TRI, QUAD, EPS, EPS_UP, EPS_DN, up, dn
from oracle_binding import OracleScene, RefScene, recorded_reference, ref_available

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_intersect_edges.npz")
KIND_NAMES = {"tri": ("tri",), "quad": ("quad",), "mixed": ("tri", "quad")}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(x, y):
    """the same float32 value (a zero of either sign is zero)"""
    return bool(F(x) == F(y))


@pytest.fixture(scope="module")
def ref():
    yield from recorded_reference(GOLDEN, ref_available())


def verdicts(s, idx):
    return [s.verdict(i) for i in idx]


def one(s, *parts):
    idx = s.where(*parts)
    assert len(idx) == 1, (s.name, s.kind, parts, len(idx))
    return idx[0]


# ------------------------------------------------------------------------------------------------
# the sets themselves
# ------------------------------------------------------------------------------------------------
def test_sets_are_deterministic_and_small():
    for name, kind in S.all_sets():
        a, b = S.BUILDERS[name](kind), S.BUILDERS[name](kind)
        assert 0 < len(a) <= 4000 and len(a.types) >= 9, (name, kind)           # at least three leaves of at most four
        assert a.label == b.label and len(set(a.label)) == len(a.label), (name, kind)
        for x, y in zip(a.scene + (a.o, a.d, a.t_min, a.t_max), b.scene + (b.o, b.d, b.t_min, b.t_max)):
            assert x.tobytes() == y.tobytes(), (name, kind)
        want = {"tri": {TRI}, "quad": {QUAD}, "mixed": {TRI, QUAD}}[kind]
        assert set(a.types.tolist()) == want, (name, kind)
        assert S.oracle_scene(name, kind).n_nodes >= 5, (name, kind)


@pytest.mark.parametrize("kind", S.KINDS)
def test_barycentric_edges_are_there(kind):
    s = S.edge_set("barycentric", kind)
    zero, one_ = F(0), F(1)
    for name in KIND_NAMES[kind]:
        full = kind != "mixed" or name == "tri"           # the stacked target of the mixed scene steps in x only
        for way in ("up", "down", "oblique"):
            centre = s.where(name, "bary", "dx+0dy+0", way)
            points = S.TRI_POINTS if name == "tri" else S.QUAD_POINTS
            assert len(centre) == len(points)             # "dropping one vertex set" fails here
            for i in centre:                              # the point itself - vertex, edge, diagonal, interior - is hit, at t = 1
                ok, t, _ = s.verdict(i)
                assert ok and same(t, 1.0), s.label[i]
        rows = [(i, s.terms(i, 0), s.terms(i, 1) if name == "quad" else None, s.verdict(i)) for i in s.where(name, "bary", "up")]
        def seen(pred):
            return [r for r in rows if pred(r)]
        if name == "tri":
            # u: exactly 0 and 1 accepted, one float outside rejected at the u stage, one float inside accepted
            assert seen(lambda r: same(r[1][1], 0.0) and r[3][0]) and seen(lambda r: same(r[1][1], dn(zero)) and r[3][2] == "u")
            assert seen(lambda r: same(r[1][1], up(zero)) and r[3][0])
            assert seen(lambda r: same(r[1][1], 1.0) and r[3][0]) and seen(lambda r: same(r[1][1], up(one_)) and r[3][2] == "u")
            assert seen(lambda r: same(r[1][1], dn(one_)) and same(r[1][2], 0.0) and r[3][0])
            # v: exactly 0 accepted, one float below rejected at the v stage
            assert seen(lambda r: same(r[1][2], 0.0) and r[3][0]) and seen(lambda r: same(r[1][2], dn(zero)) and r[3][2] == "v" and r[1][1] > 0)
            # u + v: exactly 1 accepted; one float of a coordinate above ROUNDS to 1 and is accepted; the next float of the sum is rejected
            assert seen(lambda r: same(r[1][1] + r[1][2], 1.0) and r[1][1] > 0 and r[1][2] > 0 and r[3][0])
            assert seen(lambda r: same(r[1][1], up(F(0.25))) and same(r[1][2], 0.75) and r[3][0])
            assert seen(lambda r: same(r[1][1] + r[1][2], up(one_)) and r[1][1] > 0 and r[1][2] > 0 and r[3][2] == "v")
            assert seen(lambda r: same(r[1][1] + r[1][2], dn(one_)) and r[3][0])
        else:
            # on the diagonal both halves accept, with equal t: (u, v) = (0, y) in the first, (x, 0) in the second
            both = seen(lambda r: same(r[1][1], 0.0) and same(r[2][2], 0.0) and r[1][2] > 0 and same(r[1][3], r[2][3]) and r[3][0])
            assert len(both) >= 3
            # one float off the diagonal only one half accepts: the quad form's u >= 0 / v >= 0, one float below zero
            assert seen(lambda r: same(r[1][1], up(zero)) and r[2][2] < 0 and r[3][0]) or not full
            assert seen(lambda r: float(r[1][1]) in (-2.0 ** -26, -2.0 ** -25, -2.0 ** -24) and same(r[2][2], -r[1][1]) and r[3][0])   # u = x - y, one float
            # the outer edges: u + v == 1 in the first half (x == 1), u == 1 and one float beyond
            assert seen(lambda r: same(r[1][1] + r[1][2], 1.0) and r[1][2] > 0 and r[3][0])
            assert seen(lambda r: r[1][1] + r[1][2] > 1 and r[2][1] > 1 and not r[3][0])
            assert seen(lambda r: same(r[1][1], 1.0) and same(r[1][2], 0.0) and r[3][0])
            assert seen(lambda r: same(r[2][2], 1.0) and same(r[2][1], 0.0) and r[3][0]) or not full
            assert seen(lambda r: same(r[2][1], dn(zero)) and not r[3][0])


@pytest.mark.parametrize("kind", S.KINDS)
def test_determinant_edge_tells_the_triangle_from_the_quad(kind):
    s = S.edge_set("determinant", kind)
    ans = S.oracle_answers("determinant", kind)
    for name in KIND_NAMES[kind]:
        for sign in ("pos", "neg"):
            for way in ("up", "down"):
                got = {}
                for where, mag in (("below", EPS_DN), ("at", EPS), ("above", EPS_UP), ("twice", F(2) * EPS)):
                    i = one(s, name, "det", where, sign, way)
                    a = s.terms(i)[0]
                    assert same(abs(a), mag) and (a < 0) == ((sign == "pos") == (way == "up")), s.label[i]
                    got[where] = (bool(s.verdict(i)[0]), bool(ans["hit"][i]))
                # |a| == eps: the triangle's |a| < eps lets it through, the quad's |a| > eps does not; the oracle says the same
                at = (True, True) if name == "tri" else (False, False)
                assert got == dict(below=(False, False), at=at, above=(True, True), twice=(True, True)), (name, sign, way, got)


@pytest.mark.parametrize("kind", S.KINDS)
def test_lower_and_upper_bounds_are_there(kind):
    s = S.edge_set("bounds", kind)
    for name in KIND_NAMES[kind]:
        def v(*parts):
            i = one(s, name, *parts)
            ok, t, _ = s.verdict(i)
            assert same(t if ok or name == "tri" else s.terms(i)[3], -s.o[i][2])          # t is the origin's distance, exactly
            return bool(ok)
        for t_min in ("tmin0", "tmin_eps"):               # t > 1e-8f is strict: 1e-8f itself is rejected, its successor accepted
            assert [v("lower", t_min, w) for w in ("below", "eps", "eps_up", "above")] == [False, False, True, True]
        for t_min in ("tmin0.0001", "tmin0.5"):           # t >= t_min is not
            assert [v("lower", t_min, w) for w in ("below", "at", "above")] == [False, True, True]
        for t_max in ("tmax1", "tmax2.5"):                # the triangle accepts t == t_max, the quad only t < t_max ...
            assert [v("upper", t_max, w) for w in ("below", "at", "above")] == [True, name == "tri", False]
            # ... and the scene keeps neither: the closer-hit rule is the strict t < closest_t, and closest_t starts at t_max
            assert [bool(s.scene_verdict(one(s, name, "upper", t_max, w))[0]) for w in ("below", "at", "above")] == [True, False, False]
        assert v("pinched", "tmin==t==tmax") == (name == "tri") and not s.scene_verdict(one(s, name, "pinched", "tmin==t==tmax"))[0]


@pytest.mark.parametrize("kind", S.KINDS)
def test_slab_edges_are_there(kind):
    s = S.edge_set("slab", kind)
    ans = S.oracle_answers("slab", kind)
    for name in KIND_NAMES[kind]:
        targets = sorted({int(s.target[i]) for i in s.where(name, "slab")})
        assert len(targets) >= 2
        for k in targets:
            bmin, bmax = S.prim_box(s.types[k], s.verts[k])
            v = s.verts[k][: 3 if s.types[k] == TRI else 4]
            assert (bits(bmin) == bits(v.min(0))).all() and (bits(bmax) == bits(v.max(0))).all()      # the 1e-6 is rounded away
            mine = [i for i in s.where(name, "slab") if s.target[i] == k]
            def slab(i):
                return S.slab_verdict(bmin, bmax, s.o[i], s.d[i], s.t_min[i], s.t_max[i])
            def pick(*parts):
                r = [i for i in mine if all(p in s.label[i].split(":") for p in parts)]
                assert len(r) == 1, (parts, len(r))
                return r[0]
            # an origin ON a face with a zero of either sign: 0 * inf = NaN is ignored, the box is entered, the primitive hit there
            for face in ("face_x_lo", "face_x_hi", "face_y_lo", "face_y_hi", "edge_xhi_ylo", "edge_xlo_yhi"):
                for z in ("+0", "-0"):
                    i = pick(face, z)
                    a = 0 if "x" in face.split("_")[1] else 1
                    assert s.o[i][a] in (bmin[a], bmax[a]) and s.d[i][a] == 0 and np.signbit(s.d[i][a]) == (z == "-0")
                    assert slab(i)[0] and ans["hit"][i] and ans["prim"][i] == k, s.label[i]
            for z in ("+0", "-0"):
                assert slab(pick("face_z_lo", z))[0] and slab(pick("face_z_hi", z))[0]
            # through a corner: tmin_box == tmax_box passes, one float later the box is missed
            below, at, above = (pick("corner", w) for w in ("below", "at", "above"))
            ok, lo, hi = slab(at)
            assert ok and same(lo, hi) and same(lo, 1.0) and ans["hit"][at] and ans["prim"][at] == k and same(ans["t"][at], 1.0)
            assert slab(below)[0] and not slab(above)[0] and not ans["hit"][above]
            # entered exactly at closest_t: passes; one float before: missed.  Either way nothing inside is near enough.
            below, at, above = (pick("enter_at_closest", w) for w in ("below", "at", "above"))
            assert not slab(below)[0] and slab(at)[0] and same(slab(at)[1], slab(at)[2]) and slab(above)[0]
            # t_min exactly at the exit: passes, and the vertex that lies AT the exit is hit; one float later the box is missed
            below, at, above = (pick("tmin_at_exit_vertex", w) for w in ("below", "at", "above"))
            assert slab(at)[0] and same(slab(at)[1], slab(at)[2]) and ans["hit"][at] and same(ans["t"][at], 2.0)
            assert ans["hit"][below] and not slab(above)[0] and not ans["hit"][above]
            # tiny direction components: the primitive is hit whatever the component is
            for lab in ("tiny_dx", "tiny_dy", "tiny_dz", "tiny_dxdz"):
                for z, _ in S.TINY:
                    i = pick(lab, z)
                    assert ans["hit"][i] and ans["prim"][i] == k, s.label[i]
    p = S.edge_set("planar", kind)
    pa = S.oracle_answers("planar", kind)
    b = S.oracle_scene("planar", kind).bvh()
    assert (bits(b["bmin"][:, 2]) == bits(b["bmax"][:, 2])).all() and len(b["count"]) >= 5           # zero thickness, every node
    for i in range(len(p)):
        want = not p.label[i].endswith(("in_plane", "from_the_plane"))
        assert bool(pa["hit"][i]) == want and (not want or pa["prim"][i] == p.target[i]), p.label[i]


def test_nonfinite_and_extent_rays_do_what_their_labels_say():
    for kind in S.KINDS:
        s = S.edge_set("nonfinite", kind)
        ans = S.oracle_answers("nonfinite", kind)
        for name in KIND_NAMES[kind]:
            assert ans["hit"][one(s, name, "nonfinite", "control")]
            assert sum(not np.isfinite(s.d[i]).all() for i in s.where(name, "nonfinite")) >= 18
        s = S.edge_set("extent", kind)
        ans = S.oracle_answers("extent", kind)
        for name in KIND_NAMES[kind]:
            for mirror in ("plus", "minus"):
                for where, v in (("vertex", 0.0), ("edge_mid", 0.5)):
                    i = one(s, name, "extent", "u_nan", where, "far", mirror)
                    a, u, vv, t = s.terms(i)
                    assert np.isfinite(a) and np.isnan(u) and vv == F(v) and same(t, S.BIG_S), s.label[i]
                    # the reference's triangle lets the NaN u through, its quad does not
                    assert bool(s.verdict(i)[0]) == (name == "tri") == bool(ans["hit"][i]), s.label[i]
                    i = one(s, name, "extent", "u_nan", where, "near", mirror)            # the other side of the overflow
                    a, u, vv, t = s.terms(i)
                    assert u == 0 and vv == F(v) and s.verdict(i)[0] and ans["hit"][i] and ans["prim"][i] == s.target[i]
                    i = one(s, name, "extent", "q_nan", where, "far", mirror)
                    a, u, vv, t = s.terms(i)
                    assert np.isfinite(a) and np.isnan(t) and not s.verdict(i)[0] and not ans["hit"][i]
        # the scene passes the host's check as it stands: edges below 1e18, coordinate sums below 3e38
        for k in range(len(s.types)):
            v = s.verts[k][: 3 if s.types[k] == TRI else 4].astype(np.float64)
            assert np.abs(v - v[0]).max() < 1e18 and np.abs(v).sum(-1).max() < 3e38


def test_host_refuses_quads_where_the_products_could_overflow():
    """SceneState::checkExtent through the host-only scene: largest quad edge x reach <= 2^124, on both sides of the bound; scenes of
    triangles are not held to it (the reference's triangle lets a NaN through as the device does)."""
    bound = S.QUAD_REACH_BOUND
    for name in ("extent", "extent_in", "extent_out"):
        for kind in S.KINDS:
            s = S.edge_set(name, kind)
            hs = ptmi.HostScene.from_arrays(*s.scene)
            product = S.quad_reach_product(s)
            if kind == "tri" or name == "extent_in":
                assert product <= bound
                hs.check_extent()
            else:
                assert product > bound
                with pytest.raises(ptmi.PtmiError, match="quad edge"):
                    hs.check_extent()
    # the two sides lie within a factor of two of the bound, and inside it nothing overflows: every term is a number
    for kind in ("quad", "mixed"):
        s, out = S.edge_set("extent_in", kind), S.edge_set("extent_out", kind)
        assert bound / 2 < S.quad_reach_product(s) <= bound < S.quad_reach_product(out) <= 2 * bound
        for i in range(len(s)):
            assert np.isfinite(s.terms(i)).all() and (s.types[s.target[i]] == TRI or np.isfinite(s.terms(i, 1)[:3]).all()), s.label[i]
        # an origin outside the scene - a camera, a hook's ray - is held to the same bound
        hs = ptmi.HostScene.from_arrays(*s.scene)
        near, far = (0, 0, -2.0 ** 62), (0, 0, -2.0 ** 65)
        assert S.quad_reach_product(s, near) <= bound < S.quad_reach_product(s, far)
        hs.check_extent(near)
        with pytest.raises(ptmi.PtmiError, match="quad edge"):
            hs.check_extent(far)
    ptmi.HostScene.from_arrays(*S.edge_set("extent", "tri").scene).check_extent((2.0 ** 100, 0, 0))


# ------------------------------------------------------------------------------------------------
# restatement, oracle, tree, compiled reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in S.BUILDERS if not n.startswith("ties")])
def test_restatement_is_the_oracles_answer(name):
    """Outside the tie sets a ray can only hit the primitive it is aimed at: the verdict of the restatement on that primitive is
    the oracle's answer for the scene, with the same bits of t."""
    checked = 0
    for kind in S.KINDS:
        s = S.edge_set(name, kind)
        ans = S.oracle_answers(name, kind, use_bvh=False)
        for i in range(len(s)):
            ok, t, _ = s.scene_verdict(i)
            assert bool(ans["hit"][i]) == bool(ok), (kind, s.label[i])
            if ok:
                assert ans["prim"][i] == s.target[i] and same(ans["t"][i], t), (kind, s.label[i])
                checked += 1
    assert checked >= 4


def test_tree_and_linear_pass_differ_only_by_visiting_order():
    crossed = {}
    for name, kind in S.all_sets():
        s = S.edge_set(name, kind)
        tree, lin = S.oracle_answers(name, kind), S.oracle_answers(name, kind, use_bvh=False)
        assert (tree["hit"] == lin["hit"]).all() and (bits(tree["t"]) == bits(lin["t"])).all(), (name, kind)
        differ = tree["prim"] != lin["prim"]
        assert not (differ & ~s.tree_matters).any(), (name, kind)
        if not name.startswith("ties"):
            continue
        b = S.oracle_scene(name, kind).bvh()
        visit = {}                                         # primitive -> its place in the tree's leaf order
        for place, k in enumerate(b["indices"]):
            visit[int(k)] = place
        leaf_of = {}
        for node in np.nonzero(b["count"] > 0)[0]:
            for j in range(b["count"][node]):
                leaf_of[int(b["indices"][b["left"][node] + j])] = int(node)
        for i in np.nonzero(s.tree_matters)[0]:
            # coincident candidates: every primitive that the linear pass would accept at the same t
            same_t = [k for k in range(len(s.types))
                      if (lambda r: r[0] and same(r[1], lin["t"][i]))(S.prim_verdict(s.types[k], s.verts[k], s.o[i], s.d[i], s.t_min[i], s.t_max[i]))]
            assert len(same_t) >= 2 and lin["prim"][i] == min(same_t), (name, kind, s.label[i])     # load order: strict t < closest
            assert tree["prim"][i] in same_t
            if len({leaf_of[k] for k in same_t}) > 1:
                first_leaf = min(leaf_of[k] for k in same_t)                  # pre-order: the leaf with the smaller index is visited first
                assert leaf_of[int(tree["prim"][i])] == first_leaf
                if differ[i] and leaf_of[int(lin["prim"][i])] != first_leaf:
                    crossed[(name.split("_")[0], kind)] = True
            if len({leaf_of[k] for k in same_t}) == 1:
                assert tree["prim"][i] == min(same_t, key=lambda k: visit[k])                         # within a leaf: leaf order
        for i in s.where("ulp:farther:plane_first") + s.where("ulp:farther:plane_second") + s.where("ulp:nearer:plane_first") + s.where("ulp:nearer:plane_second"):
            assert tree["prim"][i] == s.target[i] == lin["prim"][i]
            assert same(tree["t"][i], 1.0 if "farther" in s.label[i] else dn(F(1))), s.label[i]
    assert all(crossed.get(("ties", kind)) for kind in S.KINDS), crossed       # ties ACROSS leaves, in every kind of scene


@pytest.mark.parametrize("name", list(S.BUILDERS))
def test_compiled_reference_agrees_on_every_ray(ref, name):
    for kind in S.KINDS:
        s = S.edge_set(name, kind)

        def ask(use_bvh):
            r = RefScene(*s.scene)
            out = dict(hit=np.zeros(len(s), np.int32), prim=np.full(len(s), -1, np.int32), t=np.zeros(len(s), F))
            for t_min, t_max, idx in s.groups():
                h = r.intersect(s.o[idx], s.d[idx], t_min, t_max, use_bvh)
                for j, i in enumerate(idx):
                    out["hit"][i] = h[j].hit
                    if h[j].hit:
                        out["prim"][i], out["t"][i] = h[j].prim, h[j].t
            return out
        for use_bvh in (True, False):
            want = ref(f"{name}/{kind}/{'tree' if use_bvh else 'linear'}", lambda: ask(use_bvh))
            got = S.oracle_answers(name, kind, use_bvh)
            assert (got["hit"] == want["hit"]).all() and (got["prim"] == want["prim"]).all(), (name, kind, use_bvh)
            assert (bits(got["t"]) == bits(want["t"])).all(), (name, kind, use_bvh)
