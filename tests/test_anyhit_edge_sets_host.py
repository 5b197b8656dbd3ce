"""The blocker scenes of the any-hit tests (tests/anyhit_edge_sets.py), proven on the CPU - no GPU: the segment each scene states
is the one the oracle's solver asks along, every blocker sits where its label says, and each placed blocker turns the form
factor of its pair - moving it by one float, or taking it away, changes the row."""
import ctypes as C

import numpy as np
import pytest

import anyhit_edge_sets as A
import intersect_edge_sets as S
from intersect_edge_sets import F, TRI, QUAD
from oracle_binding import OracleScene, oracle_lib


@pytest.fixture(scope="module")
def solved():
    """per scene: (oracle scene, the oracle's form-factor rows 0 and 1)"""
    out = {}
    for case, member, arrs, blocked in A.all_scenes():
        o = OracleScene.from_arrays(*arrs)
        out[(case, member)] = (o, o.form_factor_rows([0, 1], use_monte_carlo=False, num_iterations=1)[0])
    return out


def test_every_case_is_there():
    cases = A.cases()
    assert len(cases) == 26 and len(A.all_scenes()) == 64
    for case, fam in cases.items():
        for member, arrs, blocked in fam:
            assert 3 <= len(arrs[0]) <= 40 and set(arrs[0][:2].tolist()) == {TRI if case.startswith("tri") else QUAD}
    assert max(len(a[0]) for _, _, a, _ in A.all_scenes()) == 40


def test_segment_and_verdicts(solved):
    L = oracle_lib()
    flips = 0
    for case, fam in A.cases().items():
        verdicts = []
        for member, arrs, blocked in fam:
            types, verts, normal = arrs[0], arrs[1], arrs[2]
            o, d, max_dist = A.segment(types, verts, normal)
            scene, rows = solved[(case, member)]
            # the stated segment: the source's centroid is the oracle's, the origin is (0, 0, 0) exactly
            area, c0 = scene.prim_geometry(0)
            assert (c0 == np.array([0, 0, A.ZS], F)).all() and (o == 0).all(), (case, member)
            c1 = scene.prim_geometry(1)[1]                      # r = sqrt(fl(dz * dz)) for a target on the axis
            if c1[0] == 0:
                dz = F(c1[2] - A.ZS)
                assert max_dist == F(np.sqrt(F(dz * dz), dtype=F) - F(2e-4)), (case, member)
            if "tiny_negative_dx" in case:                      # fl(-2^-24 / 3) / 4 and -2^-26 / 4, normalised: within 1e-8 of zero
                assert d[0] == F(float.fromhex("-0x1.555326p-28" if case.startswith("tri") else "-0x1.fffcb8p-29")) and abs(d[0]) < F(1e-8)
                assert d[1] == 0 and not np.signbit(d[1]), (case, d)
            elif "negative_zero_dx" in case:
                assert d[0] == 0 and np.signbit(d[0]) and d[1] == 0 and not np.signbit(d[1]) and d[2] == 1, (case, d)
            else:
                assert (d == np.array([0, 0, 1], F)).all() and np.signbit(d[:2]).sum() == 0, (case, d)
            got = L.po_visibility_blocked(scene.h, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), C.c_float(float(max_dist)), 0, 1)
            assert bool(got) == blocked, (case, member)
            # the restatement of the reference's primitive tests says the same of the blocker (primitive 2), from its own t
            if len(types) > 2 and "pair_only" not in case:
                ok, t, _ = S.prim_verdict(types[2], verts[2], o, d, 1e-5, max_dist)
                if types[2] == QUAD: ok = ok and t < max_dist
                assert bool(ok) == blocked, (case, member, t)
                if case.endswith(("t_lo", "t_hi")):                  # t is the blocker's height, exactly
                    assert S.mt_terms(verts[2][0], verts[2][1], verts[2][2], o, d)[3] == verts[2][0][2]
            # ... and the pair's form factor is zero exactly where it is blocked (row 1 asks from the target: another segment)
            assert (rows[0, 1] == 0) == blocked, (case, member, rows[0, 1])
            verdicts.append(blocked)
            # ---- the node-level cases: the box of the leaf that holds primitive 2, through the restated slab test ----
            if "node_" in case or case == "quad:pair_skipped":
                b = scene.bvh()
                leaf = [n for n in np.nonzero(b["count"] > 0)[0] if 2 in b["indices"][b["left"][n]: b["left"][n] + b["count"][n]]][0]
                visited, tmin, tmax = A.anyhit_slab(b["bmin"][leaf], b["bmax"][leaf], o, d, max_dist)
            if case.endswith("node_tmin_eq_tmax") and member == "flat":
                assert visited and tmin == tmax == F(64) and b["bmin"][leaf][2] == b["bmax"][leaf][2] == F(64)
            if case.endswith("node_tmin_eq_max_dist"):
                assert tmin == F(64) and tmax > tmin and visited == (member == "at") and (max_dist == F(64)) == (member == "at")
                assert max_dist == (F(64) if member == "at" else F(float.fromhex("0x1.fffffcp+5")))
            if case.endswith("node_tmax_eq_lo") and member == "touching":
                inner = [n for n in range(len(b["count"])) if b["count"][n] == 0 and A.anyhit_slab(b["bmin"][n], b["bmax"][n], o, d, max_dist)[2] == F(1e-5)]
                assert visited and tmax == F(1e-5) and tmin < tmax and inner             # a leaf AND an inner node left at exactly 1e-5f
                assert F(A.Z_TMAX_LO + F(1e-6)) == F(1e-5) and A.Z_TMAX_LO < F(1e-5)
                assert S.mt_terms(verts[2][0], verts[2][1], verts[2][2], o, d)[3] == A.Z_TMAX_LO          # met below 1e-5f: rejected
                other = solved[(case, "absent")][1]
                assert rows[0, 1] == other[0, 1] and rows[0, 1] > 0                                      # the row is the open one either way
            if case == "quad:pair_skipped":
                # the target, tested like any other primitive, is hit inside the bounds - on its fold, both halves - ...
                ok, t, stages = S.prim_verdict(QUAD, verts[1], o, d, 1e-5, max_dist)
                assert ok and t == F(2) and t < max_dist and stages == ("hit", "t")
                # ... and the oracle's walk says "blocked" as soon as it is not told to skip it
                assert L.po_visibility_blocked(scene.h, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), C.c_float(float(max_dist)), 0, -1)
                assert rows[0, 1] > 0
        if len(set(verdicts)) > 1:
            flips += 1
        else:
            assert case.split(":")[1] in ("pair_only", "diagonal", "node_tmax_eq_lo", "pair_skipped"), case
    assert flips == 20
    # the two kinds differ exactly where the contract says: t == max_dist and |a| == 1e-8f
    for name in ("t_hi", "det_pos", "det_neg"):
        tri = dict((m, b) for m, _, b in A.cases()[f"tri:{name}"]); quad = dict((m, b) for m, _, b in A.cases()[f"quad:{name}"])
        assert tri["at"] and not quad["at"] and tri["below"] == quad["below"] and tri["above"] == quad["above"]
