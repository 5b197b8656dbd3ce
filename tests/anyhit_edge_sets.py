"""Scenes that put ONE blocker on an edge of the solver's visibility question (csrc/anyhit.h; visibility_test_anyhit,
form_factors.h:143-208), reached through the point-to-point form factors (use_monte_carlo = 0).

The pair is always (0, 1).  The kernel (csrc/form_factors.hip: p2p_pair) asks along the segment
    o = centroid_0 + 1e-4f * normal_0,   d = unit_vector((centroid_1 - centroid_0) / r),   max_dist = r - 2e-4f,   r = |centroid_1 - centroid_0|
and a primitive other than 0 and 1 blocks if Primitive::intersect(ray, 1e-5f, max_dist) accepts: a triangle with
1e-5f <= t <= max_dist, a quad with 1e-5f <= t < max_dist.  The source lies in the plane z = -1e-4f with its centroid at
(0, 0, -1e-4f) and the normal (0, 0, 1), the target in z = 4 with its centroid at (0, 0, 4): o = (0, 0, 0) exactly, d = (0, 0, 1)
- two direction components are zeros, which anyhit_inv turns into the slope 1e8 - and a blocker in the plane z = zb is met at
t = zb exactly.  segment() restates the three formulas in float32; the host test checks them against these numbers.  The
node-level cases move the target (z = 128, z = 64 + 13 floats) or its vertices; anyhit_slab restates the node test.

Each case is a family of scenes that differ by one float of one blocker coordinate, with the verdict (blocked or not) that the
reference's rules give each member.  3 to 40 primitives per scene.
"""
import functools

import numpy as np

from intersect_edge_sets import F, TRI, QUAD, EPS, EPS_UP, EPS_DN, UNIT_TRI, UNIT_QUAD, around, up, dn

ZS = -F(1e-4)
T_LO = F(1e-5)
Z_TMAX_LO = F(8.999999e-06)           # fl(Z_TMAX_LO + 1e-6f) == 1e-5f: the one float with that sum


def segment(types, verts, normal):
    """(o, d, max_dist) of the pair (0, 1) as p2p_pair forms it (centroids: primitive.h:92-98), float32"""
    def over(v, t):                                    # vector.h's v / t: v * (1 / t), the reciprocal rounded to float32
        return (v * F(1.0 / np.float64(t))).astype(F)

    def centroid(k):
        v = verts[k]
        return over((v[0] + v[1]) + v[2], F(3)) if types[k] == TRI else (((v[0] + v[1]) + v[2]) + v[3]) * F(0.25)
    ci, cj = centroid(0), centroid(1)
    vec = (cj - ci).astype(F)
    r = np.sqrt((F(0) + vec[0] * vec[0]) + vec[1] * vec[1] + vec[2] * vec[2], dtype=F)
    d = over(vec, r)
    d = over(d, np.sqrt((F(0) + d[0] * d[0]) + d[1] * d[1] + d[2] * d[2], dtype=F))
    o = (ci + F(1e-4) * normal[0]).astype(F)
    return o, d, F(r - F(2e-4))


def scene(pair_kind, blockers, n_fill=1, target_dx=None, target_z=4, fill_z=1, target=None):
    """source (0) and target (1) of pair_kind, the blockers (kind, verts), n_fill primitives far off the segment in the plane
    z = fill_z; target: the target's vertices as given (its plane is then its own)"""
    big = (UNIT_TRI * F(3) - F(1)) if pair_kind == TRI else (UNIT_QUAD * F(2) - F(1))       # centroid (0, 0): (-1,-1) (2,-1) (-1,2)
    big = big * np.array([1, 1, 0], F)
    prims = [(pair_kind, big + np.array([0, 0, ZS], F)), (pair_kind, big + np.array([0, 0, F(target_z)], F))]
    if target_dx is not None:                          # the target's x coordinates as given: its centroid leaves the axis
        v = prims[1][1].copy(); v[:, 0] = np.asarray(target_dx, F); prims[1] = (pair_kind, v)
    if target is not None:
        prims[1] = (pair_kind, np.asarray(target, F))
    prims += list(blockers)
    for k in range(n_fill):
        shape = UNIT_TRI if (k % 2 == 0) == (pair_kind == TRI) else UNIT_QUAD
        prims.append((TRI if len(shape) == 3 else QUAD, shape + np.array([8 + 2 * k, 0, F(fill_z)], F)))
    n = len(prims)
    types = np.array([k for k, _ in prims], np.int32)
    verts = np.zeros((n, 4, 3), F)
    for i, (_, v) in enumerate(prims):
        verts[i, : len(v)] = v
    normal = np.tile(np.array([[0, 0, 1]], F), (n, 1)); normal[1] = [0, 0, -1]
    bsdf = np.full((n, 3), 0.5, F); Le = np.zeros((n, 3), F); Le[0] = 1.0
    return types, verts, normal, bsdf, Le


def target_at(kind, z):
    """the big target with its centroid at (0, 0, z) EXACTLY.  A quad in the plane z has it; a triangle's (3 z) / 3 may round away
    from z, so its three heights are taken a few floats apart - the first such triple, by smallest spread, whose centroid is z."""
    big = ((UNIT_TRI * F(3) - F(1)) if kind == TRI else (UNIT_QUAD * F(2) - F(1))) * np.array([1, 1, 0], F)
    if kind == QUAD:
        return big + np.array([0, 0, z], F)
    third = F(1.0 / np.float64(F(3)))
    near = [dn(z, n) for n in range(4, 0, -1)] + [F(z)] + [up(z, n) for n in range(1, 5)]
    triples = sorted(((max(a, b, c) - min(a, b, c), i, j, l) for i, a in enumerate(near) for j, b in enumerate(near) for l, c in enumerate(near)
                      if F(F(F(a + b) + c) * third) == F(z)))
    _, i, j, l = triples[0]
    v = big.copy(); v[:, 2] = [near[i], near[j], near[l]]
    return v


def blocker(kind, at, shape=None):
    shape = (UNIT_TRI if kind == TRI else UNIT_QUAD) if shape is None else np.asarray(shape, F)
    return kind, (shape + np.asarray(at, F)).astype(F)


@functools.lru_cache(maxsize=None)
def cases():
    """{case: [(member, scene arrays, blocked)]}"""
    out = {}
    probe = scene(TRI, [])
    max_dist = segment(probe[0], probe[1], probe[2])[2]
    for kname, k in (("tri", TRI), ("quad", QUAD)):
        inside = (-0.25, -0.25) if k == TRI else (-0.75, -0.25)            # the axis passes through the blocker's interior
        # t at 1e-5f: t >= 1e-5f blocks
        out[f"{kname}:t_lo"] = [(w, scene(k, [blocker(k, inside + (z,))], 2), bool(z >= T_LO))
                                for w, z in zip(("below", "at", "above"), around(T_LO))]
        # t at max_dist: the triangle accepts t <= max_dist, the quad only t < max_dist
        out[f"{kname}:t_hi"] = [(w, scene(k, [blocker(k, inside + (z,))], 2), bool(z < max_dist or (z == max_dist and k == TRI)))
                                for w, z in zip(("below", "at", "above"), around(max_dist))]
        # touching at u == 0 (the axis runs along the blocker's edge x == x0), one float either side
        y0 = F(-0.25)
        out[f"{kname}:u0"] = [(w, scene(k, [blocker(k, (x0, y0, 1))], 3), bool(x0 <= 0))
                              for w, x0 in zip(("inside", "on", "outside"), around(F(0.0)))]
        # through the vertex v0, and one float outside it in y (v < 0)
        out[f"{kname}:vertex"] = [(w, scene(k, [blocker(k, (0, y, 1))], 1), bool(y <= 0))
                                  for w, y in zip(("inside", "on", "outside"), around(F(0.0)))]
        # |a| at 1e-8f: a sliver of width w; the triangle accepts |a| == eps, the quad does not
        for sign in (1, -1):
            fam = []
            for w_, wd in (("below", EPS_DN), ("at", EPS), ("above", EPS_UP)):
                wd = F(sign) * wd
                shape = [[0, 0, 0], [wd, 0, 0], [0, 1, 0]] if k == TRI else [[0, 0, 0], [wd, 0, 0], [wd, 1, 0], [0, 1, 0]]
                at = (-wd * (F(0.25) if k == TRI else F(0.5)), -0.25, 1)
                fam.append((w_, scene(k, [blocker(k, at, shape)], 2), bool(wd * sign > EPS or (abs(wd) == EPS and k == TRI))))
            out[f"{kname}:det_{'pos' if sign > 0 else 'neg'}"] = fam
        # ---- the slab test of a NODE (form_factors.h:162-180: tmax < 1e-5f || tmin > max_dist || tmin > tmax skips it) ----
        # tmin == tmax: the blocker and its leaf-mates lie in the plane z = 64, where the 1e-6 by which a box is widened is rounded
        # away; the leaf's box has no thickness in z, the axis enters and leaves it at t = 64, and the blocker there is hit
        out[f"{kname}:node_tmin_eq_tmax"] = [("flat", scene(k, [blocker(k, inside + (64,))], 4, target_z=128, fill_z=64), True),
                                             ("absent", scene(k, [], 5, target_z=128, fill_z=64), False)]
        # tmin == max_dist: the target's centroid 13 floats above 64 (target_at) makes max_dist = fl(fl(zt + 1e-4f) - 2e-4f) == 64 exactly; a TRIANGLE in
        # the plane z = 64 (flat box: tmin == 64) is accepted at t == max_dist.  One float less of zt: max_dist < 64, open.
        out[f"{kname}:node_tmin_eq_max_dist"] = [(w, scene(k, [blocker(TRI, (-0.25, -0.25, 64))], 4, target=target_at(k, up(F(64), n)), fill_z=64), b)
                                                 for w, n, b in (("at", 13, True), ("beyond", 12, False))]
        # tmax == 1e-5f: fl(zb + 1e-6f) == 1e-5f for zb = 8.999999e-6f, so the box of primitives in the plane z = zb is left at
        # exactly 1e-5f and is NOT skipped - but whatever it holds is met at t <= zb < 1e-5f and rejected by the primitive's own
        # t >= 1e-5f: the decision cannot turn a row.  Built all the same: the row is the open one, with and without.
        out[f"{kname}:node_tmax_eq_lo"] = [("touching", scene(k, [blocker(k, inside + (Z_TMAX_LO,))], 4, target_z=16, fill_z=Z_TMAX_LO), False),
                                           ("absent", scene(k, [], 5, target_z=16, fill_z=Z_TMAX_LO), False)]
        # a direction component of -0: the x sum of the target's vertices is -2^-149, its centroid's x underflows to -0 and
        # cj.x - ci.x = (-0) - (+0) = -0.  anyhit_inv's slope is +1e8 all the same.
        tgt = [[-1.5, -1, 4], [1.5, -1, 4], [-(2.0 ** -149), 2, 4]] if k == TRI else [[-1, 0, 4], [0, -1, 4], [1, 0, 4], [-(2.0 ** -149), 1, 4]]
        out[f"{kname}:negative_zero_dx"] = [("open", scene(k, [], 2, target=tgt), False),
                                            ("blocked", scene(k, [blocker(k, inside + (1,))], 2, target=tgt), True)]
        # source and target are the only candidates on the axis: nothing blocks, with 1 and with 38 bystanders.  (Both lie
        # outside [1e-5f, max_dist] on the segment, so these do not show that the walk SKIPS them: quad:pair_skipped does.)
        out[f"{kname}:pair_only"] = [("3", scene(k, [], 1), False), ("40", scene(k, [], 38), False)]
        # a direction component of -5e-9 (the target's centroid 2^-24 / 3, or 2^-26, off the axis): anyhit_inv's slope is +1e8 there
        dx = (-0.5, 1.0, F(-0.5) - F(2.0 ** -24)) if k == TRI else (-0.5, 0.5, 0.5, F(-0.5) - F(2.0 ** -24))
        out[f"{kname}:tiny_negative_dx"] = [("open", scene(k, [], 2, dx), False),
                                            ("blocked", scene(k, [blocker(k, inside + (1,))], 2, dx), True)]
    # the pair's own primitives are skipped, not merely out of range: the target is folded along its diagonal v00-v11, which
    # crosses the axis at z = 2 (t = 2, inside [1e-5f, max_dist]) while its centroid stays at z = 4.  Tested like any other
    # primitive it would block its own pair.  (A triangle is planar and meets the segment at its centroid only: no such case.)
    folded = [[-1, -1, 2], [1, -1, 6], [1, 1, 2], [-1, 1, 6]]
    out["quad:pair_skipped"] = [("folded", scene(QUAD, [], 3, target=folded), False)]
    # the quad's diagonal: both halves touch the axis; one float off it, one half still does
    out["quad:diagonal"] = [(w, scene(QUAD, [blocker(QUAD, (x0, -0.5, 1))], 2), True)
                            for w, x0 in zip(("below", "on", "above"), around(F(-0.5)))]
    return out


def all_scenes():
    return [(case, member, arrs, blocked) for case, fam in cases().items() for member, arrs, blocked in fam]


def anyhit_slab(bmin, bmax, o, d, max_dist):
    """the slab test of visibility_test_anyhit on one box (form_factors.h:157-180), float32: (visited, tmin, tmax)"""
    with np.errstate(all="ignore"):
        inv = [F(1) / (F(d[a]) if abs(F(d[a])) > F(1e-8) else F(1e-8)) for a in range(3)]
        tmin, tmax = None, None
        for a in range(3):
            t1, t2 = (F(bmin[a]) - F(o[a])) * inv[a], (F(bmax[a]) - F(o[a])) * inv[a]
            lo, hi = min(t1, t2), max(t1, t2)
            tmin, tmax = (lo, hi) if a == 0 else (max(tmin, lo), min(tmax, hi))
        return (not (tmax < F(1e-5) or tmin > F(max_dist) or tmin > tmax)), tmin, tmax
