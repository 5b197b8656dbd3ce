"""Rays aimed at the decisions of the closest-hit walks: every ray of every set sits on, or one float beside, an edge of the
ray/primitive test (triangle.h:64-96, quad.h:49-132), of the slab test (scene.h:66-81) or of the closer-hit rule (scene.h:89-96).

Coordinates are dyadic - small integers times powers of two - and directions are axis-aligned or have small dyadic components, so
every product of Moller-Trumbore and of the slab test is exact and u, v, t, a and the slab distances are known exactly.  For the
unit triangle (0,0,0) (1,0,0) (0,1,0) and the ray from (x, y, -t) along +z:  a = -1, u = x, v = y, t = t.  For the unit quad
(0,0,0) (1,0,0) (1,1,0) (0,1,0): half (v00, v10, v11) has u = x - y, v = y, half (v00, v11, v01) has u = x, v = y - x.  The
neighbours of an edge are one np.nextafter step of an origin or vertex coordinate away.

A set is a scene (arrays for load_scene_arrays / OracleScene.from_arrays) and rays (o, d, t_min, t_max) with, per ray, a label
naming the edge and the load index of the primitive it is aimed at.  mt_terms / tri_verdict / quad_verdict / slab_verdict restate the
REFERENCE's formulas in float32 numpy scalars - its order of operations, its early-outs, the true division - and are used only to
label rays and to prove on the CPU (tests/test_intersect_edge_sets_host.py) that each edge is really there.  Everything is
deterministic; nothing here is random.
"""
import numpy as np

F = np.float32
TRI, QUAD = 0, 1
KINDS = ("tri", "quad", "mixed")
EPS = F(1e-8)                                   # EPSILON of triangle.h / quad.h
FLT_MAX = F(np.finfo(F).max)
INF = F(np.inf)
T_MIN = F(1e-4)                                 # the t_min of every ray that does not test a bound


def up(x, n=1):
    x = F(x)
    for _ in range(n):
        x = np.nextafter(x, INF)
    return x


def dn(x, n=1):
    x = F(x)
    for _ in range(n):
        x = np.nextafter(x, -INF)
    return x


def around(x, n=1):
    """x with its n float neighbours on either side, ascending"""
    return [dn(x, k) for k in range(n, 0, -1)] + [F(x)] + [up(x, k) for k in range(1, n + 1)]


EPS_UP, EPS_DN = up(EPS), dn(EPS)


# ------------------------------------------------------------------------------------------------
# the reference's formulas, float32 (labels only)
# ------------------------------------------------------------------------------------------------
def _v(a):
    return [F(a[0]), F(a[1]), F(a[2])]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _dot(a, b):                                 # vector.h:198-203
    s = F(0)
    s = s + a[0] * b[0]
    s = s + a[1] * b[1]
    s = s + a[2] * b[2]
    return s


def _cross(a, b):                               # vector.h:211-218
    return [a[1] * b[2] - a[2] * b[1], -(a[0] * b[2] - a[2] * b[0]), a[0] * b[1] - a[1] * b[0]]


def mt_terms(v0, va, vb, o, d):
    """(a, u, v, t) of Moller-Trumbore for the triangle (v0, va, vb), every term computed whatever the others are"""
    with np.errstate(all="ignore"):
        v0, va, vb, o, d = _v(v0), _v(va), _v(vb), _v(o), _v(d)
        e1, e2 = _sub(va, v0), _sub(vb, v0)
        h = _cross(d, e2)
        a = _dot(e1, h)
        f = F(1) / a
        s = _sub(o, v0)
        u = f * _dot(s, h)
        q = _cross(s, e1)
        v = f * _dot(d, q)
        t = f * _dot(e2, q)
        return a, u, v, t


def tri_verdict(verts, o, d, t_min, t_max):
    """Triangle::intersect (triangle.h:64-96): (accepted, t, stage of the exit)"""
    with np.errstate(all="ignore"):
        a, u, v, t = mt_terms(verts[0], verts[1], verts[2], o, d)
        if abs(a) < EPS: return False, t, "a"
        if u < 0 or u > 1: return False, t, "u"
        if v < 0 or u + v > 1: return False, t, "v"
        if t > EPS and t >= F(t_min) and t <= F(t_max): return True, t, "hit"
        return False, t, "t"


def quad_half_verdict(v0, va, vb, o, d, t_min, closest):
    with np.errstate(all="ignore"):
        a, u, v, t = mt_terms(v0, va, vb, o, d)
        if not abs(a) > EPS: return False, t, "a"
        if not (u >= 0 and u <= 1): return False, t, "u"
        if not (v >= 0 and u + v <= 1): return False, t, "v"
        if t > EPS and t >= F(t_min) and t < closest: return True, t, "hit"
        return False, t, "t"


def quad_verdict(verts, o, d, t_min, t_max):
    """Quad::intersect (quad.h:49-132): (accepted, t, (stage of half 1, stage of half 2))"""
    closest = F(t_max)
    h1, t1, s1 = quad_half_verdict(verts[0], verts[1], verts[2], o, d, t_min, closest)
    if h1: closest = t1
    h2, t2, s2 = quad_half_verdict(verts[0], verts[2], verts[3], o, d, t_min, closest)
    if h2: closest = t2
    return (h1 or h2), closest, (s1, s2)


def prim_verdict(kind, verts, o, d, t_min, t_max):
    return tri_verdict(verts, o, d, t_min, t_max) if kind == TRI else quad_verdict(verts, o, d, t_min, t_max)


def passes_a_u(kind, verts, o, d):
    """whether any half of the primitive passes the (a, u) stage: the stage behind which the walks vote"""
    halves = [(0, 1, 2)] if kind == TRI else [(0, 1, 2), (0, 2, 3)]
    with np.errstate(all="ignore"):
        for i, j, k in halves:
            a, u, _, _ = mt_terms(verts[i], verts[j], verts[k], o, d)
            if not abs(a) < EPS and not (u < 0 or u > 1):      # a NaN passes, as it does in triangle.h
                return True
    return False


def prim_box(kind, verts):
    """BVHBuilder::computeBounds of one primitive (bvh.h:108-148): its bounds widened by 1e-6, in float32"""
    v = np.asarray(verts, F)[: 3 if kind == TRI else 4]
    return (v.min(0) - F(1e-6)).astype(F), (v.max(0) + F(1e-6)).astype(F)


def slab_verdict(bmin, bmax, o, d, t_min, closest):
    """the slab test of scene.h:57-81: (passes, tmin_box, tmax_box)"""
    with np.errstate(all="ignore"):
        tmin_box, tmax_box = F(t_min), F(closest)
        for a in range(3):
            inv = F(1) / F(d[a])
            t0 = (F(bmin[a]) - F(o[a])) * inv
            t1 = (F(bmax[a]) - F(o[a])) * inv
            if inv < 0: t0, t1 = t1, t0
            tmin_box = t0 if t0 > tmin_box else tmin_box
            tmax_box = t1 if t1 < tmax_box else tmax_box
        return (not tmax_box < tmin_box), tmin_box, tmax_box


# ------------------------------------------------------------------------------------------------
# scenes and rays
# ------------------------------------------------------------------------------------------------
UNIT_TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
UNIT_QUAD = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F)


class EdgeSet:
    """scene: (types, verts, normal, bsdf, Le);  o, d: (n, 3);  t_min, t_max: (n,);  label: n strings;  target: (n,) load index of
    the primitive a ray is aimed at (-1: none);  tree_matters: (n,) the answer depends on the order in which the tree visits"""

    def __init__(self, name, kind, big=False, big_at=(-40, -40, 0)):
        self.name, self.kind, self.big, self.big_at = name, kind, big, big_at
        self._prims, self._rays = [], []

    def _filler_kinds(self):
        return {"tri": (TRI,), "quad": (QUAD,), "mixed": (TRI, QUAD)}[self.kind]

    # -- building --
    def prim(self, kind, verts, at=(0, 0, 0)):
        v = np.zeros((4, 3), F)
        vv = (np.asarray(verts, F) + np.asarray(at, F)).astype(F)
        v[: len(vv)] = vv
        self._prims.append((kind, v))
        return len(self._prims) - 1

    def ray(self, o, d, label, target=-1, t_min=T_MIN, t_max=FLT_MAX, tree_matters=False):
        self._rays.append((np.asarray(o, F), np.asarray(d, F), F(t_min), F(t_max), label, target, tree_matters))

    def fillers(self, count, first=(2, 0, 0), step=(2, 0, 0), kinds=None):
        """small primitives beside the targets, so that the scene has a tree and a target's leaf holds more than the target"""
        kinds = kinds or self._filler_kinds()
        for k in range(count):
            kind = kinds[k % len(kinds)]
            at = np.asarray(first, F) + F(k) * np.asarray(step, F)
            self.prim(kind, (UNIT_TRI if kind == TRI else UNIT_QUAD) * F(0.5), at)

    def finish(self, reverse=False):
        if self.big:                                       # 128 more primitives, away from every ray: the scenes of the wide tree
            at = np.asarray(self.big_at, F)
            for k in range(128):
                self.fillers(1, first=at + np.array([-2 * (k % 16), -2 * (k // 16), 0], F), kinds=(self._filler_kinds()[k % len(self._filler_kinds())],))
        prims = self._prims
        order = list(range(len(prims)))
        if reverse:
            order.reverse()
        new_index = {old: new for new, old in enumerate(order)}
        n = len(prims)
        self.types = np.array([prims[i][0] for i in order], np.int32)
        self.verts = np.array([prims[i][1] for i in order], F)
        k = np.arange(n)
        self.normal = np.stack([(k % 8) / 8.0, (k // 8 % 8) / 8.0, np.ones(n)], 1).astype(F)      # one normal per primitive
        self.bsdf = np.full((n, 3), 0.5, F)
        self.Le = np.zeros((n, 3), F); self.Le[0] = 1.0
        r = self._rays
        self.o = np.array([x[0] for x in r], F).reshape(-1, 3); self.d = np.array([x[1] for x in r], F).reshape(-1, 3)
        self.t_min = np.array([x[2] for x in r], F); self.t_max = np.array([x[3] for x in r], F)
        self.label = [x[4] for x in r]
        self.target = np.array([new_index.get(x[5], -1) for x in r], np.int32)
        self.tree_matters = np.array([x[6] for x in r], bool)
        for a in (self.types, self.verts, self.normal, self.bsdf, self.Le, self.o, self.d, self.t_min, self.t_max, self.target):
            a.setflags(write=False)
        del self._prims, self._rays
        return self

    # -- reading --
    @property
    def scene(self):
        return self.types, self.verts, self.normal, self.bsdf, self.Le

    def __len__(self):
        return len(self.label)

    def groups(self):
        """[(t_min, t_max, ray indices)]: the rays that one debug_intersect call can take together"""
        key = np.stack([self.t_min.view(np.uint32), self.t_max.view(np.uint32)], 1)
        out = []
        for k in np.unique(key, axis=0):
            idx = np.nonzero((key == k).all(1))[0]
            out.append((float(self.t_min[idx[0]]), float(self.t_max[idx[0]]), idx))
        return out

    def verdict(self, i):
        """the restatement's verdict of ray i on its target: (accepted, t, stage)"""
        k = self.target[i]
        return prim_verdict(self.types[k], self.verts[k], self.o[i], self.d[i], self.t_min[i], self.t_max[i])

    def scene_verdict(self, i):
        """the same with the closer-hit rule of scene.h:89-96 on top: closest_t starts at t_max and a hit must lie strictly below"""
        ok, t, stage = self.verdict(i)
        return bool(ok and t < self.t_max[i]), t, stage

    def terms(self, i, half=0):
        k = self.target[i]
        a, b, c = ((0, 1, 2), (0, 2, 3))[half]
        return mt_terms(self.verts[k][a], self.verts[k][b], self.verts[k][c], self.o[i], self.d[i])

    def where(self, *parts):
        """indices of the rays whose label holds every one of `parts` as a ':'-separated field"""
        return [i for i, s in enumerate(self.label) if all(p in s.split(":") for p in parts)]


def _targets(s, y_step=4):
    """the unit primitive(s) of the set's kind, stacked in y: [(name, kind, load index, y offset)]"""
    out = []
    for name, kind, shape in (("tri", TRI, UNIT_TRI), ("quad", QUAD, UNIT_QUAD)):
        if s.kind in (name, "mixed"):
            y = F(len(out) * y_step)
            out.append((name, kind, s.prim(kind, shape, (0, y, 0)), y))
    return out


INTERIOR = {"tri": (F(0.25), F(0.25)), "quad": (F(0.75), F(0.25))}
TRI_POINTS = [("v0", 0, 0), ("v1", 1, 0), ("v2", 0, 1), ("e_v0", 0.25, 0), ("e_u0", 0, 0.25), ("e_uv1", 0.25, 0.75), ("e_uv1_mid", 0.5, 0.5),
              ("inside", 0.25, 0.25)]
QUAD_POINTS = [("v00", 0, 0), ("v10", 1, 0), ("v11", 1, 1), ("v01", 0, 1), ("e_bottom", 0.5, 0), ("e_right", 1, 0.5), ("e_top", 0.5, 1),
               ("e_left", 0, 0.5), ("diag_lo", 0.25, 0.25), ("diag_mid", 0.5, 0.5), ("diag_hi", 0.75, 0.75), ("half1", 0.75, 0.25),
               ("half2", 0.25, 0.75)]
OBLIQUE = (F(0.25), F(-0.5), F(1.0))


def barycentric_set(kind, big=False):
    """u == 0, u == 1, v == 0, u + v == 1 with two float neighbours either side: through each vertex, along each edge, on the
    quad's diagonal.  Directions: +z from below, -z from above (a changes sign), one oblique dyadic direction."""
    s = EdgeSet("barycentric", kind, big)
    for name, k, idx, y0 in _targets(s):
        for pname, px, py in (TRI_POINTS if k == TRI else QUAD_POINTS):
            xs, ys = around(px, 2), around(py, 2)
            for i, x in enumerate(xs):
                for j, y in enumerate(ys):
                    step = f"dx{i - 2:+d}dy{j - 2:+d}"
                    if y0 != 0 and j != 2:
                        continue                       # y0 + a neighbour of y is not a float: the stacked target steps in x only
                    s.ray((x, y0 + y, -1), (0, 0, 1), f"{name}:bary:{pname}:{step}:up", idx)
                    s.ray((x, y0 + y, 1), (0, 0, -1), f"{name}:bary:{pname}:{step}:down", idx)
                    s.ray((x - OBLIQUE[0], y0 + y - OBLIQUE[1], -1), OBLIQUE, f"{name}:bary:{pname}:{step}:oblique", idx)
    s.fillers(11)
    return s.finish()


def determinant_set(kind, big=False):
    """|a| below, at and above 1e-8f in both signs: edge1 = (x, 0, 0), edge2 = (0, 1, 0), d = (0, 0, +-1) give a = -+x exactly.
    At |a| == 1e-8f the triangle accepts (it rejects |a| < eps) and the quad rejects (it accepts |a| > eps)."""
    s = EdgeSet("determinant", kind, big)
    row = 0
    for name, k in (("tri", TRI), ("quad", QUAD)):
        if kind not in (name, "mixed"):
            continue
        for sign in (1, -1):
            for where, x in (("below", EPS_DN), ("at", EPS), ("above", EPS_UP), ("twice", F(2) * EPS)):
                w, y0 = F(sign) * x, F(4 * row)
                row += 1
                shape = [[0, 0, 0], [w, 0, 0], [0, 1, 0]] if k == TRI else [[0, 0, 0], [w, 0, 0], [w, 1, 0], [0, 1, 0]]
                idx = s.prim(k, shape, (0, y0, 0))
                ox = w * (F(0.25) if k == TRI else F(0.5))
                s.ray((ox, y0 + F(0.25), -1), (0, 0, 1), f"{name}:det:{where}:{'pos' if sign > 0 else 'neg'}:up", idx)
                s.ray((ox, y0 + F(0.25), 1), (0, 0, -1), f"{name}:det:{where}:{'pos' if sign > 0 else 'neg'}:down", idx)
    s.fillers(7)
    return s.finish()


def bounds_set(kind, big=False):
    """The lower bound t > 1e-8f && t >= t_min (t_min 0, exactly 1e-8f, 1e-4, 0.5) and the upper bound (the triangle accepts
    t == t_max, the quad only t < t_max): t is the distance of the origin below the plane, exactly."""
    s = EdgeSet("bounds", kind, big)
    for name, k, idx, y0 in _targets(s):
        x, y = INTERIOR[name]
        def shoot(t, t_min, t_max, label):
            s.ray((x, y0 + y, -t), (0, 0, 1), f"{name}:{label}", idx, t_min, t_max)
        for i, t in enumerate([EPS_DN, EPS, EPS_UP, up(EPS_UP)]):
            shoot(t, 0.0, FLT_MAX, f"lower:tmin0:{('below', 'eps', 'eps_up', 'above')[i]}")
            shoot(t, EPS, FLT_MAX, f"lower:tmin_eps:{('below', 'eps', 'eps_up', 'above')[i]}")
        for t_min in (F(1e-4), F(0.5)):
            for i, t in enumerate(around(t_min)):
                shoot(t, t_min, FLT_MAX, f"lower:tmin{float(t_min):g}:{('below', 'at', 'above')[i]}")
        for t_max in (F(1.0), F(2.5)):
            for i, t in enumerate(around(t_max)):
                shoot(t, T_MIN, t_max, f"upper:tmax{float(t_max):g}:{('below', 'at', 'above')[i]}")
        shoot(F(1.0), F(1.0), F(1.0), "pinched:tmin==t==tmax")
    s.fillers(11)
    return s.finish()


def ties_set(kind, reverse=False, big=False):
    """Coincident primitives - the reference keeps the one it visits first - and primitives one ulp of t apart.  The big
    primitives A (three times), the small B and, in the mixed and quad scenes, the quad C all lie in
    the plane z = 0 and share the corner (0, 0); their centroids differ, so the tree can put them into different leaves and visit
    them in another order than they were loaded.  `reverse` loads the same scene back to front."""
    s = EdgeSet("ties_rev" if reverse else "ties", kind, big)
    big = {TRI: UNIT_TRI * F(8), QUAD: UNIT_QUAD * F(8)}
    small = {TRI: UNIT_TRI * F(2), QUAD: UNIT_QUAD * F(2)}
    main = QUAD if kind == "quad" else TRI
    over = {"tri": TRI, "quad": QUAD, "mixed": QUAD}[kind]
    s.prim(main, big[main]); s.prim(main, big[main]); s.prim(main, big[main])
    s.prim(over, UNIT_QUAD * F(4) if over == QUAD else UNIT_TRI * F(4))
    s.prim(main, small[main])
    for pname, x, y in (("all", 0.5, 0.5), ("all_b", 0.25, 1.0), ("big_and_over", 1.5, 1.0), ("big_only", 1.0, 5.0), ("corner", 0, 0)):
        s.ray((x, y, -1), (0, 0, 1), f"tie:{pname}:up", -1, tree_matters=True)
        s.ray((x, y, 1), (0, 0, -1), f"tie:{pname}:down", -1, tree_matters=True)
        s.ray((x - OBLIQUE[0], y - OBLIQUE[1], -1), OBLIQUE, f"tie:{pname}:oblique", -1, tree_matters=True)
    # one ulp of t: t = 1 exactly on the first, 1 + 2^-23 on the farther, 1 - 2^-24 on the nearer (exact: the planes are dyadic)
    shape = UNIT_TRI if main == TRI else UNIT_QUAD
    x, y = INTERIOR["tri" if main == TRI else "quad"]
    for pname, z, y0 in (("farther", F(2.0 ** -23), 16), ("nearer", F(-2.0 ** -24), 24)):
        for first_then in ((0.0, z), (z, 0.0)):
            a = s.prim(main, shape, (0, y0, first_then[0])); b = s.prim(main, shape, (0, y0, first_then[1]))
            want = a if (first_then[0] < first_then[1]) else b
            s.ray((x, F(y0) + y, -1), (0, 0, 1), f"ulp:{pname}:{'plane_first' if first_then[0] == 0 else 'plane_second'}", want)
            y0 += 4
    s.fillers(9, first=(16, 0, 0), step=(4, 0, 0))
    return s.finish(reverse)


SLAB_BASE = F(64)           # 1e-6 is less than half an ulp of 64: the boxes' planes ARE the vertex coordinates
TINY = [("+0", F(0.0)), ("-0", F(-0.0)), ("2^-101", F(2.0 ** -101)), ("2^-100", F(2.0 ** -100)), ("-2^-100", F(-2.0 ** -100)),
        ("denormal", F(1e-40)), ("-denormal", F(-1e-40))]


def slab_set(kind, big=False):
    """The slab test's own edges, on tilted primitives (v0, v0 + x, v0 + y + z: thick boxes) at coordinates around 64, where the
    1e-6 by which the reference widens a box is rounded away: a box's planes are exactly its primitives' extreme coordinates, so a
    ray in a face plane, along a box edge or through a box corner can still hit a primitive there.  For the ray from (x, y, z)
    relative to v0 along +z:  u = x, v = y, t = y - z."""
    s = EdgeSet("slab", kind, big, big_at=(24, 24, 64))
    B = SLAB_BASE
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 1]], F); quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 1], [0, 1, 1]], F)
    kinds = {"tri": (TRI,), "quad": (QUAD,), "mixed": (TRI, QUAD)}[kind]
    prims = []
    for k in range(12):
        pk = kinds[k % len(kinds)]
        prims.append((pk, s.prim(pk, tri if pk == TRI else quad, (B + F(2 * k), B, B)), B + F(2 * k)))
    for pk, idx, X in (prims[0], prims[5], prims[6], prims[11]):
        name = "tri" if pk == TRI else "quad"
        def shoot(rel, d, label, t_min=T_MIN, t_max=FLT_MAX):
            s.ray((X + F(rel[0]), B + F(rel[1]), B + F(rel[2])), d, f"{name}:slab:p{idx}:{label}", idx, t_min, t_max)
        for zname, z in TINY[:2]:
            # the origin on a face, the matching direction component a zero of either sign: 0 * inf
            shoot((0, 0.5, -1), (z, 0, 1), f"face_x_lo:{zname}")            # in the plane of the edge u == 0
            shoot((1, 0, -1), (z, 0, 1), f"face_x_hi:{zname}")              # through v1: u == 1
            shoot((0.25, 0, -1), (0, z, 1), f"face_y_lo:{zname}")           # in the plane of the edge v == 0
            shoot((0, 1, -1), (0, z, 1), f"face_y_hi:{zname}")              # through the top corner
            shoot((-1, 0.5, 0), (1, 0, z), f"face_z_lo:{zname}")            # in the bottom plane, along x: parallel to edge1
            shoot((0.25, -1, 1), (0, 1, z), f"face_z_hi:{zname}")           # in the top plane, along y
            # in two face planes at once: along a box edge
            shoot((1, 0, -1), (z, z, 1), f"edge_xhi_ylo:{zname}")
            shoot((0, 1, -1), (z, -z, 1), f"edge_xlo_yhi:{zname}")
        # through a box corner: the x slab is entered where the z slab is left, tmin_box == tmax_box, and one float either side
        for i, oz in enumerate(around(B)):
            s.ray((X - F(1), B + F(1), oz), (1, 0, 1), f"{name}:slab:p{idx}:corner:{('below', 'at', 'above')[i]}", idx)
        # a box entered exactly at closest_t (t_max), and t_min exactly at a box's exit; the vertex v0 + y + z is hit AT the exit
        for i, t in enumerate(around(1.0)):
            shoot((0.25, 0.5, -1), (0, 0, 1), f"enter_at_closest:{('below', 'at', 'above')[i]}", t_max=t)
        for i, t in enumerate(around(2.0)):
            shoot((0.25, 0.5, -1), (0, 0, 1), f"tmin_at_exit:{('below', 'at', 'above')[i]}", t_min=t)
            shoot((0, 1, -1), (0, 0, 1), f"tmin_at_exit_vertex:{('below', 'at', 'above')[i]}", t_min=t)
        # each direction component tiny in turn
        for zname, z in TINY:
            shoot((0.25, 0.5, -1), (z, 0, 1), f"tiny_dx:{zname}")
            shoot((0.25, 0.5, -1), (0, z, 1), f"tiny_dy:{zname}")
            shoot((0.25, -1, 0.5), (0, 1, z), f"tiny_dz:{zname}")
            shoot((0.25, -1, 0.5), (z, 1, z), f"tiny_dxdz:{zname}")
    return s.finish()


def planar_set(kind, big=False):
    """A planar scene at z = 64: every box of the tree has zero thickness, so every hit has tmin_box == tmax_box in z."""
    s = EdgeSet("planar", kind, big, big_at=(24, 24, 64))
    B = SLAB_BASE
    kinds = {"tri": (TRI,), "quad": (QUAD,), "mixed": (TRI, QUAD)}[kind]
    for k in range(12):
        pk = kinds[k % len(kinds)]
        idx = s.prim(pk, UNIT_TRI if pk == TRI else UNIT_QUAD, (B + F(2 * k), B, B))
        name = "tri" if pk == TRI else "quad"
        x, y = INTERIOR[name]
        X = B + F(2 * k)
        s.ray((X + x, B + y, B - 1), (0, 0, 1), f"{name}:planar:p{idx}:up", idx)
        s.ray((X + x, B + y, B + 1), (0, 0, -1), f"{name}:planar:p{idx}:down", idx)
        s.ray((X + x - OBLIQUE[0], B + y - OBLIQUE[1], B - 1), OBLIQUE, f"{name}:planar:p{idx}:oblique", idx)
        s.ray((X, B, B - 1), (0, 0, 1), f"{name}:planar:p{idx}:corner", idx)                       # along a box edge, through v0
        s.ray((X - 1, B + y, B), (1, 0, 0), f"{name}:planar:p{idx}:in_plane", idx)                  # lies in the plane: a == 0
        s.ray((X + x, B + y, B), (0, 0, 1), f"{name}:planar:p{idx}:from_the_plane", idx)            # t == 0
    return s.finish()


def nonfinite_set(kind, big=False):
    """A NaN and an infinite direction component, a NaN origin: no answer but the oracle's, and no fault."""
    s = EdgeSet("nonfinite", kind, big)
    nan = F(np.nan)
    for name, k, idx, y0 in _targets(s):
        x, y = INTERIOR[name]
        for a in range(3):
            for vname, val in (("nan", nan), ("+inf", INF), ("-inf", -INF)):
                d = [F(0.25), F(-0.5), F(1.0)]; d[a] = val
                s.ray((x, y0 + y, -1), d, f"{name}:nonfinite:d{a}:{vname}", idx)
                d = [F(0), F(0), F(1.0)] if a != 2 else [F(0), F(1.0), F(0)]; d[a] = val
                s.ray((x, y0 + y, -1), d, f"{name}:nonfinite:axis_d{a}:{vname}", idx)
            o = [x, y0 + y, F(-1)]; o[a] = nan
            s.ray(o, (0, 0, 1), f"{name}:nonfinite:o{a}:nan", idx)
            o = [x, y0 + y, F(-1)]; o[a] = INF
            s.ray(o, (0, 0, 1), f"{name}:nonfinite:o{a}:inf", idx)
        s.ray((x, y0 + y, -1), (0, 0, 1), f"{name}:nonfinite:control", idx)
    s.fillers(11)
    return s.finish()


def origins_set(kind, big=False):
    """The same few rays from ever farther away: o = p - 2^k d for a vertex, an edge point and an interior point, t = 2^k exactly.
    The certified walk sends origins beyond its guard (four times the scale of the scene) through the reference's walk: the
    distances straddle that limit for every scene here."""
    s = EdgeSet("origins", kind, big)
    for name, k, idx, y0 in _targets(s):
        x, y = INTERIOR[name]
        for pname, px, py in (("vertex", F(0), F(0)), ("edge", F(0.5), F(0)), ("inside", x, y)):
            for e in range(0, 22):
                dist = F(2.0 ** e)
                s.ray((px, y0 + py, -dist), (0, 0, 1), f"{name}:origin:{pname}:up:2^{e}", idx)
                s.ray((px - dist, y0 + py, -dist), (1, 0, 1), f"{name}:origin:{pname}:diagonal:2^{e}", idx)
    s.fillers(11)
    return s.finish()


BIG_E = F(2.0 ** 59)        # an edge just under the 1e18 of the host's check
BIG_S = F(2.0 ** 69)        # |o - v0|: BIG_E * BIG_S == 2^128 overflows
SHORT_E = F(2.0 ** -10)     # the other edge: BIG_E * BIG_S * SHORT_E stays finite


def extent_set(kind, big=False, S=BIG_S, name="extent"):
    """At the host's extent check: edge1 = (e, 0, 0) with e = 2^-10, edge2 = (E, E, 0) with E = 2^59, d = -+(1, 1, -1) and
    o - v0 = +-(S, S, -S) with S = 2^69.  h = d x edge2 = (-+E, +-E, 0), so dot(s, h) is (-inf) + (+inf) = NaN while a = -e E,
    q = (0, -+S e, -+S e), v and t = S stay finite: the ray passes exactly through the vertex v0 (v == 0), or through the middle of
    edge2 (v == 0.5).  Triangle::intersect lets the NaN u through (u < 0 || u > 1 is false) and accepts; Quad::intersect
    (u >= 0 && u <= 1) rejects.  `near` is the same ray from S / 4, where nothing overflows: u == 0 and both accept.  With edge1
    the long edge instead (q_nan), q overflows to NaN, t is NaN and both reject.  The primitives are stacked 4 S apart in z, the
    mirrored ones below the others: a NaN u makes a primitive accept rays far outside its box (the verdict is left to v and t), and
    in this order v < 0 or t < 0 for every ray on every primitive but its own, so that the tree and the linear pass agree."""
    s = EdgeSet(name, kind, big)
    E, e = BIG_E, SHORT_E
    row = 0
    for sign in (1, -1):
        sg = F(sign)
        for name, k in (("tri", TRI), ("quad", QUAD)):
            if kind not in (name, "mixed"):
                continue
            for which in ("u_nan", "q_nan"):
                z0 = sg * F(row) * F(4) * S; row += 1
                short, long_ = [sg * e, 0, 0], [sg * E, sg * E, 0]
                v1, v2 = (short, long_) if which == "u_nan" else (long_, short)
                shape = [[0, 0, 0], v1, v2] if k == TRI else [[0, 0, 0], v1, v2, [0, sg * E, 0]]
                idx = s.prim(k, shape, (0, 0, z0))
                mirror = "plus" if sign > 0 else "minus"
                for far, dist in (("far", S), ("near", S / F(4))):
                    s.ray((sg * dist, sg * dist, z0 - sg * dist), (-sg, -sg, sg), f"{name}:extent:{which}:vertex:{far}:{mirror}", idx)
                    s.ray((sg * (dist + E / 2), sg * (dist + E / 2), z0 - sg * dist), (-sg, -sg, sg),
                          f"{name}:extent:{which}:edge_mid:{far}:{mirror}", idx)
    s.fillers(5, first=(0, 0, F(64) * S), step=(0, 0, F(4) * S))
    return s.finish()


# The host refuses a scene with quads whose largest quad edge times its extent exceeds 2^124 (SceneState::checkExtent): the
# scenes of extent_set reach 84 S in z.  S = 2^58 lies inside the bound (and nothing overflows: u is a number, both kinds accept),
# S = 2^59 outside it, S = 2^69 where the products overflow.
EXTENT_IN, EXTENT_OUT = F(2.0 ** 58), F(2.0 ** 59)
QUAD_REACH_BOUND = 2.0 ** 124


def quad_reach_product(s, origin=None):
    """largest quad edge x reach of the scene (of `origin` from the scene), as SceneState::checkExtent / checkQuadOrigin form it"""
    lo = np.full(3, np.inf); hi = np.full(3, -np.inf); edge = 0.0
    for k in range(len(s.types)):
        v = s.verts[k][: 3 if s.types[k] == TRI else 4]
        lo = np.minimum(lo, v.min(0).astype(np.float64)); hi = np.maximum(hi, v.max(0).astype(np.float64))
        if s.types[k] == QUAD:
            edge = max(edge, float(np.abs((v - v[0]).astype(F)).max()))
    o = lo if origin is None else np.asarray(origin, F).astype(np.float64)
    far = max(np.abs(o - lo).max(), np.abs(o - hi).max())
    coord = max(np.abs(o).max(), np.abs(lo).max(), np.abs(hi).max())
    return edge * (far + coord * 2.0 ** -20)


BUILDERS = dict(barycentric=barycentric_set, determinant=determinant_set, bounds=bounds_set, ties=ties_set,
                ties_rev=lambda kind, big=False: ties_set(kind, True, big), origins=origins_set, slab=slab_set, planar=planar_set, nonfinite=nonfinite_set, extent=extent_set,
                extent_in=lambda kind, big=False: extent_set(kind, big, EXTENT_IN, "extent_in"),
                extent_out=lambda kind, big=False: extent_set(kind, big, EXTENT_OUT, "extent_out"))
_cache = {}


def edge_set(name, kind, big=False):
    """the set `name` over the scene of `kind` (built once, read-only); big: the same with 128 more primitives away from the rays"""
    if (name, kind, big) not in _cache:
        _cache[(name, kind, big)] = BUILDERS[name](kind, big=big)
    return _cache[(name, kind, big)]


def all_sets():
    return [(name, kind) for name in BUILDERS for kind in KINDS]


# ------------------------------------------------------------------------------------------------
# wave placement
# ------------------------------------------------------------------------------------------------
def wave_companions(s, i, leaf_box):
    """For ray i of set s, aimed at primitive k: (rejecter, hitter) - a ray that enters the box of k's leaf and fails the (a, u)
    stage of k, and one that passes it, both with i's direction where that is axis-aligned and finite.  leaf_box: (bmin, bmax) of
    the leaf that holds k.  rejecter is None where the leaf's box holds no such ray (the leaf is the primitive)."""
    k = s.target[i]
    kind, verts = s.types[k], s.verts[k]
    d = s.d[i]
    axis_z = np.isfinite(d).all() and d[0] == 0 and d[1] == 0 and d[2] != 0
    d = d if axis_z else np.array([0, 0, 1], F)
    oz = s.o[i][2] if axis_z and np.isfinite(s.o[i][2]) else verts[0][2] - d[2]
    bmin, bmax = leaf_box
    x, y = INTERIOR["tri" if kind == TRI else "quad"]
    e1, e2 = verts[1] - verts[0], verts[(2 if kind == TRI else 3)] - verts[0]
    hitter = np.array([verts[0][0] + x * e1[0] + y * e2[0], verts[0][1] + x * e1[1] + y * e2[1], oz], F)
    if not passes_a_u(kind, verts, hitter, d):
        hitter = None
    rejecter = None
    for fx in (0.5, 0.25, 0.75, 0.125, 0.875, 0.0625, 0.9375):
        for fy in (0.5, 0.25, 0.75):
            c = np.array([bmin[0] + F(fx) * (bmax[0] - bmin[0]), bmin[1] + F(fy) * (bmax[1] - bmin[1]), oz], F)
            if slab_verdict(bmin, bmax, c, d, 0.0, FLT_MAX)[0] and not passes_a_u(kind, verts, c, d):
                rejecter = c
                break
        if rejecter is not None:
            break
    return (None if rejecter is None else (rejecter, d)), (None if hitter is None else (hitter, d))


# ------------------------------------------------------------------------------------------------
# the oracle's answers, computed once per set and shared read-only
# ------------------------------------------------------------------------------------------------
_answers = {}


def oracle_scene(name, kind, big=False):
    from oracle_binding import OracleScene
    key = (name, kind, big, "scene")
    if key not in _answers:
        _answers[key] = OracleScene.from_arrays(*edge_set(name, kind, big).scene)
    return _answers[key]


def answers_for(scene, o, d, t_min, t_max, use_bvh=True):
    """OracleScene.intersect per ray: dict(hit, prim, t, p, n) of arrays"""
    n = len(o)
    out = dict(hit=np.zeros(n, np.int32), prim=np.full(n, -1, np.int32), t=np.zeros(n, F), p=np.zeros((n, 3), F), n=np.zeros((n, 3), F))
    for i in range(n):
        h = scene.intersect(o[i], d[i], float(t_min[i]), float(t_max[i]), use_bvh)
        out["hit"][i], out["prim"][i] = h.hit, h.prim
        if h.hit:
            out["t"][i] = h.t; out["p"][i] = list(h.p); out["n"][i] = list(h.n)
    return out


def oracle_answers(name, kind, use_bvh=True, big=False):
    key = (name, kind, big, bool(use_bvh))
    if key not in _answers:
        s = edge_set(name, kind, big)
        a = answers_for(oracle_scene(name, kind, big), s.o, s.d, s.t_min, s.t_max, use_bvh)
        for v in a.values():
            v.setflags(write=False)
        _answers[key] = a
    return _answers[key]
