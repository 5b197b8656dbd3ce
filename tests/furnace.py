"""White-furnace scenes for next-event estimation (include/ptmi.h, "next-event estimation") - no GPU needed to build them.

Every primitive a ray can reach has the same Le and the same Kd = rho, and the scene is closed, so every pixel's expected value,
for the reference's estimator and for NEE alike, is Le_c * (1 - rho_c^D) / (1 - rho_c) per channel at max_depth = D: the
camera hits at depths 0 .. D-1 each add rho^depth * Le, whatever the geometry inside.  Russian roulette (depth > 2) and MIS keep
that expectation, and with rho <= 0.7 and D <= 12 the |beta| < 1e-5 exit cannot trigger.  At D <= 3 there is no roulette yet, so
the reference's estimator returns exactly that value on every sample.

The outer box is [-HALF, HALF]^3 around the default camera (0.5, 3, 8.5); its walls reach past each other at the edges, so that
no ray finds a crack.  Geometric normals of the box point along +axis on both walls of an axis: seen from inside, one wall of
each pair faces the camera and the other faces away.
"""
import os

import numpy as np

F = np.float32
RHO = (0.3, 0.5, 0.7)
LE = (1.0, 0.75, 0.5)
HALF = 20.0
CAMERA = (0.5, 3.0, 8.5)


def expected(depth, rho=RHO, le=LE):
    """the analytic pixel value per channel at max_depth = depth (float64)"""
    rho = np.asarray(rho, np.float64); le = np.asarray(le, np.float64)
    return le * (1.0 - rho ** depth) / (1.0 - rho)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


class Scene:
    """Primitives in load order: (types, verts, normal, bsdf, Le) arrays for load_scene_arrays.  Every primitive gets RHO and LE
    unless told otherwise; the stored normal is the geometric one unless given."""

    def __init__(self, rho=RHO, le=LE):
        self.rho, self.le = rho, le
        self.t, self.v, self.n, self.b, self.e = [], [], [], [], []

    def tri(self, a, b, c, normal=None, le=None):
        a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
        self.t.append(0); self.v.append([a, b, c, np.zeros(3)])
        self.n.append(_unit(np.cross(b - a, c - a)) if normal is None else _unit(normal))
        self.b.append(self.rho); self.e.append(self.le if le is None else le)

    def quad(self, v00, v10, v11, v01, normal=None, le=None):
        v00, v10, v11, v01 = (np.asarray(x, np.float64) for x in (v00, v10, v11, v01))
        self.t.append(1); self.v.append([v00, v10, v11, v01])
        self.n.append(_unit(np.cross(v10 - v00, v01 - v00)) if normal is None else _unit(normal))
        self.b.append(self.rho); self.e.append(self.le if le is None else le)

    def __len__(self):
        return len(self.t)

    def arrays(self):
        return (np.array(self.t, np.int32), np.array(self.v, F), np.array(self.n, F), np.array(self.b, F), np.array(self.e, F))

    def write_obj(self, directory, name="furnace"):
        """The scene as name.obj + name.mtl (one material; the stored normal as every face's vn): the .obj loader's path"""
        assert len(set(map(tuple, np.asarray(self.e, np.float64)))) == 1, "one material only"
        obj, mtl = os.path.join(directory, name + ".obj"), os.path.join(directory, name + ".mtl")
        with open(mtl, "w") as f:
            f.write("newmtl furnace\nKd %r %r %r\nKe %r %r %r\n" % (tuple(map(float, self.rho)) + tuple(map(float, self.e[0]))))
        lines = [f"mtllib {name}.mtl", "usemtl furnace"]
        k = 0
        for p, (t, v, n) in enumerate(zip(self.t, self.v, self.n)):
            m = 4 if t == 1 else 3
            lines += ["v %r %r %r" % tuple(map(float, F(v[i]))) for i in range(m)]
            lines.append("vn %r %r %r" % tuple(map(float, F(n))))
            lines.append("f " + " ".join(f"{k + i + 1}//{p + 1}" for i in range(m)))
            k += m
        with open(obj, "w") as f:
            f.write("\n".join(lines) + "\n")
        return obj


def box(s, quads=False, tilt_deg=0.0, half=HALF):
    """The six walls, extended by 1 past each other; tilt_deg tilts every wall's stored normal towards one in-plane axis, on the
    geometric normal's side"""
    h, g = half, half + 1.0
    for a in range(3):
        u, w = (a + 1) % 3, (a + 2) % 3
        for side in (-1.0, 1.0):
            def p(du, dw):
                x = np.zeros(3); x[a] = side * h; x[u] = du * g; x[w] = dw * g
                return x
            nrm = np.zeros(3); nrm[a] = 1.0                       # cross(e_u, e_w) = +e_a
            tan = np.zeros(3); tan[u] = 1.0
            th = np.radians(tilt_deg)
            stored = np.cos(th) * nrm + np.sin(th) * tan if tilt_deg else None
            if quads:
                s.quad(p(-1, -1), p(1, -1), p(1, 1), p(-1, 1), normal=stored)
            else:
                s.tri(p(-1, -1), p(1, -1), p(1, 1), normal=stored)
                s.tri(p(-1, -1), p(1, 1), p(-1, 1), normal=stored)
    return s


def _random_tris(s, rng, n, size=(1.0, 4.0), spread=14.0):
    for _ in range(n):
        c = rng.uniform(-spread, spread, 3)
        r = rng.uniform(*size)
        s.tri(*(c + rng.normal(0, r, (3, 3))))


def _random_quads(s, rng, n, size=(1.0, 4.0), spread=14.0):
    """planar quads: parallelograms v00, v00 + a, v00 + a + b, v00 + b"""
    for _ in range(n):
        c = rng.uniform(-spread, spread, 3)
        r = rng.uniform(*size)
        a, b = rng.normal(0, r, (2, 3))
        s.quad(c, c + a, c + a + b, c + b)


def _chain(s, n=100, quads=False, x0=1.0e9):
    """test_gpu_parity's deep-tree geometry, moved out of the box: centroids at x0 + 2^90 * 2.2^-i make the midpoint split peel
    one primitive per level (tree depth 76).  The box splits off some 50 levels down, above the reference's 62-entry stack limit,
    and no member of the chain can be reached from inside."""
    x = (x0 + 2.0 ** 90 * 2.2 ** (-np.arange(n, dtype=np.float64))).astype(F)
    for i in range(n):
        z = float(F(i) * F(0.01))
        a, b, c = [x[i], -0.004, z], [x[i], 0.004, z], [x[i], 0.0, z + 0.008]
        if quads:
            s.quad(a, b, [x[i], 0.004, z + 0.008], [x[i], -0.004, z + 0.008], normal=(1, 0, 0))
        else:
            s.tri(a, b, c, normal=(1, 0, 0))


def variant(name, seed=1):
    """A furnace variant of the NEE expectation tests, as a furnace.Scene"""
    rng = np.random.default_rng(seed)
    s = Scene()
    if name == "tris":                               # a: <= 64 triangles (the lane walk)
        box(s); _random_tris(s, rng, 40)
    elif name == "quads":                            # b: <= 64 planar quads
        box(s, quads=True); _random_quads(s, rng, 40)
    elif name == "tris_many":                        # c: > 64 triangles (the certified walk)
        box(s); _random_tris(s, rng, 300)
    elif name == "quads_many":                       # c: > 64 quads (the certified walk)
        box(s, quads=True); _random_quads(s, rng, 300)
    elif name == "emitters_4k":                      # d: > 4 096 emitters of unequal area; a few dozen tiny ones are absorbed
        box(s)
        inner = Scene(); _random_tris(inner, rng, 2900, size=(0.02, 1.5), spread=17.0)
        for k in range(len(inner)):                  # every other one has a 4x larger twin outside the box: sampled, never seen
            a, b, c = inner.v[k][:3]
            s.tri(a, b, c)
            if k % 2:
                s.tri(*(2.0 * (x - a) + a + (3 * HALF, 0.0, 0.0) for x in (a, b, c)))
    elif name == "deep":                             # e: a tree deeper than 62 levels (the stack walk)
        box(s); _chain(s)
    elif name == "deep_quads":
        box(s, quads=True); _chain(s, quads=True)
    elif name == "declined":                         # f: the 8-wide builder declines (a coordinate of 2e9), far outside the box
        box(s); _random_tris(s, rng, 100)
        s.tri((30.0, 0.0, 0.0), (30.0, 1.0, 0.0), (2.0e9, 1.0, -3.0), le=(0.0, 0.0, 0.0))
    elif name == "panels":                           # g: thin two-sided panels seen from both sides
        box(s)
        for k in range(6):
            ang = k * np.pi / 6
            d = np.array([np.cos(ang), 0.35 * (k % 3 - 1), np.sin(ang)])
            c = np.array([0.5 * (k - 2.5), 1.0 + 0.5 * k, -3.0 - 1.5 * k])
            up = np.array([0.0, 1.0, 0.0])
            e = np.cross(d, up)
            s.tri(c - 6 * d - 6 * up, c + 6 * d - 6 * up, c + 6 * up + e)
    elif name == "tilted":                           # h: stored normals of the walls tilted 30 degrees (all the power)
        box(s, tilt_deg=30.0)
    elif name == "tilted_mixed":                     # h: every wall triangle's stored normal tilted 10 .. 40 degrees, two directions
        box(s)
        th = np.radians(rng.uniform(10.0, 40.0, len(s)))
        for k in range(len(s)):                      # box(): 4 triangles per axis, geometric normal +axis
            ng = np.zeros(3); ng[k // 4] = 1.0
            tan = np.zeros(3); tan[(k // 4 + 1 + k % 2) % 3] = 1.0
            s.n[k] = _unit(np.cos(th[k]) * ng + np.sin(th[k]) * tan)
    elif name == "warped":                           # i: one non-planar interior emitter quad
        box(s)
        s.quad((-12.0, -10.0, -12.0), (12.0, -10.0, -12.0), (12.0, 12.0, 4.0), (-12.0, 12.0, -12.0))
    else:
        raise KeyError(name)
    return s


VARIANTS = ["tris", "quads", "tris_many", "quads_many", "emitters_4k", "deep", "deep_quads", "declined", "panels", "tilted",
            "tilted_mixed", "warped"]
# the variants whose stored normals are not the plane normal: the reference's estimator leaves the box after a self-hit (a spawn
# point on the wrong side), so the analytic value holds only at max_depth <= 2
TILTED = ("tilted", "tilted_mixed", "tilted_obj")


def load_pair(name, tmpdir=None, seed=1):
    """(arrays or obj path, Scene) of a variant; "tilted_obj" is "tilted" written as .obj + .mtl into tmpdir (the loader path)"""
    if name == "tilted_obj":
        s = variant("tilted", seed)
        return s.write_obj(str(tmpdir)), s
    s = variant(name, seed)
    return s.arrays(), s
