"""Input sets of the per-call tests of the next-event kernel's light and surface sampling functions (ptmi_debug_nee_call).

Every set is a seeded random bulk plus edges constructed exactly - by bit pattern or by searching the restatement's own float32
arithmetic where a decimal would miss them - and has a length that is no multiple of 256.  tests/test_nee_call_sets_host.py
asserts that the edges are present and reach every exit; tests/test_gpu_nee_per_call.py runs the sets on the device.  The sets
that depend on a table (environment, emitters) take the restatement's table.
"""
import os

import numpy as np

import nee_oracle as NO
import rough_oracle as RO
import specular_oracle as SO
from oracle_binding import SCENES, OracleScene

F = np.float32
SMALLEST = F(2.0 ** -33)                   # the smallest uniform the generator returns (curand_uniform: x * 2^-32 + 2^-33)
TINY_NORMAL = F(1.17549435e-38)
FLT_MAX = F(3.4028234663852886e38)
DENORM_MIN = F(1.4e-45)
NAN = F(np.nan)


def bits(u):
    return np.array([u], np.uint32).view(F)[0]


def up(x, k=1):
    x = F(x)
    for _ in range(k):
        x = np.nextafter(x, F(np.inf))
    return x


def down(x, k=1):
    x = F(x)
    for _ in range(k):
        x = np.nextafter(x, F(-np.inf))
    return x


def around(x):
    return [down(x), F(x), up(x)]


def ragged(a):
    """the set as float32 rows, one row dropped where the length is a multiple of 256"""
    a = np.ascontiguousarray(a, F)
    if len(a) % 256 == 0:
        a = a[:-1]
    return a


def uniforms(rng, shape):
    """(0, 1] float32, as the generator's"""
    return np.maximum(F(1.0) - rng.random(shape, F), SMALLEST).astype(F)


def unit_rows(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


# ------------------------------------------------------------------------------------------------
# environment
# ------------------------------------------------------------------------------------------------
ROTATIONS = (0.0, 77.7)                    # 77.7 / 360 is no dyadic fraction


def env_maps():
    """name -> rgb (height, width, 3); names are width x height"""
    rng = np.random.default_rng(41)
    one = np.ones((1, 1, 3), F)
    col = rng.uniform(0.2, 3.0, (7, 1, 3)).astype(F)
    row = rng.uniform(0.2, 3.0, (1, 8, 3)).astype(F)
    holes = np.zeros((3, 5, 3), F)
    holes[0, :, 0] = [1.0, 0.0, 0.0, 2.0, 0.5]            # a zero run inside a row
    holes[0, :, 1] = [0.5, 0.0, 0.0, 0.0, 0.25]
    holes[2, :, 2] = [0.0, 3.0, 1.0, 0.0, 0.0]            # a row that begins and ends with zeros; row 1 is all zero
    hot = np.full((32, 64, 3), 0.01, F)
    hot[9, 41] = 5000.0
    return {"1x1": one, "1x7": col, "8x1": row, "5x3_holes": holes, "64x32_hot": hot}


def env_lookup_set(tab, seed=1):
    """directions d (n, 3) for texel(d)"""
    rng = np.random.default_rng(seed)
    z = tab["z"]; w = tab["row_cdf"].shape[1]; rot = float(tab["rot"])
    rows = [unit_rows(rng, 1500), unit_rows(rng, 200) * F(1e-3), unit_rows(rng, 200) * F(250.0)]
    edge = []
    ys = [F(1.0), F(-1.0), down(1.0), up(-1.0), up(1.0), down(-1.0), F(1.5), F(-1.5), F(1e30), F(-1e30), F(0.0), F(-0.0)]
    for r in range(len(z)):
        ys += around(z[r])
    for y in ys:
        for _ in range(3):
            a = rng.uniform(0, 2 * np.pi)
            edge.append([np.cos(a), y, np.sin(a)])
    for y in (1.0, -1.0, 0.3, -0.3, 0.0):                 # the pole's axis, and the seam from either side
        edge += [[0.0, y, 0.0], [-0.0, y, 0.0], [0.0, y, -0.0], [-0.0, y, -0.0]]
        edge += [[-1.0, y, 0.0], [-1.0, y, -0.0], [-1e-30, y, 0.0], [-1e-30, y, -0.0], [-3.0, y, 1e-38], [-3.0, y, -1e-38]]
        edge += [[1.0, y, 0.0], [1.0, y, -0.0]]
        for dz in (-1e-45, -1e-30, -1e-10, -1e-8, -2.9e-8, -3e-8, -5.9e-8, -6e-8, -1.2e-7, 1e-45, 1e-10):   # t at the float below 1, and t - floor(t) = 1
            edge.append([1.0, y, dz])
    for k in range(w + 1):                                # t * w on an integer: phi = 2 pi (k / w + rot), and directions next to it
        phi = 2.0 * np.pi * (k / w + rot)
        for e in (0.0, 1e-7, -1e-7, 3e-7, -3e-7, 1e-6, -1e-6):
            for y in (0.0, 0.5):
                edge.append([np.cos(phi + e), y, np.sin(phi + e)])
        c, s = F(np.cos(phi)), F(np.sin(phi))
        for dc in (down(c), up(c)):
            edge.append([dc, 0.25, s])
        for ds in (down(s), up(s)):
            edge.append([c, 0.25, ds])
    return ragged(np.concatenate(rows + [np.array(edge, np.float64).astype(F)]))


def env_sample_set(tab, seed=2):
    """(r1, r2, r3, r4) rows for the environment's light sample"""
    rng = np.random.default_rng(seed)
    m = tab["marginal_cdf"]; c = tab["row_cdf"]; h, w = c.shape
    rows = [uniforms(rng, (2000, 4))]
    edge = []
    ok = lambda u: F(0.0) < u <= F(1.0)
    for r in range(h):                                    # r1 on every stored entry of the marginal and next to it
        for u in around(m[r]):
            if ok(u):
                for _ in range(2):
                    edge.append([u] + list(uniforms(rng, 3)))
    for r in range(h):                                    # r2 on every stored entry of every row and next to it; r1 selects the row
        if not ok(m[r]) or (r > 0 and m[r] == m[r - 1]):
            continue                                      # a row of weight 0 is never selected
        for j in range(w):
            for u in around(c[r, j]):
                if ok(u):
                    edge.append([m[r], u] + list(uniforms(rng, 2)))
            if ok(c[r, j]):
                edge.append([uniforms(rng, 1)[0], c[r, j]] + list(uniforms(rng, 2)))
    for r1 in (SMALLEST, F(1.0)):
        for r2 in (SMALLEST, F(1.0)):
            for r3 in (SMALLEST, F(0.5), F(1.0)):
                for r4 in (SMALLEST, F(0.5), F(1.0)):
                    edge.append([r1, r2, r3, r4])
    return ragged(np.concatenate(rows + [np.array(edge, F)]))


# ------------------------------------------------------------------------------------------------
# emitters
# ------------------------------------------------------------------------------------------------
def array_scene():
    """Twelve axis-aligned triangles on a grid of eighths (so that areas and translations are exact), five of them emitters of
    very uneven power, two of equal power (4 and 7: one triangle translated); emitter 10 has a vertex in the origin and little
    power, so that a vertex can stand 1e-20 from a sampled point and p_l underflows.  Arrays for load_scene_arrays."""
    n = 12
    types = np.zeros(n, np.int32)
    verts = np.zeros((n, 4, 3), F)
    for i in range(n):
        z = F(i // 4) * F(0.5) + F(0.25)
        x, y = F(i % 4) * F(0.5) - F(1.0), F(i % 3) * F(0.375) - F(0.5)
        verts[i, 0] = [x, y, z]; verts[i, 1] = [x + F(0.375), y, z]; verts[i, 2] = [x, y + F(0.25), z]
    verts[7, :3] = verts[4, :3] + np.array([0.25, 0.5, 1.0], F)        # exact: the same triangle elsewhere
    verts[10, 0] = [0.5, 0.0, 0.0]; verts[10, 1] = [0.0, 0.75, 0.0]; verts[10, 2] = [0.0, 0.0, 0.0]
    verts[2, :3] = verts[2, :3][:, [2, 0, 1]]                          # an emitter in a plane x = const
    normal = np.tile(F([0, 0, 1]), (n, 1)); normal[2] = [1, 0, 0]
    bsdf = np.full((n, 3), 0.6, F)
    Le = np.zeros((n, 3), F)
    Le[2] = [1000.0, 200.0, 0.5]; Le[4] = [4.0, 4.0, 4.0]; Le[7] = [4.0, 4.0, 4.0]; Le[9] = [0.0, 3.0, 0.0]; Le[10] = [0.01, 0.0, 0.0]
    return types, verts, normal, bsdf, Le


def emitter_scenes():
    """name -> (how a Renderer loads it, the OracleScene)"""
    out = {}
    for name in ("cbox", "cbox_quads"):
        path = os.path.join(SCENES, name + ".obj")
        out[name] = (("file", path), OracleScene.load(path))
    arrays = array_scene()
    out["array"] = (("arrays", arrays), OracleScene.from_arrays(*arrays))
    return out


class EmitterTable:
    """the restatement's emitter table of a scene, with what the per-call restatement needs"""

    def __init__(self, oscene):
        self.s = oscene
        self.prim, self.cdf, self.pdf_area, self.total = NO.emitter_table(oscene, with_total=True)
        self.ng = NO.geometric_normals(oscene)
        self.verts = oscene.prims()["verts"]

    def point(self, j, r1, r2):
        yv = np.zeros(3, F)
        NO.lib().po_prim_sample_uniform(self.s.h, int(self.prim[j]), F(r1), F(r2), yv.ctypes.data)
        return yv


def emitter_set(et, seed=3):
    """(u_sel, r1, r2, o2) rows; o2 is placed relative to the point the row's own (u_sel, r1, r2) samples"""
    rng = np.random.default_rng(seed)
    ne = len(et.prim)
    lo, hi = et.verts.min(axis=(0, 1)), et.verts.max(axis=(0, 1))
    rows = []
    n_bulk = 2500
    u = uniforms(rng, (n_bulk, 3))
    o2 = (lo + rng.random((n_bulk, 3)) * (hi - lo)).astype(F)
    rows.append(np.concatenate([u, o2], axis=1))
    edge = []
    ends = [F(0.0)] + [F(cj / et.total) for cj in et.cdf]
    usel = [F(1.0), SMALLEST]
    for j in range(ne):
        usel += [x for x in around(ends[j + 1]) if F(0.0) < x <= F(1.0)]
    for x in usel:
        for _ in range(4):
            edge.append([x] + list(uniforms(rng, 2)) + list((lo + rng.random(3) * (hi - lo)).astype(F)))
    for j in range(ne):                                   # every record, and around each selected point
        a, b = float(ends[j]), float(ends[j + 1])
        ng = et.ng[et.prim[j]]
        ax_n = int(np.argmax(np.abs(ng))); ax_t = (ax_n + 1) % 3
        for k in range(40 * max(1, 4 // ne)):              # at least 20 cases of each kind below in every scene
            us = F(a + (b - a) * (0.1 + 0.8 * rng.random()))
            r1, r2 = uniforms(rng, 2)
            if k % 8 == 7:
                r1, r2 = F(1.0), F(1.0)                   # the point is the record's third vertex, exactly
            yv = et.point(j, r1, r2)
            t = np.zeros(3, F); t[ax_t] = 1.0
            nn = np.zeros(3, F); nn[ax_n] = 1.0
            kind = k % 8
            if kind == 0:
                o = (lo + rng.random(3) * (hi - lo)).astype(F)
            elif kind == 1:                               # on the emitter's plane (its normal is an axis): cos_l == 0
                o = yv.copy(); o[ax_t] += F(0.3 + rng.random()); o[(ax_n + 2) % 3] -= F(rng.random())
            elif kind == 2:                               # on the sampled point: dist2 == 0
                o = yv.copy()
            elif kind == 3:                               # 1e19 away, nearly in the plane: dist2 stays finite, p_l overflows
                o = (yv + F(1e19) * t + F(1e19 * 10.0 ** -rng.integers(8, 12)) * nn).astype(F)
            elif kind == 4:                               # 2e19 and more away: dist2 overflows to inf
                o = (yv + F(2e19) * (t + nn)).astype(F)
            elif kind == 5:                               # 1e19 away along the normal: a large finite p_l
                o = (yv + F(1e19) * nn).astype(F)
            elif kind == 6:                               # 1e-4 off the plane, the offset of a vertex on the emitter's neighbour
                o = (yv + F(1e-4) * nn + F(0.05) * t).astype(F)
            else:                                         # the third vertex: 1e-20 from it where it is the origin (dist2 subnormal),
                o = (yv + F(1e-20) * (nn + t)).astype(F)  # else the point itself
                if k % 16 == 15:
                    o = (yv + F(10.0 ** -rng.integers(21, 24)) * nn).astype(F)
            edge.append([us, r1, r2] + list(o))
        if not et.verts[et.prim[j], 2].any():             # the third vertex is the origin: points 1e-21 .. 1e-22 from it, where
            for _ in range(30):                           # dist2 is subnormal and pdf_area * dist2 underflows to 0
                us = F(a + (b - a) * (0.1 + 0.8 * rng.random()))
                o = (F(10.0 ** -rng.uniform(21.0, 22.2)) * (nn + F(rng.random()) * t)).astype(F)
                edge.append([us, F(1.0), F(1.0)] + list(o))
    return ragged(np.concatenate(rows + [np.array(edge, F)]))


# ------------------------------------------------------------------------------------------------
# mirror and glass
# ------------------------------------------------------------------------------------------------
IOR_ABOVE_ONE = up(1.0)
IORS = (F(1.0), F(1.5), F(8.0), IOR_ABOVE_ONE)
Y = np.array([0.0, 1.0, 0.0], F)


def s2_of(eta, ci):
    """the float32 s2 of the header for (eta, ci)"""
    eta, ci = F(eta), F(ci)
    return F(F(eta * eta) * max(F(0.0), F(F(1.0) - F(ci * ci))))


def critical_ci(ior):
    """the largest float ci with s2 >= 1 inside a body of index ior (s2 does not grow with ci)"""
    a, b = F(0.0).view(np.uint32), F(1.0).view(np.uint32)            # s2(a) >= 1 > s2(b): bisect the bit patterns
    assert s2_of(ior, 0.0) >= 1 > s2_of(ior, 1.0)
    while b - a > 1:
        mid = np.uint32((int(a) + int(b)) // 2)
        if s2_of(ior, bits(mid)) >= 1:
            a = mid
        else:
            b = mid
    return bits(a)


def inside(ci, phi=0.0):
    """a direction leaving a body whose stored normal is +y (it travels along the normal) with cosine of incidence ci exactly"""
    s = np.sqrt(max(0.0, 1.0 - float(ci) ** 2))
    return [s * np.cos(phi), F(ci), s * np.sin(phi)]


def outside(ci, phi=0.0):
    s = np.sqrt(max(0.0, 1.0 - float(ci) ** 2))
    return [s * np.cos(phi), -F(ci), s * np.sin(phi)]


def specular_set(seed=4):
    """(d, stored normal, kind, ior, u) rows"""
    rng = np.random.default_rng(seed)
    rows = []

    def add(d, n, kind, ior, u):
        rows.append(list(np.asarray(d, np.float64).astype(F)) + list(np.asarray(n, np.float64).astype(F)) + [F(kind), F(ior), F(u)])

    def fresnel_of(d, n, ior):
        d = np.asarray(d, np.float64).astype(F); n = np.asarray(n, np.float64).astype(F)
        with np.errstate(all="ignore"):
            _, eta, ci = SO.interface(d, n, F(ior))
            return SO.fresnel(eta, ci)[0]

    # bulk: mirrors; glass refracting, glass reflecting by the draw, total internal reflection, ior 1
    for d, n in zip(unit_rows(rng, 1500), unit_rows(rng, 1500)):
        add(d, n, SO.MIRROR, 1.5, uniforms(rng, 1)[0])
    iors = [F(1.5), F(8.0), F(1.33), F(2.4), IOR_ABOVE_ONE]
    for k, (d, n) in enumerate(zip(unit_rows(rng, 4200), unit_rows(rng, 4200))):
        ior = iors[k % 4] if k % 50 else iors[4]
        f = fresnel_of(d, n, ior)
        if k % 2:                                          # u <= F: reflected by the draw (where F > 0)
            add(d, n, SO.GLASS, ior, max(F(f * F(rng.random())), SMALLEST))
        else:
            add(d, n, SO.GLASS, ior, uniforms(rng, 1)[0])
    for k in range(1500):                                  # beyond the critical angle, inside the body
        ior = (F(1.5), F(8.0), F(1.33))[k % 3]
        cc = float(critical_ci(ior))
        add(inside(cc * rng.random() * 0.98, rng.uniform(0, 2 * np.pi)), Y, SO.GLASS, ior, uniforms(rng, 1)[0])
    for k, (d, n) in enumerate(zip(unit_rows(rng, 400), unit_rows(rng, 400))):
        add(d, n, SO.GLASS, 1.0, uniforms(rng, 1)[0] if k % 2 else SMALLEST)
    # edges
    tilted = np.array([0.3, 0.9, -0.2])
    for kind in (SO.MIRROR, SO.GLASS):
        for ior in IORS:
            for n in (Y, tilted / np.linalg.norm(tilted)):
                n = np.asarray(n, np.float64)
                for sgn in (-1.0, 1.0):                    # normal incidence from either side
                    for u in (SMALLEST, F(0.04), F(1.0)):
                        add(sgn * n.astype(F).astype(np.float64), n, kind, ior, u)
            for e in range(0, 46):                         # ci down to the smallest positive float, from either side
                ci = F(10.0 ** -e) if e < 45 else DENORM_MIN
                for u in (SMALLEST, F(1.0)):
                    add(outside(ci), Y, kind, ior, u)
                    add(inside(ci), Y, kind, ior, u)
            for length in (1e-18, 1e18, 1e-30, 1e20, 0.0):   # stored normals of any length, tilted; the zero normal
                for n in (Y, tilted):
                    for d in (outside(0.8, 1.0), inside(0.9, 2.0)):
                        add(d, np.asarray(n, np.float64) * length, kind, ior, F(0.5))
    for ior in (F(1.5), F(8.0), F(1.33), F(2.4), IOR_ABOVE_ONE):       # around asin(1 / ior): the float ci where s2 first reaches 1
        cc = critical_ci(ior)
        for k in range(-6, 7):
            ci = up(cc, k) if k >= 0 else down(cc, -k)
            for u in (SMALLEST, F(0.5), F(1.0)):
                add(inside(ci), Y, SO.GLASS, ior, u)
                add([0.0, ci, np.sqrt(max(0.0, 1.0 - float(ci) ** 2))], Y, SO.GLASS, ior, u)
    for d, n in zip(unit_rows(rng, 300), unit_rows(rng, 300)):         # u on the restated F and next to it
        ior = iors[int(rng.integers(0, 4))]
        f = fresnel_of(d, n, ior)
        for u in around(f):
            if F(0.0) < u <= F(1.0):
                add(d, n, SO.GLASS, ior, u)
    for e in range(0, 12):
        for ior in (F(1.5), F(8.0)):
            d = outside(F(10.0 ** (-e / 3.0)))
            for u in around(fresnel_of(d, Y, ior)):
                if F(0.0) < u <= F(1.0):
                    add(d, Y, SO.GLASS, ior, u)
    return ragged(np.array(rows, F))


# ------------------------------------------------------------------------------------------------
# rough metal
# ------------------------------------------------------------------------------------------------
ALPHAS = (F(0.05), F(0.25), F(0.5), F(1.0), F(0.0025))
Z = np.array([0.0, 0.0, 1.0], F)
CO_SWEEP = np.concatenate([[1.0, 0.999, 0.9, 0.5, 0.1], 10.0 ** -np.arange(2.0, 18.5, 0.5)]).astype(F)


def co_around_min_cos2():
    """floats c around sqrt(1e-37): f32(c * c) just above and just below PTMI_ROUGH_MIN_COS2"""
    c0 = F(np.sqrt(1e-37))
    cs = [down(c0, k) for k in range(8, 0, -1)] + [c0] + [up(c0, k) for k in range(1, 9)]
    sq = [F(c * c) > RO.MIN_COS2 for c in cs]
    assert not sq[0] and sq[-1]
    return cs


def incidence(co, phi=0.0):
    """d arriving at a vertex of normal +z with cos(theta_o) = co exactly"""
    so = np.sqrt(max(0.0, 1.0 - float(co) ** 2))
    return [-so * np.cos(phi), -so * np.sin(phi), -F(co)]


def near_minus_z():
    """unit normals with n.z = -1 and within a few floats of -0.9999999f, on either side"""
    out = [[0.0, 0.0, -1.0]]
    for k in range(1, 6):
        z = float(up(-1.0, k))
        x = np.sqrt(1.0 - z * z)
        out += [[x, 0.0, z], [0.0, -x, z], [x * 0.6, x * 0.8, z]]
    return out


def rough_vertices(rng, n_bulk):
    """(sn, d, alpha) rows: the bulk, the edges of the vertex, what fails the grazing test, NaN"""
    rows = []
    sn = unit_rows(rng, n_bulk); d = unit_rows(rng, n_bulk)
    up_z = np.arange(n_bulk) % 10 < 9
    sn[up_z, 2] = np.abs(sn[up_z, 2])                      # most of the bulk away from the frame's pole at -z
    flip = (np.einsum("ij,ij->i", sn, d) > 0)
    d[flip] = -d[flip]                                     # sn is turned against d
    scale = np.where(rng.random(n_bulk) < 0.2, 10.0 ** rng.uniform(-3, 3, n_bulk), 1.0).astype(F)
    for i in range(n_bulk):
        rows.append(list(sn[i] * scale[i]) + list(d[i]) + [ALPHAS[i % len(ALPHAS)]])
    for alpha in ALPHAS:
        for co in list(CO_SWEEP) + co_around_min_cos2():
            rows.append(list(Z) + incidence(co) + [alpha])
            rows.append(list(Z) + incidence(co, 2.1) + [alpha])
        rows.append(list(Z) + [0.0, 0.0, -1.0] + [alpha])                  # d = -un: lensq == 0
        rows.append([0.0, 2.0, 0.0] + [0.0, -1.0, 0.0] + [alpha])
        for n in near_minus_z():
            nn = np.asarray(n, np.float64)
            rows.append(list(nn) + list(-nn) + [alpha])                    # and d = -un in the other frame branch
            rows.append(list(nn) + [0.3, 0.1, 0.9] + [alpha])
    k = 0
    while k < 260:                                         # the grazing exit: co tiny, zero or negative
        alpha = ALPHAS[k % len(ALPHAS)]
        co = (-1.0) ** (k % 3 == 0) * 10.0 ** -rng.uniform(19, 40) if k % 5 else 0.0
        if k % 7 == 0:
            co = -rng.random()
        rows.append(list(Z) + incidence(co, rng.uniform(0, 6.28)) + [alpha])
        k += 1
    for k in range(260):                                   # a NaN co
        dd = list(unit_rows(rng, 1)[0]); dd[k % 3] = NAN
        if k % 4 == 0:
            dd = [0.6, 0.0, NAN]
        rows.append(list(Z if k % 2 else unit_rows(rng, 1)[0]) + dd + [ALPHAS[k % len(ALPHAS)]])
    return rows


def rough_vertex_set(seed=5):
    return ragged(np.array(rough_vertices(np.random.default_rng(seed), 3000), F))


def _world(v, wl):
    """the unit world direction along local wl in vertex v's frame (binary64 is enough: these are inputs)"""
    wl = np.asarray(wl, np.float64) / np.linalg.norm(wl)
    return wl[0] * v.T.astype(np.float64) + wl[1] * v.B.astype(np.float64) + wl[2] * v.un.astype(np.float64)


def rough_eval_set(seed=6):
    """(sn, d, alpha, wi) rows"""
    rng = np.random.default_rng(seed)
    rows = []
    n_bulk = 7000
    for k, base in enumerate(rough_vertices(rng, n_bulk)):
        b = np.array(base, F)
        with np.errstate(all="ignore"):
            v = RO.Vertex(b[0:3], b[3:6], b[6])
        wis = []
        if np.isfinite(v.wo).all() and np.isfinite(v.un).all():
            wo = v.wo.astype(np.float64)
            if k >= n_bulk or k % 2 == 0:
                wis.append(_world(v, np.array([-wo[0], -wo[1], wo[2]])))   # the mirror direction: h = un, the lobe's peak
            if k % 6 == 0:
                wis.append(_world(v, np.array([np.cos(k), np.sin(k), 0.0])))                  # at the horizon
            if k % 6 == 1:
                wis.append(_world(v, np.array([0.6 * np.cos(k), 0.6 * np.sin(k), -0.8])))     # below it
            if k % 12 == 2:
                wis.append(_world(v, np.array([np.cos(k), np.sin(k), 10.0 ** -rng.uniform(0, 25)])))   # just above it
        w = unit_rows(rng, 1)[0].astype(np.float64)
        if np.isfinite(v.un).all() and w @ v.un.astype(np.float64) < 0 and k % 4:
            w = -w
        if np.isfinite(v.un).all() and k % 10 < 9:         # most of the bulk clear of the horizon
            mu = rng.uniform(0.06, 1.0); ph = rng.uniform(0, 2 * np.pi)
            w = _world(v, np.array([np.sqrt(1 - mu * mu) * np.cos(ph), np.sqrt(1 - mu * mu) * np.sin(ph), mu]))
        if k < n_bulk or not wis:
            wis.append(w)
        if k % 29 == 0:
            wis.append([NAN, 0.5, 0.5])
        for wi in wis:
            rows.append(list(b) + list(np.asarray(wi, np.float64).astype(F)))
    return ragged(np.array(rows, F))


def rough_sample_set(seed=7):
    """(sn, d, alpha, u1, u2) rows"""
    rng = np.random.default_rng(seed)
    rows = []
    for k, base in enumerate(rough_vertices(rng, 6500)):
        u = uniforms(rng, 2)
        rows.append(base + [u[0], u[1]])
        if k % 6 == 0:
            for u1 in (SMALLEST, F(1.0)):
                for u2 in (SMALLEST, F(0.25), F(0.5), F(1.0)):
                    rows.append(base + [u1, u2])
    for k in range(300):                                   # wide lobes at grazing incidence: many samples go below the horizon
        co = 10.0 ** -rng.uniform(0.7, 3.0)
        u = uniforms(rng, 2)
        rows.append(list(Z) + incidence(co, rng.uniform(0, 6.28)) + [(F(1.0), F(0.5))[k % 2], u[0], u[1]])
    return ragged(np.array(rows, F))


def light_weight_set(seed=8):
    """(rough, sn, d, alpha, wi, cos_s, p) rows"""
    rng = np.random.default_rng(seed)
    ev = rough_eval_set(seed)
    pick = np.flatnonzero((np.arange(len(ev)) % 2 == 0) | np.isnan(ev).any(axis=1))
    rows = []
    ps = (TINY_NORMAL, F(1.0), FLT_MAX)
    for k, i in enumerate(pick):
        b = ev[i]
        with np.errstate(all="ignore"):
            cos_s = NO._dot(b[0:3], b[7:10])
        p = F(10.0 ** rng.uniform(-6, 6))
        rows.append([F(k % 4 != 0)] + list(b) + [cos_s, p])
        if k % 25 == 0:
            for pp in ps:
                for cs in (DENORM_MIN, F(1.0)):
                    for rough in (0.0, 1.0):
                        rows.append([F(rough)] + list(b) + [cs, pp])
    return ragged(np.array(rows, F))
