"""CPU restatement of the vertex normals (include/ptmi.h: "vertex normals"), written from the header in numpy float32: the flat /
smooth classification, the interpolated normal of one vertex, and the per-lane estimator with it - SmoothRenderer is PathRenderer
(tests/path_oracle.py) with ONE change, the normal its hits report."""
import numpy as np

from nee_oracle import FLT_MAX, _dot, _unit, f32
from path_oracle import PathRenderer

ZERO, ONE = f32(0.0), f32(1.0)


def classify(prims, table):
    """(n_prims,) bool: smooth - a corner normal that is read differs (==, so -0.0 equals 0.0) from the stored normal"""
    table = np.asarray(table, f32)
    stored = np.asarray(prims["normal"], f32)
    out = np.zeros(len(stored), bool)
    for i in range(len(stored)):
        read = 4 if prims["type"][i] == 1 else 3
        with np.errstate(all="ignore"):
            out[i] = not bool((table[i, :read] == stored[i][None]).all())
    return out


def _valid(x):
    return bool(x > 0) and bool(x <= FLT_MAX)


def _half(ea, eb, w):
    """(den, r1, r2) of w over the edges (ea, eb)"""
    d00, d01, d11, d20, d21 = _dot(ea, ea), _dot(ea, eb), _dot(eb, eb), _dot(w, ea), _dot(w, eb)
    den = f32(f32(d00 * d11) - f32(d01 * d01))
    r1 = f32(f32(f32(d11 * d20) - f32(d01 * d21)) / den)
    r2 = f32(f32(f32(d00 * d21) - f32(d01 * d20)) / den)
    return den, r1, r2


def _blend(r1, r2, n0, na, nb):
    """the clamped weights' normal over (n0, na, nb), or None where the sum has no direction"""
    b1 = ZERO if r1 < 0 else (ONE if r1 > 1 else r1)
    m = f32(ONE - b1)
    b2 = ZERO if r2 < 0 else (m if r2 > m else r2)
    b0 = f32(m - b2)
    s = ((b0 * n0 + b1 * na).astype(f32) + b2 * nb).astype(f32)
    len2 = _dot(s, s)
    if not _valid(len2):
        return None
    return _unit(s).astype(f32)


def vertex_normal(prims, table, k, p):
    """(N, interpolated) of load-order primitive k at the point p: the contract of include/ptmi.h.  prims: dict(type, verts,
    normal); table (n_prims, 4, 3).  interpolated False: a flat primitive or a fallback, N is the stored normal untouched."""
    stored = np.asarray(prims["normal"][k], f32).copy()
    quad = prims["type"][k] == 1
    c = np.asarray(table[k], f32)
    read = 4 if quad else 3
    with np.errstate(all="ignore"):
        if bool((c[:read] == stored[None]).all()):
            return stored, False
        v = np.asarray(prims["verts"][k], f32)
        w = (np.asarray(p, f32) - v[0]).astype(f32)
        e1, e2 = (v[1] - v[0]).astype(f32), (v[2] - v[0]).astype(f32)
        den, r1, r2 = _half(e1, e2, w)
        if quad and not (_valid(den) and r1 >= 0):
            e3 = (v[3] - v[0]).astype(f32)
            den, r1, r2 = _half(e2, e3, w)
            corner = (c[0], c[2], c[3])
        else:
            corner = (c[0], c[1], c[2])
        if not _valid(den):
            return stored, False
        n = _blend(r1, r2, *corner)
    return (stored, False) if n is None else (n, True)


class SmoothRenderer(PathRenderer):
    """PathRenderer over a scene with a vertex-normal table (n_prims, 4, 3), load order (the kernel's SMOOTH): a hit on a smooth
    primitive reports the interpolated normal, and the loop reads it where it read the stored one."""

    def __init__(self, oscene, cam, width, height, table, **kw):
        super().__init__(oscene, cam, width, height, **kw)
        self.table = np.ascontiguousarray(table, f32)
        self.smooth = classify(self.prims, self.table)

    def _intersect(self, o, d):
        h = super()._intersect(o, d)
        if h.hit and self.smooth[h.prim]:
            n, _ = vertex_normal(self.prims, self.table, h.prim, np.array(h.p, f32))
            h.n[:] = [float(x) for x in n]
        return h
