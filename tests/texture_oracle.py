"""CPU restatement of the albedo texture (include/ptmi.h: "albedo texture"), written from the header in numpy float32: the UV of
one vertex, the texel under both filters, Kd(p) = Kd_k * T, and the per-lane estimator with it - TexturedRenderer is PathRenderer
(tests/path_oracle.py) with ONE change, the colour its hits report.  The change is a mixin over _intersect, so it composes with
SmoothRenderer's override of the same method (TexturedSmoothRenderer)."""
import numpy as np

from nee_oracle import FLT_MAX, f32
from path_oracle import PathRenderer
from smooth_oracle import SmoothRenderer, _half, _valid

ZERO, ONE, HALF = f32(0.0), f32(1.0), f32(0.5)
NEAREST, BILINEAR = 0, 1
FILTERS = {"nearest": NEAREST, "bilinear": BILINEAR, 0: NEAREST, 1: BILINEAR}


def _weights(r1, r2):
    """the clamped weights (b0, b1, b2) of "vertex normals" """
    b1 = ZERO if r1 < 0 else (ONE if r1 > 1 else r1)
    m = f32(ONE - b1)
    b2 = ZERO if r2 < 0 else (m if r2 > m else r2)
    return f32(m - b2), f32(b1), f32(b2)


def wrap(u):
    """s = u - floorf(u), pinned into [0, 1): 1.0 and a NaN become 0"""
    with np.errstate(all="ignore"):
        u = f32(u)
        s = f32(u - f32(np.floor(u)))
        return s if (s >= 0 and s < 1) else ZERO


def raw_uv(prims, uv, k, p):
    """(u, v) of load-order primitive k at the point p BEFORE the wrap.  prims: dict(type, verts); uv (n_prims, 4, 2)."""
    c = np.asarray(uv[k], f32)
    quad = prims["type"][k] == 1
    with np.errstate(all="ignore"):
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
            return f32(c[0][0]), f32(c[0][1])
        b0, b1, b2 = _weights(r1, r2)
        out = []
        for a in range(2):
            out.append(f32(f32(f32(b0 * corner[0][a]) + f32(b1 * corner[1][a])) + f32(b2 * corner[2][a])))
    return out[0], out[1]


def uv_at(prims, uv, k, p):
    """the wrapped (s_u, s_v) of load-order primitive k at the point p"""
    u, v = raw_uv(prims, uv, k, p)
    return wrap(u), wrap(v)


def _axis_nearest(s, n):
    i = int(f32(s * f32(n)))
    return min(i, n - 1)


def _axis_bilinear(s, n):
    x = f32(f32(s * f32(n)) - HALF)
    x0 = f32(np.floor(x))
    fx = f32(x - x0)
    i0 = int(x0); i1 = i0 + 1
    if i0 < 0:
        i0 = n - 1
    if i1 > n - 1:
        i1 = 0
    return i0, i1, fx


def texel(image, filter, s_u, s_v):
    """T (3,) float32 of the image (h, w, 3) at the wrapped coordinates"""
    image = np.asarray(image, f32)
    h, w = image.shape[:2]
    s_u, s_v = f32(s_u), f32(s_v)
    if FILTERS[filter] == NEAREST:
        return image[_axis_nearest(s_v, h), _axis_nearest(s_u, w)].copy()
    i0, i1, fx = _axis_bilinear(s_u, w)
    j0, j1, fy = _axis_bilinear(s_v, h)
    gx, gy = f32(ONE - fx), f32(ONE - fy)
    a = ((gx * image[j0, i0]).astype(f32) + (fx * image[j0, i1]).astype(f32)).astype(f32)
    b = ((gx * image[j1, i0]).astype(f32) + (fx * image[j1, i1]).astype(f32)).astype(f32)
    return ((gy * a).astype(f32) + (fy * b).astype(f32)).astype(f32)


def make_table(image, uv, textured=None, filter="bilinear"):
    """the table albedo() and the renderers take: dict(image, uv, textured (n_prims,) bool, filter 0 / 1)"""
    uv = np.ascontiguousarray(uv, f32)
    mask = np.ones(len(uv), bool) if textured is None else np.asarray(textured) != 0
    return dict(image=np.ascontiguousarray(image, f32), uv=uv, textured=mask, filter=FILTERS[filter])


def lookup(prims, table, k, p):
    """(s_u, s_v, T, textured) as ptmi_debug_albedo reports them: (0, 0, ones, False) for an untextured primitive"""
    if not table["textured"][k]:
        return ZERO, ZERO, np.ones(3, f32), False
    s_u, s_v = uv_at(prims, table["uv"], k, p)
    return s_u, s_v, texel(table["image"], table["filter"], s_u, s_v), True


def albedo(prims, table, k, p):
    """Kd(p) = Kd_k * T of load-order primitive k at the point p; Kd_k untouched for an untextured primitive.  prims has bsdf."""
    kd = np.asarray(prims["bsdf"][k], f32).copy()
    _, _, T, textured = lookup(prims, table, k, p)
    return (kd * T).astype(f32) if textured else kd


class TextureMixin:
    """ONE change over the renderer it is mixed into: a hit on a textured primitive reports Kd_k * T as its colour.  image, uv,
    textured and filter are keyword arguments; everything else goes on to the next class."""

    def __init__(self, *args, image, uv, textured=None, filter="bilinear", **kw):
        super().__init__(*args, **kw)
        self.texture = make_table(image, uv, textured, filter)
        if len(self.texture["uv"]) != len(self.prims["type"]):
            raise ValueError("uv does not match the scene")

    def _intersect(self, o, d):
        h = super()._intersect(o, d)
        if h.hit and self.texture["textured"][h.prim]:
            s_u, s_v = uv_at(self.prims, self.texture["uv"], h.prim, np.array(h.p, f32))
            T = texel(self.texture["image"], self.texture["filter"], s_u, s_v)
            kd = (np.array(h.bsdf, f32) * T).astype(f32)
            h.bsdf[:] = [float(x) for x in kd]
        return h


class TexturedRenderer(TextureMixin, PathRenderer):
    """PathRenderer over a scene with an albedo texture (the kernel's TEX)"""


class TexturedSmoothRenderer(TextureMixin, SmoothRenderer):
    """SmoothRenderer (the vertex-normal table is its 5th positional argument) with an albedo texture: SMOOTH and TEX together"""
