"""CPU restatement of next-event estimation with MIS (include/ptmi.h, "next-event estimation"), written from the header.

Every float operation is float32 in the order the header writes it; the pieces the header takes from the reference - the
closest hit, Primitive::sampleUniform, sampleCosineHemisphere, misPowerHeuristic, area, the camera ray, the RNG, the tone map -
come from the CPU oracle (oracle/ptmi_oracle.c) through ctypes.  The function types are declared here; oracle_binding.py
supplies the scene handles and the library path only.
"""
import ctypes as C

import numpy as np

from oracle_binding import ORACLE_SO, CameraFrame, Hit

f32 = np.float32
FLT_MAX = 3.4028234663852886e38

_L = None


def lib():
    global _L
    if _L is None:
        L = C.CDLL(ORACLE_SO)
        vp, f = C.c_void_p, C.c_float
        L.po_prim_geometry.argtypes = [vp, C.c_int, C.POINTER(f), vp]; L.po_prim_geometry.restype = None
        L.po_prim_sample_uniform.argtypes = [vp, C.c_int, f, f, vp]; L.po_prim_sample_uniform.restype = None
        L.po_sample_cosine_hemisphere.argtypes = [vp, f, f, vp]; L.po_sample_cosine_hemisphere.restype = None
        L.po_mis_power_heuristic.argtypes = [f, f]; L.po_mis_power_heuristic.restype = f
        L.po_intersect.argtypes = [vp, vp, vp, f, f, C.c_int, C.POINTER(Hit)]; L.po_intersect.restype = None
        L.po_rng_init.argtypes = [C.c_uint64, C.c_uint64, vp]; L.po_rng_init.restype = None
        L.po_rng_uniform.argtypes = [vp]; L.po_rng_uniform.restype = f
        L.po_camera_frame_setup.argtypes = [vp, C.c_int, C.c_int, C.POINTER(CameraFrame)]; L.po_camera_frame_setup.restype = None
        L.po_camera_ray.argtypes = [C.POINTER(CameraFrame), f, f, vp, vp]; L.po_camera_ray.restype = None
        L.po_average.argtypes = [vp, C.c_int, vp]; L.po_average.restype = None
        L.po_tonemap.argtypes = [vp, vp]; L.po_tonemap.restype = None
        _L = L
    return _L


def areas(oscene):
    """Triangle/Quad::area of every primitive, load order (po_prim_geometry)"""
    L = lib()
    out = np.zeros(oscene.n_prims, f32)
    a = C.c_float(); cen = np.zeros(3, f32)
    for i in range(oscene.n_prims):
        L.po_prim_geometry(oscene.h, i, C.byref(a), cen.ctypes.data)
        out[i] = a.value
    return out


def geometric_normals(oscene):
    """ng of every primitive, load order: unit_vector(cross(e1, e2)) of the triangle's (v1 - v0, v2 - v0), the quad's
    (v10 - v00, v01 - v00), float32 as pt_vec.h (NaN or 0 where the edges are degenerate)"""
    p = oscene.prims()
    v = p["verts"]
    e1 = v[:, 1] - v[:, 0]
    e2 = np.where((p["type"] == 1)[:, None], v[:, 3], v[:, 2]) - v[:, 0]
    with np.errstate(all="ignore"):
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], -(e1[:, 0] * e2[:, 2] - e1[:, 2] * e2[:, 0]),
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(f32)
        ln = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]).astype(f32)
        k = (f32(1.0) / ln).astype(f32)
        return (c * k[:, None]).astype(f32)


def planar(verts, ng):
    """a quad is an emitter only if |dot(ng, v11 - v00)| <= 1e-4f * length(v11 - v00), float32"""
    dg = (verts[2] - verts[0]).astype(f32)
    with np.errstate(all="ignore"):
        return bool(abs(_dot(ng, dg)) <= f32(f32(1e-4) * f32(np.sqrt(_dot(dg, dg)))))


def emitter_table(oscene, with_total=False):
    """The emitter table of the header: (prim, cdf, pdf_area), in the order written.  Float32 running sums over the candidates
    that skip an absorbed weight, pdf_area = (w / total) / area; where a weight or the sum overflows float, the same in binary64,
    cdf = (float)(C_j / total) skipping entries that round to the one before (total 1).  with_total: also the total."""
    p = oscene.prims()
    le = p["Le"]
    area = areas(oscene)
    ng = geometric_normals(oscene)
    cand = [i for i in range(oscene.n_prims)
            if np.isfinite(ng[i]).all() and not (p["type"][i] == 1 and not planar(p["verts"][i], ng[i]))]
    prim, cdf, ws = [], [], []
    pdf_area = np.zeros(oscene.n_prims, f32)
    c = f32(0.0)
    overflow = False
    with np.errstate(all="ignore"):
        for i in cand:
            w = f32(area[i] * f32(f32(le[i, 0] + le[i, 1]) + le[i, 2]))
            if not w > 0:
                continue
            if not (w <= FLT_MAX and f32(c + w) <= FLT_MAX):
                overflow = True
                break
            if not f32(c + w) > c:
                continue
            c = f32(c + w)
            prim.append(i); cdf.append(c); ws.append(w)
    if not overflow:
        total = c
        for j, i in enumerate(prim):
            pdf_area[i] = f32(f32(ws[j] / total) / area[i])
    else:
        prim, cdf = [], []
        pos, wd, cd = [], [], []
        t = 0.0
        for i in cand:
            w = float(area[i]) * ((float(le[i, 0]) + float(le[i, 1])) + float(le[i, 2]))
            if not (w > 0 and np.isfinite(w)):
                continue
            t = t + w
            pos.append(i); wd.append(w); cd.append(t)
        prev = f32(0.0)
        for i, w, ci in zip(pos, wd, cd):
            cj = f32(ci / t)
            if not cj > prev:
                continue
            pdf_area[i] = f32((w / t) / float(area[i]))
            prim.append(i); cdf.append(cj)
            prev = cj
        total = f32(1.0) if prim else f32(0.0)
    out = (np.array(prim, np.int32), np.array(cdf, f32), pdf_area)
    return out + (total,) if with_total else out


def _dot(a, b):
    p = a * b
    return f32(f32(p[0] + p[1]) + p[2])


def _over_pi(x):
    return f32(np.float64(x) / np.pi)


def _unit(v):
    k = f32(f32(1.0) / f32(np.sqrt(_dot(v, v))))
    return v * k


def select(cdf, total, u_sel):
    """the emitter u_sel selects: the smallest j with u_sel * total <= cdf[j]"""
    return min(int(np.searchsorted(cdf, f32(u_sel * total), side="left")), len(cdf) - 1)


def emitter_sample(oscene, i, ng_i, pdf_area_i, r1, r2, o2, omq=None):
    """The light sample towards primitive i (load order) from o2: (wi, dist2, cos_l, p_l, p_l scaled), p_l the area density turned
    into one per solid angle, scaled by omq where the environment is a light too (omq None: p_l itself)"""
    yv = np.zeros(3, f32)
    lib().po_prim_sample_uniform(oscene.h, int(i), r1, r2, yv.ctypes.data)
    with np.errstate(all="ignore"):
        vv = (yv - o2).astype(f32)
        dist2 = _dot(vv, vv)
        dist = f32(np.sqrt(dist2))
        wi = (vv / dist).astype(f32)
        cos_l = abs(_dot(ng_i, wi))
        p_l = f32(f32(pdf_area_i * dist2) / cos_l)
        p_s = p_l if omq is None else f32(omq * p_l)
    return wi, dist2, cos_l, p_l, p_s


def sample_counts(cos_l, p_l):
    """the guards of a light sample on an emitter: seen edge on, or a p_l of 0 or inf, it weighs 0"""
    return bool(cos_l > 0 and 0 < p_l <= FLT_MAX)


class NeeRenderer:
    """Frames of the NEE estimator over an OracleScene with persistent per-pixel streams (as a ptmi context keeps them)."""

    def __init__(self, oscene, cam, width, height, seed_base=2023):
        L = lib()
        self.s, self.w, self.h = oscene, width, height
        self.prims = oscene.prims()
        self.prim, self.cdf, self.pdf_area, self.total = emitter_table(oscene, with_total=True)
        self.ng = geometric_normals(oscene)
        self.cf = CameraFrame()
        L.po_camera_frame_setup(C.byref(cam), width, height, C.byref(self.cf))
        self.rng = np.zeros((height * width, 6), np.uint32)
        for pix in range(height * width):
            L.po_rng_init(seed_base + pix, pix, self.rng[pix].ctypes.data)
        self.hit = Hit()
        self.vec = np.zeros(3, f32)

    def _u(self, st):
        return f32(lib().po_rng_uniform(st.ctypes.data))

    def _intersect(self, o, d):
        lib().po_intersect(self.s.h, o.ctypes.data, d.ctypes.data, 1e-4, FLT_MAX, 1, C.byref(self.hit))
        return self.hit

    def sample(self, x, y, st, max_depth):
        L = lib()
        u = f32(f32(f32(x) + self._u(st)) / f32(self.w))
        v = f32(f32(f32(y) + self._u(st)) / f32(self.h))
        o = np.zeros(3, f32); d = np.zeros(3, f32)
        L.po_camera_ray(C.byref(self.cf), u, v, o.ctypes.data, d.ctypes.data)
        tp = np.ones(3, f32); Lr = np.zeros(3, f32)
        pb_prev = f32(0.0)
        for depth in range(max_depth):
            h = self._intersect(o, d)
            if not h.hit:
                break
            k = h.prim
            n_k = np.array(h.n, f32); Le = np.array(h.Le, f32); kd = np.array(h.bsdf, f32)
            t = f32(h.t); p = np.array(h.p, f32)
            pa = self.pdf_area[k] if depth > 0 else f32(0.0)
            if pa > 0:
                p_l = f32(f32(pa * f32(t * t)) / abs(_dot(self.ng[k], d)))
                w = f32(L.po_mis_power_heuristic(pb_prev, p_l))
                Lr = Lr + (tp * Le) * w
            else:
                Lr = Lr + tp * Le
            if depth > 2:
                rr = min(max(tp[0], max(tp[1], tp[2])), f32(0.95))
                if self._u(st) > rr:
                    break
                tp = tp * f32(f32(1.0) / rr)
            tp = tp * kd
            if f32(np.sqrt(_dot(tp, tp))) < f32(1e-5):
                break
            sn = n_k if _dot(d, n_k) < 0 else -n_k
            o2 = p + f32(1e-4) * sn
            if depth + 1 < max_depth and len(self.prim):
                u_sel, r1, r2 = self._u(st), self._u(st), self._u(st)
                i = int(self.prim[select(self.cdf, self.total, u_sel)])
                wi, _, cos_l, _, p_l = emitter_sample(self.s, i, self.ng[i], self.pdf_area[i], r1, r2, o2)
                cos_s = _dot(sn, wi)
                if cos_s > 0 and sample_counts(cos_l, p_l):
                    hs = self._intersect(o2, wi)
                    if hs.hit and hs.prim == i:
                        p_b = _over_pi(cos_s)
                        w = f32(f32(p_b * f32(L.po_mis_power_heuristic(p_l, p_b))) / p_l)
                        Lr = Lr + (tp * self.prims["Le"][i].astype(f32)) * w
            uu, vw = self._u(st), self._u(st)
            if depth + 1 >= max_depth:
                break
            nxt = np.zeros(3, f32)
            L.po_sample_cosine_hemisphere(sn.ctypes.data, uu, vw, nxt.ctypes.data)
            pb_prev = _over_pi(max(_dot(sn, nxt), f32(0.0)))
            o = o2
            d = _unit(nxt)
        return Lr

    def sums(self, spp, max_depth, rows=None, color=None):
        """Colour sums of spp samples for every pixel of `rows` (default all; row 0 = bottom), going on from `color`"""
        rows = range(self.h) if rows is None else rows
        out = np.zeros((self.h, self.w, 3), f32) if color is None else color.copy()
        for y in rows:
            for x in range(self.w):
                st = self.rng[y * self.w + x]
                c = out[y, x].copy()
                for _ in range(spp):
                    c = c + self.sample(x, y, st, max_depth)
                out[y, x] = c
        return out

    @staticmethod
    def resolve(sums, spp):
        """mean -> Reinhard -> gamma -> 8 bit of a frame's resolve: (rgb8, radiance), each (rows, width, 3)"""
        L = lib()
        rad = np.zeros_like(sums); rgb = np.zeros(sums.shape, np.uint8)
        for idx in np.ndindex(sums.shape[:2]):
            s = np.ascontiguousarray(sums[idx], f32)
            L.po_average(s.ctypes.data, int(spp), rad[idx].ctypes.data)
            c = np.ascontiguousarray(rad[idx]); out = np.zeros(3, np.uint8)
            L.po_tonemap(c.ctypes.data, out.ctypes.data)
            rgb[idx] = out
        return rgb, rad

    def frame(self, spp, max_depth):
        """One frame (streams carry over to the next call): (rgb8, radiance), row 0 = bottom"""
        return self.resolve(self.sums(spp, max_depth), spp)
