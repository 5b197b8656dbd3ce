"""CPU restatement of next-event estimation with MIS (include/ptmi.h, "next-event estimation"), written from the header.

Every float operation is float32 in the order the header writes it; the pieces the header takes from the reference - the
closest hit, Primitive::sampleUniform, sampleCosineHemisphere, misPowerHeuristic, area, the camera ray, the RNG, the tone map -
come from the CPU oracle (oracle/ptmi_oracle.c) through ctypes.  The function types are declared here; oracle_binding.py
supplies the scene handles and the library path only.  The estimator that uses these pieces is tests/path_oracle.py's one path loop.
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
