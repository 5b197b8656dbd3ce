"""CPU restatement of the participating medium (include/ptmi.h: "participating medium"), written from the header in numpy float32:
the block, the segment, the transmittance, the free flight, the phase function, and the per-lane estimator with them.

MediumMixin overrides `sample` with the per-lane loop of tests/path_oracle.py plus the medium's steps - a second copy of that loop,
because the medium enters it in four places (after the walk, at the vertex, in the light sample's weight, at the shadow ray).
With the medium switched off inside (medium None: no draw, no vertex) the copy must give PathRenderer's sums and trace bit for
bit, and tests/test_medium_host.py pins exactly that.  The loop calls self._intersect throughout, so the mixin composes with
SmoothRenderer, TextureMixin and LensMixin.  log comes through po_math_batch op 2 and exp through po_expf, the host build of
include/ptmi_math.h."""
import ctypes as C

import numpy as np

from env_oracle import lookup, sample_direction, sincosf
from lens_oracle import LensMixin
from nee_oracle import FLT_MAX, _dot, _over_pi, _unit, emitter_sample, f32, lib, sample_counts, select
from oracle_binding import math_batch, oracle_lib
from path_oracle import EPS, ONE, PathRenderer
from rough_oracle import ROUGH, Vertex, frame as tangent_frame, light_weight, sample as rough_sample
from smooth_oracle import SmoothRenderer
from specular_oracle import GLASS, MIRROR, scatter, shading_normal
from texture_oracle import TexturedSmoothRenderer

MEDIUM = 4                                # the kind a medium vertex has in a trace
ZERO = f32(0.0)
INF = f32(np.inf)
MATH_LOG_D = 2                            # PTMI_MATH_LOG_D of po_math_batch


def medium_block(lo, hi, sigma_t, albedo=(1.0, 1.0, 1.0), g=0.0):
    """THE MEDIUM BLOCK (3, 4) float32: (lo, sigma_t) (hi, g) (albedo, 0)"""
    out = np.zeros((3, 4), f32)
    out[0, :3], out[0, 3] = np.asarray(lo, f32), f32(sigma_t)
    out[1, :3], out[1, 3] = np.asarray(hi, f32), f32(g)
    out[2, :3] = np.broadcast_to(np.asarray(albedo, f32), (3,))
    return out


def segment(block, o, d, t_end):
    """THE SEGMENT: (nonempty, t0, t1), t0 and t1 as the loop leaves them"""
    t0, t1 = ZERO, f32(t_end)
    inside = True
    with np.errstate(all="ignore"):
        for a in range(3):
            lo, hi, oa, da = block[0, a], block[1, a], f32(o[a]), f32(d[a])
            if da != 0:
                ta = f32(f32(lo - oa) / da)
                tb = f32(f32(hi - oa) / da)
                near, far = np.fmin(ta, tb), np.fmax(ta, tb)
                if near > t0:
                    t0 = near
                if far < t1:
                    t1 = far
            elif not (lo <= oa and oa <= hi):
                inside = False
        return bool(inside and t1 > t0), f32(t0), f32(t1)


def expf(x):
    return f32(oracle_lib().po_expf(C.c_float(float(x))))


def transmittance(block, o, d, t_end):
    """TRANSMITTANCE of the ray's segment; 1 exactly where it is empty"""
    ok, t0, t1 = segment(block, o, d, t_end)
    if not ok:
        return ONE
    with np.errstate(all="ignore"):
        return expf(f32(-f32(block[0, 3] * f32(t1 - t0))))


def flight(sigma_t, u_m):
    """s of the draw u_m"""
    ld = math_batch(MATH_LOG_D, np.array([u_m], f32))[0, 0]
    return f32(f32(-f32(ld)) / f32(sigma_t))


def free_flight(block, o, d, t_end, u_m):
    """FREE FLIGHT: (vertex, tm)"""
    ok, t0, t1 = segment(block, o, d, t_end)
    with np.errstate(all="ignore"):
        tm = f32(t0 + flight(block[0, 3], u_m))
        return bool(ok and tm < t1), tm


FOUR_PI = 4.0 * np.pi


def hg(g, c):
    """THE PHASE FUNCTION of the cosine c, binary64, rounded once"""
    c = np.fmin(np.fmax(f32(c), f32(-1.0)), f32(1.0))
    g = f32(g)
    if g == 0:
        return f32(1.0 / FOUR_PI)
    gd, cd = np.float64(g), np.float64(c)
    t = (1.0 + gd * gd) - (2.0 * gd) * cd
    return f32((1.0 - gd * gd) / (FOUR_PI * (t * np.sqrt(t))))


def hg_cosine(g, u):
    """the sampled cosine of the uniform u (a scalar, or an array: the same operations element by element)"""
    g = f32(g)
    ud = np.asarray(u, f32).astype(np.float64)
    if g == 0:
        return f32(1.0 - 2.0 * ud)
    gd = np.float64(g)
    s = 2.0 * ud - 1.0
    den = 1.0 + gd * s
    g2 = gd * gd
    num = ((s + (gd * (s * s + 3.0)) * 0.5) + g2 * s) + (g2 * gd) * ((s * s - 1.0) * 0.5)
    c = num / (den * den)
    return f32(np.minimum(np.maximum(c, -1.0), 1.0))


def hg_direction(d, c, v):
    """the scattered unit direction about d for the sampled cosine c and the draw v"""
    c = f32(c)
    s = f32(np.sqrt(max(ZERO, f32(ONE - f32(c * c)))))
    sp, cp = sincosf(f32(2.0 * np.pi * float(f32(v))))
    T, B = tangent_frame(d)
    nxt = ((f32(s * cp) * T).astype(f32) + (f32(s * sp) * B).astype(f32)).astype(f32)
    return _unit((nxt + (c * d).astype(f32)).astype(f32)).astype(f32)


def medium_light_weight(g, d, wi, p):
    """(ph / p) * mis(p, ph) of a light sample of density p towards wi at a medium vertex reached along d"""
    with np.errstate(all="ignore"):
        ph = hg(g, _dot(d, wi))
        return f32(f32(ph / p) * f32(lib().po_mis_power_heuristic(p, ph)))


# ---- binary64 helpers for the analytic tests: the same formulas, vectorised, sharing no code with the float32 half -------------
def hg_pdf64(g, c):
    c = np.asarray(c, np.float64)
    if g == 0:
        return np.full_like(c, 1.0 / FOUR_PI)
    return (1.0 - g * g) / (FOUR_PI * (1.0 + g * g - 2.0 * g * c) ** 1.5)


def hg_cdf64(g, c):
    """P(cosine <= c) under hg: the integral of 2 pi hg over [-1, c]"""
    c = np.asarray(c, np.float64)
    if g == 0:
        return 0.5 * (c + 1.0)
    return (1.0 - g * g) / (2.0 * g) * (1.0 / np.sqrt(1.0 + g * g - 2.0 * g * c) - 1.0 / (1.0 + g))


def segment64(lo, hi, o, d, t_end):
    """the slab segment in binary64: (t0, t1), empty where t1 <= t0"""
    lo, hi, o, d = (np.asarray(x, np.float64) for x in (lo, hi, o, d))
    t0, t1 = 0.0, float(t_end)
    for a in range(3):
        if d[a] != 0:
            ta, tb = (lo[a] - o[a]) / d[a], (hi[a] - o[a]) / d[a]
            t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
        elif not lo[a] <= o[a] <= hi[a]:
            return 0.0, 0.0
    return t0, t1


class MediumMixin:
    """The per-lane loop plus the medium.  medium: None, or (lo, hi, sigma_t, albedo, g); sigma_t 0 is None."""

    def __init__(self, *args, medium=None, **kw):
        super().__init__(*args, **kw)
        self.medium = None if medium is None or not medium[2] > 0 else medium_block(*medium)

    def sample(self, x, y, st, max_depth):
        L = lib()
        M = self.medium
        self.samples += 1
        u = f32(f32(f32(x) + self._u(st)) / f32(self.w))
        v = f32(f32(f32(y) + self._u(st)) / f32(self.h))
        o = np.zeros(3, f32); d = np.zeros(3, f32)
        L.po_camera_ray(C.byref(self.cf), u, v, o.ctypes.data, d.ctypes.data)
        tp = np.ones(3, f32); Lr = np.zeros(3, f32)
        pb_prev = f32(0.0)
        spec_prev = False
        q = self.q; omq = f32(ONE - q)
        mis = lambda a, b: f32(L.po_mis_power_heuristic(a, b))
        seen = lambda so, sd, t_end: ONE if M is None else transmittance(M, so, sd, t_end)      # T of a visible shadow ray

        def add(Lr, c, w, so, sd, t_end):
            c = (c * w).astype(f32)
            return Lr + c if M is None else Lr + (c * seen(so, sd, t_end)).astype(f32)

        for depth in range(max_depth):
            h = self._intersect(o, d)
            before = self.draws
            # 0: the free flight - one draw per path ray, whatever comes of it
            mv = False
            if M is not None:
                mv, tm = free_flight(M, o, d, f32(h.t) if h.hit else INF, self._u(st))
            # 1': a miss ends the sample, after the lookup where there is a map
            if not h.hit and not mv:
                if self.tab is not None:
                    r, j = lookup(self.tab, d)
                    E = self.tab["texel"][r, j, :3]; pdf = self.tab["texel"][r, j, 3]
                    if self.sampled and depth >= 1 and not spec_prev:
                        Lr = Lr + (tp * E) * mis(pb_prev, f32(q * pdf))
                    else:
                        Lr = Lr + tp * E
                break
            if mv:
                kind = MEDIUM
                kd = M[2, :3]
                p = (o + (tm * d).astype(f32)).astype(f32)
                g = M[1, 3]
            else:
                k = h.prim
                kind = int(self.kind[k])
                n_k = np.array(h.n, f32); Le = np.array(h.Le, f32); kd = np.array(h.bsdf, f32)
                t = f32(h.t); p = np.array(h.p, f32)
                # 1: emitted light, MIS-weighted where a light sample could have found it
                pa = self.pdf_area[k] if depth > 0 and self.next_event and not spec_prev else f32(0.0)
                if pa > 0:
                    p_l = f32(f32(pa * f32(t * t)) / abs(_dot(self.ng[k], d)))
                    if self.sampled:
                        p_l = f32(omq * p_l)
                    Lr = Lr + (tp * Le) * mis(pb_prev, p_l)
                else:
                    Lr = Lr + tp * Le
            # 2: the roulette, the throughput and its exit, sn and o'
            if depth > 2:
                rr = min(max(tp[0], max(tp[1], tp[2])), f32(0.95))
                if self._u(st) > rr:
                    self._seen(kind, depth, before)
                    break
                tp = tp * f32(ONE / rr)
            tp = tp * kd
            if f32(np.sqrt(_dot(tp, tp))) < f32(1e-5):
                self._seen(kind, depth, before)
                break
            if mv:
                sn = None
                o2 = p                                                 # no offset
            else:
                sn = shading_normal(d, n_k)
                o2 = p + EPS * sn
            # the delta kinds: no light sample; a mirror draws nothing, glass one number
            if kind in (MIRROR, GLASS):
                uu = self._u(st) if kind == GLASS else ONE
                self._seen(kind, depth, before)
                if depth + 1 >= max_depth:
                    self.cut += 1
                    break
                nxt, reflected, _ = scatter(d, n_k, kind, self.ior[k], uu)
                with np.errstate(all="ignore"):
                    len2 = _dot(nxt, nxt)
                if not (len2 > 0 and len2 <= FLT_MAX):
                    break
                o = o2 if reflected else (p - EPS * sn).astype(f32)
                d = _unit(nxt)
                spec_prev = True
                continue
            spec_prev = False
            rv = Vertex(sn, d, self.alpha[k]) if kind == ROUGH else None
            # 3 (3'): the light sample - three draws, five where the environment is sampled, whatever comes of them
            if self.next_event and depth + 1 < max_depth and (len(self.prim) or self.sampled):
                u_sel, r1, r2 = self._u(st), self._u(st), self._u(st)
                to_env = False
                if self.sampled:
                    r3, r4 = self._u(st), self._u(st)
                    to_env = u_sel <= q
                    if to_env:
                        r, j, wi = sample_direction(self.tab, r1, r2, r3, r4)
                        E = self.tab["texel"][r, j, :3]; pdf = self.tab["texel"][r, j, 3]
                        p_e = f32(q * pdf)
                        if mv:
                            w = medium_light_weight(g, d, wi, p_e) if 0 < p_e <= FLT_MAX else None
                        else:
                            cos_s = _dot(sn, wi)
                            w = light_weight(rv, wi, cos_s, p_e) if cos_s > 0 and 0 < p_e <= FLT_MAX else None
                        if w is not None and not self._intersect(o2, wi).hit:
                            Lr = add(Lr, tp * E, w, o2, wi, INF)
                    else:
                        u_sel = f32(f32(u_sel - q) / omq)
                if not to_env:
                    i = int(self.prim[select(self.cdf, self.total, u_sel)])
                    wi, _, cos_l, _, p_l = emitter_sample(self.s, i, self.ng[i], self.pdf_area[i], r1, r2, o2, omq if self.sampled else None)
                    if mv:
                        w = medium_light_weight(g, d, wi, p_l) if sample_counts(cos_l, p_l) else None
                    else:
                        with np.errstate(all="ignore"):
                            cos_s = _dot(sn, wi)
                        w = light_weight(rv, wi, cos_s, p_l) if cos_s > 0 and sample_counts(cos_l, p_l) else None
                    if w is not None:
                        hs = self._intersect(o2, wi)
                        if hs.hit and hs.prim == i:
                            Lr = add(Lr, tp * self.prims["Le"][i].astype(f32), w, o2, wi, f32(hs.t))
            # 4: the BSDF or phase sample - two draws, then the depth test
            uu, vw = self._u(st), self._u(st)
            self._seen(kind, depth, before)
            if depth + 1 >= max_depth:
                self.cut += 1
                break
            if mv:
                c = hg_cosine(g, uu)
                pb_prev = hg(g, c)
                d = hg_direction(d, c, vw)
                o = o2
                continue
            if kind == ROUGH:
                bs = rough_sample(rv, uu, vw) if rv.good else None
                if bs is None:
                    break
                nxt, wgt, pb_prev = bs
                with np.errstate(all="ignore"):
                    len2 = _dot(nxt, nxt)
                if not (len2 > 0 and len2 <= FLT_MAX):
                    break
                tp = (tp * wgt).astype(f32)
            else:
                nxt = np.zeros(3, f32)
                L.po_sample_cosine_hemisphere(sn.ctypes.data, uu, vw, nxt.ctypes.data)
                pb_prev = _over_pi(max(_dot(sn, nxt), f32(0.0)))
            o = o2
            d = _unit(nxt)
        return Lr


class MediumRenderer(MediumMixin, PathRenderer):
    """PathRenderer with a participating medium"""


class MediumLensRenderer(LensMixin, MediumMixin, PathRenderer):
    """MediumRenderer through a thin lens: the lens draws come first, as the mixin order says"""


class MediumTexturedSmoothRenderer(MediumMixin, TexturedSmoothRenderer):
    """TexturedSmoothRenderer (vertex normals and an albedo texture together) with a participating medium"""
