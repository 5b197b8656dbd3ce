"""CPU restatement of the specular surfaces (include/ptmi.h, "specular surfaces"), written from the header.

Every float operation is float32 in the order the header writes it.  The estimator extends tests/env_oracle.py's EnvRenderer
(which restates next-event estimation and environment lighting and supplies the scene, the camera and the streams) by the
spec_prev flag and the mirror / glass vertex.
"""
import ctypes as C

import numpy as np

from env_oracle import EnvRenderer, lookup, sample_direction
from nee_oracle import FLT_MAX, _dot, _over_pi, _unit, emitter_sample, f32, lib, sample_counts, select

DIFFUSE, MIRROR, GLASS = 0, 1, 2
ONE, TWO, HALF_F, EPS = f32(1.0), f32(2.0), f32(0.5), f32(1e-4)


def shading_normal(d, n_k):
    """sn: the stored normal turned against d"""
    return n_k if _dot(d, n_k) < 0 else -n_k


def reflect(d, un):
    """next = d - (2 * dn) * un"""
    dn = _dot(d, un)
    return (d - f32(TWO * dn) * un).astype(f32)


def fresnel(eta, ci):
    """(F, ct) of the header; total internal reflection (s2 >= 1): (1, None)"""
    s2 = f32(f32(eta * eta) * max(f32(0.0), f32(ONE - f32(ci * ci))))
    if s2 >= ONE and eta != ONE:
        return ONE, None
    ct = ci if eta == ONE else f32(np.sqrt(f32(ONE - s2)))
    rs = f32(f32(f32(eta * ci) - ct) / f32(f32(eta * ci) + ct))
    rp = f32(f32(ci - f32(eta * ct)) / f32(ci + f32(eta * ct)))
    return f32(HALF_F * f32(f32(rs * rs) + f32(rp * rp))), ct


def refract(d, un, eta, ci, ct):
    """next = eta * d + (eta * ci - ct) * un"""
    return (eta * d + f32(f32(eta * ci) - ct) * un).astype(f32)


def interface(d, n_k, ior):
    """(un, eta, ci) of a glass vertex: the unit shading normal, n_i / n_t and the clamped cosine of incidence"""
    un = _unit(shading_normal(d, n_k))
    eta = f32(ONE / f32(ior)) if _dot(d, n_k) < 0 else f32(ior)
    ci = min(ONE, f32(-_dot(d, un)))
    return un, eta, ci


def scatter(d, n_k, kind, ior, u):
    """The specular vertex: (next, reflected, F) - next is NOT normalised (the header normalises after its length test); u is the
    glass vertex's draw (ignored for a mirror)"""
    with np.errstate(all="ignore"):
        if kind == MIRROR:
            return reflect(d, _unit(shading_normal(d, n_k))), True, ONE
        un, eta, ci = interface(d, n_k, ior)
        F, ct = fresnel(eta, ci)
        if ct is None or u <= F:
            return reflect(d, un), True, F
        return refract(d, un, eta, ci, ct), False, F


class SpecRenderer(EnvRenderer):
    """Frames of a context with a surface table: kind (n_prims,) and ior (n_prims,) or a scalar (None: 1.5), load order.  With an
    all-diffuse table this is EnvRenderer's estimator draw for draw (NeeRenderer's where there is no map and next_event is set).
    cut counts the samples ended by max_depth; trace (a list, or None) receives (kind, depth, draws) of every vertex."""

    def __init__(self, oscene, cam, width, height, kind, ior=None, env_rgb=None, next_event=False, **prm):
        super().__init__(oscene, cam, width, height, env_rgb, next_event, **prm)
        n = len(self.prims["type"])
        self.kind = np.zeros(n, np.int32) if kind is None else np.asarray(kind, np.int32).reshape(n)
        self.ior = np.broadcast_to(np.asarray(1.5 if ior is None else ior, f32), (n,)).astype(f32)
        self.cut = 0
        self.samples = 0
        self.draws = 0
        self.trace = None

    def _u(self, st):
        self.draws += 1
        return super()._u(st)

    def _seen(self, kind, depth, before):
        if self.trace is not None:
            self.trace.append((int(kind), depth, self.draws - before))

    def sample(self, x, y, st, max_depth):
        L = lib()
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
        for depth in range(max_depth):
            h = self._intersect(o, d)
            if not h.hit:
                if self.tab is not None:                     # 1'
                    r, j = lookup(self.tab, d)
                    E = self.tab["texel"][r, j, :3]; pdf = self.tab["texel"][r, j, 3]
                    if self.sampled and depth >= 1 and not spec_prev:
                        Lr = Lr + (tp * E) * mis(pb_prev, f32(q * pdf))
                    else:
                        Lr = Lr + tp * E
                break
            before = self.draws
            k = h.prim
            n_k = np.array(h.n, f32); Le = np.array(h.Le, f32); kd = np.array(h.bsdf, f32)
            t = f32(h.t); p = np.array(h.p, f32)
            pa = self.pdf_area[k] if depth > 0 and self.next_event and not spec_prev else f32(0.0)
            if pa > 0:
                p_l = f32(f32(pa * f32(t * t)) / abs(_dot(self.ng[k], d)))
                if self.sampled:
                    p_l = f32(omq * p_l)
                Lr = Lr + (tp * Le) * mis(pb_prev, p_l)
            else:
                Lr = Lr + tp * Le
            if depth > 2:
                rr = min(max(tp[0], max(tp[1], tp[2])), f32(0.95))
                if self._u(st) > rr:
                    self._seen(self.kind[k], depth, before)
                    break
                tp = tp * f32(ONE / rr)
            tp = tp * kd
            if f32(np.sqrt(_dot(tp, tp))) < f32(1e-5):
                self._seen(self.kind[k], depth, before)
                break
            sn = shading_normal(d, n_k)
            o2 = p + EPS * sn
            if self.kind[k] != DIFFUSE:
                uu = self._u(st) if self.kind[k] == GLASS else ONE
                self._seen(self.kind[k], depth, before)
                if depth + 1 >= max_depth:
                    self.cut += 1
                    break
                nxt, reflected, _ = scatter(d, n_k, self.kind[k], self.ior[k], uu)
                with np.errstate(all="ignore"):
                    len2 = _dot(nxt, nxt)
                if not (len2 > 0 and len2 <= FLT_MAX):
                    break
                o = o2 if reflected else (p - EPS * sn).astype(f32)
                d = _unit(nxt)
                spec_prev = True
                continue
            spec_prev = False
            if self.next_event and depth + 1 < max_depth and (len(self.prim) or self.sampled):
                u_sel, r1, r2 = self._u(st), self._u(st), self._u(st)
                to_env = False
                if self.sampled:
                    r3, r4 = self._u(st), self._u(st)
                    to_env = u_sel <= q
                    if to_env:
                        r, j, wi = sample_direction(self.tab, r1, r2, r3, r4)
                        E = self.tab["texel"][r, j, :3]; pdf = self.tab["texel"][r, j, 3]
                        cos_s = _dot(sn, wi)
                        p_e = f32(q * pdf)
                        if cos_s > 0 and 0 < p_e <= FLT_MAX and not self._intersect(o2, wi).hit:
                            p_b = _over_pi(cos_s)
                            w = f32(f32(p_b * mis(p_e, p_b)) / p_e)
                            Lr = Lr + (tp * E) * w
                    else:
                        u_sel = f32(f32(u_sel - q) / omq)
                if not to_env:
                    i = int(self.prim[select(self.cdf, self.total, u_sel)])
                    wi, _, cos_l, _, p_l = emitter_sample(self.s, i, self.ng[i], self.pdf_area[i], r1, r2, o2, omq if self.sampled else None)
                    with np.errstate(all="ignore"):
                        cos_s = _dot(sn, wi)
                    if cos_s > 0 and sample_counts(cos_l, p_l):
                        hs = self._intersect(o2, wi)
                        if hs.hit and hs.prim == i:
                            p_b = _over_pi(cos_s)
                            w = f32(f32(p_b * mis(p_l, p_b)) / p_l)
                            Lr = Lr + (tp * self.prims["Le"][i].astype(f32)) * w
            uu, vw = self._u(st), self._u(st)
            self._seen(DIFFUSE, depth, before)
            if depth + 1 >= max_depth:
                self.cut += 1
                break
            nxt = np.zeros(3, f32)
            L.po_sample_cosine_hemisphere(sn.ctypes.data, uu, vw, nxt.ctypes.data)
            pb_prev = _over_pi(max(_dot(sn, nxt), f32(0.0)))
            o = o2
            d = _unit(nxt)
        return Lr
