"""CPU restatement of the per-lane estimator (include/ptmi.h: "next-event estimation", "environment lighting", "specular surfaces",
"rough metal"), written from the header: ONE path loop, PathRenderer.sample, laid out in the order of the contract's steps.

The loop is configured as the kernel is: next_event, the map (the kernel's ENV) and the surface table (its SURF: no table,
mirror / glass, rough metal too) switch steps on and off inside it.  What a step computes is restated once, in the module of the
section that introduces it - nee_oracle (the binding, the emitter table, the emitter sample), env_oracle (the table, the lookup,
the sampled direction), specular_oracle (scatter), rough_oracle (the GGX vertex) - and the loop only calls it.  NeeRenderer,
EnvRenderer, SpecRenderer and RoughRenderer are constructors of configurations and nothing else;
tests/golden/restatement_pinned.npz pins each to the separate loop it once had (tests/test_restatement_pinned.py).
"""
import ctypes as C

import numpy as np

from env_oracle import lookup, sample_direction, table
from nee_oracle import FLT_MAX, _dot, _over_pi, _unit, emitter_sample, emitter_table, f32, geometric_normals, lib, sample_counts, select
from oracle_binding import CameraFrame, Hit
from rough_oracle import ROUGH, Vertex, light_weight, sample as rough_sample
from specular_oracle import GLASS, MIRROR, scatter, shading_normal

ONE, EPS = f32(1.0), f32(1e-4)


class PathRenderer:
    """Frames of a context over an OracleScene with persistent per-pixel streams (as a ptmi context keeps them).
    kind (n_prims,) of 0 .. 3 (None: all diffuse), ior and roughness (n_prims,) or scalars (None: 1.5, 0.3), load order; env_rgb
    the map (None: none), with scale, rotation_deg and select_fraction as ptmi_env_params.  samples and draws count the samples
    and the stream's draws, cut the samples ended by max_depth; trace (a list, or None) receives (kind, depth, draws) of every
    vertex."""

    def __init__(self, oscene, cam, width, height, kind=None, ior=None, roughness=None, env_rgb=None, next_event=False,
                 scale=1.0, rotation_deg=0.0, select_fraction=0.5, seed_base=2023):
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
        self.tab = None if env_rgb is None else table(env_rgb, scale, rotation_deg)
        self.next_event = bool(next_event)
        self.sampled = self.next_event and self.tab is not None and self.tab["total"] > 0
        self.q = f32(1.0) if len(self.prim) == 0 else f32(select_fraction)
        n = len(self.prims["type"])
        self.kind = np.zeros(n, np.int32) if kind is None else np.asarray(kind, np.int32).reshape(n)
        self.ior = np.broadcast_to(np.asarray(1.5 if ior is None else ior, f32), (n,)).astype(f32)
        r = np.broadcast_to(np.asarray(0.3 if roughness is None else roughness, f32), (n,)).astype(f32)
        self.alpha = (r * r).astype(f32)
        self.samples = self.draws = self.cut = 0
        self.trace = None

    def _u(self, st):
        self.draws += 1
        return f32(lib().po_rng_uniform(st.ctypes.data))

    def _intersect(self, o, d):
        lib().po_intersect(self.s.h, o.ctypes.data, d.ctypes.data, 1e-4, FLT_MAX, 1, C.byref(self.hit))
        return self.hit

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
            # 1': a miss ends the sample, after the lookup where there is a map
            if not h.hit:
                if self.tab is not None:
                    r, j = lookup(self.tab, d)
                    E = self.tab["texel"][r, j, :3]; pdf = self.tab["texel"][r, j, 3]
                    if self.sampled and depth >= 1 and not spec_prev:
                        Lr = Lr + (tp * E) * mis(pb_prev, f32(q * pdf))
                    else:
                        Lr = Lr + tp * E
                break
            before = self.draws
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
                        cos_s = _dot(sn, wi)
                        p_e = f32(q * pdf)
                        if cos_s > 0 and 0 < p_e <= FLT_MAX:
                            w = light_weight(rv, wi, cos_s, p_e)
                            if w is not None and not self._intersect(o2, wi).hit:
                                Lr = Lr + (tp * E) * w
                    else:
                        u_sel = f32(f32(u_sel - q) / omq)
                if not to_env:
                    i = int(self.prim[select(self.cdf, self.total, u_sel)])
                    wi, _, cos_l, _, p_l = emitter_sample(self.s, i, self.ng[i], self.pdf_area[i], r1, r2, o2, omq if self.sampled else None)
                    with np.errstate(all="ignore"):
                        cos_s = _dot(sn, wi)
                    if cos_s > 0 and sample_counts(cos_l, p_l):
                        w = light_weight(rv, wi, cos_s, p_l)
                        if w is not None:
                            hs = self._intersect(o2, wi)
                            if hs.hit and hs.prim == i:
                                Lr = Lr + (tp * self.prims["Le"][i].astype(f32)) * w
            # 4: the BSDF sample - two draws, then the depth test
            uu, vw = self._u(st), self._u(st)
            self._seen(kind, depth, before)
            if depth + 1 >= max_depth:
                self.cut += 1
                break
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


class NeeRenderer(PathRenderer):
    """next-event estimation over the emitters: no map, no table (the kernel's ENV = 0, SURF = 0)"""

    def __init__(self, oscene, cam, width, height, seed_base=2023):
        super().__init__(oscene, cam, width, height, next_event=True, seed_base=seed_base)


class EnvRenderer(PathRenderer):
    """a context with an environment (ENV = 1, SURF = 0): next_event False - the reference's estimator plus the lookup where a
    path ray misses; True - NEE with the environment as a second light.  env_rgb None: no environment (NeeRenderer's estimator
    for next_event True, the reference's for False)."""

    def __init__(self, oscene, cam, width, height, env_rgb, next_event, scale=1.0, rotation_deg=0.0, select_fraction=0.5, seed_base=2023):
        super().__init__(oscene, cam, width, height, None, None, None, env_rgb, next_event, scale, rotation_deg, select_fraction, seed_base)


class SpecRenderer(PathRenderer):
    """a context with a surface table of kinds 0 .. 2 (SURF = 1): kind (n_prims,) and ior (n_prims,) or a scalar (None: 1.5)"""

    def __init__(self, oscene, cam, width, height, kind, ior=None, env_rgb=None, next_event=False, **prm):
        super().__init__(oscene, cam, width, height, kind, ior, None, env_rgb, next_event, **prm)


class RoughRenderer(PathRenderer):
    """a context with a surface table that may hold rough metal (SURF = 2): kinds 0 .. 3, ior and roughness (n_prims,) or scalars
    (None: 1.5, 0.3)"""

    def __init__(self, oscene, cam, width, height, kind, ior=None, roughness=None, env_rgb=None, next_event=False, **prm):
        super().__init__(oscene, cam, width, height, kind, ior, roughness, env_rgb, next_event, **prm)
