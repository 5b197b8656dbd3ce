"""CPU restatement of rough metal (include/ptmi.h, "rough metal"), written from the header.

Every float operation of the estimator is float32 in the order the header writes it; sincosf is ptmi_sincosf through the
oracle's math batch, as tests/env_oracle.py takes it.  This is the kind-3 vertex alone - its frame, the light sample's weight and
the BSDF sample: the estimator that meets it is tests/path_oracle.py's one path loop.  The second half holds binary64 helpers for the analytic values (albedo by quadrature, the sampler's statistics):
they restate the same formulas in vectorised numpy float64 and share no code with the float32 half.
"""
import numpy as np

from env_oracle import PI_D, sincosf
from nee_oracle import _dot, _over_pi, _unit, f32, lib

ROUGH = 3
ZERO, ONE, TWO, FOUR, HALF_F = f32(0.0), f32(1.0), f32(2.0), f32(4.0), f32(0.5)
PI_F = f32(PI_D)
MIN_COS2 = f32(1e-37)                     # PTMI_ROUGH_MIN_COS2


def ok(c):
    with np.errstate(all="ignore"):
        return bool(c > 0 and f32(c * c) > MIN_COS2)


def frame(un):
    """(T, B) of sampleCosineHemisphere for the unit normal un"""
    if un[2] < f32(-0.9999999):
        return np.array([0, -1, 0], f32), np.array([-1, 0, 0], f32)
    a = f32(ONE / f32(ONE + un[2]))
    b = f32(f32(f32(-un[0]) * un[1]) * a)
    T = np.array([f32(ONE - f32(f32(un[0] * un[0]) * a)), b, f32(-un[0])], f32)
    B = np.array([b, f32(ONE - f32(f32(un[1] * un[1]) * a)), f32(-un[1])], f32)
    return T, B


def lam(a2, c):
    with np.errstate(all="ignore"):
        c2 = f32(c * c)
        return f32(HALF_F * f32(f32(np.sqrt(f32(ONE + f32(a2 * f32(f32(ONE - c2) / c2))))) - ONE))


def ggx_d(a2, h):
    t = f32(f32(f32(h[0] * h[0]) + f32(h[1] * h[1])) + f32(a2 * f32(h[2] * h[2])))
    return f32(a2 / f32(f32(PI_F * t) * t))


def cross(a, b):
    return np.array([f32(f32(a[1] * b[2]) - f32(a[2] * b[1])), f32(-f32(f32(a[0] * b[2]) - f32(a[2] * b[0]))),
                     f32(f32(a[0] * b[1]) - f32(a[1] * b[0]))], f32)


def _sum3(a, b, c):
    return ((a + b).astype(f32) + c).astype(f32)


class Vertex:
    """the frame of a rough vertex: un, T, B, wo, co, alpha, a2, good (the grazing test)"""

    @classmethod
    def local(cls, wo, alpha):
        """a vertex whose frame is the world's axes (sn = +z): wo is given directly"""
        v = cls.__new__(cls)
        v.un = np.array([0, 0, 1], f32)
        v.T, v.B = frame(v.un)
        v.wo = np.asarray(wo, f32)
        v.co = v.wo[2]
        v.alpha = f32(alpha); v.a2 = f32(v.alpha * v.alpha)
        v.good = ok(v.co)
        return v

    def __init__(self, sn, d, alpha):
        with np.errstate(all="ignore"):
            self.un = _unit(sn)
            self.T, self.B = frame(self.un)
            md = (-d).astype(f32)
            self.wo = np.array([_dot(md, self.T), _dot(md, self.B), _dot(md, self.un)], f32)
        self.co = self.wo[2]
        self.alpha = f32(alpha); self.a2 = f32(self.alpha * self.alpha)
        self.good = ok(self.co)


def evaluate(v, wi):
    """the light sample towards wi (world): (g, p_b), or None where it contributes nothing"""
    if not v.good:
        return None
    wl = np.array([_dot(wi, v.T), _dot(wi, v.B), _dot(wi, v.un)], f32)
    ci = wl[2]
    if not ok(ci):
        return None
    h = _unit((v.wo + wl).astype(f32))
    dh = ggx_d(v.a2, h)
    four_co = f32(FOUR * v.co)
    one_lo = f32(ONE + lam(v.a2, v.co))
    g = f32(dh / f32(four_co * f32(one_lo + lam(v.a2, ci))))
    p_b = f32(dh / f32(four_co * one_lo))
    return g, p_b


def sample_local(alpha, wo, u1, u2):
    """the visible-normal sample in the local frame: (h, wl)"""
    with np.errstate(all="ignore"):
        vh = _unit(np.array([f32(alpha * wo[0]), f32(alpha * wo[1]), wo[2]], f32))
        l2 = f32(f32(vh[0] * vh[0]) + f32(vh[1] * vh[1]))
        if l2 > 0:
            l = f32(np.sqrt(l2))
            T1 = np.array([f32(f32(-vh[1]) / l), f32(vh[0] / l), 0], f32)
        else:
            T1 = np.array([1, 0, 0], f32)
        T2 = cross(vh, T1)
        r = f32(np.sqrt(f32(u1)))
        sp, cp = sincosf(f32((2.0 * PI_D) * float(f32(u2))))
        t1 = f32(r * cp); t2 = f32(r * sp)
        s = f32(HALF_F * f32(ONE + vh[2]))
        t2 = f32(f32(f32(ONE - s) * f32(np.sqrt(max(ZERO, f32(ONE - f32(t1 * t1)))))) + f32(s * t2))
        z = f32(np.sqrt(max(ZERO, f32(f32(ONE - f32(t1 * t1)) - f32(t2 * t2)))))
        nh = _sum3(t1 * T1, t2 * T2, z * vh)
        h = _unit(np.array([f32(alpha * nh[0]), f32(alpha * nh[1]), max(ZERO, nh[2])], f32))
        wl = (f32(TWO * _dot(wo, h)) * h - wo).astype(f32)
    return h, wl


def sample(v, u1, u2):
    """the BSDF sample: (next (world, not normalised), weight, p_b), or None where the path ends"""
    h, wl = sample_local(v.alpha, v.wo, u1, u2)
    ci = wl[2]
    if not ok(ci):
        return None
    one_lo = f32(ONE + lam(v.a2, v.co))
    weight = f32(one_lo / f32(one_lo + lam(v.a2, ci)))
    p_b = f32(ggx_d(v.a2, h) / f32(f32(FOUR * v.co) * one_lo))
    nxt = _sum3(wl[0] * v.T, wl[1] * v.B, wl[2] * v.un)
    return nxt, weight, p_b


def light_weight(rv, wi, cos_s, p_light):
    """(f * cos * mis(p_light, p_b)) / p_light of a light sample of density p_light, without the colour: the cosine lobe (rv None),
    or the GGX lobe of the rough vertex rv; None where the sample contributes nothing"""
    mis = lambda a, b: f32(lib().po_mis_power_heuristic(a, b))
    with np.errstate(all="ignore"):
        if rv is None:
            p_b = _over_pi(cos_s)
            return f32(f32(p_b * mis(p_light, p_b)) / p_light)
        e = evaluate(rv, wi)
        if e is None:
            return None
        return f32(f32(e[0] * mis(p_light, e[1])) / p_light)


# ---- binary64: the analytic values ------------------------------------------------------------------------------------------------
def lam64(a2, c):
    c2 = c * c
    return 0.5 * (np.sqrt(1.0 + a2 * (1.0 - c2) / c2) - 1.0)


def d64(a2, z):
    t = z * z * (a2 - 1.0) + 1.0
    return a2 / (np.pi * t * t)


def wo64(theta):
    return np.array([np.sin(theta), 0.0, np.cos(theta)])


def f64(alpha, wo, wi):
    """the BSDF f = D G2 / (4 co ci) without the tint; wi (..., 3), ci > 0"""
    a2 = alpha * alpha
    h = wo + wi
    h = h / np.linalg.norm(h, axis=-1, keepdims=True)
    co, ci = wo[..., 2], wi[..., 2]
    g2 = 1.0 / (1.0 + lam64(a2, co) + lam64(a2, ci))
    return d64(a2, h[..., 2]) * g2 / (4.0 * co * ci)


def pdf64(alpha, wo, wi):
    """the visible-normal sampler's density over wi: G1(wo) D(h) / (4 co)"""
    a2 = alpha * alpha
    h = wo + wi
    h = h / np.linalg.norm(h, axis=-1, keepdims=True)
    return d64(a2, h[..., 2]) / (4.0 * wo[2] * (1.0 + lam64(a2, wo[2])))


def hemisphere_quadrature(fn, n_theta, n_phi):
    """midpoint rule over the upper hemisphere of wi: the integral of fn(wi) dOmega"""
    mu = (np.arange(n_theta) + 0.5) / n_theta                       # cos theta, uniform: dOmega = dmu dphi
    phi = (np.arange(n_phi) + 0.5) * (2.0 * np.pi / n_phi)
    total = 0.0
    for m in mu:                                                    # row by row keeps the arrays small
        s = np.sqrt(1.0 - m * m)
        wi = np.stack([s * np.cos(phi), s * np.sin(phi), np.full(n_phi, m)], axis=-1)
        total += fn(wi).sum()
    return total * (1.0 / n_theta) * (2.0 * np.pi / n_phi)


def albedo64(alpha, theta, n_theta=1500, n_phi=3000):
    """directional albedo: the integral of f cos over wi, by quadrature over wi (alpha >= 0.25)"""
    wo = wo64(theta)
    return hemisphere_quadrature(lambda wi: f64(alpha, wo, wi) * wi[..., 2], n_theta, n_phi)


def albedo_half_vector64(alpha, theta, n_r=4000, n_phi=2000):
    """the same albedo integrated over the half vector, where the lobe is narrow: albedo = integral of D_vis(h) G2 / G1 dh with
    D_vis(h) = G1(wo) max(0, wo.h) D(h) / co.  h is laid out through the slope radius r = tan(theta_h) / alpha, in which D is the
    fixed shape 1 / (pi (1 + r^2)^2) dA: r = tan(v) substitutes the infinite range to v in [0, pi / 2)."""
    a2 = alpha * alpha
    wo = wo64(theta)
    co = wo[2]
    lo = lam64(a2, co)
    v = (np.arange(n_r) + 0.5) * (0.5 * np.pi / n_r)
    r = np.tan(v)
    phi = (np.arange(n_phi) + 0.5) * (2.0 * np.pi / n_phi)
    total = 0.0
    for rv, vv in zip(r, v):
        th = np.arctan(alpha * rv)
        hz = np.cos(th); hs = np.sin(th)
        h = np.stack([hs * np.cos(phi), hs * np.sin(phi), np.full(n_phi, hz)], axis=-1)
        woh = h @ wo
        wi = 2.0 * woh[:, None] * h - wo
        ci = wi[:, 2]
        good = (woh > 0) & (ci > 1e-12)
        li = lam64(a2, np.where(good, ci, 1.0))
        # D(h) dOmega_h = D(h) sin(th) dth dphi; th = atan(alpha r): dth = alpha / (1 + a2 r^2) dr; dr = (1 + r^2) dv
        jac = hs * alpha / (1.0 + a2 * rv * rv) * (1.0 + rv * rv)
        val = np.where(good, woh / co * d64(a2, hz) / (1.0 + lo + li), 0.0)
        total += val.sum() * jac
    return total * (0.5 * np.pi / n_r) * (2.0 * np.pi / n_phi)


def sample64(alpha, wo, u1, u2):
    """the visible-normal sampler in binary64, vectorised over u1, u2: (wl, weight) with weight 0 below the horizon"""
    a2 = alpha * alpha
    vh = np.array([alpha * wo[0], alpha * wo[1], wo[2]])
    vh = vh / np.linalg.norm(vh)
    l2 = vh[0] * vh[0] + vh[1] * vh[1]
    T1 = np.array([-vh[1], vh[0], 0.0]) / np.sqrt(l2) if l2 > 0 else np.array([1.0, 0.0, 0.0])
    T2 = np.cross(vh, T1)
    r = np.sqrt(u1); phi = 2.0 * np.pi * u2
    t1 = r * np.cos(phi); t2 = r * np.sin(phi)
    s = 0.5 * (1.0 + vh[2])
    t2 = (1.0 - s) * np.sqrt(np.maximum(0.0, 1.0 - t1 * t1)) + s * t2
    nh = t1[:, None] * T1 + t2[:, None] * T2 + np.sqrt(np.maximum(0.0, 1.0 - t1 * t1 - t2 * t2))[:, None] * vh
    h = np.stack([alpha * nh[:, 0], alpha * nh[:, 1], np.maximum(0.0, nh[:, 2])], axis=-1)
    h = h / np.linalg.norm(h, axis=-1, keepdims=True)
    wl = 2.0 * (h @ wo)[:, None] * h - wo
    ci = wl[:, 2]
    up = ci > 0
    lo = lam64(a2, wo[2])
    w = np.where(up, (1.0 + lo) / (1.0 + lo + lam64(a2, np.where(up, ci, 1.0))), 0.0)
    return wl, w
