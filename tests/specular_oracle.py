"""CPU restatement of the specular surfaces (include/ptmi.h, "specular surfaces"), written from the header.

Every float operation is float32 in the order the header writes it.  This is the mirror / glass vertex alone: the estimator
that meets it is tests/path_oracle.py's one path loop.
"""
import numpy as np

from nee_oracle import _dot, _unit, f32

DIFFUSE, MIRROR, GLASS = 0, 1, 2
ONE, TWO, HALF_F = f32(1.0), f32(2.0), f32(0.5)


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
