"""CPU restatement of environment lighting (include/ptmi.h, "environment lighting"), written from the header.

The table is binary64 where the header says so (Python floats: IEEE + - * / without fma) and float32 elsewhere; ptmi_sincos_d is
restated from include/ptmi_math.h because the table feeds it a binary64 argument; ptmi_atan2f and ptmi_sincosf come from the
oracle's po_math_batch.  These are the table, the lookup and the sampled direction: the estimator that uses them is
tests/path_oracle.py's one path loop.
"""
import numpy as np

from nee_oracle import f32
from oracle_binding import math_batch

PI_D = 3.14159265358979323846
MATH_SINCOSF, MATH_ATAN2F = 5, 8


def sincos_d(x):
    """ptmi_sincos_d (include/ptmi_math.h) in Python floats, operation for operation"""
    INV_PIO2 = 6.36619772367581382433e-01
    PIO2_1 = 1.57079632673412561417e+00
    PIO2_1T = 6.07710050650619224932e-11
    y = x * INV_PIO2 + 0.5
    k = int(y)
    if float(k) > y:
        k -= 1
    kd = float(k)
    r = (x - kd * PIO2_1) - kd * PIO2_1T
    z = r * r
    S = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06,
         -2.50507602534068634195e-08, 1.58969099521155010221e-10)
    ps = S[5]
    for c in (S[4], S[3], S[2], S[1], S[0]):
        ps = ps * z + c
    sr = r + (r * z) * ps
    Cc = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07,
          2.08757232129817482790e-09, -1.13596475577881948265e-11)
    pc = Cc[5]
    for c in (Cc[4], Cc[3], Cc[2], Cc[1], Cc[0]):
        pc = pc * z + c
    cr = (1.0 - 0.5 * z) + (z * z) * pc
    return ((sr, cr), (cr, -sr), (-sr, -cr), (-cr, sr))[k & 3]


def sincosf(x):
    s, c = math_batch(MATH_SINCOSF, [x])[0]
    return f32(s), f32(c)


def atan2f(y, x):
    return f32(math_batch(MATH_ATAN2F, [y], [x])[0, 0])


def table(rgb, scale=1.0, rotation_deg=0.0):
    """THE TABLE of the header: dict(z, marginal_cdf, row_cdf, texel, total, rot, omega)"""
    rgb = np.ascontiguousarray(rgb, f32)
    h, w = rgb.shape[:2]
    z = np.array([f32(sincos_d((PI_D * float(r)) / float(h))[1]) for r in range(h + 1)], f32)
    z[0] = 1.0; z[h] = -1.0
    rot = f32(f32(rotation_deg) / f32(360.0))
    E = (rgb * f32(scale)).astype(f32)
    zd = z.astype(np.float64)
    omega = ((2.0 * PI_D) / float(w)) * (zd[:-1] - zd[1:])
    Ed = E.astype(np.float64)
    W = omega[:, None] * ((Ed[..., 0] + Ed[..., 1]) + Ed[..., 2])
    R = np.zeros((h, w)); T = np.zeros(h); M = np.zeros(h)
    tot = 0.0
    for r in range(h):
        acc = 0.0
        for j in range(w):
            acc = acc + W[r, j]
            R[r, j] = acc
        T[r] = acc
        tot = tot + acc
        M[r] = tot
    c = np.zeros((h, w), f32); m = np.zeros(h, f32)
    for r in range(h):
        if tot > 0:
            m[r] = f32(M[r] / tot)
        if T[r] > 0:
            c[r] = (R[r] / T[r]).astype(f32)
    md = m.astype(np.float64); cd = c.astype(np.float64)
    pm = md - np.concatenate([[0.0], md[:-1]])
    pc = cd - np.concatenate([np.zeros((h, 1)), cd[:, :-1]], axis=1)
    P = pm[:, None] * pc
    pdf = np.zeros((h, w), f32)
    for r in range(h):
        for j in range(w):
            if P[r, j] > 0:
                pdf[r, j] = f32(P[r, j] / omega[r])
    texel = np.concatenate([E, pdf[..., None]], axis=2).astype(f32)
    return dict(z=z, marginal_cdf=m, row_cdf=c, texel=texel, total=f32(tot), rot=rot, omega=omega, prob=P)


def lookup(tab, d):
    """THE LOOKUP texel(d): (row, column)"""
    z = tab["z"]; h = len(z) - 1; w = tab["row_cdf"].shape[1]
    y = min(max(f32(d[1]), f32(-1.0)), f32(1.0))
    r = h - 1
    for k in range(h):                                   # the smallest r with z[r + 1] < y
        if z[k + 1] < y:
            r = k
            break
    phi = atan2f(d[2], d[0])
    s = f32(float(phi) / (2.0 * PI_D))
    t = f32(s - tab["rot"])
    t = f32(t - f32(np.floor(t)))
    j = min(int(f32(t * f32(w))), w - 1)
    return r, j


def first_at_least(cdf, u):
    """the smallest index with u <= cdf[index]"""
    return int(np.searchsorted(cdf, u, side="left"))


def sample_direction(tab, r1, r2, r3, r4):
    """step 3' of the header: (row, column, wi)"""
    z = tab["z"]; w = tab["row_cdf"].shape[1]
    r = first_at_least(tab["marginal_cdf"], r1)
    j = first_at_least(tab["row_cdf"][r], r2)
    ct = f32(z[r + 1] + f32(r3 * f32(z[r] - z[r + 1])))
    st = f32(np.sqrt(max(f32(0.0), f32(f32(1.0) - f32(ct * ct)))))
    a = f32(f32(f32(f32(j) + r4) / f32(w)) + tab["rot"])
    sp, cp = sincosf(f32((2.0 * PI_D) * float(a)))
    return r, j, np.array([f32(st * cp), ct, f32(st * sp)], f32)


# ------------------------------------------------------------------------------------------------
# One vertex of the contract, vectorised in binary64 - for expectation tests that need 10^6 .. 10^7 samples (the scalar
# restatement above makes 10^4 a second).  A surface point with shading normal `normal` and no emitter in the scene (q = 1),
# from which every ray escapes: a sample is the light sample of step 3' plus the BSDF ray's miss of step 1'.  The table, the two
# searches, the direction formulas, p_e, p_b and the weights are the header's; the float32 roundings of the direction
# arithmetic are not kept (the tests that use this compare means, not bits; test_env_furnace_host checks it against the scalar
# functions above draw for draw).  Returns the samples per unit albedo and channel 0 of the map.
# ------------------------------------------------------------------------------------------------
def _lookup_many(tab, d):
    z = tab["z"].astype(np.float64); h = len(z) - 1; w = tab["row_cdf"].shape[1]
    y = np.clip(d[:, 1], -1.0, 1.0)
    r = np.clip(np.searchsorted(-z[1:], -y, side="right"), 0, h - 1)          # the smallest r with z[r + 1] < y
    t = np.arctan2(d[:, 2], d[:, 0]) / (2.0 * np.pi) - float(tab["rot"])
    t = t - np.floor(t)
    j = np.minimum((t * w).astype(np.int64), w - 1)
    return r, j


def _mis(a, b):
    with np.errstate(all="ignore"):
        return np.where(a > 0, (a * a) / (a * a + b * b), 0.0)


def vertex_directions(tab, r1, r2, r3, r4):
    """step 3' for arrays of draws: (row, column, wi)"""
    z = tab["z"].astype(np.float64); w = tab["row_cdf"].shape[1]
    r = np.searchsorted(tab["marginal_cdf"], r1.astype(f32), side="left")
    flat = (tab["row_cdf"].astype(np.float64) + np.arange(len(z) - 1)[:, None] * 2.0).ravel()   # rows made one increasing sequence
    j = np.searchsorted(flat, r2.astype(f32).astype(np.float64) + r * 2.0, side="left") - r * w
    ct = z[r + 1] + r3 * (z[r] - z[r + 1])
    st = np.sqrt(np.maximum(0.0, 1.0 - ct * ct))
    a = (j + r4) / w + float(tab["rot"])
    return r, j, np.stack([st * np.cos(2.0 * np.pi * a), ct, st * np.sin(2.0 * np.pi * a)], 1)


def vertex_samples(tab, normal, n, rng, next_event):
    n_ = np.asarray(normal, np.float64); n_ = n_ / np.linalg.norm(n_)
    E = tab["texel"][..., 0].astype(np.float64); pdf = tab["texel"][..., 3].astype(np.float64)
    u = 1.0 - rng.random((n, 6))                                               # (0, 1], as curand_uniform
    out = np.zeros(n)
    if next_event:
        r, j, wi = vertex_directions(tab, u[:, 0], u[:, 1], u[:, 2], u[:, 3])
        cos_s = wi @ n_
        p_e = pdf[r, j]                                                        # q = 1
        p_b = cos_s / np.pi
        ok = (cos_s > 0) & (p_e > 0)
        with np.errstate(all="ignore"):
            out += np.where(ok, E[r, j] * (p_b * _mis(p_e, p_b)) / p_e, 0.0)
    # the BSDF sample: a cosine-distributed direction about the normal (any tangent frame: the density is what matters)
    t = np.cross(n_, [0.0, 0.0, 1.0] if abs(n_[2]) < 0.9 else [1.0, 0.0, 0.0]); t = t / np.linalg.norm(t)
    b = np.cross(n_, t)
    rr, phi = np.sqrt(u[:, 4]), 2.0 * np.pi * u[:, 5]
    cz = np.sqrt(np.maximum(0.0, 1.0 - u[:, 4]))
    d = (rr * np.cos(phi))[:, None] * t + (rr * np.sin(phi))[:, None] * b + cz[:, None] * n_
    r, j = _lookup_many(tab, d)
    out += E[r, j] * (_mis(cz / np.pi, pdf[r, j]) if next_event else 1.0)
    return out
