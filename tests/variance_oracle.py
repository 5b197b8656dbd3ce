"""Independent numpy restatement of the variance-guided a-trous filter (include/ptmi.h: ptmi_denoise_variance), written from
the header's contract: vectorised over the image, one tap at a time, every value float32 in the header's order.  With T =
np.float64 the same formulas are evaluated in binary64 (the constants stay the float32 ones), for the rounding bound of
tests/test_variance_host.py."""
import numpy as np

from denoise_oracle import B3, auto_sigma_position, lum  # noqa: F401  (auto_sigma_position: for the callers)

F = np.float32
G3 = [F(0.25), F(0.5), F(0.25)]


def _window(h, w, dy, dx):
    """(P, Q): the pixels p whose tap q = p + (dx, dy) lies inside the image, and those taps; None if there are none"""
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def _wn(nrm, P, Q, normal_squarings, T):
    a, b = nrm[P], nrm[Q]
    wn = np.fmax(T(0), (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2])
    for _ in range(normal_squarings):
        wn = wn * wn
    return wn


def _wx(pos, P, Q, sx2, T):
    e = pos[P] - pos[Q]
    d2x = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    return T(1) / (T(1) + d2x / sx2)


def demodulated(radiance, albedo, demodulate, T=F):
    """step 1"""
    rad = np.asarray(radiance, T)
    c = rad.copy()
    if demodulate:
        alb = np.asarray(albedo, T)
        nz = alb != 0
        c[nz] = rad[nz] / alb[nz]
    return c


def accumulation_variance(c, radiance, m2, passes, T=F):
    """step 2 for every pixel (meaningful where passes >= 2)"""
    k = np.asarray(passes, np.uint32)
    kk = (k * (k - np.uint32(1))).astype(T)                       # the uint32 product of the stopping rule
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.fmax(T(0), np.asarray(m2, T) / kk)
        lr = lum(np.asarray(radiance, T))
        s = lum(c) / lr
        return np.where(lr > 0, (v * s) * s, v).astype(T)


def spatial_variance(c, nrm, pos, radius, normal_squarings, sigma_x, T=F):
    """step 3 for every pixel: two sweeps over the (2 radius + 1)^2 window"""
    h, w, _ = c.shape
    sx2 = T(sigma_x) * T(sigma_x)
    L = lum(c)
    taps = []
    W = np.zeros((h, w), T); A = np.zeros((h, w), T)
    for dj in range(-radius, radius + 1):
        for di in range(-radius, radius + 1):
            pq = _window(h, w, dj, di)
            if pq is None:
                continue
            P, Q = pq
            wt = _wn(nrm, P, Q, normal_squarings, T) * _wx(pos, P, Q, sx2, T)
            taps.append((P, Q, wt))
            W[P] = W[P] + wt
            A[P] = A[P] + wt * L[Q]
    ok = W > 0
    m = np.zeros((h, w), T)
    m[ok] = A[ok] / W[ok]
    B = np.zeros((h, w), T)
    for P, Q, wt in taps:
        d = L[Q] - m[P]
        B[P] = B[P] + wt * (d * d)
    v = np.zeros((h, w), T)
    v[ok] = B[ok] / W[ok]
    return v


def atrous(c, v, nrm, pos, iterations, sigma_luminance, epsilon, sigma_x, normal_squarings, T=F, trace=None):
    """step 4 on the demodulated colour c (h, w, 3) and the variance v (h, w); returns (c, v) after the last iteration.
    trace: a list that receives every iteration's (W, V, gd), each (h, w)"""
    h, w, _ = c.shape
    sx2 = T(sigma_x) * T(sigma_x)
    sl2 = T(sigma_luminance) * T(sigma_luminance)
    eps = T(epsilon)
    c = np.asarray(c, T).copy(); v = np.asarray(v, T).copy()
    for it in range(iterations):
        s = 1 << it
        gn = np.zeros((h, w), T); gd = np.zeros((h, w), T)
        for dj in range(-1, 2):
            for di in range(-1, 2):
                pq = _window(h, w, dj, di)
                if pq is None:
                    continue
                P, Q = pq
                g = T(G3[dj + 1] * G3[di + 1])
                gn[P] = gn[P] + g * v[Q]
                gd[P] = gd[P] + g
        a = sl2 * (gn / gd) + eps
        L = lum(c)
        W = np.zeros((h, w), T); S = np.zeros((h, w, 3), T); V = np.zeros((h, w), T)
        for dj in range(-2, 3):
            for di in range(-2, 3):
                pq = _window(h, w, dj * s, di * s)
                if pq is None:
                    continue
                P, Q = pq
                dl = L[P] - L[Q]
                wl = T(1) / (T(1) + (dl * dl) / a[P])
                wt = (((B3[dj + 2] * B3[di + 2]) * wl) * _wn(nrm, P, Q, normal_squarings, T)) * _wx(pos, P, Q, sx2, T)
                W[P] = W[P] + wt
                S[P] = S[P] + wt[..., None] * c[Q]
                V[P] = V[P] + (wt * wt) * v[Q]
        if trace is not None:
            trace.append((W.copy(), V.copy(), gd.copy()))
        ok = W > 0
        c2 = c.copy(); v2 = v.copy()
        c2[ok] = S[ok] / W[ok][:, None]
        v2[ok] = (V[ok] / W[ok]) / W[ok]
        c, v = c2, v2
    return c, v


def denoise_variance(radiance, feat, iterations, sigma_luminance, epsilon, sigma_x, normal_squarings, demodulate=True,
                     spatial_radius=3, moments=None, T=F, trace=None):
    """Steps 1 - 5 on radiance (h, w, 3) with the feature dict.  moments: None (spatial everywhere) or (M2, passes) of the
    accumulation whose pass image radiance is (source = 0).  Returns (filtered radiance, variance_in, variance_out)."""
    with np.errstate(all="ignore"):                             # non-finite pixels are inputs like any other
        rad = np.asarray(radiance, T)
        alb = np.asarray(feat["albedo"], T); nrm = np.asarray(feat["normal"], T); pos = np.asarray(feat["position"], T)
        c = demodulated(rad, alb, demodulate, T)
        v = spatial_variance(c, nrm, pos, spatial_radius, normal_squarings, sigma_x, T)
        if moments is not None:
            m2, passes = moments
            v = np.where(np.asarray(passes) >= 2, accumulation_variance(c, rad, m2, passes, T), v).astype(T)
        if iterations == 0:
            return rad.copy(), v, v.copy()
        c, vo = atrous(c, v, nrm, pos, iterations, sigma_luminance, epsilon, sigma_x, normal_squarings, T, trace)
        if demodulate:
            nz = alb != 0
            c[nz] = c[nz] * alb[nz]
        return c, v, vo
