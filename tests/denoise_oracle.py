"""Independent numpy float32 restatements of the feature pass and the denoiser (include/ptmi.h: ptmi_render_features,
ptmi_denoise), written from the header's contract.  The features are traced through the CPU oracle's camera and intersect;
the filter is vectorised over the image, one tap at a time, every value float32 in the header's order."""
import numpy as np

from oracle_binding import camera_frame, camera_ray

F = np.float32
B3 = [F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16)]


def features(scene, cam, width, height, g, rows=None):
    """Feature buffers of a width x height frame (rows: the global rows to compute, default all) with g x g rays per pixel:
    dict of albedo, normal, position (len(rows), width, 3) and hit_fraction (len(rows), width)."""
    rows = np.arange(height) if rows is None else np.asarray(rows)
    cf = camera_frame(cam, width, height)
    prims = scene.prims()
    kd, nrm = prims["bsdf"], prims["normal"]
    out = {k: np.zeros((len(rows), width, 3), F) for k in ("albedo", "normal", "position")}
    hits = np.zeros((len(rows), width), F)
    offs = [(F(i) + F(0.5)) / F(g) for i in range(g)]
    for r, y in enumerate(rows):
        for x in range(width):
            a = np.zeros(3, F); n = np.zeros(3, F); p = np.zeros(3, F); h = F(0)
            for j in range(g):
                v = (F(y) + offs[j]) / F(height)
                for i in range(g):
                    u = (F(x) + offs[i]) / F(width)
                    o, d = camera_ray(cf, u, v)
                    hit = scene.intersect(o, d, 1e-4)
                    if hit.hit:
                        k = hit.prim
                        a = a + kd[k]; n = n + nrm[k]; p = p + (o + F(hit.t) * d); h = h + F(1)
            s = F(1) / F(g * g)
            out["albedo"][r, x] = a * s; out["normal"][r, x] = n * s; out["position"][r, x] = p * s; hits[r, x] = h * s
    out["hit_fraction"] = hits
    return out


def lum(c):
    T = c.dtype.type
    return T(F(0.2126)) * c[..., 0] + T(F(0.7152)) * c[..., 1] + T(F(0.0722)) * c[..., 2]


def auto_sigma_position(bmin, bmax):
    """0.02f x the diagonal of the root box of the scene's BVH"""
    d = (np.asarray(bmax, F) - np.asarray(bmin, F)).astype(F)
    return F(0.02) * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], dtype=F)


def denoise(radiance, feat, iterations, sigma_color, color_floor, sigma_x, normal_squarings, demodulate=True, T=F, trace=None):
    """The filter of include/ptmi.h on radiance (h, w, 3) float32 with the feature dict; returns the filtered radiance.  min and
    max are fmin and fmax (the header's NON-FINITE VALUES).  With T = np.float64 the same formulas are evaluated in binary64
    (the constants stay the float32 ones).  trace: a list that receives every iteration's W (h, w)."""
    rad = np.asarray(radiance, T)
    if iterations == 0:
        return rad.copy()
    alb = np.asarray(feat["albedo"], T)
    nrm = np.asarray(feat["normal"], T)
    pos = np.asarray(feat["position"], T)
    h, w, _ = rad.shape
    c = rad.copy()
    with np.errstate(all="ignore"):
        if demodulate:
            nz = alb != 0
            c[nz] = rad[nz] / alb[nz]
        sx2 = T(F(sigma_x)) * T(F(sigma_x))
        floor = T(F(color_floor))
        for it in range(iterations):
            s = 1 << it
            sc = T(F(sigma_color)) * T(2.0 ** -it)
            L = lum(c)
            W = np.zeros((h, w), T)
            S = np.zeros((h, w, 3), T)
            for dj in range(-2, 3):
                for di in range(-2, 3):
                    # q = p + (di s, dj s); the pixels p whose q is inside the image
                    y0, y1 = max(0, -dj * s), min(h, h - dj * s)
                    x0, x1 = max(0, -di * s), min(w, w - di * s)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + dj * s, y1 + dj * s), slice(x0 + di * s, x1 + di * s))
                    cp, cq = c[P], c[Q]
                    d = cp - cq
                    d2c = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    a = sc * (np.fmin(L[P], L[Q]) + floor)
                    wc = T(1) / (T(1) + d2c / (a * a))
                    np_, nq = nrm[P], nrm[Q]
                    wn = np.fmax(T(0), (np_[..., 0] * nq[..., 0] + np_[..., 1] * nq[..., 1]) + np_[..., 2] * nq[..., 2])
                    for _ in range(normal_squarings):
                        wn = wn * wn
                    e = pos[P] - pos[Q]
                    d2x = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                    wx = T(1) / (T(1) + d2x / sx2)
                    wt = ((T(B3[dj + 2] * B3[di + 2])) * wc * wn) * wx
                    W[P] = W[P] + wt
                    S[P] = S[P] + wt[..., None] * cq
            if trace is not None:
                trace.append(W.copy())
            out = c.copy()
            ok = W > 0
            out[ok] = S[ok] / W[ok][:, None]
            c = out
        if demodulate:
            nz = alb != 0
            c[nz] = c[nz] * alb[nz]
    return c
