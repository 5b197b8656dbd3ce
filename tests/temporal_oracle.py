"""Independent numpy float32 restatement of the temporal step (include/ptmi.h: ptmi_temporal_accumulate), written from the
header's contract.  Its inputs are what the GPU exposes: the image, the features, the sample counts and the camera frames;
the features themselves are pinned to the CPU oracle by test_gpu_denoise.py.  Vectorised over the image, one tap at a
time, every value float32 in the header's order."""
import numpy as np

F = np.float32


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], -(a[0] * b[2] - a[2] * b[0]), a[0] * b[1] - a[1] * b[0]], F)


def auto_sigma_position(bmin, bmax):
    """0.01f x the diagonal of the root box of the scene's BVH"""
    d = (np.asarray(bmax, F) - np.asarray(bmin, F)).astype(F)
    return F(0.01) * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], dtype=F)


class History:
    """The history after a step: colour (h, w, 3), count (h, w), the features of its view and its camera frame."""

    def __init__(self, color, count, feat, cam):
        self.color, self.count = color, count
        self.albedo, self.normal, self.position, self.hf = feat["albedo"], feat["normal"], feat["position"], feat["hit_fraction"]
        self.cam = np.asarray(cam, F).copy()


def reproject(hist_cam, cam_origin, feat, w, h):
    """Steps 2 - 3 and the tap geometry of step 4 for every pixel of the feature dict (arrays (..., 3) and (...)): a dict of x, nc,
    ac, den, fn, sp, sc, px, py (as computed, before any test), ok (p has taps at all), x0, y0 (int64), fx, fy."""
    hist_cam = np.asarray(hist_cam, F); cam_origin = np.asarray(cam_origin, F)
    hf = np.asarray(feat["hit_fraction"], F)
    with np.errstate(all="ignore"):
        x = np.asarray(feat["position"], F) / hf[..., None]
        nc = np.asarray(feat["normal"], F) / hf[..., None]
        ac = np.asarray(feat["albedo"], F) / hf[..., None]
        o, llc, hor, ver = hist_cam[0:3], hist_cam[3:6], hist_cam[6:9], hist_cam[9:12]
        f = llc - o
        nrm = cross(hor, ver)
        d = x - o
        den = dot(d, nrm)
        fn = dot(f, nrm)
        sp = dot(nc, o - x)
        sc = dot(nc, cam_origin - x)
        ok = (hf != 0) & (((fn > 0) & (den > 0)) | ((fn < 0) & (den < 0))) & (((sp > 0) & (sc > 0)) | ((sp < 0) & (sc < 0)))
        s = fn / den
        q = s[..., None] * d - f
        u = dot(q, hor) / dot(hor, hor)
        v = dot(q, ver) / dot(ver, ver)
        px = u * F(w) - F(0.5)
        py = v * F(h) - F(0.5)
        ok = ok & (px >= F(-1)) & (px < F(w)) & (py >= F(-1)) & (py < F(h))
        pxs = np.where(ok, px, F(0))
        pys = np.where(ok, py, F(0))
        x0f, y0f = np.floor(pxs), np.floor(pys)
        fx, fy = pxs - x0f, pys - y0f
    return dict(x=x, nc=nc, ac=ac, den=den, fn=fn, sp=sp, sc=sc, px=px, py=py, ok=ok, x0=x0f.astype(np.int64), y0=y0f.astype(np.int64),
                fx=fx, fy=fy)


def step(hist, radiance, m, feat, cam, max_history=32, normal_min=0.9, sigma_x=None, sigma_albedo=0.1, trace=None):
    """One step.  hist: a History or None (empty); radiance (h, w, 3); m: samples per pixel, a number or (h, w); feat: the
    current features (dict of albedo, normal, position (h, w, 3) and hit_fraction (h, w)); cam: the current camera frame (12 floats).
    Returns (radiance out, the new History, (accepted, rejected, missed)).  min is fmin (the header's NON-FINITE VALUES).
    trace: a dict that receives reproject()'s values, W (h, w), keep (4, h, w) and the per-tap dot products nn, ee, aa (4, h, w)."""
    cur = np.asarray(radiance, F)
    h, w, _ = cur.shape
    m = np.broadcast_to(np.asarray(m, F), (h, w))
    cam = np.asarray(cam, F)
    hf = feat["hit_fraction"].astype(F)
    reuse = np.zeros((h, w), bool)
    H = np.zeros((h, w, 3), F)
    nacc = np.zeros((h, w), F)
    if hist is not None and np.array_equal(hist.cam.view(np.uint32), cam.view(np.uint32)) and hist.color.shape == cur.shape:
        H, nacc = hist.color.copy(), hist.count.copy()                       # still camera: every pixel's only tap is itself
        reuse[:] = True
    elif hist is not None:
        hh, hw = hist.count.shape                                            # (the history's resolution is the current one's)
        r = reproject(hist.cam, cam[0:3], feat, w, h)
        x, nc, ac, ok, x0, y0, fx, fy = r["x"], r["nc"], r["ac"], r["ok"], r["x0"], r["y0"], r["fx"], r["fy"]
        with np.errstate(all="ignore"):
            gx, gy = F(1) - fx, F(1) - fy
            sx2 = F(sigma_x) * F(sigma_x)
            W = np.zeros((h, w), F)
            S = np.zeros((h, w, 3), F)
            Sn = np.zeros((h, w), F)
            keeps, nns, ees, aas = [], [], [], []
            for k in range(4):
                tx, ty = x0 + (k & 1), y0 + (k >> 1)
                wt = (fx if k & 1 else gx) * (fy if k >> 1 else gy)
                keep = ok & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
                tyc, txc = np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)
                thf = hist.hf[tyc, txc]
                keep &= thf != 0
                nt = hist.normal[tyc, txc] / thf[..., None]
                nn = dot(nc, nt)
                keep &= nn >= F(normal_min)
                e = x - hist.position[tyc, txc] / thf[..., None]
                ee = dot(e, e)
                keep &= ee <= sx2
                ea = ac - hist.albedo[tyc, txc] / thf[..., None]
                aa = dot(ea, ea)
                keep &= aa <= F(sigma_albedo) * F(sigma_albedo)
                W = np.where(keep, W + wt, W)
                S = np.where(keep[..., None], S + wt[..., None] * hist.color[tyc, txc], S)
                Sn = np.where(keep, Sn + wt * hist.count[tyc, txc], Sn)
                keeps.append(keep); nns.append(nn); ees.append(ee); aas.append(aa)
            reuse = ok & (W > F(0.01))
            H = np.where(reuse[..., None], S / W[..., None], F(0))
            nacc = np.where(reuse, Sn / W, F(0))
        if trace is not None:
            trace.update(r, W=W, keep=np.array(keeps), nn=np.array(nns), ee=np.array(ees), aa=np.array(aas), reuse=reuse)
    with np.errstate(all="ignore"):
        n = np.fmin(nacc + m, F(max_history) * m)
        alpha = m / n
        blended = H + alpha[..., None] * (cur - H)
    out = np.where(reuse[..., None], blended, cur).astype(F)
    count = np.where(reuse, n, m).astype(F)
    missed = ~reuse & (hf == 0)
    stats = (int(reuse.sum()), int((~reuse & ~missed).sum()), int(missed.sum()))
    return out, History(out, count, feat, cam), stats
