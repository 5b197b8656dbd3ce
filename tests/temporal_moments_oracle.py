"""Independent numpy restatement of the history's luminance statistics (include/ptmi.h: ptmi_set_temporal_moments) and of the
variance-guided filter steered by them (ptmi_denoise_temporal_variance), written from the header's contract.  The step itself
is temporal_oracle.step, unchanged: its trace gives the taps kept, their weights and W, and the statistics are resampled and
blended beside it.  The filter is variance_oracle's, with its step 2 replaced.  Every value float32 in the header's order; with
T = np.float64 the recurrence alone is evaluated in binary64 (tests/test_temporal_moments_host.py)."""
import numpy as np

import temporal_oracle as TO
import variance_oracle as VO
from denoise_oracle import lum

F = np.float32
MIN_FRAMES = F(4.0)                                                  # PTMI_TEMPORAL_MIN_FRAMES


def blend(mu_h, s2_h, k_h, l, alpha, max_history, T=F):
    """BLEND of the header: (mu, s2, k) from the resampled history, the input's luminance and step 5's alpha"""
    one = T(1)
    d = l - mu_h
    mu = mu_h + alpha * d
    s2 = (one - alpha) * (s2_h + alpha * (d * d))
    k = np.fmin(k_h + one, T(max_history))
    return mu, s2, k


def raw_blend(m1_h, m2_h, l, alpha):
    """the form the contract rejects: the first and second raw moments blended, variance = E[l^2] - E[l]^2"""
    m1 = m1_h + alpha * (l - m1_h)
    m2 = m2_h + alpha * (l * l - m2_h)
    return m1, m2, m2 - m1 * m1


def step(hist, mom, radiance, m, feat, cam, max_history=32, normal_min=0.9, sigma_x=None, sigma_albedo=0.1):
    """temporal_oracle.step with the statistics: mom is (mu, s2, k), each (h, w), or None with an empty history.  Returns
    (radiance out, the new History, stats, the new (mu, s2, k))."""
    trace = {}
    out, new, stats = TO.step(hist, radiance, m, feat, cam, max_history, normal_min, sigma_x, sigma_albedo, trace=trace)
    cur = np.asarray(radiance, F)
    h, w, _ = cur.shape
    cam = np.asarray(cam, F)
    with np.errstate(all="ignore"):
        l = lum(cur)
        zero = np.zeros((h, w), F)
        if hist is None:
            reuse = np.zeros((h, w), bool)
            mu_h = s2_h = k_h = zero
        elif np.array_equal(hist.cam.view(np.uint32), cam.view(np.uint32)) and hist.color.shape == cur.shape:
            reuse = np.ones((h, w), bool)
            mu_h, s2_h, k_h = (np.asarray(a, F) for a in mom)
        else:
            reuse, W, fx, fy, x0, y0 = trace["reuse"], trace["W"], trace["fx"], trace["fy"], trace["x0"], trace["y0"]
            gx, gy = F(1) - fx, F(1) - fy
            S = [zero.copy() for _ in range(3)]
            for t in range(4):
                keep = trace["keep"][t]
                wt = (fx if t & 1 else gx) * (fy if t >> 1 else gy)
                tyc, txc = np.clip(y0 + (t >> 1), 0, h - 1), np.clip(x0 + (t & 1), 0, w - 1)
                for i in range(3):
                    S[i] = np.where(keep, S[i] + wt * np.asarray(mom[i], F)[tyc, txc], S[i])
            mu_h, s2_h, k_h = (np.where(reuse, s / W, F(0)) for s in S)
        mm = np.broadcast_to(np.asarray(m, F), (h, w))
        alpha = mm / new.count                                       # step 5's: n' is the new history's count where reuse holds
        mu, s2, k = blend(mu_h, s2_h, k_h, l, alpha, max_history)
    mu = np.where(reuse, mu, l).astype(F)
    s2 = np.where(reuse, s2, F(0)).astype(F)
    k = np.where(reuse, k, F(1)).astype(F)
    return out, new, stats, (mu, s2, k)


def temporal_variance(c, history, s2, k, T=F):
    """TEMPORAL VARIANCE for every pixel (meaningful where owned(k)); c: the demodulated colour, history: the history's colour"""
    with np.errstate(all="ignore"):
        v = np.fmax(T(0), np.asarray(s2, T) / (np.asarray(k, T) - T(1)))
        lr = lum(np.asarray(history, T))
        s = lum(c) / lr
        return np.where(lr > 0, (v * s) * s, v).astype(T)


def owned(k):
    with np.errstate(invalid="ignore"):
        return np.asarray(k, F) >= MIN_FRAMES                         # a NaN k is the spatial estimate's


def denoise_temporal_variance(history, feat, mom, iterations, sigma_luminance, epsilon, sigma_x, normal_squarings, demodulate=True,
                              spatial_radius=3, source=0):
    """ptmi_denoise_temporal_variance on the history's colour (h, w, 3), its features and (mu, s2, k).  Returns (filtered
    radiance, variance_in, variance_out)."""
    with np.errstate(all="ignore"):
        rad = np.asarray(history, F)
        alb = np.asarray(feat["albedo"], F); nrm = np.asarray(feat["normal"], F); pos = np.asarray(feat["position"], F)
        c = VO.demodulated(rad, alb, demodulate)
        v = VO.spatial_variance(c, nrm, pos, spatial_radius, normal_squarings, sigma_x)
        if source == 0:
            v = np.where(owned(mom[2]), temporal_variance(c, rad, mom[1], mom[2]), v).astype(F)
        if iterations == 0:
            return rad.copy(), v, v.copy()
        c, vo = VO.atrous(c, v, nrm, pos, iterations, sigma_luminance, epsilon, sigma_x, normal_squarings)
        if demodulate:
            nz = alb != 0
            c[nz] = c[nz] * alb[nz]
        return c, v, vo
