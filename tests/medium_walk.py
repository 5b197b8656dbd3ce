"""A vectorised binary64 random walk of the process the per-lane estimator runs in the two furnaces of
tests/test_gpu_medium_expectation.py (include/ptmi.h: "participating medium"), to estimate on the CPU, before any GPU run, the share
of samples that max_depth cuts: those samples lose what the rest of their path would have collected, so the share bounds the bias
of the furnace's value from below.  Only what decides a path's LENGTH is simulated - free flights, Henyey-Greenstein scattering,
the roulette at depth > 2 (throughput 1: albedo 1 and Kd 1, so it survives with 0.95), the depth count - and no radiance.
  furnace: a closed cube of half-width `half` whose walls have Kd 0: a wall hit ends the path by the throughput exit, not by depth
  sky:     the plane y = 0 with Kd 1 below the medium (a cosine bounce) and nothing else: a miss ends the path"""
import numpy as np


def _slab(lo, hi, o, d, t_end):
    with np.errstate(all="ignore"):
        ta, tb = (lo - o) / d, (hi - o) / d
    par = d == 0
    near = np.where(par, -np.inf, np.minimum(ta, tb)); far = np.where(par, np.inf, np.maximum(ta, tb))
    inside = (~par | ((lo <= o) & (o <= hi))).all(1)
    t0 = np.maximum(near.max(1), 0.0); t1 = np.minimum(far.min(1), t_end)
    return inside & (t1 > t0), t0, t1


def _frame(n):
    a = np.where(np.abs(n[:, :1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    t = np.cross(a, n); t /= np.linalg.norm(t, axis=1, keepdims=True)
    return t, np.cross(n, t)


def _hg_cos(g, u):
    if g == 0:
        return 1.0 - 2.0 * u
    q = (1.0 - g * g) / (1.0 - g + 2.0 * g * u)
    return np.clip((1.0 + g * g - q * q) / (2.0 * g), -1.0, 1.0)


def cut_share(kind, o, d, lo, hi, sigma_t, g, max_depth, seed=1, half=20.0):
    """(cut, n): the samples among the n camera rays (o, d) that reach depth == max_depth"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    o = np.array(o, np.float64); d = np.array(d, np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n = len(o)
    depth = np.zeros(n, int)
    cut = 0
    while len(o):
        # the walk: the surface hit
        with np.errstate(all="ignore"):
            if kind == "furnace":
                t_hit = np.where(d > 0, (half - o) / d, np.where(d < 0, (-half - o) / d, np.inf)).min(1)
                hit = np.ones(len(o), bool)
            else:
                t_hit = np.where(d[:, 1] < 0, -o[:, 1] / d[:, 1], np.inf)
                hit = np.isfinite(t_hit) & (t_hit > 1e-9)
                t_hit = np.where(hit, t_hit, np.inf)
        ok, t0, t1 = _slab(lo, hi, o, d, t_hit)
        tm = t0 - np.log(rng.uniform(size=len(o))) / sigma_t
        mv = ok & (tm < t1)
        alive = mv | (hit if kind == "sky" else np.zeros(len(o), bool))       # a furnace wall or a miss ends the path
        o, d, depth, mv, tm, t_hit = o[alive], d[alive], depth[alive], mv[alive], tm[alive], t_hit[alive]
        keep = (depth <= 2) | (rng.uniform(size=len(o)) <= 0.95)               # the roulette
        o, d, depth, mv, tm, t_hit = o[keep], d[keep], depth[keep], mv[keep], tm[keep], t_hit[keep]
        depth = depth + 1
        done = depth >= max_depth
        cut += int(done.sum())
        o, d, depth, mv, tm, t_hit = o[~done], d[~done], depth[~done], mv[~done], tm[~done], t_hit[~done]
        if not len(o):
            break
        u, v = rng.uniform(size=len(o)), rng.uniform(size=len(o))
        x = o + np.where(mv, tm, t_hit)[:, None] * d
        axis = np.where(mv[:, None], d, [[0.0, 1.0, 0.0]])
        c = np.where(mv, _hg_cos(g, u), np.sqrt(1.0 - u))                      # the phase sample, or the plane's cosine sample
        s = np.sqrt(np.maximum(0.0, 1.0 - c * c))
        t, b = _frame(axis)
        phi = 2.0 * np.pi * v
        d = (s * np.cos(phi))[:, None] * t + (s * np.sin(phi))[:, None] * b + c[:, None] * axis
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        o = np.where(mv[:, None], x, x + 1e-4 * axis)
    return cut, n


def camera_rays(frame12, n, seed=2):
    """n rays of the frame (org, llc, hor, ver) through uniformly random image points"""
    org, llc, hor, ver = np.asarray(frame12, np.float64).reshape(4, 3)
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(size=(n, 1)), rng.uniform(size=(n, 1))
    return np.broadcast_to(org, (n, 3)).copy(), llc + u * hor + v * ver - org
