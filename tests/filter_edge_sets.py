"""Constructed inputs for the post-processing kernels (csrc/denoise.hip, denoise_variance.hip, temporal.hip): images and feature
buffers in which every data-dependent decision of include/ptmi.h's ptmi_denoise, ptmi_denoise_variance and
ptmi_temporal_accumulate sits at a labelled pixel, given to a context through ptmi_debug_set_filter_inputs.

A set is a dict of arrays (radiance (h, w, 3); feat: albedo, normal, position (h, w, 3), hit_fraction (h, w)) plus
labels: label -> list of pixels (row, column), and declared: label -> how many pixels carry it.  Everything is deterministic
(an integer hash stands in for noise).  tests/test_filter_edge_sets_host.py proves on the restatements alone that each label's
pixel takes the branch the label names; tests/test_gpu_filter_edges.py compares the kernels with the restatements, bit for bit.

  a. atrous_set(w, h)        a piecewise-planar room, a block of misses with one hit inside, labelled radiance and albedo pixels
  b. underflow_set()         a pixel of the variance-guided filter with 0 < W and W * W == 0 in float32
  c. nonfinite_set()         set (a) at 33 x 19 with a NaN and an Inf radiance, a NaN normal and an Inf position
     mixed_infinity_set()    ... with one (+Inf, -Inf, .) radiance: a NaN luminance beside an infinite colour distance
  d. temporal_set(w, h)      two views; the second view's pixels are aimed, by a np.nextafter search on the float32 restatement,
                             at the thresholds of the reprojection, of the bilinear taps and of the acceptance tests
     temporal_nonfinite_set(), temporal_wide_set(w): set (d) with non-finite colours and features; two views 16k +- 1 wide
  WIDE_SIZES                 16383 x 2 and 16385 x 2 for set (a): the ragged last tile of a grid over a thousand workgroups wide
"""
import itertools

import numpy as np

import temporal_oracle as TO
from oracle_binding import camera_frame, default_camera

F = np.float32
INF = F(np.inf)


def up(x, n=1):
    x = F(x)
    for _ in range(n):
        x = np.nextafter(x, INF)
    return x


def dn(x, n=1):
    x = F(x)
    for _ in range(n):
        x = np.nextafter(x, -INF)
    return x


def noise(x, y, k=0):
    """an integer hash of (x, y, k) in [0, 1), a multiple of 2^-16"""
    v = (np.asarray(x, np.int64) * 73856093) ^ (np.asarray(y, np.int64) * 19349663) ^ ((np.asarray(k, np.int64) + 1) * 83492791)
    v = ((v ^ (v >> 13)) & 0x7FFFFFFF) * 1274126177
    return ((v >> 7) & 0xFFFF).astype(F) / F(65536)


def _add(labels, name, pix):
    labels.setdefault(name, []).append((int(pix[0]), int(pix[1])))


# ------------------------------------------------------------------------------------------------
# a. the a-trous family on finite inputs
# ------------------------------------------------------------------------------------------------
ATROUS_SIZES = [(1, 1), (1, 9), (9, 1), (15, 17), (17, 16), (33, 19)]       # (width, height)
ATROUS_FULL = [(15, 17), (17, 16), (33, 19)]                                 # the sizes that hold every label
SIGMA_X = 0.25                                                               # the sets' sigma_position where a case sets no other
ATROUS_LABELS = ("spike", "zero", "denormal", "albedo_zero_channel", "albedo_tiny", "miss", "hit_among_misses", "seam", "partial_hit")

# parameter sets of ptmi_denoise / ptmi_denoise_variance (fields over the defaults, sigma_position = SIGMA_X unless given)
DENOISE_PARAMS = [dict(), dict(normal_squarings=0), dict(normal_squarings=10), dict(iterations=0), dict(iterations=1), dict(iterations=10),
                  dict(demodulate=0), dict(sigma_position=1e-6), dict(sigma_position=1e12), dict(sigma_color=1e-4, color_floor=1e-6),
                  dict(sigma_color=1e4, color_floor=1e-6)]
VARIANCE_PARAMS = [dict(), dict(normal_squarings=0), dict(normal_squarings=10), dict(iterations=0), dict(iterations=1), dict(iterations=10),
                   dict(demodulate=0), dict(spatial_radius=1), dict(spatial_radius=2), dict(sigma_position=1e-6), dict(sigma_position=1e12),
                   dict(epsilon=1e-12)]


DENOISE_DEFAULTS = dict(iterations=5, sigma_color=4.0, color_floor=2.0, sigma_position=SIGMA_X, normal_squarings=7, demodulate=1)
VARIANCE_DEFAULTS = dict(iterations=5, sigma_luminance=2.0, epsilon=0.01, sigma_position=SIGMA_X, normal_squarings=7, demodulate=1, spatial_radius=3)


def restate_denoise(DO, s, prm, **kw):
    """DO.denoise (tests/denoise_oracle.py) on set s with the parameter set prm"""
    p = dict(DENOISE_DEFAULTS, **prm)
    return DO.denoise(s["radiance"], s["feat"], p["iterations"], p["sigma_color"], p["color_floor"], F(p["sigma_position"]), p["normal_squarings"],
                      bool(p["demodulate"]), **kw)


def restate_variance(VO, s, prm, **kw):
    """VO.denoise_variance (tests/variance_oracle.py) on set s with the parameter set prm: (radiance, variance_in, variance_out)"""
    p = dict(VARIANCE_DEFAULTS, **prm)
    return VO.denoise_variance(s["radiance"], s["feat"], p["iterations"], p["sigma_luminance"], p["epsilon"], F(p["sigma_position"]),
                               p["normal_squarings"], bool(p["demodulate"]), p["spatial_radius"], **kw)


def atrous_set(w, h):
    """Set (a).  The room: a floor (normal +y) below a back wall (normal +z), and from two thirds of the width on a side wall
    whose normal (-0.6, 0, 0.8) makes 0.8 with the back wall's (wn = 0.8^(2^k): neither 0 nor 1) and 0 with the floor's."""
    yy, xx = np.mgrid[0:h, 0:w]
    fx, fy = xx.astype(F), yy.astype(F)
    floor = yy < h // 2
    side = (xx >= (2 * w) // 3) & ~floor & (w >= 9)
    nrm = np.zeros((h, w, 3), F); pos = np.zeros((h, w, 3), F); alb = np.zeros((h, w, 3), F)
    nrm[floor] = (0, 1, 0); nrm[~floor] = (0, 0, 1); nrm[side] = (-0.6, 0, 0.8)
    pos[..., 0] = fx * F(0.25); pos[..., 1] = np.where(floor, F(0), (fy - F(h // 2)) * F(0.25)); pos[..., 2] = np.where(floor, (F(h // 2) - fy) * F(0.25), F(0))
    pos[side, 2] = (fx[side] - F((2 * w) // 3)) * F(0.1875)
    alb[floor] = (0.75, 0.75, 0.75); alb[~floor] = (0.25, 0.5, 0.75); alb[side] = (0.75, 0.25, 0.25)
    hf = np.ones((h, w), F)
    shade = F(0.5) + F(0.03) * fx + F(0.02) * fy
    rad = (alb * shade[..., None] * (F(1) + F(0.25) * np.stack([noise(xx, yy, k) for k in range(3)], -1))).astype(F)
    labels = {}
    used = np.zeros((h, w), bool)

    # the block of misses with one hit inside (a hit pixel among misses: every tap but its own weighs 0; a miss: W > 0 fails)
    bw, bh = min(5, w), min(5, h)
    if w * h >= 9:
        bx, by = (w - bw) // 2, (h - bh) // 2 + (1 if h > 9 else 0)
        cy, cx = by + bh // 2, bx + bw // 2
        for y in range(by, by + bh):
            for x in range(bx, bx + bw):
                used[y, x] = True
                if (y, x) == (cy, cx):
                    _add(labels, "hit_among_misses", (y, x))
                    continue
                nrm[y, x] = 0; pos[y, x] = 0; alb[y, x] = 0; hf[y, x] = 0
                rad[y, x] = (0.05, 0.06, 0.07)                    # what a path through the opening would have found
                _add(labels, "miss", (y, x))
    # a pixel half of whose feature rays hit: the sums of the hits times 1 / g^2 (a normal of length 0.5)
    slots = [("partial_hit", 0.2, 0.8), ("spike", 0.2, 0.2), ("zero", 0.8, 0.2), ("denormal", 0.5, 0.1), ("albedo_zero_channel", 0.1, 0.5),
             ("albedo_tiny", 0.9, 0.6), ("seam", 0.3, None)]
    for name, sx, sy in slots:
        x = int(sx * (w - 1) + 0.5)
        y = h // 2 if sy is None else int(sy * (h - 1) + 0.5)     # the seam: the first row of the back wall, its taps cross to the floor
        if used[y, x] or (name == "seam" and h < 2):
            continue
        used[y, x] = True
        _add(labels, name, (y, x))
        if name == "partial_hit":
            nrm[y, x] *= F(0.5); pos[y, x] *= F(0.5); alb[y, x] *= F(0.5); hf[y, x] = F(0.5)
        elif name == "spike":
            rad[y, x] = rad[y, x] * F(1e6)                        # 1e6 x what its neighbours hold
        elif name == "zero":
            rad[y, x] = 0
        elif name == "denormal":
            rad[y, x] = F(1e-40)
        elif name == "albedo_zero_channel":
            alb[y, x, 1] = 0
        elif name == "albedo_tiny":
            alb[y, x] = F(1e-30)
            rad[y, x] = (F(2e-22), F(3e-22), F(1e-22))            # demodulated: ~1e8, whose square a float still holds
    feat = dict(albedo=alb, normal=nrm, position=pos, hit_fraction=hf)
    return dict(width=w, height=h, radiance=rad, feat=feat, labels=labels, declared={k: len(v) for k, v in labels.items()})


def pad_into(s, w, h, x0, y0):
    """set s placed at (x0, y0) of a w x h image of misses (launch geometry: the same pixels in other workgroups and lanes)"""
    rad = np.zeros((h, w, 3), F)
    feat = {k: np.zeros((h, w, 3), F) for k in ("albedo", "normal", "position")}
    feat["hit_fraction"] = np.zeros((h, w), F)
    sl = (slice(y0, y0 + s["height"]), slice(x0, x0 + s["width"]))
    rad[sl] = s["radiance"]
    for k in feat:
        feat[k][sl] = s["feat"][k]
    return dict(width=w, height=h, radiance=rad, feat=feat, labels={}, declared={})


# ------------------------------------------------------------------------------------------------
# b. 0 < W and W * W == 0
# ------------------------------------------------------------------------------------------------
UNDERFLOW_PARAMS = dict(iterations=2, normal_squarings=10, sigma_position=1e-6, spatial_radius=1)


def underflow_set():
    """Set (b), 9 x 9.  Every normal is +z; the labelled pixel's has length s with s^2 = 0.9453 (a pixel 97 % of whose feature rays
    hit), so with normal_squarings = 10 its own tap weighs (s^2)^1024 ~ 1e-25 and its neighbours' (s^1024 ~ 3e-13) are cut to ~1e-25 by
    the position weight (positions a whole unit apart, sigma_position = 1e-6): W ~ 3e-25 > 0 and W * W ~ 1e-49 rounds to 0."""
    w = h = 9
    yy, xx = np.mgrid[0:h, 0:w]
    nrm = np.zeros((h, w, 3), F); nrm[..., 2] = 1
    pos = np.stack([xx.astype(F), yy.astype(F), np.zeros((h, w), F)], -1)
    alb = np.full((h, w, 3), F(0.5))
    hf = np.ones((h, w), F)
    rad = (F(0.25) + F(0.5) * np.stack([noise(xx, yy, k + 7) for k in range(3)], -1)).astype(F)
    p = (4, 4)
    s = F(0.97227)
    nrm[p] = (0, 0, s); pos[p] = pos[p] * s; alb[p] = alb[p] * s; hf[p] = s
    pos[p] = (F(4), F(4), F(0))                                  # (the position stays on the grid: the distances are whole units)
    return dict(width=w, height=h, radiance=rad, feat=dict(albedo=alb, normal=nrm, position=pos, hit_fraction=hf),
                labels={"w_squared_underflows": [p]}, declared={"w_squared_underflows": 1})


# ------------------------------------------------------------------------------------------------
# c. non-finite pixels
# ------------------------------------------------------------------------------------------------
NONFINITE_DENOISE = dict(iterations=2)
NONFINITE_VARIANCE = dict(iterations=2, spatial_radius=1)
NONFINITE_REACH = 7          # spatial_radius + 2 * (2^iterations - 1) = 1 + 6 (ptmi_denoise alone: 6), include/ptmi.h NON-FINITE VALUES


def nonfinite_set():
    """Set (c): (set (a) at 33 x 19 with four pixels made non-finite, the same set without them).  The four lie 28 columns and
    16 rows apart: their reaches (squares of half-width NONFINITE_REACH, clipped by the image) do not overlap, and
    labels["control"] lists the pixels outside all four."""
    clean = atrous_set(33, 19)
    s = atrous_set(33, 19)
    bad = {"nan_radiance": (1, 2), "inf_radiance": (1, 30), "nan_normal": (17, 2), "inf_position": (17, 30)}
    for name, p in bad.items():
        assert all(p not in v for v in s["labels"].values())
        _add(s["labels"], name, p)
    s["radiance"][bad["nan_radiance"]] = (F(np.nan), F(0.5), F(0.25))
    s["radiance"][bad["inf_radiance"]] = (F(0.5), INF, F(0.25))
    s["feat"]["normal"][bad["nan_normal"]] = (F(0), F(np.nan), F(1))
    s["feat"]["position"][bad["inf_position"]] = (F(1), F(1), INF)
    yy, xx = np.mgrid[0:19, 0:33]
    dist = np.min([np.maximum(abs(yy - p[0]), abs(xx - p[1])) for p in bad.values()], axis=0)
    s["labels"]["control"] = [(int(y), int(x)) for y, x in zip(*np.nonzero(dist > NONFINITE_REACH))]
    s["reach"] = {name: np.maximum(abs(yy - p[0]), abs(xx - p[1])) <= NONFINITE_REACH for name, p in bad.items()}
    s["declared"] = {k: len(v) for k, v in s["labels"].items()}
    return s, clean


def mixed_infinity_set():
    """Set (c'), 33 x 19: set (a) with one pixel of radiance (+Inf, -Inf, 1/4).  Its luminance is NaN (Inf - Inf) while its colour
    distance to a finite neighbour is Inf, not NaN: the one input at which the min of ptmi_denoise's colour weight decides.  fminf
    keeps the neighbour's luminance, so wc = 0, W stays finite and the neighbour gets 0 * Inf = NaN in two channels and a finite
    third; a NaN-propagating min would make wc and W NaN and leave the neighbour untouched."""
    s = atrous_set(33, 19)
    p = (5, 12)
    assert all(p not in v and (p[0], p[1] + 1) not in v for v in s["labels"].values())
    _add(s["labels"], "plus_minus_inf_radiance", p)
    s["radiance"][p] = (INF, -INF, F(0.25))
    s["declared"] = {k: len(v) for k, v in s["labels"].items()}
    return s


# 16k +- 1 wide: a grid of more than a thousand workgroups in x with a ragged last tile, the staged tile of ptmi_variance_spatial at
# the far right edge, a row stride of 16k pixels
WIDE_SIZES = [(16383, 2), (16385, 2)]
WIDE_DENOISE_PARAMS = [dict(iterations=1), dict(iterations=2, normal_squarings=0)]
WIDE_VARIANCE_PARAMS = [dict(iterations=1), dict(iterations=2, spatial_radius=1)]


def temporal_wide_set(w, h=2):
    """Two views of the history's surface at a 16k-wide resolution: view A's pixels see it through their centres, view B's hold
    points of it wherever the hash puts them (accepted), misses, and points that project outside.  Same keys as temporal_set."""
    cam_a, cam_b = cameras()
    fa, fb = _frame(cam_a, w, h), _frame(cam_b, w, h)
    n0 = _axis_facing(fa, fb, w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    f64 = fa.astype(np.float64)
    o, llc, hor, ver = f64[0:3], f64[3:6], f64[6:9], f64[9:12]
    point = lambda px, py: o + DEPTH * (llc + ((px + 0.5) / w)[..., None] * hor + ((py + 0.5) / h)[..., None] * ver - o)
    ones = np.ones((h, w), F)
    feat_a = dict(albedo=np.full((h, w, 3), F(0.5)), normal=np.broadcast_to(n0, (h, w, 3)).copy(), position=point(xx.astype(np.float64), yy.astype(np.float64)).astype(F),
                  hit_fraction=ones.copy())
    kind = (xx + 3 * yy) % 8
    px = noise(xx, yy, 3).astype(np.float64) * (w + 1) - 1.0
    py = noise(xx, yy, 5).astype(np.float64) * (h + 1) - 1.0
    px = np.where(kind == 1, w + 3.0, px)
    hit = (kind != 0)
    hfb = hit.astype(F)
    feat_b = dict(albedo=np.full((h, w, 3), F(0.5)) * hfb[..., None], normal=np.broadcast_to(n0, (h, w, 3)) * hfb[..., None],
                  position=point(px, py).astype(F) * hfb[..., None], hit_fraction=hfb)
    rad = lambda k: (F(0.25) + F(2) * np.stack([noise(xx, yy, k + i) for i in range(3)], -1)).astype(F)
    return dict(width=w, height=h, cam_a=cam_a, cam_b=cam_b, frame_a=fa, frame_b=fb, feat_a=feat_a, rad_a=rad(11), feat_b=feat_b, rad_b=rad(23),
                rad_c=rad(37), labels={}, declared={}, tap={}, exact={}, n0=n0)


def temporal_nonfinite_set():
    """Set (d) at 17 x 13 with non-finite values: the history pixel the top-right corner's one tap reads holds a NaN colour (it
    travels with the kept tap, also at alpha = 1), the one the top-left corner's reads +Inf; in view B one filler's position is NaN
    and one's normal Inf (no taps: a restart), and the bottom-right corner's own colour is NaN."""
    d = temporal_set(17, 13)
    d = dict(d, rad_a=d["rad_a"].copy(), rad_b=d["rad_b"].copy(), feat_b={k: v.copy() for k, v in d["feat_b"].items()})
    d["rad_a"][12, 16] = (F(np.nan), F(0.5), F(0.25))
    d["rad_a"][12, 0] = (F(0.5), INF, F(0.25))
    fill = d["labels"]["filler"]
    d["feat_b"]["position"][fill[0]] = (F(np.nan), F(1), F(1))
    d["feat_b"]["normal"][fill[1]] = (INF, F(0), F(0))
    d["rad_b"][d["labels"]["corner_bottom_right"][0]] = (F(0.5), F(np.nan), F(0.25))
    d["nonfinite"] = dict(nan_position=fill[0], inf_normal=fill[1])
    return d


# ------------------------------------------------------------------------------------------------
# d. the temporal step
# ------------------------------------------------------------------------------------------------
TEMPORAL_SIZES = [(1, 1), (17, 13), (33, 19)]
TEMPORAL_SPP = 3
# sigma_position 1 and sigma_albedo 1/8: their squares are exact, so a difference vector (1, 0, 0) or (1/8, 0, 0) sits on the
# threshold.  normal_min: the default's float.
TEMPORAL_PARAMS = dict(normal_min=0.9, sigma_position=1.0, sigma_albedo=0.125, max_history=65536)
TEMPORAL_PARAMS_ZERO_ALBEDO = dict(normal_min=0.9, sigma_position=1.0, sigma_albedo=0.0, max_history=1)
YAW_A, YAW_B = 93.0, 90.0         # the history's view is the oblique one: px and py then answer to all three coordinates
DEPTH = 6.0                  # the history's surface: the points at this multiple of the vectors from the eye to the image plane
W_MIN = F(0.01)


def cameras():
    a, b = default_camera(), default_camera()
    a.yaw_deg, b.yaw_deg = YAW_A, YAW_B
    return a, b


def _frame(cam, w, h):
    return camera_frame(cam, w, h).as_array()


def _point(frame, w, h, px, py, t):
    """binary64 inverse projection: the point at t times the eye-to-image-plane vector through the continuous pixel (px, py)"""
    f = np.asarray(frame, np.float64)
    o, llc, hor, ver = f[0:3], f[3:6], f[6:9], f[9:12]
    return o + t * (llc + ((px + 0.5) / w) * hor + ((py + 0.5) / h) * ver - o)


def _steps(base, offs):
    """base (3,) float32 moved by offs (n, 3) np.nextafter steps per coordinate"""
    return (base.view(np.uint32).astype(np.int64)[None, :] + offs).astype(np.uint32).view(F)


def _cloud(seed, radius):
    """the float32 points within `radius` np.nextafter steps of seed in every coordinate, nearest first"""
    base = np.asarray(seed, np.float64).astype(F)
    offs = np.array(sorted(itertools.product(range(-radius, radius + 1), repeat=3), key=lambda o: (max(map(abs, o)), sum(map(abs, o)), o)), np.int64)
    return _steps(base, offs)


def _sheet(seed, frame, ri, rj):
    """the float32 points i steps along the world axis the frame's horizontal mostly follows and j steps along the vertical's,
    |i| <= ri, |j| <= rj, nearest first: px answers to the one, py to the other, each on a lattice far coarser than the floats
    (q = s d - f is rounded at the size of f and then scaled by width / |hor|), so a target float is met only every few hundred steps"""
    base = np.asarray(seed, np.float64).astype(F)
    ah, av = int(np.argmax(np.abs(frame[6:9]))), int(np.argmax(np.abs(frame[9:12])))
    i, j = np.meshgrid(np.arange(-ri, ri + 1), np.arange(-rj, rj + 1), indexing="ij")
    i, j = i.ravel(), j.ravel()
    order = np.lexsort((np.abs(i) + np.abs(j), np.maximum(np.abs(i), np.abs(j))))
    offs = np.zeros((len(i), 3), np.int64)
    offs[:, ah] += i[order]; offs[:, av] += j[order]
    return _steps(base, offs)


def _aim(frame_a, origin_b, w, h, px, py, want, nc, t=DEPTH):
    """The float32 position near the binary64 inverse projection of (px, py) for which the float32 restatement's values satisfy
    `want` (a function of TO.reproject's dict -> bool array): the nearest in a small cube, else in ever wider sheets of
    np.nextafter steps.  Returns (position, the restatement's values at it)."""
    seed = _point(frame_a, w, h, px, py, t)
    for c in (lambda: _cloud(seed, 2), lambda: _sheet(seed, frame_a, 24, 24), lambda: _sheet(seed, frame_a, 1500, 1),
              lambda: _sheet(seed, frame_a, 1, 1500), lambda: _sheet(seed, frame_a, 300, 300)):
        c = c()
        n = len(c)
        feat = dict(position=c, normal=np.broadcast_to(np.asarray(nc, F), (n, 3)), albedo=np.zeros((n, 3), F), hit_fraction=np.ones(n, F))
        r = TO.reproject(frame_a, origin_b, feat, w, h)
        ok = np.nonzero(want(r))[0]
        if len(ok):
            i = ok[0]
            return c[i], {k: v[i] for k, v in r.items() if np.ndim(v) >= 1 and len(v) == n}
    raise AssertionError("no float32 position within reach of pixel (%r, %r) satisfies the target" % (px, py))


def _axis_facing(frame_a, frame_b, w, h):
    """the axis-aligned unit normal that faces both cameras best from the history's surface"""
    c = _point(frame_a, w, h, (w - 1) / 2, (h - 1) / 2, DEPTH)
    best = max((np.array(v, np.float64) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))),
               key=lambda n: min(n @ (frame_a[0:3] - c), n @ (frame_b[0:3] - c)))
    return best.astype(F)


def temporal_set(w, h, variant=None):
    """Set (d).  View A is the history's: its features are a surface at DEPTH seen through every pixel centre, facing the camera,
    plus the blocks of taps the acceptance cases need.  View B is the current one: every labelled pixel holds a position aimed
    at a reprojection target in view A (the kernel never asks where in view B a pixel's own position lies).  Returns a dict:
      cam_a, cam_b (oracle_binding.Camera), frame_a, frame_b; feat_a, rad_a; feat_b, rad_b; rad_c (a second image for view B, the
      still step); labels (label -> pixels of view B), declared, tap (label -> tap index, for the labels about one tap);
      exact (label -> whether float32 reaches the target exactly); dead_branch / live_branch: the (fn, den) sign pairs.
    variant (1 x 1 only): which single case the only pixel is."""
    cam_a, cam_b = cameras()
    fa, fb = _frame(cam_a, w, h), _frame(cam_b, w, h)
    ob = fb[0:3]
    n0 = _axis_facing(fa, fb, w, h)
    t1 = np.roll(n0, 1)                                           # an axis orthogonal to n0
    a0 = np.array([0.5, 0.5, 0.5], F)
    yy, xx = np.mgrid[0:h, 0:w]
    # ---- view A ----
    pos_a = np.zeros((h, w, 3), F)
    for y in range(h):
        for x in range(w):
            pos_a[y, x] = _point(fa, w, h, x, y, DEPTH).astype(F)
    nrm_a = np.broadcast_to(n0, (h, w, 3)).copy(); alb_a = np.broadcast_to(a0, (h, w, 3)).copy(); hf_a = np.ones((h, w), F)
    rad_a = (F(0.125) + F(2) * np.stack([noise(xx, yy, k + 11) for k in range(3)], -1)).astype(F)
    # ---- view B ----
    pos_b = np.zeros((h, w, 3), F); nrm_b = np.zeros((h, w, 3), F); alb_b = np.zeros((h, w, 3), F); hf_b = np.zeros((h, w), F)
    rad_b = (F(0.25) + F(2) * np.stack([noise(xx, yy, k + 23) for k in range(3)], -1)).astype(F)
    rad_c = (F(0.5) + F(2) * np.stack([noise(xx, yy, k + 37) for k in range(3)], -1)).astype(F)
    labels, tap, exact = {}, {}, {}
    n = w * h
    order = [(i * 7) % n for i in range(n)] if n > 1 else [0]     # where in view B the cases go: spread over the waves
    cursor = [0]

    def place(name, x, nc=n0, alb=a0, hf=1.0, k=None, is_exact=True):
        """the next free pixel of view B gets position x (None: a miss) and the label(s) `name`"""
        p = divmod(order[cursor[0]], w); cursor[0] += 1
        if x is not None:
            pos_b[p] = np.asarray(x, F) * F(hf); nrm_b[p] = np.asarray(nc, F) * F(hf); alb_b[p] = np.asarray(alb, F) * F(hf); hf_b[p] = F(hf)
        for i, nm in enumerate(name if isinstance(name, (list, tuple)) else [name]):
            _add(labels, nm, p)
            if k is not None:
                tap[nm] = k[i] if isinstance(k, (list, tuple)) else k
            exact[nm] = is_exact
        return p

    inside = lambda r: r["ok"]
    fw, fh = F(w), F(h)

    def aim_1d(axis, thr, side, other, t=DEPTH):
        """A position whose px (axis 0) or py (axis 1) is, of all the values the float32 positions around the target reach, the
        one nearest `thr` on `side`: "on" - the smallest >= thr; "above" - the smallest > thr that is not the "on" value; "below" -
        the largest < thr.  Returns (position, whether that value is thr itself / its float neighbour on that side)."""
        key = "px" if axis == 0 else "py"
        seed = _point(fa, w, h, *((float(thr), other) if axis == 0 else (other, float(thr))), t)
        c = np.concatenate([_cloud(seed, 6), _sheet(seed, fa, 1500, 1), _sheet(seed, fa, 1, 1500)])
        feat = dict(position=c, normal=np.broadcast_to(n0, c.shape), albedo=np.zeros_like(c), hit_fraction=np.ones(len(c), F))
        v = TO.reproject(fa, ob, feat, w, h)[key]
        thr = F(thr)
        on = v[v >= thr].min()
        val = {"on": on, "above": v[v > on].min(), "below": v[v < thr].max()}[side]
        good = {"on": val == thr, "above": val == up(thr), "below": val == dn(thr)}[side]
        return c[np.nonzero(v == val)[0][0]], bool(good)

    def cases_1d(axis):
        """the targets of one coordinate (0: px against the width, 1: py against the height); the other coordinate is mid-block"""
        nm, size = ("px", w) if axis == 0 else ("py", h)
        other = 2.5 if (h if axis == 0 else w) > 4 else 0.25
        for name, thr, side in ((nm + "_on_minus1", -1, "on"), (nm + "_below_minus1", -1, "below"), (nm + "_above_minus1", -1, "above"),
                                (nm + "_below_0", 0, "below"), (nm + "_on_0", 0, "on"), (nm + "_below_size", size, "below"), (nm + "_on_size", size, "on")):
            x, good = aim_1d(axis, thr, side, other)
            place(name, x, is_exact=good)
        for name, v in ((nm + "_between_minus1_and_0", -0.5), (nm + "_between_last_and_size", size - 0.5)):
            x, _ = _aim(fa, ob, w, h, *((v, other) if axis == 0 else (other, v)), inside, n0)
            place(name, x)

    if n == 1:
        v = variant or "corner_bottom_left"
        targets = {"corner_bottom_left": (-0.5, -0.5), "corner_top_right": (0.5, 0.5), "inside": (0.25, 0.25), "missed": None}
        if v == "missed":
            place("missed", None)
        else:
            one_d = {"px_on_minus1": (0, -1), "py_on_minus1": (1, -1), "px_on_0": (0, 0), "py_on_0": (1, 0), "px_on_size": (0, 1), "py_on_size": (1, 1)}
            if v in one_d:
                x, good = aim_1d(*one_d[v], "on", 0.25)
            else:
                (x, _), good = _aim(fa, ob, w, h, *targets[v], inside, n0), True
            place(v, x, is_exact=good)
            pos_a[0, 0] = x                                       # the history's only pixel holds the same surface point
    else:
        for axis in (0, 1):
            cases_1d(axis)
        for name, px, py, k in (("corner_bottom_left", -0.5, -0.5, 3), ("corner_bottom_right", w - 0.5, -0.5, 2), ("corner_top_left", -0.5, h - 0.5, 1),
                                ("corner_top_right", w - 0.5, h - 0.5, 0)):
            x, _ = _aim(fa, ob, w, h, px, py, inside, n0)
            place(name, x, k=k)                                   # k: the one tap inside the image
        x, good = aim_1d(0, 7, "on", 2.5)
        place("fx_on_0", x, is_exact=good)                        # px on 7: the taps of column 8 weigh fx = 0 (or next to nothing)
        # W on 0.01f and its neighbours: the block (0, 0) .. (1, 1) keeps its tap (1, 1) alone - (1, 0) and (0, 1) are misses of the
        # history, and (0, 0), the bottom-left corner's tap, lies at another depth, more than sigma_position away
        hf_a[0, 1] = 0; hf_a[1, 0] = 0
        nrm_a[0, 1] = 0; nrm_a[1, 0] = 0; pos_a[0, 1] = 0; pos_a[1, 0] = 0; alb_a[0, 1] = 0; alb_a[1, 0] = 0
        pos_a[0, 0] = _point(fa, w, h, 0, 0, DEPTH - 2.0).astype(F)
        bl = labels["corner_bottom_left"][0]
        xbl, _ = _aim(fa, ob, w, h, -0.5, -0.5, inside, n0, t=DEPTH - 2.0)
        pos_b[bl] = xbl
        for name, wt in (("W_eq_min", W_MIN), ("W_below_min", dn(W_MIN)), ("W_above_min", up(W_MIN))):
            want = lambda r: r["ok"] & (r["x0"] == 0) & (r["y0"] == 0) & (r["fx"] * r["fy"] == wt)
            x = None
            for px, py in ((0.1, 0.1), (0.05, 0.2), (0.2, 0.05), (0.04, 0.25), (0.25, 0.04), (0.08, 0.125), (0.125, 0.08), (0.02, 0.5), (0.5, 0.02)):
                try:                                              # fx * fy = 0.01 is a curve: any point of it will do
                    x, _ = _aim(fa, ob, w, h, px, py, want, n0)
                    break
                except AssertionError:
                    continue
            assert x is not None, name
            place(name, x, k=3)
        # ---- blocks of the acceptance tests: a pixel at the centre of a 2 x 2 block (four taps of weight 1/4), each tap's history
        # on one side of a threshold.  The current pixel sits at DEPTH exactly like the block, so the other tests pass.
        def block(x0, y0):
            x, r = _aim(fa, ob, w, h, x0 + 0.5, y0 + 0.5, lambda r: r["ok"] & (r["x0"] == x0) & (r["y0"] == y0) & (r["fx"] > 0.25) & (r["fx"] < 0.75)
                        & (r["fy"] > 0.25) & (r["fy"] < 0.75), n0)
            return x, [(y0 + (k >> 1), x0 + (k & 1)) for k in range(4)]

        # the history's hit fraction: 0, 1/4, 1/4 and 1 (features are sums over the hits: scaled with it)
        x, taps = block(13, 5)
        hf_a[taps[0]] = 0; nrm_a[taps[0]] = 0; pos_a[taps[0]] = 0; alb_a[taps[0]] = 0
        for k in (1, 2):
            hf_a[taps[k]] = F(0.25); nrm_a[taps[k]] = n0 * F(0.25); pos_a[taps[k]] = x * F(0.25); alb_a[taps[k]] = a0 * F(0.25)
        pos_a[taps[3]] = x
        place(["tap_hf_eq_0", "tap_hf_quarter"], x, k=[0, 1])
        place("both_hf_quarter", x, hf=0.25, k=2)
        # dot(n_c, n_t) on normal_min, below, above: n_t = c n0 + sqrt(1 - c^2) t1 has n0 . n_t = c exactly
        nmin = F(TEMPORAL_PARAMS["normal_min"])
        x, taps = block(4, 5)
        for k, c in ((0, nmin), (1, dn(nmin)), (2, up(nmin))):
            nrm_a[taps[k]] = c * n0 + F(np.sqrt(1.0 - float(c) ** 2)) * t1
            pos_a[taps[k]] = x
        pos_a[taps[3]] = x
        place(["normal_eq_min", "normal_below_min", "normal_above_min"], x, k=[0, 1, 2])
        # dot(e, e) on sigma_x^2 = 1, below, above: e = (1, 0, 0) turned to the axes n0 and t1
        x, taps = block(7, 5)
        sx2 = F(TEMPORAL_PARAMS["sigma_position"]) * F(TEMPORAL_PARAMS["sigma_position"])
        found = _threshold_vectors(x, n0, t1, F(1), sx2)
        for k, key in ((0, "eq"), (1, "above"), (2, "below")):
            pos_a[taps[k]] = found[key][0]
        pos_a[taps[3]] = x
        place(["position_eq_sigma", "position_above_sigma", "position_below_sigma"], x, k=[0, 1, 2], is_exact=found["above"][1] and found["below"][1])
        # dot(ea, ea) on sigma_a^2 = 1/64
        x, taps = block(10, 5)
        sa2 = F(TEMPORAL_PARAMS["sigma_albedo"]) * F(TEMPORAL_PARAMS["sigma_albedo"])
        found = _threshold_vectors(a0, np.array([1, 0, 0], F), np.array([0, 1, 0], F), F(TEMPORAL_PARAMS["sigma_albedo"]), sa2)
        for k, key in ((0, "eq"), (1, "above"), (2, "below")):
            alb_a[taps[k]] = found[key][0]
        for k in range(4):
            pos_a[taps[k]] = x
        place(["albedo_eq_sigma", "albedo_above_sigma", "albedo_below_sigma", "albedo_equal"], x, k=[0, 1, 2, 3], is_exact=found["above"][1] and found["below"][1])
        # a surface seen from its back in both views: n_c = -n0 and a history that agrees
        x, taps = block(4, 8)
        for k in range(4):
            nrm_a[taps[k]] = -n0; pos_a[taps[k]] = x
        place("back_in_both_views", x, nc=-n0)
        # ---- the current pixel itself
        place("missed", None)
        x, _ = _aim(fa, ob, w, h, 9.25, 9.4, inside, n0)
        place("current_hf_quarter", x, hf=0.25)
        # behind the previous camera: the mirror image of a visible point through the eye; den changes its sign
        place("behind_previous_camera", _point(fa, w, h, 8.0, 6.0, -DEPTH).astype(F), nc=n0)
        # the two eyes on different sides of the surface: a normal along the line from eye B to eye A, through a point between them
        oa64, ob64 = fa[0:3].astype(np.float64), fb[0:3].astype(np.float64)
        nb = (oa64 - ob64) / np.linalg.norm(oa64 - ob64)
        vd = _point(fa, w, h, (w - 1) / 2, (h - 1) / 2, 1.0) - oa64
        x = (oa64 + ob64) / 2 + DEPTH * (vd - (vd @ nb) * nb)
        place("back_in_one_view", x.astype(F), nc=nb.astype(F))
        # ---- the rest: points of the history's surface wherever the hash puts them (no label claims anything), misses, and
        # points that project far outside
        while cursor[0] < n:
            i = cursor[0]
            kind = i % 8
            if kind == 0:
                place("filler_missed", None)
            elif kind == 1:
                place("filler_outside", _point(fa, w, h, w + 3.0 + i % 5, -4.0, DEPTH).astype(F))
            else:
                px = float(noise(i, 1, 3)) * (w + 1) - 1.0
                py = float(noise(i, 2, 5)) * (h + 1) - 1.0
                place("filler", _point(fa, w, h, px, py, DEPTH).astype(F))
    feat_a = dict(albedo=alb_a, normal=nrm_a, position=pos_a, hit_fraction=hf_a)
    feat_b = dict(albedo=alb_b, normal=nrm_b, position=pos_b, hit_fraction=hf_b)
    # the sign of fn = dot(llc - o, cross(hor, ver)) is the frame's handedness: one of the two (fn, den) pairs cannot occur
    fn = TO.dot(fa[3:6] - fa[0:3], TO.cross(fa[6:9], fa[9:12]))
    live, dead = ("fn>0,den>0", "fn<0,den<0") if fn > 0 else ("fn<0,den<0", "fn>0,den>0")
    return dict(width=w, height=h, cam_a=cam_a, cam_b=cam_b, frame_a=fa, frame_b=fb, feat_a=feat_a, rad_a=rad_a, feat_b=feat_b, rad_b=rad_b,
                rad_c=rad_c, labels=labels, declared={k: len(v) for k, v in labels.items()}, tap=tap, exact=exact, live_branch=live,
                dead_branch=dead, n0=n0)


def _threshold_vectors(x, e1, e2, length, bound):
    """History values y near x - length * e1 whose d = x - y gives dot(d, d) == bound ("eq"), the float above ("above") and the float
    below ("below"), found by stepping y along e1 by np.nextafter steps and along e2 by small dyadic amounts.  Returns
    key -> (y, whether dot(d, d) is exactly that value; where not, the nearest value on that side)."""
    x = np.asarray(x, F)
    i1, i2 = int(np.argmax(np.abs(e1))), int(np.argmax(np.abs(e2)))
    s1 = F(np.sign(e1[i1]))
    seen = {}
    for k1 in range(-6, 7):
        for k2 in [0.0] + [j * 2.0 ** -e for e in (12, 15, 18, 21) for j in range(1, 65)]:
            y = x.copy()
            v = F(x[i1] - s1 * length)
            for _ in range(abs(k1)):
                v = np.nextafter(v, INF if k1 > 0 else -INF)
            y[i1] = v
            y[i2] = F(x[i2] - F(k2))
            d = x - y
            dd = TO.dot(d, d)
            seen.setdefault(F(dd), y)
    vals = np.array(sorted(seen))
    out = {"eq": (seen[F(bound)], True)}
    above = vals[vals > bound].min(); below = vals[vals < bound].max()
    out["above"] = (seen[F(above)], bool(above == up(bound)))
    out["below"] = (seen[F(below)], bool(below == dn(bound)))
    return out


# what each label of set (d) must come to in the second step: (has taps at all, reused)
TEMPORAL_VERDICTS = {
    "px_on_minus1": (True, False), "px_below_minus1": (False, False), "px_above_minus1": (True, False), "px_between_minus1_and_0": (True, True),
    "px_below_0": (True, True), "px_on_0": (True, True), "px_between_last_and_size": (True, True), "px_below_size": (True, False),
    "px_on_size": (False, False),
    "py_on_minus1": (True, False), "py_below_minus1": (False, False), "py_above_minus1": (True, False), "py_between_minus1_and_0": (True, True),
    "py_below_0": (True, True), "py_on_0": (True, True), "py_between_last_and_size": (True, True), "py_below_size": (True, False),
    "py_on_size": (False, False),
    "corner_bottom_left": (True, True), "corner_bottom_right": (True, True), "corner_top_left": (True, True), "corner_top_right": (True, True),
    "fx_on_0": (True, True), "W_eq_min": (True, False), "W_below_min": (True, False), "W_above_min": (True, True),
    "tap_hf_eq_0": (True, True), "tap_hf_quarter": (True, True), "both_hf_quarter": (True, True),
    "normal_eq_min": (True, True), "normal_below_min": (True, True), "normal_above_min": (True, True),
    "position_eq_sigma": (True, True), "position_above_sigma": (True, True), "position_below_sigma": (True, True),
    "albedo_eq_sigma": (True, True), "albedo_above_sigma": (True, True), "albedo_below_sigma": (True, True), "albedo_equal": (True, True),
    "back_in_both_views": (True, True), "missed": (False, False), "current_hf_quarter": (True, True),
    "behind_previous_camera": (False, False), "back_in_one_view": (False, False),
}
# per tap: whether the tap named by tap[label] is kept
TEMPORAL_TAP_KEPT = {
    "tap_hf_eq_0": False, "tap_hf_quarter": True, "both_hf_quarter": True,
    "normal_eq_min": True, "normal_below_min": False, "normal_above_min": True,
    "position_eq_sigma": True, "position_above_sigma": False, "position_below_sigma": True,
    "albedo_eq_sigma": True, "albedo_above_sigma": False, "albedo_below_sigma": True, "albedo_equal": True,
}
