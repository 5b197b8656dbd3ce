"""Constructed inputs for the kernels that turn a radiosity solution into the records guided sampling reads
(csrc/radiosity.hip: ptmi_cdf_records<0|1|2>, ptmi_filter_pdfs, ptmi_radiosity_grid), given to a context through
ptmi_debug_cdf_records, ptmi_debug_filter_pdfs and ptmi_debug_radiosity_grid, and the restatements they are compared with.

The restatements are numpy, one rounded operation per line of the reference, written from grid.h:88-134 / application_state.h
:509-571 (records), grid_filter.h:35-41 and the float filters + normalize_pdf_kernel behind "Apply Filter & Rebuild CDFs"
(filter), form_factors.h:408-442 and bilateralFilterCell / gaussianFilterCell (grid update).  exp is the contract's ptmi_expf
through po_math_batch, the cell of a direction is po_direction_to_grid_index; everything else is IEEE arithmetic of numpy's.
Each restatement takes the number type T: np.float32 is THE restatement (bit for bit what the kernels must give), np.float64
the same formulas in binary64, against which tests/test_guided_record_sets_host.py bounds the float32 one.

  record_set()   dict(labels, pdf (m, 256), rgb (m, 256, 3), has_rgb (m,)): one grid per label.  pdf is what kind 2 takes;
                 rgb, where has_rgb, is a grid whose restated luminance is pdf bit for bit (kinds 0 and 1)
  filter_set()   list of dict(label, grid (256,), rgb (256, 3), sigma_spatial, sigma_range, designed): a float grid, given as
                 counts, and an rgb grid with that luminance; run with the Gaussian and the bilateral filter
  grid_worlds()  list of dict(label, centre, normal, ff, rad, filtering): one small world per case

Measured against the binary64 restatement over the ordinary cases (tests/test_guided_record_sets_host.py prints them):
  records  9.0e-07   the largest relative error of a row sum, a CDF entry or the total (RECORD_BOUND is four times that)
  filter   6.9e-07   ... of a normalised pdf value (FILTER_BOUND)
  grid     1.3e-06   ... of a grid cell's component (GRID_BOUND)
"""
import numpy as np

from oracle_binding import math_batch, oracle_lib

F = np.float32
D = np.float64
INF = F(np.inf)
NAN = F(np.nan)
EPS_TOTAL = F(1e-6)          # total_weight > 1e-6f, row_sum < 1e-6f, r < 1e-6f, total filter weight > 1e-6f
EPS_SUM = F(1e-12)           # normalize_pdf_kernel: sum <= 1e-12f leaves the values as they are
LUM = (F(0.2126), F(0.7152), F(0.0722))
MATH_EXPF = 7                # PTMI_MATH_EXPF of po_math_batch
RECORD_BOUND, FILTER_BOUND, GRID_BOUND = 4 * 9.0e-7, 4 * 6.9e-7, 4 * 1.3e-6

def quiet():
    return np.errstate(all="ignore")


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


def noise(i, k=0):
    """an integer hash of (i, k) in [0, 1), a multiple of 2^-16"""
    v = (np.asarray(i, np.int64) * 73856093) ^ ((np.asarray(k, np.int64) + 1) * 83492791)
    v = ((v ^ (v >> 13)) & 0x7FFFFFFF) * 1274126177
    return ((v >> 7) & 0xFFFF).astype(F) / F(65536)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    """bit for bit, NaN counted equal to NaN"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def first_float(pred, lo=0.0, hi=3e38):
    """the smallest float32 x in [lo, hi] (both >= 0) with pred(x), pred being monotone (False ... True); None if pred(hi) fails"""
    a, b = int(F(lo).view(np.uint32)), int(F(hi).view(np.uint32))
    if not pred(np.uint32(b).view(F)):
        return None
    while a < b:
        m = (a + b) // 2
        if pred(np.uint32(m).view(F)):
            b = m
        else:
            a = m + 1
    return np.uint32(a).view(F)


# ------------------------------------------------------------------------------------------------
# restatements
# ------------------------------------------------------------------------------------------------
def luminance(rgb, T=F):
    """luminanceFromRGB (grid_filter.h:39-41; grid.h:68-70): ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b)"""
    rgb = np.asarray(rgb, T)
    with quiet():
        return (T(LUM[0]) * rgb[..., 0] + T(LUM[1]) * rgb[..., 1]) + T(LUM[2]) * rgb[..., 2]


def luminance_fused(rgb):
    """the same expression as a compiler that contracts would evaluate it: fma(c2, b, fma(c1, g, c0 * r)), each fma rounded once.
    The products of two float32 are exact in binary64; the sum's one rounding to binary64 before the rounding to float32 can
    only matter on a tie, which fused_differs_exactly() rules out for the cells it names."""
    rgb = np.asarray(rgb, D)
    with quiet():
        t = (D(LUM[0]) * rgb[..., 0]).astype(F)
        t = (D(LUM[1]) * rgb[..., 1] + t.astype(D)).astype(F)
        return (D(LUM[2]) * rgb[..., 2] + t.astype(D)).astype(F)


def fused_differs_exactly(rgb_cell):
    """exact rational arithmetic: does the fused evaluation of one cell differ from the rounded one?"""
    from fractions import Fraction as Q

    def rnd(q):                                         # round a rational to float32, ties to even
        f = F(float(q))                                 # a neighbour of the answer at worst; the exact distances decide
        cands = sorted((abs(Q(float(c)) - q), int(c.view(np.uint32)) & 1, float(c)) for c in (dn(f), f, up(f)))
        return F(cands[0][2])
    c = [Q(float(x)) for x in LUM]; v = [Q(float(x)) for x in rgb_cell]
    plain = rnd(Q(float(rnd(Q(float(rnd(c[0] * v[0]))) + Q(float(rnd(c[1] * v[1])))))) + Q(float(rnd(c[2] * v[2]))))
    fused = rnd(c[2] * v[2] + Q(float(rnd(c[1] * v[1] + Q(float(rnd(c[0] * v[0])))))))
    return plain != fused


def restate_records(pdf, T=F, row_sum_lt=None, valid_gt=None, divide=False, force_last=True, descending=False):
    """grid.h:88-134 (buildCDFs) for the upper hemisphere, application_state.h:560-565 for the lower: (m, 530) words in the
    PrecomputedCDF layout (pdf 0, row_sums 256, marginal_cdf 264, row_cdfs 272, total_weight 528, is_valid 529).  For T = float64
    the words are float64 and is_valid is 0.0 / 1.0.  The keyword arguments are the MUTANTS of the issue, for the host test that
    shows the sets can tell them: row_sum_lt / valid_gt replace the comparison, divide uses running / sum, force_last = False
    drops the forced marginal[7] = 1, descending sums a row from u = 15 down."""
    pdf = np.asarray(pdf, T).reshape(-1, 16, 16)
    m = len(pdf)
    eps = T(EPS_TOTAL); inv_res = T(1.0 / 16)
    out = np.zeros((m, 530), T)
    with quiet():
        row_sums = np.zeros((m, 8), T)
        for v in range(8):
            s = np.zeros(m, T)
            for u in (range(15, -1, -1) if descending else range(16)):
                s = s + pdf[:, v, u]
            row_sums[:, v] = s
        total = np.zeros(m, T)
        for v in range(8):
            total = total + row_sums[:, v]
        inv_total = np.where(total > eps, T(1) / total, T(0)).astype(T)
        marginal = np.zeros((m, 8), T)
        running = np.zeros(m, T)
        for v in range(8):
            running = running + row_sums[:, v]
            marginal[:, v] = running / total if divide else running * inv_total
        if divide:
            marginal[~(total > eps)] = 0                  # inv_total = 0: the mutant divides only where the original inverts
        if force_last:
            marginal[:, 7] = 1
        rows = np.zeros((m, 16, 16), T)
        uniform = (np.arange(1, 17).astype(T) * inv_res).astype(T)
        for v in range(8):
            rs = row_sums[:, v]
            small = (rs <= eps) if row_sum_lt == "le" else (rs < eps)
            inv = T(1) / rs
            run = np.zeros(m, T)
            for u in range(16):
                run = run + pdf[:, v, u]
                rows[:, v, u] = run / rs if divide else run * inv
            rows[:, v, 15] = 1
            rows[small, v, :] = uniform
        rows[:, 8:, :] = uniform
        valid = (total >= eps) if valid_gt == "ge" else (total > eps)
    out[:, 0:256] = pdf.reshape(m, 256); out[:, 256:264] = row_sums; out[:, 264:272] = marginal
    out[:, 272:528] = rows.reshape(m, 256); out[:, 528] = total
    if T is F:
        out[:, 529] = valid.astype(np.int32).view(F)
    else:
        out[:, 529] = valid
    return out


def expf(x):
    """ptmi_expf of the contract (include/ptmi_math.h) on a float32 array"""
    x = np.ascontiguousarray(x, F)
    return math_batch(MATH_EXPF, x.reshape(-1))[:, 0].astype(F).reshape(x.shape)


def gaussian_weight(distance, sigma, T=F):
    """grid_filter.h:35-37: expf(-(distance * distance) / (2.0f * sigma * sigma))"""
    distance = np.asarray(distance, T); sigma = T(sigma)
    with quiet():
        arg = -(distance * distance) / (T(2) * sigma * sigma)
        return expf(arg) if T is F else np.exp(arg)


def _taps():
    """(di, dj, distance) in the loop order of the 5 x 5 window; distance = sqrtf((float)(di * di + dj * dj))"""
    return [(di, dj, np.sqrt(F(di * di + dj * dj))) for di in range(-2, 3) for dj in range(-2, 3)]


def restate_filter_float(src, bilateral, sigma_spatial, sigma_range, T=F, clamp_phi=False):
    """gaussianFilterCellFloat / bilateral_filter_float_kernel (grid_filter.h) on (m, 256) grids: phi (columns) wraps, theta (rows)
    does not; a total weight that is not > 1e-6f leaves the centre value.  clamp_phi: the MUTANT that clamps the column."""
    src = np.asarray(src, T).reshape(-1, 16, 16); m = len(src)
    ws = np.zeros((m, 16, 16), T); tw = np.zeros((m, 16, 16), T)
    ii, jj = np.mgrid[0:16, 0:16]
    with quiet():
        for di, dj, dist in _taps():
            ni = ii + di
            nj = np.clip(jj + dj, 0, 15) if clamp_phi else (jj + dj + 16) % 16
            ok = (ni >= 0) & (ni < 16)
            nb = src[:, np.clip(ni, 0, 15), nj]
            w = gaussian_weight(T(dist), sigma_spatial, T)
            if bilateral:
                w = w * gaussian_weight(np.abs(src - nb), sigma_range, T)
            ws = np.where(ok, ws + nb * w, ws)
            tw = np.where(ok, tw + w, tw)
        out = np.where(tw > T(EPS_TOTAL), ws / tw, src)
    return out.reshape(m, 256).astype(T)


def restate_normalize(f, T=F, le=True, pairwise=False):
    """normalize_pdf_kernel: the sequential sum of the 256 values; a sum <= 1e-12f leaves them.  le = False: the MUTANT `<`;
    pairwise: the MUTANT that sums as a tree."""
    f = np.asarray(f, T).reshape(-1, 256)
    with quiet():
        if pairwise:
            t = f.copy()
            while t.shape[1] > 1:
                t = t[:, 0::2] + t[:, 1::2]
            s = t[:, 0]
        else:
            s = np.zeros(len(f), T)
            for c in range(256):
                s = s + f[:, c]
        keep = (s <= T(EPS_SUM)) if le else (s < T(EPS_SUM))
        return np.where(keep[:, None], f, f / s[:, None]).astype(T), s


def restate_filter_pdfs(rgb, counts, bilateral, sigma_spatial, sigma_range, T=F, **mutant):
    """"Apply Filter & Rebuild CDFs" up to the pdfs: (formfactor from the counts, radiosity from the luminance), (m, 256) each"""
    lum = luminance(rgb, T).reshape(-1, 256)
    cnt = np.zeros_like(lum) if counts is None else np.asarray(counts, T).reshape(-1, 256)
    norm = {k: v for k, v in mutant.items() if k in ("le", "pairwise")}
    filt = {k: v for k, v in mutant.items() if k in ("clamp_phi",)}
    ff = restate_normalize(restate_filter_float(cnt, bilateral, sigma_spatial, sigma_range, T, **filt), T, **norm)[0]
    rad = restate_normalize(restate_filter_float(lum, bilateral, sigma_spatial, sigma_range, T, **filt), T, **norm)[0]
    return ff, rad


def _div_scalar(v, t, T):
    """vector.h:90-94, 189-195: division by a scalar multiplies by T k = 1.0 / t (the binary64 quotient rounded to T)"""
    with quiet():
        k = (D(1.0) / np.asarray(t, D)).astype(T)
        return (np.asarray(v, T) * k[..., None]).astype(T)


def restate_filter_rgb(grid, bilateral, sigma_spatial, sigma_range, T=F):
    """bilateralFilterCell / gaussianFilterCell (grid_filter.h:54-101) on one (256, 3) grid"""
    g = np.asarray(grid, T).reshape(16, 16, 3)
    lum = luminance(g, T)
    ws = np.zeros((16, 16, 3), T); tw = np.zeros((16, 16), T)
    ii, jj = np.mgrid[0:16, 0:16]
    with quiet():
        for di, dj, dist in _taps():
            ni = ii + di; nj = (jj + dj + 16) % 16
            ok = (ni >= 0) & (ni < 16)
            nb = g[np.clip(ni, 0, 15), nj]
            w = np.broadcast_to(gaussian_weight(T(dist), sigma_spatial, T), (16, 16)).astype(T)
            if bilateral:
                w = w * gaussian_weight(np.abs(lum - lum[np.clip(ni, 0, 15), nj]), sigma_range, T)
            ws = np.where(ok[..., None], ws + w[..., None] * nb, ws)
            tw = np.where(ok, tw + w, tw)
        out = np.where((tw > T(EPS_TOTAL))[..., None], _div_scalar(ws, tw, T), g)
    return out.reshape(256, 3).astype(T)


def grid_index(direction, normal):
    """direction_to_grid_indices_local (form_factors.h:107-130) as the oracle's C states it, on float32 vectors"""
    d = np.ascontiguousarray(direction, F); n = np.ascontiguousarray(normal, F)
    return oracle_lib().po_direction_to_grid_index(d.ctypes.data, n.ctypes.data)


def world_geometry(w, i, T=F):
    """per source j of receiver i, as update_radiosity_grid computes them in float32: (r (n,), unit directions (n, 3))"""
    c = np.asarray(w["centre"], F)
    with quiet():
        d = (c - c[i]).astype(F)
        s = np.zeros(len(c), F)
        for k in range(3):
            s = s + d[:, k] * d[:, k]
        r = np.sqrt(s)
        return r, _div_scalar(d, r, F)


def restate_grid_update(w, T=F, take="not_le", r_skip="lt", descending=False, skip_self=True):
    """update_radiosity_grid (form_factors.h:408-442) + the optional rgb filter, on world w: (n, 256, 3).  The geometry (the
    distance, the unit direction, the cell) is float32 for either T - a cell is a decision, not a value; the sums are T's.
    MUTANTS: take = "gt" (F_ij > 0 instead of not F_ij <= 0), r_skip = "le", descending j, skip_self = False."""
    n = len(w["centre"])
    ff = np.asarray(w["ff"], F); rad = np.asarray(w["rad"], T)
    out = np.zeros((n, 256, 3), T)
    with quiet():
        for i in range(n):
            row = ff[i]
            taken = (row > 0) if take == "gt" else ~(row <= 0)
            if skip_self:
                taken[i] = False
            if not taken.any():
                continue
            r, dirs = world_geometry(w, i)
            taken &= ~((r <= EPS_TOTAL) if r_skip == "le" else (r < EPS_TOTAL))
            js = np.flatnonzero(taken)
            for j in (js[::-1] if descending else js):
                c = grid_index(dirs[j], w["normal"][i])
                out[i, c] = out[i, c] + T(row[j]) * rad[j]
            if w.get("filtering") is not None:
                bil, ss, sr = w["filtering"]
                out[i] = restate_filter_rgb(out[i], bil, ss, sr, T)
    return out


# ------------------------------------------------------------------------------------------------
# rgb grids with a given luminance
# ------------------------------------------------------------------------------------------------
def rgb_for_luminance(lum):
    """(rgb (..., 3), found (...)): per value a single-channel rgb whose restated luminance is the value bit for bit - the other
    two products are +0 and (0 + p) + 0 == p.  A channel c reaches v where some float x near v / c has fl(c * x) == v; the
    three channels are tried in turn.  Not found (found False, rgb 0): -0 (the sum gives +0), and the few values no channel hits."""
    lum = np.asarray(lum, F); flat = lum.reshape(-1)
    rgb = np.zeros((flat.size, 3), F); found = np.zeros(flat.size, bool)
    with quiet():
        for ch in (1, 0, 2):
            x0 = (flat / LUM[ch]).astype(F)
            for step in (0, 1, -1, 2, -2, 3, -3):
                x = x0.copy()
                for _ in range(abs(step)):
                    x = np.nextafter(x, F(np.inf) if step > 0 else F(-np.inf)).astype(F)
                cand = np.zeros((flat.size, 3), F); cand[:, ch] = x
                hit = ~found & same_each(luminance(cand), flat) & ~(np.signbit(flat) & (flat == 0))
                rgb[hit] = cand[hit]; found |= hit
        for step in (0, 1, -1, 2, -2, 3, -3):             # a grey x: values too large for one channel (x / c overflows)
            x = flat.copy()
            for _ in range(abs(step)):
                x = np.nextafter(x, F(np.inf) if step > 0 else F(-np.inf)).astype(F)
            cand = np.stack([x, x, x], 1)
            hit = ~found & same_each(luminance(cand), flat) & ~(np.signbit(flat) & (flat == 0))
            rgb[hit] = cand[hit]; found |= hit
    return rgb.reshape(lum.shape + (3,)), found.reshape(lum.shape)


def same_each(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------------------------------------
# 1. records
# ------------------------------------------------------------------------------------------------
N_RANDOM = 300
# the valid edge records whose SAMPLING is recorded from the compiled reference and replayed on the device
SAMPLED = ("inf_cell", "negative_rows", "total_above", "row_sum_below", "row_3e38")


def base_grid(k=0, scale=1.0):
    """a positive 16 x 16 grid of hashed values in [0.25, 1.25) * scale"""
    return ((noise(np.arange(256), k) + F(0.25)) * F(scale)).astype(F).reshape(16, 16)


def _total(g):
    return restate_records(g.reshape(1, 256))[0, 528]


def _with(g, cell, x):
    h = g.copy(); h[cell] = x
    return h


def record_edge_grids():
    """[(label, pdf (16, 16))].  tests/test_guided_record_sets_host.py proves each label on the restatement."""
    out = []
    # total_weight at 1e-6f: one cell of a grid whose other cells sum to about 0.9e-6 is searched float by float
    g = base_grid(1, 0.9e-6 / 96)
    cell = (3, 5)
    above = first_float(lambda x: _total(_with(g, cell, x)) > EPS_TOTAL, 0, 1e-6)
    at = first_float(lambda x: _total(_with(g, cell, x)) >= EPS_TOTAL, 0, 1e-6)
    out += [("total_below", _with(g, cell, dn(at))), ("total_at", _with(g, cell, at)), ("total_above", _with(g, cell, above))]
    # row_sum at 1e-6f inside a grid that is otherwise valid
    g = base_grid(2)
    g[2] = base_grid(3, 0.9e-6 / 12)[2]
    rs = lambda x: restate_records(_with(g, (2, 9), x).reshape(1, 256))[0, 256 + 2]
    at = first_float(lambda x: rs(x) >= EPS_TOTAL, 0, 1e-6)
    above = first_float(lambda x: rs(x) > EPS_TOTAL, 0, 1e-6)
    out += [("row_sum_below", _with(g, (2, 9), dn(at))), ("row_sum_at", _with(g, (2, 9), at)), ("row_sum_above", _with(g, (2, 9), above))]
    # sums whose order matters: 2^24 + 1 + 1 ... stays 2^24 term by term, 1 + ... + 1 + 2^24 does not
    big = F(2.0 ** 24)
    g = base_grid(4); g[1] = 1; g[1, 0] = big; g[5] = 1; g[5, 15] = big
    out.append(("row_order", g))
    g = np.zeros((16, 16), F); g[0, 3] = big; g[1:8, 4] = 1
    out.append(("marginal_order_head", g))
    g = np.zeros((16, 16), F); g[7, 3] = big; g[0:7, 4] = 1
    out.append(("marginal_order_tail", g))
    # a row where running * (1 / row_sum) differs from running / row_sum: the first hashed grid that has one in every upper row
    for k in range(10, 200):
        g = base_grid(k)
        a = restate_records(g.reshape(1, 256))[0, 272:400]; b = restate_records(g.reshape(1, 256), divide=True)[0, 272:400]
        if (bits(a) != bits(b)).reshape(8, 16).any(axis=1).all():
            break
    out.append(("inverse_not_quotient", g))
    # the entry before the forced final 1.0f lies above it.  With cells >= 0 it cannot: row_sum * fl(1 / row_sum) is 1 + e with
    # |e| <= 2^-24, which rounds to at most 1.0f; a negative last cell puts running[14] above row_sum
    g = base_grid(5); g[3, 15] = F(-0.5); g[6, 15] = F(-1e-3)
    out.append(("penultimate_above_one", g))
    for r in range(8):
        g = np.zeros((16, 16), F); g[r, (5 * r + 3) % 16] = F(0.75)
        out.append((f"one_hot_row{r}", g))
    g = np.zeros((16, 16), F); g[12, 7] = 1
    out.append(("one_hot_lower", g))
    out.append(("zero", np.zeros((16, 16), F)))
    out.append(("denormal", (np.arange(1, 257).astype(F) * F(1e-45)).reshape(16, 16)))
    g = base_grid(6); g[4] = luminance(np.full(3, 3e38, F))           # the luminance of the grey (3e38, 3e38, 3e38): about 3e38
    out.append(("row_3e38", g))
    out.append(("nan_cell", _with(base_grid(7), (2, 11), NAN)))
    out.append(("inf_cell", _with(base_grid(8), (5, 2), INF)))
    g = base_grid(9); g[1, 3::4] = F(-0.9); g[6, 2] = F(-3.0); g[6, 9] = F(-0.125)
    out.append(("negative_rows", g))
    g = lum_of_g((F(10.0) ** (noise(np.arange(256), 11) * F(24) - F(12))).astype(F)).reshape(16, 16)   # a luminance some rgb has
    out.append(("decades_24", g))
    return out


def random_rgb_grids():
    """N_RANDOM rgb grids over many scales; a third sparse (zero cells, empty rows)"""
    rng = np.random.default_rng(20)
    g = rng.uniform(0, 1, (N_RANDOM, 16, 16, 3)).astype(F) ** rng.integers(1, 6, (N_RANDOM, 1, 1, 1)).astype(F)
    g *= (F(10.0) ** rng.uniform(-4, 4, (N_RANDOM, 1, 1, 1))).astype(F)
    g[::3] *= (rng.random((len(g[::3]), 16, 16, 1)) < 0.4)
    g[1::7, 2] = 0
    return g.astype(F).reshape(N_RANDOM, 256, 3)


_record_set = None


def record_set():
    global _record_set
    if _record_set is None:
        edges = record_edge_grids()
        labels = [l for l, _ in edges] + [f"random{k}" for k in range(N_RANDOM)]
        pdf_e = np.array([g.reshape(256) for _, g in edges], F)
        rgb_e, found = rgb_for_luminance(pdf_e)
        has = found.all(axis=1)
        rgb_e[~has] = 0
        rgb_r = random_rgb_grids()
        _record_set = dict(labels=labels, n_edges=len(edges), pdf=np.concatenate([pdf_e, luminance(rgb_r)]),
                           rgb=np.concatenate([rgb_e, rgb_r]), has_rgb=np.concatenate([has, np.ones(N_RANDOM, bool)]))
    return _record_set


def record_index(label):
    return record_set()["labels"].index(label)


# cases the binary64 bound leaves out, with the reason (tests/test_guided_record_sets_host.py asserts fewer than a quarter)
RECORD_NOT_ORDINARY = {
    "total_below": "a threshold binary64 can take the other way", "total_at": "a threshold binary64 can take the other way",
    "total_above": "a threshold binary64 can take the other way", "row_sum_below": "a threshold binary64 can take the other way",
    "row_sum_at": "a threshold binary64 can take the other way", "row_sum_above": "a threshold binary64 can take the other way",
    "row_3e38": "non-finite: the float32 row sum overflows", "nan_cell": "a non-finite input", "inf_cell": "a non-finite input",
    "negative_rows": "negative cells that cancel", "penultimate_above_one": "negative cells that cancel",
}


# ------------------------------------------------------------------------------------------------
# 2. filter
# ------------------------------------------------------------------------------------------------
SIGMA_S, SIGMA_R = F(1.5), F(0.3)            # the reference's defaults


def smallest_sigma():
    """the smallest sigma whose 2.0f * sigma * sigma is not 0 in float32"""
    return first_float(lambda s: F(2) * s * s > 0, 0, 1)


def _filtered_sum(g, bilateral, ss=SIGMA_S, sr=SIGMA_R):
    return restate_normalize(restate_filter_float(g.reshape(1, 256), bilateral, ss, sr))[1][0]


def lum_of_g(g):
    """the luminance of the rgb grid (0, g, 0): (0 + 0.7152f * g) + 0"""
    g = np.asarray(g, F)
    return luminance(np.stack([np.zeros_like(g), g, np.zeros_like(g)], -1))


def filter_set():
    """[dict(label, grid (256,), rgb (256, 3), sigma_spatial, sigma_range, designed)].  Every grid is built in the G channel: rgb =
    (0, g, 0) and grid = its restated luminance, so the kernel sees the same 256 floats whether they come as counts or as rgb.
    designed: None, or the `bilateral` value the label's property was searched for (the case still runs with both filters)."""
    out = []

    def add(label, g, ss=SIGMA_S, sr=SIGMA_R, designed=None, **extra):
        g = np.asarray(g, F).reshape(256)
        rgb = np.zeros((256, 3), F); rgb[:, 1] = g
        out.append(dict(label=label, grid=lum_of_g(g), rgb=rgb, sigma_spatial=F(ss), sigma_range=F(sr), designed=designed, **extra))
    for c in range(256):
        g = np.zeros(256, F); g[c] = 1
        add(f"impulse{c}", g)
    # a luminance step at which the range weight reaches ptmi_expf's cut-off (x < -104 -> 0): the last step with a nonzero
    # weight, the first with a zero one, and the steps on either side of the argument -104 itself
    zero = first_float(lambda x: gaussian_weight(lum_of_g(x), SIGMA_R) == 0, 0.1, 100)
    cut = first_float(lambda x: range_argument(lum_of_g(x)) < F(-104), 0.1, 100)
    for name, x in (("range_last_nonzero", dn(zero)), ("range_first_zero", zero), ("range_cut_at", dn(cut)), ("range_cut_below", cut)):
        g2 = np.zeros((16, 16), F); g2[:, 8:] = x                       # a step across phi: exactly 0 | x, at column 8 and at the wrap
        add(name, g2, designed=1, step=lum_of_g(x))
        g = base_grid(21, 0.01).reshape(256).copy(); g[128:] = g[128:] + x   # a noisy step across theta
        add(name + "_noisy", g, designed=1)
    add("inf_neighbour", _with(base_grid(22), (6, 6), INF))
    add("nan_cell", _with(base_grid(22), (6, 6), NAN))
    add("nan_cell_control", base_grid(22))
    tiny = smallest_sigma()
    for name, s in (("1e-23", F(1e-23)), ("smallest", tiny), ("0.6", F(0.6)), ("1.5", F(1.5)), ("3", F(3)), ("1e18", F(1e18))):
        add(f"sigma_spatial_{name}", base_grid(23), ss=s)
        add(f"sigma_range_{name}", base_grid(23), sr=s)
    add("sigma_both_1e-23", base_grid(23), ss=1e-23, sr=1e-23)
    # the sum of the 256 filtered values at 1e-12f: 256 cells of a luminance of about 0.75 * s sum to about 0.9e-12; one cell is searched
    b = base_grid(24, 0.9e-12 / 192 / 0.7152)
    for bil in (0, 1):
        f = lambda x: _filtered_sum(lum_of_g(_with(b, (7, 7), x)), bil)
        at = first_float(lambda x: f(x) >= EPS_SUM, 0, 1e-12)
        above = first_float(lambda x: f(x) > EPS_SUM, 0, 1e-12)
        tag = "b" if bil else "g"
        for name, x in (("below", dn(at)), ("at", at), ("above", above)):
            add(f"sum_{name}_{tag}", _with(b, (7, 7), x), designed=bil)
    # a sum whose order matters: with sigma 1e-23 every cell keeps its centre value, so the sum is over the grid itself:
    # 0.7152 * 2^24 and 255 values of 0.3576, each of which the running sum absorbs
    g = np.full(256, 0.5, F); g[0] = F(2.0 ** 24)
    add("sum_order", g, ss=1e-23)
    add("zero", np.zeros(256, F))
    return out


def range_argument(d, sigma=None):
    """the argument of the range weight's expf for a luminance difference d"""
    sigma = SIGMA_R if sigma is None else F(sigma)
    with quiet():
        return -(F(d) * F(d)) / (F(2) * sigma * sigma)


FILTER_NOT_ORDINARY_PREFIX = {
    "inf_neighbour": "a non-finite input", "nan_cell": "a non-finite input", "sum_below": "a threshold binary64 can take the other way",
    "sum_at": "a threshold binary64 can take the other way", "sum_above": "a threshold binary64 can take the other way",
    "range_": "a threshold: the float32 range weight is 0 or the smallest denormal where binary64 has 1e-45",
    "sigma_spatial_1e-23": "non-finite: 2 * sigma * sigma is 0 in float32", "sigma_range_1e-23": "non-finite: 2 * sigma * sigma is 0 in float32",
    "sigma_both_1e-23": "non-finite: 2 * sigma * sigma is 0 in float32", "sum_order": "non-finite: 2 * sigma * sigma is 0 in float32",
    "sigma_spatial_smallest": "a threshold: 2 * sigma * sigma is the smallest denormal", "sigma_range_smallest": "a threshold: 2 * sigma * sigma is the smallest denormal",
}


def filter_not_ordinary(label):
    for p, why in FILTER_NOT_ORDINARY_PREFIX.items():
        if label.startswith(p) and not label.startswith("nan_cell_control"):
            return why
    return None


def filter_groups(cases):
    """the cases grouped by their sigmas, so that each group is one launch: {(ss, sr): [index]}"""
    groups = {}
    for k, c in enumerate(cases):
        groups.setdefault((float(c["sigma_spatial"]), float(c["sigma_range"])), []).append(k)
    return groups


# ------------------------------------------------------------------------------------------------
# 3. grid update
# ------------------------------------------------------------------------------------------------
def frisvad(n):
    """the tangent frame of form_factors.h:93-103 in binary64, to AIM sources (the restatement takes the cell from the oracle)"""
    n = np.asarray(n, D)
    if n[2] < -0.9999999:
        return np.array([0, -1.0, 0]), np.array([-1.0, 0, 0])
    a = 1 / (1 + n[2]); c = -n[0] * n[1] * a
    return np.array([1 - n[0] * n[0] * a, c, -n[0]]), np.array([c, 1 - n[1] * n[1] * a, -n[1]])


def cell_direction(cell, normal):
    """the direction through the centre of grid cell `cell` (theta over [0, pi] in 16 rows, phi over [0, 2 pi) in 16 columns)"""
    t, b = frisvad(normal)
    th = (cell // 16 + 0.5) * np.pi / 16; ph = (cell % 16 + 0.5) * 2 * np.pi / 16
    return np.sin(th) * np.cos(ph) * t + np.sin(th) * np.sin(ph) * b + np.cos(th) * np.asarray(normal, D)


def _world(label, centre, normal, ff, rad, filtering=None, **extra):
    n = len(centre)
    w = dict(label=label, centre=np.asarray(centre, F).reshape(n, 3), normal=np.asarray(normal, F).reshape(n, 3),
             ff=np.asarray(ff, F).reshape(n, n), rad=np.asarray(rad, F).reshape(n, 3), filtering=filtering)
    w.update(extra)
    return w


def random_world(n, seed):
    rng = np.random.default_rng(seed)
    nrm = rng.normal(0, 1, (n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    ff = rng.uniform(0, 0.2, (n, n)) * (rng.random((n, n)) < 0.8)
    return _world(f"random_n{n}", rng.uniform(-2, 2, (n, 3)), nrm, ff, rng.uniform(0, 3, (n, 3)))       # the diagonal is nonzero


TILTED = np.array([0.48, -0.6, 0.64])                    # a unit normal off every axis


def cells_world(normal, label):
    """receiver 0 at the origin, source 1 + c aimed through the centre of cell c, rows 8 .. 15 (below the horizon) included"""
    n = 257
    centre = np.zeros((n, 3)); nrm = np.tile(np.asarray(normal, D), (n, 1))
    for c in range(256):
        centre[1 + c] = cell_direction(c, normal) * (1.5 + (c % 5) * 0.25)
    ff = np.zeros((n, n)); ff[0, 1:] = 0.001 + np.arange(256) / 4096.0
    rad = np.stack([1 + np.arange(n) % 3, 2 - (np.arange(n) % 2) * 0.5, 0.25 + (np.arange(n) % 7)], 1)
    return _world(label, centre, nrm, ff, rad, cells=np.arange(256))


def order_group(n, first, label, filtering=None):
    """receiver 0; sources first .. first + 3 lie on one ray, so in one cell, and carry F = 2^24, 1, 1, 1 over radiosity 1: added in
    ascending j the cell holds 2^24, in any other order more"""
    centre = np.zeros((n, 3)); centre[:, 0] = 3 + np.arange(n) * 0.001; centre[0] = 0
    d = cell_direction(3 * 16 + 5, (0, 0, 1))
    for k in range(4):
        centre[first + k] = d * (2 + k)
    nrm = np.tile([0.0, 0, 1], (n, 1))
    ff = np.zeros((n, n)); ff[0, first:first + 4] = (2.0 ** 24, 1, 1, 1)
    ff[1:, 0] = 0.01                                     # every other receiver sees primitive 0 alone
    ff[first + 1, first] = 0.5
    return _world(label, centre, nrm, ff, np.ones((n, 3)), filtering, group=(first, 3 * 16 + 5))


def grid_worlds():
    out = [_world("n1", [[0.5, 0.25, -1]], [[0, 0, 1]], [[0.7]], [[1, 2, 3]])]
    out += [random_world(n, 100 + n) for n in (2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 40)]
    # one row with every kind of form factor; the sources sit in different cells, radiosity 1, 2, 4 ...
    kinds = [("diag", 0.9), ("plus_zero", 0.0), ("minus_zero", -0.0), ("denormal", 1e-42), ("negative", -0.25), ("nan", np.nan),
             ("inf", np.inf), ("ordinary", 0.125)]
    n = len(kinds)
    centre = np.zeros((n, 3)); cells = [0] + [16 * k + 2 * k + 1 for k in range(1, n)]
    for k in range(1, n):
        centre[k] = cell_direction(cells[k], TILTED) * 2
    ff = np.full((n, n), 0.01); ff[0] = [v for _, v in kinds]
    out.append(_world("ff_kinds", centre, np.tile(TILTED, (n, 1)), ff, np.stack([2.0 ** np.arange(n)] * 3, 1) * [1, 0.5, 0.25],
                      kinds=[k for k, _ in kinds], cells=np.array(cells)))
    # coinciding centres, and centres whose float32 distance is 1e-6f, just below and just above
    dist = lambda x: world_geometry(dict(centre=np.array([[0, 0, 0], [x, 0, 0]], F)), 0)[0][1]
    at = first_float(lambda x: dist(x) >= EPS_TOTAL, 1e-7, 1e-5)
    above = first_float(lambda x: dist(x) > EPS_TOTAL, 1e-7, 1e-5)
    centre = np.array([[0, 0, 0], [0, 0, 0], [dn(at), 0, 0], [at, 0, 0], [above, 0, 0], [1, 1, 1]], F)
    out.append(_world("near", centre, np.tile([0.0, 0, 1], (6, 1)), np.full((6, 6), 0.25), np.stack([2.0 ** np.arange(6)] * 3, 1),
                      near=dict(coincide=1, below=2, at=3, above=4)))
    out.append(cells_world((0, 0, 1), "cells_z"))
    out.append(cells_world(TILTED, "cells_tilted"))
    out.append(order_group(9, 3, "order_n9"))
    out.append(order_group(2050, 2046, "order_n2050"))    # the group straddles the kernel's 2048-entry chunk
    for bil in (0, 1):
        w = _world(f"single_source_{'bilateral' if bil else 'gaussian'}", [[0, 0, 0], cell_direction(2 * 16 + 15, TILTED)], [TILTED, TILTED],
                   [[0, 0.5], [0.25, 0]], [[1, 2, 3], [3, 2, 1]], filtering=(bil, SIGMA_S, SIGMA_R))
        out.append(w)
    # a NaN cell under the rgb filter: outside the NaN's 5 x 5 footprint the grid equals that of the same world without it
    for bil in (0, 1):
        for label, f in (("filtered_nan", np.nan), ("filtered_nan_control", 0.0)):
            w = cells_world(TILTED, f"{label}_{'bilateral' if bil else 'gaussian'}")
            w["ff"][0, 1 + 5 * 16 + 0] = f               # cell (5, 0): its footprint wraps to columns 14, 15
            w["filtering"] = (bil, SIGMA_S, SIGMA_R)
            out.append(w)
    return out


GRID_NOT_ORDINARY = {"ff_kinds": "a non-finite input", "filtered_nan_gaussian": "a non-finite input", "filtered_nan_bilateral": "a non-finite input"}
