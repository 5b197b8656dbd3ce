"""Input sets for the numerics-contract tests (tests/test_numerics_contract.py on the host build of include/ptmi_math.h,
tests/test_gpu_numerics_contract.py on the gfx950 build).  Deterministic: fixed seeds, nothing read from outside.

Every function's set stays inside the domain its comment in ptmi_math.h states and has three parts:
  stratified  every binade of the domain, denormals included: PER_BINADE mantissas each, the binade's first and last value
              among them, both signs where the domain has both
  working     N_WORKING uniform values from the range in which the kernels call the function.  These are what tells a
              contracted (fma) build of the header from a strict one: on exponent-stratified inputs alone the binary64
              results of the two builds hardly differ (tests/test_numerics_contract.py::test_sets_tell_a_contracted_build)
  edges       named values: signed zeros, +-1, the cut-offs of ptmi_expf and their neighbours, pi/2, pi, 2 pi, NaN and +-inf
              where the domain has them
"""
import numpy as np

F = np.float32
PER_BINADE = 64
N_WORKING = 20000
N_PAIRS = 20000
POW_EXPONENTS = np.array([F(1.0) / F(2.2), 0.5, 1.0, 2.0], F)      # the gamma step's exponent first


def _from_bits(bits):
    return np.ascontiguousarray(bits, np.uint32).view(F)


def binades(e_lo=0, e_hi=254, signs=(0, 1), seed=0):
    """PER_BINADE floats from every binade with biased exponent e_lo..e_hi (0 = the denormals), under each sign bit in `signs`.
    The first and last value of every binade are among them (the denormals' first value is the smallest denormal, not 0)."""
    rng = np.random.default_rng(seed)
    out = []
    for e in range(e_lo, e_hi + 1):
        m = rng.integers(0, 1 << 23, PER_BINADE, dtype=np.uint32)
        m[0] = 1 if e == 0 else 0
        m[1] = (1 << 23) - 1
        if e == 0:
            m[m == 0] = 1
        for s in signs:
            out.append((np.uint32(s) << np.uint32(31)) | (np.uint32(e) << np.uint32(23)) | m)
    return _from_bits(np.concatenate(out))


def _neighbours(x):
    x = F(x)
    return [np.nextafter(x, F(-np.inf)), x, np.nextafter(x, F(np.inf))]


_PI = [F(np.pi / 2), F(np.pi), F(2 * np.pi)]
_ZEROS_ONES = [F(0.0), F(-0.0), F(1.0), F(-1.0), np.nextafter(F(1), F(0)), -np.nextafter(F(1), F(0))]
_EXP_CUTS = _neighbours(-104.0) + _neighbours(88.75) + _neighbours(-100.0)      # exp(-100) is a denormal float
_NONFINITE = [F(np.nan), F(np.inf), F(-np.inf)]


def _cat(*parts):
    return np.concatenate([np.asarray(p, F).reshape(-1) for p in parts]).astype(F)


def _within(x, bound):
    return x[np.abs(x) <= F(bound)]


def _sincos_parts():
    rng = np.random.default_rng(11)
    return (_within(binades(0, 127 + 16, seed=1), 1e5), rng.uniform(0.0, 2 * np.pi, N_WORKING),
            _cat(_ZEROS_ONES, _PI, [-p for p in _PI], [1e5, -1e5]))


def _tan_parts():
    rng = np.random.default_rng(12)
    return _within(binades(0, 127 + 16, seed=2), 1e5), rng.uniform(0.0, 1.5, N_WORKING), _cat(_ZEROS_ONES, _PI, [1e5, -1e5])


def _unit_interval(rng):
    """N_WORKING uniform floats in (0, 1]"""
    return np.maximum((1.0 - rng.uniform(0.0, 1.0, N_WORKING)).astype(F), np.finfo(F).smallest_subnormal)


def _log_parts():
    return (binades(0, 254, signs=(0,), seed=3), _unit_interval(np.random.default_rng(13)),
            _cat([1.0, np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2)), 0.5, 2.0]))


def _exp_d_parts():
    rng = np.random.default_rng(14)
    return _within(binades(0, 127 + 9, seed=4), 700.0), rng.uniform(-20.0, 0.0, N_WORKING), _cat(_ZEROS_ONES, _EXP_CUTS, [700.0, -700.0])


def sincos_set():
    """sin, cos: |x| <= 1e5"""
    return _cat(*_sincos_parts())


def tan_set():
    """tan: |x| <= 1e5"""
    return _cat(*_tan_parts())


def log_set():
    """log: positive finite"""
    return _cat(*_log_parts())


def exp_d_set():
    """ptmi_exp_d: |x| <= 700"""
    return _cat(*_exp_d_parts())


def expf_set():
    """ptmi_expf: any float"""
    rng = np.random.default_rng(15)
    work = rng.uniform(-20.0, 0.0, N_WORKING)
    return _cat(binades(0, 254, seed=5), work, _ZEROS_ONES, _EXP_CUTS, _NONFINITE)


def powf_set():
    """ptmi_powf: any x, the exponents of POW_EXPONENTS in turn.  Returns (x, y)."""
    work = _unit_interval(np.random.default_rng(16))
    edges = np.repeat(_cat(_ZEROS_ONES, _NONFINITE, [0.5, np.finfo(F).max, np.finfo(F).smallest_subnormal]), len(POW_EXPONENTS))
    x = _cat(binades(0, 254, seed=6), work, edges)
    return x, POW_EXPONENTS[np.arange(len(x)) % len(POW_EXPONENTS)]


def acosf_set():
    """ptmi_acosf: |x| <= 1, and a few |x| > 1 (NaN on every build)"""
    rng = np.random.default_rng(17)
    work = rng.uniform(-1.0, 1.0, N_WORKING)
    return _cat(binades(0, 126, seed=7), work, _ZEROS_ONES, [np.nextafter(F(1), F(2)), -np.nextafter(F(1), F(2)), 2.0, -2.0, 1e10])


def _atan2_parts():
    rng = np.random.default_rng(18)
    ys = binades(0, 254, seed=8)
    xs = binades(0, 254, seed=9)[rng.permutation(len(ys))]
    # working range: |y / x| in [2^-6, 2^6], the four quadrants
    wx = (rng.uniform(1.0, 2.0, N_WORKING) * 2.0 ** rng.integers(-20, 21, N_WORKING)).astype(F)
    wy = (wx.astype(np.float64) * 2.0 ** rng.uniform(-6.0, 6.0, N_WORKING)).astype(F)
    wx = wx * rng.choice(np.array([-1.0, 1.0], F), N_WORKING)
    wy = wy * rng.choice(np.array([-1.0, 1.0], F), N_WORKING)
    tiny, big = np.finfo(F).smallest_subnormal, np.finfo(F).max
    e = _cat([0.0, -0.0, 1.0, -1.0, tiny, -tiny, big, -big])
    ey, ex = np.meshgrid(e, e, indexing="ij")
    return (ys, wy, ey), (xs, wx, ex)


def atan2_set():
    """ptmi_atan2f / ptmi_atan2_d: any finite pair.  Returns (y, x)."""
    py, px = _atan2_parts()
    return _cat(*py), _cat(*px)


def binary64_working_ranges():
    """{function: (a, b)}: only the working-range part of the five binary64 functions' sets (b: zeros but for atan2)"""
    z = np.zeros(N_WORKING, F)
    py, px = _atan2_parts()
    return {"sincos": (_cat(_sincos_parts()[1]), z), "tan": (_cat(_tan_parts()[1]), z), "log": (_cat(_log_parts()[1]), z),
            "exp": (_cat(_exp_d_parts()[1]), z), "atan2": (_cat(py[1]), _cat(px[1]))}


def pairs_set(seed=19):
    """Division and the binary64 -> binary32 rounding: N_PAIRS (a, b) spread evenly over the 255 x 255 pairs of binades (denormal
    operands, denormal quotients and products, quotients and products that overflow), then products that are exact ties
    between two floats (odd 25-bit products of two 13-bit odd factors), in the normal range and among the denormals."""
    rng = np.random.default_rng(seed)
    k = (np.arange(N_PAIRS, dtype=np.int64) * (255 * 255)) // N_PAIRS
    ea, eb = (k // 255).astype(np.uint32), (k % 255).astype(np.uint32)

    def make(e):
        m = rng.integers(0, 1 << 23, N_PAIRS, dtype=np.uint32)
        m[(e == 0) & (m == 0)] = 1
        s = rng.integers(0, 2, N_PAIRS, dtype=np.uint32)
        return _from_bits((s << np.uint32(31)) | (e << np.uint32(23)) | m)

    a, b = make(ea), make(eb)
    m2 = np.arange(4097, 8191, 2, dtype=np.int64)                       # 4097 * m2 is odd and in [2^24, 2^25): a tie
    ta = (4097.0 * 2.0 ** rng.integers(-40, 41, len(m2))).astype(F)
    tb = (m2 * 2.0 ** rng.integers(-40, 41, len(m2))).astype(F)
    den_a = np.array([1.0, 3.0, 5.0, 7.0], np.float64) * 2.0 ** -100      # odd x 2^-150: ties among the denormals
    den_b = np.full(4, 2.0 ** -50)
    return _cat(a, ta, den_a), _cat(b, tb, den_b)


def rcp_set():
    return _cat(binades(0, 254, seed=20), [np.inf, -np.inf])


def sqrt_set():
    return _cat(binades(0, 254, signs=(0,), seed=21), [0.0, -0.0, np.inf, 1.0, 4.0, 2.0])


def trunc_set():
    """(int)a for |a| < 2^31, and -2^31 itself"""
    return _cat(binades(0, 127 + 30, seed=22), [0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2147483520.0, -2147483520.0, -2147483648.0])


# ---- directions at the grid cells' boundaries -----------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(F)


GRID_NORMALS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1],
                         _unit([1, 2, 3]), _unit([-0.6, 0.48, -0.64]),
                         [-0.0, 0.0, -1.0], [-0.0, -0.0, 1.0]], F)


def _frame(n):
    """the Frisvad frame the kernels build (grid.h:287-297), in float32; only used to aim the inputs"""
    n = n.astype(F)
    if n[2] < F(-0.9999999):
        return np.array([0, -1, 0], F), np.array([-1, 0, 0], F)
    a = F(1) / (F(1) + n[2])
    c = -n[0] * n[1] * a
    return np.array([F(1) - n[0] * n[0] * a, c, -n[0]], F), np.array([c, F(1) - n[1] * n[1] * a, -n[1]], F)


def _local_dirs():
    """Local directions at phi = k pi / 8 and theta = j pi / 16 (every boundary of the shading grid's 8 x 16 cells over the upper
    hemisphere and of the solver grid's 16 x 16 over the sphere), angles built in float32, and at the cells' centres."""
    out = []
    for jj in np.arange(0, 16.5, 0.5):
        for kk in np.arange(0, 16.5, 0.5):
            if (jj % 1 == 0) != (kk % 1 == 0):
                continue                                                 # corners and centres only
            th = np.float64(F(jj) * F(np.pi / 16)); ph = np.float64(F(kk) * F(np.pi / 8))
            out.append([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    return np.array(out, np.float64).astype(F)


def grid_directions():
    """(dirs, normals), float32 (n, 3): per normal of GRID_NORMALS
      - the boundary and centre directions of _local_dirs in the normal's frame, and for each the nextafter neighbours of every
        component
      - the six axis directions with both signs of zero in the other components
      - directions in the tangent plane (lz = +-0 where the frame is exact), dir == +-normal"""
    local = _local_dirs()
    dirs, normals = [], []
    signed_axes = []
    for ax in range(3):
        for s in (1.0, -1.0):
            for z1 in (0.0, -0.0):
                for z2 in (0.0, -0.0):
                    v = [z1, z2]; v.insert(ax, s)
                    signed_axes.append(v)
    signed_axes = np.array(signed_axes, F)
    for n in GRID_NORMALS:
        t, b = _frame(n)
        world = (local[:, 0:1] * t[None] + local[:, 1:2] * b[None] + local[:, 2:3] * n[None]).astype(F)
        group = [world]
        for c in range(3):
            for to in (F(-np.inf), F(np.inf)):
                w = world.copy(); w[:, c] = np.nextafter(w[:, c], to)
                group.append(w)
        ph = (np.arange(32, dtype=F) * F(np.pi / 16)).astype(np.float64)
        plane = (np.cos(ph)[:, None] * t[None].astype(np.float64) + np.sin(ph)[:, None] * b[None].astype(np.float64)).astype(F)
        plane_neg = plane.copy(); plane_neg[plane_neg == 0] = F(-0.0)
        group += [signed_axes, plane, plane_neg, n[None], -n[None]]
        g = np.concatenate(group).astype(F)
        dirs.append(g); normals.append(np.repeat(n[None], len(g), axis=0))
    return np.concatenate(dirs), np.concatenate(normals)


def solver_grid_directions():
    """grid_directions, then the same directions at lengths 1e-20 (the squares underflow: r == 0) and 1e18, and the zero vector"""
    d, n = grid_directions()
    pick = np.arange(0, len(d), 3)
    zeros = np.zeros((len(GRID_NORMALS), 3), F)
    return (np.concatenate([d, d[pick] * F(1e-20), d[pick] * F(1e18), zeros, -zeros]),
            np.concatenate([n, n[pick], n[pick], GRID_NORMALS, GRID_NORMALS]))


def distinct_cell_grid():
    """A (256, 3) radiosity grid whose 128 upper-hemisphere cells have distinct luminances (the lower rows are not read)"""
    g = np.zeros((256, 3), F)
    g[:128] = (1.0 + 0.37 * np.arange(128, dtype=np.float64))[:, None].astype(F)
    return g
