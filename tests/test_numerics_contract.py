"""include/ptmi_math.h (the shared numerics contract) against float64 libm, and the
XORWOW skip-ahead machinery against brute-force stepping."""
import ctypes as C

import numpy as np

from oracle_binding import oracle_lib, rng_stream

F = np.float32


def _sincos(xs):
    L = oracle_lib()
    s = C.c_float(); c = C.c_float()
    out = np.zeros((len(xs), 2), F)
    for i, x in enumerate(xs):
        L.po_sincosf(float(x), C.byref(s), C.byref(c)); out[i] = (s.value, c.value)
    return out


def test_sincos_close_to_correctly_rounded():
    rng = np.random.default_rng(1)
    xs = np.concatenate([rng.uniform(0, 2 * np.pi, 20000), rng.uniform(-40, 40, 5000),
                         [0.0, np.pi / 2, np.pi, 2 * np.pi, 1e-30, 6.2831855]]).astype(F)
    got = _sincos(xs)
    ref = np.stack([np.sin(xs.astype(np.float64)), np.cos(xs.astype(np.float64))], 1)
    cr = ref.astype(F)                       # correctly rounded (float64 libm error << float ulp/2 boundary)
    assert (got == cr).mean() > 0.9999
    ulp = np.spacing(np.abs(cr)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - ref) <= 0.5000001 * ulp + 1e-45).all()


def test_powf_gamma():
    L = oracle_lib()
    rng = np.random.default_rng(2)
    xs = np.concatenate([rng.uniform(0, 1, 20000), 10.0 ** rng.uniform(-30, 0, 2000), [0.0, 1.0, 0.5]]).astype(F)
    g = F(1.0) / F(2.2)
    got = np.array([L.po_powf(float(x), float(g)) for x in xs], F)
    ref = np.power(xs.astype(np.float64), np.float64(g))
    assert (got == ref.astype(F)).mean() > 0.9999
    rel = np.abs(got.astype(np.float64) - ref) / np.maximum(ref, 1e-300)
    assert rel[xs > 0].max() < 6.1e-8
    assert L.po_powf(0.0, float(g)) == 0.0 and L.po_powf(1.0, float(g)) == 1.0


def test_expf_for_the_filter_weights():
    """ptmi_expf (grid_filter.h:35-37 gaussianWeight): correctly rounded on > 99.99 % of the range the filters use
    (x <= 0), exact limits: exp(0) = 1, underflow to 0 below -104, denormal results, +inf above 88.75, NaN through."""
    L = oracle_lib()
    rng = np.random.default_rng(3)
    xs = np.concatenate([-rng.uniform(0, 20, 20000), -10.0 ** rng.uniform(-30, 2, 5000), rng.uniform(0, 80, 2000),
                         [0.0, -0.0, -87.3, -88.0, -95.0, -103.0, -103.9]]).astype(F)
    got = np.array([L.po_expf(float(x)) for x in xs], F)
    ref = np.exp(xs.astype(np.float64))
    with np.errstate(over="ignore", under="ignore"):
        cr = ref.astype(F)
    assert (got == cr).mean() > 0.9999
    ulp = np.spacing(np.maximum(np.abs(cr), np.finfo(F).tiny)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - ref) <= 0.5000001 * ulp + 1e-45).all()
    assert L.po_expf(0.0) == 1.0 and L.po_expf(-104.5) == 0.0 and L.po_expf(-1e30) == 0.0
    assert 0.0 < L.po_expf(-100.0) < np.finfo(F).tiny                       # denormal, not flushed
    assert L.po_expf(89.0) == np.inf and np.isnan(L.po_expf(float("nan")))


def test_xorwow_matrix_powers_equal_direct_stepping():
    L = oracle_lib()
    L.po_rng_selftest.argtypes = [C.c_int, C.c_void_p]
    rng = np.random.default_rng(5)
    for log2n in (0, 1, 5, 12, 18):
        v = rng.integers(0, 2 ** 32, 5, dtype=np.uint64).astype(np.uint32)
        assert L.po_rng_selftest(log2n, v.ctypes.data) == 0


def test_curand_uniform_range_and_streams():
    u0, st0 = rng_stream(2023, 0, 4096)
    assert (u0 > 0).all() and (u0 <= 1).all() and abs(float(u0.mean()) - 0.5) < 0.02
    # subsequence 0 applies no jump: state = seed scramble, then plain xorwow steps
    s = np.uint32(2023) ^ np.uint32(0xaad26b49); t0 = np.uint32((1099087573 * int(s)) & 0xffffffff)
    t1 = np.uint32((2591861531 * 0xf7dcefdd) & 0xffffffff)
    v = [np.uint32((123456789 + int(t0)) & 0xffffffff), np.uint32(362436069) ^ t0,
         np.uint32((521288629 + int(t1)) & 0xffffffff), np.uint32(88675123) ^ t1, np.uint32((5783321 + int(t0)) & 0xffffffff)]
    d = (6615241 + int(t1) + int(t0)) & 0xffffffff
    outs = []
    for _ in range(4):
        t = int(v[0]) ^ (int(v[0]) >> 2)
        v = v[1:] + [np.uint32((int(v[4]) ^ ((int(v[4]) << 4) & 0xffffffff)) ^ (t ^ ((t << 1) & 0xffffffff)))]
        d = (d + 362437) & 0xffffffff
        x = (int(v[4]) + d) & 0xffffffff
        outs.append(F(F(x) * F(2.3283064e-10) + F(2.3283064e-10) / F(2.0)))
    assert (u0[:4] == np.array(outs, F)).all()
    # different pixels -> different streams
    u1, _ = rng_stream(2024, 1, 64)
    assert not (u0[:64] == u1).any()


# ---- the new sets (tests/numerics_sets.py): the host build against mpmath, the primitives against numpy, and their sharpness ----
import os
import shutil
import subprocess

import pytest

import numerics_sets as S
from oracle_binding import math_batch
from ptmi import Renderer as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _against_mpmath(got, want):
    """got: float32 results; want: their true values as mpf.  The file's two bounds: at least 99.99 % correctly rounded, and
    every error <= 0.5000001 ulp (+ 1e-45).  A true value that rounds to +-inf must give exactly that."""
    mp = pytest.importorskip("mpmath")
    got = np.asarray(got, F)
    with np.errstate(over="ignore", under="ignore"):
        cr = np.array([float(w) for w in want], np.float64).astype(F)
    fin = np.isfinite(cr)
    assert (got[~fin] == cr[~fin]).all()
    assert (got == cr).mean() > 0.9999
    with np.errstate(over="ignore"):
        ulp = np.spacing(np.abs(cr[fin])).astype(np.float64)           # inf above FLT_MAX
    err = np.array([float(abs(mp.mpf(float(g)) - w)) for g, w in zip(got[fin], np.asarray(want, object)[fin])])
    bad = np.flatnonzero(~(err <= 0.5000001 * ulp + 1e-45))
    assert len(bad) == 0, [(got[fin][k], err[k] / ulp[k]) for k in bad[:5]]


@pytest.fixture(scope="module")
def mp():
    m = pytest.importorskip("mpmath")
    m.mp.prec = 200
    return m


def test_sincosf_against_mpmath(mp):
    x = S.sincos_set()
    got = math_batch(R.MATH_SINCOSF, x).astype(F)
    xm = [mp.mpf(float(v)) for v in x]
    _against_mpmath(got[:, 0], [mp.sin(v) for v in xm])
    _against_mpmath(got[:, 1], [mp.cos(v) for v in xm])


def test_expf_against_mpmath(mp):
    x = S.expf_set()
    got = math_batch(R.MATH_EXPF, x)[:, 0].astype(F)
    nan = np.isnan(x)
    assert nan.sum() == 1 and np.isnan(got[nan]).all()
    assert got[x == np.inf] == np.inf and got[x == -np.inf] == 0.0
    fin = np.isfinite(x)
    _against_mpmath(got[fin], [mp.exp(mp.mpf(float(v))) for v in x[fin]])
    d = got[x == F(-100.0)]
    assert len(d) and (d > 0).all() and (d < np.finfo(F).tiny).all()          # a denormal, not flushed


def test_powf_against_mpmath(mp):
    x, y = S.powf_set()
    got = math_batch(R.MATH_POWF, x, y)[:, 0].astype(F)
    assert np.isnan(got[np.isnan(x)]).all() and np.isnan(x).sum() == len(S.POW_EXPONENTS)
    nonpos = ~np.isnan(x) & ~(x > 0)
    assert nonpos.sum() > 16000 and (got[nonpos].view(np.uint32) == 0).all()   # ptmi_powf: +0 for every x that is not > 0
    pos = (x > 0) & np.isfinite(x)
    _against_mpmath(got[pos], [mp.power(mp.mpf(float(a)), mp.mpf(float(b))) for a, b in zip(x[pos], y[pos])])
    assert {float(v) for v in y[pos]} == {float(v) for v in S.POW_EXPONENTS}


def test_acosf_against_mpmath(mp):
    x = S.acosf_set()
    got = math_batch(R.MATH_ACOSF, x)[:, 0].astype(F)
    out = np.abs(x) > 1
    assert out.sum() == 5 and np.isnan(got[out]).all()
    _against_mpmath(got[~out], [mp.acos(mp.mpf(float(v))) for v in x[~out]])
    assert got[x == 1.0] == 0.0 and (got[x == -1.0] == F(np.pi)).all()


def test_atan2f_against_mpmath_and_ieee_zeros(mp):
    y, x = S.atan2_set()
    got = math_batch(R.MATH_ATAN2F, y, x)[:, 0].astype(F)
    zero = (y == 0) | (x == 0)
    assert zero.sum() >= 28
    _against_mpmath(got[~zero], [mp.atan2(mp.mpf(float(a)), mp.mpf(float(b))) for a, b in zip(y[~zero], x[~zero])])
    # mpmath has no signed zero: IEEE 754 / C Annex F known answers instead
    pi, hpi, z = F(np.pi), F(np.pi / 2), F(0.0)
    known = [(z, F(1), z), (-z, F(1), -z), (z, F(-1), pi), (-z, F(-1), -pi), (z, z, z), (-z, z, -z), (z, -z, pi), (-z, -z, -pi),
             (F(1), z, hpi), (F(1), -z, hpi), (F(-1), z, -hpi), (F(-1), -z, -hpi)]
    ky, kx, kw = (np.array(c, F) for c in zip(*known))
    kg = math_batch(R.MATH_ATAN2F, ky, kx)[:, 0].astype(F)
    assert (kg.view(np.uint32) == kw.view(np.uint32)).all(), (kg, kw)
    # the set's own cases with a zero: the sign of y, and 0 / pi / pi/2 by the sign bit of x
    sy, sx = np.signbit(y[zero]), np.signbit(x[zero])
    want = np.where(y[zero] == 0, np.where(sx, pi, z), hpi)
    want = np.where(sy, -want, want).astype(F)
    assert (got[zero].view(np.uint32) == want.view(np.uint32)).all()


def test_host_primitives_are_ieee():
    """The oracle's build of the primitives the kernels rely on, against numpy's float32 / float64 arithmetic (IEEE on x86):
    division, reciprocal, square root, the single rounding of an exact binary64 product, truncation."""
    a, b = S.pairs_set()
    with np.errstate(all="ignore"):
        q = a / b
        p = (a.astype(np.float64) * b.astype(np.float64)).astype(F)
        assert (np.isfinite(a) & np.isfinite(b)).all()
        den = lambda v: (v != 0) & (np.abs(v) < np.finfo(F).tiny)
        assert den(a).sum() > 50 and den(b).sum() > 50 and den(q).sum() > 500 and np.isinf(q).sum() > 500
        assert den(p).sum() > 500 and np.isinf(p).sum() > 500
        exact = a.astype(np.float64) * b.astype(np.float64)
        ties = np.isfinite(p) & (np.abs(exact - p) == 0.5 * np.spacing(np.minimum(np.abs(p), np.abs(np.nextafter(p, F(0))))).astype(np.float64))
        assert ties.sum() >= 2000
        same = lambda got, want: (np.asarray(got, F).view(np.uint32) == np.asarray(want, F).view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        assert same(math_batch(R.MATH_DIV, a, b)[:, 0].astype(F), q).all()
        assert same(math_batch(R.MATH_ROUND, a, b)[:, 0].astype(F), p).all()
        r = S.rcp_set()
        assert same(math_batch(R.MATH_RCP, r)[:, 0].astype(F), F(1) / r).all()
        s = S.sqrt_set()
        assert same(math_batch(R.MATH_SQRT, s)[:, 0].astype(F), np.sqrt(s)).all()
        t = S.trunc_set()
        got = math_batch(R.MATH_TRUNC, t)
        assert (got[:, 0] == np.trunc(t.astype(np.float64))).all() and (got[:, 1] == got[:, 0]).all()


def test_grid_direction_set_reaches_every_cell():
    """tests/numerics_sets.py's directions, through the oracle: the shading grid's 128 cells and its "below the horizon" return,
    the solver grid's 256 cells.  (tests/test_gpu_numerics_contract.py compares the kernels' answers on the same directions.)"""
    from oracle_binding import OracleScene, SCENES, oracle_lib
    L = oracle_lib()
    o = OracleScene.load(os.path.join(SCENES, "cbox.obj"))
    o.set_radiosity_grids(np.repeat(S.distinct_cell_grid()[None], o.n_prims, axis=0))
    rec = o.cdfs()[0].copy()
    d, n = S.grid_directions()
    pdf = np.array([L.po_grid_pdf(rec.ctypes.data, d[i].ctypes.data, n[i].ctypes.data) for i in range(len(d))], F)
    values = set(pdf.tolist())
    assert 0.0 in values and len(values) == 129                        # 128 distinct cell pdfs + below the horizon
    d, n = S.solver_grid_directions()
    cells = {L.po_direction_to_grid_index(d[i].ctypes.data, n[i].ctypes.data) for i in range(len(d))}
    assert cells == set(range(256))


def _has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma " in line + " " for line in f)
    except OSError:
        return False


def test_sets_tell_a_contracted_build(tmp_path):
    """The binary64 sets must be able to see a build of ptmi_math.h that contracts a * b + c into fma: float results cannot (the
    two builds round to the same floats), and exponent-stratified inputs alone hardly can.  tests/contract_shim.c compiled with
    the oracle's flags answers as the oracle does; compiled with -mfma -ffp-contract=fast it must differ on at least 10 of each
    function's 20 000 working-range inputs (gcc gives about 20 for log and atan2, about 400 for sin/cos and tan, 2 000 for exp)."""
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    if not _has_fma() or cc is None:
        pytest.skip("needs an x86 CPU with fma and a C compiler")
    src = os.path.join(ROOT, "tests", "contract_shim.c")
    strict = ["-O3", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v2"]     # oracle/Makefile CFLAGS
    fused = ["-O3", "-std=gnu11", "-fPIC", "-mfma", "-ffp-contract=fast"]
    libs = {}
    for name, flags in (("strict", strict), ("fused", fused)):
        so = str(tmp_path / f"libshim_{name}.so")
        subprocess.check_call([cc] + flags + ["-shared", "-o", so, src])
        L = C.CDLL(so)
        L.shim_math_d.restype = None; L.shim_math_d.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        libs[name] = L

    def run(L, op, a, b):
        out = np.zeros((len(a), 2), np.float64)
        L.shim_math_d(op, len(a), a.ctypes.data, b.ctypes.data, out.ctypes.data)
        return out.view(np.uint64)

    ay, ax = S.atan2_set()
    for name, op, a, b in (("sincos", R.MATH_SINCOS_D, S.sincos_set(), None), ("tan", R.MATH_TAN_D, S.tan_set(), None),
                           ("log", R.MATH_LOG_D, S.log_set(), None), ("exp", R.MATH_EXP_D, S.exp_d_set(), None),
                           ("atan2", R.MATH_ATAN2_D, ay, ax)):
        b = np.zeros_like(a) if b is None else b
        assert (run(libs["strict"], op, a, b) == math_batch(op, a, b).view(np.uint64)).all(), name     # the shim is the oracle's build
    ops = dict(sincos=R.MATH_SINCOS_D, tan=R.MATH_TAN_D, log=R.MATH_LOG_D, exp=R.MATH_EXP_D, atan2=R.MATH_ATAN2_D)
    counts = {}
    for name, (a, b) in S.binary64_working_ranges().items():
        assert len(a) == S.N_WORKING == 20000
        counts[name] = int((run(libs["strict"], ops[name], a, b) != run(libs["fused"], ops[name], a, b)).any(axis=1).sum())
    print("a contracted build differs on, of 20000 working-range inputs each:", counts)
    assert min(counts.values()) >= 10, counts
