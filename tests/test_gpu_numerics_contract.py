"""The numerics contract on the device: the gfx950 build of include/ptmi_math.h, called per operation through ptmi_debug_math
(debug_hooks.hip, the bounce kernels' flags), against the host build inside the oracle (po_math_batch) - binary64 bits for the
_d functions, binary32 bits for the float wrappers, no mismatch allowed - and the IEEE primitives the kernels rely on against
numpy's float32 / float64 arithmetic.  Then the two places where acosf / atan2f meet a 16-way quantiser, at the cells'
boundaries: grid_compute_pdf (shading.h) through the GUIDED_GRID_PDF hook, direction_to_grid_index_local (the form-factor
kernel's) through ptmi_debug_grid_index.  Inputs: tests/numerics_sets.py.
"""
import os

import numpy as np
import pytest

import numerics_sets as S
import ptmi
from bit_compare import assert_same_bits
from oracle_binding import SCENES, OracleScene, math_batch, oracle_lib

pytestmark = pytest.mark.gpu
F = np.float32
M = ptmi.Renderer


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def both(R, op, a, b=None):
    return R.debug_math(op, a, b), math_batch(op, a, b)


def test_binary64_functions_device_against_host(R):
    """ptmi_sincos_d, ptmi_tan_d, ptmi_log_d, ptmi_exp_d, ptmi_atan2_d: the binary64 results themselves.  Only these can tell
    a build that contracts a * b + c (or lowers the f64 division or square root differently) from the contract's; the rounded
    floats hide it."""
    n = 0
    for name, op, a in (("sincos_d", M.MATH_SINCOS_D, S.sincos_set()), ("tan_d", M.MATH_TAN_D, S.tan_set()),
                        ("log_d", M.MATH_LOG_D, S.log_set()), ("exp_d", M.MATH_EXP_D, S.exp_d_set())):
        got, want = both(R, op, a)
        n += assert_same_bits(name, got, want, a)
    y, x = S.atan2_set()
    got, want = both(R, M.MATH_ATAN2_D, y, x)
    n += assert_same_bits("atan2_d", got[:, 0], want[:, 0], y, x)
    assert n > 100000


def test_binary32_wrappers_device_against_host(R):
    """ptmi_sincosf, ptmi_powf, ptmi_expf, ptmi_atan2f, ptmi_acosf: float bits, NaN and +-inf where the domain has them"""
    n = 0
    a = S.sincos_set()
    got, want = both(R, M.MATH_SINCOSF, a)
    n += assert_same_bits("sincosf", got.astype(F), want.astype(F), a)
    x, y = S.powf_set()
    got, want = both(R, M.MATH_POWF, x, y)
    n += assert_same_bits("powf", got[:, 0].astype(F), want[:, 0].astype(F), x, y)
    a = S.expf_set()
    got, want = both(R, M.MATH_EXPF, a)
    n += assert_same_bits("expf", got[:, 0].astype(F), want[:, 0].astype(F), a)
    d = got[a == F(-100.0), 0]
    assert len(d) and (d > 0).all() and (d < np.finfo(F).tiny).all()           # a denormal result, not flushed
    y, x = S.atan2_set()
    got, want = both(R, M.MATH_ATAN2F, y, x)
    n += assert_same_bits("atan2f", got[:, 0].astype(F), want[:, 0].astype(F), y, x)
    a = S.acosf_set()
    got, want = both(R, M.MATH_ACOSF, a)
    n += assert_same_bits("acosf", got[:, 0].astype(F), want[:, 0].astype(F), a)
    assert n > 100000
    for op, args in ((M.MATH_SINCOSF, (S.sincos_set(),)), (M.MATH_POWF, S.powf_set())):     # float results came back promoted: exact
        g = R.debug_math(op, *args)
        assert (g.astype(F).astype(np.float64) == g)[~np.isnan(g)].all()


def test_ieee_primitives_device_against_numpy(R):
    """f32 a / b, rcp_rn, sqrt_rn (-fhip-fp32-correctly-rounded-divide-sqrt, pt_vec.h), the single rounding of an exact binary64
    product to binary32 (ties, denormal results, overflow) and float -> int truncation, against x86 IEEE arithmetic."""
    a, b = S.pairs_set()
    with np.errstate(all="ignore"):
        n = assert_same_bits("a / b", R.debug_math(M.MATH_DIV, a, b)[:, 0].astype(F), a / b, a, b)
        n += assert_same_bits("(float)((double)a * (double)b)", R.debug_math(M.MATH_ROUND, a, b)[:, 0].astype(F),
                              (a.astype(np.float64) * b.astype(np.float64)).astype(F), a, b)
        r = S.rcp_set()
        n += assert_same_bits("rcp_rn", R.debug_math(M.MATH_RCP, r)[:, 0].astype(F), F(1) / r, r)
        s = S.sqrt_set()
        n += assert_same_bits("sqrt_rn", R.debug_math(M.MATH_SQRT, s)[:, 0].astype(F), np.sqrt(s), s)
    t = S.trunc_set()
    want = t.astype(np.float64).astype(np.int64).astype(np.float64)       # toward zero; -0.3 -> 0, not -0
    n += assert_same_bits("(int)a, (int)(double)a", R.debug_math(M.MATH_TRUNC, t), np.stack([want, want], axis=1), t)
    assert n > 100000


@pytest.fixture(scope="module")
def distinct_record():
    """One PrecomputedCDF record whose 128 cells have distinct pdfs, so that grid_compute_pdf's answer names the cell"""
    o = OracleScene.load(os.path.join(SCENES, "cbox.obj"))
    o.set_radiosity_grids(np.repeat(S.distinct_cell_grid()[None], o.n_prims, axis=0))
    return o.cdfs()[0].copy()


def test_shading_grid_cells_at_their_boundaries(R, distinct_record):
    """grid_compute_pdf (shading.h) against the oracle's, bit for bit, on directions at every cell boundary (and their nextafter
    neighbours), the axis directions with both signs of zero (dot_from_zero), lz = +-0 and dir == +-normal"""
    L = oracle_lib()
    d, n = S.grid_directions()
    want = np.array([L.po_grid_pdf(distinct_record.ctypes.data, d[i].ctypes.data, n[i].ctypes.data) for i in range(len(d))], F)
    values = set(want.tolist())
    assert 0.0 in values and len(values) == 129            # the 128 cells and the "below the horizon" return are all reached
    out, _ = R.debug_guided_sample(R.GUIDED_GRID_PDF, n, d, np.zeros((len(d), 6), np.uint32),
                                   recs=distinct_record[None], rec_idx=np.zeros(len(d), np.int32))
    assert_same_bits("grid_compute_pdf", out[:, 3], want, d, n)


def test_solver_grid_cells_at_their_boundaries(R):
    """direction_to_grid_index_local (the form-factor kernel's own, pt_device.h) against po_direction_to_grid_index on the same
    directions, unnormalised ones (1e-20: r == 0, 1e18) and the zero vector"""
    L = oracle_lib()
    d, n = S.solver_grid_directions()
    want = np.array([L.po_direction_to_grid_index(d[i].ctypes.data, n[i].ctypes.data) for i in range(len(d))], np.int32)
    assert set(want.tolist()) == set(range(256))
    got = R.debug_grid_index(d, n)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"{len(bad)} of {len(d)} differ: " + \
        "; ".join(f"dir {d[k].view(np.uint32)} normal {n[k].view(np.uint32)} device {got[k]} host {want[k]}" for k in bad[:5])
