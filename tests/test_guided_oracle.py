"""Guided sampling modes in the oracle: properties that need no GPU.
Parity status: restated from grid.h / integrator.h:91-263 / application_state.h:492-585.  What pins them: the sampling
functions and integrator() against the reference's own, compiled over a stand-in for cuRAND (tests/test_integrator_vs_ref.py);
the PrecomputedCDF records against the reference's Grid::initFromRadiosity / initFromFormFactor + buildCDFs on constructed edge
grids, and the filter and the grid update against an independent numpy restatement (tests/test_guided_record_sets_host.py).
The tests below are the properties that need neither."""
import numpy as np

from guided_fixtures import synthetic_radiosity_grids
from oracle_binding import OracleScene, SCENES, default_camera, oracle_lib

F = np.float32


def test_acos_atan2_contract():
    L = oracle_lib()
    rng = np.random.default_rng(4)
    xs = np.concatenate([rng.uniform(-1, 1, 20000), [1, -1, 0, 1 - 1e-7]]).astype(F)
    got = np.array([L.po_acosf(float(x)) for x in xs], F)
    assert (got == np.arccos(xs.astype(np.float64)).astype(F)).mean() > 0.9999
    ys = rng.normal(0, 1, 20000).astype(F); xx = rng.normal(0, 1, 20000).astype(F)
    ys[:4] = [0, 0, 1, -1]; xx[:4] = [1, -1, 0, 0]
    got = np.array([L.po_atan2f(float(a), float(b)) for a, b in zip(ys, xx)], F)
    assert (got == np.arctan2(ys.astype(np.float64), xx.astype(np.float64)).astype(F)).mean() > 0.9999


def test_modes_without_grids_equal_bsdf_mode():
    """No CDF records: every guided mode falls back to cosine sampling with the same RNG draws (integrator.h:258-261)."""
    o = OracleScene.load(SCENES + "/cbox.obj")
    ref = o.render(default_camera(), 48, 48, 4, sampling_mode=0)
    for mode in (1, 2, 3, 4):
        got = o.render(default_camera(), 48, 48, 4, sampling_mode=mode)
        assert (got[1].view(np.uint32) == ref[1].view(np.uint32)).all() and (got[0] == ref[0]).all()
    o.set_radiosity_grids(np.zeros((o.n_prims, 256, 3), F))       # all-empty grids: records exist but are invalid
    got = o.render(default_camera(), 48, 48, 4, sampling_mode=3)
    assert (got[1].view(np.uint32) == ref[1].view(np.uint32)).all()


def test_precomputed_cdf_records():
    o = OracleScene.load(SCENES + "/cbox.obj")
    g = synthetic_radiosity_grids(o.n_prims)
    o.set_radiosity_grids(g)
    c = o.cdfs()
    pdf, row_sums, marg, rows = c[:, :256], c[:, 256:264], c[:, 264:272], c[:, 272:528].reshape(-1, 16, 16)
    total, valid = c[:, 528], c[:, 529].view(np.int32)
    lum = (0.2126 * g[:, :, 0] + 0.7152 * g[:, :, 1] + 0.0722 * g[:, :, 2])
    assert np.allclose(pdf, lum, rtol=1e-6)
    assert (valid == (total > 1e-6)).all() and valid[4] == 0 and valid[0] == 1
    ok = valid == 1
    assert (np.diff(marg[ok], axis=1) >= 0).all() and (marg[ok][:, -1] == 1).all()
    assert (np.diff(rows, axis=2) >= -1e-7).all() and (rows[:, :, -1] == 1).all()
    assert np.allclose(rows[:, 8:], (np.arange(16) + 1) / 16)          # lower hemisphere: uniform
    assert np.allclose(rows[1, 2:5], (np.arange(16) + 1) / 16)         # empty rows: uniform
    assert np.allclose(row_sums[ok].sum(1), total[ok], rtol=1e-5)


def test_guided_modes_are_consistent_estimators():
    """Grid and MIS sampling reweight by cos/(pi pdf): on a smooth grid (no 10x clamp hits) the image mean must agree
    with BSDF sampling to Monte-Carlo accuracy, while individual pixels differ (different directions are drawn)."""
    o = OracleScene.load(SCENES + "/cbox.obj")
    W = H = 96; spp = 48
    _, ref, st0 = o.render(default_camera(), W, H, spp, sampling_mode=0)
    o.set_radiosity_grids(synthetic_radiosity_grids(o.n_prims, empty_every=0))
    means = {}
    for mode in (2, 3):
        _, rad, st = o.render(default_camera(), W, H, spp, sampling_mode=mode)
        means[mode] = float(rad.mean())
        assert (rad != ref).any()
        assert st.rays != st0.rays                      # other directions -> other paths
    m0 = float(ref.mean())
    assert abs(means[3] - m0) / m0 < 0.03, (means, m0)       # MIS: unbiased up to the weight clamp
    assert abs(means[2] - m0) / m0 < 0.10, (means, m0)       # pure grid sampling: clamp at 10 and the theta cap bias it slightly
    # With a tiny grid-selection probability the reference's 10x weight clamp (integrator.h:157) cuts the rare grid
    # samples' weights and the estimator loses energy - reproduced here, not "fixed":
    o.set_mis_fraction(0.99)
    _, rad, _ = o.render(default_camera(), W, H, spp, sampling_mode=3)
    assert 0.75 < float(rad.mean()) / m0 < 0.95
