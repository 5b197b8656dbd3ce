"""Host half of rough metal (include/ptmi.h, "rough metal"): ptmi_check_surfaces_rough, the float32 restatement
(tests/rough_oracle.py) against binary64 - reciprocity, the sample weight, the sampler's density, the directional albedo - the
density bound, the estimator's draws, and ptmi_scenes.cornell_blocks.  No GPU."""
import os

import numpy as np
import pytest

import path_oracle as PO
import ptmi
import ptmi_scenes
import rough_oracle as RO
from oracle_binding import OracleScene, SCENES, default_camera

F = np.float32
CBOX = os.path.join(SCENES, "cbox.obj")
CBOX_QUADS = os.path.join(SCENES, "cbox_quads.obj")
# the directional albedo at 0 / 30 / 60 degrees and the share of samples below the horizon at 60 degrees, as the issue that
# introduced the kind recorded them (binary64, quadrature against 2 M samples, agreement 3e-4)
ALBEDO = {0.25: (0.9158, 0.9042, 0.8573), 0.5: (0.6879, 0.6831, 0.6983), 1.0: (0.3069, 0.3352, 0.4507)}
ANGLES = (0.0, 30.0, 60.0)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# ptmi_check_surfaces_rough
# ------------------------------------------------------------------------------------------------
def test_check_accepts_what_the_header_allows():
    assert ptmi.SURFACE_ROUGH == 3
    ptmi.check_surfaces([0, 1, 2, 3], None, 0.3)
    ptmi.check_surfaces([3, 3], [1.0, 8.0], [0.05, 1.0])
    ptmi.check_surfaces([0], 1.5, 1.0)
    L = ptmi.lib()
    k = np.array([3, 0], np.int32)
    assert L.ptmi_check_surfaces_rough(2, k.ctypes.data, None, None) == 0          # roughness NULL: 0.3, nothing to check


@pytest.mark.parametrize("kind,ior,roughness,word", [
    ([0, 4], None, 0.3, "kind"), ([-1], None, 0.3, "kind"),
    ([3, 3], None, [0.3, np.nan], "roughness"), ([3, 3], None, [np.inf, 0.3], "roughness"),
    ([3], None, [0.049], "roughness"), ([3], None, [1.001], "roughness"),
    ([0, 3], None, [np.nan, 0.3], "roughness"), ([0, 3], None, [0.049, 0.3], "roughness"),      # on a diffuse entry too
    ([0, 3], None, [1.001, 0.3], "roughness"), ([0, 3], None, [-np.inf, 0.3], "roughness"),
    ([3], [0.5], 0.3, "ior"),
])
def test_check_rejects(kind, ior, roughness, word):
    with pytest.raises(ptmi.PtmiError) as e:
        ptmi.check_surfaces(kind, ior, roughness)
    assert word in str(e.value)


def test_check_rejects_null_and_empty():
    L = ptmi.lib()
    k = np.zeros(1, np.int32)
    assert L.ptmi_check_surfaces_rough(1, None, None, None) == -1 and "kind" in L.ptmi_last_error().decode()
    assert L.ptmi_check_surfaces_rough(0, k.ctypes.data, None, None) == -1 and "n_prims" in L.ptmi_last_error().decode()


def test_the_old_entry_still_rejects_kind_3():
    L = ptmi.lib()
    k = np.array([0, 3], np.int32)
    assert L.ptmi_check_surfaces(2, k.ctypes.data, None) == -1 and "kind" in L.ptmi_last_error().decode()
    with pytest.raises(ptmi.PtmiError):
        ptmi.check_surfaces([0, 3])                           # no roughness: the old entry point


# ------------------------------------------------------------------------------------------------
# the restatement against binary64
# ------------------------------------------------------------------------------------------------
def directions(n, seed):
    rng = np.random.default_rng(seed)
    mu = rng.uniform(0.05, 1.0, n); phi = rng.uniform(0, 2 * np.pi, n)
    s = np.sqrt(1 - mu * mu)
    return np.stack([s * np.cos(phi), s * np.sin(phi), mu], axis=-1)


@pytest.mark.parametrize("roughness", [0.05, 0.3, 0.5, 1.0])
def test_f_is_symmetric_and_the_restatement_evaluates_it(roughness):
    alpha = roughness * roughness
    a, b = directions(200, 1), directions(200, 2)
    for wo, wi in zip(a, b):
        f_ab = RO.f64(alpha, wo, wi[None])[0]; f_ba = RO.f64(alpha, wi, wo[None])[0]
        assert abs(f_ab - f_ba) <= 1e-12 * f_ab
        # float32: g = f * ci from either side, p_b the sampler's density
        v = RO.Vertex.local(wo.astype(F), F(alpha))
        g, p_b = RO.evaluate(v, wi.astype(F))
        wo32, wi32 = v.wo.astype(np.float64), wi.astype(F).astype(np.float64)
        f32_ab = RO.f64(float(v.alpha), wo32, wi32[None])[0]
        assert abs(float(g) - f32_ab * wi32[2]) <= 2e-5 * f32_ab * wi32[2]
        assert abs(float(p_b) - RO.pdf64(float(v.alpha), wo32, wi32[None])[0]) <= 2e-5 * float(p_b)
        g2, _ = RO.evaluate(RO.Vertex.local(wi.astype(F), F(alpha)), wo.astype(F))
        assert abs(float(g) / wi32[2] - float(g2) / wo32[2]) <= 4e-5 * f32_ab


@pytest.mark.parametrize("roughness", [0.05, 0.3, 0.5, 1.0])
@pytest.mark.parametrize("theta_deg", [0.0, 30.0, 60.0, 85.0, 89.9])
def test_g_over_p_b_is_the_sample_weight(roughness, theta_deg):
    """the light sample's g / p_b towards a sampled direction is the weight the BSDF sample gives beta, to 1e-6 relative, and the
    two densities agree: the two MIS weights of a direction sum to 1"""
    th = np.radians(theta_deg)
    v = RO.Vertex.local(np.array([np.sin(th), 0.0, np.cos(th)], F), F(roughness) * F(roughness))
    rng = np.random.default_rng(5)
    seen = 0
    for u1, u2 in rng.uniform(0, 1, (100, 2)):
        s = RO.sample(v, F(u1), F(u2))
        if s is None:
            continue
        nxt, weight, p_b = s                                  # the frame is the world's axes: nxt is wl
        e = RO.evaluate(v, nxt)
        assert e is not None
        g, p_b2 = e
        assert abs(float(g) / float(p_b2) - float(weight)) <= 1e-6 * float(weight)
        assert 0 < float(weight) <= 1.0
        # h comes back from wo + wl, whose unit-sized components cancel: dh = 2^-23 / |wo + wl| per component, and D's t =
        # h_xy^2 + a2 h_z^2 moves by 2 h_xy dh <= t dh / alpha; D goes as t^-2, and several roundings add up
        dh = 2.0 ** -23 / float(np.linalg.norm(v.wo.astype(np.float64) + nxt.astype(np.float64)))
        assert abs(float(p_b2) - float(p_b)) <= (1e-5 + 8 * dh / float(v.alpha)) * float(p_b)
        seen += 1
    assert seen >= 40


_quadrature = {}


def albedo(alpha, deg):
    """(the fine quadrature's value, |fine - coarse|): computed once per case"""
    key = (alpha, deg)
    if key not in _quadrature:
        th = np.radians(deg)
        coarse = RO.albedo64(alpha, th, 750, 1500)
        fine = RO.albedo64(alpha, th, 1500, 3000)
        _quadrature[key] = (fine, abs(fine - coarse))
    return _quadrature[key]


@pytest.mark.parametrize("alpha", [0.25, 0.5, 1.0])
def test_albedo_by_quadrature_and_by_sampling(alpha):
    """the mean weight of the visible-normal samples is the directional albedo; the quadrature shows its own error by a run at
    twice the resolution; the values recorded with the contract"""
    n = 2_000_000
    rng = np.random.default_rng(11)
    for deg, recorded in zip(ANGLES, ALBEDO[alpha]):
        value, err = albedo(alpha, deg)
        assert err <= 1e-4, (alpha, deg, err)
        assert abs(value - recorded) <= 3e-4 + 5e-5, (alpha, deg, value)      # (recorded to four digits)
        _, w = RO.sample64(alpha, RO.wo64(np.radians(deg)), rng.uniform(0, 1, n), rng.uniform(0, 1, n))
        se = w.std() / np.sqrt(n)
        print(f"alpha {alpha} at {deg}: quadrature {value:.5f} (+- {err:.1e}), samples {w.mean():.5f} +- {se:.1e}, weight std {w.std():.3f}, "
              f"below the horizon {np.mean(w == 0):.3f}")
        assert abs(w.mean() - value) <= 5 * se + err


@pytest.mark.parametrize("alpha", [0.25, 0.5, 1.0])
def test_density_integrates_to_the_share_above_the_horizon(alpha):
    n = 2_000_000
    rng = np.random.default_rng(12)
    for deg in ANGLES:
        wo = RO.wo64(np.radians(deg))
        coarse = RO.hemisphere_quadrature(lambda wi: RO.pdf64(alpha, wo, wi), 750, 1500)
        fine = RO.hemisphere_quadrature(lambda wi: RO.pdf64(alpha, wo, wi), 1500, 3000)
        assert abs(fine - coarse) <= 1e-4
        _, w = RO.sample64(alpha, wo, rng.uniform(0, 1, n), rng.uniform(0, 1, n))
        below = np.mean(w == 0)
        se = np.sqrt(max(below * (1 - below), 1.0 / n) / n)
        print(f"alpha {alpha} at {deg}: density integrates to {fine:.5f}, 1 - below = {1 - below:.5f} +- {se:.1e}")
        assert abs(fine - (1 - below)) <= 5 * se + abs(fine - coarse)


def test_half_vector_quadrature_agrees_where_both_converge():
    """the narrow-lobe albedo of the expectation tests (alpha 0.0025) comes from the half-vector quadrature: here it meets the
    quadrature over wi at alpha 0.25, and shows its own error at alpha 0.0025"""
    for deg in (0.0, 45.0, 60.0):
        a = RO.albedo_half_vector64(0.25, np.radians(deg), 2000, 1000)
        b = RO.albedo64(0.25, np.radians(deg))
        assert abs(a - b) <= 2e-4, (deg, a, b)
    coarse = RO.albedo_half_vector64(0.0025, np.radians(45.0), 1000, 500)
    fine = RO.albedo_half_vector64(0.0025, np.radians(45.0), 2000, 1000)
    assert abs(fine - coarse) <= 1e-4
    assert 0.99 < fine <= 1.0 + 1e-6


def test_density_bound_over_grazing_angles():
    """p_b <= 1 / (2 PI alpha^3) (factor 1.01) at roughness 0.05 for co from 1 down to 1e-18, at the lobe's peak (h = un, the
    mirror direction) and off it; and no square of it overflows"""
    alpha = F(0.05) * F(0.05)
    bound = 1.01 / (2.0 * np.pi * float(alpha) ** 3)
    assert bound < 1.1e7
    worst = 0.0
    for co in np.concatenate([[1.0, 0.999, 0.9, 0.5, 0.1], 10.0 ** -np.arange(2.0, 18.5, 0.5)]):
        so = np.sqrt(max(0.0, 1.0 - co * co))
        v = RO.Vertex.local(np.array([so, 0.0, co], F), alpha)
        assert v.good
        for tilt in (0.0, 1e-4, 1e-3, 2.5e-3, 1e-2):           # the half vector's angle from un, in the plane of incidence
            h = np.array([np.sin(tilt), 0.0, np.cos(tilt)])
            wo = v.wo.astype(np.float64)
            wi = (2.0 * np.dot(wo, h) * h - wo).astype(F)
            e = RO.evaluate(v, wi)
            if e is None:
                continue
            g, p_b = e
            assert np.isfinite(float(p_b)) and 0 < float(p_b) <= bound, (co, tilt, float(p_b))
            assert 0 <= float(g) <= float(p_b) * (1 + 1e-6)
            worst = max(worst, float(p_b))
    assert worst > 0.5 * bound / 1.01                         # the bound is approached towards grazing
    assert np.isfinite(F(worst) * F(worst))


def test_grazing_and_zero_normals_end_the_vertex():
    d = np.array([1.0, 0.0, 0.0], F)
    for sn in (np.zeros(3, F), np.array([0.0, 0.0, 1.0], F), np.array([0.0, 0.0, 1e-30], F) * 0):
        v = RO.Vertex(sn, d, F(0.09))
        assert not v.good and RO.evaluate(v, np.array([0.0, 0.0, 1.0], F)) is None
    v = RO.Vertex(np.array([0.0, 0.0, 1.0], F), np.array([1.0, 0.0, -1e-20], F), F(0.09))     # co * co underflows the threshold
    assert not v.good
    v = RO.Vertex(np.array([0.0, 0.0, 2.0], F), np.array([np.cos(1e-4), 0.0, -np.sin(1e-4)], F), F(0.09))
    assert v.good and RO.sample(v, F(0.3), F(0.6)) is not None


# ------------------------------------------------------------------------------------------------
# the estimator
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
@pytest.mark.parametrize("depth", [3, 8])
def test_a_rough_vertex_draws_what_a_diffuse_one_draws(next_event, depth):
    o = OracleScene.load(CBOX)
    kind = ptmi_scenes.cornell_blocks(o.prims(), short=ptmi.SURFACE_GLASS, tall=ptmi.SURFACE_ROUGH)
    r = PO.RoughRenderer(o, default_camera(), 16, 16, kind, roughness=0.3, next_event=next_event)
    r.trace = []
    before = r.draws
    r.sums(2, depth)
    seen = {0: 0, 2: 0, 3: 0}
    for k, d, n in r.trace:
        roulette = 1 if d > 2 else 0
        nee = 3 if next_event and d + 1 < depth else 0
        full = {0: roulette + nee + 2, 2: roulette + 1, 3: roulette + nee + 2}[k]
        assert n == full or (roulette and n == 1) or (k == 0 and n == 0), (k, d, n)
        seen[k] += 1
    assert min(seen.values()) > 20
    assert r.draws - before == 2 * r.samples + sum(n for _, _, n in r.trace)


def test_the_rough_block_shows_in_the_restatement():
    o = OracleScene.load(CBOX)
    kind = ptmi_scenes.cornell_blocks(o.prims(), short=0, tall=ptmi.SURFACE_ROUGH)
    a = PO.RoughRenderer(o, default_camera(), 8, 8, kind, next_event=True).sums(2, 5)
    b = PO.SpecRenderer(o, default_camera(), 8, 8, np.zeros_like(kind), next_event=True).sums(2, 5)
    assert np.isfinite(a).all() and not np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("path,sub", [(CBOX, 0), (CBOX_QUADS, 0), (CBOX, 2)])
def test_cornell_blocks_defaults_and_kinds(path, sub):
    p = ptmi.HostScene.load(path, sub).prims()
    old = ptmi_scenes.cornell_blocks(p)
    assert old.dtype == np.int32 and set(np.unique(old)) == {0, 1, 2}
    assert np.array_equal(old, ptmi_scenes.cornell_blocks(p, ptmi.SURFACE_MIRROR, ptmi.SURFACE_GLASS))
    new = ptmi_scenes.cornell_blocks(p, short=ptmi.SURFACE_GLASS, tall=ptmi.SURFACE_ROUGH)
    assert np.array_equal(new == 2, old == 1) and np.array_equal(new == 3, old == 2)
