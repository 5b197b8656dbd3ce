"""Host half of environment lighting (include/ptmi.h, "environment lighting"): ptmi_host_env_table against the numpy restatement
of the header (tests/env_oracle.py) bit for bit, the properties the contract promises for the stored pdf, the texel lookup, and
the parameter and size checks.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import env_oracle as EO
import env_scenes as ES
import ptmi

F = np.float32
PARAMS = [dict(), dict(scale=2.5, rotation_deg=70.0), dict(scale=0.125, rotation_deg=-133.0)]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def tables():
    """(library table, restated table) of every map and parameter set, computed once"""
    out = {}
    for name, make in ES.HOST_MAPS.items():
        for k, prm in enumerate(PARAMS):
            rgb = make()
            out[name, k] = (rgb, prm, ptmi.host_env_table(rgb, **prm), EO.table(rgb, prm.get("scale", 1.0), prm.get("rotation_deg", 0.0)))
    return out


@pytest.mark.parametrize("name", list(ES.HOST_MAPS))
@pytest.mark.parametrize("k", range(len(PARAMS)))
def test_table_matches_the_restatement(tables, name, k):
    _, _, got, exp = tables[name, k]
    for key in ("z", "marginal_cdf", "row_cdf", "texel"):
        assert np.array_equal(bits(got[key]), bits(exp[key])), (name, k, key)
    assert bits(got["total"]) == bits(exp["total"])


@pytest.mark.parametrize("name", list(ES.HOST_MAPS))
@pytest.mark.parametrize("k", range(len(PARAMS)))
def test_pdf_is_the_density_of_the_stored_cdfs(tables, name, k):
    rgb, prm, got, exp = tables[name, k]
    h, w = rgb.shape[:2]
    z = got["z"].astype(np.float64)
    assert z[0] == 1.0 and z[-1] == -1.0 and (np.diff(z) < 0).all()
    omega = (2.0 * np.pi / w) * (z[:-1] - z[1:])
    assert abs(omega.sum() * w - 4.0 * np.pi) < 1e-6
    pdf = got["texel"][..., 3].astype(np.float64)
    m = got["marginal_cdf"].astype(np.float64); c = got["row_cdf"].astype(np.float64)
    step_m = np.diff(np.concatenate([[0.0], m])); step_c = np.diff(np.concatenate([np.zeros((h, 1)), c], axis=1), axis=1)
    assert (step_m >= 0).all() and (step_c >= 0).all()
    if name == "zero":
        assert got["total"] == 0 and (pdf == 0).all() and (m == 0).all() and (c == 0).all()
        return
    assert got["total"] > 0 and m[-1] == 1.0
    assert (c[step_m > 0, -1] == 1.0).all()
    assert abs((pdf * omega[:, None]).sum() - 1.0) < 1e-6
    zero_step = (step_m[:, None] == 0) | (step_c == 0)
    assert (pdf[zero_step] == 0).all() and (pdf[~zero_step] > 0).all()
    if name == "spike":
        assert zero_step.sum() > 0                           # the absorbed steps the map is there for
    # the texels carry the scaled radiance, and the density is proportional to it up to the CDFs' rounding
    assert np.array_equal(bits(got["texel"][..., :3]), bits(rgb * F(prm.get("scale", 1.0))))
    lum = got["texel"][..., :3].astype(np.float64).sum(axis=2)
    big = pdf * omega[:, None] > 1e-3
    ratio = pdf[big] / lum[big]
    assert np.allclose(ratio, ratio[0], rtol=1e-3)


def directions(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


@pytest.mark.parametrize("shape,rot", [((16, 32), 0.0), ((5, 7), 70.0), ((1, 1), -20.0)])
def test_lookup_of_seeded_directions(shape, rot):
    """the restated lookup against the map's geometry in binary64, away from texel boundaries"""
    h, w = shape
    tab = EO.table(np.ones((h, w, 3), F), 1.0, rot)
    n = 10000 if shape == (16, 32) else 500
    ds = directions(n, 7)
    zb = np.cos(np.pi * np.arange(h + 1) / h)
    checked = 0
    for d in ds:
        dd = d.astype(np.float64)
        r_exact = np.searchsorted(-zb, -dd[1], side="left") - 1
        t = (np.arctan2(dd[2], dd[0]) / (2 * np.pi) - rot / 360.0) % 1.0 * w
        if min(abs(dd[1] - zb).min(), abs(t - np.round(t))) < 1e-4:
            continue                                         # on a boundary: either side may answer
        checked += 1
        assert EO.lookup(tab, d) == (int(np.clip(r_exact, 0, h - 1)), int(t) % w), d
    assert checked > 0.9 * n


def test_lookup_at_the_poles_and_the_seam():
    h, w = 16, 32
    tab = EO.table(np.ones((h, w, 3), F), 1.0, 0.0)
    assert EO.lookup(tab, np.array([0, 1, 0], F))[0] == 0
    assert EO.lookup(tab, np.array([0, -1, 0], F))[0] == h - 1
    assert EO.lookup(tab, np.array([0, 1.5, 0], F))[0] == 0 and EO.lookup(tab, np.array([0, -1.5, 0], F))[0] == h - 1
    assert EO.lookup(tab, np.array([1, 0, 1e-6], F))[1] == 0                     # just past +x towards +z
    assert EO.lookup(tab, np.array([1, 0, -1e-6], F))[1] == w - 1                # just before it
    assert EO.lookup(tab, np.array([1, 0, 0], F))[1] == 0
    assert EO.lookup(tab, np.array([-1, 0, 0], F))[1] == w // 2                  # phi = +pi
    assert EO.lookup(tab, np.array([0, 0, 1], F))[1] == w // 4                   # +z is a quarter turn from +x
    # row r covers z_{r+1} < y <= z_r: the boundary z_3 is row 3's upper end, the next float above it is in row 2
    z = tab["z"]
    assert EO.lookup(tab, np.array([0.5, z[3], 0.1], F))[0] == 3
    assert EO.lookup(tab, np.array([0.5, np.nextafter(z[3], F(2)), 0.1], F))[0] == 2
    turned = EO.table(np.ones((h, w, 3), F), 1.0, 90.0)
    assert EO.lookup(turned, np.array([0, 0, 1], F))[1] == 0                     # column 0 starts at +z now


@pytest.mark.parametrize("name,k", [("32x16", 0), ("7x5", 1), ("spike", 2), ("4x2", 0)])
def test_a_sampled_direction_looks_up_its_own_texel(tables, name, k):
    rgb, prm, _, tab = tables[name, k]
    rng = np.random.default_rng(5)
    own = 0
    n = 400
    for _ in range(n):
        r1, r2, r3, r4 = (F(1.0) - rng.random(4).astype(F))                      # (0, 1], as curand_uniform
        r, j, wi = EO.sample_direction(tab, r1, r2, r3, r4)
        assert tab["texel"][r, j, 3] > 0                                          # only texels of positive pdf are ever picked
        assert abs(float(np.linalg.norm(wi.astype(np.float64))) - 1.0) < 1e-6
        if min(r3, F(1.0) - r3, r4, F(1.0) - r4) < 1e-3:
            continue                                                              # within rounding of a boundary
        own += 1
        assert EO.lookup(tab, wi) == (r, j)
    assert own > 0.9 * n


def test_sampler_frequencies_follow_the_stored_pdf(tables):
    """the two searches pick texel (r, j) with probability pdf * Omega (chi-square-free: 5 sigma per texel)"""
    _, _, _, tab = tables["7x5", 0]
    rng = np.random.default_rng(9)
    n = 20000
    u = F(1.0) - rng.random((n, 2)).astype(F)
    rows = np.searchsorted(tab["marginal_cdf"], u[:, 0], side="left")
    cols = np.array([np.searchsorted(tab["row_cdf"][r], x, side="left") for r, x in zip(rows, u[:, 1])])
    counts = np.zeros(tab["prob"].shape); np.add.at(counts, (rows, cols), 1)
    p = tab["prob"]
    assert (np.abs(counts - n * p) <= 5.0 * np.sqrt(n * p * (1 - p)) + 1).all()


def test_parameter_and_size_checks():
    L = ptmi.lib()
    assert L.ptmi_check_env_params(C.byref(ptmi.default_env_params())) == 0
    d = ptmi.default_env_params()
    assert (d.scale, d.rotation_deg, d.select_fraction) == (1.0, 0.0, 0.5)
    for bad in (dict(scale=-1.0), dict(scale=np.inf), dict(scale=np.nan), dict(rotation_deg=np.nan), dict(rotation_deg=np.inf),
                dict(rotation_deg=400.0), dict(select_fraction=-0.1), dict(select_fraction=1.5), dict(select_fraction=np.nan)):
        assert L.ptmi_check_env_params(C.byref(ptmi.default_env_params(**bad))) == -1, bad
        assert "environment" in L.ptmi_last_error().decode()
        with pytest.raises(ptmi.PtmiError):
            ptmi.host_env_table(np.ones((2, 2, 3), F), **bad)
    assert L.ptmi_check_env_params(None) == -1
    for value in (-1.0, np.nan, np.inf):
        m = np.ones((2, 3, 3), F); m[1, 2, 1] = value
        with pytest.raises(ptmi.PtmiError, match="texel"):
            ptmi.host_env_table(m)
    with pytest.raises(ptmi.PtmiError):                       # finite texels that the scale takes to infinity
        ptmi.host_env_table(np.full((2, 2, 3), 3e38, F), scale=10.0)
    one = np.ones(3, F)
    for w, h in ((0, 1), (1, 0), (-1, 4), (1 << 13, (1 << 12) + 1)):
        assert L.ptmi_host_env_table(w, h, one.ctypes.data, None, None, None, None, None, None) == -1, (w, h)
    assert L.ptmi_host_env_table(1, 1, None, None, None, None, None, None, None) == -1
    total = C.c_float()
    assert L.ptmi_host_env_table(1, 1, one.ctypes.data, None, None, None, None, None, C.byref(total)) == 0   # NULL params: defaults
    assert abs(total.value - 3.0 * 4.0 * np.pi) < 1e-4


def test_the_largest_map_is_accepted():
    """2^25 texels as 2^25 rows of one column: the rows next to the poles have z_r = z_{r+1} in float - empty, weight 0, pdf 0"""
    h = 1 << 25
    rgb = np.ones((h, 1, 3), F)
    t = ptmi.host_env_table(rgb)
    pdf = t["texel"][..., 3]
    z = t["z"]
    empty = z[:-1] == z[1:]
    assert empty.any() and (pdf[empty, 0] == 0).all() and t["marginal_cdf"][-1] == 1.0


def test_new_symbols_are_exported():
    L = ptmi.lib()
    for name in ("ptmi_default_env_params", "ptmi_check_env_params", "ptmi_set_environment", "ptmi_environment_info", "ptmi_host_env_table"):
        assert name in ptmi.EXPORTS and hasattr(L, name)
    import ptmi_scenes
    m = ptmi_scenes.sky(32, 16)
    assert m.shape == (16, 32, 3) and m.dtype == F and (m >= 0).all() and (m[..., 0] > 100).sum() == 1
