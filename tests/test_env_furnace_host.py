"""Environment lighting against analytic values on the CPU (include/ptmi.h, "environment lighting") - no GPU.  The restatement of
the contract (tests/path_oracle.py with tests/env_oracle.py) alone must reach the values tests/test_gpu_env_expectation.py holds the GPU to: that shows
the contract itself unbiased, and the chosen inputs inside the noise cap, before any kernel runs.

Every case renders 16 x 16 pixels; a pixel has its own stream, so the pixel-to-pixel spread gives the standard error, and the
sample count is what brings 5 SE under 0.5 % of the value.  The scalar restatement makes about 10^4 samples a second: the cube
and the open furnaces run through it; under the sun the plain estimator needs 10^7 samples, so those cases run the contract's
vertex vectorised in binary64 (env_oracle.vertex_samples), which is first checked against the scalar functions draw for draw.
"""
import numpy as np
import pytest

import env_oracle as EO
import env_scenes as ES
import path_oracle as PO
from oracle_binding import OracleScene, default_camera

SIZE = 16
Z_MAX = 5.0
CAP = ES.CAP


def stats(px, value):
    """(mean, SE) per channel of independent pixel estimates; a floor of 2e-5 of the value on the SE absorbs float rounding
    where an estimator has no variance"""
    px = np.asarray(px, np.float64).reshape(-1, np.size(value))
    se = px.std(0, ddof=1) / np.sqrt(len(px))
    return px.mean(0), np.maximum(se, 2e-5 * np.abs(value))


def check(tag, px, value, lower=None):
    """|mean - value| < 5 SE and 5 SE <= 0.5 % of the value; with `lower`, the expectation may lie anywhere in [lower, value]"""
    value = np.atleast_1d(np.asarray(value, np.float64))
    mean, se = stats(px, value)
    below = (value if lower is None else np.atleast_1d(lower)) - mean
    z = np.maximum(mean - value, below) / se
    print(f"{tag}: mean {mean}, value {value}, SE {se}, z {z}")
    assert (Z_MAX * se <= CAP * np.abs(value)).all(), (tag, "too noisy to see a bias of 0.5 %", se, value)
    assert (z < Z_MAX).all(), (tag, mean, value, se, z)


# ------------------------------------------------------------------------------------------------
# 1. a convex body under a constant map
# ------------------------------------------------------------------------------------------------
RHO = np.array((0.3, 0.5, 0.7)); L0 = np.array((0.5, 0.4, 0.3)); E = np.array((0.875, 0.75, 0.5))    # few mantissa bits: a pixel's sum of n x E is exact


@pytest.fixture(scope="module")
def cube():
    """(oracle scene, mask of the pixels whose four corners all hit the cube - the body is convex, so the whole pixel does -
    and mask of the pixels that lie outside the bounding box of the cube's projected vertices, which no ray of theirs can hit)"""
    import oracle_binding as OB
    body = ES.cube(RHO, L0, half=1.75)
    o = OracleScene.from_arrays(*body.arrays())
    cf = OB.camera_frame(default_camera(), SIZE, SIZE)
    corner = np.zeros((SIZE + 1, SIZE + 1), bool)
    for y in range(SIZE + 1):
        for x in range(SIZE + 1):
            ro, rd = OB.camera_ray(cf, x / SIZE, y / SIZE)
            corner[y, x] = bool(o.intersect(ro, rd).hit)
    inside = corner[:-1, :-1] & corner[1:, :-1] & corner[:-1, 1:] & corner[1:, 1:]
    org, llc, hor, ver = (np.array(getattr(cf, k)[:], np.float64) for k in ("origin", "lower_left_corner", "horizontal", "vertical"))
    pts = np.array(body.v, np.float64)[:, :3].reshape(-1, 3)
    uv = np.array([np.linalg.solve(np.stack([hor, ver, -(p - org)], 1), org - llc)[:2] for p in pts]) * SIZE
    lo, hi = np.floor(uv.min(0) - 1e-6), np.ceil(uv.max(0) + 1e-6)
    xs = np.arange(SIZE)
    out_x = (xs + 1 <= lo[0]) | (xs >= hi[0]); out_y = (xs + 1 <= lo[1]) | (xs >= hi[1])
    outside = out_y[:, None] | out_x[None, :]
    assert inside.sum() >= 60 and outside.sum() >= 20 and not (inside & outside).any()
    return o, inside, outside


def test_cube_plain_estimator_is_exact_per_sample(cube):
    o, inside, outside = cube
    for depth, value in ((1, L0), (2, L0 + RHO * E), (5, L0 + RHO * E)):
        _, rad = PO.EnvRenderer(o, default_camera(), SIZE, SIZE, ES.constant_map(E), False).frame(2, depth)
        assert np.abs(rad[inside].astype(np.float64) / value - 1.0).max() < 1e-6, depth
        assert (rad[outside] == E.astype(np.float32)).all(), depth


def test_cube_with_next_event(cube):
    o, inside, outside = cube
    r = PO.EnvRenderer(o, default_camera(), SIZE, SIZE, ES.constant_map(E), True)
    _, rad = r.frame(2, 1)
    assert np.abs(rad[inside].astype(np.float64) / L0 - 1.0).max() < 1e-6
    # the emitter half of the light samples (q = 0.5) finds nothing from a convex body's own surface; the environment half and
    # the BSDF ray share rho * E by their weights.  Measured: 5 SE = 0.28 % of the value at 256 spp over these pixels -> 128 spp:
    # 0.39 %.
    _, rad = PO.EnvRenderer(o, default_camera(), SIZE, SIZE, ES.constant_map(E), True).frame(128, 2)
    check("cube NEE depth 2", rad[inside], L0 + RHO * E)
    assert (rad[outside] == E.astype(np.float32)).all()


# ------------------------------------------------------------------------------------------------
# 2. the ground quad under a sun: the contract's vertex, vectorised
# ------------------------------------------------------------------------------------------------
def test_the_vectorised_vertex_is_the_scalar_restatement():
    """same draws, same texels, same directions and lookups (to binary64-vs-float32 rounding)"""
    env, _, _, _ = ES.sun_case(35.0, 70.0)
    tab = EO.table(env, 1.0, 70.0)
    rng = np.random.default_rng(3)
    u = (1.0 - rng.random((300, 4))).astype(np.float32)
    r, j, wi = EO.vertex_directions(tab, *(u[:, k].astype(np.float64) for k in range(4)))
    rl, jl = EO._lookup_many(tab, wi)
    for k in range(len(u)):
        rs, js, ws = EO.sample_direction(tab, *u[k])
        assert (rs, js) == (r[k], j[k])
        assert np.abs(ws.astype(np.float64) - wi[k]).max() < 2e-6
        if min(u[k, 2], 1 - u[k, 2], u[k, 3], 1 - u[k, 3]) > 1e-3:
            assert EO.lookup(tab, ws) == (rl[k], jl[k]) == (rs, js)
    assert set(zip(r.tolist(), j.tolist())) >= {(ES.SUN_ROW, ES.SUN_COL)}     # the sun is found


def test_the_sun_arithmetic():
    """The choice of the sun's radiance.  F_s = (z_3^2 - z_4^2) / 32 = 0.19134 / 32 = 0.005979 is the largest form factor a
    texel of a 32 x 16 map has.  Per unit albedo, with a sun texel of radiance a over a sky of 1:
        V = 1 + (a - 1) F_s,   Var = (1 - F_s) + a^2 F_s - V^2 per sample,   N = 128^2 x 1024 = 16 777 216 samples.
    Half the irradiance from the sun means (a - 1) F_s = 1: a = 168, V = 2, Var = 165.7, 5 sqrt(Var / N) = 0.0157 = 0.79 % of V -
    over the cap.  The cap itself, with a tenth of margin, 5 sqrt(Var / N) = 0.9 x 0.005 V, gives a = 67: V = 1.3946, Var = 25.89,
    5 SE = 0.445 % of V, and the sun carries 0.3946 / 1.3946 = 28 % of the irradiance - the brightest one-texel sun this size
    can hold to 0.5 %."""
    env, Fm, v, var = ES.sun_case()
    fs = Fm[ES.SUN_ROW, ES.SUN_COL]
    assert abs(fs - 0.005979) < 1e-6 and fs == Fm.max() and abs(Fm.sum() - 1.0) < 1e-12
    assert env[ES.SUN_ROW, ES.SUN_COL, 0] == 67.0
    assert abs(v - (1.0 + 66.0 * fs)) < 1e-12 and abs(var - ((1.0 - fs) + 67.0 ** 2 * fs - v * v)) < 1e-9
    assert 0.27 < 66.0 * fs / v < 0.29
    for case in ((0.0, 0.0), (35.0, 70.0)):
        _, _, v, var = ES.sun_case(*case)
        assert 0.85 * CAP * v < 5.0 * np.sqrt(var / ES.N_GPU) <= 0.9 * CAP * v
    half = (1.0 - fs) + 168.0 ** 2 * fs - 4.0
    assert 5.0 * np.sqrt(half / ES.N_GPU) > CAP * 2.0


@pytest.mark.parametrize("tilt,rot", [(0.0, 0.0), (35.0, 70.0)])
def test_ground_quad_under_the_sun(tilt, rot):
    env, Fm, v, var = ES.sun_case(tilt, rot)
    tab = EO.table(env, 1.0, rot)
    n = ES.tilted_normal(tilt)
    rng = np.random.default_rng(11)
    # NEE: measured variance per sample about 0.3 V^2 -> 2^20 samples: 5 SE = 0.27 % of V
    nee = EO.vertex_samples(tab, n, 1 << 20, rng, True)
    check(f"sun tilt {tilt} NEE", nee.reshape(SIZE * SIZE, -1).mean(1), v)
    # plain: Var is closed form (test_the_sun_arithmetic); 2^22 samples show the mean and the variance, N_GPU meets the cap
    plain = EO.vertex_samples(tab, n, 1 << 22, rng, False)
    px = plain.reshape(SIZE * SIZE, -1).mean(1)
    mean, se = stats(px, v)
    assert abs(mean[0] - v) < Z_MAX * se[0], (mean, v, se)
    assert abs(plain.var() / var - 1.0) < 0.03, (plain.var(), var)
    assert nee.var() < plain.var() / 5.0
    print(f"sun tilt {tilt}: variance per sample plain {plain.var():.3f} (closed form {var:.3f}), NEE {nee.var():.3f}")


def test_the_scalar_restatement_under_the_sun():
    """the whole path through the scalar restatement at a count it can afford: within 5 of its own SE (no cap)"""
    env, _, v, _ = ES.sun_case()
    rho = np.array((0.3, 0.5, 0.7))
    o = OracleScene.from_arrays(*ES.ground_quad(rho).arrays())
    _, rad = PO.EnvRenderer(o, ES.top_down_camera(), SIZE, SIZE, env, True).frame(16, 3)
    mean, se = stats(rad, rho * v)
    assert (np.abs(mean - rho * v) < Z_MAX * se).all(), (mean, rho * v, se)
    assert (se < 0.02 * rho * v).all()


# ------------------------------------------------------------------------------------------------
# 3. open furnaces: Le = (1 - rho) E on every primitive under a constant map E
# ------------------------------------------------------------------------------------------------
F_RHO = np.array((0.3, 0.4, 0.5)); F_E = np.array((1.0, 0.75, 0.5)); DEPTH = 12


def open_furnace(name):
    s = ES.without_box(name)
    s.b = [tuple(F_RHO)] * len(s); s.e = [tuple((1.0 - F_RHO) * F_E)] * len(s)
    return s


@pytest.mark.parametrize("name,q", [("tris_many", 0.25), ("quads_many", 0.75)])
def test_open_furnace(name, q):
    """every path vertex adds (1 - rho) E and passes rho on, a path that escapes adds the rest, E: the value is E at any depth
    the path still lives at, and at least E (1 - rho^D) when it is cut at D.  rho^12 <= 2.5e-4."""
    assert (F_RHO ** DEPTH <= 2.5e-4).all()
    o = OracleScene.from_arrays(*open_furnace(name).arrays())
    # measured at 64 spp, blue (the noisiest channel): 5 SE = 0.53 % of the value with the quads at q = 0.75 -> 96 spp: 0.43 %
    r = PO.EnvRenderer(o, default_camera(), SIZE, SIZE, ES.constant_map(F_E), True, select_fraction=q)
    _, rad = r.frame(96, DEPTH)
    check(f"{name} q {q}", rad, F_E, lower=F_E * (1.0 - F_RHO ** DEPTH))
