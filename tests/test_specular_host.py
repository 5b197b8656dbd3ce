"""Host half of the specular surfaces (include/ptmi.h, "specular surfaces"): the restatement's reflection, refraction and Fresnel
term (tests/specular_oracle.py) against binary64 Snell and Fresnel, ptmi_check_surfaces, ptmi_scenes.cornell_blocks, and the
estimator's draws.  No GPU."""
import os

import numpy as np
import pytest

import env_scenes as ES
import path_oracle as PO
import ptmi
import ptmi_scenes
import specular_oracle as SO
import specular_scenes as SS
from oracle_binding import OracleScene, SCENES, default_camera

F = np.float32
CBOX = os.path.join(SCENES, "cbox.obj")
CBOX_QUADS = os.path.join(SCENES, "cbox_quads.obj")
TOL = 1e-6


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def direction(theta, normal=(0.0, 1.0, 0.0), tangent=(1.0, 0.0, 0.0)):
    """a unit direction arriving at angle theta from `normal`, travelling against it, in the plane of `tangent` (binary64)"""
    n, t = np.asarray(normal, np.float64), np.asarray(tangent, np.float64)
    return np.sin(theta) * t - np.cos(theta) * n


def fresnel64(n_i, n_t, theta):
    """(F, rs, rp, theta_t) of an unpolarised wave in binary64; total internal reflection: (1, None, None, None)"""
    s = n_i / n_t * np.sin(theta)
    if s >= 1.0:
        return 1.0, None, None, None
    tt = np.arcsin(s)
    ci, ct = np.cos(theta), np.cos(tt)
    rs = (n_i * ci - n_t * ct) / (n_i * ci + n_t * ct)
    rp = (n_t * ci - n_i * ct) / (n_t * ci + n_i * ct)
    return 0.5 * (rs * rs + rp * rp), rs, rp, tt


# ------------------------------------------------------------------------------------------------
# reflect, refract, fresnel against binary64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta_deg", [0.0, 10.0, 45.0, 56.30993247402021, 80.0, 89.9])
@pytest.mark.parametrize("ior", [1.0, 1.33, 1.5, 2.4, 8.0])
def test_fresnel_and_refraction_from_outside(theta_deg, ior):
    th = np.radians(theta_deg)
    n = np.array([0.0, 1.0, 0.0], F)
    d = direction(th).astype(F)
    un, eta, ci = SO.interface(d, n, ior)
    assert abs(float(eta) - 1.0 / ior) < TOL and abs(float(ci) - np.cos(th)) < TOL
    Fr, ct = SO.fresnel(eta, ci)
    F64, _, _, tt = fresnel64(1.0, ior, th)
    assert abs(float(Fr) - F64) < TOL, (float(Fr), F64)
    nxt = SO.refract(d, un, eta, ci, ct).astype(np.float64)
    expect = direction(tt)                                   # Snell: the same plane, angle theta_t from -n
    assert np.abs(nxt - expect).max() < TOL
    assert abs(np.linalg.norm(nxt) - 1.0) < TOL
    r = SO.reflect(d, un).astype(np.float64)
    assert np.abs(r - (np.sin(th) * np.array([1.0, 0, 0]) + np.cos(th) * np.array([0, 1.0, 0]))).max() < TOL


def test_normal_incidence_brewster_and_grazing():
    n = np.array([0.0, 1.0, 0.0], F)
    _, eta, ci = SO.interface(direction(0.0).astype(F), n, 1.5)
    assert abs(float(SO.fresnel(eta, ci)[0]) - 0.04) < TOL
    # Brewster's angle atan(1.5): the p-polarised amplitude vanishes, F = rs^2 / 2
    th = np.arctan(1.5)
    _, eta, ci = SO.interface(direction(th).astype(F), n, 1.5)
    Fr, ct = SO.fresnel(eta, ci)
    rp = F(F(ci - F(eta * ct)) / F(ci + F(eta * ct)))
    _, rs64, rp64, _ = fresnel64(1.0, 1.5, th)
    assert abs(float(rp)) < TOL and abs(rp64) < 1e-12
    assert abs(float(Fr) - 0.5 * rs64 * rs64) < TOL
    # grazing: F -> 1
    prev = 0.0
    for deg in (80.0, 89.0, 89.9, 89.99, 90.0):
        _, eta, ci = SO.interface(direction(np.radians(deg)).astype(F), n, 1.5)
        Fr = float(SO.fresnel(eta, ci)[0])
        assert Fr >= prev
        prev = Fr
    assert abs(prev - 1.0) < TOL


def test_total_internal_reflection_from_the_critical_angle():
    """inside the body (d along the stored normal): eta = 1.5, and s2 >= 1 exactly from asin(1 / 1.5) on"""
    n = np.array([0.0, 1.0, 0.0], F)
    crit = np.arcsin(1.0 / 1.5)
    for delta, tir in ((-0.3, False), (-0.05, False), (-1e-3, False), (-1e-5, False), (1e-5, True), (1e-3, True), (0.3, True)):
        th = crit + delta
        d = np.array([np.sin(th), np.cos(th), 0.0]).astype(F)                      # leaving: travelling along +n
        un, eta, ci = SO.interface(d, n, 1.5)
        assert eta == F(1.5) and np.array_equal(un, -n)
        Fr, ct = SO.fresnel(eta, ci)
        assert (ct is None) == tir, delta
        if tir or delta <= -0.05:                            # (next to the critical angle F has no bounded slope: only the decision is checked)
            assert abs(float(Fr) - fresnel64(1.5, 1.0, th)[0]) < TOL
        nxt, reflected, _ = SO.scatter(d, n, SO.GLASS, 1.5, F(1.0))                # u = 1: refract wherever F < 1
        assert reflected == tir
        if tir:
            assert np.abs(nxt.astype(np.float64) - np.array([d[0], -d[1], d[2]], np.float64)).max() < TOL
        elif delta <= -0.05:
            tt = fresnel64(1.5, 1.0, th)[3]
            assert np.abs(nxt.astype(np.float64) - np.array([np.sin(tt), np.cos(tt), 0.0])).max() < TOL


@pytest.mark.parametrize("theta_deg", [0.0, 30.0, 75.0, 89.9, 89.999])
@pytest.mark.parametrize("inside", [False, True])
def test_ior_one_passes_straight_through(theta_deg, inside):
    """eta == 1 takes ct = ci: F is 0 and the direction is d, bit for bit, at any angle and from either side"""
    n = np.array([0.0, 1.0, 0.0], F)
    d = direction(np.radians(theta_deg)).astype(F)
    if inside:
        d = -d
    nxt, reflected, Fr = SO.scatter(d, n, SO.GLASS, 1.0, F(1e-7))
    assert not reflected and Fr == 0
    assert np.array_equal(nxt, d)


@pytest.mark.parametrize("kind", [SO.MIRROR, SO.GLASS])
def test_a_tilted_stored_normal_of_any_length_gives_a_unit_direction(kind):
    rng = np.random.default_rng(3)
    for _ in range(50):
        n = (rng.normal(0, 1, 3) * rng.uniform(0.1, 30.0)).astype(F)
        d = rng.normal(0, 1, 3); d = (d / np.linalg.norm(d)).astype(F)
        for u in (F(1e-7), F(1.0)):
            nxt, reflected, _ = SO.scatter(d, n, kind, 1.5, u)
            assert abs(np.linalg.norm(nxt.astype(np.float64)) - 1.0) < 4 * TOL
            un = n.astype(np.float64) / np.linalg.norm(n.astype(np.float64))
            side = np.dot(nxt, un) * np.dot(d.astype(np.float64), un)
            assert (side < 0) == reflected or abs(side) < TOL      # a reflection changes sides of the surface, a refraction keeps going


def test_a_zero_normal_ends_the_path_without_a_direction():
    d = np.array([0.0, 0.0, -1.0], F)
    for kind in (SO.MIRROR, SO.GLASS):
        nxt, _, _ = SO.scatter(d, np.zeros(3, F), kind, 1.5, F(0.5))
        len2 = float(np.dot(nxt, nxt))
        assert not (len2 > 0 and len2 <= PO.FLT_MAX)


# ------------------------------------------------------------------------------------------------
# ptmi_check_surfaces
# ------------------------------------------------------------------------------------------------
def test_check_surfaces_accepts_what_the_header_allows():
    ptmi.check_surfaces([0, 1, 2, 0])
    ptmi.check_surfaces([0, 1, 2], [1.0, 8.0, 1.5])
    ptmi.check_surfaces([2], 1.33)
    L = ptmi.lib()
    assert ptmi.SURFACE_DIFFUSE == 0 and ptmi.SURFACE_MIRROR == 1 and ptmi.SURFACE_GLASS == 2
    k = np.zeros(3, np.int32)
    assert L.ptmi_check_surfaces(3, k.ctypes.data, None) == 0


@pytest.mark.parametrize("kind,ior,word", [
    ([0, 3], None, "kind"), ([-1], None, "kind"), ([2, 1 << 30], None, "kind"),
    ([0, 2], [1.5, np.nan], "ior"), ([0, 2], [np.inf, 1.5], "ior"), ([0, 2], [1.5, -np.inf], "ior"),
    ([2], [0.999], "ior"), ([2], [8.001], "ior"), ([0], [0.0], "ior"), ([1, 0], [1.5, -1.5], "ior"),
])
def test_check_surfaces_rejects(kind, ior, word):
    with pytest.raises(ptmi.PtmiError) as e:
        ptmi.check_surfaces(kind, ior)
    assert word in str(e.value)


def test_check_surfaces_rejects_null_and_empty():
    L = ptmi.lib()
    k = np.zeros(1, np.int32)
    assert L.ptmi_check_surfaces(1, None, None) == -1 and "kind" in L.ptmi_last_error().decode()
    assert L.ptmi_check_surfaces(0, k.ctypes.data, None) == -1 and "n_prims" in L.ptmi_last_error().decode()
    assert L.ptmi_check_surfaces(-4, k.ctypes.data, None) == -1


# ------------------------------------------------------------------------------------------------
# cornell_blocks finds the blocks from the geometry
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,sub,short,tall", [(CBOX, 0, 10, 10), (CBOX_QUADS, 0, 5, 5), (CBOX, 2, 160, 160), (CBOX_QUADS, 1, 20, 20)])
def test_cornell_blocks(path, sub, short, tall):
    hs = ptmi.HostScene.load(path, sub)
    p = hs.prims()
    kind = ptmi_scenes.cornell_blocks(p)
    assert kind.dtype == np.int32 and len(kind) == len(p["type"])
    assert ((kind == 1).sum(), (kind == 2).sum()) == (short, tall)
    top = lambda k: p["verts"][kind == k][:, :3, 1].max()
    assert top(1) < 2.0 < top(2)                              # the short block is the mirror
    assert not p["Le"][kind != 0].any()
    for k in (1, 2):                                          # a block is one run of the file's primitives: nothing else got in
        idx = np.flatnonzero(kind == k)
        assert np.abs(p["verts"][idx][:, :3, 0]).max() < 2.5
    with pytest.raises(ValueError):
        ptmi_scenes.cornell_blocks({k: v[:4] for k, v in p.items()})


# ------------------------------------------------------------------------------------------------
# the estimator: an all-diffuse table changes nothing; the draws of each kind of vertex
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_event", [False, True])
def test_all_diffuse_table_is_the_estimator_without_one(next_event):
    """Every constructor's configuration without next-event estimation, map or table is the reference's estimator: the bits of
    OracleScene.render, which the C oracle computes independently of the path loop.  next_event on, which is all NeeRenderer
    offers, is that estimator where the scene has no emitter - primitives whose Le sums to 0 are none, yet shine.  (That each
    constructor gives what its own loop gave before there was one loop: tests/test_restatement_pinned.py, cases "plain".)"""
    cam = default_camera()
    if next_event:
        arrays = ES.soup()
        arrays[4][0::2] = (2.0, -1.0, -1.0); arrays[4][1::2] = (0.5, 0.5, -1.0)
        o = OracleScene.from_arrays(*arrays)
    else:
        o = OracleScene.load(CBOX)
    _, rad, _ = o.render(cam, 8, 8, 2, max_depth=5)
    assert np.abs(rad).max() > 0
    refs = [PO.EnvRenderer(o, cam, 8, 8, None, next_event), PO.SpecRenderer(o, cam, 8, 8, None, next_event=next_event),
            PO.SpecRenderer(o, cam, 8, 8, np.zeros(o.n_prims, np.int32), next_event=next_event),
            PO.RoughRenderer(o, cam, 8, 8, None, next_event=next_event)]
    if next_event:
        refs.append(PO.NeeRenderer(o, cam, 8, 8))
        assert all(len(r.prim) == 0 for r in refs)
    for ref in refs:
        assert np.array_equal(bits(ref.frame(2, 5)[1]), bits(rad)), type(ref).__name__


@pytest.mark.parametrize("next_event", [False, True])
@pytest.mark.parametrize("depth", [3, 8])
def test_draws_per_vertex(next_event, depth):
    """a mirror vertex draws nothing and a glass vertex one number, beyond the roulette's; a diffuse vertex what it draws today"""
    o = OracleScene.load(CBOX)
    kind = ptmi_scenes.cornell_blocks(o.prims())
    r = PO.SpecRenderer(o, default_camera(), 16, 16, kind, next_event=next_event)
    r.trace = []
    before = r.draws
    r.sums(2, depth)
    seen = {0: 0, 1: 0, 2: 0}
    for k, d, n in r.trace:
        roulette = 1 if d > 2 else 0
        nee = 3 if next_event and d + 1 < depth else 0
        full = {0: roulette + nee + 2, 1: roulette, 2: roulette + 1}[k]
        assert n == full or (roulette and n == 1) or (k == 0 and n == 0), (k, d, n)   # ended by the roulette, or a black surface
        seen[k] += 1
    assert min(seen.values()) > 20
    assert r.draws - before == 2 * r.samples + sum(n for _, _, n in r.trace)          # the camera's two and the vertices': nothing else
    assert r.samples == 16 * 16 * 2


def test_black_furnace_depth_cuts_few_samples():
    """the condition on tests/test_gpu_specular_expectation.py's black furnace: at its max_depth at most 1e-4 of the samples are
    ended by the depth limit (each would miss the wall's Le: a bias fifty times below that test's floor)"""
    s, kind = SS.black_furnace()
    r = PO.SpecRenderer(OracleScene.from_arrays(*s.arrays()), default_camera(), 16, 16, kind)
    r.trace = []
    sums = r.sums(64, SS.BLACK_FURNACE_DEPTH)
    print(f"cut off by max_depth {SS.BLACK_FURNACE_DEPTH}: {r.cut} of {r.samples} samples")
    assert r.samples == 16 * 16 * 64 and r.cut <= 1e-4 * r.samples
    seen = {k for k, _, _ in r.trace}
    assert seen == {0, 1, 2}                                  # the camera does see the panels and the cuboid
    assert np.abs(sums.astype(np.float64).mean((0, 1)) / 64 / np.asarray(SS.FN.LE) - 1.0).max() < 0.01
