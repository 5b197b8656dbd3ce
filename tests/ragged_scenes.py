"""Scenes of exactly n primitives for tests/test_gpu_radiosity_ragged.py, the table of solver cases that file runs, and
the oracle's solution of each case (computed once per process and shared; callers must not write into it).

random_scene(n): n small planar parallelograms scattered in a cube - dense enough that a fifth of all pairs see each other
(so no row sum, no 256-column tile and no last row or column of the form-factor matrix is empty), sparse enough that the
oracle solves 2052 of them point-to-point in under a second."""
import functools

import numpy as np

from oracle_binding import OracleScene

F = np.float32


def random_scene(n, quads=True):
    """centres uniform in [-2, 2]^3; each primitive a parallelogram spanned by two orthonormal random directions, side
    0.125 - 0.25; with quads about 40 % stay quads (v00, v10, v11, v01), the rest are the triangle (v00, v10, v11) with
    verts[:, 3] = 0; normal = (v1 - v0) x (v2 - v0); Kd uniform in [0.2, 0.9]; one primitive in ten (the first always)
    emits, Le in [1, 5]; the generator is seeded by n.  Up to n = 3 the primitives stand on a circle instead and face
    its centre, every second one a quad."""
    rng = np.random.default_rng(n)
    c = rng.uniform(-2.0, 2.0, (n, 3))
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = rng.normal(size=(n, 3)); w -= (w * u).sum(1, keepdims=True) * u; w /= np.linalg.norm(w, axis=1, keepdims=True)
    is_quad = rng.uniform(size=n) < 0.4
    if n <= 3:
        # two or three random primitives do not see each other: put them on a circle, facing its centre (u x w = the normal)
        a = 2.0 * np.pi * np.arange(n) / 3.0
        c = np.stack([np.cos(a), np.sin(a), 0.1 * np.arange(n)], 1)
        inward = np.stack([-np.cos(a), -np.sin(a), np.zeros(n)], 1)
        w = np.tile([[0.0, 0.0, 1.0]], (n, 1)); u = np.cross(w, inward)
        is_quad = np.arange(n) % 2 == 1
    hu = u * rng.uniform(0.0625, 0.125, (n, 1)); hw = w * rng.uniform(0.0625, 0.125, (n, 1))
    verts = np.stack([c - hu - hw, c + hu - hw, c + hu + hw, c - hu + hw], 1).astype(F)
    types = (is_quad & bool(quads)).astype(np.int32)
    verts[types == 0, 3] = 0
    e1 = verts[:, 1].astype(np.float64) - verts[:, 0]; e2 = verts[:, 2].astype(np.float64) - verts[:, 0]
    nr = np.cross(e1, e2); nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    bsdf = rng.uniform(0.2, 0.9, (n, 3)).astype(F)
    emits = rng.uniform(size=n) < 0.1
    emits[0] = True
    Le = (rng.uniform(1.0, 5.0, (n, 3)) * emits[:, None]).astype(F)
    return types, verts, nr.astype(F), bsdf, Le


def facing_receiver(scene, e):
    """the primitive nearest to e among those whose centre lies in front of e and sees e's centre from its own front"""
    _, verts, nr, _, _ = scene
    k = np.where(scene[0] == 1, 4, 3)[:, None]
    c = verts.astype(np.float64).sum(1) / k
    d = c - c[e]
    r = np.linalg.norm(d, axis=1); r[e] = np.inf
    ok = ((d * nr[e]).sum(1) > 0) & ((-d * nr).sum(1) > 0)
    assert ok.any()
    return int(np.argmin(np.where(ok, r, np.inf)))


def nonfinite_scene(n, emitter):
    """random_scene(n) of triangles in which primitive `emitter` has Le = (inf, 0, 3e38) and the receiver that faces it
    from nearest has a red Kd of exactly 0; returns (scene, receiver)"""
    sc = random_scene(n, quads=False)
    types, verts, nr, bsdf, Le = sc
    Le[emitter] = [np.inf, 0.0, 3e38]
    rcv = facing_receiver(sc, emitter)
    bsdf[rcv, 0] = 0.0
    return sc, rcv


MC4 = dict(mc_samples=4)
P2P = dict(use_monte_carlo=False)

# id -> (n, quads, solver parameters).  Which Jacobi kernel a size takes: the tiled one iff n % 4 == 0 and n >= 64.
CASES = {
    # n - 1 clamps, one nearly empty workgroup; n = 1 has no pair at all
    "n1":    (1, False, dict(MC4, num_iterations=1)),
    "n2":    (2, True, dict(MC4, num_iterations=3)),
    "n3":    (3, False, dict(P2P, num_iterations=1)),
    # around the launch rule: 63 lane-per-row, 64 tiled (one 64-column tile, exactly 8 row groups), 65 lane-per-row with a
    # second workgroup of one live lane, 68 tiled with a last group of 4 live rows
    "n63":   (63, True, dict(MC4, num_iterations=3)),
    "n64":   (64, False, dict(MC4, num_iterations=3)),
    "n65":   (65, False, dict(mc_samples=5, num_iterations=1)),
    "n68":   (68, True, dict(MC4, num_iterations=3)),
    "n196":  (196, True, dict(MC4, num_iterations=3)),
    # one 256-column tile to two; the certified visibility walk from 256 up; the form-factor kernel's second column block
    # holds 0, 1 or 4 live lanes
    "n252":  (252, False, dict(P2P, num_iterations=3)),
    "n255":  (255, True, dict(MC4, num_iterations=1)),
    "n256":  (256, True, dict(MC4, num_iterations=3)),
    "n257":  (257, False, dict(MC4, num_iterations=3)),
    "n260":  (260, False, dict(mc_samples=7, num_iterations=1, enable_filtering=True, use_bilateral=True)),
    # three tiles, the last of 4 columns; 516 % 8 = 4
    "n516":  (516, True, dict(MC4, num_iterations=3, enable_filtering=True, use_bilateral=False, filter_sigma_spatial=0.7)),
    # the lane-per-row kernel's 1024-entry LDS chunk border (a second chunk of one entry); five tiles
    "n1025": (1025, True, dict(P2P, num_iterations=3)),
    "n1028": (1028, False, dict(P2P, num_iterations=3)),
    # ptmi_radiosity_grid's 2048-entry chunk border with 1 and 4 entries left, on both Jacobi kernels
    "n2049": (2049, False, dict(P2P, num_iterations=1)),
    "n2052": (2052, True, dict(P2P, num_iterations=3)),
    # one Jacobi step, for the binary64 restatement
    "n1025_step": (1025, True, dict(P2P, num_iterations=1)),
    "n1028_step": (1028, False, dict(P2P, num_iterations=1)),
}
SIZE_CASES = [k for k in CASES if "_" not in k]
ENV_CASES = ["n68", "n196", "n1028", "n2052"]                  # solved by the child processes of the environment-selected kernels

# id -> (n, emitter, solver parameters): the emitter's column is 3 mod 4 (the last component of a float4 of the tile).
# nf260: the emitter lies in the first tile, so that tile takes the compare / select loop and the 4-column tile after it
# the fast one, in the same launch.  nf1028: the other way round - the partial fifth tile is the non-finite one - and two
# more steps in which every tile holds an infinite unshot value.
NONFINITE_CASES = {
    "nf260":  (260, 103, dict(MC4, num_iterations=1)),
    "nf1028": (1028, 1027, dict(P2P, num_iterations=3)),
}


def tiled(n):
    """launch_radiosity_iteration's rule"""
    return n % 4 == 0 and n >= 64


@functools.lru_cache(maxsize=None)
def case_scene(case):
    if case in NONFINITE_CASES:
        n, e, _ = NONFINITE_CASES[case]
        return nonfinite_scene(n, e)[0]
    n, quads, _ = CASES[case]
    return random_scene(n, quads)


def case_params(case):
    return dict((NONFINITE_CASES.get(case) or CASES[case])[2])


@functools.lru_cache(maxsize=None)
def oracle_case(case):
    """(OracleScene after the solve, its solution, its CDF records) - shared, read-only"""
    o = OracleScene.from_arrays(*case_scene(case))
    sol = o.radiosity_solve(**case_params(case))
    cd = o.cdfs()
    for a in list(sol.values()) + [cd]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return o, sol, cd


# ---- every form-factor kernel once (test_gpu_every_form_factor_kernel_is_the_oracles) ----------------------------------------
def deep_chain(mixed):
    """tests/test_radiosity_solver.py's 60-primitive chain whose tree is deeper than 31 levels (x falls by 2.2 per primitive from
    2^40), facing each other in turn; mixed: every fourth primitive is the quad over the same base edge"""
    n = 60
    x = (2.0 ** 40 * 2.2 ** (-np.arange(n, dtype=np.float64))).astype(F)
    verts = np.zeros((n, 4, 3), F)
    types = np.zeros(n, np.int32)
    for i in range(n):
        z = F(i) * F(0.01)
        verts[i, 0] = [x[i], -0.004, z]; verts[i, 1] = [x[i], 0.004, z]; verts[i, 2] = [x[i], 0.0, z + F(0.008)]
        if mixed and i % 4 == 3:
            types[i] = 1
            verts[i, 2] = [x[i], 0.004, z + F(0.008)]; verts[i, 3] = [x[i], -0.004, z + F(0.008)]
    nr = np.tile(np.array([[1, 0, 0]], F), (n, 1)); nr[::2] = [-1, 0, 0]
    return types, verts, nr, np.full((n, 3), 0.5, F), np.ones((n, 3), F)


FF_SCENES = {"tri68": lambda: random_scene(68, False), "mixed68": lambda: random_scene(68, True),
             "deep_tri": lambda: deep_chain(False), "deep_mixed": lambda: deep_chain(True)}
# Monte-Carlo with and without the kernel's own radiosity grid (RAD0: num_iterations == 0); point-to-point launches one kernel
# whatever num_iterations is
FF_MODES = {"mc_it0": dict(mc_samples=6, num_iterations=0), "mc_it1": dict(mc_samples=6, num_iterations=1),
            "p2p_it1": dict(use_monte_carlo=False, num_iterations=1)}
# (scene, walk asked for, mode): 2 primitive mixes x 3 walks x 3 modes + the deep tree (walk 0 only) x 2 mixes x 3 modes = the 24
# instantiations of ptmi_form_factors that launch_form_factors can reach
FF_KERNEL_CASES = [(sc, w, m) for sc in ("tri68", "mixed68") for w in (0, 1, 2) for m in FF_MODES] + \
                  [(sc, 0, m) for sc in ("deep_tri", "deep_mixed") for m in FF_MODES]


@functools.lru_cache(maxsize=None)
def ff_scene(name):
    return FF_SCENES[name]()


@functools.lru_cache(maxsize=None)
def ff_oracle(name, mode):
    """the oracle's solution of a scene of FF_SCENES in a mode of FF_MODES - shared, read-only"""
    sol = OracleScene.from_arrays(*ff_scene(name)).radiosity_solve(**FF_MODES[mode])
    for a in sol.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sol
