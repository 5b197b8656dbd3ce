"""The edge set of the participating medium's per-call functions (include/ptmi.h: "participating medium"), shared by the host test
(tests/test_medium_host.py: the restatement against binary64 geometry) and the GPU test (tests/test_gpu_medium.py: the kernel's
functions against the restatement, bit for bit).  A case is (name, o, d, t_end, nonempty) over BOX; nonempty None where the
answer hangs on a rounding (a ray that grazes an edge)."""
import numpy as np

F = np.float32
LO, HI = (-1.0, 0.0, -3.0), (2.0, 4.0, 1.0)
INF = float("inf")
S2 = float(F(np.sqrt(0.5)))
S3 = float(F(np.sqrt(1.0 / 3.0)))
L41 = float(np.sqrt(41.0))                # the length of the box's diagonal (3, 4, 4)

SEGMENTS = [
    # the origin inside, outside, on a face
    ("inside +x", (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), INF, True),
    ("inside -y", (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), INF, True),
    ("inside diagonal", (0.5, 2.0, -1.0), (S3, S3, -S3), INF, True),
    ("outside towards", (-5.0, 1.0, 0.0), (1.0, 0.0, 0.0), INF, True),
    ("outside away", (-5.0, 1.0, 0.0), (-1.0, 0.0, 0.0), INF, False),
    ("outside diagonal", (-3.0, -2.0, -5.0), (S3, S3, S3), INF, True),
    ("on a face inwards", (-1.0, 1.0, 0.0), (1.0, 0.0, 0.0), INF, True),
    ("on a face outwards", (-1.0, 1.0, 0.0), (-1.0, 0.0, 0.0), INF, False),
    ("on a face along it", (-1.0, 1.0, 0.0), (0.0, 1.0, 0.0), INF, True),
    ("on a face along it, -0 direction", (2.0, 1.0, 0.0), (-0.0, 0.0, 1.0), INF, True),
    # parallel to a slab, inside it and outside it
    ("parallel inside", (0.0, 1.0, -10.0), (0.0, 0.0, 1.0), INF, True),
    ("parallel outside x", (3.0, 1.0, -10.0), (0.0, 0.0, 1.0), INF, False),
    ("parallel outside y below", (0.0, -0.5, -10.0), (0.0, 0.0, 1.0), INF, False),
    ("parallel to two slabs, outside one", (-6.0, 5.0, 0.0), (1.0, 0.0, 0.0), INF, False),
    # through an edge and through a corner
    ("in through an edge", (-2.0, -1.0, 0.0), (S2, S2, 0.0), INF, True),
    ("touching an edge", (-2.0, 1.0, 0.0), (S2, -S2, 0.0), INF, None),
    ("just inside an edge", (-2.0, 1.5, 0.0), (S2, -S2, 0.0), INF, True),
    ("just outside an edge", (-2.0, 0.5, 0.0), (S2, -S2, 0.0), INF, False),
    ("in through a corner", (-2.0, -1.0, -4.0), (S3, S3, S3), INF, True),
    ("through two corners", (-1.75, -1.0, -4.0), (3.0 / L41, 4.0 / L41, 4.0 / L41), INF, True),
    ("touching a corner", (-2.0, 1.0, -3.0), (S2, -S2, 0.0), INF, None),
    # t_end before the box, inside it and behind it
    ("t_end before", (-5.0, 1.0, 0.0), (1.0, 0.0, 0.0), 3.5, False),
    ("t_end at the entry", (-5.0, 1.0, 0.0), (1.0, 0.0, 0.0), 4.0, False),
    ("t_end inside", (-5.0, 1.0, 0.0), (1.0, 0.0, 0.0), 5.5, True),
    ("t_end at the exit", (-5.0, 1.0, 0.0), (1.0, 0.0, 0.0), 7.0, True),
    ("t_end behind", (-5.0, 1.0, 0.0), (1.0, 0.0, 0.0), 9.0, True),
    ("t_end inside, origin inside", (0.0, 1.0, 0.0), (0.0, 0.0, -1.0), 0.25, True),
    ("t_end 0", (0.0, 1.0, 0.0), (0.0, 0.0, -1.0), 0.0, False),
    # a miss
    ("a miss beside", (-5.0, 1.0, 5.0), (1.0, 0.0, 0.0), INF, False),
    ("a miss diagonal", (-5.0, 10.0, 0.0), (S2, S2, 0.0), INF, False),
    ("a denormal direction component", (0.0, 1.0, 0.0), (1e-42, 1.0, 0.0), INF, True),
]

G_VALUES = (-0.9, -0.3, 0.0, 0.3, 0.9)
TINY = float(F(2.0 ** -33))
EDGE_U = (TINY, 0.5, 1.0)
SIGMAS = (0.05, 0.75, 40.0)


def block(sigma_t=0.75, g=0.0, albedo=(0.25, 0.5, 1.0), lo=LO, hi=HI):
    out = np.zeros((3, 4), F)
    out[0, :3], out[0, 3] = lo, sigma_t
    out[1, :3], out[1, 3] = hi, g
    out[2, :3] = albedo
    return out


def call_inputs(blk, o, d, t_end, u):
    """one case of ptmi_debug_medium_call: 20 floats"""
    return np.concatenate([np.asarray(blk, F).reshape(12), np.asarray(o, F), np.asarray(d, F), [F(t_end), F(u)]]).astype(F)


def curand_uniforms(rng, shape):
    """uniforms as the stream makes them: x * 2^-32 + 2^-33 of a 32-bit x, in binary32"""
    x = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(F)
    return (x * F(2.3283064e-10) + F(2.3283064e-10 / 2.0)).astype(F)


def random_cases(n, seed=5):
    """n random (block, o, d, t_end, u): boxes, rays from inside and outside, finite and infinite ends, every g of G_VALUES"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        lo = rng.uniform(-4, 0, 3); hi = lo + rng.uniform(0.5, 6, 3)
        blk = block(float(rng.choice(SIGMAS)), float(rng.choice(G_VALUES)), rng.uniform(0, 1, 3), lo, hi)
        o = rng.uniform(-8, 8, 3) if i % 2 else rng.uniform(lo, hi)
        d = rng.normal(size=3)
        if i % 7 == 0:
            d[rng.integers(0, 3)] = 0.0
        d = (d / np.linalg.norm(d)).astype(F)
        t_end = INF if i % 3 == 0 else float(rng.uniform(0.0, 12.0))
        out.append((blk, o.astype(F), d, t_end, float(curand_uniforms(rng, 1)[0])))
    return out
