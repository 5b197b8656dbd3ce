"""The constructed scenes and rays of tests/test_gpu_sweep_masked.py and tests/test_sweep_shared_s_host.py: triangles only, a few
primitives each, placed in front of the default camera.  No GPU is needed to build or to check them.

  tri1         one triangle: the root is a leaf, a single record
  pair         a quad cut into the fan (a, b, c), (a, c, d): two records with the same v0 in one leaf
  twins        the same triangle twice in one leaf: every ray that meets one meets both at the same t, bit for bit
  fan5         five triangles with the same v0 and the same centroid: the builder cannot split them, one leaf of five, so its
               last record is the first of the second trip of the sweep's four-way leaf loop
  pairs_apart  two fan pairs and two single triangles, laid out so that the builder puts the halves of each pair into different
               leaves: records with the same v0 that are NOT neighbours in a leaf
  zero_pair    two triangles in one leaf whose v0 are (+0, y, z) and (-0, y, z): equal as floats, different as bits
  cbox         cbox.obj
"""
import functools
import os

import numpy as np

from oracle_binding import OracleScene, SCENES

F = np.float32
NAMES = ["tri1", "pair", "twins", "fan5", "pairs_apart", "zero_pair", "cbox"]


def _arrays(tris):
    tris = np.asarray(tris, np.float64)
    n = len(tris)
    verts = np.zeros((n, 4, 3), F)
    verts[:, :3] = tris
    verts[:, 3] = verts[:, 2]
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    normal = np.cross(e1, e2)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    rng = np.random.default_rng(n)
    Le = np.zeros((n, 3), F)
    Le[0] = 3.0                                                  # an emitter in every scene
    return np.zeros(n, np.int32), verts, normal.astype(F), rng.uniform(0.3, 0.9, (n, 3)).astype(F), Le


def _quad_fan(a, b, c, d):
    return [(a, b, c), (a, c, d)]


@functools.lru_cache(maxsize=None)
def arrays(name):
    if name == "cbox":
        p = OracleScene.load(os.path.join(SCENES, "cbox.obj")).prims()
        return p["type"], p["verts"], p["normal"], p["bsdf"], p["Le"]
    if name == "tri1":
        return _arrays([((-1.5, 1.0, 0.25), (1.75, 1.5, -0.5), (0.25, 4.0, 0.5))])
    if name == "pair":
        return _arrays(_quad_fan((-1.5, 1.0, 0.0), (1.5, 1.25, -0.5), (1.75, 4.0, 0.25), (-1.25, 3.75, 0.5)))
    if name == "twins":
        t = ((-1.5, 1.0, 0.25), (1.75, 1.5, -0.5), (0.25, 4.0, 0.5))
        return _arrays([t, t])
    if name == "fan5":
        a, c = np.array([0.0, 1.0, 0.0]), np.array([0.5, 7.0, 0.25])         # every blade is (a, p, c - p): centroid (a + c) / 3
        ps = [(-2.0, 3.0, 0.5), (-1.5, 2.5, -0.25), (-1.0, 4.5, 0.75), (-0.5, 2.0, -0.5), (-2.5, 4.0, 0.0)]
        return _arrays([(a, np.array(p), c - np.array(p)) for p in ps])
    if name == "pairs_apart":
        # along x: single, first half of A | second half of A, first half of B | second half of B, single - long thin halves
        # whose centroids lie far apart
        A = _quad_fan((-0.5, 1.0, 0.0), (-3.5, 1.5, 0.25), (-0.25, 2.25, 0.5), (3.0, 1.75, -0.25))
        B = _quad_fan((0.5, 3.0, -0.5), (-3.25, 3.5, 0.0), (0.25, 4.25, 0.25), (3.5, 3.75, 0.5))
        singles = [((-3.0, 4.5, 0.0), (-2.0, 4.75, 0.5), (-2.5, 5.0, -0.25)), ((2.0, 0.25, 0.0), (3.0, 0.5, 0.25), (2.5, 0.75, -0.5))]
        return _arrays(A + B + singles)
    if name == "zero_pair":
        arrs = _arrays([((0.0, 1.0, 0.5), (1.75, 1.5, -0.5), (1.5, 4.0, 0.25)), ((0.0, 1.0, 0.5), (-1.75, 4.25, 0.0), (-1.5, 1.25, -0.25))])
        arrs[1][1, 0, 0] = -0.0
        return arrs
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle(name):
    return OracleScene.from_arrays(*arrays(name))


def leaf_order(host_scene):
    """(v0 bits per leaf-order slot as uint32 [n, 3], source primitive per slot, [(first slot, count)] of the leaves in pre-order)"""
    b, p = host_scene.bvh(), host_scene.prims()
    src = b["indices"]
    v0 = np.ascontiguousarray(p["verts"][src][:, 0], F).view(np.uint32)
    leaves = [(int(b["left"][i]), int(b["count"][i])) for i in range(len(b["left"])) if b["count"][i] > 0]
    return v0, src, leaves


def same_origin_marks(v0, leaves):
    """per leaf-order slot: not the first record of its leaf, and v0 equal AS BITS to the record before it in the leaf"""
    mark = np.zeros(len(v0), bool)
    for first, count in leaves:
        for k in range(first + 1, first + count):
            mark[k] = bool((v0[k] == v0[k - 1]).all())
    return mark
