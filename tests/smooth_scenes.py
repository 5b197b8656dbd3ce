"""Furnaces of the vertex-normal expectation tests (include/ptmi.h: "vertex normals"), as furnace.Scene objects with their corner-
normal tables - no GPU needed to build them.  A sphere in front of the default camera inside furnace.box."""
import numpy as np

import furnace as FN
import ptmi
import ptmi_scenes
import specular_scenes as SS

F = np.float32
SPHERE_DISTANCE, SPHERE_RADIUS = 5.0, 1.05
SPHERE_LEVEL = 4
# The black furnace's max_depth.  SmoothRenderer on black_sphere() at 64 x 64 x 64 spp (262 144 samples, default camera) cuts off
# 4 samples as a glass sphere (a share of 1.5e-5) and 0 as a mirror sphere at max_depth 32; the condition is a share <= 1e-4.
# The level does not move the glass sphere's share within what these counts resolve (level 2: 2 of 65 536 and level 3: 4 of
# 262 144 at twice the coverage), so the sphere is as small as "a quarter of the pixels" allows - the share goes with the
# coverage - and level 4 keeps the facets' angle at 2.5 degrees.  A cut sample is at depth 32 with 29 roulette steps behind it:
# it carries 0.95^-29 = 4.4 times a sample's weight, so the image mean lacks 4.4 times the share.  test_smooth_host.py checks
# the condition on 16 384 samples.
BLACK_FURNACE_DEPTH = 32


def _with_sphere(s, cam, width, height, level):
    """adds the sphere on the view axis; (scene, table, indices of its triangles)"""
    o, fwd, _, _ = SS.view_axes(cam, width, height)
    n_box = len(s)
    _, verts, normal, cn = ptmi_scenes.icosphere(o + SPHERE_DISTANCE * fwd, SPHERE_RADIUS, level)
    for v, n in zip(verts, normal):
        s.tri(v[0], v[1], v[2], normal=n)
    arrays = s.arrays()
    assert np.array_equal(arrays[1][n_box:, :3], verts[:, :3])          # float32 in, float32 out: shared corners stay bit-equal
    table = np.repeat(arrays[2][:, None, :], 4, axis=1).astype(F)
    table[n_box:] = cn
    return s, table, list(range(n_box, len(s)))


def white_sphere(cam=None, width=128, height=128, level=SPHERE_LEVEL, quads=False):
    """furnace.box around an icosphere, every primitive with the furnace's RHO and LE: every pixel expects furnace.expected(depth)"""
    cam = ptmi.default_camera() if cam is None else cam
    s = FN.Scene()
    FN.box(s, quads=quads)
    return _with_sphere(s, cam, width, height, level)


def black_sphere(kind, cam=None, width=128, height=128, level=SPHERE_LEVEL, le=FN.LE):
    """furnace.box with rho = 0 and Le = le around an icosphere of `kind` (mirror or glass) with tint 1 that emits nothing: every
    path ends on a wall with throughput 1, so every pixel expects le.  (scene, table, kind array)"""
    cam = ptmi.default_camera() if cam is None else cam
    s = FN.Scene(rho=SS.BLACK, le=le)
    FN.box(s)
    s, table, sphere = _with_sphere(s, cam, width, height, level)
    kinds = np.zeros(len(s), np.int32)
    for k in sphere:
        s.b[k] = SS.WHITE; s.e[k] = SS.BLACK
        kinds[k] = kind
    return s, table, kinds
