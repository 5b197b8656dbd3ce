"""Scenes and cases the vertex-normal tests share (test_smooth_host.py on the CPU, test_gpu_smooth.py on the device): a small mesh
with every kind of primitive the contract of include/ptmi.h ("vertex normals") tells apart, and (primitive, point) cases on it."""
import numpy as np

import furnace as FN

F = np.float32
# names of the mesh's primitives, in load order (quads=False drops the quads)
TRI, QUAD, SLIVER, CANCEL, ZEROS, HUGE, FLAT_TRI, FLAT_QUAD, FLAT_4TH, WARPED = (
    "tri", "quad", "sliver", "cancel", "zeros", "huge", "flat_tri", "flat_quad", "flat_4th", "warped")


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def mesh(quads=True):
    """(arrays, table, index): arrays for load_scene_arrays, the corner-normal table (n, 4, 3) and name -> load-order index"""
    s = FN.Scene(rho=(0.5, 0.5, 0.5), le=(0.0, 0.0, 0.0))
    table, index = [], {}

    def add(name, corners):
        index[name] = len(s) - 1
        c = np.zeros((4, 3), F)
        c[:len(corners)] = corners
        table.append(c)
    s.tri((0.25, 0.5, -1.0), (2.5, 0.75, -1.5), (0.75, 2.25, -0.5))
    add(TRI, [_unit((-0.4, -0.3, 1.0)), _unit((0.6, -0.1, 0.8)), _unit((0.1, 0.7, 0.9))])
    if quads:
        s.quad((3.0, 0.0, 0.0), (5.0, 0.5, 0.25), (5.5, 2.5, 0.75), (3.5, 2.0, 0.5))           # a parallelogram
        add(QUAD, [_unit((-0.5, -0.5, 1.0)), _unit((0.5, -0.5, 1.0)), _unit((0.5, 0.5, 1.0)), _unit((-0.5, 0.5, 1.0))])
    s.tri((0.0, 4.0, 0.0), (1.0, 4.0, 0.0), (3.0, 4.0, 0.0), normal=(0.0, 0.0, 1.0))         # zero area: den = 0
    add(SLIVER, [_unit((1.0, 0.0, 1.0)), _unit((0.0, 1.0, 1.0)), _unit((-1.0, 0.0, 1.0))])
    s.tri((0.0, 6.0, 0.0), (2.0, 6.0, 0.0), (0.0, 8.0, 0.0))                                 # n0 + n1 = 0 on the middle of edge 0 - 1
    add(CANCEL, [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0)])
    s.tri((4.0, 6.0, 0.0), (6.0, 6.0, 0.0), (4.0, 8.0, 0.0))                                 # zero-length corner normals are allowed
    add(ZEROS, [(0.0, 0.0, 0.0)] * 3)
    s.tri((9.0e17, 0.0, 0.0), (9.0e17, 9.0e17, 0.0), (0.0, 9.0e17, 0.0), normal=(0.0, 0.0, -1.0))   # den overflows (a scene load takes edges below 1e18)
    add(HUGE, [_unit((1.0, 0.0, 1.0)), _unit((0.0, 1.0, 1.0)), _unit((-1.0, 0.0, 1.0))])
    s.tri((8.0, 0.0, 0.0), (9.0, 0.0, 0.0), (8.0, 1.0, 0.0))
    add(FLAT_TRI, [(0.0, 0.0, 1.0)] * 3)
    if quads:
        s.quad((8.0, 2.0, 0.0), (9.0, 2.0, 0.0), (9.0, 3.0, 0.0), (8.0, 3.0, 0.0))
        add(FLAT_QUAD, [(-0.0, 0.0, 1.0), (0.0, -0.0, 1.0), (-0.0, -0.0, 1.0), (0.0, 0.0, 1.0)])   # -0.0 == 0.0: flat
    s.tri((8.0, 4.0, 0.0), (9.0, 4.0, 0.0), (8.0, 5.0, 0.0))
    add(FLAT_4TH, [(0.0, 0.0, 1.0), (0.0, 0.0, 1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)])      # a triangle's 4th entry is not read
    if quads:
        s.quad((11.0, 0.0, 0.0), (13.0, 0.0, 0.5), (13.0, 2.0, -0.5), (11.0, 2.0, 0.75))          # not planar
        add(WARPED, [_unit((-0.3, -0.3, 1.0)), _unit((0.3, -0.3, 1.0)), _unit((0.3, 0.3, 1.0)), _unit((-0.3, 0.3, 1.0))])
    return s.arrays(), np.array(table, F), index


def smooth_names(quads=True):
    return [TRI, SLIVER, CANCEL, ZEROS, HUGE] + ([QUAD, WARPED] if quads else [])


def cases(arrays, index, seed=5, n_random=64):
    """(prim (n,), p (n, 3)) float32 cases on every primitive of the mesh: corners, edge midpoints, the centroid, a quad's
    diagonal, points off the primitive (in its plane and off it) and random combinations of the corners, some far outside"""
    types, verts = arrays[0], arrays[1].astype(np.float64)
    rng = np.random.default_rng(seed)
    prim, pts = [], []
    for name, k in index.items():
        m = 4 if types[k] == 1 else 3
        v = verts[k, :m]
        local = [v[i] for i in range(m)] + [0.5 * (v[i] + v[(i + 1) % m]) for i in range(m)] + [v.mean(0)]
        if m == 4:
            local += [0.5 * (v[0] + v[2]), 0.25 * v[0] + 0.75 * v[2], (v[0] + v[1] + v[2]) / 3.0, (v[0] + v[2] + v[3]) / 3.0]
        local += [v[0] - 0.5 * (v[1] - v[0]), v[1] + 2.0 * (v[1] - v[0]) + (v[m - 1] - v[0]), v.mean(0) + (0.0, 0.0, 0.5), 3.0 * v[m - 1] - 2.0 * v.mean(0)]
        w = rng.uniform(-0.5, 1.5, (n_random, m))
        local += list((w / w.sum(1, keepdims=True)) @ v)
        prim += [k] * len(local); pts += local
    with np.errstate(all="ignore"):
        return np.array(prim, np.int32), np.array(pts, np.float64).astype(F)
