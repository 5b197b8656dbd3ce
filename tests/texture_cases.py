"""Scenes, images and cases the albedo-texture tests share (test_texture_host.py on the CPU, test_gpu_texture.py on the device):
the vertex-normal tests' mesh of edge-case primitives (tests/smooth_cases.py) with a UV table on it, the 5 x 3 random image, random
UV tables, and the Cornell box's named parts."""
import os

import numpy as np

import ptmi
import ptmi_scenes
import smooth_cases as SC
from oracle_binding import SCENES

F = np.float32
CBOX = os.path.join(SCENES, "cbox.obj")
CBOX_QUADS = os.path.join(SCENES, "cbox_quads.obj")
# what the mesh's UV table does with SC.mesh's primitives
UNTEXTURED = SC.FLAT_TRI                                       # masked out; its UVs are NaN
EDGE_UVS = SC.CANCEL                                           # corners at -65536, 65536 and 0
NEGATIVE = SC.ZEROS                                            # every UV negative


def image(seed=3, width=5, height=3):
    """random texels in [0.05, 1): odd and not square, so that an axis mix-up shows"""
    return np.random.default_rng(seed).uniform(0.05, 1.0, (height, width, 3)).astype(F)


def random_uvs(n, seed=4):
    """(n, 4, 2) UVs in [-2, 3]"""
    return np.random.default_rng(seed).uniform(-2.0, 3.0, (n, 4, 2)).astype(F)


def mesh(quads=True):
    """(arrays, uv, textured, index): SC.mesh's primitives - a triangle, a parallelogram, a zero-area sliver, a triangle whose
    den overflows, a quad that is not planar, ... - with random UVs, UVs at the limits on one, negative UVs on another and one
    primitive untextured, whose UVs are NaN"""
    arrays, _, index = SC.mesh(quads)
    n = len(arrays[0])
    uv = random_uvs(n, 9)
    uv[index[EDGE_UVS], :3] = [(-65536.0, 65536.0), (65536.0, -65536.0), (0.0, 0.0)]
    uv[index[NEGATIVE]] = -np.abs(uv[index[NEGATIVE]]) - F(0.125)
    uv[index[SC.FLAT_4TH], 3] = np.nan                         # a triangle's 4th UV is ignored
    textured = np.ones(n, bool)
    textured[index[UNTEXTURED]] = False
    uv[index[UNTEXTURED]] = np.nan
    return arrays, uv, textured, index


def cases(arrays, index):
    """SC.cases: corners, edge midpoints, centroids, a quad's diagonal, points off the primitives and random combinations"""
    return SC.cases(arrays, index)


_PARTS = {}


def cornell(which):
    """(arrays, parts) of cbox / cbox_quads / cbox_sub (cbox subdivided twice): parts has the load-order indices of the short
    and the tall block, of the emitters and of the floor (the non-emitting primitives whose stored normal points up and whose
    corners all lie at the scene's lowest y)"""
    if which not in _PARTS:
        hs = ptmi.HostScene.load(CBOX_QUADS if which == "cbox_quads" else CBOX, 2 if which == "cbox_sub" else 0)
        p = hs.prims()
        arrays = (p["type"], p["verts"], p["normal"], p["bsdf"], p["Le"])
        parts = {}
        blocks = ptmi_scenes.cornell_blocks(p, 1, 2)
        parts["short"], parts["tall"] = np.flatnonzero(blocks == 1), np.flatnonzero(blocks == 2)
        parts["emitters"] = np.flatnonzero(p["Le"].max(1) > 0)
        read = np.where(p["type"] == 1, 4, 3)
        y = np.array([p["verts"][i, :read[i], 1].max() for i in range(len(read))])
        parts["floor"] = np.flatnonzero((p["normal"][:, 1] > 0.99) & (y < p["verts"][:, :3, 1].min() + 0.05) & (p["Le"].max(1) == 0))
        _PARTS[which] = (arrays, parts)
    return _PARTS[which]


def as_prims(arrays):
    return dict(type=arrays[0], verts=arrays[1], normal=arrays[2], bsdf=arrays[3], Le=arrays[4])
