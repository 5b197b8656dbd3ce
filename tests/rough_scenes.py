"""Scenes of the rough-metal tests (include/ptmi.h: "rough metal") with their kind and roughness arrays - no GPU needed to build
them."""
import numpy as np

import env_scenes as ES
import furnace as FN
import ptmi_scenes
import specular_scenes as SS

F = np.float32
MIRROR, GLASS, ROUGH = 1, 2, 3
BLACK, WHITE = SS.BLACK, SS.WHITE


def blocks(prims):
    """the Cornell box's short block glass, its tall block rough metal"""
    return ptmi_scenes.cornell_blocks(prims, short=GLASS, tall=ROUGH)


def soup_table(n, seed=21):
    """a fifth of a soup each mirror, glass and rough metal (emitters among them), and a roughness per primitive over the range"""
    kind = np.zeros(n, np.int32)
    kind[::5] = MIRROR; kind[2::5] = GLASS; kind[1::5] = ROUGH
    rough = np.random.default_rng(seed).uniform(0.05, 1.0, n).astype(F)
    return kind, rough


def rough_furnace(quads=False, chain=False, zero_normals=0, scale_normals=False):
    """specular_scenes.black_furnace with scattering walls, its four panels (stored normals 19 degrees off their planes) turned to
    rough metal and its glass cuboid kept.  scale_normals: two panels' stored normals get lengths 5 and 0.25; zero_normals: that
    many panel primitives get a zero stored normal."""
    s, kind = SS.black_furnace(quads=quads, chain=chain)
    n_box = 6 if quads else 12
    s.b[:n_box] = [(0.6, 0.5, 0.4)] * n_box
    kind = kind.copy()
    panels = np.flatnonzero(kind == MIRROR)
    kind[panels] = ROUGH
    if scale_normals:
        for k, f in ((panels[0], 5.0), (panels[-1], 0.25)):
            s.n[k] = tuple(f * np.asarray(s.n[k]))
    arrays = list(s.arrays())
    if zero_normals:
        arrays[2][panels[:zero_normals]] = 0.0
    return tuple(arrays), kind


def skimming_quad(cam, width, height, angle=1e-4):
    """a rough quad that the view axis meets at `angle` radians, ten units ahead, under an emitter that catches what it reflects:
    the rows below the image centre meet it less flatly, the rows above pass over it"""
    o, fwd, right, up = SS.view_axes(cam, width, height)
    s = FN.Scene(rho=BLACK, le=BLACK)
    along = np.cos(angle) * fwd + np.sin(angle) * up             # rises towards the far end: the axis descends onto it
    base = o - (10.0 * np.sin(angle)) * up                       # the axis reaches the plane after about ten units
    s.quad(base - 50 * right, base + 50 * right, base + 50 * right + 100 * along, base - 50 * right + 100 * along)
    s.b[0] = (0.9, 0.8, 0.7)
    e = o + 60.0 * fwd
    s.quad(e - 200 * right - 200 * up, e + 200 * right - 200 * up, e + 200 * right + 200 * up, e - 200 * right + 200 * up, le=(2.0, 1.5, 1.0))
    return s, np.array([ROUGH, 0], np.int32)


def ground(tint=WHITE):
    """env_scenes.ground_quad as rough metal: (scene, kind)"""
    return ES.ground_quad(tint), np.array([ROUGH], np.int32)


def panel_and_emitter(cam, width, height, tint, le):
    """specular_scenes.mirror_and_emitter with the mirror made rough metal"""
    s, kind = SS.mirror_and_emitter(cam, width, height, tint, le)
    kind = kind.copy(); kind[kind == MIRROR] = ROUGH
    return s, kind
