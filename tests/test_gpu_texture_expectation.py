"""The albedo texture on the GPU against analytic values (tests/furnace.py), independent of the restatement, so that a contract that
is itself wrong - a lookup on the wrong texel, a flipped or swapped axis, the texture applied twice or not at all - shows too.

Compensated furnace: every primitive of a closed box has all its UVs at the centre of its OWN texel, of value T_i, and Kd_i = RHO /
T_i, so every vertex's effective albedo is RHO to an ulp and every pixel expects furnace.expected(depth), for both estimators and
both filters.  The texels take eight levels 0.7 * (1 / 0.7)^(l / 7), a ratio of 1.052 from one to the next, laid out as l = (i + 2
j) mod 8 on an 8 x 8 image: a texel's level differs from that of its eight neighbours (across the seams too), of its mirror images
in u and in v and of its transpose (asserted below), so a lookup that lands on any of those changes that primitive's albedo by at
least 5 %, ten times FLOOR.

Spatial map: one wall of furnace.box carries a 4 x 4 checker through ptmi_scenes.box_uvs, nearest filter, at max_depth = 2, where
a pixel whose whole footprint lies inside one texel has the closed-form value Le + (Kd * T) * Le.

Sizes, depths and the z-test are test_gpu_nee_expectation.py's."""
import numpy as np
import pytest

import furnace as FN
import ptmi
import ptmi_scenes
from test_gpu_nee_expectation import BLOCK, DEPTHS, FLOOR, H, W, Z_MAX, check, render

pytestmark = pytest.mark.gpu

F = np.float32
SIDE = 8                                                       # the compensated furnace's image: 8 x 8 texels, 8 levels
LEVELS = (0.7 * (1.0 / 0.7) ** (np.arange(8) / 7.0)).astype(F)


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    r.set_camera(ptmi.default_camera())
    yield r
    r.close()


def level_map():
    j, i = np.mgrid[0:SIDE, 0:SIDE]
    return (i + 2 * j) % 8


def tessellated_box(quads, cells=2, half=FN.HALF):
    """furnace.box with every wall cut into cells x cells: 24 quads or 48 triangles"""
    s = FN.Scene()
    g = half + 1.0
    edges = np.linspace(-g, g, cells + 1)
    for a in range(3):
        u, w = (a + 1) % 3, (a + 2) % 3
        for side in (-1.0, 1.0):
            for cu in range(cells):
                for cw in range(cells):
                    def p(du, dw):
                        x = np.zeros(3); x[a] = side * half; x[u] = edges[cu + du]; x[w] = edges[cw + dw]
                        return x
                    if quads:
                        s.quad(p(0, 0), p(1, 0), p(1, 1), p(0, 1))
                    else:
                        s.tri(p(0, 0), p(1, 0), p(1, 1)); s.tri(p(0, 0), p(1, 1), p(0, 1))
    return s


def assert_the_levels_tell_wrong_texels_apart():
    lv = level_map()
    assert LEVELS.min() >= F(0.7) and LEVELS.max() <= 1 and (LEVELS[1:] / LEVELS[:-1]).min() >= 1.05
    for j in range(SIDE):
        for i in range(SIDE):
            for dj in (-1, 0, 1):
                for di in (-1, 0, 1):
                    if dj or di:
                        assert lv[(j + dj) % SIDE, (i + di) % SIDE] != lv[j, i]
            assert lv[j, SIDE - 1 - i] != lv[j, i] and lv[SIDE - 1 - j, i] != lv[j, i]
            if i != j:
                assert lv[i, j] != lv[j, i]


@pytest.mark.parametrize("quads", [False, True])
def test_compensated_furnace(R, quads):
    assert_the_levels_tell_wrong_texels_apart()
    s = tessellated_box(quads)
    n = len(s)
    assert n >= 24 and n <= SIDE * SIDE
    image = np.repeat(LEVELS[level_map()][:, :, None], 3, axis=2).astype(F)
    uv = np.zeros((n, 4, 2), F)
    for k in range(n):
        i, j = k % SIDE, k // SIDE
        uv[k] = ((i + 0.5) / SIDE, (j + 0.5) / SIDE)          # exact in binary32: x = s * 8 - 0.5 = i, fx = 0
        s.b[k] = tuple(np.asarray(FN.RHO, F) / image[j, i])
    arrays = s.arrays()
    assert arrays[3].max() <= 1.0
    eff = arrays[3] * np.array([image[k // SIDE, k % SIDE] for k in range(n)], F)
    assert np.abs(eff / np.asarray(FN.RHO, F) - 1).max() <= 2.0 ** -23
    R.load_scene_arrays(*arrays)
    R.set_camera(ptmi.default_camera())
    for filt in ("nearest", "bilinear"):
        for depth in DEPTHS:
            value = FN.expected(depth)
            for nee in (False, True):
                R.set_config(sampling_mode=0, integrator=0, fast_tree=False)
                R.set_albedo_texture(image, uv, None, filt)
                assert R.albedo_texture_info()["n_textured"] == n
                check(f"{'quads' if quads else 'tris'} {filt} depth {depth} {'NEE' if nee else 'reference'}", render(R, depth, nee) - value, value)
    # and the compensation is needed: without the texture the same scene misses the value by far more than the test allows
    R.set_albedo_texture(None, None)
    value = FN.expected(5)
    off = render(R, 5, True, spp=64).reshape(-1, 3).mean(0) / value - 1.0
    assert (np.abs(off) > 10 * FLOOR).all(), off


def footprint_texels(frame, w, h, wall_z, scale, origin, cells):
    """Per pixel (row 0 = bottom, as read_image): the checker texel (j, i) its whole footprint lies in, or (-1, -1).  The
    footprint is the pixel widened by one pixel on every side; its four corner rays are cut with the wall's plane z = wall_z, in
    binary64, and all four must fall in the same texel, at least 1e-3 of a texel away from its edges (a convex texel holds the
    whole image of the footprint when it holds the corners').  frame: the 12 floats of ptmi_get_camera_frame."""
    o, llc, hor, ver = (np.asarray(frame[3 * k:3 * k + 3], np.float64) for k in range(4))
    out = np.full((h, w, 2), -1, int)
    for y in range(h):
        for x in range(w):
            cell = None
            for cx, cy in ((x - 1, y - 1), (x + 2, y - 1), (x - 1, y + 2), (x + 2, y + 2)):
                d = llc + (cx / w) * hor + (cy / h) * ver - o
                if d[2] * (wall_z - o[2]) <= 0:
                    cell = None; break
                p = o + ((wall_z - o[2]) / d[2]) * d
                if np.abs(p[:2]).max() > FN.HALF - 0.5:       # off the wall's visible part
                    cell = None; break
                t = ((p[:2] - np.asarray(origin[:2], np.float64)) / scale) % 1.0 * cells
                if (np.abs(t - np.round(t)) < 1e-3).any():
                    cell = None; break
                c = (int(t[1]), int(t[0]))
                if cell is not None and c != cell:
                    cell = None; break
                cell = c
            if cell is not None:
                out[y, x] = cell
    return out


def check_pixels(tag, ratio, where):
    """test_gpu_nee_expectation.check on the chosen pixels only: ratio (h, w, 3) = estimate / expected - 1 against 0 with value 1.
    The image mean and SE over the chosen pixels, and per 16 x 16 block over the block's chosen pixels where it has at least 64."""
    px = ratio[where]
    floor = 2e-5
    mean = px.mean(0); se = px.std(0, ddof=1) / np.sqrt(len(px))
    z = np.abs(mean) / np.maximum(se, floor)
    bz = 0.0
    for by in range(0, H, BLOCK):
        for bx in range(0, W, BLOCK):
            m = where[by:by + BLOCK, bx:bx + BLOCK]
            if m.sum() >= 64:
                b = ratio[by:by + BLOCK, bx:bx + BLOCK][m]
                bse = b.std(0, ddof=1) / np.sqrt(len(b))
                bz = max(bz, float((np.abs(b.mean(0)) / np.maximum(bse, floor)).max()))
    print(f"{tag}: {len(px)} pixels, mean ratio - 1 {np.array2string(mean, precision=6)}, SE {np.array2string(se, precision=6)}, "
          f"z {np.array2string(z, precision=2)}, block |z| max {bz:.2f}")
    assert (Z_MAX * se <= FLOOR).all(), (tag, "too noisy to see a bias of 0.5 %", se)
    assert (z < Z_MAX).all(), (tag, mean, se, z)
    assert bz < Z_MAX, (tag, bz)


def test_spatial_map_at_depth_2(R):
    s = FN.Scene()
    FN.box(s)
    arrays = s.arrays()
    prims = dict(type=arrays[0], verts=arrays[1], normal=arrays[2])
    wall = np.flatnonzero((arrays[1][:, :3, 2] == -FN.HALF).all(1))         # the wall the default camera faces: z = -HALF
    assert len(wall) == 2 and (np.abs(arrays[2][wall, 2]) > 0.99).all()
    cells, texel_units = 4, 10.0
    scale, origin = cells * texel_units, (-16.2, -13.7, 0.0)
    a, b = np.array((1.0, 0.9, 0.8), F), np.array((0.5, 0.6, 0.7), F)
    image = ptmi_scenes.checker(cells, a, b)
    uv = ptmi_scenes.box_uvs(prims, scale=scale, origin=origin)
    textured = np.zeros(len(arrays[0]), bool); textured[wall] = True
    R.load_scene_arrays(*arrays)
    R.set_camera(ptmi.default_camera())
    R.update_resolution(W, H)
    R.set_config(spp=4, max_depth=2, sampling_mode=0, integrator=0, fast_tree=False, next_event=False)
    R.set_albedo_texture(image, uv, textured, "nearest")
    cell = footprint_texels(R.camera_frame(), W, H, -FN.HALF, scale, origin, cells)
    chosen = cell[..., 0] >= 0
    assert chosen.sum() >= W * H // 4
    colour = (cell[..., 0] + cell[..., 1]) % 2                 # checker: a where i + j is even
    for c in (0, 1):
        assert len({tuple(t) for t in cell[chosen & (colour == c)]}) >= 4, c
    le, kd = np.asarray(FN.LE, F), np.asarray(FN.RHO, F)
    T = np.where((colour == 0)[..., None], a, b).astype(F)
    expect = (le + ((kd * T).astype(F) * le).astype(F)).astype(F)           # Le + (Kd * T) * Le, as the kernel rounds it
    # the reference's estimator: every sample of such a pixel IS that value; spp additions of equal values, one rounding each
    R.render_frame()
    rad = R.read_image(rgb8=False)[1]
    rel = np.abs(rad.astype(np.float64) / expect.astype(np.float64) - 1.0)[chosen]
    print(f"spatial map, reference: {chosen.sum()} pixels of {W * H}, largest relative error {rel.max():.3e} (bound {4 * 2.0 ** -24:.3e})")
    assert rel.max() <= 4 * 2.0 ** -24
    assert len(np.unique(rad[chosen].view(np.uint32), axis=0)) >= 2                 # both colours are there
    # next-event estimation: the same pixels, each to its own expected value
    nee = render(R, 2, True)
    check_pixels("spatial map, NEE", nee / expect.astype(np.float64) - 1.0, chosen)
