"""Host half of the vertex normals (include/ptmi.h, "vertex normals"): the restatement (tests/smooth_oracle.py) against binary64
at corners, edges and centroids, its clamps and fallbacks, ptmi_check_vertex_normals, the flat / smooth classification, and
ptmi_scenes' icosphere, smooth_normals and cornell_spheres.  No GPU."""
import os

import numpy as np
import pytest

import path_oracle as PO
import ptmi
import ptmi_scenes
import smooth_cases as SC
import smooth_oracle as SM
import smooth_scenes as SS
from oracle_binding import OracleScene, SCENES, default_camera

F = np.float32
CBOX = os.path.join(SCENES, "cbox.obj")
CBOX_QUADS = os.path.join(SCENES, "cbox_quads.obj")
TOL = 1e-6


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def unit64(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def as_prims(arrays):
    return dict(type=arrays[0], verts=arrays[1], normal=arrays[2], bsdf=arrays[3], Le=arrays[4])


@pytest.fixture(scope="module")
def mesh():
    arrays, table, index = SC.mesh()
    return as_prims(arrays), table, index


def normal_at(mesh, name, p):
    prims, table, index = mesh
    return SM.vertex_normal(prims, table, index[name], np.asarray(p, np.float64).astype(F))


# ------------------------------------------------------------------------------------------------
# the restatement against binary64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,corner_ids", [(SC.TRI, (0, 1, 2)), (SC.QUAD, (0, 1, 2)), (SC.QUAD, (0, 2, 3))])
def test_corner_edge_centroid(mesh, name, corner_ids):
    prims, table, index = mesh
    k = index[name]
    v = prims["verts"][k].astype(np.float64); c = table[k].astype(np.float64)
    ids = list(corner_ids)
    for i in ids:                                            # a corner: unit(n_i)
        n, smooth = normal_at(mesh, name, v[i])
        assert smooth and np.abs(n - unit64(c[i])).max() < TOL, (i, n)
    for a, b in ((ids[0], ids[1]), (ids[1], ids[2]), (ids[2], ids[0])):      # an edge's middle: unit(n_a + n_b)
        n, smooth = normal_at(mesh, name, 0.5 * (v[a] + v[b]))
        assert smooth and np.abs(n - unit64(c[a] + c[b])).max() < TOL, (a, b, n)
    n, smooth = normal_at(mesh, name, (v[ids[0]] + v[ids[1]] + v[ids[2]]) / 3.0)   # the centroid: unit(n0 + n1 + n2)
    assert smooth and np.abs(n - unit64(c[ids[0]] + c[ids[1]] + c[ids[2]])).max() < TOL
    assert abs(float(np.linalg.norm(n.astype(np.float64))) - 1.0) < TOL


def test_points_outside_clamp_onto_the_primitive(mesh):
    prims, table, index = mesh
    v = prims["verts"][index[SC.TRI]].astype(np.float64); c = table[index[SC.TRI]].astype(np.float64)
    e1, e2 = v[1] - v[0], v[2] - v[0]
    n, _ = normal_at(mesh, SC.TRI, v[0] - 2.0 * e1 - 3.0 * e2)          # r1 < 0, r2 < 0: corner 0
    assert np.abs(n - unit64(c[0])).max() < TOL
    n, _ = normal_at(mesh, SC.TRI, v[0] + 4.0 * e1 + 0.5 * e2)          # r1 > 1: b1 = 1, m = 0: corner 1
    assert np.abs(n - unit64(c[1])).max() < TOL
    n, _ = normal_at(mesh, SC.TRI, v[0] + 0.25 * e1 + 5.0 * e2)         # r2 > m: b2 = m = 0.75, b0 = 0
    assert np.abs(n - unit64(0.25 * c[1] + 0.75 * c[2])).max() < TOL
    n, _ = normal_at(mesh, SC.TRI, v[0] + 0.25 * e1 + 0.25 * e2 + 3.0 * np.cross(e1, e2))   # off the plane: its foot
    assert np.abs(n - unit64(0.5 * c[0] + 0.25 * c[1] + 0.25 * c[2])).max() < TOL


def test_quad_halves_and_diagonal(mesh):
    prims, table, index = mesh
    k = index[SC.QUAD]
    v = prims["verts"][k].astype(np.float64); c = table[k].astype(np.float64)
    e1, e2, e3 = v[1] - v[0], v[2] - v[0], v[3] - v[0]
    n, s = normal_at(mesh, SC.QUAD, v[0] + 0.5 * e1 + 0.25 * e2)        # the first half (v00, v10, v11)
    assert s and np.abs(n - unit64(0.25 * c[0] + 0.5 * c[1] + 0.25 * c[2])).max() < TOL
    n, s = normal_at(mesh, SC.QUAD, v[0] + 0.25 * e2 + 0.5 * e3)        # the second half (v00, v11, v01)
    assert s and np.abs(n - unit64(0.25 * c[0] + 0.25 * c[2] + 0.5 * c[3])).max() < TOL
    for f in (0.0, 0.125, 0.5, 0.875, 1.0):                            # the diagonal: both halves agree up to rounding
        n, s = normal_at(mesh, SC.QUAD, v[0] + f * e2)
        assert s and np.abs(n - unit64((1.0 - f) * c[0] + f * c[2])).max() < TOL
    n, s = normal_at(mesh, SC.WARPED, prims["verts"][index[SC.WARPED]][3])     # a quad that is not planar: corner v01
    assert s and np.abs(n - unit64(table[index[SC.WARPED]][3])).max() < TOL


def test_fallbacks_take_the_stored_normal(mesh):
    prims, table, index = mesh
    for name, p in ((SC.SLIVER, (1.5, 4.0, 0.0)),             # zero area: den = 0
                    (SC.CANCEL, (1.0, 6.0, 0.0)),             # n0 + n1 = 0 on the middle of edge 0 - 1
                    (SC.ZEROS, (4.5, 6.5, 0.0)),              # all corner normals zero
                    (SC.HUGE, (4.5e17, 4.5e17, 0.0)),         # den overflows
                    (SC.TRI, (np.nan, 0.0, 0.0)),             # a NaN point: the clamps keep it a NaN, len2 is no number
                    (SC.FLAT_TRI, (8.25, 0.25, 0.0)), (SC.FLAT_QUAD, (8.5, 2.5, 0.0)), (SC.FLAT_4TH, (8.25, 4.25, 0.0))):
        n, smooth = normal_at(mesh, name, p)
        assert not smooth and np.array_equal(bits(n), bits(prims["normal"][index[name]])), name
    n, smooth = normal_at(mesh, SC.CANCEL, (0.5, 6.5, 0.0))   # elsewhere on that triangle the sum has a direction
    assert smooth
    huge = dict(type=np.zeros(1, np.int32), normal=np.array([[0.0, 0.0, -1.0]], F),       # coordinates of 1e18
                verts=np.array([[(1.0e18, 0.0, 0.0), (1.0e18, 1.0e18, 0.0), (0.0, 1.0e18, 0.0), (0.0, 0.0, 0.0)]], F))
    n, smooth = SM.vertex_normal(huge, table[index[SC.HUGE]][None], 0, np.array((5.0e17, 5.0e17, 0.0), F))
    assert not smooth and np.array_equal(bits(n), bits(huge["normal"][0]))


# ------------------------------------------------------------------------------------------------
# the check and the classification
# ------------------------------------------------------------------------------------------------
def test_check_vertex_normals_rejects():
    good = np.zeros((3, 4, 3), F); good[..., 2] = 1.0
    ptmi.check_vertex_normals(good)
    zero = good.copy(); zero[1] = 0.0
    ptmi.check_vertex_normals(zero)                           # zero-length corner normals are allowed
    fourth = good.copy(); fourth[0, 3, 0] = np.nan
    ptmi.check_vertex_normals(fourth)                         # the 4th corner is not read without a type
    L = ptmi.lib()
    assert L.ptmi_check_vertex_normals(0, good.ctypes.data) != 0 and b"n_prims" in L.ptmi_last_error()
    assert L.ptmi_check_vertex_normals(-1, good.ctypes.data) != 0
    assert L.ptmi_check_vertex_normals(3, None) != 0 and b"NULL" in L.ptmi_last_error()
    for bad in (np.nan, np.inf, -np.inf):
        for corner in range(3):
            for comp in range(3):
                t = good.copy(); t[2, corner, comp] = bad
                with pytest.raises(ptmi.PtmiError, match="vertex normals: corner %d of primitive 2" % corner):
                    ptmi.check_vertex_normals(t)
    with pytest.raises(ValueError):
        ptmi.check_vertex_normals(np.zeros((3, 3, 3), F))
    # with the types (what ptmi_set_vertex_normals checks): a quad's 4th corner is read, a triangle's is not
    stored = good[:, 0].copy()
    assert not ptmi.classify_vertex_normals([0, 0, 0], stored, fourth).any()
    with pytest.raises(ptmi.PtmiError, match="corner 3 of primitive 0"):
        ptmi.classify_vertex_normals([1, 0, 0], stored, fourth)


def test_flat_smooth_classification(mesh):
    prims, table, index = mesh
    got = ptmi.classify_vertex_normals(prims["type"], prims["normal"], table)
    expect = np.zeros(len(table), bool)
    expect[[index[n] for n in SC.smooth_names()]] = True
    assert np.array_equal(got, expect) and np.array_equal(SM.classify(prims, table), expect)
    stored = np.array([[0.0, 0.0, 1.0]], F)
    flat = np.array([[[-0.0, 0.0, 1.0], [0.0, -0.0, 1.0], [0.0, 0.0, 1.0], [5.0, 5.0, 5.0]]], F)
    assert not ptmi.classify_vertex_normals([0], stored, flat)[0]              # -0.0 == 0.0; the 4th is ignored
    assert ptmi.classify_vertex_normals([1], stored, flat)[0]                  # a quad reads it
    off = flat.copy(); off[0, 2, 2] = np.nextafter(F(1.0), F(2.0))
    assert ptmi.classify_vertex_normals([0], stored, off)[0]                   # one ulp is smooth


# ------------------------------------------------------------------------------------------------
# ptmi_scenes
# ------------------------------------------------------------------------------------------------
def facet_theta_max(corner_normals):
    """the largest angle between two corner normals of one facet"""
    c = corner_normals[:, :3].astype(np.float64)
    c /= np.linalg.norm(c, axis=2, keepdims=True)
    cos = np.stack([np.einsum("ij,ij->i", c[:, a], c[:, b]) for a, b in ((0, 1), (1, 2), (2, 0))])
    return float(np.arccos(np.clip(cos, -1.0, 1.0)).max())


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_icosphere(level):
    center, radius = (0.5, -1.25, 2.0), 1.75
    types, verts, normal, cn = ptmi_scenes.icosphere(center, radius, level)
    n = 20 * 4 ** level
    assert types.shape == (n,) and not types.any() and verts.shape == (n, 4, 3) and normal.shape == (n, 3) and cn.shape == (n, 4, 3)
    assert verts.dtype == F and normal.dtype == F and cn.dtype == F
    corners = verts[:, :3].reshape(-1, 3)
    distinct = {c.tobytes() for c in corners}
    assert len(distinct) == 10 * 4 ** level + 2                # Euler: V = F / 2 + 2, so shared corners are bit-equal
    out = corners.astype(np.float64) - center
    assert np.abs(np.linalg.norm(out, axis=1) - radius).max() < 1e-6 * radius * 4
    assert np.abs(cn[:, :3].reshape(-1, 3) - out / np.linalg.norm(out, axis=1, keepdims=True)).max() < TOL
    assert np.abs(np.linalg.norm(cn[:, :3].astype(np.float64), axis=2) - 1.0).max() < TOL
    by_corner = {}
    for c, m in zip(corners, cn[:, :3].reshape(-1, 3)):        # one normal per shared corner
        assert by_corner.setdefault(c.tobytes(), m.tobytes()) == m.tobytes()
    v = verts.astype(np.float64)
    g = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]); g /= np.linalg.norm(g, axis=1, keepdims=True)
    assert np.abs(normal - g).max() < TOL and (np.einsum("ij,ij->i", g, v[:, 0] - center) > 0).all()   # outward geometric
    assert SM.classify(dict(type=types, normal=normal), cn).all()


def test_icosphere_interpolated_normal_is_near_the_radial_one():
    center, radius = np.array([0.5, 1.0, -2.0]), 1.5
    types, verts, normal, cn = ptmi_scenes.icosphere(center, radius, 2)
    theta_max = facet_theta_max(cn)
    prims = dict(type=types, verts=verts, normal=normal)
    rng = np.random.default_rng(3)
    k = rng.integers(0, len(types), 10_000)
    w = rng.dirichlet((1.0, 1.0, 1.0), len(k))
    p = np.einsum("ij,ijk->ik", w, verts[k, :3].astype(np.float64))
    worst = 0.0
    for i in range(len(k)):
        n, smooth = SM.vertex_normal(prims, cn, int(k[i]), p[i].astype(F))
        assert smooth
        worst = max(worst, float(np.arccos(np.clip(np.dot(n.astype(np.float64), unit64(p[i] - center)), -1.0, 1.0))))
    # both vectors lie in the facet's spherical triangle (the radial one because p lies in the facet, the interpolated one as a
    # positive combination of its corners), whose diameter is the largest angle between two of its corners
    assert worst <= theta_max + 1e-5, (worst, theta_max)
    assert worst > 0.0


@pytest.mark.parametrize("path,sub", [(CBOX, 0), (CBOX_QUADS, 0), (CBOX, 2)])
def test_smooth_normals_on_the_cornell_box_is_all_flat(path, sub):
    prims = ptmi.HostScene.load(path, sub).prims()
    table = ptmi_scenes.smooth_normals(prims)
    assert table.shape == (len(prims["type"]), 4, 3) and table.dtype == F
    assert not ptmi.classify_vertex_normals(prims["type"], prims["normal"], table).any()
    assert np.array_equal(bits(table), bits(np.repeat(prims["normal"][:, None, :], 4, axis=1)))


def test_smooth_normals_recovers_a_sphere():
    types, verts, normal, cn = ptmi_scenes.icosphere((0.0, 0.0, 0.0), 1.0, 2)
    prims = dict(type=types, verts=verts, normal=normal)
    table = ptmi_scenes.smooth_normals(prims)                 # the corner normals thrown away
    assert ptmi.classify_vertex_normals(types, normal, table).all()
    a = table[:, :3].astype(np.float64); b = cn[:, :3].astype(np.float64)
    ang = np.arccos(np.clip(np.einsum("ijk,ijk->ij", a, b) / np.linalg.norm(a, axis=2), -1.0, 1.0))
    assert ang.max() <= facet_theta_max(cn), (ang.max(), facet_theta_max(cn))
    sharp = ptmi_scenes.smooth_normals(prims, crease_deg=1.0)  # below the mesh's dihedral angles: nothing is joined
    assert not ptmi.classify_vertex_normals(types, normal, sharp).any()


@pytest.mark.parametrize("path,sub", [(CBOX, 0), (CBOX_QUADS, 0), (CBOX, 1)])
def test_cornell_spheres(path, sub):
    prims = ptmi.HostScene.load(path, sub).prims()
    kind = ptmi_scenes.cornell_blocks(prims)
    level = 1
    arrays, table, ranges = ptmi_scenes.cornell_spheres(prims, level=level)
    types, verts, normal, bsdf, le = arrays
    n_rest = int((kind == 0).sum()); n_s = 20 * 4 ** level
    assert len(types) == n_rest + 2 * n_s and table.shape == (len(types), 4, 3)
    assert ranges == dict(short=(n_rest, n_rest + n_s), tall=(n_rest + n_s, n_rest + 2 * n_s))
    assert np.array_equal(types[:n_rest], prims["type"][kind == 0]) and np.array_equal(bits(verts[:n_rest]), bits(prims["verts"][kind == 0]))
    smooth = ptmi.classify_vertex_normals(types, normal, table)
    assert not smooth[:n_rest].any() and smooth[n_rest:].all()
    ptmi.HostScene.from_arrays(*arrays)                       # loads
    floor = min(float(prims["verts"][i, :3, 1].min()) for i in np.flatnonzero(kind))
    spheres = []
    for name, block in (("short", 1), ("tall", 2)):
        a, b = ranges[name]
        c = verts[a:b, :3].reshape(-1, 3).astype(np.float64)
        bv = np.concatenate([prims["verts"][i, :4 if prims["type"][i] == 1 else 3] for i in np.flatnonzero(kind == block)]).astype(np.float64)
        lo, hi = bv.min(0), bv.max(0)
        r = 0.5 * min(hi[0] - lo[0], hi[2] - lo[2])
        center = np.array([0.5 * (lo[0] + hi[0]), lo[1] + r, 0.5 * (lo[2] + hi[2])])
        assert np.abs(np.linalg.norm(c - center, axis=1) - r).max() < 1e-5
        assert c[:, 1].min() >= lo[1] - 1e-5 and lo[1] - floor < 0.01     # it stands where its block stood, on the floor
        assert not le[a:b].any() and np.array_equal(bits(bsdf[a:b]), bits(np.repeat(prims["bsdf"][np.flatnonzero(kind == block)[:1]], n_s, 0)))
        spheres.append((center, r))
    (c0, r0), (c1, r1) = spheres
    assert np.linalg.norm(c0 - c1) > r0 + r1                  # the spheres do not touch
    rest = np.concatenate([verts[i, :4 if types[i] == 1 else 3] for i in range(n_rest)]).astype(np.float64)
    for c, r in spheres:                                      # nor do they reach out of the box
        assert c[0] - r > rest[:, 0].min() and c[0] + r < rest[:, 0].max() and c[2] - r > rest[:, 2].min() and c[1] + r < rest[:, 1].max()


# ------------------------------------------------------------------------------------------------
# the estimator
# ------------------------------------------------------------------------------------------------
def test_all_flat_table_renders_what_no_table_renders():
    s = OracleScene.load(CBOX)
    prims = s.prims()
    table = np.repeat(prims["normal"][:, None, :], 4, axis=1)
    for ne in (False, True):
        a = PO.PathRenderer(s, default_camera(), 8, 8, next_event=ne)
        b = SM.SmoothRenderer(s, default_camera(), 8, 8, table, next_event=ne)
        assert not b.smooth.any()
        ra, rb = a.frame(2, 5), b.frame(2, 5)
        assert np.array_equal(bits(ra[1]), bits(rb[1])) and np.array_equal(ra[0], rb[0]) and a.draws == b.draws


def test_smooth_table_changes_the_frame_on_the_spheres():
    prims = ptmi.HostScene.load(CBOX).prims()
    arrays, table, ranges = ptmi_scenes.cornell_spheres(prims, level=1)
    s = OracleScene.from_arrays(*arrays)
    a = PO.PathRenderer(s, default_camera(), 8, 8, next_event=True)
    b = SM.SmoothRenderer(s, default_camera(), 8, 8, table, next_event=True)
    assert int(b.smooth.sum()) == 160
    ra, rb = a.frame(2, 3), b.frame(2, 3)
    assert not np.array_equal(bits(ra[1]), bits(rb[1]))


@pytest.mark.parametrize("kind", [1, 2])
def test_black_furnace_depth_cuts_few_samples(kind):
    """max_depth 32 may cut at most 1e-4 of the restatement's samples on the black furnace around the sphere.  64 x 64 x 64 spp
    measured 4 of 262 144 for glass (1.5e-5) and 0 for the mirror (tests/smooth_scenes.py); this runs 16 384, the fewest that
    resolve the condition (one cut sample is 6e-5 of them)."""
    s, table, kinds = SS.black_sphere(kind)
    r = SM.SmoothRenderer(OracleScene.from_arrays(*s.arrays()), default_camera(), 32, 32, table, kind=kinds, next_event=True)
    assert int(r.smooth.sum()) == 20 * 4 ** SS.SPHERE_LEVEL
    r.trace = []
    r.sums(16, SS.BLACK_FURNACE_DEPTH)
    assert r.samples == 16384 and r.cut <= 1e-4 * r.samples
    assert kind in {k for k, _, _ in r.trace}                 # the sphere was met
