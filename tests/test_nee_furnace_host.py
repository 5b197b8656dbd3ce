"""White-furnace checks of next-event estimation on the CPU (tests/furnace.py; include/ptmi.h, "next-event estimation") - no
GPU needed.  The oracle's reference estimator proves every furnace closed and the analytic value right; the restatement of the
NEE contract (tests/path_oracle.py) must then reach the same value; the emitter table must stay usable at the edges of float."""
import os

import numpy as np
import pytest

import furnace as FN
import ptmi
from nee_oracle import areas, emitter_table
from oracle_binding import SCENES, OracleScene, default_camera
from path_oracle import NeeRenderer



def load(name, tmp_path):
    """(OracleScene, HostScene, furnace.Scene) of a variant, through the .obj loader for "tilted_obj" """
    src, s = FN.load_pair(name, tmp_path)
    if isinstance(src, str):
        return OracleScene.load(src), ptmi.HostScene.load(src), s
    return OracleScene.from_arrays(*src), ptmi.HostScene.from_arrays(*src), s


def stats(rad, value):
    """(mean, SE, z) per channel; every pixel is an independent estimate of one number, so their spread gives the SE.  A floor
    of 2e-5 of the value on the SE absorbs float rounding where an estimator has no variance."""
    px = rad.reshape(-1, 3).astype(np.float64)
    mean = px.mean(0)
    se = px.std(0, ddof=1) / np.sqrt(len(px))
    return mean, se, np.abs(mean - value) / np.maximum(se, 2e-5 * np.abs(value))


# ------------------------------------------------------------------------------------------------
# the scenes themselves: closed, the walk each is meant for, the formula right
# ------------------------------------------------------------------------------------------------
def test_variants_reach_the_walks_they_are_for(tmp_path):
    info = {}
    for name in FN.VARIANTS + ["tilted_obj"]:
        o, hs, s = load(name, tmp_path)
        info[name] = (hs.info(), hs.emitters())
        assert np.isfinite(o.prims()["normal"]).all()
    n = lambda k: info[k][0]["n_prims"]
    for k in ("tris", "quads", "panels", "tilted", "tilted_mixed", "tilted_obj", "warped"):
        assert n(k) <= 64, k                                             # the lane walk
    assert info["tris"][0]["n_quads"] == 0 and info["quads"][0]["n_tris"] == 0
    for k in ("tris_many", "quads_many", "emitters_4k", "declined"):
        assert n(k) > 64 and info[k][0]["bvh_depth"] <= 62, k            # the certified walk, or the reference's tree
    assert info["quads_many"][0]["n_tris"] == 0
    assert len(info["emitters_4k"][1]["prim"]) >= 4096
    for k in ("deep", "deep_quads"):
        assert info[k][0]["bvh_depth"] > 62, k                          # the stack walk
    assert info["deep_quads"][0]["n_tris"] == 0
    _, hs, _ = load("declined", tmp_path)
    with pytest.raises(ptmi.PtmiError):
        hs.fast_tree_build()                                             # the 8-wide builder declines it
    _, hs, _ = load("tris_many", tmp_path)
    hs.fast_tree_build()
    # the obj variant is the arrays variant, the stored normals included
    oa, _, _ = load("tilted", tmp_path)
    ob, _, _ = load("tilted_obj", tmp_path)
    pa, pb = oa.prims(), ob.prims()
    for key in ("type", "verts", "normal", "bsdf", "Le"):
        assert np.array_equal(pa[key], pb[key]), key


@pytest.mark.parametrize("name", FN.VARIANTS + ["tilted_obj"])
def test_closure_every_pixel_is_the_analytic_value(name, tmp_path):
    """Without roulette (max_depth <= 3) the reference's estimator has no variance in a closed furnace: a single ray that escaped,
    or a primitive of another colour, shows as one pixel off the value."""
    o, _, _ = load(name, tmp_path)
    for depth in ((1, 2) if name in FN.TILTED else (1, 2, 3)):
        _, rad, _ = o.render(default_camera(), 48, 40, 4, max_depth=depth)
        rel = rad.astype(np.float64) / FN.expected(depth) - 1.0
        assert np.abs(rel).max() < 1e-5, (name, depth, float(np.abs(rel).max()))


@pytest.mark.parametrize("name", [v for v in FN.VARIANTS if v not in FN.TILTED])
def test_closure_with_roulette(name, tmp_path):
    o, _, _ = load(name, tmp_path)
    for depth in (5, 8):
        _, rad, _ = o.render(default_camera(), 64, 64, 64, max_depth=depth)
        mean, se, z = stats(rad, FN.expected(depth))
        assert (z < 5.0).all() and (5.0 * se <= 0.005 * FN.expected(depth)).all(), (name, depth, mean, se, z)


def test_tilted_normals_leak_only_after_depth_two(tmp_path):
    """The reason variant h is compared with the reference's own mean beyond max_depth 2: after a self-hit the spawn point can lie
    outside the wall.  Were this to change, the analytic value would hold at every depth."""
    o, _, _ = load("tilted", tmp_path)
    _, rad, _ = o.render(default_camera(), 48, 40, 16, max_depth=3)
    assert rad.astype(np.float64).mean() < 0.995 * FN.expected(3).mean()


# ------------------------------------------------------------------------------------------------
# the restatement of the NEE contract in the furnaces
# ------------------------------------------------------------------------------------------------
def nee_stats(o, depth, size=16, spp=24):
    r = NeeRenderer(o, default_camera(), size, size)
    _, rad = r.frame(spp, depth)
    return rad


@pytest.mark.parametrize("name,depth", [("tris", 2), ("tris", 3), ("quads", 3), ("panels", 3), ("warped", 3),
                                        ("tilted", 2), ("tilted_obj", 2), ("tilted_mixed", 2)])
def test_restatement_reaches_the_analytic_value(name, depth, tmp_path):
    o, _, _ = load(name, tmp_path)
    value = FN.expected(depth)
    mean, se, z = stats(nee_stats(o, depth), value)
    print(f"{name} depth {depth}: NEE mean {mean}, analytic {value}, SE {se}, z {z}")
    assert (z < 5.0).all(), (name, depth, mean, value, se, z)
    assert (5.0 * se <= 0.01 * value).all(), (name, depth, se)


@pytest.mark.parametrize("name", ["tilted", "tilted_mixed"])
def test_restatement_equals_the_reference_estimator_beyond_depth_two(name, tmp_path):
    o, _, _ = load(name, tmp_path)
    m_ref, se_ref, _ = stats(o.render(default_camera(), 64, 64, 64, max_depth=3)[1], FN.expected(3))
    m_nee, se_nee, _ = stats(nee_stats(o, 3), FN.expected(3))
    z = np.abs(m_nee - m_ref) / np.hypot(se_ref, se_nee)
    print(f"{name} depth 3: NEE {m_nee} +- {se_nee}, reference estimator {m_ref} +- {se_ref}, z {z}")
    assert (z < 5.0).all(), (name, m_nee, m_ref, z)


# ------------------------------------------------------------------------------------------------
# the emitter table at its edges (ptmi_host_emitters on both loaders, against the restatement)
# ------------------------------------------------------------------------------------------------
def table(hs, o):
    got = hs.emitters()
    prim, cdf, pdf_area = emitter_table(o)
    assert np.array_equal(got["prim"], prim)
    assert got["cdf"].view(np.uint32).tolist() == cdf.view(np.uint32).tolist()
    assert got["pdf_area"].view(np.uint32).tolist() == pdf_area.view(np.uint32).tolist()
    return got


def invariants(got, o):
    prim, cdf, pa = got["prim"], got["cdf"], got["pdf_area"]
    assert np.isfinite(cdf).all() and np.isfinite(pa).all() and (pa >= 0).all()
    if len(prim) == 0:
        assert not pa.any()
        return
    # every primitive with pdf_area > 0 is an emitter, and every emitter has a non-empty selection interval (c_j > c_{j-1})
    assert set(np.flatnonzero(pa > 0).tolist()) <= set(prim.tolist())
    assert np.all(np.diff(np.concatenate([[0.0], cdf.astype(np.float64)])) > 0)
    # pdf_area is the selection probability per unit area: it integrates to 1 over the emitters
    a = areas(o).astype(np.float64)[prim]
    assert abs(float((pa[prim].astype(np.float64) * a).sum()) - 1.0) < 1e-5


@pytest.mark.parametrize("name", FN.VARIANTS + ["tilted_obj"])
def test_emitter_table_of_the_furnaces(name, tmp_path):
    o, hs, _ = load(name, tmp_path)
    got = table(hs, o)
    invariants(got, o)
    if name == "warped":                                                 # the non-planar quad is left out of the table
        assert 12 not in got["prim"].tolist() and got["pdf_area"][12] == 0 and len(got["prim"]) == 12
    if name == "emitters_4k":                                            # tiny triangles absorbed by the sum: not emitters
        assert len(got["prim"]) < hs.info()["n_prims"]


@pytest.mark.parametrize("name", ["cbox.obj", "cbox_quads.obj"])
def test_emitter_table_invariants_of_the_cornell_scenes(name):
    path = os.path.join(SCENES, name)
    o = OracleScene.load(path)
    invariants(table(ptmi.HostScene.load(path), o), o)


def two(le0, le1, scale0=1.0, scale1=1.0):
    """two triangles of the given Le and edge scale, facing each other"""
    s = FN.Scene()
    s.tri((0, 0, 0), (scale0, 0, 0), (0, scale0, 0), le=le0)
    s.tri((0, 0, 5), (0, scale1, 5), (scale1, 0, 5), le=le1)
    return s.arrays()


@pytest.mark.parametrize("case", ["absorbed", "absorbed_first", "le_1e30", "le_3e38", "le_3e38_both", "area_1e17", "area_huge"])
def test_emitter_table_edges(case):
    le = {"absorbed": ((2e9, 0, 0), (2, 0, 0)), "absorbed_first": ((2, 0, 0), (2e9, 0, 0)),
          "le_1e30": ((1e30, 1e30, 1e30), (1, 1, 1)), "le_3e38": ((3e38, 3e38, 3e38), (1, 1, 1)),
          "le_3e38_both": ((3.4e38, 3.4e38, 3.4e38), (3.4e38, 1, 0)), "area_1e17": ((3e38, 0, 0), (1, 1, 1)),
          "area_huge": ((1, 1, 1), (1, 1, 1))}[case]
    scale = {"area_1e17": (3e8, 1.0), "area_huge": (1e17, 1.0)}.get(case, (1.0, 1.0))
    arrays = two(le[0], le[1], *scale)
    o = OracleScene.from_arrays(*arrays)
    got = table(ptmi.HostScene.from_arrays(*arrays), o)
    invariants(got, o)
    if case == "absorbed":                                               # weight 1 after weight 1e9: never selected, no pdf
        assert got["prim"].tolist() == [0] and got["pdf_area"][1] == 0
    if case == "absorbed_first":                                         # the other order: both keep an interval
        assert got["prim"].tolist() == [0, 1] and (got["pdf_area"] > 0).all()
    if case == "area_huge":                                              # Triangle::area overflows: not an emitter
        assert got["prim"].tolist() == [1]
    if case in ("le_3e38", "le_3e38_both", "area_1e17"):
        assert got["pdf_area"][0] > 0


def test_emitter_table_edges_through_the_obj_loader(tmp_path):
    for ke in ("1e30 1e30 1e30", "3e38 3e38 3e38", "3.4e38 3.4e38 3.4e38"):
        (tmp_path / "e.mtl").write_text(f"newmtl hot\nKd 0.5 0.5 0.5\nKe {ke}\nnewmtl dim\nKd 0.5 0.5 0.5\nKe 1 1 1\n")
        (tmp_path / "e.obj").write_text("mtllib e.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 5\nv 0 1 5\nv 1 0 5\nv 2 0 5\nv 2 1 5\n"
                                        "usemtl hot\nf 1 2 3\nusemtl dim\nf 4 5 6\nf 6 7 8 5\n")
        path = str(tmp_path / "e.obj")
        o = OracleScene.load(path)
        got = table(ptmi.HostScene.load(path), o)
        invariants(got, o)
        assert got["pdf_area"][0] > 0
