"""Host side of next-event estimation (include/ptmi.h: ptmi_config.next_event, ptmi_host_emitters) - no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ptmi
from nee_oracle import emitter_table
from oracle_binding import SCENES, OracleScene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def soup(n, emitters, seed, zero_area=False):
    """n random triangles in the unit cube; `emitters` (index, Le) pairs; with zero_area the first emitter is degenerate"""
    rng = np.random.default_rng(seed)
    types = np.zeros(n, np.int32)
    verts = np.zeros((n, 4, 3), np.float32)
    c = rng.uniform(-1.0, 1.0, (n, 1, 3))
    verts[:, :3] = (c + rng.uniform(-0.2, 0.2, (n, 3, 3))).astype(np.float32)
    e1 = verts[:, 1] - verts[:, 0]; e2 = verts[:, 2] - verts[:, 0]
    normal = np.cross(e1, e2); normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    bsdf = np.full((n, 3), 0.6, np.float32)
    Le = np.zeros((n, 3), np.float32)
    for i, le in emitters:
        Le[i] = le
    if zero_area:
        i = emitters[0][0]
        verts[i, 2] = verts[i, 1]
    return types, verts, normal.astype(np.float32), bsdf, Le


def check(hs, os_):
    got = hs.emitters()
    prim, cdf, pdf_area = emitter_table(os_)
    assert np.array_equal(got["prim"], prim)
    assert got["cdf"].view(np.uint32).tolist() == cdf.view(np.uint32).tolist()
    assert got["pdf_area"].view(np.uint32).tolist() == pdf_area.view(np.uint32).tolist()
    return got


@pytest.mark.parametrize("name", ["cbox.obj", "cbox_quads.obj"])
def test_emitter_table_of_the_cornell_scenes(name):
    path = os.path.join(SCENES, name)
    got = check(ptmi.HostScene.load(path), OracleScene.load(path))
    assert len(got["prim"]) >= 1 and (got["pdf_area"] > 0).sum() == len(got["prim"])
    # pdf_area integrates to 1 over the emitters' area
    from nee_oracle import areas
    a = areas(OracleScene.load(path))
    assert abs(float((got["pdf_area"].astype(np.float64) * a).sum()) - 1.0) < 1e-5


def test_emitter_table_subdivided():
    path = os.path.join(SCENES, "cbox.obj")
    got = check(ptmi.HostScene.load(path, 2), OracleScene.load(path, 2))
    assert len(got["prim"]) > 2


def test_no_emitters():
    arrays = soup(40, [], 3)
    hs = ptmi.HostScene.from_arrays(*arrays)
    got = check(hs, OracleScene.from_arrays(*arrays))
    assert len(got["prim"]) == 0 and not got["pdf_area"].any()
    n = C.c_int(-1)
    assert ptmi.lib().ptmi_host_emitters(hs.h, C.byref(n), None, None, None) == 0 and n.value == 0


def test_zero_area_single_channel_and_uneven_power():
    emit = [(5, (4.0, 4.0, 4.0)), (17, (0.0, 3.0, 0.0)), (30, (1000.0, 200.0, 0.5)), (33, (1e-3, 0.0, 0.0)), (38, (-1.0, 0.5, 0.25))]
    arrays = soup(40, emit, 11, zero_area=True)
    hs = ptmi.HostScene.from_arrays(*arrays)
    got = check(hs, OracleScene.from_arrays(*arrays))
    assert 5 not in got["prim"].tolist()                  # zero area: w = 0
    assert 38 not in got["prim"].tolist()                 # (Le.x + Le.y) + Le.z < 0
    assert got["prim"].tolist() == [17, 30, 33]
    assert np.all(np.diff(got["cdf"]) > 0)


def test_the_table_ignores_stored_normals_and_leaves_out_what_select_cannot_use():
    """The table depends on the geometry and Le alone (the stored normal plays no part); a non-planar quad and an emitter whose
    weight the running sum absorbs are no emitters"""
    types, verts, normal, bsdf, Le = soup(40, [(i, (1.0, 2.0, 3.0)) for i in range(0, 40, 3)], 7)
    tilted = normal.copy(); tilted[:, 0] += 0.5
    tilted /= np.linalg.norm(tilted, axis=1, keepdims=True)
    a = check(ptmi.HostScene.from_arrays(types, verts, normal, bsdf, Le), OracleScene.from_arrays(types, verts, normal, bsdf, Le))
    b = check(ptmi.HostScene.from_arrays(types, verts, tilted, bsdf, Le), OracleScene.from_arrays(types, verts, tilted, bsdf, Le))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.all(np.diff(a["cdf"]) > 0)
    # quads: 0 planar, 1 bent out of its plane by 1e-3 of its diagonal (no emitter), 2 bent by 1e-5 (an emitter)
    types = np.ones(3, np.int32)
    verts = np.zeros((3, 4, 3), np.float32)
    for i in range(3):
        verts[i] = [(0, 0, 2 * i), (1, 0, 2 * i), (1, 1, 2 * i), (0, 1, 2 * i)]
    verts[1, 2, 2] += 1e-3 * np.sqrt(2.0); verts[2, 2, 2] += 1e-5 * np.sqrt(2.0)
    nq = np.tile(np.float32([[0, 0, 1]]), (3, 1))
    Le = np.ones((3, 3), np.float32); Le[0] = 1e9                          # quad 2's weight is absorbed behind quad 0's
    args = (types, verts, nq, np.full((3, 3), 0.5, np.float32), Le)
    got = check(ptmi.HostScene.from_arrays(*args), OracleScene.from_arrays(*args))
    assert got["prim"].tolist() == [0] and got["pdf_area"][1] == 0 and got["pdf_area"][2] == 0
    Le[0] = 1.0
    args = (types, verts, nq, np.full((3, 3), 0.5, np.float32), Le)
    got = check(ptmi.HostScene.from_arrays(*args), OracleScene.from_arrays(*args))
    assert got["prim"].tolist() == [0, 2]


def test_count_alone_and_null_scene():
    hs = ptmi.HostScene.load(os.path.join(SCENES, "cbox.obj"))
    n = C.c_int(-1)
    assert ptmi.lib().ptmi_host_emitters(hs.h, C.byref(n), None, None, None) == 0
    assert n.value == len(hs.emitters()["prim"])
    assert ptmi.lib().ptmi_host_emitters(None, C.byref(n), None, None, None) == -1      # PTMI_E_INVALID


def test_config_carries_next_event():
    names = [f for f, _ in ptmi.Config._fields_]
    assert names[-1] == "next_event"
    assert ptmi.default_config().next_event == 0
    header = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*ptmi_config;", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).group(1)
    assert body.strip().split(";")[-2].split()[-1] == "next_event"
    assert "ptmi_host_emitters" in ptmi.EXPORTS
