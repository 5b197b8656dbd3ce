"""csrc/sweep_records.h on the host, before any kernel walks its records: tests/sweep_records_check.c, a stand-alone program built
with the system compiler, runs ptmi_sweep_prepare - the function stage_scene calls in the sweep's kernels and in the intersect
hook - on the records of every tree the builder gives for 1 ... 64 random primitives (triangles only, quads only, mixed) and for
both Cornell files, at two LDS addresses of the first node, and checks

  each interior node's skip lane is the address of the node it named (address of the first node + 32 * index, index in (i, N]);
  leaf nodes and every other lane are copied as they are;
  each primitive's slot lane holds its leaf-order slot, every other word is copied as it is;
  a call strided like a 256-thread workgroup gives what the whole call gives, and neither writes outside the two tables.

The records are laid out here as SceneState::upload lays them out (host/scene_state.cpp), from HostScene.bvh().
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptmi
from oracle_binding import SCENES

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler found")
    exe = str(tmp_path_factory.mktemp("sweep_records") / "sweep_records_check")
    subprocess.run([cc, "-O1", "-g", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "sweep_records_check.c")], check=True, timeout=120)
    return exe


def soup(n, seed, quads):
    """n random primitives; quads: None mixed, False triangles only, True quads only"""
    rng = np.random.default_rng(seed)
    types = (rng.random(n) < 0.4).astype(np.int32) if quads is None else np.full(n, int(quads), np.int32)
    centers = rng.uniform(-2.5, 2.5, (n, 1, 3)) + np.array([0, 2.5, 0])
    verts = (centers + rng.normal(0, 0.6, (n, 4, 3))).astype(F)
    q = types == 1
    verts[q, 2] = verts[q, 1] + (verts[q, 3] - verts[q, 0])
    normal = rng.normal(0, 1, (n, 3)); normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    return types, verts, normal.astype(F), rng.uniform(0.2, 0.9, (n, 3)).astype(F), np.zeros((n, 3), F)


def upload_records(hs):
    """(nodes, prims, stride): the float4 tables of SceneState::upload as uint32 words"""
    b, p = hs.bvh(), hs.prims()
    n_nodes, n = len(b["left"]), len(p["type"])
    leaf = b["count"] > 0
    subtree = np.ones(n_nodes, np.int64)
    for i in range(n_nodes - 1, -1, -1):
        if not leaf[i]:
            assert b["left"][i] == i + 1                       # pre-order
            subtree[i] = 1 + subtree[b["left"][i]] + subtree[b["right"][i]]
    nodes = np.zeros((n_nodes, 2, 4), np.uint32)
    nodes[:, 0, :3] = b["bmin"].view(np.uint32); nodes[:, 1, :3] = b["bmax"].view(np.uint32)
    nodes[:, 0, 3] = np.where(leaf, b["left"], np.arange(n_nodes) + subtree).astype(np.int32).view(np.uint32)
    nodes[:, 1, 3] = np.where(leaf, -b["count"], b["right"]).astype(np.int32).view(np.uint32)
    stride = 4 if (p["type"] == 1).any() else 3
    src = b["indices"]
    v = p["verts"][src]; quad = p["type"][src] == 1
    prims = np.zeros((n, stride, 4), F)
    prims[:, 0, :3] = v[:, 0]; prims[:, 1, :3] = v[:, 1] - v[:, 0]; prims[:, 2, :3] = v[:, 2] - v[:, 0]
    if stride == 4:
        prims[quad, 3, :3] = v[quad, 3] - v[quad, 0]
    prims = prims.view(np.uint32)
    prims[:, 0, 3] = quad
    return nodes, prims, stride, leaf


def blob(hs, nodes_at):
    nodes, prims, stride, _ = upload_records(hs)
    head = np.array([len(nodes), stride, len(prims)], np.int32).tobytes() + np.array([nodes_at], np.uint32).tobytes()
    return head + nodes.tobytes() + prims.tobytes(), len(nodes), len(prims)


def run(checker, tmp_path, scenes):
    data, n_nodes, n_prims = b"", 0, 0
    for hs in scenes:
        for nodes_at in (0, 0x2A40):                           # dynamic LDS at 0, and behind static LDS
            d, a, b = blob(hs, nodes_at)
            data += d; n_nodes += a; n_prims += b
    path = tmp_path / "records.bin"
    path.write_bytes(data)
    r = subprocess.run([checker, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", str(2 * len(scenes)), str(n_nodes), str(n_prims)], r.stdout


@pytest.mark.parametrize("quads", [False, True, None], ids=["triangles", "quads", "mixed"])
def test_prepared_records_of_random_trees(checker, tmp_path, quads):
    scenes = [ptmi.HostScene.from_arrays(*soup(n, 100 * n + 7, quads)) for n in range(1, 65)]
    shapes = [upload_records(hs) for hs in (scenes[0], scenes[63])]
    assert shapes[0][0].shape[0] == 1 and shapes[0][3].all()           # one primitive: the root is a leaf, one record
    nodes, _, _, leaf = shapes[1]
    assert (nodes[~leaf, 0, 3] == len(nodes)).any()                    # 64 primitives: a skip entry names the node one past the end
    run(checker, tmp_path, scenes)


def test_prepared_records_of_the_cornell_files(checker, tmp_path):
    run(checker, tmp_path, [ptmi.HostScene.load(os.path.join(SCENES, f)) for f in ("cbox.obj", "cbox_quads.obj")])
