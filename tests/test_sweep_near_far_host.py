"""csrc/sweep_near_far.h on the host, before any kernel walks its records: tests/sweep_near_far_check.c, a stand-alone program built
with the system compiler, runs ptmi_sweep_near_far_prepare - the function stage_scene calls in the sweep's builds that read
(near, far) by address, and in the intersect hook - on the scene files of test_sweep_records_host.py: the records of every tree
the builder gives for 1 ... 64 random primitives (triangles only, quads only, mixed) and for both Cornell files, at two LDS
addresses of the first node.  It checks

  each axis group of a 64-byte record is lo, hi, hi, lo of the scene's node, bit for bit;
  w1 is copied; w0 of an interior node is the address of the node it named (address of the first node + 64 * index, index in
  (i, N]); w0 of a leaf is copied; the two pad words are 0;
  a call strided like a 256-thread workgroup gives the bytes the whole call gives, and neither writes outside the table;
  ptmi_sweep_near_far_lds_vecs is what [near/far nodes | primitives | frame block | materials] adds up to.
"""
import os
import shutil
import subprocess

import pytest

import ptmi
from oracle_binding import SCENES
from test_sweep_records_host import blob, soup, upload_records

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler found")
    exe = str(tmp_path_factory.mktemp("sweep_near_far") / "sweep_near_far_check")
    subprocess.run([cc, "-O1", "-g", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "sweep_near_far_check.c")], check=True, timeout=120)
    return exe


def run(checker, tmp_path, scenes):
    data, n_nodes = b"", 0
    for hs in scenes:
        for nodes_at in (0, 0x2A40):                           # dynamic LDS at 0, and behind static LDS
            d, a, _ = blob(hs, nodes_at)
            data += d; n_nodes += a
    path = tmp_path / "records.bin"
    path.write_bytes(data)
    r = subprocess.run([checker, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", str(2 * len(scenes)), str(n_nodes)], r.stdout


@pytest.mark.parametrize("quads", [False, True, None], ids=["triangles", "quads", "mixed"])
def test_near_far_records_of_random_trees(checker, tmp_path, quads):
    scenes = [ptmi.HostScene.from_arrays(*soup(n, 100 * n + 7, quads)) for n in range(1, 65)]
    shapes = [upload_records(hs) for hs in (scenes[0], scenes[63])]
    assert shapes[0][0].shape[0] == 1 and shapes[0][3].all()           # one primitive: the root is a leaf, one record
    nodes, _, _, leaf = shapes[1]
    assert (nodes[~leaf, 0, 3] == len(nodes)).any()                    # 64 primitives: a skip entry names the node one past the end
    run(checker, tmp_path, scenes)


def test_near_far_records_of_the_cornell_files(checker, tmp_path):
    run(checker, tmp_path, [ptmi.HostScene.load(os.path.join(SCENES, f)) for f in ("cbox.obj", "cbox_quads.obj")])
