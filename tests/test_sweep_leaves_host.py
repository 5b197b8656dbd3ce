"""csrc/sweep_leaves.h on the host, before any kernel walks its records: tests/sweep_leaves_check.c, a stand-alone program built with
the system compiler, runs ptmi_sweep_leaves_prepare - the function stage_scene calls in the sweep's builds that test the leaf boxes
alone, and in the intersect hook - and ptmi_sweep_leaves_verdict - the function SceneState::upload asks before it lets them - on
the 194 trees of test_sweep_near_far_host.py: the records of every tree the builder gives for 1 ... 64 random primitives (triangles
only, quads only, mixed) and for both Cornell files, at two LDS addresses of the first primitive record.  It checks

  the image holds the leaves alone, in pre-order, each axis group lo, hi, hi, lo of the scene's node, bit for bit;
  the link vector is (address of the leaf's first primitive record, count) twice; the leaves' slots tile the primitives in order;
  a call strided like a 256-thread workgroup gives the bytes the whole call gives, and neither writes outside the table;
  ptmi_sweep_leaf_count, and ptmi_sweep_leaves_lds_vecs = [near/far nodes | primitives | frame block | materials | leaves];
  the verdict is 1 for every built tree;
  the verdict is 0 for copies in which one child plane lies one ulp outside its parent's - each of the six planes, left and right
  children - and 1 again with that plane exactly on the parent's; 0 where a plane is +inf, -inf or NaN; 0 where the root's right
  child or skip entry keeps a consistent range but is not where pre-order puts it.
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
    exe = str(tmp_path_factory.mktemp("sweep_leaves") / "sweep_leaves_check")
    subprocess.run([cc, "-O1", "-g", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "sweep_leaves_check.c"), "-lm"], check=True, timeout=120)
    return exe


def run(checker, tmp_path, scenes):
    data, n_nodes, n_leaves, mutants = b"", 0, 0, 0
    for hs in scenes:
        nodes, _, _, leaf = upload_records(hs)
        right, skip = int(nodes[0, 1, 3]), int(nodes[0, 0, 3])
        links = 0 if len(nodes) == 1 else int(right + 1 < skip) + int(skip - 1 > right)      # wrong links the tree has room for
        for prims_at in (0x540, 0x2A40 + 0x1FC0):              # behind 21 and 127 near/far node records, the second behind static LDS too
            d, a, _ = blob(hs, prims_at)
            data += d; n_nodes += a; n_leaves += int(leaf.sum())
            mutants += 24 + (6 if a > 1 else 0) + links                # 18 non-finite planes of the last node, 6 of the root; 6 child planes moved
    path = tmp_path / "records.bin"
    path.write_bytes(data)
    r = subprocess.run([checker, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", str(2 * len(scenes)), str(n_nodes), str(n_leaves), str(mutants)], r.stdout


@pytest.mark.parametrize("quads", [False, True, None], ids=["triangles", "quads", "mixed"])
def test_leaf_records_and_verdict_of_random_trees(checker, tmp_path, quads):
    scenes = [ptmi.HostScene.from_arrays(*soup(n, 100 * n + 7, quads)) for n in range(1, 65)]
    assert upload_records(scenes[0])[3].all()                  # one primitive: the root is the only leaf
    leaf = upload_records(scenes[63])[3]
    assert leaf.sum() > 16 and not leaf[0] and leaf[-1]        # 64 primitives: a tree, its last record a leaf
    run(checker, tmp_path, scenes)


def test_leaf_records_and_verdict_of_the_cornell_files(checker, tmp_path):
    scenes = [ptmi.HostScene.load(os.path.join(SCENES, f)) for f in ("cbox.obj", "cbox_quads.obj")]
    assert int(upload_records(scenes[0])[3].sum()) == 11 and len(upload_records(scenes[0])[0]) == 21
    run(checker, tmp_path, scenes)
