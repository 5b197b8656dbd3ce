"""How often could the sweep's first Moller-Trumbore half reuse s = o - v0 of the test before it?  A triangle record could keep the
s of the record before it only where both stand in the same leaf, one right after the other, and their v0 are equal AS BITS (+0 and
-0 give different differences).  cbox.obj is 16 quads cut into fans (a, b, c), (a, c, d), so 16 of its 32 records share v0 with
their partner - but the builder sorts a leaf's records by centroid, and this test counts how many partners end up as neighbours in
a leaf of the tree the oracle builds (the tree every walk reads): 2 of 32.  Below 8 of 32 the shared subtraction cannot reach 0.5 %
of the benchmark frame (EXPERIMENTS.md), so csrc/sweep_records.h carries no such mark and the walk none of its code.  The test
keeps the count, and the constructed scenes of tests/test_gpu_sweep_masked.py, from drifting unnoticed.  No GPU.
"""
import os

import numpy as np

import ptmi
from oracle_binding import SCENES, OracleScene
import sweep_masked_scenes as S


def test_marked_count_of_cbox():
    o = OracleScene.load(os.path.join(SCENES, "cbox.obj"))
    v0, src, leaves = S.leaf_order(o)
    hv0, hsrc, hleaves = S.leaf_order(ptmi.HostScene.load(os.path.join(SCENES, "cbox.obj")))
    assert np.array_equal(v0, hv0) and np.array_equal(src, hsrc) and leaves == hleaves       # the product walks the oracle's tree
    assert len(v0) == 32 and sum(c for _, c in leaves) == 32
    # the fans: 16 records have the v0 of another record, bit for bit
    partners = sum(1 for k in range(32) if any((v0[k] == v0[j]).all() for j in range(32) if j != k))
    marks = S.same_origin_marks(v0, leaves)
    print(f"cbox.obj: {partners} of 32 records share v0 with another; {int(marks.sum())} of 32 follow such a record in their leaf")
    assert partners >= 16
    assert not any(marks[first] for first, _ in leaves)                  # never a leaf's first record
    assert int(marks.sum()) == 2
    assert int(marks.sum()) < 8                                          # the bar below which the mark is not built


def test_marks_compare_bits_and_stop_at_leaf_boundaries():
    z = np.array([[0.0, 1.0, 2.0], [-0.0, 1.0, 2.0], [-0.0, 1.0, 2.0], [-0.0, 1.0, 2.0]], np.float32)
    assert (z[0] == z[1]).all()                                          # equal as floats
    marks = S.same_origin_marks(z.view(np.uint32), [(0, 3), (3, 1)])
    assert marks.tolist() == [False, False, True, False]                 # +0 / -0 differ; slot 3 opens a leaf


def test_the_scenes_are_what_they_claim():
    shape = {}
    for name in S.NAMES:
        arrs = S.arrays(name)
        assert not arrs[0].any(), name                                   # triangles only: the builds that take the masked moves
        v0, src, leaves = S.leaf_order(S.oracle(name))
        hv0, hsrc, hleaves = S.leaf_order(ptmi.HostScene.from_arrays(*arrs))
        assert np.array_equal(v0, hv0) and np.array_equal(src, hsrc) and leaves == hleaves, name
        shape[name] = (v0, list(src), leaves, S.same_origin_marks(v0, leaves))
    assert shape["tri1"][2] == [(0, 1)]
    assert shape["pair"][2] == [(0, 2)] and shape["pair"][3].tolist() == [False, True]
    assert shape["twins"][2] == [(0, 2)]
    assert shape["fan5"][2] == [(0, 5)] and shape["fan5"][3].tolist() == [False, True, True, True, True]
    v0, src, leaves, marks = shape["pairs_apart"]
    assert len(leaves) == 2 and not marks.any()
    leaf_of = {int(s): n for n, (first, count) in enumerate(leaves) for s in src[first:first + count]}
    assert leaf_of[0] != leaf_of[1] and leaf_of[2] != leaf_of[3]         # the halves of both pairs stand in different leaves
    v0, src, leaves, marks = shape["zero_pair"]
    assert leaves == [(0, 2)] and not marks.any()
    f = v0.view(np.float32)
    assert (f[0] == f[1]).all() and not (v0[0] == v0[1]).all()           # equal as floats, not as bits
