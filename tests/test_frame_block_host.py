"""csrc/frame_block.h on the host, before a kernel reads the block: tests/frame_block_check.c, a stand-alone program built with the
system compiler, packs the frame block with ptmi_frame_block_pack - the function stage_scene calls in the sweep's kernels and in the
intersect hook - and this test compares every word with the layout laid out here, in numpy:

  vector 0  llc, (float)width      vector 1  hor, 1 / width or 0      vector 2  ver, (float)height      vector 3  org, 1 / height or 0

Each field must arrive with its bits: a -0.0 stays -0.0, a denormal is not flushed, FLT_MAX-sized components and NaN payloads pass
unchanged.  The reciprocal is the correctly rounded 1 / (float)size for 1 <= size <= 2^23 and 0 above (the kernels then keep the
IEEE division): sizes 1, 2, 3, 1024, 2^23 - 1, 2^23, 2^23 + 1, 2^24 + 1 and 2^31 - 1.
"""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
F, U = np.float32, np.uint32
SIZES = (1, 2, 3, 1024, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) + 1, (1 << 31) - 1)
FLT_MAX = np.finfo(F).max
DENORMAL_MIN = np.array([1], U).view(F)[0]                # 2^-149
DENORMAL_MAX = np.array([0x007FFFFF], U).view(F)[0]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler found")
    exe = str(tmp_path_factory.mktemp("frame_block") / "frame_block_check")
    subprocess.run([cc, "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "frame_block_check.c")], check=True, timeout=120)
    return exe


def cameras():
    """(name, 12 floats as bits: org, llc, hor, ver)"""
    rng = np.random.default_rng(23)
    plain = np.array([0.0, 2.5, 9.0, -1.2, 1.6, 7.5, 2.4, 0.0, 0.0, 0.0, 1.8, 0.0], F)
    out = [("plain", plain.view(U).copy())]
    for name, v in (("minus_zero", F(-0.0)), ("denormal_min", DENORMAL_MIN), ("denormal_max", -DENORMAL_MAX), ("flt_max", FLT_MAX),
                    ("minus_flt_max", -FLT_MAX), ("inf", F(np.inf))):
        c = plain.copy()
        c[[1, 4, 6, 7, 10, 11]] = v                      # one component of org and llc, two of hor and of ver
        out.append((name, c.view(U).copy()))
    nan = plain.view(U).copy()
    nan[[0, 5, 8, 9]] = [0x7FC12345, 0xFFC00001, 0x7F800001, 0xFFBFFFFF]       # quiet and signalling NaNs with payloads
    out.append(("nan_payloads", nan))
    out.append(("every_field_minus_zero", np.full(12, 0x80000000, U)))
    for k in range(8):
        out.append((f"random_bits_{k}", rng.integers(0, 1 << 32, 12, dtype=np.uint64).astype(U)))
    return out


def reciprocal(size):
    return F(1.0) / F(size) if 1 <= size <= (1 << 23) else F(0.0)


def expected(cam_bits, width, height):
    org, llc, hor, ver = (cam_bits[3 * i:3 * i + 3] for i in range(4))
    w = lambda x: np.array([x], F).view(U)
    return np.concatenate([llc, w(F(width)), hor, w(reciprocal(width)), ver, w(F(height)), org, w(reciprocal(height))]).astype(U)


def test_the_reciprocal_is_zero_exactly_above_2_23():
    assert [reciprocal(s) != 0 for s in SIZES] == [True, True, True, True, True, True, False, False, False]
    assert reciprocal(1) == 1.0 and reciprocal(1 << 23).view(U) == 0x34000000
    assert F((1 << 24) + 1) == F(1 << 24)                  # the block's size field is the rounded conversion the kernels made before


def test_block_reproduces_every_field(checker, tmp_path):
    cams = cameras()
    cases = [(name, c, w, h) for (name, c), (w, h) in itertools.product(cams, itertools.product(SIZES, repeat=2))]
    blob = b"".join(c.tobytes() + np.array([w, h], np.int32).tobytes() for _, c, w, h in cases)
    src, dst = tmp_path / "cases.bin", tmp_path / "blocks.bin"
    src.write_bytes(blob)
    r = subprocess.run([checker, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", str(len(cases))], r.stdout
    got = np.frombuffer(dst.read_bytes(), U).reshape(len(cases), 16)
    for (name, c, w, h), g in zip(cases, got):
        assert np.array_equal(g, expected(c, w, h)), (name, w, h, [hex(x) for x in g], [hex(x) for x in expected(c, w, h)])
    # the cases do hold what they claim: a -0.0, both ends of the denormals and FLT_MAX reached the block as they are
    words = set(got[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]].ravel().tolist())
    assert {0x80000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800001} <= words
    wide = [g for (_, _, w, h), g in zip(cases, got) if w == (1 << 23) + 1 and h == 1]
    assert wide and all(g[7] == 0 and g[15] == 0x3F800000 and g[3] == 0x4B000001 for g in wide)     # inv_width 0, 1 / 1, (float)(2^23 + 1)
