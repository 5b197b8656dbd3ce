"""csrc/shade_lean.h on the host, before any kernel uses it: tests/shade_lean_check.c, a stand-alone program built with the system
compiler and -ffp-contract=off, compares

  ptmi_sincos_2pi_fast with ptmi_sincosf over ALL 1 086 918 620 arguments in [0, (float)(2 pi)]: no difference outside the
      ambiguity flag, and at most 1e-5 of the arguments flagged (the kernels send a flagged wave the long way);
  ptmi_div_by_size_lean with a / W for every float a in [2^-33, W], for W = 1024, 1920 and 16383.

x86's fma and the GPU's v_fma_f64 / v_fma_f32 are the same IEEE operation, so what holds here holds on the device;
tests/test_gpu_shade_lean_forms.py runs the same comparisons there.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TWO_PI_BITS = 0x40C90FDB
LO33 = (127 - 33) << 23
TIME_LIMIT = 600                 # seconds for each of the two comparisons; they take a few seconds on 8 cores with hardware fma
JOBS = max(1, min(16, len(os.sched_getaffinity(0))))


def bits(x):
    return int(np.array(x, np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler found")
    exe = str(tmp_path_factory.mktemp("shade_lean") / "shade_lean_check")
    flags = ["-O2", "-ffp-contract=off"]
    with open("/proc/cpuinfo") as f:
        if any(" fma " in line + " " for line in f if line.startswith("flags")):
            flags.append("-mfma")                   # otherwise libm's fma(): the same results, more slowly
    subprocess.run([cc, *flags, "-o", exe, os.path.join(HERE, "shade_lean_check.c"), "-lm"], check=True, timeout=120)
    return exe


def run_split(exe, head, first, count):
    """the range cut into JOBS pieces, one process each, all at once; the fields of their result lines"""
    step = (count + JOBS - 1) // JOBS
    procs = []
    for j in range(JOBS):
        lo = first + j * step
        n = min(step, first + count - lo)
        if n > 0:
            procs.append(subprocess.Popen([exe, *head, str(lo), str(n)], stdout=subprocess.PIPE, text=True))
    rows = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=TIME_LIMIT)
            assert p.returncode == 0, out
            rows.append([int(v) for v in out.split()[1:]])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rows


def test_sincos_fast_all_arguments(checker):
    n = TWO_PI_BITS + 1
    rows = run_split(checker, ["sincos"], 0, n)
    bad_sin = sum(r[0] for r in rows); bad_cos = sum(r[1] for r in rows)
    flagged = sum(r[2] for r in rows); flagged_diff = sum(r[3] for r in rows)
    first = [hex(r[4]) for r in rows if r[0] or r[1]]
    print(f"ptmi_sincos_2pi_fast: {flagged} of {n} arguments flagged ({flagged / n:.2e}), {flagged_diff} of them differ")
    assert bad_sin == 0 and bad_cos == 0, (bad_sin, bad_cos, first)
    assert flagged <= 1e-5 * n, flagged


@pytest.mark.parametrize("size", [1024, 1920, 16383])
def test_division_by_image_size(checker, size):
    rows = run_split(checker, ["div", str(size)], LO33, bits(size) - LO33 + 1)
    assert all(r[2] == 1 for r in rows)                    # this size takes the short form
    assert sum(r[0] for r in rows) == 0, [hex(r[1]) for r in rows if r[0]]
