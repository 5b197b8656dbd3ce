"""host/albedo_texture.cpp - the check of a caller's image, UV table and mask, the host code of include/ptmi.h's "albedo texture"
that walks a caller's memory - under AddressSanitizer and UndefinedBehaviorSanitizer: tests/albedo_texture_check.cpp, a stand-alone
program, is built with both (host code only) together with that file and run.  Its arrays are heap blocks of exactly the stated
sizes, and the UVs of untextured primitives are missing from their block, so a read past a caller's array, or of UVs that the
contract says are never read, ends the program.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = 229


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found (the build needs it too)")
    exe = str(tmp_path_factory.mktemp("albedo_texture") / "albedo_texture_check")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                    "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(HERE, "albedo_texture_check.cpp"), os.path.join(ROOT, "cuda-pathtracer_amd", "host", "albedo_texture.cpp"),
                    "-o", exe], check=True, timeout=300)
    return exe


def test_the_check_under_the_sanitizers(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[-2].startswith("ok ") and int(lines[-2].split()[1]) == CASES and not any(ln.startswith("FAILED") for ln in lines), r.stdout[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_the_program_is_instrumented(checker):
    """the build did link the sanitizer runtimes: a test that passes without them shows nothing"""
    nm = shutil.which("nm")
    if nm is None:
        pytest.fail("nm not found")
    syms = subprocess.run([nm, "-D", checker], capture_output=True, text=True, timeout=60).stdout + \
        subprocess.run([nm, checker], capture_output=True, text=True, timeout=60).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms
