"""Identity of the built product, used to tell whether a committed rocprofv3 profile still describes the code that runs.

A profile under profiles/ carries two stamps (tools/pmc_summary.py writes them, bench.py checks them):
  lib_sha256         SHA-256 of cuda-pathtracer_amd/libptmi.so as it was profiled
  kernel_src_sha256  SHA-256 over the sources that are compiled into the render kernels (and the build flags)
The counters of a kernel stay valid while kernel_src_sha256 matches, even if an unrelated part of the library changed.
"""
import hashlib
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(_HERE)
ROOT = os.path.dirname(PKG)

def _csrc(*names):
    return [os.path.join(PKG, "csrc", n) for n in names]


# what both kernel sets include + the flags they are compiled with
_SHARED_SOURCES = _csrc("pt_device.h", "pt_vec.h", "device_scene.h", "wide_bvh.h", "wide_walk.h", "prim_sample.h") + [
    os.path.join(ROOT, "include", "ptmi_math.h"), os.path.join(PKG, "Makefile")]
# everything that reaches the render kernels' objects (the Makefile's RENDER_HIP and what those files include)
KERNEL_SOURCES = _csrc("kernels.hip", "bounce_sync.hip", "bounce_phased.hip", "bounce_wide.hip", "first_hit.hip", "debug_hooks.hip",
                       "traversal.h", "sweep_records.h", "sweep_near_far.h", "sweep_leaves.h", "frame_block.h", "shading.h", "shade_lean.h", "bounce.h") + _SHARED_SOURCES + [
    # the host loop that issues the kernels and the rule that decides how (chunks, run-ahead, segments per launch)
    os.path.join(PKG, "host", "render_run.cpp"), os.path.join(PKG, "host", "launch_rule.h"),
    # the builder of the opt-in fast tree: the tree's shape decides what ptmi_bounce_wide fetches
    os.path.join(PKG, "host", "wide_bvh.cpp"),
]
# everything that reaches build/radiosity.o and build/form_factors.o (the radiosity pre-pass kernels) + the host code that launches them
SOLVER_SOURCES = _csrc("radiosity.hip", "form_factors.hip", "anyhit.h") + _SHARED_SOURCES + [os.path.join(PKG, "host", "radiosity_state.cpp")]


def _sha(paths):
    h = hashlib.sha256()
    for p in paths:
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def lib_sha256():
    p = os.environ.get("PTMI_LIB") or os.path.join(PKG, "libptmi.so")
    if not os.path.exists(p):
        return None
    with open(p, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()        # = `sha256sum libptmi.so`


def kernel_src_sha256():
    return _sha(KERNEL_SOURCES)


def solver_src_sha256():
    return _sha(SOLVER_SOURCES)


def stamps():
    return {"lib_sha256": lib_sha256(), "kernel_src_sha256": kernel_src_sha256(), "solver_src_sha256": solver_src_sha256()}


def profile_is_current(profile, solver=False):
    """(current?, which stamp matched).  solver: the profile describes the radiosity pre-pass kernels (csrc/radiosity.hip, csrc/form_factors.hip)"""
    if profile.get("lib_sha256") and profile.get("lib_sha256") == lib_sha256():
        return True, "lib"
    if solver:
        if profile.get("solver_src_sha256") and profile.get("solver_src_sha256") == solver_src_sha256():
            return True, "solver_sources"
        return False, None
    if profile.get("kernel_src_sha256") and profile.get("kernel_src_sha256") == kernel_src_sha256():
        return True, "kernel_sources"
    return False, None
