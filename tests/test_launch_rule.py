"""The launch rule (cuda-pathtracer_amd/host/launch_rule.h) as numbers, without a GPU: segments per launch, refill, the cost order,
the automatic chunk count and the per-launch borders.  tests/launch_rule_shim.cpp is compiled with the host C++ compiler; the
expected values are the ones the launch loop has used since rounds 2 - 4."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE, PHASED, SWEEP, WIDE = 0, 1, 2, 3            # the shim's walk classes: lane / stack, phased / packed, sweep, wide / certified
REST = 65536


class RuleIn(C.Structure):
    _fields_ = [("walk", C.c_int), ("segments_per_launch", C.c_int), ("spp", C.c_int), ("n_local", C.c_longlong), ("n_frames", C.c_int),
                ("nee", C.c_int), ("is_pass", C.c_int), ("want_chunks", C.c_int), ("wave_slots", C.c_longlong), ("use_env", C.c_int)]


class RuleOut(C.Structure):
    _fields_ = [("needs_wave_slots", C.c_int), ("segments", C.c_int), ("rest_segments", C.c_int), ("fit_pct", C.c_longlong),
                ("refill", C.c_int), ("run_ahead", C.c_int), ("order_by_cost", C.c_int), ("order_classes", C.c_int),
                ("auto_chunks", C.c_int), ("publish", C.c_int)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("needs a C++ compiler")
    so = str(tmp_path_factory.mktemp("launch_rule") / "liblaunch_rule_shim.so")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(ROOT, "tests", "launch_rule_shim.cpp")])
    L = C.CDLL(so)
    L.shim_plan.restype = None; L.shim_plan.argtypes = [C.POINTER(RuleIn), C.POINTER(RuleOut)]
    L.shim_launch.restype = None; L.shim_launch.argtypes = [C.POINTER(RuleIn), C.c_longlong, C.c_longlong, C.POINTER(C.c_int)]
    L.shim_cost_order.restype = C.c_int; L.shim_cost_order.argtypes = [C.POINTER(RuleIn), C.c_int]
    return L


def rule_in(walk, segments_per_launch=0, spp=8, n_local=96 * 96, n_frames=1, nee=0, is_pass=0, want_chunks=0, slots=0, use_env=0):
    return RuleIn(walk, segments_per_launch, spp, n_local, n_frames, nee, is_pass, want_chunks, slots, use_env)


def plan(L, **kw):
    out = RuleOut()
    L.shim_plan(C.byref(rule_in(**kw)), C.byref(out))
    return out


def launch(L, active, bound=None, **kw):
    """fits, many_waves, max_waves, the launch's segments"""
    out = (C.c_int * 4)()
    L.shim_launch(C.byref(rule_in(**kw)), active, active if bound is None else bound, out)
    return bool(out[0]), bool(out[1]), out[2], out[3]


def cost_order(L, n_chunks=1, **kw):
    return bool(L.shim_cost_order(C.byref(rule_in(**kw)), n_chunks))


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    for v in ("PTMI_PUBLISH", "PTMI_REFILL", "PTMI_ORDER"):
        monkeypatch.delenv(v, raising=False)


def test_lane_and_stack_walk(shim):
    p = plan(shim, walk=LANE, slots=1000)              # slots offered although not asked for: the rule does not use them
    assert (p.needs_wave_slots, p.segments, p.refill, p.run_ahead) == (0, 32, 0, 2)
    for active in (1, 64, 19200, 76800, 10 ** 7):
        fits, many, max_waves, seg = launch(shim, active, walk=LANE, slots=1000)
        assert (fits, many, max_waves, seg) == (False, False, 0, 32)
    assert plan(shim, walk=LANE, n_local=(1 << 18) - 1).auto_chunks == 1
    assert plan(shim, walk=LANE, n_local=1 << 18).auto_chunks == 2


@pytest.mark.parametrize("walk", [LANE, PHASED, SWEEP, WIDE])
def test_forced_segments_switch_the_rule_off(shim, walk):
    p = plan(shim, walk=walk, segments_per_launch=3, spp=2048, slots=1000)
    assert (p.segments, p.needs_wave_slots, p.refill, p.run_ahead) == (3, 0, 0, 2)
    for active in (1, 64, 19200, 76800, 127937, 10 ** 7):
        fits, many, max_waves, seg = launch(shim, active, walk=walk, segments_per_launch=3, spp=2048, slots=1000)
        assert (fits, many, max_waves, seg) == (False, False, 0, 3)


def test_phased_and_packed_walk(shim):
    for spp, want in ((4, 32), (127, 32), (128, 32), (132, 33), (2048, 512), (2052, 512)):
        p = plan(shim, walk=PHASED, spp=spp, slots=1000)
        assert (p.needs_wave_slots, p.segments, p.fit_pct, p.rest_segments, p.refill) == (1, want, 120, REST, 0), spp
    assert launch(shim, 76800, walk=PHASED, slots=1000) == (True, False, 0, REST)
    assert launch(shim, 76801, walk=PHASED, slots=1000) == (False, False, 0, 32)
    assert launch(shim, 127937, walk=PHASED, slots=1000)[1] is True
    assert launch(shim, 127936, walk=PHASED, slots=1000)[1] is False
    assert launch(shim, 76800, walk=PHASED, slots=0) == (False, False, 0, 32)       # no answer from the occupancy query: never fits


def test_sweep(shim):
    for spp in (4, 128, 2048):
        p = plan(shim, walk=SWEEP, spp=spp, slots=1000)
        assert (p.needs_wave_slots, p.segments, p.fit_pct, p.rest_segments, p.refill) == (1, 32, 30, REST, 0)
    assert launch(shim, 19200, walk=SWEEP, slots=1000) == (True, False, 0, REST)
    assert launch(shim, 19201, walk=SWEEP, slots=1000) == (False, False, 0, 32)
    for active in (127936, 127937, 10 ** 7):
        assert launch(shim, active, walk=SWEEP, slots=1000)[1] is False


def test_wide_and_certified_walk(shim):
    for spp, seg in ((8, 32), (2048, 512), (4096, 512)):
        p = plan(shim, walk=WIDE, spp=spp, slots=1000)
        assert (p.segments, p.rest_segments) == (seg, max(seg, 512))
    assert plan(shim, walk=WIDE, segments_per_launch=600, slots=1000).rest_segments == 600
    # refill: slots > 0, not NEE, segments_per_launch 0
    assert plan(shim, walk=WIDE, slots=1000).refill == 1
    assert plan(shim, walk=WIDE, slots=0).refill == 0
    assert plan(shim, walk=WIDE, slots=1000, nee=1).refill == 0
    assert plan(shim, walk=WIDE, slots=1000, segments_per_launch=32).refill == 0
    assert plan(shim, walk=WIDE, slots=1000, is_pass=1).refill == 1
    for n_local in (1, (1 << 18) - 1, 1 << 18, 1 << 24):
        p = plan(shim, walk=WIDE, slots=1000, n_local=n_local)
        assert (p.refill, p.run_ahead, p.auto_chunks) == (1, 1, 1)
        for active in (1, n_local):
            assert launch(shim, active, walk=WIDE, slots=1000, n_local=n_local)[3] == REST
    assert plan(shim, walk=WIDE, slots=1000, want_chunks=3).auto_chunks == 0        # a forced count stays
    assert plan(shim, walk=WIDE, slots=0, n_local=1 << 18).auto_chunks == 2         # without refill: by size, like every walk
    # max_waves: the chunk's share of the slots, rounded down to a multiple of 4, at least 4
    assert launch(shim, 5000, 5000, walk=WIDE, slots=1001)[2] == 1000
    assert launch(shim, 300, 100, walk=WIDE, slots=1001)[2] == 332
    assert launch(shim, 100000, 1, walk=WIDE, slots=1001)[2] == 4
    assert launch(shim, 0, 0, walk=WIDE, slots=1001)[2] == 0                        # nothing in flight: no schedule
    # cost order: at most three pixels per lane of the launch, one chunk, one frame
    assert plan(shim, walk=WIDE, slots=1000, n_local=192 * 1000).order_by_cost == 1
    assert plan(shim, walk=WIDE, slots=1000, n_local=192 * 1000 + 1).order_by_cost == 0
    assert plan(shim, walk=WIDE, slots=1000).order_classes == 16
    assert cost_order(shim, 1, walk=WIDE, slots=1000, n_local=192 * 1000)
    assert not cost_order(shim, 1, walk=WIDE, slots=1000, n_local=192 * 1000 + 1)
    assert not cost_order(shim, 2, walk=WIDE, slots=1000, n_local=192 * 1000)
    assert not cost_order(shim, 1, walk=WIDE, slots=1000, n_local=192 * 1000, n_frames=2)
    assert not cost_order(shim, 1, walk=WIDE, slots=1000, n_local=192 * 1000, segments_per_launch=32)   # no refill, no order
    assert not cost_order(shim, 1, walk=PHASED, slots=1000, n_local=192 * 1000)


def test_overrides(shim, monkeypatch):
    kw = dict(walk=WIDE, slots=1000, use_env=1)
    assert plan(shim, **kw).publish == 0
    monkeypatch.setenv("PTMI_REFILL", "0")
    assert plan(shim, **kw).refill == 0
    assert plan(shim, **kw).auto_chunks == 1 and plan(shim, n_local=1 << 18, **kw).auto_chunks == 2
    assert plan(shim, walk=WIDE, slots=1000, use_env=0).refill == 1                  # read in one place only
    for other in ("1", "2", "yes", ""):
        monkeypatch.setenv("PTMI_REFILL", other)
        assert plan(shim, **kw).refill == 1
        assert plan(shim, walk=PHASED, slots=1000, use_env=1).refill == 0            # ... and switches nothing on
    big = 192 * 1000 + 1
    monkeypatch.setenv("PTMI_ORDER", "0")
    assert plan(shim, **kw).order_by_cost == 0 and not cost_order(shim, 1, **kw)
    monkeypatch.setenv("PTMI_ORDER", "1")
    p = plan(shim, n_local=big, **kw)
    assert (p.order_by_cost, p.order_classes) == (1, 16) and cost_order(shim, 1, n_local=big, **kw)
    monkeypatch.setenv("PTMI_ORDER", "32")
    p = plan(shim, n_local=big, **kw)
    assert (p.order_by_cost, p.order_classes) == (1, 32) and cost_order(shim, 1, n_local=big, **kw)
    assert not cost_order(shim, 2, n_local=big, **kw)                                # still one chunk, one frame, refill
    monkeypatch.setenv("PTMI_PUBLISH", "1")
    assert plan(shim, **kw).publish == 1
    monkeypatch.setenv("PTMI_PUBLISH", "0")
    assert plan(shim, **kw).publish == 0


def test_next_event_estimation_and_passes(shim):
    for walk in (LANE, PHASED, SWEEP, WIDE):
        p = plan(shim, walk=walk, slots=1000, nee=1, n_local=1 << 18)
        assert (p.refill, p.run_ahead, p.auto_chunks) == (0, 2, 0)
        assert plan(shim, walk=walk, slots=1000, is_pass=1, n_local=1 << 18).auto_chunks == 0
        assert not cost_order(shim, 0, walk=walk, slots=1000, nee=1)
