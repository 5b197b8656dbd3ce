"""Host half of the thin lens (include/ptmi.h, "thin lens"): ptmi_check_lens's and ptmi_host_lens_block's rejections, the block bit
for bit against the restatement (tests/lens_oracle.py), the restatement against binary64 geometry, the disc map at the edges of its
inputs, the mixin's frame against the spelled-out ray, the focus distance of a pixel on a plane at a known depth, and
host/lens.cpp under AddressSanitizer and UndefinedBehaviorSanitizer through a stand-alone program.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import lens_oracle as LO
import ptmi
from gpu_frames import ocam
from oracle_binding import camera_ray

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = 33, 19
# The restatement's lens ray against binary64 geometry on this file's own inputs (test_restatement_against_binary64 prints them):
# the largest distance of the binary64 focal-plane point from the ray, relative to its distance from the ray's origin, over
# f = 0.5, 10, 1000 (2.84e-7, 1.27e-7, 9.3e-8).  The test holds four times this.
MEASURED = 2.9e-7
CHECK_CASES = 49


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def curand_uniforms(rng, shape):
    x = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(F)
    return (x * F(2.3283064e-10) + F(2.3283064e-10 / 2.0)).astype(F)


def cameras():
    default = ptmi.default_camera()
    orbit = ptmi.default_camera(); orbit.yaw_deg, orbit.pitch_deg, orbit.vfov_deg = 60.0, 25.0, 55.0
    fixed = ptmi.default_camera(); fixed.orbit = 0; fixed.origin[:] = (1.0, 2.0, 3.0); fixed.lookat[:] = (-4.0, 0.5, -2.0)
    return dict(default=default, orbit=orbit, fixed=fixed)


# ------------------------------------------------------------------------------------------------
# the check
# ------------------------------------------------------------------------------------------------
def test_check_accepts_the_ends_of_both_ranges():
    ptmi.check_lens(0.0, 1.0)
    ptmi.check_lens(0.0, np.finfo(F).max)                      # no lens, no block: any focus distance that is a distance
    ptmi.check_lens(0.0, np.finfo(F).tiny)
    ptmi.check_lens(1e30, 1e30)
    ptmi.check_lens(1e-30, 1e-30)


def test_check_rejects_by_message():
    L = ptmi.lib()
    nan, inf = float("nan"), float("inf")
    for r, f, msg in ((nan, 1.0, b"lens: radius is a NaN"), (1.0, nan, b"lens: focus_distance is a NaN"), (0.0, nan, b"lens: focus_distance is a NaN"),
                      (inf, 1.0, b"lens: radius must be finite"), (-inf, 1.0, b"lens: radius must be finite"),
                      (1.0, inf, b"lens: focus_distance must be finite"), (1.0, -inf, b"lens: focus_distance must be finite"),
                      (-1e-30, 1.0, b"lens: radius must not be negative"), (-2.0, 1.0, b"lens: radius must not be negative"),
                      (1.0, 0.0, b"lens: focus_distance must be positive"), (0.0, 0.0, b"lens: focus_distance must be positive"),
                      (1.0, -3.0, b"lens: focus_distance must be positive"),
                      (3e38, 1.0, b"lens: the lens block is not finite (record 4")):       # R / length(hor) overflows: |hor| < 1 there
        assert L.ptmi_check_lens(r, f) == -1, (r, f)
        assert msg in L.ptmi_last_error(), (r, f, L.ptmi_last_error())
    # the overflow case: f so large that f * hor is infinite.  A camera-free check cannot know hor; over a wide camera it does
    wide = ptmi.default_camera(); wide.vfov_deg = 170.0
    out = np.full(24, -7.0, F)
    assert L.ptmi_host_lens_block(C.byref(wide), 8, 8, 0.1, 2e37, out.ctypes.data) == -1      # f * hw is finite, f * 2 hw is not
    assert b"lens: the lens block is not finite (record 1, component 0)" in L.ptmi_last_error()
    assert (out == -7.0).all()
    for bad, msg in (((0, 8, 0.1, 1.0), b"width and height must be positive"), ((8, -1, 0.1, 1.0), b"width and height must be positive"),
                     ((8, 8, 0.0, 1.0), b"radius 0 is the pinhole"), ((8, 8, 0.1, 0.0), b"focus_distance must be positive"),
                     ((8, 8, float("nan"), 1.0), b"radius is a NaN")):
        assert L.ptmi_host_lens_block(C.byref(wide), *bad, out.ctypes.data) == -1 and msg in L.ptmi_last_error(), bad
    assert L.ptmi_host_lens_block(None, 8, 8, 0.1, 1.0, out.ctypes.data) == -1 and b"NULL" in L.ptmi_last_error()
    assert L.ptmi_host_lens_block(C.byref(wide), 8, 8, 0.1, 1.0, None) == -1 and b"NULL" in L.ptmi_last_error()
    assert (out == -7.0).all()
    with pytest.raises(ptmi.PtmiError, match="focus_distance must be positive"):
        ptmi.check_lens(0.5, -1.0)


# ------------------------------------------------------------------------------------------------
# the block
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "orbit", "fixed"])
@pytest.mark.parametrize("size", [(W, H), (64, 64), (5, 40), ((1 << 23) + 1, 2)])
def test_block_equals_the_restatement(name, size):
    cam = cameras()[name]
    w, h = size
    frame = LO.frame_of(ocam(cam), w, h)
    assert np.array_equal(bits(frame), bits(ptmi.host_camera_frame(cam, w, h)))
    for radius, focus in ((0.05, 3.0), (1.0, 8.5), (0.3, 1e3), (1e-6, 0.5)):
        got = ptmi.host_lens_block(cam, w, h, radius, focus)
        assert np.array_equal(bits(got), bits(LO.lens_block(frame, w, h, radius, focus))), (radius, focus)
        assert got[0, 3] == w and got[2, 3] == h and (got[4:, 3] == 0).all()
        assert (got[1, 3] == 0 and got[3, 3] == 0) if w > (1 << 23) else (got[1, 3] == F(1) / F(w) and got[3, 3] == F(1) / F(h))
        # a and b have the radius's length and the directions of hor and ver
        a, b = got[4, :3].astype(np.float64), got[5, :3].astype(np.float64)
        assert abs(np.linalg.norm(a) / radius - 1) < 1e-6 and abs(np.linalg.norm(b) / radius - 1) < 1e-6
        assert abs(np.dot(a, b)) < 1e-6 * radius * radius


# ------------------------------------------------------------------------------------------------
# the restatement against binary64 geometry, and at the edges of the disc map's inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("focus", [0.5, 10.0, 1e3])
def test_restatement_against_binary64(focus):
    radius = 0.3
    cam = ptmi.default_camera()
    frame = LO.frame_of(ocam(cam), W, H)
    block = LO.lens_block(frame, W, H, radius, focus)
    org, llc, hor, ver = (frame.astype(np.float64).reshape(4, 3)[i] for i in range(4))
    rng = np.random.default_rng(5)
    n = 10000
    r = curand_uniforms(rng, (n, 4)); px = rng.integers(0, W, n); py = rng.integers(0, H, n)
    worst = off = 0.0
    for i in range(n):
        o, d = LO.lens_ray(block, px[i], py[i], *r[i])
        u = F(F(F(px[i]) + r[i, 2]) / F(W)); v = F(F(F(py[i]) + r[i, 3]) / F(H))
        P = org + float(F(focus)) * (llc + float(u) * hor + float(v) * ver - org)      # the focal-plane point of (u, v)
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        w = P - o64
        worst = max(worst, np.linalg.norm(w - np.dot(w, d64) * d64 / np.dot(d64, d64)) / np.linalg.norm(w))
        off = max(off, np.linalg.norm(o64 - org))
    print("focus %g: relative distance of the focal-plane point from the ray %.3g, |o - org| / R - 1 = %.3g" % (focus, worst, off / radius - 1))
    assert worst <= 4 * MEASURED
    assert off <= radius * (1 + 2.0 ** -22)


def test_disc_map_at_the_edges_of_its_inputs():
    tiny = F(2.0 ** -33)
    for r3 in (tiny, F(1.0)):
        for r4 in (tiny, F(0.25), F(0.5), F(1.0)):
            dx, dy = LO.disc(r3, r4)
            assert np.isfinite(dx) and np.isfinite(dy)
            assert float(dx) ** 2 + float(dy) ** 2 <= 1 + 2.0 ** -22, (r3, r4)
    dx, dy = LO.disc(F(1.0), F(0.25))
    assert dy == 1 and abs(dx) < 1e-7                          # a quarter turn: the top of the rim
    dx, dy = LO.disc(F(1.0), F(0.5))
    assert dx == -1 and abs(dy) < 1e-7
    dx, dy = LO.disc(tiny, F(1.0))
    assert abs(dx - 2.0 ** -16.5) < 1e-11 and abs(dy) < 1e-11


def test_the_mixin_s_frame_gives_the_spelled_out_ray():
    """LensMixin hands the sensor's get_ray (the oracle's po_camera_ray) the per-sample frame; lens_ray spells every operation out"""
    cam = cameras()["orbit"]
    block = LO.lens_block(LO.frame_of(ocam(cam), W, H), W, H, 0.7, 4.0)
    rng = np.random.default_rng(9)
    r = curand_uniforms(rng, (500, 4))
    for i in range(500):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        o, d = LO.lens_ray(block, x, y, *r[i])
        u = F(F(F(x) + r[i, 2]) / F(W)); v = F(F(F(y) + r[i, 3]) / F(H))
        o2, d2 = camera_ray(LO.sample_frame(block, LO.lens_origin(block, r[i, 0], r[i, 1])), u, v)
        assert np.array_equal(bits(o), bits(o2)) and np.array_equal(bits(d), bits(d2)), i


# ------------------------------------------------------------------------------------------------
# the focus distance of a pixel
# ------------------------------------------------------------------------------------------------
def test_focus_distance_of_a_plane_at_a_known_depth():
    depth = 7.25
    verts = np.zeros((2, 4, 3), F)
    verts[0, :3] = [(-50, -50, -depth), (50, -50, -depth), (50, 50, -depth)]
    verts[1, :3] = [(-50, -50, -depth), (50, 50, -depth), (-50, 50, -depth)]
    hs = ptmi.HostScene.from_arrays(np.zeros(2, np.int32), verts, np.tile(np.array([0, 0, 1], F), (2, 1)), np.full((2, 3), 0.5, F), np.zeros((2, 3), F))
    hs.fast_tree_build()
    cam = ptmi.default_camera()
    cam.orbit = 0; cam.origin[:] = (0, 0, 0); cam.lookat[:] = (0, 0, -1); cam.vfov_deg = 60.0
    frame = ptmi.host_camera_frame(cam, W, H)
    for px, py in ((0, 0), (W - 1, H - 1), (W // 2, H // 2), (3, 17)):
        o, d = ptmi.pinhole_centre_ray(frame, W, H, px, py)
        hit = hs.fast_tree_intersect(o[None], d[None])
        assert hit["prim"][0] >= 0
        f = ptmi.depth_along_axis(frame, d, hit["t"][0])
        assert abs(f - depth) <= 4e-6 * depth, (px, py, f)      # t and d are binary32: a few 2^-24 of the depth
        if (px, py) != (W // 2, H // 2):
            assert hit["t"][0] > depth                          # the distance along the ray is longer than the depth
    assert ptmi.default_focus_distance(ptmi.default_camera()) == float(F(np.sqrt(F(F(F(0.25) + F(0.25)) + F(72.25)))))


# ------------------------------------------------------------------------------------------------
# host/lens.cpp under the sanitizers, through a stand-alone program
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found (the build needs it too)")
    exe = str(tmp_path_factory.mktemp("lens") / "lens_check")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                    "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(HERE, "lens_check.cpp"), os.path.join(ROOT, "cuda-pathtracer_amd", "host", "lens.cpp"), "-o", exe],
                   check=True, timeout=300)
    return exe


def test_the_check_and_the_block_under_the_sanitizers(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[-2].startswith("ok ") and int(lines[-2].split()[1]) == CHECK_CASES and not any(ln.startswith("FAILED") for ln in lines), r.stdout[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------
# the blurred edge of tests/test_gpu_lens_expectation.py, on the restatement alone: 32 x 8 at 256 spp
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z0", [5.0, 20.0])
def test_restatement_reaches_the_blurred_edge(z0):
    """The analytic columns of tests/lens_edge.py against the restatement, before any kernel is asked: a mistake in the formula or
    in the contract shows here.  Measured: column |z| max 2.37 (z0 = 5) and 3.91 (z0 = 20); three other seeds at 1024 spp: 0.5 to 2.4."""
    import lens_edge as LE
    from oracle_binding import OracleScene
    w, h, spp = 32, 8, 256
    ref = LO.LensRenderer(OracleScene.from_arrays(*LE.scene(z0)), ocam(LE.camera()), w, h, radius=LE.RADIUS, focus_distance=LE.FOCUS)
    _, rad = ref.frame(spp, 1)
    prob = LE.check_edge("restatement z0 %g" % z0, rad, z0, spp)
    pin = LE.column_probability(w, h, z0, radius=0.0)
    assert (np.abs(prob - pin) > 0.05).sum() >= 2              # a column is 0.91 wide on the focal plane: the blur reaches 1 and 0.5
