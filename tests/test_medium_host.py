"""Host half of the participating medium (include/ptmi.h, "participating medium"): ptmi_check_medium's rejections by message, the
block bit for bit, the restatement's segment and transmittance (tests/medium_oracle.py) against binary64 geometry on an edge set
(tests/medium_edge.py), the phase function and its inversion, the free flight at the ends of a uniform's range, the restatement's
loop with its medium switched off against the pinned per-lane loop, and host/medium.cpp under AddressSanitizer and
UndefinedBehaviorSanitizer through a stand-alone program.  No GPU.

What is under test here: the check, the block and the sanitizer run exercise the LIBRARY (host/medium.cpp through the C ABI) and
fail without it.  Everything else - the segment, the transmittance, the phase function, the free flight, the pinned loop - validates
the RESTATEMENT (tests/medium_oracle.py), which shares no code with csrc/medium.h, against binary64 geometry, statistics and the
pinned per-lane loop; those tests need no library function of this section.  The device code is held to the restatement, bit for
bit, by tests/test_gpu_medium.py, so a restatement that is right is what makes that comparison mean something.

THE SEGMENT'S TOLERANCE, derived as DESIGN.md 4.22 derives the lens's, from the operations alone.  With u = 2^-24, a slab parameter
is fl(fl(lo - o) / d): two roundings, relative error at most (1 + u)^2 - 1 < 2.000001 u.  t0 and t1 are selections (max, min) among
those values, 0 and t_end, and |max(a', b') - max(a, b)| <= max(|a' - a|, |b' - b|), so each differs from its binary64 value by at
most 2.000001 u M, M the largest finite |slab parameter| of the case.  The test holds 3 u M.  The decision t1 > t0 is compared where
the binary64 segment is longer than twice that or empty by more than that; in between either answer is right.
The transmittance exp(-(sigma (t1 - t0))): the difference carries 2 * 3 u M plus its own rounding, the product one more, ptmi_expf
one (it is the rounding of a binary64 value within 1e-16): relative error at most sigma (6 u M + 2 u len) + 2 u; the test holds that."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import medium_edge as ME
import medium_oracle as MO
import ptmi
import test_restatement_pinned as TP
from oracle_binding import default_camera

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U = 2.0 ** -24
CHECK_CASES = 44
Z = 4.75                                  # a two-sided tail of 2e-6 per comparison


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def fog(**kw):
    args = dict(lo=ME.LO, hi=ME.HI, sigma_t=0.75, albedo=(0.25, 0.5, 1.0), g=-0.5)
    args.update(kw)
    return ptmi.make_medium(**args)


# ------------------------------------------------------------------------------------------------
# the check and the block
# ------------------------------------------------------------------------------------------------
def test_check_accepts_the_ends_of_every_range():
    ptmi.check_medium(fog())
    ptmi.check_medium(fog(sigma_t=0.0, g=0.9))
    ptmi.check_medium(fog(sigma_t=3e38, g=-0.9, albedo=(0.0, 1.0, 0.5)))
    d = ptmi.Medium()
    ptmi.lib().ptmi_default_medium(d)
    ptmi.check_medium(d)
    assert d.sigma_t == 0.0 and tuple(d.lo) == (0, 0, 0) and tuple(d.hi) == (1, 1, 1) and tuple(d.albedo) == (1, 1, 1) and d.g == 0.0


def rejections():
    nan, inf = float("nan"), float("inf")
    out = []
    for a, ax in enumerate("xyz"):
        for bad in (nan, inf, -inf):
            lo = list(ME.LO); lo[a] = bad
            hi = list(ME.HI); hi[a] = bad
            out += [(dict(lo=lo), f"medium: lo.{ax} is not finite"), (dict(hi=hi), f"medium: hi.{ax} is not finite")]
        hi = list(ME.HI); hi[a] = ME.LO[a]
        out.append((dict(hi=hi), f"medium: the box is empty: lo.{ax} must be below hi.{ax}"))
        hi = list(ME.HI); hi[a] = ME.LO[a] - 1.0
        out.append((dict(hi=hi), f"medium: the box is empty: lo.{ax} must be below hi.{ax}"))
    for c, ch in enumerate("rgb"):
        for bad, msg in ((nan, "is not finite"), (inf, "is not finite"), (-1e-30, "must lie in [0, 1]"), (1.0000001, "must lie in [0, 1]"), (-2.0, "must lie in [0, 1]")):
            al = [0.25, 0.5, 1.0]; al[c] = bad
            out.append((dict(albedo=al), f"medium: albedo.{ch} {msg}"))
    out += [(dict(sigma_t=nan), "medium: sigma_t is not finite"), (dict(sigma_t=inf), "medium: sigma_t is not finite"),
            (dict(sigma_t=-1e-30), "medium: sigma_t must not be negative"), (dict(sigma_t=-3.0), "medium: sigma_t must not be negative"),
            (dict(g=nan), "medium: g is not finite"), (dict(g=-inf), "medium: g is not finite"),
            (dict(g=0.90000004), "medium: |g| must not exceed 0.9"), (dict(g=-1.0), "medium: |g| must not exceed 0.9"),
            (dict(g=2.0, sigma_t=nan), "medium: sigma_t is not finite")]              # the finiteness of every field comes first
    return out


def test_check_rejects_by_message():
    L = ptmi.lib()
    messages = set()
    for kw, msg in rejections():
        m = fog(**kw)
        assert L.ptmi_check_medium(m) == -1, kw
        assert L.ptmi_last_error().decode() == msg, (kw, L.ptmi_last_error())
        out = np.full(12, -7.0, F)
        assert L.ptmi_host_medium_block(m, out.ctypes.data) == -1 and (out == -7.0).all(), kw
        messages.add(msg)
    assert len(messages) == 5 * 3 + 4                              # lo, hi, box, albedo finite, albedo range per axis or channel; sigma_t x 2, g x 2
    assert L.ptmi_check_medium(None) == -1 and L.ptmi_host_medium_block(fog(), None) == -1


def test_block_bit_for_bit():
    for kw in (dict(), dict(g=0.9, sigma_t=1e-30), dict(albedo=0.5), dict(lo=(-1e30, -0.0, 1e-40), hi=(1e30, 1e-45, 1.0))):
        m = fog(**kw)
        got = ptmi.host_medium_block(m)
        want = MO.medium_block(tuple(m.lo), tuple(m.hi), m.sigma_t, tuple(m.albedo), m.g)
        assert np.array_equal(bits(got), bits(want)), kw
        flat = np.array(list(m.lo) + [m.sigma_t] + list(m.hi) + [m.g] + list(m.albedo) + [0.0], F)
        assert np.array_equal(bits(got.reshape(12)), bits(flat)), kw
        assert np.array_equal(bits(ME.block(m.sigma_t, m.g, tuple(m.albedo), tuple(m.lo), tuple(m.hi))), bits(got))


# ------------------------------------------------------------------------------------------------
# the segment and the transmittance against binary64 geometry
# ------------------------------------------------------------------------------------------------
def slab_scale(lo, hi, o, d):
    """M: the largest finite |slab parameter| of the case, binary64"""
    m = 0.0
    for a in range(3):
        if d[a] != 0:
            for p in (lo[a], hi[a]):
                t = abs((float(p) - float(o[a])) / float(d[a]))
                if np.isfinite(t):
                    m = max(m, t)
    return m


def check_segment(blk, o, d, t_end, expect=None, name=""):
    o, d = np.asarray(o, F), np.asarray(d, F)
    lo, hi, sigma = blk[0, :3], blk[1, :3], float(blk[0, 3])
    ok, t0, t1 = MO.segment(blk, o, d, t_end)
    e0, e1 = MO.segment64(lo, hi, o, d, t_end)
    big = [a for a in range(3) if d[a] != 0 and not np.isfinite((float(lo[a]) - float(o[a])) / float(d[a]))]
    M = slab_scale(lo, hi, o, d)
    tol = 3 * U * M
    length = e1 - e0
    if expect is not None:
        assert ok == expect, name
    if not big:
        if length > 2 * tol:
            assert ok, (name, t0, t1, e0, e1)
            assert abs(float(t0) - e0) <= tol and (abs(float(t1) - e1) <= tol or (np.isinf(e1) and np.isinf(t1))), (name, t0, t1, e0, e1, tol)
        elif length < -2 * tol or e1 == e0 == 0.0 and not expect:
            assert not ok, (name, t0, t1, e0, e1)
    T = MO.transmittance(blk, o, d, t_end)
    if not ok:
        assert bits(T) == bits(F(1.0)), name
        return ok
    with np.errstate(all="ignore"):
        want = np.exp(-sigma * max(length, 0.0))
        bound = want * (sigma * (6 * U * M + 2 * U * abs(length)) + 2 * U) + 2.0 ** -150
    assert abs(float(T) - want) <= bound, (name, T, want, bound)
    assert 0.0 <= T <= 1.0
    return ok


@pytest.mark.parametrize("sigma", ME.SIGMAS)
def test_segment_on_the_edge_set(sigma):
    blk = ME.block(sigma)
    seen = set()
    for name, o, d, t_end, expect in ME.SEGMENTS:
        seen.add(check_segment(blk, o, d, t_end, expect, name))
    assert seen == {True, False}


def test_segment_on_random_rays():
    n_ok = 0
    for blk, o, d, t_end, _ in ME.random_cases(4096):
        n_ok += check_segment(blk, o, d, t_end)
    assert 1000 < n_ok < 4000                                        # both answers are well represented


def test_an_empty_segment_transmits_exactly_1_and_a_long_one_0():
    blk = ME.block(40.0)
    assert bits(MO.transmittance(blk, np.array([-5, 1, 5], F), np.array([1, 0, 0], F), np.inf)) == bits(F(1.0))
    assert MO.transmittance(blk, np.array([-5, 1, 0], F), np.array([1, 0, 0], F), np.inf) == 0.0        # exp(-120) < 2^-150
    huge = ME.block(1.0, lo=(-3e38, 0, -3), hi=(3e38, 4, 1))
    assert MO.transmittance(huge, np.array([0, 1, 0], F), np.array([1, 0, 0], F), np.inf) == 0.0


# ------------------------------------------------------------------------------------------------
# the phase function
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", ME.G_VALUES)
def test_hg_integrates_to_1(g):
    """Gauss-Legendre with 512 nodes over the cosine: the integrand is analytic with its pole at (1 + g^2) / (2 g), |.| >= 1.0055,
    so the rule's error is below 1e-40; what is left is the rounding of each value to float, at most 2^-24 relative, and the
    restatement's own binary64 arithmetic, a few 1e-16.  The bound is twice the former."""
    x, w = np.polynomial.legendre.leggauss(512)
    xf = x.astype(F)
    vals = np.array([MO.hg(g, c) for c in xf], np.float64)
    assert vals.dtype == np.float64 and (vals > 0).all()
    # the nodes were rounded to float: integrate the float-evaluated function at the float nodes against binary64 at the same nodes
    exact = MO.hg_pdf64(float(F(g)), xf.astype(np.float64))
    assert np.abs(vals / exact - 1.0).max() <= 2.0 ** -24 * 1.01
    assert abs(2.0 * np.pi * np.dot(w, MO.hg_pdf64(float(F(g)), x)) - 1.0) < 1e-12
    assert abs(2.0 * np.pi * np.dot(w, vals * MO.hg_pdf64(float(F(g)), x) / exact) - 1.0) <= 2.0 ** -23


@pytest.mark.parametrize("g", ME.G_VALUES)
def test_hg_sampling_follows_the_density(g):
    n, nbins = 200000, 20
    u = ME.curand_uniforms(np.random.default_rng(17), n)
    c = MO.hg_cosine(g, u)
    assert c.dtype == F and (np.abs(c) <= 1.0).all()
    gf = float(F(g))
    edges = np.linspace(-1.0, 1.0, nbins + 1)
    expected = n * np.diff(MO.hg_cdf64(gf, edges))
    assert expected.min() >= 5 and abs(expected.sum() - n) < 1e-6 * n
    counts, _ = np.histogram(c.astype(np.float64), edges)
    chi2 = ((counts - expected) ** 2 / expected).sum()
    k = nbins - 1
    bound = k * (1.0 - 2.0 / (9.0 * k) + Z * np.sqrt(2.0 / (9.0 * k))) ** 3          # Wilson-Hilferty quantile at z
    assert chi2 <= bound, (chi2, bound)
    var = (1.0 + 2.0 * gf * gf) / 3.0 - gf * gf                                   # E[c^2] of Henyey-Greenstein is (1 + 2 g^2) / 3
    assert abs(c.astype(np.float64).mean() - gf) <= Z * np.sqrt(var / n), (c.mean(), gf)
    # the density of the sampled cosine is what the value function returns: pb_prev of the next vertex
    some = c[:64]
    assert np.allclose([MO.hg(g, x) for x in some], MO.hg_pdf64(gf, some.astype(np.float64)), rtol=2e-7, atol=0)


def test_hg_at_the_ends_of_a_uniform_s_range():
    for g in ME.G_VALUES + (0.5, -0.5, 1e-30, -1e-30, float(F(0.9)), float(-F(0.9))):
        cs = [MO.hg_cosine(g, F(u)) for u in ME.EDGE_U]
        assert all(np.isfinite(c) and -1.0 <= c <= 1.0 and c.dtype == F for c in cs), (g, cs)
        assert cs[0] < cs[1] < cs[2] or g == 0 and cs[0] > cs[1] > cs[2], (g, cs)    # g = 0 takes 1 - 2 u
        assert cs[2] == (1.0 if g != 0 else -1.0)
        if abs(g) > 1e-20:
            assert abs(float(cs[0]) + 1.0) < 1e-6                                  # u = 2^-33: the backward end
        for c in (-1.0, 1.0, 2.0, -2.0, 0.0) + tuple(cs):
            v = MO.hg(g, F(c))
            assert np.isfinite(v) and v > 0, (g, c)
        assert MO.hg(g, F(2.0)) == MO.hg(g, F(1.0)) and MO.hg(g, F(-2.0)) == MO.hg(g, F(-1.0))     # the clamp
    assert bits(MO.hg(0.0, F(0.3))) == bits(F(1.0 / (4.0 * np.pi)))
    assert bits(MO.hg_cosine(0.0, F(0.25))) == bits(F(0.5))


def test_scattered_direction_is_a_unit_vector_at_the_sampled_cosine():
    rng = np.random.default_rng(3)
    for i in range(256):
        d = rng.normal(size=3)
        d = (d / np.linalg.norm(d)).astype(F)
        if i == 0:
            d = np.array([0, 0, -1], F)                                             # the frame's other branch
        c = MO.hg_cosine(float(rng.choice(ME.G_VALUES)), ME.curand_uniforms(rng, 1)[0])
        nd = MO.hg_direction(d, c, ME.curand_uniforms(rng, 1)[0])
        assert nd.dtype == F and abs(np.linalg.norm(nd.astype(np.float64)) - 1.0) < 3e-7
        assert abs(float(np.dot(nd.astype(np.float64), d.astype(np.float64))) - float(c)) < 1e-6


# ------------------------------------------------------------------------------------------------
# the free flight at the ends of a uniform's range
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", ME.SIGMAS)
def test_free_flight_at_the_ends_of_a_uniform_s_range(sigma):
    s1 = MO.flight(sigma, F(1.0))
    assert s1 == 0.0                                                               # -log 1 / sigma: the vertex at the entry
    s0 = MO.flight(sigma, F(ME.TINY))
    want = 33.0 * np.log(2.0) / float(F(sigma))
    assert np.isfinite(s0) and abs(float(s0) - want) <= 2.5 * U * want             # the rounding to float, the negation, the quotient
    blk = ME.block(sigma)
    for name, o, d, t_end, expect in ME.SEGMENTS:
        o, d = np.asarray(o, F), np.asarray(d, F)
        ok, t0, t1 = MO.segment(blk, o, d, t_end)
        v1, tm1 = MO.free_flight(blk, o, d, t_end, F(1.0))
        assert v1 == ok and bits(tm1) == bits(F(t0 + F(0.0))), name                # every ray that meets the medium scatters at once
        v0, tm0 = MO.free_flight(blk, o, d, t_end, F(ME.TINY))
        assert v0 == (ok and F(t0 + s0) < t1) and np.isfinite(tm0), name
        if v0:
            x = (o + (tm0 * d).astype(F)).astype(F)
            assert ((x >= blk[0, :3] - 1e-4) & (x <= blk[1, :3] + 1e-4)).all(), (name, x)
    assert not MO.free_flight(ME.block(0.05), np.array([0, 1, 0], F), np.array([1, 0, 0], F), np.inf, F(ME.TINY))[0]    # 457 units: out of the box
    assert MO.free_flight(ME.block(40.0), np.array([0, 1, 0], F), np.array([1, 0, 0], F), np.inf, F(ME.TINY))[0]


# ------------------------------------------------------------------------------------------------
# the second copy of the loop, pinned: medium off inside, it is PathRenderer's
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pinned():
    with np.load(TP.FIXTURE) as z:
        return {k: z[k] for k in z.files}


# plain and NEE (plain, both values of next_event), env (zero_map, soup_dark-sky), mirror plus glass, rough (blocks, quads, soup,
# furnace), and the two cases that reach the NaN and the tie exits
PIN_CASES = ["plain", "zero_map", "soup_dark-sky", "mirror_glass-sky", "mirror_glass-dark", "blocks-sky-d8", "blocks-dark-d3", "blocks-sky-d1",
             "quads", "soup", "furnace", "zero_normals", "roulette_tie"]


@pytest.mark.parametrize("next_event", [False, True])
@pytest.mark.parametrize("case", PIN_CASES)
def test_the_loop_with_its_medium_off_is_the_pinned_loop(pinned, case, next_event):
    o, kind, rough, env, depth, prm = TP.build(case)
    off = (ME.LO, ME.HI, 0.0, (1.0, 1.0, 1.0), 0.0) if next_event else None        # sigma_t 0 and None are both "no medium"
    r = MO.MediumRenderer(o, default_camera(), TP.W, TP.H, kind, None, rough, env, next_event, medium=off, **prm)
    assert r.medium is None
    r.trace = []
    got = {f"sums{k}": r.sums(TP.SPP, depth) for k in range(TP.FRAMES)}
    got["rng"] = r.rng.copy()
    got["counts"] = np.array([r.samples, r.draws, r.cut], np.int64)
    got["trace"] = np.array(r.trace, np.uint8).reshape(-1, 3)
    prefix = TP.key(case, next_event, "RoughRenderer") + "/"
    assert {k[len(prefix):] for k in pinned if k.startswith(prefix)} == set(got)
    for k, a in got.items():
        e = pinned[prefix + k]
        assert a.dtype == e.dtype and a.shape == e.shape, k
        if a.dtype == F:
            a, e = a.view(np.uint32), e.view(np.uint32)
        assert np.array_equal(a, e), (k, int((a != e).sum()))


def test_the_loop_with_a_medium_differs_and_draws_once_per_path_ray():
    o, kind, rough, env, depth, prm = TP.build("plain")
    cam = default_camera()
    base = MO.MediumRenderer(o, cam, TP.W, TP.H, next_event=True)
    base.trace = []
    a = base.sums(2, 5)
    # a box no ray meets: the draws alone - one more per path ray - and nothing else
    far = MO.MediumRenderer(o, cam, TP.W, TP.H, next_event=True, medium=((100, 100, 100), (101, 101, 101), 1.0, 1.0, 0.0))
    far.trace = []
    b = far.sums(2, 5)
    assert far.draws > base.draws and not any(t[0] == MO.MEDIUM for t in far.trace)
    assert not np.array_equal(bits(a), bits(b))                                    # other draws, another image
    fog_ = MO.MediumRenderer(o, cam, TP.W, TP.H, next_event=True, medium=((-10, -10, -10), (10, 10, 10), 0.2, (0.9, 0.8, 0.7), 0.6))
    fog_.trace = []
    c = fog_.sums(2, 5)
    assert any(t[0] == MO.MEDIUM for t in fog_.trace) and np.isfinite(c).all() and c.max() > 0


# ------------------------------------------------------------------------------------------------
# host/medium.cpp under the sanitizers, through a stand-alone program
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found (the build needs it too)")
    exe = str(tmp_path_factory.mktemp("medium") / "medium_check")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                    "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(HERE, "medium_check.cpp"), os.path.join(ROOT, "cuda-pathtracer_amd", "host", "medium.cpp"), "-o", exe],
                   check=True, timeout=300)
    return exe


def test_the_check_and_the_block_under_the_sanitizers(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[-2].startswith("ok ") and int(lines[-2].split()[1]) == CHECK_CASES and not any(ln.startswith("FAILED") for ln in lines), r.stdout[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
