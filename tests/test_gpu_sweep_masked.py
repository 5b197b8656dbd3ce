"""The sweep walk's two masked moves (csrc/traversal.h: SWEEP_MASKED_HIT in mt_accept_update, SWEEP_MASKED_CURSOR in
intersect_sweep's node pass): closest_t and slot_hit are written under the accept mask, and the cursor takes a missed interior
node's skip address under the mask (interior) & !pass after every lane of the pass took here + 64 - a narrowed EXEC around moves
where the builds before had selects.  A lane outside the mask must keep its value and a lane inside must get the new one, whatever
the other lanes of its wave do, so every comparison here is of bits, with no tolerance: hit, primitive and t per ray against the CPU
oracle and against the LANE walk (which has neither move), radiance, the 8-bit image and the workload counters per frame.

  scenes   tests/sweep_masked_scenes.py: one triangle; a fan pair in one leaf; the same triangle twice in one leaf; five triangles in
           one leaf (a second trip of the four-way leaf loop); two fan pairs whose halves stand in different leaves; a pair whose
           v0 differ only in the sign of a zero; cbox.obj.  Triangles only: a scene with a quad runs the quad builds, which keep
           their selects
  rays     debug_intersect, which stages and walks as the timed build does.  Per scene 2 048 rays of the kind of
           tests/test_gpu_sweep_near_far.py - octants mixed and one per wave, +-0 and denormal components, origins on box planes,
           and here origins with a +-0 component too - and then, wave by wave (64 rays each):
             all    every lane's ray meets the first triangle inside: all 64 lanes accept
             one    lane 37 alone does; the others pass close by on the far side of the edge opposite v0
             none   every lane passes close by: the (a, u) vote passes, no lane accepts
             edge   rays through points of the edge v0 - v2 of the first triangle (the diagonal of a fan pair: both halves may
                    accept, at t that may be equal; the first in leaf order keeps the hit)
           In `twins` every ray that hits meets both records at the same t, bit for bit: the first in leaf order must win.
  frames   64 x 64, 4 spp, max_depth 8: two successive frames with collect_stats off (the builds that take the moves) and on (the
           STATS builds, which do not), a batch of 2 (the BATCH build), against the oracle; then the same through LANE
"""
import functools

import numpy as np
import pytest

import ptmi
import sweep_masked_scenes as S
from oracle_binding import default_camera
from test_gpu_sweep_passes import SPP, assert_frame, bits

pytestmark = pytest.mark.gpu
F = np.float32
W = H = 64
DEPTH = 8
N_CONSTRUCTED = 2048
WAVES = ("all", "one", "none", "edge")
ONE = 37
OCTANTS = np.array([[1.0 if (k >> a) & 1 == 0 else -1.0 for a in range(3)] for k in range(8)])
ZEROS = [((a,), (z,)) for a in range(3) for z in (0.0, -0.0)] + \
        [((a, b), (za, zb)) for a, b in ((0, 1), (0, 2), (1, 2)) for za in (0.0, -0.0) for zb in (0.0, -0.0)]


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


@pytest.fixture
def loaded(R, request):
    """the scene of the test's `name` parameter on the device, walked by the sweep"""
    name = request.node.callspec.params["name"]
    R.load_scene_arrays(*S.arrays(name))
    R.set_camera(ptmi.default_camera())
    assert R.set_traversal(-1) == R.SWEEP
    yield R
    R.set_traversal(-1)
    R.set_config(segments_per_launch=0, collect_stats=False)


def first_triangle(name):
    """(v0, e1, e2) of the record in leaf-order slot 0, float64"""
    o = S.oracle(name)
    v = o.prims()["verts"][o.bvh()["indices"][0]].astype(np.float64)
    return v[0], v[1] - v[0], v[2] - v[0]


@functools.lru_cache(maxsize=None)
def rays(name):
    """(origins, unit directions): N_CONSTRUCTED rays of the constructed kinds, then one wave of 64 per entry of WAVES"""
    arrs = S.arrays(name)
    n_prims = len(arrs[0])
    rng = np.random.default_rng(7000 + n_prims)
    b = S.oracle(name).bvh()
    n = N_CONSTRUCTED
    target = arrs[1][rng.integers(0, n_prims, n)][:, :3].astype(np.float64).mean(axis=1) + rng.normal(0, 0.3, (n, 3))
    d = np.abs(rng.normal(0, 1, (n, 3))) + 0.05
    octant = np.empty(n, np.int64)
    octant[:512] = rng.permuted(np.tile(np.arange(8), (8, 8)), axis=1).ravel()       # mixed: every wave holds each octant 8 times
    octant[512:1536] = np.repeat(np.arange(8), 128)                                  # one octant per wave
    octant[1536:] = rng.integers(0, 8, n - 1536)
    d *= OCTANTS[octant]
    for i in range(1536, 1792):                                                      # signed zeros
        axes, zeros = ZEROS[i % len(ZEROS)]
        d[i, list(axes)] = zeros
    tiny = np.array([1e-40, -1e-40, 3e-39, -4e-45])
    for i in list(range(1792, 1856)) + [1856 + 37]:                                  # a denormal: in every lane, in one lane
        d[i, i % 3] = tiny[i % 4]
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    for i in list(range(1792, 1856)) + [1856 + 37]:                                  # still a denormal after the division
        d[i, i % 3] = tiny[i % 4]
    org = target - d * rng.uniform(1.0, 9.0, (n, 1))
    for i in range(1856, 1920):                                                      # an origin component exactly +0 or -0
        a = i % 3
        if abs(d[i, a]) > 1e-3:
            org[i] -= d[i] * (org[i, a] / d[i, a])                                   # slide along the ray to the plane
        org[i, a] = (0.0, -0.0)[(i // 3) % 2]
    leaves = np.flatnonzero(b["count"] > 0)
    for i in range(1920, 2048):                                                      # origins on a box plane: the root's, a leaf's
        node = 0 if i < 1984 else int(leaves[i % len(leaves)])
        a = i % 3
        lo, hi = b["bmin"][node].astype(np.float64), b["bmax"][node].astype(np.float64)
        org[i] = lo + (hi - lo) * rng.uniform(-0.2, 1.2, 3)
        org[i, a] = (lo, hi)[(i // 3) % 2][a]
        if (i // 6) % 3 < 2:
            d[i, a] = (0.0, -0.0)[(i // 6) % 3]
            d[i] /= np.linalg.norm(d[i])
    # the voting waves, aimed at the first record of the first leaf: v0 + u e1 + v e2
    v0, e1, e2 = first_triangle(name)
    nrm = np.cross(e1, e2); nrm /= np.linalg.norm(nrm)
    u = rng.uniform(0.1, 0.4, (len(WAVES), 64)); v = rng.uniform(0.1, 0.4, (len(WAVES), 64))
    beyond = rng.uniform(0.62, 0.8, 64)                          # u = v = beyond: u + v > 1, past the edge opposite v0
    u[1], v[1] = beyond, beyond
    u[1, ONE], v[1, ONE] = 0.3, 0.3
    u[2], v[2] = beyond, beyond
    u[3], v[3] = 0.0, rng.uniform(0.0, 1.0, 64)                  # on the edge v0 - v2
    for w in range(len(WAVES)):
        p = v0 + u[w][:, None] * e1 + v[w][:, None] * e2
        dw = -nrm * np.where(np.arange(64) % 2 == 0, 1.0, -1.0)[:, None] + rng.normal(0, 0.15, (64, 3))
        dw /= np.linalg.norm(dw, axis=1, keepdims=True)
        org = np.concatenate([org, p - dw * rng.uniform(2.0, 6.0, (64, 1))])
        d = np.concatenate([d, dw])
    return org.astype(F), d.astype(F)


@functools.lru_cache(maxsize=None)
def oracle_hits(name):
    """(hit, prim, t) of rays(name) from the oracle, shared and read-only"""
    org, d = rays(name)
    o = S.oracle(name)
    want = [o.intersect(org[i], d[i]) for i in range(len(org))]
    out = (np.array([h.hit for h in want], np.int32), np.array([h.prim for h in want], np.int32), np.array([h.t for h in want], F))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_frames(name, n):
    """the oracle's first n frames, streams carried over: [(rgb8, radiance, counters)], shared and read-only"""
    state = np.zeros((H * W, 6), np.uint32)
    out = []
    for k in range(n):
        rgb, rad, st = S.oracle(name).render(default_camera(), W, H, SPP, max_depth=DEPTH, rng_state=state, reset_rng=(k == 0))
        rgb.setflags(write=False); rad.setflags(write=False)
        out.append((rgb, rad, (st.samples, st.rays, st.node_visits, st.prim_tests, st.hits)))
    return out


def wave(k):
    return slice(N_CONSTRUCTED + 64 * k, N_CONSTRUCTED + 64 * k + 64)


def test_the_rays_are_what_they_claim():
    for name in S.NAMES:
        org, d = rays(name)
        assert org.shape == d.shape == (N_CONSTRUCTED + 64 * len(WAVES), 3)
        neg = np.signbit(d)
        code = neg[:, 0] + 2 * neg[:, 1] + 4 * neg[:, 2]
        for w in range(8):
            assert np.array_equal(np.bincount(code[64 * w:64 * w + 64], minlength=8), np.full(8, 8)), name
        for w in range(8, 24):
            assert (code[64 * w:64 * w + 64] == (w - 8) // 2).all(), name
        z = d[1536:1792]
        assert ((z == 0).sum(axis=1) >= 1).all() and (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
        den = (d != 0) & (np.abs(d) < np.finfo(F).tiny)
        assert (den[1792:1856].sum(axis=1) == 1).all() and den[1856:1920].sum() == 1
        oz = org[1856:1920]
        assert ((oz == 0).sum(axis=1) >= 1).all() and (np.signbit(oz) & (oz == 0)).any() and (~np.signbit(oz) & (oz == 0)).any()
        assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    # one triangle: the voting waves do what their names say, by the oracle
    hit = oracle_hits("tri1")[0]
    assert hit[wave(0)].all()
    assert hit[wave(1)].sum() == 1 and hit[wave(1)][ONE]
    assert not hit[wave(2)].any()
    # ... and the (a, u) vote of the `none` wave does pass: u of some lane lies in [0, 1]
    org, d = rays("tri1")
    v0, e1, e2 = first_triangle("tri1")
    o64, d64 = org[wave(2)].astype(np.float64), d[wave(2)].astype(np.float64)
    h = np.cross(d64, e2)
    a = h @ e1
    uu = ((o64 - v0) * h).sum(axis=1) / a
    assert ((np.abs(a) > 1e-8) & (uu >= 0) & (uu <= 1)).any()
    # the same triangle twice: whatever hits, hits the record that stands first in the leaf
    hit, prim, _ = oracle_hits("twins")
    first = int(S.oracle("twins").bvh()["indices"][0])
    assert hit.any() and (prim[hit != 0] == first).all()
    # the diagonal of the fan pair: both halves are hit along it
    hit, prim, _ = oracle_hits("pair")
    assert hit[wave(3)].any()
    assert set(prim[hit != 0].tolist()) == {0, 1}


@pytest.mark.parametrize("name", S.NAMES)
def test_rays_match_oracle_and_lane(loaded, name):
    R = loaded
    org, d = rays(name)
    whit, wprim, wt = oracle_hits(name)
    got = R.debug_intersect(org, d)
    bad = np.flatnonzero((got["hit"] != 0) != (whit != 0))
    assert bad.size == 0, f"{name}: hit differs for rays {bad[:8]}"
    on = whit != 0
    assert on.any() and not on.all()
    assert np.array_equal(got["prim"][on], wprim[on]), f"{name}: primitive differs for rays {np.flatnonzero(on)[got['prim'][on] != wprim[on]][:8]}"
    tb = bits(got["t"][on]) != bits(wt[on])
    assert not tb.any(), f"{name}: t differs in bits for rays {np.flatnonzero(on)[tb][:8]}"
    assert R.set_traversal(R.LANE) == R.LANE
    lane = R.debug_intersect(org, d)
    for key in ("hit", "prim"):
        assert np.array_equal(got[key], lane[key]), f"{name}: {key} differs between the sweep and LANE"
    assert np.array_equal(bits(got["t"]), bits(lane["t"])), f"{name}: t differs in bits between the sweep and LANE"


@pytest.mark.parametrize("name", S.NAMES)
def test_frames_match_oracle_and_lane(loaded, name):
    R = loaded
    want = oracle_frames(name, 2)
    assert want[0][2][4] > 0                                 # the camera does see the scene

    def render(what):
        out = []
        for stats in (False, True):
            R.update_resolution(W, H)                        # re-seeds the streams
            R.set_config(spp=SPP, max_depth=DEPTH, segments_per_launch=0, collect_stats=stats, sampling_mode=0)
            for k in range(2):
                st = R.render_frame()
                assert_frame(R, want[k], f"{name} {what} stats {stats} frame {k}", st if stats else None)
                out.append(R.read_image())
        R.update_resolution(W, H)
        R.set_config(spp=SPP, max_depth=DEPTH, segments_per_launch=0, collect_stats=False, sampling_mode=0)
        st = R.render_frames(2)
        assert st.samples == W * H * SPP * 2
        for k in range(2):
            R.select_frame(k)
            assert_frame(R, want[k], f"{name} {what} frame {k} of the batch")
            out.append(R.read_image())
        return out

    swept = render("sweep")
    assert R.set_traversal(R.LANE) == R.LANE
    for k, ((rgb, rad), (lrgb, lrad)) in enumerate(zip(swept, render("LANE"))):
        assert np.array_equal(bits(rad), bits(lrad)) and np.array_equal(rgb, lrgb), f"{name}: LANE and the sweep differ in image {k}"
