"""The sweep's leaf-only walk (csrc/sweep_leaves.h, csrc/traversal.h: sweep_leaves_walk): a wave whose rays all take ray_inv's short
form slab-tests the leaf boxes alone, in pre-order, and runs a leaf's primitives under the lanes that pass; a wave whose vote fails
walks every node as before.  The claim is that both enter the leaves the reference enters, with the same closest_t - so every
comparison here is of bits, with no tolerance: hit, primitive and t per ray against the CPU oracle and against the LANE walk,
radiance, the 8-bit image and (collect_stats) the reference's counters per frame.

  scenes   tri1 (the root is the only leaf), tri3, tri64, cbox of tests/test_gpu_sweep_passes.py;
           sheets: ten large parallel triangles, two or three per leaf, laid out so that the tree's order is not the order along
             any ray: the five high sheets have their centroids at x = -1.5 and stand first in pre-order, the five low ones at
             x = +1.5.  A ray going down meets the first group nearest first and finds the whole second group behind its hit; a ray
             going up meets the second group's leaves nearest first.  Either way a later leaf's box is entered by the ray but lies
             beyond closest_t: pruned by closest_t alone, which the interior tests never see;
           chain: 18 triangles along x at 1, 2, 4, ... 2^17, so that the midpoint split peels one leaf per level: depth >= 12;
           ties: ten overlapping triangles in one plane, met by rays whose arithmetic is exact, so that every triangle under a
             ray gives the same t, bit for bit, and the hit is the one of the leaf visited FIRST - the one place where the order
             of the leaves, and not only the set entered, decides a result
  rays     debug_intersect, which stages and walks as the timed build does, on 32 waves of 64 rays per scene:
             waves  0 -  3  all eight sign octants mixed, lane by lane;
             waves  4 - 19  one octant each, two per octant;
             waves 20 - 21  one or two components exactly +0 or -0, all 18 patterns in each wave (the wave walks every node);
             wave  22       a denormal component in every lane; wave 23: in ONE lane - the whole wave takes the cold side;
             waves 24 - 25  the origin on a plane of the root's box and of a leaf's, the direction's component along that axis
                            +0, -0 or not zero;
             wave  26       an origin component +inf in one lane and -inf in another; wave 27: NaN in one lane; wave 28: 2^101 in
                            one lane; waves 29 - 31: the same three in every lane (both signs) - the vote does not look at the
                            origin, so these waves stay on the hot side
  frames   cbox and tri3 at 72x56 and 70x50 (3 500 pixels: a ragged last workgroup with a partial wave), 4 spp, max_depth 8: two
           successive frames and a batch of 3 against the oracle with collect_stats off (the builds that take the form) and on
           (they keep the full walk: node_visits stay the oracle's), then the same frames through LANE against the sweep's

For the sheets the oracle must really prune a leaf by closest_t for at least one ray of each wave; that is asserted for waves 0 - 28.
Waves 29 - 31 hold a non-finite or 2^101 origin component in every lane: no ray of theirs can meet the scene, so none can prune.
"""
import functools

import numpy as np
import pytest

import ptmi
from oracle_binding import OracleScene
from test_gpu_sweep_passes import SIZES, SPP, assert_frame, bits, cameras, oracle_frames
from test_gpu_sweep_passes import scene as passes_scene

pytestmark = pytest.mark.gpu
F = np.float32
RAY_SCENES = ["tri1", "tri3", "tri64", "cbox", "sheets", "chain"]
FRAME_SCENES = ["cbox", "tri3"]
DEPTH = 8
OCTANTS = np.array([[1.0 if (k >> a) & 1 == 0 else -1.0 for a in range(3)] for k in range(8)])
ZEROS = [((a,), (z,)) for a in range(3) for z in (0.0, -0.0)] + \
        [((a, b), (za, zb)) for a, b in ((0, 1), (0, 2), (1, 2)) for za in (0.0, -0.0) for zb in (0.0, -0.0)]
BIG = 2.0 ** 101
HOT_WAVES = list(range(20)) + list(range(26, 32))        # every live lane has its three components in [2^-100, 2^100]


def triangles(verts):
    n = len(verts)
    v = np.zeros((n, 4, 3), F)
    v[:, :3] = verts
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    normal = np.cross(e1.astype(np.float64), e2.astype(np.float64))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    Le = np.zeros((n, 3), F); Le[0] = 3.0
    return np.zeros(n, np.int32), v, normal.astype(F), np.full((n, 3), 0.6, F), Le


@functools.lru_cache(maxsize=None)
def scene(name):
    """(arrays, oracle scene, camera fields, sweep_max_prims), as tests/test_gpu_sweep_passes.py: scene"""
    if name == "sheets":
        z = np.array([1.0, 1.2, 1.4, 1.6, 1.8, 0.0, 0.2, 0.4, 0.6, 0.8])
        cx = np.where(np.arange(10) < 5, -1.5, 1.5)
        corners = np.array([[-9.0, -6.0], [9.0, -6.0], [0.0, 12.0]])             # centroid (0, 0)
        verts = np.zeros((10, 3, 3))
        verts[:, :, :2] = corners[None]
        verts[:, :, 0] += cx[:, None]
        verts[:, :, 2] = z[:, None]
        arrs = triangles(verts)
    elif name == "chain":
        x = 2.0 ** np.arange(18)
        verts = np.zeros((18, 3, 3))
        verts[:, 0] = np.stack([x, -0.4 * x, -0.3 * x], axis=1)
        verts[:, 1] = np.stack([x, 0.5 * x, -0.2 * x], axis=1)
        verts[:, 2] = np.stack([x, -0.1 * x, 0.5 * x], axis=1)
        arrs = triangles(verts)
    elif name == "ties":
        k = np.arange(5.0)
        a = np.stack([np.stack([0 * k, k, 0 * k], 1), np.stack([0 * k + 8, k, 0 * k], 1), np.stack([0 * k, k + 8, 0 * k], 1)], 1)
        b = np.stack([np.stack([0 * k + 8, k, 0 * k], 1), np.stack([0 * k + 8, k + 8, 0 * k], 1), np.stack([0 * k, k + 8, 0 * k], 1)], 1)
        arrs = triangles(np.concatenate([a, b]))
    else:
        return passes_scene(name)
    return arrs, OracleScene.from_arrays(*arrs), None, 64


def tree(name):
    """the builder's tree: (bvh arrays, pre-order leaf indices, depth of the tree in levels)"""
    b = ptmi.HostScene.from_arrays(*scene(name)[0]).bvh()
    depth = np.zeros(len(b["left"]), np.int64)
    for i in range(len(depth)):
        if b["count"][i] == 0:
            depth[b["left"][i]] = depth[b["right"][i]] = depth[i] + 1
    return b, np.flatnonzero(b["count"] > 0), int(depth.max()) + 1


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


@pytest.fixture
def loaded(R, request):
    """the scene of the test's `name` parameter on the device, walked by the sweep"""
    name = request.node.callspec.params["name"]
    arrs, _, cam, max_prims = scene(name)
    R.load_scene_arrays(*arrs)
    R.set_camera(cameras(cam)[1])
    assert R.set_traversal(-1, sweep_max_prims=max_prims) == R.SWEEP
    yield R
    R.set_traversal(-1)
    R.set_camera(ptmi.default_camera())
    R.set_config(segments_per_launch=0, collect_stats=False)


@functools.lru_cache(maxsize=None)
def rays(name):
    """(origins, unit directions) of 32 waves of 64; read-only"""
    arrs = scene(name)[0]
    rng = np.random.default_rng(2000 + len(arrs[0]))
    b, leaves, _ = tree(name)
    n = 32 * 64
    tri = arrs[1][rng.integers(0, len(arrs[0]), n)][:, :3]
    size = np.linalg.norm(tri[:, 1] - tri[:, 0], axis=1, keepdims=True)
    target = tri.mean(axis=1) + rng.normal(0, 0.3, (n, 3)) * np.minimum(size, 1.0)
    d = np.abs(rng.normal(0, 1, (n, 3))) + 0.05
    octant = np.empty(n, np.int64)
    octant[:256] = rng.permuted(np.tile(np.arange(8), (4, 8)), axis=1).ravel()       # mixed: every wave holds each octant 8 times
    octant[256:1280] = np.repeat(np.arange(8), 128)                                  # one octant per wave
    octant[1280:] = rng.integers(0, 8, n - 1280)
    d *= OCTANTS[octant]
    for i in range(1280, 1408):                                                      # signed zeros
        axes, zeros = ZEROS[i % len(ZEROS)]
        d[i, list(axes)] = zeros
    tiny = np.array([1e-40, -1e-40, 3e-39, -4e-45])
    for i in list(range(1408, 1472)) + [1472 + 37]:                                  # a denormal: in every lane, in one lane
        d[i, i % 3] = tiny[i % 4]
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    org = target - d * rng.uniform(1.0, 9.0, (n, 1)) * np.maximum(size, 1.0)
    for i in range(1536, 1664):                                                      # origins on a box plane: root, then leaves
        node = 0 if i < 1600 else int(leaves[i % len(leaves)])
        a = i % 3
        lo, hi = b["bmin"][node].astype(np.float64), b["bmax"][node].astype(np.float64)
        org[i] = lo + (hi - lo) * rng.uniform(-0.2, 1.2, 3)
        org[i, a] = (lo, hi)[(i // 3) % 2][a]
        if (i // 6) % 3 < 2:
            d[i, a] = (0.0, -0.0)[(i // 6) % 3]
            d[i] /= np.linalg.norm(d[i])
    org = org.astype(F)
    org[26 * 64 + 11, 0] = np.inf; org[26 * 64 + 40, 2] = -np.inf                   # one lane each
    org[27 * 64 + 23, 1] = np.nan
    org[28 * 64 + 5, 2] = BIG
    lanes = np.arange(64)
    org[29 * 64 + lanes, lanes % 3] = np.where(lanes % 2 == 0, np.inf, -np.inf)      # every lane
    org[30 * 64 + lanes, lanes % 3] = np.nan
    org[31 * 64 + lanes, lanes % 3] = np.where(lanes % 2 == 0, BIG, -BIG)
    d = d.astype(F)
    org.setflags(write=False); d.setflags(write=False)
    return org, d


@functools.lru_cache(maxsize=None)
def oracle_hits(name):
    """the oracle's (hit, prim, t) for rays(name); read-only"""
    o = scene(name)[1]
    org, d = rays(name)
    want = [o.intersect(org[i], d[i]) for i in range(len(org))]
    out = (np.array([h.hit for h in want], np.int32), np.array([h.prim for h in want], np.int32), np.array([h.t for h in want], F))
    for a in out:
        a.setflags(write=False)
    return out


def in_vote_range(d):
    a = np.abs(d.astype(np.float64))
    return ((a >= 2.0 ** -100) & (a <= 2.0 ** 100)).all(axis=1)


def test_the_scenes_and_rays_are_what_they_claim():
    for name in RAY_SCENES:
        org, d = rays(name)
        assert org.shape == d.shape == (2048, 3)
        neg = np.signbit(d)
        code = neg[:, 0] + 2 * neg[:, 1] + 4 * neg[:, 2]
        for w in range(4):
            assert np.array_equal(np.bincount(code[64 * w:64 * w + 64], minlength=8), np.full(8, 8)), name
        for w in range(4, 20):
            assert (code[64 * w:64 * w + 64] == (w - 4) // 2).all(), name
        z = d[1280:1408]
        assert ((z == 0).sum(axis=1) >= 1).all() and ((z == 0).sum(axis=1) == 2).any()
        assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
        den = (d != 0) & (np.abs(d) < np.finfo(F).tiny)
        assert (den[1408:1472].sum(axis=1) == 1).all() and den[1472:1536].sum() == 1 and den[1472 + 37].any()
        on = d[1536:1664]
        assert ((on == 0) & np.signbit(on)).any() and ((on == 0) & ~np.signbit(on)).any() and (on != 0).all(axis=1).any()
        assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
        # which side a wave takes: the vote sees the directions only
        ok = in_vote_range(d).reshape(32, 64).all(axis=1)
        assert ok[HOT_WAVES].all() and not ok[20:24].any(), name
        assert in_vote_range(d[1472:1536]).sum() == 63                        # wave 23: one lane sends 64 to the cold side
        fin = np.isfinite(org).all(axis=1)
        assert fin[:26 * 64].all()
        assert [int((~fin[64 * w:64 * w + 64]).sum()) for w in range(26, 32)] == [2, 1, 0, 64, 64, 0]
        assert np.isinf(org[26 * 64 + 11, 0]) and np.isinf(org[26 * 64 + 40, 2]) and org[26 * 64 + 40, 2] < 0 and np.isnan(org[27 * 64 + 23, 1])
        assert (np.isinf(org[29 * 64:30 * 64]).sum(axis=1) == 1).all() and (org[29 * 64:30 * 64] == -np.inf).any()
        assert (np.isnan(org[30 * 64:31 * 64]).sum(axis=1) == 1).all()
        assert org[28 * 64 + 5, 2] == BIG and ((np.abs(org[31 * 64:]) == BIG).sum(axis=1) == 1).all() and (org[31 * 64:] == -BIG).any()
    assert [len(scene(n)[0][0]) for n in ("tri1", "tri3", "tri64", "sheets", "chain")] == [1, 3, 64, 10, 18]
    for n in RAY_SCENES + FRAME_SCENES:                      # no quad anywhere: every scene runs the builds that take the form
        assert not scene(n)[0][0].any(), n
    b, leaves, depth = tree("tri1")
    assert len(b["left"]) == 1 and list(leaves) == [0]       # the root is the only leaf
    b, leaves, depth = tree("cbox")
    assert len(b["left"]) == 21 and len(leaves) == 11
    b, leaves, depth = tree("chain")
    assert depth >= 12 and len(leaves) == depth, (depth, len(leaves))        # one leaf peeled per level, the last four primitives stay together
    b, leaves, depth = tree("sheets")
    assert set(b["count"][leaves]) == {2, 3} and len(leaves) == 4
    zs = [sorted(scene("sheets")[0][1][b["indices"][b["left"][i]:b["left"][i] + b["count"][i]], 0, 2]) for i in leaves]
    assert zs[0][0] >= 1.0 and zs[1][0] > zs[0][-1] and zs[2][-1] < zs[0][0] and zs[3][0] > zs[2][-1]      # high group first, each group ascending


def pruned_by_closest_t(name):
    """per ray: the oracle hit something, and a leaf that stands after the hit's leaf in pre-order has a box the ray enters (slab
    test against [t_min, inf) in float64, with margins) only beyond the hit: the reference skips it for closest_t alone"""
    b, leaves, _ = tree(name)
    org, d = (a.astype(np.float64) for a in rays(name))
    hit, prim, t = oracle_hits(name)
    slot_of = np.empty(len(b["indices"]), np.int64); slot_of[b["indices"]] = np.arange(len(b["indices"]))
    first = b["left"][leaves].astype(np.int64)
    hit_leaf = np.searchsorted(first, slot_of[np.where(hit != 0, prim, 0)], side="right") - 1          # index among the leaves
    out = np.zeros(len(org), bool)
    with np.errstate(all="ignore"):
        for j, node in enumerate(leaves):
            t0 = (b["bmin"][node].astype(np.float64) - org) / d
            t1 = (b["bmax"][node].astype(np.float64) - org) / d
            near, far = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
            entered = np.isfinite(near) & np.isfinite(far) & (near * (1 + 1e-5) < far) & (far > 1e-3)
            out |= (hit != 0) & (j > hit_leaf) & entered & (near > t.astype(np.float64) * (1 + 1e-5) + 1e-6)
    return out


def test_the_sheets_prune_by_closest_t_in_every_wave():
    pruned = pruned_by_closest_t("sheets").reshape(32, 64)
    with np.errstate(invalid="ignore"):
        near = (np.abs(rays("sheets")[0]) < 2.0 ** 100).all(axis=1).reshape(32, 64).any(axis=1)      # waves with a ray that can meet the scene
    assert list(np.flatnonzero(near)) == list(range(29))
    assert pruned[near].any(axis=1).all(), np.flatnonzero(~pruned.any(axis=1))
    assert pruned[HOT_WAVES[:20]].sum() > 200                                         # and not by a thread: hundreds of rays do


def tie_rays():
    """4 waves of 64 rays onto the plane of `ties`, in numbers for which every product and sum of Moller-Trumbore is exact: the
    origin at z = 4, the direction (dx, dy, -1) with dx, dy in +-{1/8, 1/4, 1/2} (not unit vectors: the hook takes them as they
    are, and the vote passes), the point met a multiple of 1/4.  a = +-64 for every triangle, so f is exact and t is 4.0 for each
    triangle that holds the point: the reference keeps the one it visits first."""
    rng = np.random.default_rng(77)
    n = 256
    point = np.stack([rng.integers(1, 31, n) / 4.0, rng.integers(1, 47, n) / 4.0, np.zeros(n)], 1)
    d = np.stack([rng.choice([-0.5, -0.25, -0.125, 0.125, 0.25, 0.5], n), rng.choice([-0.5, -0.25, -0.125, 0.125, 0.25, 0.5], n), -np.ones(n)], 1)
    return (point - 4.0 * d).astype(F), d.astype(F), point


def test_the_ties_are_ties():
    arrs, o, _, _ = scene("ties")
    b, leaves, _ = tree("ties")
    assert len(leaves) >= 3
    org, d, point = tie_rays()
    assert np.array_equal(org.astype(np.float64) + 4.0 * d.astype(np.float64), point)                 # exact in binary32
    v = arrs[1][:, :3].astype(np.float64)
    x, y = point[:, None, 0] - v[None, :, 0, 0], point[:, None, 1] - v[None, :, 0, 1]                  # in the frame of v0 (exact)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    assert (np.abs(det) == 64.0).all()                                                                 # a = +-64: 1 / a is exact
    uu = (x * e2[None, :, 1] - y * e2[None, :, 0]) / det
    vv = (y * e1[None, :, 0] - x * e1[None, :, 1]) / det
    holds = (uu >= 0) & (vv >= 0) & (uu + vv <= 1)                                                     # rays x triangles, edges included
    slot_of = np.empty(10, np.int64); slot_of[b["indices"]] = np.arange(10)
    leaf_of = np.searchsorted(b["left"][leaves], slot_of, side="right") - 1
    first = np.where(holds, leaf_of[None, :], 99).min(axis=1)
    last = np.where(holds, leaf_of[None, :], -1).max(axis=1)
    several = holds.any(axis=1) & (last > first)
    assert several.reshape(4, 64).sum(axis=1).min() >= 16                      # in every wave: rays whose tie spans leaves
    want = [o.intersect(org[i], d[i]) for i in range(len(org))]
    for i in np.flatnonzero(several):
        assert want[i].hit and want[i].t == 4.0 and leaf_of[want[i].prim] == first[i], i              # the first leaf's, not the last's


@pytest.mark.parametrize("name", ["ties"])
def test_ties_keep_the_leaf_visited_first(loaded, name):
    R = loaded
    o = scene(name)[1]
    org, d, _ = tie_rays()
    got = R.debug_intersect(org, d)
    want = [o.intersect(org[i], d[i]) for i in range(len(org))]
    whit = np.array([h.hit for h in want], np.int32)
    on = whit != 0
    assert np.array_equal(got["hit"] != 0, on) and on.sum() > 128
    assert np.array_equal(got["prim"][on], np.array([h.prim for h in want], np.int32)[on])
    assert np.array_equal(bits(got["t"][on]), bits(np.array([h.t for h in want], F)[on]))


@pytest.mark.parametrize("name", RAY_SCENES)
def test_rays_match_oracle_and_lane(loaded, name):
    R = loaded
    assert R.scene_info()["n_bvh_nodes"] == len(tree(name)[0]["left"])
    org, d = rays(name)
    got = R.debug_intersect(org, d)
    whit, wprim, wt = oracle_hits(name)
    bad = np.flatnonzero((got["hit"] != 0) != (whit != 0))
    assert bad.size == 0, f"{name}: hit differs for rays {bad[:8]}"
    on = whit != 0
    assert on.any() and not on.all()
    assert on[:1280].reshape(20, 64).any(axis=1).all()                                         # every octant wave does meet the scene
    assert np.array_equal(got["prim"][on], wprim[on]), f"{name}: primitive differs for rays {np.flatnonzero(on)[got['prim'][on] != wprim[on]][:8]}"
    tb = bits(got["t"][on]) != bits(wt[on])
    assert not tb.any(), f"{name}: t differs in bits for rays {np.flatnonzero(on)[tb][:8]}"
    assert R.set_traversal(R.LANE) == R.LANE
    lane = R.debug_intersect(org, d)
    assert np.array_equal(lane["hit"], got["hit"]) and np.array_equal(lane["prim"], got["prim"]) and np.array_equal(bits(lane["t"]), bits(got["t"]))


@pytest.mark.parametrize("stats", [False, True], ids=["timed", "stats"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", FRAME_SCENES)
def test_frames_match_oracle_and_lane(loaded, name, size, stats):
    R = loaded
    W, H = size
    want = oracle_frames(name, W, H, DEPTH, 3)

    def render(what):
        out = []
        R.update_resolution(W, H)                            # re-seeds the streams
        R.set_config(spp=SPP, max_depth=DEPTH, segments_per_launch=0, collect_stats=stats, sampling_mode=0)
        for k in range(2):
            st = R.render_frame()
            assert_frame(R, want[k], f"{name} {W}x{H} {what} frame {k}", st if stats else None)      # stats: node_visits are the oracle's
            out.append(R.read_image())
        R.update_resolution(W, H)
        st = R.render_frames(3)
        assert st.samples == W * H * SPP * 3
        if stats:
            assert (st.rays, st.node_visits, st.prim_tests, st.hits) == tuple(sum(w[2][c] for w in want) for c in (1, 2, 3, 4))
        for k in range(3):
            R.select_frame(k)
            assert_frame(R, want[k], f"{name} {W}x{H} {what} frame {k} of the batch")
            out.append(R.read_image())
        return out

    swept = render("sweep")
    assert R.set_traversal(R.LANE) == R.LANE
    for k, ((rgb, rad), (lrgb, lrad)) in enumerate(zip(swept, render("LANE"))):
        assert np.array_equal(bits(rad), bits(lrad)) and np.array_equal(rgb, lrgb), f"{name} {W}x{H}: LANE and the sweep differ in image {k}"
