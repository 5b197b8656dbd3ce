"""The closest-hit walks of the device at the edges of their decisions, per ray (tests/intersect_edge_sets.py; the sets are proven on
the CPU by tests/test_intersect_edge_sets_host.py).  Everything is exact: hit, primitive, and the bits of t, p and n against
OracleScene.intersect.  No tolerance anywhere.

  walks      debug_intersect with the traversal forced to SWEEP, LANE and STACK (the mode set_traversal returns is asserted), on
             scenes of triangles only, quads only and both - both sweep forms and both branches of leaf_prim; debug_first_hit -
             first_hit as the Radiosity view and the feature pass call it - through CERTIFIED, LANE and STACK on the same sets over
             scenes of 140 primitives and more; debug_intersect_fast, the wide walk alone, on those
  placement  every labelled ray alone at lanes 0, 37 and 63 of a wave whose other 63 rays fail the (a, u) stage of the primitive it
             is aimed at, at lane 37 of a wave whose others pass it, and the whole set shuffled with a partial last wave: the
             answers do not change.  This pins the votes of mt_accept / mt_candidate / mt_accept_update and of ray_inv - a lane's
             answer must not depend on its neighbours.
"""
import functools

import numpy as np
import pytest

import intersect_edge_sets as S
import ptmi
from intersect_edge_sets import F

pytestmark = pytest.mark.gpu
MODES = (("SWEEP", ptmi.Renderer.SWEEP), ("LANE", ptmi.Renderer.LANE), ("STACK", ptmi.Renderer.STACK))
KEYS5 = ("hit", "prim", "t", "p", "n")


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.set_traversal(-1)
    r.close()


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def assert_same(got, want, keys, what, labels=None):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        bad = words(g) != words(w)
        if k in ("p", "n"):
            bad &= ~(np.isnan(g) & np.isnan(w))                     # p = o + t d of a non-finite ray: a NaN is a NaN, whatever its payload;
                                                                    # hit, prim and t are compared in every bit
        if bad.any():
            i = int(np.nonzero(bad.reshape(len(g), -1).any(1))[0][0])
            raise AssertionError(f"{what}: {k} differs for {int(bad.reshape(len(g), -1).any(1).sum())} rays, first {i}"
                                 f" ({labels[i] if labels else ''}): got {g[i]}, oracle {w[i]}")


def load(R, s, mode):
    R.load_scene_arrays(*s.scene)
    got = R.set_traversal(mode, sweep_max_prims=max(64, len(s.types)))
    assert got == mode, (got, mode)


def in_groups(s, call, keys):
    """call(o, d, t_min, t_max) per group of rays with the same bounds, gathered in the set's order"""
    out = None
    for t_min, t_max, idx in s.groups():
        g = call(s.o[idx], s.d[idx], t_min, t_max)
        if out is None:
            out = {k: np.zeros((len(s),) + g[k].shape[1:], g[k].dtype) for k in keys}
        for k in keys:
            out[k][idx] = g[k]
    return out


# ------------------------------------------------------------------------------------------------
# every set through the three reference walks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("name", list(S.BUILDERS))
def test_every_edge_ray_answers_as_the_oracle(R, name, kind):
    s = S.edge_set(name, kind)
    if kind != "tri" and name in ("extent", "extent_out"):          # quads beyond the bound of SceneState::checkExtent
        with pytest.raises(ptmi.PtmiError, match="quad edge"):
            R.load_scene_arrays(*s.scene)
        return
    want = S.oracle_answers(name, kind)
    for mname, mode in MODES:
        load(R, s, mode)
        got = in_groups(s, R.debug_intersect, KEYS5)
        assert_same(got, want, KEYS5, f"{name}/{kind}/{mname}", s.label)


# ------------------------------------------------------------------------------------------------
# wave placement
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def placement(name, kind):
    """Per group of equal bounds: the labelled rays with a target, a rejecter and a hitter for each (None where the leaf of the
    target holds no rejecter), and the oracle's answers for all three - computed once, shared by the modes."""
    s = S.edge_set(name, kind)
    scene = S.oracle_scene(name, kind)
    b = scene.bvh()
    leaf_box = {}
    for node in np.nonzero(b["count"] > 0)[0]:
        for j in range(b["count"][node]):
            leaf_box[int(b["indices"][b["left"][node] + j])] = (b["bmin"][node], b["bmax"][node])
    want = S.oracle_answers(name, kind)
    out = []
    cache = {}
    for t_min, t_max, idx in s.groups():
        idx = np.array([i for i in idx if s.target[i] >= 0], np.int64)
        if not len(idx):
            continue
        rej, hitr = [], []
        for i in idx:
            key = (int(s.target[i]), s.o[i][2].tobytes(), s.d[i].tobytes())
            if key not in cache:
                cache[key] = S.wave_companions(s, i, leaf_box[int(s.target[i])])
            r, h = cache[key]
            far = (np.array([-1000, -1000, s.o[i][2]], F), np.array([0, 0, 1], F))          # misses the root's box
            rej.append(r if r is not None else far); hitr.append(h if h is not None else far)
        ro, rd = np.array([x[0] for x in rej], F), np.array([x[1] for x in rej], F)
        ho, hd = np.array([x[0] for x in hitr], F), np.array([x[1] for x in hitr], F)
        tm, tx = np.full(len(idx), t_min, F), np.full(len(idx), t_max, F)
        real = sum(cache[(int(s.target[i]), s.o[i][2].tobytes(), s.d[i].tobytes())][0] is not None for i in idx)
        out.append(dict(t_min=t_min, t_max=t_max, idx=idx, want={k: want[k][idx] for k in KEYS5},
                        rej=(ro, rd, S.answers_for(scene, ro, rd, tm, tx)), hit=(ho, hd, S.answers_for(scene, ho, hd, tm, tx)), real=real))
    return out


def waves(o, d, want, other, lane):
    """one wave per ray: the ray at `lane`, `other`'s ray of the same row at the 63 other lanes; the expected answers alike"""
    n = len(o)
    oo, od, ow = other
    O = np.repeat(oo[:, None, :], 64, 1); D = np.repeat(od[:, None, :], 64, 1)
    O[:, lane] = o; D[:, lane] = d
    W = {}
    for k in KEYS5:
        w = np.repeat(ow[k][:, None], 64, 1)
        w[:, lane] = want[k]
        W[k] = w.reshape((n * 64,) + w.shape[2:])
    return O.reshape(-1, 3), D.reshape(-1, 3), W


PLACED = [(n, k) for n in ("barycentric", "determinant", "bounds", "slab", "planar", "nonfinite", "extent_in") for k in S.KINDS] + [("extent", "tri")]


@pytest.mark.parametrize("name,kind", PLACED)
def test_a_lanes_answer_does_not_depend_on_its_wave(R, name, kind):
    s = S.edge_set(name, kind)
    groups = placement(name, kind)
    # every ray stands among REAL rejecters - rays that enter its primitive's leaf and fail the (a, u) stage there - not among
    # far-away rays that never reach the vote.  (The extent scenes' leaves are the primitives: no such ray exists for most.)
    assert groups and (name.startswith("extent") or all(g["real"] == len(g["idx"]) for g in groups))
    rng = np.random.default_rng(11)
    for mname, mode in MODES:
        load(R, s, mode)
        for g in groups:
            o, d, want = s.o[g["idx"]], s.d[g["idx"]], g["want"]
            labels = [s.label[i] for i in g["idx"]]
            for other, lanes in (("rej", (0, 37, 63)), ("hit", (37,))):
                for lane in lanes:
                    O, D, W = waves(o, d, want, g[other], lane)
                    got = R.debug_intersect(O, D, g["t_min"], g["t_max"])
                    assert_same(got, W, KEYS5, f"{name}/{kind}/{mname}/{other}@{lane}", [labels[i // 64] + f" wave lane {i % 64}" for i in range(len(O))])
            # the whole group shuffled, the last wave partial
            order = rng.permutation(len(o))
            if len(order) % 64 == 0:
                order = order[:-1]
            got = R.debug_intersect(o[order], d[order], g["t_min"], g["t_max"])
            assert_same(got, {k: want[k][order] for k in KEYS5}, KEYS5, f"{name}/{kind}/{mname}/shuffled", [labels[i] for i in order])


def test_origins_beyond_the_quad_bound_are_refused(R):
    """Where the scene has quads, a ray origin so far out that the quad test's products could overflow is refused on the host - a
    hook's ray and the camera alike; rays with a non-finite component pass (no primitive accepts them), and a scene of triangles
    takes every origin."""
    s, far = S.edge_set("extent_in", "quad"), S.edge_set("extent", "quad")
    R.load_scene_arrays(*s.scene)
    i = far.where("quad", "extent", "u_nan", "vertex", "far", "plus")[0]
    for call in (R.debug_intersect, R.debug_first_hit, R.debug_intersect_fast):
        with pytest.raises(ptmi.PtmiError, match="quad edge"):
            call(far.o[i:i + 1], far.d[i:i + 1])
    nan = np.array([[np.nan, 0, 0]], F)
    assert R.debug_intersect(far.o[i:i + 1], nan)["hit"][0] == 0 and R.debug_intersect(nan, far.d[i:i + 1])["hit"][0] == 0
    R.update_resolution(8, 8)
    R.set_config(spp=1, max_depth=1)
    R.set_camera(ptmi.Camera((2.0 ** 69, 2.0 ** 69, -2.0 ** 69), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 90.0, 0.0, 0))
    try:
        with pytest.raises(ptmi.PtmiError, match="quad edge"):
            R.render_frame()
    finally:
        R.set_camera(ptmi.default_camera())
    R.render_frame()
    t = S.edge_set("extent", "tri")
    R.load_scene_arrays(*t.scene)
    assert R.debug_intersect(far.o[i:i + 1], far.d[i:i + 1])["hit"][0] == 1


# ------------------------------------------------------------------------------------------------
# first_hit (the certified walk and the reference's) and the wide walk alone, on scenes of 140 primitives and more
# ------------------------------------------------------------------------------------------------
BIG_SETS = ["barycentric", "determinant", "bounds", "ties", "ties_rev", "origins", "slab", "planar", "nonfinite"]


def open_rays(s):
    """the rays first_hit can take: t_max == FLT_MAX, grouped by t_min"""
    return [(t_min, idx) for t_min, t_max, idx in s.groups() if t_max == float(S.FLT_MAX)]


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("name", BIG_SETS)
def test_first_hit_is_the_references_hit_in_every_mode(R, name, kind):
    s = S.edge_set(name, kind, big=True)
    assert len(s.types) >= 128
    want = S.oracle_answers(name, kind, big=True)
    R.load_scene_arrays(*s.scene)
    auto = R.set_traversal(-1)
    assert auto == R.CERTIFIED, auto                               # the default walk of these scenes
    for mname, mode in (("CERTIFIED", -1), ("LANE", R.LANE), ("STACK", R.STACK)):
        assert R.set_traversal(mode) == (auto if mode < 0 else mode)
        for t_min, idx in open_rays(s):
            got = R.debug_first_hit(s.o[idx], s.d[idx], t_min)
            assert_same(got, {k: want[k][idx] for k in KEYS5[:3]}, KEYS5[:3], f"{name}/{kind}/{mname}", [s.label[i] for i in idx])
            order = np.random.default_rng(3).permutation(len(idx))[: max(1, len(idx) - 1)]      # another company in every wave
            got = R.debug_first_hit(s.o[idx][order], s.d[idx][order], t_min)
            assert_same(got, {k: want[k][idx][order] for k in KEYS5[:3]}, KEYS5[:3], f"{name}/{kind}/{mname}/shuffled", [s.label[i] for i in idx[order]])


@pytest.mark.parametrize("name", BIG_SETS)
def test_wide_walk_finds_the_nearest_primitive(R, name):
    """The wide walk alone (no proof, no fallback) promises the nearest hit: where one primitive is nearest - everywhere but on the
    tie rays - it is the oracle's primitive, and t is the oracle's on every ray."""
    s = S.edge_set(name, "tri", big=True)
    want = S.oracle_answers(name, "tri", big=True)
    R.load_scene_arrays(*s.scene)
    R.set_traversal(-1)
    got = in_groups(s, lambda o, d, t_min, t_max: R.debug_intersect_fast(o, d, t_min, t_max), KEYS5[:3])
    assert_same(got, want, ("hit", "t"), f"{name}/wide", s.label)
    unique = ~s.tree_matters
    assert_same({"prim": got["prim"][unique]}, {"prim": want["prim"][unique]}, ("prim",), f"{name}/wide", [s.label[i] for i in np.nonzero(unique)[0]])
