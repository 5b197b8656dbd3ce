"""The cases of tests/test_solver_vs_ref.py (oracle against the compiled reference's radiosity pre-pass, CPU) and of
tests/test_gpu_solver_vs_ref.py (the HIP solver against the same recorded answers).  Inputs only: nothing here is derived
from the reference.  The record (tests/golden/ref_solver.npz) keeps a hash of each case's inputs next to the answers, so a
changed case is noticed rather than compared with a stale answer.

Scenes.  The smallest at which each rule can go wrong: the two Cornell boxes, tests/ragged_scenes.py's soups at n = 1, 2, 3
(no pair / one pair / a ring), 65 (a second 8 x 8 block row with one live thread, a second 64-lane group of one) and 257
(the certified walk's threshold of 256 crossed by one; 8 samples at most), its two 60-primitive chains whose tree is deeper
than 31 levels, `coincident` (two triangles with the same centroid - dist < 1e-6 - under a ceiling that faces them and over a
floor that they turn their backs to) and `scripted` (below).
"""
import functools
import os

import numpy as np

import anyhit_edge_sets
import guided_record_sets as G
from oracle_binding import OracleScene, SCENES, sha
from ragged_scenes import deep_chain, nonfinite_scene, random_scene

F = np.float32
U32 = np.uint32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_solver.npz")
FFFF = 0xFFFFFFFF


def _scene(prims):
    """prims: [(verts (3 or 4, 3), normal, Le)] -> arrays; Kd 0.5"""
    n = len(prims)
    types = np.array([len(v) - 3 for v, _, _ in prims], np.int32)
    verts = np.zeros((n, 4, 3), F)
    for i, (v, _, _) in enumerate(prims):
        verts[i, :len(v)] = np.asarray(v, F)
    normal = np.array([p[1] for p in prims], F); Le = np.array([[p[2]] * 3 for p in prims], F)
    return types, verts, normal, np.full((n, 3), 0.5, F), Le


def coincident_scene():
    up, down = (0, 0, 1), (0, 0, -1)
    return _scene([([(-3, -1, 0), (3, -1, 0), (0, 2, 0)], up, 1.0),            # 0 and 1: the same centroid, (0, 0, 0) exactly
                   ([(3, 1, 0), (-3, 1, 0), (0, -2, 0)], up, 0.0),
                   ([(-2, -2, 2), (2, -2, 2), (2, 2, 2), (-2, 2, 2)], down, 2.0),   # 2: a ceiling that faces both
                   ([(-2, -2, -2), (2, -2, -2), (0, 3, -2)], up, 0.5)])         # 3: a floor behind them (back-facing pairs)


S2 = float(F(np.sqrt(0.5)))
W49 = int(4 / 9 * 2 ** 32)       # r1 = 4/9: sqrt(r1) = 2/3, so with r2 = 1/2 a triangle is sampled at its centroid
W12 = 0x80000000                 # r2 = 1/2


def scripted_scene():
    """Four groups 100 apart in y, so that no group can block another's segments.
    0, 1   an open book: page 0 (triangle, plane z = x) and page 1 (quad, plane z = -x) face each other and share the vertex
           (0, 1, 0), which is v2 of the triangle and v01 of the quad: the vertex both are sampled at by r1 = r2 = 1.0f, so
           raw words 0xFFFFFFFF put p_i on p_j (r == 0 < 1e-6).
    2, 3   a floor triangle (normal +z) and an upright triangle that crosses the floor's plane: their centroids face each other,
           but r1 near 0 samples the upright one at its v0, below the plane (cos_theta_i < 0).
    4 - 6  two triangles facing each other, 4 apart, and a 10 x 10 quad between them: every sample is blocked.
    7, 8   a small triangle 1 under the centroid of a triangle of area 300: sampled centroid to centroid, F_ij is 300 / pi.
    9 - 11 two triangles facing each other, 4 apart, and a quad 0.5e-4 in front of the upper one: a segment from 9 to 10 of
           length r meets it at about r - 1.9e-4 from its origin (which lies 1e-4 above 9), between the r - 2e-4f at which the
           reference stops looking and the r - 1e-4 a misreading would stop at.  Not blocked.
    """
    up, down = (0, 0, 1), (0, 0, -1)
    tri = np.array([(-1, -1, 0), (1, -1, 0), (0, 2, 0)], np.float64)
    at = lambda v, y, z=0.0: np.asarray(v, np.float64) + (0, y, z)
    return _scene([([(1, -1, 1), (1, 1, 1), (0, 1, 0)], (-S2, 0, S2), 1.0),
                   ([(-1, 1, 1), (-1, -1, 1), (0, -1, 0), (0, 1, 0)], (S2, 0, S2), 2.0),
                   (at(tri, 100), up, 1.0),
                   (at([(2, 0, -1), (2, 1, 2), (2, -1, 2)], 100), (-1, 0, 0), 3.0),
                   (at(tri, 200), up, 1.0), (at(tri, 200, 4), down, 1.0),
                   (at([(-5, -5, 2), (5, -5, 2), (5, 5, 2), (-5, 5, 2)], 200), up, 0.0),
                   (at(tri * 0.1, 300), up, 1.0),
                   (at(tri * 10, 300, 1), down, 4.0),
                   (at(tri, 400), up, 1.0), (at(tri, 400, 4), down, 1.0),
                   (at([(-5, -5, 0), (5, -5, 0), (5, 5, 0), (-5, 5, 0)], 400, float(F(4) - F(0.5e-4))), up, 0.0)])


@functools.lru_cache(maxsize=None)
def scene_arrays(name):
    if name.startswith("soup"):
        return random_scene(int(name[4:]))
    if name.startswith("deep_"):
        t, v, n, b, le = deep_chain(name.startswith("deep_mixed"))
        if name.endswith("_mirror"):
            # The chain's x falls along it, so each node's far leaf is the RIGHT child, which the walk pops first: its stack never
            # grows and nothing is dropped.  Mirrored in x the far leaf is the left child and waits on the stack while the walk
            # descends: one entry per level, 30 of them at level 30.
            v = v * np.array([-1, 1, 1], F); n = n * np.array([-1, 1, 1], F)
        return t, v, n, b, le
    if name == "coincident":
        return coincident_scene()
    if name == "scripted":
        return scripted_scene()
    if name == "nf65":                                   # soup65's triangles with Le[0] = (inf, 0, 3e38): 0 * inf under a wrong F_ij test
        return nonfinite_scene(65, 0)[0]
    p = OracleScene.load(os.path.join(SCENES, name + ".obj")).prims()
    return p["type"], p["verts"], p["normal"], p["bsdf"], p["Le"]


def inputs_sha(*arrays):
    return sha(np.concatenate([np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8) for a in arrays]))


def scene_sha(name):
    t, v, n, b, le = scene_arrays(name)
    return inputs_sha(np.asarray(t, np.int32), *(np.asarray(a, F) for a in (v, n, b, le)))


def canon(a):
    """a with every NaN replaced by the one quiet NaN 0x7fc00000: what a device answer is compared through, since a NaN's sign
    and payload are the hardware's"""
    a = np.array(a, copy=True)
    if a.dtype == F:
        a[np.isnan(a)] = np.array([0x7FC00000], U32).view(F)[0]
    return a


def bulky(a, rows=4):
    """what the record keeps of an answer too large to keep whole: its hash, the hash of canon() of it, and its first rows"""
    a = np.ascontiguousarray(a)
    return dict(sha=sha(a), sha_nan=sha(canon(a)), head=a[:rows].copy())


def same_bulky(got, rec, nan_equal=False):
    """nan_equal: NaN matches NaN whatever its bits (device answers); otherwise bit for bit"""
    got = np.ascontiguousarray(got)
    head = np.asarray(rec["head"])
    if nan_equal:
        return canon(got[:len(head)]).tobytes() == canon(head).tobytes() and np.array_equal(sha(canon(got)), rec["sha_nan"])
    return got[:len(head)].tobytes() == head.tobytes() and np.array_equal(sha(got), rec["sha"])


# ---- form-factor rows -------------------------------------------------------------------------------------------------------
ROWS_257 = [0, 1, 63, 64, 128, 255, 256]                  # 256: the one row (and column) of the second block of 256
CHAINS = ("deep_tri", "deep_mixed", "deep_tri_mirror", "deep_mixed_mirror")
SMALL = ("cbox", "cbox_quads", "soup1", "soup2", "soup3", "soup65") + CHAINS + ("coincident", "scripted")
# (scene, use_monte_carlo, mc_samples): 1, 3, 8 and 64 samples make max(1, n / 4) = 1, 2, 16, max(2, n / 2) = 2, 4, 32 and n
FF_ROW_CASES = [(s, 1, m) for s in SMALL for m in (1, 3, 8, 64)] + [(s, 0, 1) for s in SMALL] + \
               [("soup257", 1, m) for m in (1, 3, 8)] + [("soup257", 0, 1)]


def ff_rows(scene):
    return np.array(ROWS_257 if scene == "soup257" else range(len(scene_arrays(scene)[0])), np.int32)


def ff_key(c):
    return f"ff_rows/{c[0]}/{'mc%d' % c[2] if c[1] else 'p2p'}"


# ---- whole solves -------------------------------------------------------------------------------------------------------------
FILTERS = {"off": dict(enable_filtering=False), "bilateral": dict(enable_filtering=True, use_bilateral=True),
           "gaussian": dict(enable_filtering=True, use_bilateral=False)}
SOLVE_CASES = [(s, it, f, 1) for s in ("cbox", "soup65") for it in (0, 1, 3) for f in FILTERS] + \
              [(s, 3, "bilateral", 0) for s in ("cbox", "soup65")] + \
              [("nf65", 1, "off", 1), ("nf65", 3, "off", 0)]                  # ... and an infinite emitter that most receivers do not see


def solve_params(c):
    scene, it, filt, mc = c
    return dict(num_iterations=it, mc_samples=64 if scene == "cbox" else 8 if scene == "soup65" else 3, use_monte_carlo=bool(mc), **FILTERS[filt])


def solve_key(c):
    return f"solve/{c[0]}/it{c[1]}/{c[2]}/{'mc' if c[3] else 'p2p'}"


SOLVE_FIELDS = ("form_factors", "radiosity", "unshot", "grid", "radiosity_grid")


# ---- scripted pairs -----------------------------------------------------------------------------------------------------------
def scripted_cases():
    """[(label, i, j, n_samples, words)] on scripted_scene()"""
    rng = np.random.default_rng(41)
    rnd = lambda k: [int(x) for x in rng.integers(0, 2 ** 32, k)]
    centre = [W49, W12]
    out = [("coincide", 0, 1, 1, [FFFF] * 4), ("coincide_twice", 0, 1, 2, [FFFF] * 8), ("coincide_back", 1, 0, 1, [FFFF] * 4),
           ("zeros", 0, 1, 1, [0] * 4), ("zeros_back", 1, 0, 1, [0] * 4), ("zero_ones", 0, 1, 1, [0, FFFF, FFFF, 0]),
           ("ones_zero", 1, 0, 1, [FFFF, 0, 0, FFFF]), ("overrun", 0, 1, 2, [FFFF] * 4 + [5, 6]),
           ("coincide_then_live", 0, 1, 3, [FFFF] * 4 + rnd(8)),
           ("cos_negative", 2, 3, 1, centre + [0, 0]), ("cos_negative_then_live", 2, 3, 2, centre + [0, 0] + centre + centre),
           ("cos_live", 2, 3, 1, centre + centre), ("cos_back", 3, 2, 1, [0, 0] + centre),
           ("blocked_1", 4, 5, 1, rnd(4)), ("blocked_8", 4, 5, 8, rnd(32)), ("blocked_back", 5, 4, 8, rnd(32)),
           ("clamped", 7, 8, 1, centre + centre), ("clamped_8", 7, 8, 8, (centre + centre) * 8), ("unclamped_back", 8, 7, 1, centre + centre),
           ("window", 9, 10, 1, centre + centre), ("window_8", 9, 10, 8, rnd(32)), ("window_back", 10, 9, 8, rnd(32)),
           ("self", 3, 3, 4, rnd(16)), ("other_group", 2, 5, 64, rnd(256))]
    for k in range(6):
        out.append((f"random{k}_book", 0, 1, 3, rnd(12))); out.append((f"random{k}_book_back", 1, 0, 8, rnd(32)))
        out.append((f"random{k}_cross", 2, 3, 8, rnd(32))); out.append((f"random{k}_big", 7, 8, 8, rnd(32)))
    return out


# ---- grid index ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_index_cases():
    """(directions, normals): the pair directions of tests/guided_record_sets.py's worlds as update_radiosity_grid forms them
    (float32), the cell centres and borders of every cell about an axis, a tilted and the Frisvad-branch normal, and vectors
    of zeros, of -0 and along +-normal."""
    dirs, nrms = [], []
    for w in G.grid_worlds():
        n = len(w["centre"])
        rows = range(n) if n <= 40 else [0]
        for i in rows:
            d = (w["centre"] - w["centre"][i]).astype(F)
            r = np.sqrt((d.astype(np.float64) ** 2).sum(1)).astype(F)
            ok = (r > 0) & (np.arange(n) != i)
            dirs.append((d[ok] / r[ok, None]).astype(F)); nrms.append(np.tile(w["normal"][i], (int(ok.sum()), 1)))
    z = F(-0.9999999)
    frisvad = [(0, 0, -1), (np.sqrt(max(0.0, 1 - float(z) ** 2)), 0, z), (0, np.sqrt(max(0.0, 1 - float(np.nextafter(z, F(0))) ** 2)), np.nextafter(z, F(0)))]
    for normal in [(0, 0, 1), (1, 0, 0), (0, -1, 0), tuple(G.TILTED)] + frisvad:
        nf = np.asarray(normal, np.float64)
        t, b = G.frisvad(nf)
        for th in np.arange(0, 17) * np.pi / 16:
            for ph in np.arange(0, 33) * np.pi / 16:
                dirs.append(np.array([np.sin(th) * np.cos(ph) * t + np.sin(th) * np.sin(ph) * b + np.cos(th) * nf], F)); nrms.append(np.array([nf], F))
        extra = np.array([nf, -nf, (0, 0, 0), (-0.0, -0.0, -0.0), t, -t, b, -b, 2 * nf, 1e-30 * nf, -1e30 * t], F)
        dirs.append(extra); nrms.append(np.tile(np.asarray(nf, F), (len(extra), 1)))
    return np.concatenate(dirs).astype(F), np.concatenate(nrms).astype(F)


# ---- visibility -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def anyhit_rays():
    """[(case, member, scene arrays, o, d, max_dist, expected)]: tests/anyhit_edge_sets.py's families, pair (0, 1)"""
    out = []
    for case, member, arrs, blocked in anyhit_edge_sets.all_scenes():
        o, d, md = anyhit_edge_sets.segment(arrs[0], arrs[1], arrs[2])
        out.append((case, member, arrs, o, d, md, blocked))
    return out


def chain_rays(arrs, centroid):
    """the shadow segment of every ordered pair of the chain (the first n * (n - 1) rays), as calculate_form_factors_kernel forms it (float32; the unit
    direction is renormalised by Ray's constructor on both sides): o, d, max_dist, source, target"""
    n = len(arrs[0]); nr = arrs[2]
    O, D, M, S, T = [], [], [], [], []
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            v = (centroid[j] - centroid[i]).astype(F)
            r = F(np.sqrt(np.float64(v[0]) ** 2 + np.float64(v[1]) ** 2 + np.float64(v[2]) ** 2))
            O.append((centroid[i] + F(1e-4) * nr[i]).astype(F)); D.append((v / r).astype(F)); M.append(F(r - F(2e-4))); S.append(i); T.append(j)
    # and one ray aimed at each primitive k alone, from 1.5 x_k along the x axis through its centroid and no further than
    # 0.5 x_k (the next primitive stands at x_k / 2.2), nothing skipped: blocked if the walk reaches k's leaf and the slab test
    # lets it in.  (Where 0.5 x_k > 4e5 it does not: the zero direction components get the slope 1e8, and 0.004 * 1e8 is the
    # furthest such a ray stays inside a box 0.008 wide.)
    for k in range(n):
        c = centroid[k]
        O.append(np.array([F(1.5) * c[0], c[1], c[2]], F)); D.append(np.array([-np.sign(c[0]), 0, 0], F)); M.append(F(abs(c[0]))); S.append(-1); T.append(-1)
    return np.array(O, F), np.array(D, F), np.array(M, F), np.array(S, np.int32), np.array(T, np.int32)


# ---- "Apply Filter & Rebuild CDFs" -------------------------------------------------------------------------------------------
KEPT_IMPULSES = (0, 15, 16 * 7 + 8, 16 * 8, 255)         # the corners, the horizon rows, the phi wrap


@functools.lru_cache(maxsize=None)
def filter_cases():
    """[dict(label, rgb (256, 3), counts (256,), sigma_spatial, sigma_range)]: one-hot, all-zero and huge-range grids, and the
    constructed grids of tests/guided_record_sets.py (of its 256 impulses, five)."""
    out = []

    def add(label, rgb, counts, ss=G.SIGMA_S, sr=G.SIGMA_R):
        out.append(dict(label=label, rgb=np.asarray(rgb, F).reshape(256, 3), counts=np.asarray(counts, F).reshape(256), sigma_spatial=F(ss),
                        sigma_range=F(sr)))
    hot = np.zeros((256, 3), F); hot[16 * 3 + 5] = (1, 2, 3)
    cnt = np.zeros(256, F); cnt[16 * 3 + 5] = 7
    add("one_hot", hot, cnt)
    add("all_zero", np.zeros((256, 3), F), np.zeros(256, F))
    huge = np.full((256, 3), 1e-30, F); huge[16 * 2 + 7] = 1e30; huge[16 * 6 + 1] = 3e-38
    hc = np.ones(256, F); hc[16 * 2 + 7] = 2.0 ** 24; hc[16 * 6 + 1] = 0
    add("huge_range", huge, hc)
    rng = np.random.default_rng(77)
    add("random", rng.uniform(0, 2, (256, 3)) ** 4, rng.integers(0, 9, 256))
    for c in G.filter_set():
        if c["label"].startswith("impulse") and int(c["label"][7:]) not in KEPT_IMPULSES:
            continue
        add("set:" + c["label"], c["rgb"], c["grid"], c["sigma_spatial"], c["sigma_range"])
    return out


def filter_groups():
    """{(sigma_spatial, sigma_range): [case index]}: one call of the wrapper per group"""
    groups = {}
    for k, c in enumerate(filter_cases()):
        groups.setdefault((float(c["sigma_spatial"]), float(c["sigma_range"])), []).append(k)
    return groups


# ---- update_radiosity_grid on constructed worlds ---------------------------------------------------------------------------------
def world_as_scene(w):
    """a world of centres and normals as primitives: quad k has all four corners at centre k, so that its centroid,
    (c + c + c + c) * 0.25f, is c exactly; update_radiosity_grid reads nothing else of the geometry"""
    n = len(w["centre"])
    verts = np.repeat(w["centre"].astype(F)[:, None, :], 4, axis=1)
    return np.ones(n, np.int32), verts, w["normal"].astype(F), np.full((n, 3), 0.5, F), np.zeros((n, 3), F)


@functools.lru_cache(maxsize=None)
def grid_worlds():
    return [w for w in G.grid_worlds()]


# ---- subdivision -----------------------------------------------------------------------------------------------------------------
SUBDIVIDE_CASES = [(s, lv) for s in ("cbox", "cbox_quads", "mixed") for lv in (0, 1, 2)]
