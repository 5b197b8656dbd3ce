"""oracle/ptmi_oracle.c against the REFERENCE's own shading half - rendering/integrator.h and rendering/grid.h compiled into
oracle/_ref/libptmi_ref_integrator.so (oracle/ref_integrator_harness.cpp, only where the reference tree exists).  Bit-exact.

Per call, over scripted raw 32-bit draws: sampleCosineHemisphere, misPowerHeuristic, Grid::loadPrecomputed + sample (direction,
out_pdf, draws), Grid::computePDF, sampleMIS (direction, weight, used_bsdf, draws).  Whole frames, with the oracle's
generator behind curand_uniform (stream mode): render_init + render (depth 5, rgb8) and render_radiosity, and the radiance of
integrator() at other depths.  The cases sit at the edges where a restatement goes wrong: raw words 0 and 0xFFFFFFFF, draws
on and next to every CDF entry, xi == BSDF_PROB, the theta clamp, phi = 2 pi, normals at and around the -0.9999999f branch of
the Frisvad frame, -0 components, one-hot and all-zero grids, a huge dynamic range, directions on the horizon and at
atan2 = +-pi, and emitters that drive the tone-map to 1 and the sample sum to inf.

Every answer of the compiled reference is recorded in tests/golden/ref_integrator.npz.  Where oracle/_ref is built the tests
ask it live and also require the recorded bits; everywhere else they compare the oracle with the record.
Re-record (where oracle/_ref is built):  python tests/golden/make_golden.py --ref-only
"""
import ctypes as C
import os

import numpy as np
import pytest

from guided_fixtures import synthetic_radiosity_grids
from oracle_binding import (OracleScene, RefIntegratorScene, SCENES, default_camera, oracle_lib, recorded_reference,
                            ref_int_available)

F = np.float32
U32 = np.uint32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_integrator.npz")
SEED = 2023                              # render_init: curand_init(2023 + pixel_index, pixel_index, 0)
BSDF, GRID, MIS = 0, 2, 3                # SamplingMode (render_config.h)


@pytest.fixture(scope="module")
def ref():
    yield from recorded_reference(GOLDEN, ref_int_available())


def bits(a):
    return np.ascontiguousarray(a, F).view(U32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- cases ------------------------------------------------------------------------------------------------------------------
def word_to_uniform(w):
    return oracle_lib().po_word_to_uniform(int(w))


def first_word(pred):
    """The smallest raw word whose curand_uniform satisfies pred (monotone in the word); 0xFFFFFFFF if none does."""
    lo, hi = 0, 0xFFFFFFFF
    while lo < hi:
        mid = (lo + hi) // 2
        if pred(F(word_to_uniform(mid))):
            hi = mid
        else:
            lo = mid + 1
    return lo


def words_around(p):
    """Raw words whose uniforms are the float just below p, p itself (where a word maps there) and the float just above."""
    p = F(p)
    w = first_word(lambda x: x >= p)
    return sorted({max(w - 1, 0), w, first_word(lambda x: x > p)})


def one_hot(t, p, value=1.0):
    g = np.zeros((16, 16, 3), F)
    g[t, p] = value
    return g


def grid_cases():
    """(name, 16 x 16 x 3 radiosity grid).  The records are the oracle's precomputeCDFs of these grids, which
    tests/test_guided_record_sets_host.py pins to the reference's own Grid::initFromRadiosity + buildCDFs."""
    rng = np.random.default_rng(5)
    smooth = synthetic_radiosity_grids(1, seed=3, empty_every=0)[0].reshape(16, 16, 3)
    ties = np.ones((16, 16, 3), F)                                   # marginal k/8, rows (u+1)/16: exact binary fractions
    huge = np.full((16, 16, 3), 1e-30, F); huge[2, 7] = 1e30; huge[6, 1] = 3e-38
    spiky = rng.uniform(0, 1, (16, 16, 3)).astype(F) ** 8
    return [("zero", np.zeros((16, 16, 3), F)), ("hot_row0", one_hot(0, 5)), ("hot_row7", one_hot(7, 9)),
            ("hot_phi0", one_hot(3, 0)), ("hot_phi15", one_hot(4, 15)), ("ties", ties), ("huge", huge),
            ("smooth", smooth), ("spiky", spiky)]


def records(grids):
    """The oracle's PrecomputedCDF records (530 words each) of the grids, through a one-triangle scene per grid."""
    out = []
    for _, g in grids:
        s = OracleScene.from_arrays(np.zeros(1, np.int32), np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0]]], F),
                                    np.array([[0, 0, 1]], F), np.full((1, 3), 0.5, F), np.zeros((1, 3), F))
        s.set_radiosity_grids(g.reshape(1, 256, 3))
        out.append(s.cdfs()[0].copy())
    return np.array(out, F)


def normal_cases():
    z = F(-0.9999999)
    below, above = np.nextafter(z, F(-2)), np.nextafter(z, F(0))
    out = [[0, 0, -1], [0, 0, 1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [-0.0, -0.0, 1], [-0.0, 0.0, -1],
           [-0.0, -1, -0.0], [1, -0.0, -0.0]]
    for zz in (z, below, above):
        out.append([np.sqrt(max(0.0, 1 - float(zz) ** 2)), 0, zz])
        out.append([0, -np.sqrt(max(0.0, 1 - float(zz) ** 2)), zz])
    rng = np.random.default_rng(9)
    r = rng.normal(0, 1, (6, 3)); r /= np.linalg.norm(r, axis=1, keepdims=True)
    return np.concatenate([np.array(out, F), r.astype(F)])


MIS_FRACTIONS = [0.0, 0.01, 0.5, 0.99, 1.0]
EDGE_WORDS = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]


def cdf_words(rec):
    """Raw words on and next to every entry of the marginal CDF and of the rows that can be picked."""
    ws = set()
    for c in rec[264:272]:
        if 0 < c <= 1:
            ws.update(words_around(c))
    return sorted(ws)


def grid_scripts(rec):
    """Four-word scripts for Grid::sample: row draw, column draw, theta jitter, phi jitter."""
    rng = np.random.default_rng(int(bits(rec[:256]).sum()) % 2**32)
    marg = cdf_words(rec)
    rows = sorted(set(w for c in rec[272:272 + 128] if 0 < c <= 1 for w in words_around(c)))
    out = []
    for w in marg + EDGE_WORDS:
        out.append([w, int(rng.integers(2**32)), int(rng.integers(2**32)), int(rng.integers(2**32))])
    for w in rows + EDGE_WORDS:
        out.append([int(rng.integers(2**32)), w, int(rng.integers(2**32)), int(rng.integers(2**32))])
    for j in EDGE_WORDS:                                             # jitter = 1.0 on the last row / column: theta clamp, phi = 2 pi
        out.append([0xFFFFFFFF, 0xFFFFFFFF, j, j])
        out.append([0xFFFFFFFF, 0, j, 0xFFFFFFFF])
        out.append([0, 0xFFFFFFFF, 0xFFFFFFFF, j])
    for _ in range(24):
        out.append([int(x) for x in rng.integers(0, 2**32, 4)])
    return np.array(out, U32)


def pdf_directions(n):
    """Directions for computePDF about normal n: along it, on the horizon, below it, -n, atan2 at +-pi, random."""
    n = np.asarray(n, np.float64)
    if n[2] < -0.9999999:
        t, b = np.array([0, -1.0, 0]), np.array([-1.0, 0, 0])
    else:
        a = 1 / (1 + n[2]); c = -n[0] * n[1] * a
        t = np.array([1 - n[0] * n[0] * a, c, -n[0]]); b = np.array([c, 1 - n[1] * n[1] * a, -n[1]])
    out = [n, -n, t, -t, b, -b, (t + b) / np.sqrt(2), -t + 1e-7 * b, -t - 1e-7 * b, -t + 0.3 * n, -t - 0.3 * n, n * 0.6 - t * 0.8,
           0.01 * n - t, -0.01 * n + b]
    rng = np.random.default_rng(13)
    r = rng.normal(0, 1, (10, 3)); r /= np.linalg.norm(r, axis=1, keepdims=True)
    d = np.concatenate([np.array(out), r]).astype(F)
    d[2] = F(np.float64(d[2]))
    return d


@pytest.fixture(scope="module")
def cases():
    grids = grid_cases()
    recs = records(grids)
    normals = normal_cases()
    rng = np.random.default_rng(17)
    cos_words = [[a, b] for a in EDGE_WORDS for b in EDGE_WORDS] + [[int(x) for x in rng.integers(0, 2**32, 2)] for _ in range(8)]
    return dict(names=[g[0] for g in grids], recs=recs, normals=normals, cos_words=np.array(cos_words, U32))


# ---- oracle side ----------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data


def po_cosine(n, words):
    out = np.zeros(3, F); n = np.ascontiguousarray(n, F); w = np.ascontiguousarray(words, U32)
    used = oracle_lib().po_sample_cosine_words(_p(n), _p(w), len(w), _p(out))
    return out, used


def po_grid_sample(rec, n, words):
    out = np.zeros(3, F); pdf = C.c_float(); n = np.ascontiguousarray(n, F); w = np.ascontiguousarray(words, U32)
    used = oracle_lib().po_grid_sample(_p(rec), _p(n), _p(w), len(w), _p(out), C.addressof(pdf))
    return out, F(pdf.value), used


def po_sample_mis(rec, n, frac, words):
    out = np.zeros(3, F); wt = C.c_float(); ub = C.c_int(); n = np.ascontiguousarray(n, F); w = np.ascontiguousarray(words, U32)
    used = oracle_lib().po_sample_mis(_p(rec), _p(n), F(frac), _p(w), len(w), _p(out), C.addressof(wt), C.addressof(ub))
    return out, F(wt.value), ub.value, used


# ---- reference side (live) ------------------------------------------------------------------------------------------------
# Every per-call record holds its inputs (in_*, one row per case) next to the reference's answers, so the record describes
# itself and tests/test_gpu_integrator_vs_ref.py replays the same cases through the device hook without the oracle.
def ref_lib():
    from oracle_binding import ref_int_lib
    return ref_int_lib()


def flat_cases(normals, per_normal):
    """The (normal, item) pairs of every normal with every item, normal-major: (normals (m, 3), items (m, ...))."""
    nn = np.repeat(np.asarray(normals, F), len(per_normal), axis=0)
    it = np.concatenate([np.asarray(per_normal)] * len(normals))
    return nn, it


def ask_cosine(inp):
    L = ref_lib(); m = len(inp["in_normal"])
    dirs = np.zeros((m, 3), F); used = np.zeros(m, np.int32)
    for k in range(m):
        n = np.ascontiguousarray(inp["in_normal"][k]); w = np.ascontiguousarray(inp["in_words"][k])
        used[k] = L.ref_sample_cosine_hemisphere(_p(n), _p(w), len(w), _p(dirs[k]))
    return dict(inp, dir=dirs, used=used)


def ask_grid_sample(inp):
    L = ref_lib(); m = len(inp["in_normal"]); rec = np.ascontiguousarray(inp["in_rec"])
    dirs = np.zeros((m, 3), F); pdf = np.zeros(m, F); used = np.zeros(m, np.int32); valid = C.c_int()
    for k in range(m):
        n = np.ascontiguousarray(inp["in_normal"][k]); w = np.ascontiguousarray(inp["in_words"][k]); p = C.c_float()
        used[k] = L.ref_grid_sample(_p(rec), _p(n), _p(w), len(w), _p(dirs[k]), C.addressof(p), C.addressof(valid))
        pdf[k] = p.value
    return dict(inp, dir=dirs, pdf=pdf, used=used, valid=np.int32(valid.value))


def ask_grid_pdf(inp):
    L = ref_lib(); rec = np.ascontiguousarray(inp["in_rec"])
    pdf = [L.ref_grid_pdf(_p(rec), _p(np.ascontiguousarray(d)), _p(np.ascontiguousarray(n))) for n, d in zip(inp["in_normal"], inp["in_dir"])]
    return dict(inp, pdf=np.array(pdf, F))


def ask_sample_mis(inp):
    L = ref_lib(); m = len(inp["in_normal"]); rec = np.ascontiguousarray(inp["in_rec"])
    dirs = np.zeros((m, 3), F); wt = np.zeros(m, F); ub = np.zeros(m, np.int32); used = np.zeros(m, np.int32)
    for k in range(m):
        n = np.ascontiguousarray(inp["in_normal"][k]); w = np.ascontiguousarray(inp["in_words"][k]); a = C.c_float(); b = C.c_int()
        used[k] = L.ref_sample_mis(_p(rec), _p(n), F(inp["in_frac"][0]), _p(w), len(w), _p(dirs[k]), C.addressof(a), C.addressof(b))
        wt[k] = a.value; ub[k] = b.value
    return dict(inp, dir=dirs, weight=wt, used_bsdf=ub, used=used)


def recorded_for(ref, key, ask, inp):
    """ref(key, ...) for the cases `inp`; the record must hold exactly these inputs (else the cases changed: re-record)."""
    r = ref(key, lambda: ask(inp))
    for k, v in inp.items():
        assert np.array_equal(np.asarray(r[k]), np.asarray(v)), f"{key}: the cases' {k} differ from the recorded ones - re-record"
    return r


# ---- per call ---------------------------------------------------------------------------------------------------------------
def test_scripted_state_reproduces_words():
    """po_xorwow_script: the next five raw draws of the state it builds are the script, for random and extreme scripts."""
    L = oracle_lib(); rng = np.random.default_rng(1)
    scripts = [rng.integers(0, 2**32, 5) for _ in range(300)] + [[0] * 5, [0xFFFFFFFF] * 5, [0, 0xFFFFFFFF, 1, 0x80000000, 7]]
    for s in scripts:
        s = np.array(s, U32); st = np.zeros(6, U32); out = np.zeros(5, U32)
        L.po_xorwow_script(_p(s), 5, _p(st))
        L.po_xorwow_next_raw(_p(st), 5, _p(out))
        assert (out == s).all(), (s, out)
    assert word_to_uniform(0xFFFFFFFF) == 1.0 and word_to_uniform(0) == F(2.0 ** -33)


def test_sample_cosine_hemisphere_vs_ref(cases, ref):
    nn, ww = flat_cases(cases["normals"], cases["cos_words"])
    r = recorded_for(ref, "cosine", ask_cosine, dict(in_normal=nn, in_words=ww.astype(U32)))
    for k in range(len(nn)):
        d, used = po_cosine(nn[k], ww[k])
        assert used == r["used"][k] == 2
        assert same_bits(d, r["dir"][k]), (nn[k], ww[k], d, r["dir"][k])


def test_mis_power_heuristic_vs_ref(ref):
    vals = np.array([0.0, -0.0, -1.0, 1e-30, 1e-20, 1e-6, 0.3183099, 1.0, 3.0, 1e19, 1e20, 3e38, np.inf], F)
    pairs = np.array([(a, b) for a in vals for b in vals], F)

    def ask(inp):
        return dict(inp, w=np.array([ref_lib().ref_mis_power_heuristic(a, b) for a, b in inp["in_pairs"]], F))
    r = recorded_for(ref, "mis_power", ask, dict(in_pairs=pairs))
    got = np.array([oracle_lib().po_mis_power_heuristic(a, b) for a, b in pairs], F)
    assert same_bits(got, r["w"])


def test_grid_records_validity(cases):
    """The all-zero grid is the only invalid record (is_valid false -> the integrator's cosine fallback)."""
    valid = cases["recs"][:, 529].view(np.int32)
    assert [n for n, v in zip(cases["names"], valid) if not v] == ["zero"]


def test_grid_sample_vs_ref(cases, ref):
    for name, rec in zip(cases["names"], cases["recs"]):
        nn, ww = flat_cases(cases["normals"], grid_scripts(rec))
        r = recorded_for(ref, f"grid_sample/{name}", ask_grid_sample, dict(in_rec=rec, in_normal=nn, in_words=ww.astype(U32)))
        assert int(np.asarray(r["valid"]).reshape(-1)[0]) == int(rec[529:530].view(np.int32)[0])
        if name == "zero":
            continue                                   # sample() of an invalid grid: its private fallback, unreachable
        for k in range(len(nn)):
            d, pdf, used = po_grid_sample(rec, nn[k], ww[k])
            assert used == r["used"][k] == 4, (name, k)
            assert same_bits(d, r["dir"][k]) and same_bits(pdf, r["pdf"][k]), (name, nn[k], ww[k], d, r["dir"][k], pdf, r["pdf"][k])


def pdf_cases(normals):
    nn = np.concatenate([np.repeat(np.asarray([n], F), len(pdf_directions(n)), axis=0) for n in normals])
    dd = np.concatenate([pdf_directions(n) for n in normals])
    return nn, dd


def test_grid_pdf_vs_ref(cases, ref):
    nn, dd = pdf_cases(cases["normals"])
    for name, rec in zip(cases["names"], cases["recs"]):
        if name == "zero":
            continue                                   # computePDF of an invalid grid: cosinePDF, unreachable from integrator()
        r = recorded_for(ref, f"grid_pdf/{name}", ask_grid_pdf, dict(in_rec=rec, in_normal=nn, in_dir=dd))
        got = [oracle_lib().po_grid_pdf(_p(rec), _p(np.ascontiguousarray(d)), _p(np.ascontiguousarray(n))) for n, d in zip(nn, dd)]
        assert same_bits(np.array(got, F), r["pdf"]), name


def mis_scripts(rec, frac):
    rng = np.random.default_rng(int(frac * 1000) + 7)
    p = max(min(F(frac), F(0.99)), F(0.01))                          # BSDF_PROB
    xis = sorted(set(words_around(p) + EDGE_WORDS))                  # xi == BSDF_PROB exactly, and the floats on either side
    out = []
    for xi in xis:
        for tail in ([int(x) for x in rng.integers(0, 2**32, 4)], [0xFFFFFFFF] * 4, [0, 0, 0xFFFFFFFF, 0xFFFFFFFF]):
            out.append([xi] + tail)
    marg = cdf_words(rec)
    for w in marg[::2]:
        out.append([0xFFFFFFFF, w] + [int(x) for x in rng.integers(0, 2**32, 3)])
    return np.array(out, U32)


def test_sample_mis_vs_ref(cases, ref):
    for name, rec in zip(cases["names"], cases["recs"]):
        if name == "zero":
            continue                                   # integrator() never calls sampleMIS on an invalid grid
        for frac in MIS_FRACTIONS:
            nn, ww = flat_cases(cases["normals"][::2], mis_scripts(rec, frac))
            r = recorded_for(ref, f"sample_mis/{name}/{frac}", ask_sample_mis,
                             dict(in_rec=rec, in_frac=np.array([frac], F), in_normal=nn, in_words=ww.astype(U32)))
            for k in range(len(nn)):
                d, wt, ub, used = po_sample_mis(rec, nn[k], frac, ww[k])
                assert (ub, used) == (r["used_bsdf"][k], r["used"][k]), (name, frac, nn[k], ww[k])
                assert same_bits(d, r["dir"][k]) and same_bits(wt, r["weight"][k]), (name, frac, nn[k], ww[k], wt, r["weight"][k])

# ---- frames -----------------------------------------------------------------------------------------------------------------
def random_soup(seed, n):
    rng = np.random.default_rng(seed)
    types = (rng.random(n) < 0.3).astype(np.int32)
    centers = rng.uniform(-2.5, 2.5, (n, 1, 3)) + np.array([0, 2.5, 0])
    verts = (centers + rng.normal(0, 0.6 if n < 100 else 0.25, (n, 4, 3))).astype(F)
    q = types == 1
    verts[q, 2] = verts[q, 1] + (verts[q, 3] - verts[q, 0])
    normal = rng.normal(0, 1, (n, 3)); normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    bsdf = rng.uniform(0.2, 0.9, (n, 3)); Le = rng.uniform(0, 4, (n, 3)) * (rng.random((n, 1)) < 0.15)
    return types, verts, normal.astype(F), bsdf.astype(F), Le.astype(F)


def scene_arrays(name):
    if name.startswith("soup"):
        return random_soup(int(name[4:]), int(name[4:]))
    base, _, le = name.partition("_Le")
    p = OracleScene.load(os.path.join(SCENES, base + ".obj")).prims()
    arrs = [p["type"], p["verts"], p["normal"], p["bsdf"], p["Le"].copy()]
    if le:                                               # tone-map edges: every emitter's Le replaced
        on = (arrs[4] > 0).any(axis=1)
        arrs[4][on] = F(le)
    return tuple(arrs)


# (scene, width, height, spp, mode).  Le 1e30: c / (c + 1) == 1; Le 3e38: the sum over 16 samples overflows to inf.
FRAMES = [(s, 64, 64, 16, m) for s in ("cbox", "cbox_quads") for m in (BSDF, GRID, MIS)] + [("cbox", 64, 64, 4, BSDF), ("cbox", 32, 32, 3, MIS)] + \
         [(f"soup{n}", 48, 48, 4, m) for n in (7, 65, 3000) for m in (BSDF, MIS)] + \
         [(f"cbox_Le{le}", 32, 32, 16, BSDF) for le in ("0", "1e30", "3e38")]
# spp 3 and 12: color /= float(spp) multiplies by a reciprocal taken in binary64 (vector.h:90-94), which a true division
# matches whenever spp is a power of two
RADIANCE = [("cbox", 64, 64, 16, BSDF, 8), ("cbox", 64, 64, 4, BSDF, 5), ("cbox_quads", 64, 64, 16, MIS, 3),
            ("cbox", 32, 32, 3, BSDF, 5), ("cbox_quads", 32, 32, 12, GRID, 6)]


def frame_id(c):
    return "_".join(str(x) for x in c)


def scene_pair(name, mode):
    """The oracle scene and the arrays + records the reference is given (synthetic radiosity grids in the guided modes)."""
    arrs = scene_arrays(name)
    o = OracleScene.from_arrays(*arrs)
    cdfs = None
    if mode != BSDF:
        o.set_radiosity_grids(synthetic_radiosity_grids(len(arrs[0]), seed=len(arrs[0])))
        cdfs = o.cdfs()
    return o, arrs, cdfs


def ref_frame(ref, case, arrs=None, cdfs=None):
    name, W, H, spp, mode = case
    if arrs is None:
        _, arrs, cdfs = scene_pair(name, mode)
    return ref(f"frame/{frame_id(case)}", lambda: dict(rgb8=RefIntegratorScene(*arrs, cdfs=cdfs).render(default_camera(), W, H, spp, mode)))


def ref_radiance(ref, case, arrs=None, cdfs=None):
    name, W, H, spp, mode, depth = case
    if arrs is None:
        _, arrs, cdfs = scene_pair(name, mode)
    return ref(f"radiance/{frame_id(case)}",
               lambda: dict(radiance=RefIntegratorScene(*arrs, cdfs=cdfs).radiance(default_camera(), W, H, spp, depth, mode)))


@pytest.mark.parametrize("case", FRAMES, ids=frame_id)
def test_render_frame_vs_ref(case, ref):
    name, W, H, spp, mode = case
    o, arrs, cdfs = scene_pair(name, mode)
    cam = default_camera()
    r = ref_frame(ref, case, arrs, cdfs)
    rgb, rad, _ = o.render(cam, W, H, spp, max_depth=5, sampling_mode=mode, seed_base=SEED)
    bad = np.argwhere((rgb != r["rgb8"]).any(axis=2))
    assert len(bad) == 0, f"{len(bad)} pixels differ, first (y, x) {bad[:5].tolist()}"
    if name.endswith("Le3e38"):
        assert np.isinf(rad).any()                     # the overflow edge was reached
    if name.endswith("Le1e30"):
        assert (rgb == 255).any()


@pytest.mark.parametrize("case", RADIANCE, ids=frame_id)
def test_radiance_vs_ref(case, ref):
    name, W, H, spp, mode, depth = case
    o, arrs, cdfs = scene_pair(name, mode)
    cam = default_camera()
    r = ref_radiance(ref, case, arrs, cdfs)
    _, rad, _ = o.render(cam, W, H, spp, max_depth=depth, sampling_mode=mode, seed_base=SEED)
    assert same_bits(rad, r["radiance"])


def test_radiosity_view_vs_ref(ref):
    arrs = scene_arrays("cbox")
    rad = np.random.default_rng(3).uniform(0, 1.5, (len(arrs[0]), 3)).astype(F)
    rad[::4] = 0
    cam = default_camera()
    r = ref("radiosity_view/cbox_48x40_4", lambda: dict(rgb8=RefIntegratorScene(*arrs, radiosity=rad).render_radiosity(cam, 48, 40, 4)))
    o = OracleScene.from_arrays(*arrs)
    o.set_radiosity(rad)
    rgb = o.render_radiosity(cam, 48, 40, 4)[0]
    assert np.array_equal(rgb, r["rgb8"])


def test_raw_grid_fallback_matches_records(ref):
    """initGridFromPrimitive without precomputed CDFs builds the grid from the primitive's raw radiosity grid every sample
    (Grid::initFromRadiosity + buildCDFs).  The product never takes that path (it always uploads the records), but the
    reference frame it gives must be the one of the records."""
    arrs = scene_arrays("cbox")
    grids = synthetic_radiosity_grids(len(arrs[0]), seed=len(arrs[0]))
    cam = default_camera()
    r = ref("raw_grid_fallback/cbox_32x32_8_mis", lambda: dict(rgb8=RefIntegratorScene(*arrs, rad_grids=grids).render(cam, 32, 32, 8, MIS)))
    o = OracleScene.from_arrays(*arrs)
    o.set_radiosity_grids(grids)
    rgb, _, _ = o.render(cam, 32, 32, 8, max_depth=5, sampling_mode=MIS, seed_base=SEED)
    assert np.array_equal(rgb, r["rgb8"])


def test_golden_frames_match_reference(ref):
    """The committed oracle frames whose case is recorded above from the reference: the same bits."""
    checked = 0
    for case in FRAMES:
        name, W, H, spp, mode = case
        path = os.path.join(HERE, "golden", f"frame_{name}_s0c0_{W}x{H}_{spp}spp_d5.npz")
        if mode == BSDF and os.path.exists(path):
            assert np.array_equal(np.load(path)["rgb8"], ref_frame(ref, case)["rgb8"])
            checked += 1
    for case in RADIANCE:
        name, W, H, spp, mode, depth = case
        path = os.path.join(HERE, "golden", f"frame_{name}_s0c0_{W}x{H}_{spp}spp_d{depth}.npz")
        if mode == BSDF and os.path.exists(path):
            assert same_bits(np.load(path)["radiance"], ref_radiance(ref, case)["radiance"])
            checked += 1
    assert checked == 3


def test_tonemap_edges():
    """po_tonemap (the oracle's tone-map, shared by po_render) at the edges whole frames reach: 0, c / (c + 1) == 1, inf
    (inf / inf = NaN, which fminf turns into 1) and NaN."""
    L = oracle_lib()
    out = np.zeros(3, np.uint8)
    for c, want in [((0, 0, 0), (0, 0, 0)), ((1e30, 3e38, 1e8), (255, 255, 255)), ((np.inf, np.inf, 0), (255, 255, 0)),
                    ((np.nan, 0, np.inf), (255, 0, 255))]:
        L.po_tonemap(_p(np.array(c, F)), _p(out))
        assert tuple(out) == want, (c, tuple(out))
