"""GPU per-call sampling and GPU frames against the REFERENCE's own integrator, as recorded in tests/golden/ref_integrator.npz by
tests/test_integrator_vs_ref.py (the reference compiled on the CPU: oracle/ref_integrator_harness.cpp).  Bit-exact: rgb8 of
render() (depth 5, tone-mapped) and the radiance of integrator() at other depths, for BSDF, GRID and MIS sampling, random
soups, tone-map edges (Le 0, c / (c + 1) == 1, an inf sample sum) and the Radiosity view.  Per call, the recorded cases
(inputs and answers, scripted raw draws at the CDF entries, xi == BSDF_PROB, the clamps and the frame's branch) are replayed
through ptmi_debug_guided_sample, which runs the bounce kernels' own device functions.  Reads only the record: no reference
tree is needed here.
"""
import numpy as np
import pytest

import ptmi
from guided_fixtures import synthetic_radiosity_grids
from test_integrator_vs_ref import BSDF, FRAMES, GOLDEN, RADIANCE, frame_id, scene_arrays

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(GOLDEN))


def xorwow_script(words):
    """A XORWOW state (v0..v4, d = 0) whose next raw outputs are `words` (at most 5; the rest 0): the i-th draw returns
    x[4+i] + i * 362437 with x[k+5] = f(x[k+4]) ^ g(x[k]), f(x) = x ^ (x << 4), g(x) = t ^ (t << 1), t = x ^ (x >> 2)."""
    M = 0xFFFFFFFF

    def inv_shl(y, k):
        x = y
        for s in range(k, 32, k):
            x ^= (y << s) & M
        return x

    def inv_shr(y, k):
        x = y
        for s in range(k, 32, k):
            x ^= y >> s
        return x

    f = lambda x: (x ^ (x << 4)) & M
    g_inv = lambda y: inv_shr(inv_shl(y, 1), 2)
    w = [int(v) for v in words] + [0] * (5 - len(words))
    x = [0] * 5 + [(w[i] - (i + 1) * 362437) & M for i in range(5)]
    x[4] = g_inv(x[9] ^ f(x[8]))
    for k in range(4):
        x[k] = g_inv(x[5 + k] ^ f(x[4 + k]))
    return x[:5] + [0]


def states_of(words):
    return np.array([xorwow_script(w) for w in words], np.uint32)


def xorwow_raw(st, n):
    st = [int(v) for v in st]; out = []
    for _ in range(n):
        t = st[0] ^ (st[0] >> 2)
        st = st[1:5] + [((st[4] ^ (st[4] << 4)) ^ (t ^ (t << 1))) & 0xFFFFFFFF] + [(st[5] + 362437) & 0xFFFFFFFF]
        out.append((st[4] + st[5]) & 0xFFFFFFFF)
    return out


def test_script_states_reproduce_words():
    rng = np.random.default_rng(2)
    for w in [list(rng.integers(0, 2**32, 5)) for _ in range(200)] + [[0] * 5, [0xFFFFFFFF] * 5]:
        assert xorwow_raw(xorwow_script(w), 5) == [int(v) for v in w]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def keys(recorded, prefix):
    return sorted({k[:k.rindex("/")] for k in recorded if k.startswith(prefix + "/")})


def test_gpu_cosine_per_call(R, recorded):
    r = {k: recorded[f"cosine/{k}"] for k in ("in_normal", "in_words", "dir", "used")}
    out, used = R.debug_guided_sample(R.GUIDED_COSINE, r["in_normal"], np.zeros_like(r["in_normal"]), states_of(r["in_words"]))
    assert (used == r["used"]).all()
    bad = np.flatnonzero((bits(out[:, :3]) != bits(r["dir"])).any(axis=1))
    assert len(bad) == 0, [(r["in_normal"][k], r["in_words"][k]) for k in bad[:5]]


def test_gpu_grid_sample_per_call(R, recorded):
    for key in keys(recorded, "grid_sample"):
        r = {k: recorded[f"{key}/{k}"] for k in ("in_rec", "in_normal", "in_words", "dir", "pdf", "used", "valid")}
        if not int(np.asarray(r["valid"]).reshape(-1)[0]):
            continue                                   # the integrator never samples an invalid grid
        m = len(r["in_normal"])
        out, used = R.debug_guided_sample(R.GUIDED_GRID_SAMPLE, r["in_normal"], np.zeros((m, 3), F), states_of(r["in_words"]),
                                          recs=r["in_rec"][None], rec_idx=np.zeros(m, np.int32))
        assert (used == r["used"]).all(), key
        bad = np.flatnonzero((bits(out[:, :4]) != bits(np.concatenate([r["dir"], r["pdf"][:, None]], axis=1))).any(axis=1))
        assert len(bad) == 0, (key, [(r["in_normal"][k], r["in_words"][k]) for k in bad[:5]])


def test_gpu_grid_pdf_per_call(R, recorded):
    for key in keys(recorded, "grid_pdf"):
        r = {k: recorded[f"{key}/{k}"] for k in ("in_rec", "in_normal", "in_dir", "pdf")}
        m = len(r["in_normal"])
        out, _ = R.debug_guided_sample(R.GUIDED_GRID_PDF, r["in_normal"], r["in_dir"], np.zeros((m, 6), np.uint32),
                                       recs=r["in_rec"][None], rec_idx=np.zeros(m, np.int32))
        bad = np.flatnonzero(bits(out[:, 3]) != bits(r["pdf"]))
        assert len(bad) == 0, (key, [(r["in_normal"][k], r["in_dir"][k]) for k in bad[:5]])


def test_gpu_sample_mis_per_call(R, recorded):
    n_keys = 0
    for key in keys(recorded, "sample_mis"):
        r = {k: recorded[f"{key}/{k}"] for k in ("in_rec", "in_frac", "in_normal", "in_words", "dir", "weight", "used_bsdf", "used")}
        m = len(r["in_normal"])
        in3 = np.zeros((m, 3), F); in3[:, 0] = r["in_frac"][0]
        out, used = R.debug_guided_sample(R.GUIDED_MIS, r["in_normal"], in3, states_of(r["in_words"]),
                                          recs=r["in_rec"][None], rec_idx=np.zeros(m, np.int32))
        assert (used == r["used"]).all() and ((used == 3) == (r["used_bsdf"] != 0)).all(), key   # BSDF branch: xi, u, v
        bad = np.flatnonzero((bits(out[:, :4]) != bits(np.concatenate([r["dir"], r["weight"][:, None]], axis=1))).any(axis=1))
        assert len(bad) == 0, (key, [(r["in_normal"][k], r["in_words"][k]) for k in bad[:5]])
        n_keys += 1
    assert n_keys == 8 * 5                              # every valid grid at every MIS fraction


def test_gpu_mis_power_heuristic_per_call(R, recorded):
    pairs, want = recorded["mis_power/in_pairs"], recorded["mis_power/w"]
    m = len(pairs)
    in3 = np.zeros((m, 3), F); in3[:, :2] = pairs
    out, _ = R.debug_guided_sample(R.GUIDED_MIS_WEIGHT, np.zeros((m, 3), F), in3, np.zeros((m, 6), np.uint32))
    nan = np.isnan(want)                                # inf / inf: any NaN (its sign and payload are the hardware's)
    assert (np.isnan(out[:, 3]) == nan).all() and (bits(out[~nan, 3]) == bits(want[~nan])).all()


def test_gpu_tonemap_per_call(R):
    """resolve_pixel (the frame resolve's and the denoiser's tone-map) at the edges - 0, c / (c + 1) == 1, inf (inf / inf is
    NaN, which fminf turns into 1), NaN - and against the oracle's tone-map, which the reference frames pin, elsewhere."""
    from oracle_binding import oracle_lib
    edges = np.array([[0, 0, 0], [1e30, 3e38, 1e8], [np.inf, np.inf, 0], [np.nan, 0, np.inf]], F)
    want_edges = np.array([[0, 0, 0], [255, 255, 255], [255, 255, 0], [255, 0, 255]], np.uint8)
    rng = np.random.default_rng(4)
    spread = np.concatenate([rng.uniform(0, 1, (200, 3)), 10.0 ** rng.uniform(-8, 8, (200, 3))]).astype(F)
    cols = np.concatenate([edges, spread])
    m = len(cols)
    out, _ = R.debug_guided_sample(R.GUIDED_TONEMAP, np.zeros((m, 3), F), cols, np.zeros((m, 6), np.uint32))
    rgb = out[:, :3].astype(np.uint8)
    assert (bits(out[:, 3:6]) == bits(cols)).all()                        # radiance = colour x 1
    assert (rgb[:4] == want_edges).all(), rgb[:4]
    want = np.zeros(3, np.uint8)
    for k in range(4, m):
        oracle_lib().po_tonemap(cols[k].ctypes.data, want.ctypes.data)
        assert (rgb[k] == want).all(), (cols[k], rgb[k], want)


def render(R, name, W, H, spp, mode, depth):
    arrs = scene_arrays(name)
    R.load_scene_arrays(*arrs)
    R.set_radiosity_grids(None if mode == BSDF else synthetic_radiosity_grids(len(arrs[0]), seed=len(arrs[0])))
    R.update_resolution(W, H)
    R.set_config(spp=spp, max_depth=depth, seed_base=2023, sampling_mode=mode, mis_bsdf_fraction=0.5, integrator=0)
    R.render_frame()
    return R.read_image()                               # one GPU: the local rows are the whole frame


@pytest.mark.parametrize("case", FRAMES, ids=frame_id)
def test_gpu_frame_is_the_references(R, recorded, case):
    name, W, H, spp, mode = case
    rgb, _ = render(R, name, W, H, spp, mode, 5)
    want = recorded[f"frame/{frame_id(case)}/rgb8"]
    bad = np.argwhere((rgb != want).any(axis=2))
    assert len(bad) == 0, f"{len(bad)} pixels differ, first (y, x) {bad[:5].tolist()}"


@pytest.mark.parametrize("case", RADIANCE, ids=frame_id)
def test_gpu_radiance_is_the_references(R, recorded, case):
    name, W, H, spp, mode, depth = case
    _, rad = render(R, name, W, H, spp, mode, depth)
    want = recorded[f"radiance/{frame_id(case)}/radiance"]
    assert np.array_equal(np.ascontiguousarray(rad, F).view(np.uint32), want.view(np.uint32))


def test_gpu_radiosity_view_is_the_references(R, recorded):
    arrs = scene_arrays("cbox")
    rad = np.random.default_rng(3).uniform(0, 1.5, (len(arrs[0]), 3)).astype(F)   # as test_radiosity_view_vs_ref
    rad[::4] = 0
    R.load_scene_arrays(*arrs)
    R.set_radiosity_grids(None)
    R.set_radiosity(rad)
    R.update_resolution(48, 40)
    R.set_config(spp=4, seed_base=2023, integrator=1)
    try:
        R.render_frame()
        rgb, _ = R.read_image()
    finally:
        R.set_config(integrator=0)
    assert np.array_equal(rgb, recorded["radiosity_view/cbox_48x40_4/rgb8"])
