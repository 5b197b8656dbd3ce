"""The launching test hooks (ptmi_debug_*, csrc/c_api_hooks.cpp) at the edges of the sequence they share - check, upload, launch
once, synchronise, download - on one context, cbox.obj at 8 x 8:

  n == 0       the five hooks that accept it return 0 and leave their outputs bit for bit as they were
  refusals     one refused call per hook with a live context returns -1 with the text the library gave before the hooks moved
               onto one launch helper, leaves the outputs as they were, and a valid call of 65 cases right after it returns
               what the same call returned before (65: one full wave and one lane, where a wrong count in the helper shows)
  optional     a buffer the caller leaves out (recs, counts, queue_in) against its counterpart on the same inputs
  shared body  the three bit-sweep checks over 2^16 patterns from 1.0f: no mismatch, first_bad_bits 0

Outputs are preset to a sentinel pattern, so "untouched" and "written in full" are both seen.
"""
import ctypes as C
import os

import numpy as np
import pytest

import ptmi
from oracle_binding import SCENES

pytestmark = pytest.mark.gpu

F, I32, U32, U64, F64 = np.float32, np.int32, np.uint32, np.uint64, np.float64
CBOX = os.path.join(SCENES, "cbox.obj")
N = 65
ONE_BITS = 0x3f800000
SENTINEL = 0xa5
POSITIVE_N, NOT_NEGATIVE_N = b"n must be positive", b"n must not be negative"
COUNT_RANGE = b"count must be in [1, 2^32]"
_CT = {np.dtype(F): C.c_float, np.dtype(I32): C.c_int, np.dtype(U32): C.c_uint32, np.dtype(U64): C.c_uint64, np.dtype(F64): C.c_double}


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(_CT[a.dtype]))


def out(dtype, *shape):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = SENTINEL
    return a


def untouched(outs):
    return all((o.view(np.uint8) == SENTINEL).all() for o in outs)


def same(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    r.load_scene(CBOX, 0)
    r.set_camera(ptmi.default_camera())
    r.update_resolution(8, 8)
    r.set_config(spp=1, max_depth=5)
    r.set_lens(0.05)
    prims = ptmi.HostScene.load(CBOX).prims()
    n_prims = len(prims["type"])
    rng = np.random.default_rng(3)
    t = prims["normal"].astype(F64)[:, None, :] + 0.5 * rng.normal(0, 1, (n_prims, 4, 3))
    r.set_vertex_normals(unit(t))
    r.set_albedo_texture(rng.uniform(0.1, 0.9, (4, 4, 3)).astype(F), rng.uniform(0, 1, (n_prims, 4, 2)).astype(F), None, "bilinear")
    assert r.vertex_normals_info()["n_smooth"] > 0 and r.albedo_texture_info()["n_textured"] > 0      # the table hooks launch
    r.n_prims = n_prims
    r.verts = prims["verts"]
    yield r
    r.close()


class Inputs:
    """the inputs of every hook for n cases, drawn once"""
    def __init__(self, R, n=N):
        rng = np.random.default_rng(7)
        cam = ptmi.default_camera()
        eye, at = np.array(cam.origin, F64), np.array(cam.lookat, F64)
        self.n = n
        self.o = np.tile(eye, (n, 1)).astype(F)
        self.d = unit((at - eye)[None] + 0.2 * rng.normal(0, 1, (n, 3)))
        self.dirs = unit(rng.normal(0, 1, (n, 3)))
        self.normals = unit(rng.normal(0, 1, (n, 3)))
        self.u, self.v = rng.uniform(0, 1, n).astype(F), rng.uniform(0, 1, n).astype(F)
        self.x = rng.uniform(-6, 6, n).astype(F)
        self.live = (rng.uniform(0, 1, n) < 0.8).astype(I32)
        self.states = rng.integers(1, 2 ** 32, (n, 6), dtype=np.uint64).astype(U32)
        self.pixels = rng.integers(0, 64, n).astype(I32)
        self.px, self.py = (self.pixels % 8).astype(I32), (self.pixels // 8).astype(I32)
        self.r4 = rng.uniform(0, 1, (n, 4)).astype(F)
        self.prim = rng.integers(0, R.n_prims, n).astype(I32)
        self.p = R.verts[self.prim, :3].astype(F64).mean(axis=1).astype(F)            # each triangle's centroid
        self.medium = np.zeros((n, ptmi.MEDIUM_CALL_IN), F)                           # HG value: in[15..17] d, in[19] the cosine
        self.medium[:, 8] = 0.3                                                       # a block with g somewhere; op 2 reads what it reads
        self.medium[:, 15:18] = self.dirs; self.medium[:, 19] = rng.uniform(-1, 1, n)
        self.nee = np.zeros((n, 16), F)                                               # SPECULAR: d, n_k, kind, ior, u
        self.nee[:, 0:3] = self.dirs; self.nee[:, 3:6] = self.normals; self.nee[:, 6] = 2.0; self.nee[:, 7] = 1.5; self.nee[:, 8] = self.u
        self.pdf = rng.uniform(0.1, 1, (n, 256)).astype(F)
        self.rgb = rng.uniform(0.1, 1, (n, 256, 3)).astype(F)
        self.cost = rng.integers(0, 1000, n).astype(U32)
        self.queue = rng.permutation(n).astype(I32)
        self.centre = rng.uniform(-1, 1, (n, 3)).astype(F)
        self.ff = rng.uniform(0, 0.1, (n, n)).astype(F)
        self.rad = rng.uniform(0, 1, (n, 3)).astype(F)


@pytest.fixture(scope="module")
def X(R):
    x = Inputs(R)
    x.recs = R.debug_cdf_records(2, x.pdf[:4])
    x.rec_idx = (np.arange(x.n) % 4).astype(I32)
    return x


FLT_MAX = 3.4028234663852886e38


def calls(R, X, n=None):
    """hook -> (outputs, call(**changes)): the valid call of n cases; a change replaces one argument by name"""
    n = X.n if n is None else n
    L, h = R.L, R.h
    table = {}

    def hook(name, outs, order, **args):
        def call(**changes):
            a = dict(args, **changes)
            return getattr(L, "ptmi_debug_" + name)(h, *[ptr(a[k]) if isinstance(a[k], np.ndarray) else a[k] for k in order.split()])
        table[name] = (outs, call)

    o = [out(F, n, 6)]
    hook("lens_ray", o, "n px py r out", n=n, px=X.px, py=X.py, r=X.r4, out=o[0])
    o = [out(F, n, ptmi.MEDIUM_CALL_OUT)]
    hook("medium_call", o, "op n in out", op=ptmi.MEDIUM_HG_VALUE, n=n, **{"in": X.medium}, out=o[0])
    o = [out(I32, n), out(I32, n), out(F, n), out(U64, 2)]
    hook("intersect_fast", o, "n o d t_min t_max hit prim t counts", n=n, o=X.o, d=X.d, t_min=1e-4, t_max=FLT_MAX, hit=o[0], prim=o[1], t=o[2], counts=o[3])
    o = [out(I32, n), out(I32, n), out(F, n)]
    hook("first_hit", o, "n o d t_min hit prim t", n=n, o=X.o, d=X.d, t_min=1e-4, hit=o[0], prim=o[1], t=o[2])
    o = [out(I32, n), out(I32, n), out(F, n), out(F, n, 3), out(F, n, 3)]
    hook("intersect", o, "n o d t_min t_max hit prim t p nrm", n=n, o=X.o, d=X.d, t_min=1e-4, t_max=FLT_MAX, hit=o[0], prim=o[1], t=o[2], p=o[3], nrm=o[4])
    o = [out(F, n, 3)]
    hook("rng", o, "seed n pixels count out", seed=5, n=n, pixels=X.pixels, count=3, out=o[0])
    for name in ("rcp_check", "sqrt_check"):
        o = [out(U64, 1), out(U32, 1)]
        hook(name, o, "first count bad first_bad", first=ONE_BITS, count=n, bad=o[0], first_bad=o[1])
    o = [out(U64, 1), out(U32, 1), out(I32, 1)]
    hook("size_div_check", o, "size first count bad first_bad lean", size=8, first=ONE_BITS, count=n, bad=o[0], first_bad=o[1], lean=o[2])
    o = [out(U64, 1), out(U64, 1), out(U32, 1), out(U64, 1), out(U32, 8), out(I32, 1)]
    hook("sincos_lean_check", o, "first count bs bc first_bad fl kept nk", first=ONE_BITS, count=n, bs=o[0], bc=o[1], first_bad=o[2], fl=o[3], kept=o[4], nk=o[5])
    o = [out(F, n, 3)]
    hook("ray_inv", o, "n d live out", n=n, d=X.dirs, live=X.live, out=o[0])
    o = [out(F, n, 4)]
    hook("sincos_lean", o, "n x live out", n=n, x=X.x, live=X.live, out=o[0])
    o = [out(F, n, 6)]
    hook("unit_voted", o, "n w live out", n=n, w=X.centre, live=X.live, out=o[0])
    o = [out(F, n, 3)]
    hook("cosine_sample", o, "n normals u v out", n=n, normals=X.normals, u=X.u, v=X.v, out=o[0])
    o = [out(F, n, 6), out(I32, n)]
    hook("guided_sample", o, "op n n_recs recs rec_idx normals in3 states out used", op=1, n=n, n_recs=len(X.recs), recs=X.recs, rec_idx=X.rec_idx,
         normals=X.normals, in3=X.dirs, states=X.states, out=o[0], used=o[1])
    o = [out(F64, n, 2)]
    hook("math", o, "op n a b out", op=R.MATH_ATAN2F, n=n, a=X.x, b=X.u, out=o[0])
    o = [out(I32, n)]
    hook("grid_index", o, "n dirs normals out", n=n, dirs=X.dirs, normals=X.normals, out=o[0])
    o = [out(F, n, 16), out(I32, n, 4)]
    hook("nee_call", o, "op n in out_f out_i", op=R.NEE_CALL_SPECULAR, n=n, **{"in": X.nee}, out_f=o[0], out_i=o[1])
    o = [out(F, n, 4)]
    hook("vertex_normal", o, "n prim p out", n=n, prim=X.prim, p=X.p, out=o[0])
    o = [out(F, n, 6)]
    hook("albedo", o, "n prim p out", n=n, prim=X.prim, p=X.p, out=o[0])
    o = [out(I32, n), out(I32, 512)]
    hook("order_by_cost", o, "n queue_in cost n_cost cost_max classes queue_out hist", n=n, queue_in=X.queue, cost=X.cost, n_cost=X.n,
         cost_max=int(X.cost.max()), classes=4, queue_out=o[0], hist=o[1])
    o = [out(F, n, 530)]
    hook("cdf_records", o, "n src_kind src out", n=n, src_kind=2, src=X.pdf, out=o[0])
    o = [out(F, n, 256), out(F, n, 256)]
    hook("filter_pdfs", o, "n rgb counts bilateral ss sr ff rad", n=n, rgb=X.rgb, counts=X.pdf, bilateral=1, ss=1.5, sr=0.3, ff=o[0], rad=o[1])
    o = [out(F, n, 256, 3)]
    hook("radiosity_grid", o, "n centre normal ff rad filtering bilateral ss sr out", n=n, centre=X.centre, normal=X.normals, ff=X.ff, rad=X.rad,
         filtering=0, bilateral=1, ss=1.5, sr=0.3, out=o[0])
    return table


# hook -> (the change that makes the call refused, the refusal's text)
REFUSALS = {
    "lens_ray": (dict(n=-1), NOT_NEGATIVE_N),
    "medium_call": (dict(op=4), b"op must be 0 .. 3"),
    "intersect_fast": (dict(n=0), POSITIVE_N),
    "first_hit": (dict(n=0), POSITIVE_N),
    "intersect": (dict(n=-1), POSITIVE_N),
    "rng": (dict(n=0), b"n_pixels and count must be positive"),
    "rcp_check": (dict(count=0), COUNT_RANGE),
    "sqrt_check": (dict(count=0), COUNT_RANGE),
    "size_div_check": (dict(size=0), b"size must be positive"),
    "sincos_lean_check": (dict(count=0), COUNT_RANGE),
    "ray_inv": (dict(n=0), POSITIVE_N),
    "sincos_lean": (dict(n=0), POSITIVE_N),
    "unit_voted": (dict(n=-1), POSITIVE_N),
    "cosine_sample": (dict(n=0), POSITIVE_N),
    "guided_sample": (dict(rec_idx=np.full(N, 4, I32)), b"record index out of range"),
    "math": (dict(op=99), b"unknown op"),
    "grid_index": (dict(n=0), POSITIVE_N),
    "nee_call": (dict(op=8), b"unknown op"),
    "vertex_normal": (None, b"prim out of range"),             # prim: one entry = n_prims, made in the test
    "albedo": (None, b"prim out of range"),
    "order_by_cost": (dict(queue_in=np.r_[np.arange(N - 1), N].astype(I32)), b"a queue entry lies outside cost[]"),
    "cdf_records": (dict(src_kind=3), b"src_kind must be 0, 1 or 2"),
    "filter_pdfs": (dict(n=0), POSITIVE_N),
    "radiosity_grid": (dict(n=0), POSITIVE_N),
}


def fresh(outs):
    for o in outs:
        o.view(np.uint8)[...] = SENTINEL


def test_every_launching_hook_is_covered(R, X):
    launching = {n[len("ptmi_debug_"):] for n in ptmi.EXPORTS if n.startswith("ptmi_debug_")} - {
        "lens_block", "place_tiles", "set_traversal", "get_traversal", "set_solver_walk", "set_packed_min_nodes", "set_packed_top",
        "set_fast_tree", "set_temporal_moments", "set_filter_inputs", "accum_step"}            # state-setting hooks and the plain copy
    assert launching == set(calls(R, X)) == set(REFUSALS)


@pytest.mark.parametrize("name", ["nee_call", "vertex_normal", "albedo", "lens_ray", "medium_call"])
def test_no_cases_write_nothing(R, X, name):
    outs, call = calls(R, X)[name]
    assert call(n=0) == 0, R.L.ptmi_last_error()
    assert untouched(outs)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_a_refusal_leaves_outputs_and_the_next_call_alone(R, X, name):
    outs, call = calls(R, X)[name]
    change, text = REFUSALS[name]
    if change is None:
        bad = X.prim.copy(); bad[N - 1] = R.n_prims
        change = dict(prim=bad)
    assert call() == 0, R.L.ptmi_last_error()
    assert not any((o.view(np.uint8) == SENTINEL).all() for o in outs), "an output was not written"
    before = [o.copy() for o in outs]
    fresh(outs)
    assert call(**change) == -1 and R.L.ptmi_last_error() == text, R.L.ptmi_last_error()
    assert untouched(outs)
    assert call() == 0, R.L.ptmi_last_error()
    assert same(outs, before)


def test_table_hooks_without_a_table_answer_on_the_host(R, X):
    """no launch: the stored normal with flag 0, and (0, 0, 1, 1, 1, 0)"""
    fresh_r = ptmi.Renderer(0)
    try:
        fresh_r.load_scene(CBOX, 0)
        stored = ptmi.HostScene.load(CBOX).prims()["normal"]
        vn = fresh_r.debug_vertex_normal(X.prim, X.p)
        assert np.array_equal(vn[:, :3].view(U32), stored[X.prim].astype(F).view(U32)) and (vn[:, 3] == 0).all()
        assert np.array_equal(fresh_r.debug_albedo(X.prim, X.p), np.tile(np.array([0, 0, 1, 1, 1, 0], F), (N, 1)))
    finally:
        fresh_r.close()


def test_optional_buffers(R, X):
    tab = calls(R, X)
    # guided_sample op 0 (the cosine lobe) reads no record: without recs as with them
    outs, call = tab["guided_sample"]
    assert call(op=0) == 0
    with_recs = [o.copy() for o in outs]; fresh(outs)
    assert call(op=0, n_recs=0, recs=None, rec_idx=None) == 0 and same(outs, with_recs)
    fresh(outs)
    assert call(op=1, n_recs=0, recs=None, rec_idx=None) == -1 and R.L.ptmi_last_error() == b"ops 1-3 need CDF records and their indices"
    assert untouched(outs)
    # filter_pdfs: counts = NULL is a form-factor pdf of +0 everywhere, and the radiosity pdf does not read them
    outs, call = tab["filter_pdfs"]
    assert call() == 0
    with_counts = [o.copy() for o in outs]; fresh(outs)
    assert call(counts=None) == 0
    assert (outs[0].view(U32) == 0).all() and same(outs[1:], with_counts[1:]) and with_counts[0].any()
    # order_by_cost: queue_in = NULL is the identity queue
    outs, call = tab["order_by_cost"]
    assert call(queue_in=np.arange(N, dtype=I32)) == 0
    identity = [o.copy() for o in outs]; fresh(outs)
    assert call(queue_in=None) == 0 and same(outs, identity)
    assert sorted(outs[0].tolist()) == list(range(N)) and outs[1][:256].sum() == N and outs[1][256:].max() == N   # counts; class ends
    fresh(outs)
    assert call(queue_in=None, n_cost=N - 1) == -1 and R.L.ptmi_last_error() == b"the identity queue needs n <= n_cost" and untouched(outs)
    # intersect_fast: the counters are downloaded only where asked for, start at zero, and do not change the hits
    outs, call = tab["intersect_fast"]
    assert call() == 0
    counted = [o.copy() for o in outs]; fresh(outs)
    assert call(counts=None) == 0
    assert same(outs[:3], counted[:3]) and untouched(outs[3:])
    assert counted[3][0] >= N and counted[3][1] > 0 and counted[0].any()                      # every ray visits the root; some hit
    assert call() == 0 and same(outs, counted)                                                # zeroed again, not added up


def test_vote_hooks_write_zero_where_a_lane_is_not_live(R, X):
    tab = calls(R, X)
    for name in ("sincos_lean", "unit_voted"):
        outs, call = tab[name]
        assert call() == 0
        assert (outs[0].view(U32)[X.live == 0] == 0).all() and outs[0][X.live != 0].any(axis=1).all(), name


def test_bit_sweeps_share_one_body(R):
    """2^16 patterns from 1.0f: each check runs its own kernel - no mismatch, and first_bad_bits is 0 where there is none"""
    assert R.debug_rcp_check(ONE_BITS, 1 << 16) == (0, 0)
    assert R.debug_sqrt_check(ONE_BITS, 1 << 16) == (0, 0)
    assert R.debug_size_div_check(8, ONE_BITS, 1 << 16) == (0, 0, True)
    assert R.debug_size_div_check(7, ONE_BITS, 1 << 16) == (0, 0, True)
    assert R.debug_size_div_check((1 << 23) + 1, ONE_BITS, 1 << 16) == (0, 0, False)      # above 2^23 the size keeps the IEEE division
    bs, bc, first, fl, kept = R.debug_sincos_lean_check(ONE_BITS, 1 << 16)
    assert (bs, bc, first) == (0, 0, 0) and len(kept) == min(fl, 8)
