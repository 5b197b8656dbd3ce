"""The one path loop of tests/path_oracle.py against the four separate loops it replaced (NeeRenderer.sample, EnvRenderer.sample,
SpecRenderer.sample, RoughRenderer.sample, each a copy of the one before), bit for bit: tests/golden/restatement_pinned.npz holds
what the four classes gave at the commit before the loops were merged.  No GPU.

A case runs through RoughRenderer and through every narrower constructor that can express it, each against its own record: the
colour sums of two consecutive frames (the streams carry over), the final streams, and - for the two classes that kept them then,
SpecRenderer and RoughRenderer - samples, draws, cut and the trace.  Together the cases reach every line of PathRenderer.sample but
one (a sys.settrace line tracer over this file's cases): the exit for a rough BSDF sample whose direction has no finite length,
which finite input cannot reach - a vertex that passes the grazing test has a finite frame, and a sample below the horizon or with
a NaN half vector ends one line earlier.

The fixture is never recorded from path_oracle.py: `python tests/test_restatement_pinned.py record PATH`, run in a checkout of the
commit before it with this one file copied in, takes the four names from the modules they lived in and stores that commit's hash."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PYTHON = os.path.join(os.path.dirname(HERE), "cuda-pathtracer_amd", "python")
if PYTHON not in sys.path:                                   # run as a script (the __main__ block below), nothing else has put it there
    sys.path.insert(0, PYTHON)

import env_scenes as ES
import furnace as FN
import ptmi_scenes
import rough_scenes as RS
import specular_scenes as SS
from oracle_binding import OracleScene, SCENES, default_camera, rng_stream

F = np.float32
FIXTURE = os.path.join(HERE, "golden", "restatement_pinned.npz")
W = H = 8
SPP, FRAMES = 2, 2
COUNTED = ("SpecRenderer", "RoughRenderer")                  # the classes that kept samples, draws, cut and trace before the merge
# The stream of seed TIE_SEED, subsequence 0 (pixel 0 under seed_base = TIE_SEED) draws exactly 0.95f, the roulette's cap, as its
# draw TIE_DRAW, and nothing above it from draw 2 on: in a box of white mirrors, where a vertex draws nothing but the roulette's
# number, that is the roulette of depth TIE_DRAW + 1, and the path goes on only if the test is u > rr.  One draw in 1.7e7 is such
# a tie; seeds were searched upwards from 0 for the first one within a sample's first 13 roulette draws.
TIE_SEED, TIE_DRAW = 1745464, 10


def constructors():
    """the four names: path_oracle's; before it existed (where the fixture is recorded), the module each lived in"""
    try:
        import path_oracle as PO
        return {n: getattr(PO, n) for n in ("NeeRenderer", "EnvRenderer", "SpecRenderer", "RoughRenderer")}
    except ImportError:
        from env_oracle import EnvRenderer
        from nee_oracle import NeeRenderer
        from rough_oracle import RoughRenderer
        from specular_oracle import SpecRenderer
        return dict(NeeRenderer=NeeRenderer, EnvRenderer=EnvRenderer, SpecRenderer=SpecRenderer, RoughRenderer=RoughRenderer)


def small_sky():
    return ES.random_map(7, 5, 12)


def obj(name):
    o = OracleScene.load(os.path.join(SCENES, name))
    return o, o.prims()


def zero_normal_furnace():
    """specular_scenes.black_furnace with a zero stored normal on mirror and on glass primitives: scatter gives a NaN direction"""
    s, kind = SS.black_furnace()
    arrays = list(s.arrays())
    arrays[2][np.flatnonzero(kind == SS.MIRROR)[:2]] = 0.0
    arrays[2][np.flatnonzero(kind == SS.GLASS)[:4]] = 0.0
    return OracleScene.from_arrays(*arrays), kind


def mirror_box():
    """furnace.box, every wall a white mirror that emits: a path ends by the roulette or by max_depth alone"""
    s = FN.box(FN.Scene(rho=SS.WHITE, le=FN.LE))
    return OracleScene.from_arrays(*s.arrays()), np.full(len(s), SS.MIRROR, np.int32)


def build(name):
    """a case by name: (scene, kind, roughness, map, depth, further keywords); kind None: no table, map None: no map"""
    return build_scene(name) + (dict(seed_base=TIE_SEED) if name == "roulette_tie" else {},)


def build_scene(name):
    part = name.split("-")
    if name == "roulette_tie":
        o, kind = mirror_box()
        return o, kind, None, None, 16
    if part[0] == "blocks":                                  # cbox, the short block glass and the tall one rough: -sky / -dark, -d<depth>
        o, p = obj("cbox.obj")
        return o, RS.blocks(p), None, small_sky() if part[1] == "sky" else None, int(part[2][1:])
    if part[0] == "mirror_glass":                            # cbox with cornell_blocks: no kind 3
        o, p = obj("cbox.obj")
        return o, ptmi_scenes.cornell_blocks(p), 0.7, small_sky() if part[1] == "sky" else None, 8
    if name == "quads":
        o, p = obj("cbox_quads.obj")
        return o, RS.blocks(p), 0.7, small_sky(), 5
    if name == "plain":                                      # no table, no map: next-event estimation as it began
        return obj("cbox.obj")[0], None, None, None, 5
    if name == "zero_map":                                   # total 0: a map that is looked up but never sampled
        return obj("cbox.obj")[0], None, None, np.zeros((4, 8, 3), F), 5
    if name == "soup":
        arrays = ES.soup()
        kind, rough = RS.soup_table(len(arrays[0]))
        return OracleScene.from_arrays(*arrays), kind, rough, small_sky(), 5
    if part[0] == "soup_dark":                               # no emitter: q = 1 with the map, no light at all without
        return OracleScene.from_arrays(*ES.soup(emitters=False)), None, None, small_sky() if part[1] == "sky" else None, 5
    if name == "furnace":
        arrays, kind = RS.rough_furnace(zero_normals=2, scale_normals=True)
        return OracleScene.from_arrays(*arrays), kind, 0.4, None, 8
    if name == "zero_normals":
        o, kind = zero_normal_furnace()
        return o, kind, None, None, 8
    raise KeyError(name)


CASES = ([f"blocks-{sky}-d{depth}" for sky in ("dark", "sky") for depth in (1, 3, 8)]
         + ["mirror_glass-sky", "mirror_glass-dark", "quads", "plain", "zero_map", "soup", "soup_dark-sky", "soup_dark-dark", "furnace",
            "zero_normals", "roulette_tie"])
NO_ROUGH = ("mirror_glass-sky", "mirror_glass-dark", "zero_normals", "roulette_tie")          # a table without a kind 3: SpecRenderer's too
NO_TABLE = ("plain", "zero_map", "soup_dark-sky", "soup_dark-dark")          # SpecRenderer's and EnvRenderer's too
NO_MAP = ("plain", "soup_dark-dark")                                         # and, with next_event on, NeeRenderer's


def runs():
    """(case, next_event, constructor) of every run"""
    out = []
    for case in CASES:
        for next_event in (False, True):
            names = ["RoughRenderer"]
            if case in NO_ROUGH or case in NO_TABLE:
                names.append("SpecRenderer")
            if case in NO_TABLE:
                names.append("EnvRenderer")
            if case in NO_MAP and next_event:
                names.append("NeeRenderer")
            out += [(case, next_event, n) for n in names]
    return out


def run(case, next_event, name):
    """the case through the constructor `name`: dict of arrays"""
    o, kind, rough, env, depth, prm = build(case)
    ctor, cam = constructors()[name], default_camera()
    if name == "RoughRenderer":
        r = ctor(o, cam, W, H, kind, None, rough, env, next_event, **prm)
    elif name == "SpecRenderer":
        r = ctor(o, cam, W, H, kind, None, env, next_event, **prm)
    elif name == "EnvRenderer":
        r = ctor(o, cam, W, H, env, next_event, **prm)
    else:
        r = ctor(o, cam, W, H, **prm)
    if name in COUNTED:
        r.trace = []
    out = {f"sums{k}": r.sums(SPP, depth) for k in range(FRAMES)}
    out["rng"] = r.rng.copy()
    if name in COUNTED:
        out["counts"] = np.array([r.samples, r.draws, r.cut], np.int64)
        out["trace"] = np.array(r.trace, np.uint8).reshape(-1, 3)
        assert np.array_equal(out["trace"], np.array(r.trace, np.int64).reshape(-1, 3))
    return out


def key(case, next_event, name):
    return f"{case}/{int(next_event)}/{name}"


@pytest.fixture(scope="module")
def pinned():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case,next_event,name", runs(), ids=lambda v: str(int(v)) if isinstance(v, bool) else v)
def test_the_loop_gives_what_the_separate_loops_gave(pinned, case, next_event, name):
    got = run(case, next_event, name)
    prefix = key(case, next_event, name) + "/"
    assert {k[len(prefix):] for k in pinned if k.startswith(prefix)} == set(got)
    for k, a in got.items():
        e = pinned[prefix + k]
        assert a.dtype == e.dtype and a.shape == e.shape, k
        if a.dtype == F:
            a, e = a.view(np.uint32), e.view(np.uint32)
        assert np.array_equal(a, e), (k, int((a != e).sum()))


def test_the_tie_case_draws_the_roulette_cap():
    u, _ = rng_stream(TIE_SEED, 0, TIE_DRAW + 1)
    assert u[TIE_DRAW] == F(0.95) and (u[2:TIE_DRAW] < F(0.95)).all()


def test_the_fixture_holds_these_runs_and_no_others(pinned):
    assert {k.rsplit("/", 1)[0] for k in pinned if k != "parent"} == {key(*r) for r in runs()}
    assert len(str(pinned["parent"])) == 40
    assert os.path.getsize(FIXTURE) < 256 * 1024


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "record":
        sys.exit("usage: test_restatement_pinned.py record PATH")
    if "path_oracle" in {c.__module__ for c in constructors().values()}:
        sys.exit("record the fixture at the commit before tests/path_oracle.py, never from the merged loop")
    data = {"parent": np.array(subprocess.check_output(["git", "-C", HERE, "rev-parse", "HEAD"], text=True).strip())}
    for r in runs():
        data.update({f"{key(*r)}/{k}": a for k, a in run(*r).items()})
    np.savez_compressed(sys.argv[2], **data)
    print(f"{len(runs())} runs, {os.path.getsize(sys.argv[2])} bytes")
