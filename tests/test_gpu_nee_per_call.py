"""The light and surface sampling functions of the next-event kernel on the device, per call: ptmi_debug_nee_call runs the
kernel's own functions (csrc/light_sample.h, csrc/rough.h; debug_hooks.hip, the kernel's flags) on the cases of
tests/nee_call_sets.py against the context's own device tables, and every float must equal the float32 restatement of the
contract (tests/nee_call_oracle.py) bit for bit, every index and verdict exactly.  Outputs a function leaves undefined behind a
false verdict are not compared; the verdict always is.  (assert_same_bits counts two NaNs as equal: sign and payload of a NaN
are the hardware's.  A NaN only ever stands where the contract's own arithmetic makes one - a zero stored normal, a light
sample on the vertex itself - and there the verdict beside it is compared.)  Each op runs once on its full set, whose length
is no multiple of the block, and once with n = 1.  tests/test_nee_call_sets_host.py shows what the sets reach.
"""
import numpy as np
import pytest

import env_oracle as EO
import nee_call_oracle as O
import nee_call_sets as S
import ptmi
from bit_compare import assert_same_bits

pytestmark = pytest.mark.gpu
F = np.float32
M = ptmi.Renderer


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.close()


def compare(name, R, op, rows, want):
    """the full set, then its last case alone"""
    wf, wk, defined = want
    assert len(rows) % 256 != 0
    for sel in (slice(None), slice(len(rows) - 1, len(rows))):
        f, k = R.debug_nee_call(op, rows[sel])
        bad = np.flatnonzero((k != wk[sel]).any(axis=1))
        assert len(bad) == 0, f"{name}: indices / verdicts of {len(bad)} of {len(k)} cases differ\n" + "\n".join(
            f"in {rows[sel][i].view(np.uint32)}: device {k[i]} host {wk[sel][i]}" for i in bad[:5])
        assert_same_bits(name, np.where(defined[sel], f, F(0)), np.where(defined[sel], wf[sel], F(0)), *rows[sel].T)
    return len(rows)


def env_cases():
    """(name, map, rotation, the restatement's table) of every map of the sets, unrotated and rotated"""
    for name, rgb in S.env_maps().items():
        for rot in S.ROTATIONS:
            yield f"{name} rot {rot}", rgb, rot, EO.table(rgb, 1.0, rot)


def test_env_lookup(R):
    """env_texel: rows and columns of a direction (the row search, the clamps of d.y and of t * w, the poles, the seam)"""
    n = 0
    for name, rgb, rot, tab in env_cases():
        R.set_environment(rgb, rotation_deg=rot)
        d = S.env_lookup_set(tab)
        n += compare(f"env_texel {name}", R, M.NEE_CALL_ENV_LOOKUP, d, O.env_lookup(tab, d))
    R.set_environment(None)
    assert n > 20000


def test_env_sample(R):
    """the environment's light sample: the two CDF searches (entries hit exactly, flat runs, texels of weight 0) and the direction
    built from r3, r4"""
    n = 0
    for name, rgb, rot, tab in env_cases():
        R.set_environment(rgb, rotation_deg=rot)
        u = S.env_sample_set(tab)
        n += compare(f"env_sample {name}", R, M.NEE_CALL_ENV_SAMPLE, u, O.env_sample(tab, u))
    R.set_environment(None)
    assert n > 20000


def load(R, how):
    if how[0] == "file":
        R.load_scene(how[1])
    else:
        R.load_scene_arrays(*how[1])


def test_emitter_sample(R):
    """emitter_select, sample_uniform (triangles and quads), the area-to-solid-angle density and its guards on the device's own
    emitter table of three scenes; the array scene with an environment too, where p_l is scaled by 1 - q"""
    n = 0
    for name, (how, osc) in S.emitter_scenes().items():
        load(R, how)
        et = S.EmitterTable(osc)
        idx = R.scene_bvh()["indices"]
        slot_of = np.zeros(len(idx), np.int32); slot_of[idx] = np.arange(len(idx))
        rows = S.emitter_set(et)
        R.set_environment(None)
        n += compare(f"emitter_sample {name}", R, M.NEE_CALL_EMITTER_SAMPLE, rows, O.emitter_sample(et, slot_of, rows))
        if name == "array":
            R.set_environment(S.env_maps()["1x7"], select_fraction=0.375)
            omq = F(F(1.0) - F(0.375))
            n += compare(f"emitter_sample {name} with an environment", R, M.NEE_CALL_EMITTER_SAMPLE, rows, O.emitter_sample(et, slot_of, rows, omq))
            R.set_environment(None)
    assert n > 9000


def test_specular_vertex(R):
    """the mirror / glass vertex: Fresnel, total internal reflection at the float where s2 reaches 1, ior 1, the draw against F,
    stored normals of any length, the length test"""
    rows = S.specular_set()
    assert compare("specular_vertex", R, M.NEE_CALL_SPECULAR, rows, O.specular(rows)) > 9000


def test_rough_vertex(R):
    rows = S.rough_vertex_set()
    assert compare("rough_vertex", R, M.NEE_CALL_ROUGH_VERTEX, rows, O.rough_vertex(rows)) > 4000


def test_rough_eval(R):
    rows = S.rough_eval_set()
    assert compare("rough_eval", R, M.NEE_CALL_ROUGH_EVAL, rows, O.rough_eval(rows)) > 9000


def test_rough_sample(R):
    rows = S.rough_sample_set()
    assert compare("rough_sample", R, M.NEE_CALL_ROUGH_SAMPLE, rows, O.rough_sample(rows)) > 9000


def test_light_weight(R):
    """light_weight<0> (the cosine lobe whatever the vertex) and light_weight<2> (the GGX lobe at a rough vertex)"""
    rows = S.light_weight_set()
    assert compare("light_weight", R, M.NEE_CALL_LIGHT_WEIGHT, rows, O.light_weight(rows)) > 9000


def test_the_hook_checks_its_arguments(R):
    L = ptmi.lib()
    a = np.zeros((4, M.NEE_CALL_IN), F); f = np.zeros((4, M.NEE_CALL_OUT_F), F); k = np.zeros((4, M.NEE_CALL_OUT_I), np.int32)
    call = lambda op, n, i=a, o=f, q=k: L.ptmi_debug_nee_call(R.h, op, n, None if i is None else i.ctypes.data,
                                                              None if o is None else o.ctypes.data, None if q is None else q.ctypes.data)
    err = lambda: L.ptmi_last_error().decode()
    R.set_environment(None)
    R.load_scene_arrays(*S.array_scene())
    assert call(M.NEE_CALL_SPECULAR, 4) == 0 and call(M.NEE_CALL_SPECULAR, 0) == 0
    assert call(M.NEE_CALL_SPECULAR, -1) == -1 and "n must" in err()
    assert call(8, 4) == -1 and "op" in err()
    assert call(-1, 4) == -1 and "op" in err()
    for args in ((None, f, k), (a, None, k), (a, f, None)):
        assert call(M.NEE_CALL_SPECULAR, 4, *args) == -1 and "NULL" in err()
    assert L.ptmi_debug_nee_call(None, 0, 4, a.ctypes.data, f.ctypes.data, k.ctypes.data) == -1
    for op in (M.NEE_CALL_ENV_LOOKUP, M.NEE_CALL_ENV_SAMPLE):
        assert call(op, 4) == -1 and "environment" in err()
    R.set_environment(S.env_maps()["1x7"])
    for bad in (np.nan, np.inf, -np.inf):                                        # no column exists for a non-finite direction
        d = np.zeros((4, M.NEE_CALL_IN), F); d[:, 0] = 1.0; d[2, 2] = bad
        assert call(M.NEE_CALL_ENV_LOOKUP, 4, d) == -1 and "finite" in err()
    R.set_environment(None)
    types, verts, normal, bsdf, Le = S.array_scene()
    R.load_scene_arrays(types, verts, normal, bsdf, np.zeros_like(Le))
    assert call(M.NEE_CALL_EMITTER_SAMPLE, 4) == -1 and "emitter" in err()
    assert call(M.NEE_CALL_ROUGH_EVAL, 4) == 0
