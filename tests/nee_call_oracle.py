"""What ptmi_debug_nee_call returns, restated per case from the float32 restatements of the contract (env_oracle, nee_oracle,
specular_oracle, rough_oracle): for each op a function from the input rows to (out_f, out_i, defined), laid out as
include/ptmi.h lists the op's outputs.  `defined` marks the floats the contract defines for the case: what a function leaves
behind a false verdict is compared nowhere, the verdict always.
"""
import numpy as np

import env_oracle as EO
import nee_oracle as NO
import rough_oracle as RO
import specular_oracle as SO

F = np.float32
OUT_F, OUT_I = 16, 4


def _blank(n):
    return np.zeros((n, OUT_F), F), np.zeros((n, OUT_I), np.int32), np.zeros((n, OUT_F), bool)


def env_lookup(tab, rows):
    f, k, ok = _blank(len(rows))
    for i, d in enumerate(rows):
        r, j = EO.lookup(tab, d[:3])
        k[i, :2] = (r, j)
        f[i, :4] = tab["texel"][r, j]
        ok[i, :4] = True
    return f, k, ok


def env_sample(tab, rows):
    f, k, ok = _blank(len(rows))
    for i, a in enumerate(rows):
        r, j, wi = EO.sample_direction(tab, a[0], a[1], a[2], a[3])
        k[i, :2] = (r, j)
        f[i, :3] = wi
        f[i, 3] = tab["texel"][r, j, 3]
        f[i, 4:7] = tab["texel"][r, j, :3]
        ok[i, :7] = True
    return f, k, ok


def emitter_sample(et, slot_of, rows, omq=None):
    """et: nee_call_sets.EmitterTable; slot_of: load-order index -> leaf-order slot; omq: 1 - q where the environment is a light
    too, else None"""
    f, k, ok = _blank(len(rows))
    for i, a in enumerate(rows):
        j = NO.select(et.cdf, et.total, a[0])
        p = int(et.prim[j])
        wi, dist2, cos_l, p_l, p_s = NO.emitter_sample(et.s, p, et.ng[p], et.pdf_area[p], a[1], a[2], a[3:6], omq)
        k[i, :3] = (j, slot_of[p], NO.sample_counts(cos_l, p_s))
        f[i, :3] = wi
        f[i, 3:7] = (dist2, cos_l, p_l, p_s)
        ok[i, :7] = True
    return f, k, ok


def specular(rows):
    f, k, ok = _blank(len(rows))
    for i, a in enumerate(rows):
        with np.errstate(all="ignore"):
            nxt, reflected, fr = SO.scatter(a[0:3], a[3:6], int(a[6]), a[7], a[8])
            len2 = NO._dot(nxt, nxt)
            walk = bool(len2 > 0 and len2 <= NO.FLT_MAX)
            k[i, :2] = (reflected, walk)
            f[i, 0] = fr
            f[i, 1:4] = nxt
            f[i, 4:7] = NO._unit(nxt)
        ok[i, :4] = True
        ok[i, 4:7] = walk                                  # no direction is made of a next that fails the length test
    return f, k, ok


def _vertex(b):
    return RO.Vertex(b[0:3], b[3:6], b[6])


def rough_vertex(rows):
    f, k, ok = _blank(len(rows))
    for i, a in enumerate(rows):
        v = _vertex(a)
        k[i, 0] = v.good
        f[i, 0:3] = v.un; f[i, 3:6] = v.T; f[i, 6:9] = v.B; f[i, 9:12] = v.wo
        f[i, 12] = RO.lam(v.a2, v.co) if v.good else 0.0
        ok[i, :13] = True
    return f, k, ok


def rough_eval(rows):
    f, k, ok = _blank(len(rows))
    for i, a in enumerate(rows):
        with np.errstate(all="ignore"):
            e = RO.evaluate(_vertex(a), a[7:10])
        k[i, 0] = e is not None
        if e is not None:
            f[i, :2] = e
            ok[i, :2] = True
    return f, k, ok


def rough_sample(rows):
    f, k, ok = _blank(len(rows))
    for i, a in enumerate(rows):
        v = _vertex(a)
        s = RO.sample(v, a[7], a[8]) if v.good else None
        k[i, 0] = s is not None
        if s is not None:
            f[i, :3] = s[0]; f[i, 3] = s[1]; f[i, 4] = s[2]
            ok[i, :5] = True
    return f, k, ok


def light_weight(rows):
    f, k, ok = _blank(len(rows))
    for i, a in enumerate(rows):
        b = a[1:]
        w0 = RO.light_weight(None, b[7:10], b[10], b[11])
        w2 = RO.light_weight(_vertex(b), b[7:10], b[10], b[11]) if a[0] != 0 else w0
        k[i, :2] = (1, w2 is not None)
        f[i, 0] = w0; ok[i, 0] = True
        if w2 is not None:
            f[i, 1] = w2; ok[i, 1] = True
    return f, k, ok
