"""CPU restatement of the shaded feature pass (include/ptmi.h: "shaded features"), written from the header in numpy float32: the
feature pass of tests/denoise_oracle.py with the section's TWO per-hit changes, on the restatements of "albedo texture"
(tests/texture_oracle.py) and "vertex normals" (tests/smooth_oracle.py).  With flags 0, or without the table a flag names, every
value is formed exactly as denoise_oracle.features forms it."""
import numpy as np

import smooth_oracle as SO
import texture_oracle as TX
from oracle_binding import camera_frame, camera_ray

F = np.float32
TEXTURED_ALBEDO, SHADING_NORMAL = 1, 2


def features(scene, cam, width, height, g, flags=0, texture=None, normals=None, rows=None):
    """Feature buffers of a width x height frame (rows: the global rows to compute, default all) with g x g rays per pixel: dict of
    albedo, normal, position (len(rows), width, 3) and hit_fraction (len(rows), width).  flags: the PTMI_FEATURE_* bits; texture:
    texture_oracle.make_table's dict or None (no albedo table); normals: the corner-normal table (n_prims, 4, 3) or None."""
    if flags < 0 or flags > 3:
        raise ValueError("flags must be in 0 .. 3")
    rows = np.arange(height) if rows is None else np.asarray(rows)
    cf = camera_frame(cam, width, height)
    prims = scene.prims()
    kd, nrm = prims["bsdf"], prims["normal"]
    tex_on = bool(flags & TEXTURED_ALBEDO) and texture is not None
    smooth_on = bool(flags & SHADING_NORMAL) and normals is not None
    if smooth_on:
        normals = np.ascontiguousarray(normals, F)
    out = {k: np.zeros((len(rows), width, 3), F) for k in ("albedo", "normal", "position")}
    hits = np.zeros((len(rows), width), F)
    offs = [(F(i) + F(0.5)) / F(g) for i in range(g)]
    for r, y in enumerate(rows):
        for x in range(width):
            a = np.zeros(3, F); n = np.zeros(3, F); p = np.zeros(3, F); h = F(0)
            for j in range(g):
                v = (F(y) + offs[j]) / F(height)
                for i in range(g):
                    u = (F(x) + offs[i]) / F(width)
                    o, d = camera_ray(cf, u, v)
                    hit = scene.intersect(o, d, 1e-4)
                    if hit.hit:
                        k = hit.prim
                        point = (o + F(hit.t) * d).astype(F)                  # the one p: added to P, the UV's and the normal's
                        ka = TX.albedo(prims, texture, k, point) if tex_on else kd[k]
                        ns = SO.vertex_normal(prims, normals, k, point)[0] if smooth_on else nrm[k]
                        a = a + ka; n = n + ns; p = p + point; h = h + F(1)
            s = F(1) / F(g * g)
            out["albedo"][r, x] = a * s; out["normal"][r, x] = n * s; out["position"][r, x] = p * s; hits[r, x] = h * s
    out["hit_fraction"] = hits
    return out
