#!/usr/bin/env python3
"""What vertex normals (include/ptmi.h: ptmi_set_vertex_normals) cost per frame - the measurements of DESIGN.md 4.19.

  1024^2, depth 8, 64 spp, next_event 0 and 1:
    one      cbox.obj plus ONE triangle no ray reaches, flat everywhere but there: the SMOOTH = true kernel does the SMOOTH =
             false kernel's work plus one 16-byte table read per vertex.  Against the table dropped under next_event = 1 this is
             the share of time the SMOOTH parameter itself costs; under next_event = 0 the table also moves the frame from the
             tuned bounce kernels to the per-lane kernel.
    spheres  ptmi_scenes.cornell_spheres level 3 (2 x 1280 triangles, every sphere vertex interpolates) with its table and with
             the table dropped (faceted spheres), and cornell_blocks' scene - the box with its blocks - next to them.

  Device time (hipEvents, ptmi_stats.seconds) after a warm-up frame of each variant; the variants alternate frame by frame,
  --reps frames each; median and range.

  python tools/smooth_probe.py [--reps N]      (one JSON line)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cuda-pathtracer_amd", "python"), os.path.dirname(os.path.abspath(__file__))]
import ptmi  # noqa: E402
import ptmi_scenes  # noqa: E402
from specular_probe import CBOX, DEPTH, SIDE, SPP, hidden_triangle_scene  # noqa: E402


def measure(renderers, next_event, reps):
    """ms per frame of every variant (name -> (renderer, table or None)), alternating"""
    ms = {k: [] for k in renderers}
    for rep in range(reps + 1):                             # rep 0 warms every variant up
        for key, (r, table) in renderers.items():
            r.set_config(next_event=next_event)
            r.set_vertex_normals(table)
            st = r.render_frame()
            if rep:
                ms[key].append(st.seconds * 1e3)
    out = {}
    for key, v in ms.items():
        out[key] = {"ms": round(float(np.median(v)), 3), "range_ms": [round(min(v), 3), round(max(v), 3)],
                    "msamples_per_s": round(SIDE * SIDE * SPP / (np.median(v) * 1e-3) / 1e6, 1)}
    return out


def context(arrays=None):
    r = ptmi.Renderer(0)
    r.set_camera(ptmi.default_camera())
    if arrays is None:
        r.load_scene(CBOX, 0)
    else:
        r.load_scene_arrays(*arrays)
    r.update_resolution(SIDE, SIDE)
    r.set_config(spp=SPP, max_depth=DEPTH)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    arrays, hidden = hidden_triangle_scene()
    one = np.repeat(arrays[2][:, None, :], 4, axis=1).astype(np.float32)
    one[hidden, :3] = [(0.6, 0.0, 0.8), (0.0, 0.6, 0.8), (-0.6, 0.0, 0.8)]
    sph_arrays, sph_table, _ = ptmi_scenes.cornell_spheres(ptmi.HostScene.load(CBOX).prims(), level=3)
    r_one, r_sph, r_box = context(arrays), context(sph_arrays), context()
    out = {}
    for nee in (0, 1):
        m = measure({"dropped": (r_one, None), "one": (r_one, one), "blocks": (r_box, None), "spheres_flat": (r_sph, None),
                     "spheres": (r_sph, sph_table)}, bool(nee), a.reps)
        m["one"]["ratio_to_dropped"] = round(m["one"]["ms"] / m["dropped"]["ms"], 3)
        m["spheres"]["ratio_to_spheres_flat"] = round(m["spheres"]["ms"] / m["spheres_flat"]["ms"], 3)
        m["spheres"]["ratio_to_blocks"] = round(m["spheres"]["ms"] / m["blocks"]["ms"], 3)
        out[f"next_event_{nee}"] = m
    for r in (r_one, r_sph, r_box):
        r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
