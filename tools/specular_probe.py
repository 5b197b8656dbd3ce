#!/usr/bin/env python3
"""What specular surfaces (include/ptmi.h: ptmi_set_surfaces) cost per frame - the measurements of DESIGN.md 4.16.

  cbox.obj 1024^2, depth 8, 64 spp, next_event 0 and 1:
    blocks   the table of ptmi_scenes.cornell_blocks (short block a mirror, tall block glass) against the same context with the
             table dropped (next_event 0: the tuned bounce kernels; 1: the per-lane kernel's SPEC = false instantiation);
    one      a table that is diffuse but for ONE mirror triangle no ray reaches: the SPEC = true kernel does the SPEC = false
             kernel's work plus the table read per vertex.  Against the table dropped under next_event = 1 this is the share
             of time the SPEC parameter itself costs.

  Device time (hipEvents, ptmi_stats.seconds) after a warm-up frame of each variant; the variants alternate frame by frame,
  --reps frames each; median and range.

  python tools/specular_probe.py [--reps N]      (one JSON line)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cuda-pathtracer_amd", "python")]
import ptmi  # noqa: E402
import ptmi_scenes  # noqa: E402

CBOX = os.path.join(ROOT, "tests", "golden", "scenes", "cbox.obj")
SIDE, SPP, DEPTH = 1024, 64, 8


def hidden_triangle_scene():
    """cbox.obj plus one triangle outside the box behind its back wall, where no ray arrives; (arrays, the triangle's index)"""
    p = ptmi.HostScene.load(CBOX).prims()
    tri = np.zeros((1, 4, 3), np.float32)
    tri[0, :3] = [(-0.5, 2.0, -7.0), (0.5, 2.0, -7.0), (0.0, 3.0, -7.0)]
    one = lambda a, row: np.concatenate([a, np.asarray([row], a.dtype)])
    return (one(p["type"], 0), np.concatenate([p["verts"], tri]), one(p["normal"], (0.0, 0.0, 1.0)), one(p["bsdf"], (0.9, 0.9, 0.9)),
            one(p["Le"], (0.0, 0.0, 0.0))), len(p["type"])


def measure(r, variants, next_event, reps):
    """ms per frame of every variant (name -> kind array or None), alternating"""
    ms = {k: [] for k in variants}
    r.set_config(next_event=next_event)
    for rep in range(reps + 1):                             # rep 0 warms every variant up
        for key, kind in variants.items():
            r.set_surfaces(kind)
            st = r.render_frame()
            if rep:
                ms[key].append(st.seconds * 1e3)
    r.set_surfaces(None)
    out = {}
    for key, v in ms.items():
        out[key] = {"ms": round(float(np.median(v)), 3), "range_ms": [round(min(v), 3), round(max(v), 3)],
                    "msamples_per_s": round(SIDE * SIDE * SPP / (np.median(v) * 1e-3) / 1e6, 1)}
    for key in variants:
        if key != "dropped":
            out[key]["ratio_to_dropped"] = round(out[key]["ms"] / out["dropped"]["ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    r = ptmi.Renderer(0)
    r.set_camera(ptmi.default_camera())
    arrays, hidden = hidden_triangle_scene()
    r.load_scene_arrays(*arrays)
    r.update_resolution(SIDE, SIDE)
    r.set_config(spp=SPP, max_depth=DEPTH)
    blocks = ptmi_scenes.cornell_blocks(r.scene_prims())
    one = np.zeros(hidden + 1, np.int32); one[hidden] = ptmi.SURFACE_MIRROR
    out = {}
    for nee in (0, 1):
        out[f"next_event_{nee}"] = measure(r, {"dropped": None, "blocks": blocks, "one": one}, bool(nee), a.reps)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
