#!/usr/bin/env python3
"""What rough metal (include/ptmi.h: ptmi_set_surfaces_rough) costs per frame - the measurements of DESIGN.md 4.17.

  cbox.obj (plus one triangle no ray reaches) 1024^2, depth 8, 64 spp, next_event 0 and 1:
    blocks   the table of ptmi_scenes.cornell_blocks (short block a mirror, tall block glass): the SURF = 1 kernel;
    hidden   the same table with the unreachable triangle made rough metal: the SURF = 2 kernel doing the SURF = 1 kernel's work -
             the price of the instantiation itself (registers, code size, the kind test per vertex);
    rough    the short block glass and the tall block rough metal at roughness 0.3.
  --sub N: the scene subdivided N times (2: 513 primitives, the certified walk); --sky: under an environment (ENV).

  Device time (hipEvents, ptmi_stats.seconds) after a warm-up frame of each variant; the variants alternate frame by frame,
  --reps frames each; median and range.

  python tools/rough_probe.py [--reps N] [--sub N] [--sky]      (one JSON line)
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


def hidden_triangle_scene(sub):
    """cbox.obj plus one triangle outside the box behind its back wall, where no ray arrives; (arrays, the triangle's index)"""
    p = ptmi.HostScene.load(CBOX, sub).prims()
    tri = np.zeros((1, 4, 3), np.float32)
    tri[0, :3] = [(-0.5, 2.0, -7.0), (0.5, 2.0, -7.0), (0.0, 3.0, -7.0)]
    one = lambda a, row: np.concatenate([a, np.asarray([row], a.dtype)])
    return (one(p["type"], 0), np.concatenate([p["verts"], tri]), one(p["normal"], (0.0, 0.0, 1.0)), one(p["bsdf"], (0.9, 0.9, 0.9)),
            one(p["Le"], (0.0, 0.0, 0.0))), len(p["type"])


def measure(r, variants, next_event, reps):
    """ms per frame of every variant (name -> kind array), alternating"""
    ms = {k: [] for k in variants}
    r.set_config(next_event=next_event)
    for rep in range(reps + 1):                             # rep 0 warms every variant up
        for key, kind in variants.items():
            r.set_surfaces(kind, None, 0.3)
            st = r.render_frame()
            if rep:
                ms[key].append(st.seconds * 1e3)
    r.set_surfaces(None)
    out = {}
    for key, v in ms.items():
        out[key] = {"ms": round(float(np.median(v)), 3), "range_ms": [round(min(v), 3), round(max(v), 3)],
                    "msamples_per_s": round(SIDE * SIDE * SPP / (np.median(v) * 1e-3) / 1e6, 1)}
    for key in variants:
        if key != "blocks":
            out[key]["ratio_to_blocks"] = round(out[key]["ms"] / out["blocks"]["ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sub", type=int, default=0)
    ap.add_argument("--sky", action="store_true", help="with ptmi_scenes.sky(32, 16) as environment: the ENV instantiations")
    a = ap.parse_args()
    r = ptmi.Renderer(0)
    r.set_camera(ptmi.default_camera())
    arrays, hidden = hidden_triangle_scene(a.sub)
    r.load_scene_arrays(*arrays)
    r.update_resolution(SIDE, SIDE)
    r.set_config(spp=SPP, max_depth=DEPTH)
    if a.sky:
        r.set_environment(ptmi_scenes.sky(32, 16))
    inside = {k: v[:hidden] for k, v in r.scene_prims().items()}
    pad = lambda kind: np.append(kind, 0).astype(np.int32)
    blocks = pad(ptmi_scenes.cornell_blocks(inside))
    one = blocks.copy(); one[hidden] = ptmi.SURFACE_ROUGH
    rough = pad(ptmi_scenes.cornell_blocks(inside, short=ptmi.SURFACE_GLASS, tall=ptmi.SURFACE_ROUGH))
    out = {"walk": int(r.traversal()), "n_prims": hidden + 1}
    for nee in (0, 1):
        out[f"next_event_{nee}"] = measure(r, {"blocks": blocks, "hidden": one, "rough": rough}, bool(nee), a.reps)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
