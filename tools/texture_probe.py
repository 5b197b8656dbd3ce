#!/usr/bin/env python3
"""What an albedo texture (include/ptmi.h: ptmi_set_albedo_texture) costs per frame - the measurements of DESIGN.md 4.20.

  cbox.obj plus ONE triangle no ray reaches, 1024^2, depth 8, 64 spp, next_event 1:
    plain     no texture: the frame the parent commit renders.  With next_event = 1 and nothing else set it runs the TEX = false
              instantiation of ptmi_render_nee, which the ISA digest shows byte-identical to the parent's kernel, so this IS the
              parent's baseline, measured in the same process and interleaved with the others.  (PTMI_LIB=<a library built from
              the parent commit> measures the parent's own binary: without ptmi_set_albedo_texture only `plain` is reported.)
    one       the image applied to the unreachable triangle only: the TEX = true kernel paying the 16-byte decision per vertex
    nearest   the image applied to every primitive, nearest filter: one more 16-byte record and one texel read per vertex
    bilinear  the same, bilinear: four texel reads

  Device time (hipEvents, ptmi_stats.seconds) after a warm-up frame of each variant; the variants alternate frame by frame,
  --reps frames each; median and range, and each ratio to `plain` with the range of the per-repetition ratios.

  python tools/texture_probe.py [--reps N] [--size N]      (one JSON line)
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
from specular_probe import DEPTH, SIDE, SPP, hidden_triangle_scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=256, help="side of the square image")
    a = ap.parse_args()
    arrays, hidden = hidden_triangle_scene()
    n = len(arrays[0])
    prims = dict(type=arrays[0], verts=arrays[1], normal=arrays[2])
    image = np.random.default_rng(1).uniform(0.2, 1.0, (a.size, a.size, 3)).astype(np.float32)
    uv = ptmi_scenes.box_uvs(prims, scale=1.7)
    only = np.zeros(n, bool); only[hidden] = True
    variants = {"plain": None}
    if hasattr(ptmi.lib(), "ptmi_set_albedo_texture"):
        variants.update(one=(only, "nearest"), nearest=(None, "nearest"), bilinear=(None, "bilinear"))
    r = ptmi.Renderer(0)
    r.set_camera(ptmi.default_camera())
    r.load_scene_arrays(*arrays)
    r.update_resolution(SIDE, SIDE)
    r.set_config(spp=SPP, max_depth=DEPTH, next_event=True)
    ms = {k: [] for k in variants}
    for rep in range(a.reps + 1):                           # rep 0 warms every variant up
        for key, v in variants.items():
            if len(variants) > 1:
                if v is None:
                    r.set_albedo_texture(None, None)
                else:
                    r.set_albedo_texture(image, uv, v[0], v[1])
            st = r.render_frame()
            if rep:
                ms[key].append(st.seconds * 1e3)
    r.close()
    out = {"side": SIDE, "spp": SPP, "depth": DEPTH, "image": a.size, "reps": a.reps}
    base = np.array(ms["plain"])
    for key, v in ms.items():
        v = np.array(v)
        out[key] = {"ms": round(float(np.median(v)), 3), "range_ms": [round(float(v.min()), 3), round(float(v.max()), 3)],
                    "msamples_per_s": round(SIDE * SIDE * SPP / (float(np.median(v)) * 1e-3) / 1e6, 1)}
        if key != "plain":
            ratio = v / base
            out[key]["ratio_to_plain"] = round(float(np.median(v) / np.median(base)), 4)
            out[key]["ratio_range"] = [round(float(ratio.min()), 4), round(float(ratio.max()), 4)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
