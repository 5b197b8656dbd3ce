#!/usr/bin/env python3
"""What a participating medium (include/ptmi.h: ptmi_set_medium) costs per frame - the measurements of DESIGN.md 4.24.

  cbox.obj, 1024^2, depth 8, 64 spp, next_event 1:
    none      no medium: ptmi_render_nee's MEDIUM = false instantiation - the kernel the parent commit runs plus one unread argument
    far       a box no camera ray and no bounce ray meets: the MEDIUM = true instantiation, the draw, the logarithm and the slab
              test per path ray, the slab test per visible shadow ray, and never a medium vertex
    fog       fog filling the room at sigma_t = 0.18: an optical depth of about 1 over the room's 5.6 units

  Device time (hipEvents, ptmi_stats.seconds) after a warm-up frame of each variant; the variants alternate frame by frame,
  --reps frames each; median and range, and each ratio to `none` with the range of the per-repetition ratios.

  --against LIB: `none` alone, this tree's library and LIB (one built from the parent commit) by turns, each turn a process of its
  own that warms up and renders --frames frames; the difference of the medians next to the spread each library shows by itself.

  python tools/medium_probe.py [--reps N] [--against LIB [--turns N] [--frames N]]      (one JSON line)
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cuda-pathtracer_amd", "python"), os.path.dirname(os.path.abspath(__file__))]
import ptmi  # noqa: E402
from specular_probe import DEPTH, SIDE, SPP  # noqa: E402

CBOX = os.path.join(ROOT, "tests", "golden", "scenes", "cbox.obj")
ROOM = ((-10.0, -10.0, -10.0), (10.0, 10.0, 10.0))
VARIANTS = {"none": None, "far": ((1000.0, 1000.0, 1000.0), (1001.0, 1001.0, 1001.0), 0.18, (0.9, 0.9, 0.9), 0.6), "fog": ROOM + (0.18, (0.9, 0.9, 0.9), 0.6)}


def context():
    r = ptmi.Renderer(0)
    r.set_camera(ptmi.default_camera())
    r.load_scene(CBOX)
    r.update_resolution(SIDE, SIDE)
    r.set_config(spp=SPP, max_depth=DEPTH, next_event=True)
    return r


def summary(v):
    v = np.array(v)
    return {"ms": round(float(np.median(v)), 3), "range_ms": [round(float(v.min()), 3), round(float(v.max()), 3)],
            "msamples_per_s": round(SIDE * SIDE * SPP / (float(np.median(v)) * 1e-3) / 1e6, 1)}


def variants(reps):
    r = context()
    ms = {k: [] for k in VARIANTS}
    for rep in range(reps + 1):                             # rep 0 warms every variant up
        for key, medium in VARIANTS.items():
            if medium is None:
                r.set_medium(None)
            else:
                r.set_medium(*medium)
            st = r.render_frame()
            assert st.bounce_launches == 1
            if rep:
                ms[key].append(st.seconds * 1e3)
    r.close()
    out = {"side": SIDE, "spp": SPP, "depth": DEPTH, "reps": reps}
    base = np.array(ms["none"])
    for key, v in ms.items():
        out[key] = summary(v)
        if key != "none":
            ratio = np.array(v) / base
            out[key]["ratio_to_none"] = round(float(np.median(v) / np.median(base)), 4)
            out[key]["ratio_range"] = [round(float(ratio.min()), 4), round(float(ratio.max()), 4)]
    return out


def one_turn(frames):
    """a child of --against: the frames' device times of whatever library PTMI_LIB names, no medium call made"""
    r = context()
    r.render_frame()
    print(json.dumps([r.render_frame().seconds * 1e3 for _ in range(frames)]))
    r.close()


def against(lib, turns, frames):
    ms = {"this": [], "parent": []}
    for _ in range(turns):
        for key in ms:
            env = dict(os.environ)
            env.pop("PTMI_LIB", None)
            if key == "parent":
                env["PTMI_LIB"] = os.path.abspath(lib)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--turn", str(frames)], env=env, check=True, capture_output=True,
                                 text=True, timeout=300)
            ms[key].append(json.loads(res.stdout.strip().split("\n")[-1]))
    out = {"side": SIDE, "spp": SPP, "depth": DEPTH, "turns": turns, "frames": frames}
    for key, v in ms.items():
        out[key] = summary(np.concatenate(v))
        out[key]["turn_medians_ms"] = [round(float(np.median(t)), 3) for t in v]
    out["this_over_parent"] = round(out["this"]["ms"] / out["parent"]["ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--against", default=None, metavar="LIB")
    ap.add_argument("--turns", type=int, default=3); ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--turn", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.turn:
        one_turn(a.turn)
    elif a.against:
        print(json.dumps(against(a.against, a.turns, a.frames)))
    else:
        print(json.dumps(variants(a.reps)))


if __name__ == "__main__":
    main()
