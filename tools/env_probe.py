#!/usr/bin/env python3
"""What environment lighting (include/ptmi.h: ptmi_set_environment) costs per frame - the measurements of DESIGN.md 4.15.

  cbox.obj 1024^2, depth 8, 64 spp:
    (a) a constant map with next_event = 0 against the plain frame without a map (the tuned bounce kernel): the price of the
        per-lane route that a context with an environment takes;
    (b) the sun sky (ptmi_scenes.sky) with next_event = 1 against the NEE frame without a map.
  The 1 M-triangle scene (ptmi_scenes.tessellated_cornell) at 512^2, depth 5, 64 spp: NEE without a map and under the sun sky.
  Also the pixel-to-pixel variance of the ground quad under its sun (tests/env_scenes.py), plain against NEE.

  Device time (hipEvents, ptmi_stats.seconds) after a warm-up frame of each variant; the two variants of a pair alternate frame
  by frame, --reps frames each; median and range.

  python tools/env_probe.py [--reps N] [--skip-1m]      (one JSON line)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cuda-pathtracer_amd", "python"), os.path.join(ROOT, "tests")]
import ptmi  # noqa: E402
import ptmi_scenes  # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def load(r, name):
    if name == "c2":
        r.load_scene(os.path.join(SCENES, "cbox.obj"))
        return
    base = ptmi.HostScene.load(os.path.join(SCENES, "cbox_quads.obj")).prims()
    sc = ptmi_scenes.tessellated_cornell(base, 256, 128, seed=1)
    r.load_scene_arrays(sc["type"], sc["verts"], sc["normal"], sc["bsdf"], sc["Le"])


def pair(r, side, spp, next_event, env, reps):
    """ms per frame without a map and with `env`, alternating"""
    variants = {"without": None, "with": env}
    ms = {k: [] for k in variants}
    for rep in range(reps + 1):                             # rep 0 warms both variants up
        for key, e in variants.items():
            r.set_environment(e)
            r.set_config(next_event=next_event)
            st = r.render_frame()
            if rep:
                ms[key].append(st.seconds * 1e3)
    r.set_environment(None)
    out = {}
    for key, v in ms.items():
        out[f"{key}_ms"] = round(float(np.median(v)), 3)
        out[f"{key}_range_ms"] = [round(min(v), 3), round(max(v), 3)]
        out[f"{key}_msamples_per_s"] = round(side * side * spp / (np.median(v) * 1e-3) / 1e6, 1)
    out["ratio"] = round(out["with_ms"] / out["without_ms"], 3)
    return out


def ground_variance(r):
    import env_scenes as ES
    out = {}
    for tilt, rot in ((0.0, 0.0), (35.0, 70.0)):
        env, _, v, var = ES.sun_case(tilt, rot)
        r.load_scene_arrays(*ES.ground_quad((0.3, 0.5, 0.7), tilt).arrays())
        r.set_camera(ES.top_down_camera(tilt))
        r.set_environment(env, rotation_deg=rot)
        r.update_resolution(128, 128)
        pv = {}
        for nee in (False, True):
            r.set_config(spp=1024, max_depth=5, next_event=nee)
            r.render_frame()
            pv[nee] = r.read_image(rgb8=False)[1].astype(np.float64).reshape(-1, 3).var(0, ddof=1)
        out[f"tilt_{int(tilt)}"] = {"plain": pv[False].tolist(), "nee": pv[True].tolist(), "ratio": (pv[False] / pv[True]).tolist()}
    r.set_environment(None)
    r.set_camera(ptmi.default_camera())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-1m", action="store_true")
    a = ap.parse_args()
    r = ptmi.Renderer(0)
    r.set_camera(ptmi.default_camera())
    out = {}
    load(r, "c2")
    r.update_resolution(1024, 1024)
    r.set_config(spp=64, max_depth=8)
    out["c2_constant_map_plain"] = pair(r, 1024, 64, False, np.full((1, 1, 3), 0.5, np.float32), a.reps)
    out["c2_sun_sky_nee"] = pair(r, 1024, 64, True, ptmi_scenes.sky(64, 32), a.reps)
    if not a.skip_1m:
        load(r, "1m")
        r.update_resolution(512, 512)
        r.set_config(spp=64, max_depth=5)
        out["1m_sun_sky_nee"] = pair(r, 512, 64, True, ptmi_scenes.sky(64, 32), a.reps)
    out["ground_quad_variance"] = ground_variance(r)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
