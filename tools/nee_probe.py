#!/usr/bin/env python3
"""What next-event estimation (include/ptmi.h: ptmi_config.next_event) costs per sample and buys in noise.

  For c2 (cbox.obj 1024^2, depth 8, 64 spp) and the 1 M-triangle scene (ptmi_scenes.tessellated_cornell, 512^2, depth 5, 64 spp):
  ms per frame (median of --reps frames after a warm-up frame) and Msamples/s of both estimators; the MSE of each one's
  linear radiance against a 4096-spp frame of the reference estimator rendered in the same run (other streams: the frames
  come after it); the equal-time efficiency (MSE_pt * t_pt) / (MSE_nee * t_nee).  Also the frame-to-frame variance ratio of
  cbox 32^2, depth 5, 16 frames of 512 spp, over the image and over the pixels no camera ray of which sees an emitter
  (tests/test_gpu_nee.py).

  python tools/nee_probe.py [--reps N] [--skip-1m]      (one JSON line)
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

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def load(r, name):
    if name == "c2":
        r.load_scene(os.path.join(SCENES, "cbox.obj"))
        return
    base = ptmi.HostScene.load(os.path.join(SCENES, "cbox_quads.obj")).prims()
    sc = ptmi_scenes.tessellated_cornell(base, 256, 128, seed=1)
    r.load_scene_arrays(sc["type"], sc["verts"], sc["normal"], sc["bsdf"], sc["Le"])


def measure(r, name, side, depth, spp, ref_spp, reps):
    load(r, name)
    r.update_resolution(side, side)
    r.set_config(spp=ref_spp, max_depth=depth, next_event=False)
    r.render_frame()
    ref = r.read_image()[1].astype(np.float64)
    out = {"scene": name, "side": side, "depth": depth, "spp": spp, "ref_spp": ref_spp}
    for tag, nee in (("pt", False), ("nee", True)):
        r.set_config(spp=spp, next_event=nee)
        r.render_frame()                                    # warm-up
        ms, mse = [], []
        for _ in range(reps):
            st = r.render_frame()
            ms.append(st.seconds * 1e3)
            mse.append(float(((r.read_image()[1].astype(np.float64) - ref) ** 2).mean()))
        t = float(np.median(ms))
        out[f"{tag}_ms"] = round(t, 3)
        out[f"{tag}_msamples_per_s"] = round(side * side * spp / (t * 1e-3) / 1e6, 1)
        out[f"{tag}_mse"] = float(np.mean(mse))
    out["efficiency"] = round((out["pt_mse"] * out["pt_ms"]) / (out["nee_mse"] * out["nee_ms"]), 3)
    return out


def variance_ratio(r):
    stacks = {}
    for nee in (False, True):
        r.load_scene(os.path.join(SCENES, "cbox.obj"))
        r.update_resolution(32, 32)
        r.set_config(spp=512, max_depth=5, next_event=nee)
        frames = []
        for _ in range(16):
            r.render_frame()
            frames.append(r.read_image()[1].astype(np.float64))
        stacks[nee] = np.stack(frames)
    r.set_config(spp=64, max_depth=1, next_event=False)     # pixels some camera ray of which sees an emitter
    r.render_frame()
    lit = (r.read_image()[1] > 0).any(axis=2)
    vp, vn = stacks[False].var(axis=0, ddof=1), stacks[True].var(axis=0, ddof=1)
    return float(vp.sum() / vn.sum()), float(vp[~lit].sum() / vn[~lit].sum()), int(lit.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-1m", action="store_true")
    a = ap.parse_args()
    r = ptmi.Renderer(0)
    res = {"c2": measure(r, "c2", 1024, 8, 64, 4096, a.reps)}
    if not a.skip_1m:
        res["c5"] = measure(r, "c5", 512, 5, 64, 4096, a.reps)
    whole, unlit, n_lit = variance_ratio(r)
    res["cbox32_variance_ratio"] = round(whole, 3)
    res["cbox32_variance_ratio_no_emitter_in_view"] = round(unlit, 3)
    res["cbox32_pixels_seeing_an_emitter"] = n_lit
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
