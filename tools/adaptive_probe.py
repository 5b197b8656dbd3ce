#!/usr/bin/env python3
"""What progressive and adaptive accumulation (include/ptmi.h: ptmi_accum_pass) cost and buy, on the benchmark's scenes.

  1. the cost of a pass boundary: K passes of spp samples against ONE frame of K * spp (the same samples, bit for bit) -
     c2 (cbox 1024^2, depth 8) at spp 8 / 32 with K = 8, c5tile (an eighth of the 1 M-triangle frame) at spp 64 with K = 4;
  2. what adaptivity buys at the default parameters: total samples, time and RMSE against a high-spp image (other seed) of
     the adaptive run, of a fixed run at max_passes * spp, and of a fixed run at the adaptive run's mean samples per pixel.

  python tools/adaptive_probe.py [--quick]          (one JSON line per measurement)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cuda-pathtracer_amd", "python")]
import ptmi  # noqa: E402
import ptmi_scenes  # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def setup(r, name):
    if name == "c2":
        r.load_scene(os.path.join(SCENES, "cbox.obj"))
        r.update_resolution(1024, 1024)
        return dict(max_depth=8)
    base = ptmi.HostScene.load(os.path.join(SCENES, "cbox_quads.obj")).prims()
    sc = ptmi_scenes.tessellated_cornell(base, 256, 128, seed=1)
    r.load_scene_arrays(sc["type"], sc["verts"], sc["normal"], sc["bsdf"], sc["Le"])
    r.update_resolution(2048, 2048, n_ranks=8, rank=3, row_block=8)
    return dict(max_depth=8)


def frame(r, spp, **cfg):
    r.set_config(spp=spp, **cfg)
    st = r.render_frame()
    return st.seconds, r.read_image()[1]


def boundary_cost(r, name, spp, K):
    cfg = setup(r, name)
    r.set_config(spp=spp, **cfg)
    r.render_frame()                                    # warm-up (code objects, cost order)
    r.update_resolution(r.width, r.height, *tiling(name))
    r.set_config(spp=spp, **cfg)
    t_pass = 0.0
    w0 = time.perf_counter()
    for _ in range(K):
        t_pass += r.accum_pass().seconds
    wall_pass = time.perf_counter() - w0
    _, rad_p = r.read_image()
    r.update_resolution(r.width, r.height, *tiling(name))   # the same streams again
    w0 = time.perf_counter()
    t_frame, rad_f = frame(r, K * spp, **cfg)
    wall_frame = time.perf_counter() - w0
    return dict(probe="pass_boundary", config=name, spp=spp, passes=K, passes_s=round(t_pass, 5), frame_s=round(t_frame, 5),
                ratio=round(t_pass / t_frame, 4), wall_ratio=round(wall_pass / wall_frame, 4),
                bit_equal=bool((rad_p.view(np.uint32) == rad_f.view(np.uint32)).all()))


def tiling(name):
    return (1, 0, 8) if name == "c2" else (8, 3, 8)


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def adaptivity(r, name, spp, ref_spp):
    cfg = setup(r, name)
    prm = ptmi.default_adaptive_params()
    r.set_config(seed_base=7)                             # an independent high-spp estimate: other streams
    r.update_resolution(r.width, r.height, *tiling(name))
    _, ref = frame(r, ref_spp, **cfg)
    r.set_config(seed_base=2023)
    r.update_resolution(r.width, r.height, *tiling(name))
    r.set_config(spp=spp, **cfg)
    passes = r.render_adaptive(min_passes=prm.min_passes, max_passes=prm.max_passes, threshold=prm.threshold, floor=prm.floor)
    _, rad_a = r.read_image()
    counts = r.sample_counts()
    n_pix = counts.size
    ad = dict(samples=int(counts.sum()), seconds=round(sum(p.seconds for p in passes), 5), passes=len(passes), rmse=rmse(rad_a, ref),
              stopped_early=round(float((counts < prm.max_passes * spp).mean()), 4))
    r.update_resolution(r.width, r.height, *tiling(name))
    t_max, rad_max = frame(r, prm.max_passes * spp, **cfg)
    mean_spp = max(1, int(round(ad["samples"] / n_pix)))
    r.update_resolution(r.width, r.height, *tiling(name))
    t_eq, rad_eq = frame(r, mean_spp, **cfg)
    return dict(probe="adaptivity", config=name, spp_per_pass=spp, params=dict(min_passes=prm.min_passes, max_passes=prm.max_passes,
                threshold=prm.threshold, floor=prm.floor), reference_spp=ref_spp, adaptive=ad,
                fixed_max=dict(spp=prm.max_passes * spp, samples=n_pix * prm.max_passes * spp, seconds=round(t_max, 5), rmse=rmse(rad_max, ref)),
                fixed_same_samples=dict(spp=mean_spp, samples=n_pix * mean_spp, seconds=round(t_eq, 5), rmse=rmse(rad_eq, ref)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--quick", action="store_true", help="c2 only")
    a = ap.parse_args()
    r = ptmi.Renderer(0)
    runs = [("c2", 8, 8), ("c2", 32, 8)] + ([] if a.quick else [("c5tile", 64, 4)])
    for name, spp, K in runs:
        print(json.dumps(boundary_cost(r, name, spp, K)), flush=True)
    for name, spp, ref_spp in [("c2", 8, 4096)] + ([] if a.quick else [("c5tile", 16, 4096)]):
        print(json.dumps(adaptivity(r, name, spp, ref_spp)), flush=True)
    r.close()


if __name__ == "__main__":
    main()
