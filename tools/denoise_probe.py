#!/usr/bin/env python3
"""What the feature pass and the a-trous denoiser (include/ptmi.h: ptmi_render_features, ptmi_denoise) cost and buy.

  1. device time (hipEvents, after warm-up; the median of --reps runs) of the feature pass (g = 2) and of the filter at the
     default 5 iterations: c2 (cbox 1024^2) and c3 (cbox_quads 1920 x 1080);
  2. RMSE of the radiance against a high-spp frame of another seed, noisy and denoised, at 4 / 16 / 64 spp, with the time of
     the frame and of features + filter: c2, and the 1 M-triangle scene of c5tile rendered whole at 1024^2 (the denoiser needs
     the whole frame on one GPU; c5tile is an eighth of a 2048^2 frame).  The question it answers: how many spp plus the
     denoiser reach the RMSE of a plain frame, and at what total time.

  3. --variance: the variance-guided filter (ptmi_denoise_variance) beside ptmi_denoise on the same c3 image, in one process,
     the two alternating: the variance estimate (spatial, radius 3; and the accumulation's after two passes) and the filter
     proper at 5 iterations; medians with the min .. max of the runs.

  python tools/denoise_probe.py [--quick]          (one JSON line per measurement)
  python tools/denoise_probe.py --variance         (PTMI_LIB=ab_libs/libptmi_x.so: another build of the library, make ab-post-lib)
  (per-kernel breakdown: rocprofv3 --kernel-trace --stats -- python tools/denoise_probe.py --timing-only, in a run of its own)
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


def setup(r, name, side):
    if name == "c2":
        r.load_scene(os.path.join(SCENES, "cbox.obj"))
        r.update_resolution(side, side)
        return 8
    if name == "c3":
        r.load_scene(os.path.join(SCENES, "cbox_quads.obj"))
        r.update_resolution(1920, 1080)
        return 5
    base = ptmi.HostScene.load(os.path.join(SCENES, "cbox_quads.obj")).prims()
    sc = ptmi_scenes.tessellated_cornell(base, 256, 128, seed=1)
    r.load_scene_arrays(sc["type"], sc["verts"], sc["normal"], sc["bsdf"], sc["Le"])
    r.update_resolution(side, side)
    return 8


def timing(r, name, reps):
    depth = setup(r, name, 1024)
    r.set_config(spp=4, max_depth=depth)
    r.render_frame()
    r.denoise()                                                # warm-up (buffers, code objects)
    f_ms, d_ms = [], []
    for _ in range(reps):
        r.render_features(2)
        r.denoise()                                            # features current: the filter alone
        f, d = r.denoise_timing()
        f_ms.append(f); d_ms.append(d)
    print(json.dumps(dict(what="timing", config=name, width=r.width, height=r.height, features_g2_ms=float(np.median(f_ms)),
                          denoise_5it_ms=float(np.median(d_ms)), reps=reps)), flush=True)


def variance_timing(r, reps):
    depth = setup(r, "c3", 0)
    r.set_config(spp=1, max_depth=depth)
    stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
    for source in ("spatial", "accumulation"):
        if source == "spatial":
            r.render_frame()
        else:
            r.accum_reset(); r.accum_pass(None); r.accum_pass(None)
        for _ in range(3):                                     # warm-up (buffers, code objects, clocks)
            r.denoise(); r.denoise_variance()
        d_ms, e_ms, f_ms = [], [], []
        for _ in range(reps):
            r.denoise()
            d_ms.append(r.denoise_timing()[1])
            r.denoise_variance()
            e, f = r.variance_timing()
            e_ms.append(e); f_ms.append(f)
        print(json.dumps(dict(what="variance_timing", lib=os.path.basename(ptmi.LIB_PATH), source=source, width=r.width, height=r.height,
                              iterations=5, reps=reps, denoise_ms=stat(d_ms), estimate_ms=stat(e_ms), filter_ms=stat(f_ms),
                              filter_over_denoise=float(np.median(f_ms) / np.median(d_ms)),
                              estimate_over_denoise=float(np.median(e_ms) / np.median(d_ms)))), flush=True)


def quality(r, name, side, ref_spp, spps):
    depth = setup(r, name, side)
    r.set_config(spp=ref_spp, max_depth=depth, seed_base=77)
    r.render_frame()
    _, ref = r.read_image()
    ref = ref.astype(np.float64)
    rmse = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - ref) ** 2)))
    for spp in spps:
        r.set_config(spp=spp, max_depth=depth, seed_base=2023)
        r.update_resolution(side, side)
        st = r.render_frame()
        _, noisy = r.read_image()
        _, den = r.denoise()
        f, d = r.denoise_timing()
        print(json.dumps(dict(what="quality", config=name, side=side, ref_spp=ref_spp, spp=spp, frame_ms=st.seconds * 1e3,
                              features_ms=f, denoise_ms=d, rmse_noisy=rmse(noisy), rmse_denoised=rmse(den))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions, lower reference spp")
    ap.add_argument("--timing-only", action="store_true")
    ap.add_argument("--variance", action="store_true", help="only the variance-guided filter's timing beside ptmi_denoise's")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    r = ptmi.Renderer(0)
    reps = 5 if a.quick else a.reps
    if a.variance:
        variance_timing(r, reps)
        r.close()
        return
    for name in ("c2", "c3"):
        timing(r, name, reps)
    if not a.timing_only:
        quality(r, "c2", 1024, 1024 if a.quick else 4096, (4, 16, 64, 256))
        quality(r, "c5scene", 1024, 256 if a.quick else 1024, (4, 16, 64, 256))
    r.close()


if __name__ == "__main__":
    main()
