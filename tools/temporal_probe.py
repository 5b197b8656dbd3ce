#!/usr/bin/env python3
"""What the temporal accumulation (include/ptmi.h: ptmi_temporal_accumulate) costs and buys on an orbiting camera.

  1. device time (hipEvents, after warm-up; the median of --reps steps) of one step, the camera turned 1 degree between
     frames (the feature pass it then runs is reported apart) and with a still camera: c2 (cbox 1024^2) and c3 (cbox_quads
     1920 x 1080);
  2. RMSE of the radiance against a high-spp frame of another seed at the same view, along an orbit of --views views
     --yaw-step degrees apart at 4 and 16 spp: the frame alone, the frame through the a-trous denoiser, the temporal
     history, and the history through the denoiser (ptmi_denoise_temporal); then one 90-degree jump.  Default: c2.

  3. --moments: the same with the history carrying its luminance statistics (ptmi_set_temporal_moments): the step's time, the
     variance estimate of ptmi_denoise_temporal_variance from them (all pixels own theirs after the still steps) beside the
     spatial estimate (source = 1) on the same history, alternating, and the RMSE of the history through that filter.

  python tools/temporal_probe.py [--quick] [--side 1024] [--moments]     (one JSON line per measurement; PTMI_LIB: another build)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cuda-pathtracer_amd", "python")]
import ptmi  # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def stat(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def timing(r, name, reps, moments=False):
    if name == "c2":
        r.load_scene(os.path.join(SCENES, "cbox.obj")); r.update_resolution(1024, 1024); depth = 8
    else:
        r.load_scene(os.path.join(SCENES, "cbox_quads.obj")); r.update_resolution(1920, 1080); depth = 5
    r.set_config(spp=4, max_depth=depth)
    cam = ptmi.default_camera()
    r.set_camera(cam)
    r.render_frame()
    r.temporal_accumulate()                                    # warm-up (buffers, code objects)
    moving, feats, still = [], [], []
    for i in range(reps):
        cam.yaw_deg = 90.0 + (i + 1)
        r.set_camera(cam)
        r.render_frame()
        _, _, st = r.temporal_accumulate()
        moving.append(st.seconds * 1e3); feats.append(st.features_ms)
    for _ in range(reps):
        r.render_frame()
        _, _, st = r.temporal_accumulate()
        still.append(st.seconds * 1e3)
    print(json.dumps(dict(what="timing", lib=os.path.basename(ptmi.LIB_PATH), config=name, moments=int(moments), width=r.width,
                          height=r.height, step_moving_ms=float(np.median(moving)), features_g2_ms=float(np.median(feats)),
                          step_still_ms=float(np.median(still)), moving=stat(moving), still=stat(still), reps=reps)), flush=True)
    if not moments:
        return
    for _ in range(3):                                         # warm-up
        r.denoise_temporal_variance(); r.denoise_temporal_variance(source=1)
    hist, spatial, filt = [], [], []
    for _ in range(reps):
        r.denoise_temporal_variance()
        e, f = r.variance_timing()
        hist.append(e); filt.append(f)
        r.denoise_temporal_variance(source=1)
        spatial.append(r.variance_timing()[0])
    owned = float((r.temporal_moments()[2] >= 4.0).mean())
    print(json.dumps(dict(what="estimate_timing", config=name, width=r.width, height=r.height, owned_fraction=owned,
                          estimate_history_ms=stat(hist), estimate_spatial_ms=stat(spatial), filter_5it_ms=stat(filt), reps=reps)), flush=True)


def quality(r, side, ref_spp, views, yaw_step, spps, moments=False):
    r.load_scene(os.path.join(SCENES, "cbox.obj"))
    depth = 8
    cam = ptmi.default_camera()
    yaw0 = cam.yaw_deg
    checkpoints = sorted({1, 2, 4, 8, views} & set(range(1, views + 1)))
    jump = views + 1                                            # one 90-degree jump after the orbit
    refs = {}
    r.set_config(spp=ref_spp, max_depth=depth, seed_base=77)
    r.update_resolution(side, side)                             # (the streams start from the seed at a resolution update)
    for k in checkpoints + [jump]:
        cam.yaw_deg = yaw0 + ((k - 1) * yaw_step if k <= views else (views - 1) * yaw_step + 90.0)
        r.set_camera(cam)
        r.render_frame()
        refs[k] = r.read_image()[1].astype(np.float64)
    for spp in spps:
        r.set_config(spp=spp, max_depth=depth, seed_base=2023)
        r.update_resolution(side, side)
        for k in range(1, jump + 1):
            cam.yaw_deg = yaw0 + ((k - 1) * yaw_step if k <= views else (views - 1) * yaw_step + 90.0)
            r.set_camera(cam)
            r.render_frame()
            _, frame = r.read_image()
            _, hist, st = r.temporal_accumulate()
            if k not in refs:
                continue
            rmse = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - refs[k]) ** 2)))
            _, hist_f = r.denoise_temporal()
            _, frame_f = r.denoise()
            counts = r.history_counts()
            extra = dict(rmse_temporal_variance=rmse(r.denoise_temporal_variance()[1])) if moments else {}
            print(json.dumps(dict(extra, what="quality", side=side, ref_spp=ref_spp, spp=spp, view=k, jump=k == jump, yaw_step=yaw_step,
                                  accepted=st.accepted, rejected=st.rejected, missed=st.missed, mean_history_spp=float(counts.mean()),
                                  rmse_frame=rmse(frame), rmse_frame_denoised=rmse(frame_f), rmse_temporal=rmse(hist),
                                  rmse_temporal_denoised=rmse(hist_f))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions, lower reference spp")
    ap.add_argument("--timing-only", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--yaw-step", type=float, default=2.0)
    ap.add_argument("--moments", action="store_true", help="the history carries its luminance statistics (ptmi_set_temporal_moments)")
    a = ap.parse_args()
    r = ptmi.Renderer(0)
    if a.moments:
        r.set_temporal_moments(1)
    reps = 5 if a.quick else a.reps
    for name in ("c2", "c3"):
        timing(r, name, reps, a.moments)
    if not a.timing_only:
        quality(r, a.side, 1024 if a.quick else 4096, a.views, a.yaw_step, (4, 16), a.moments)
    r.close()


if __name__ == "__main__":
    main()
