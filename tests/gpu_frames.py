"""What the GPU frame tests of the per-lane estimator share (test_gpu_nee.py, test_gpu_env.py, test_gpu_specular.py,
test_gpu_rough.py): the comparison of a context's frames with the restatement's (tests/path_oracle.py), and a few scene pieces."""
import os

import numpy as np

import env_scenes as ES
import ptmi
from oracle_binding import Camera as OCamera, SCENES

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CBOX = os.path.join(SCENES, "cbox.obj")
CBOX_QUADS = os.path.join(SCENES, "cbox_quads.obj")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check_frames(R, ref, spp, depth, frames=2):
    """`frames` consecutive frames of the context R, set up as the restatement `ref` is, against ref's (the streams of both carry
    over): radiance bit for bit, the 8-bit image, the sample count, one launch.  Returns the last frame's (rgb, radiance, stats)."""
    for frame in range(frames):
        st = R.render_frame()
        rgb, rad = R.read_image()
        ergb, erad = ref.frame(spp, depth)
        assert np.array_equal(bits(rad), bits(erad)), (frame, int((bits(rad) != bits(erad)).sum()))
        assert np.array_equal(rgb, ergb)
        assert st.samples == ref.w * ref.h * spp and st.bounce_launches == 1
    return rgb, rad, st


def small_sky():
    return ES.random_map(7, 5, 12)


def ocam(cam):
    """the oracle's camera of a ptmi camera"""
    return OCamera(tuple(cam.origin), tuple(cam.lookat), tuple(cam.vup), cam.vfov_deg, cam.yaw_deg, cam.pitch_deg, cam.orbit)


def hidden_mirror(which):
    """the scene's arrays plus one triangle that no ray can reach; (arrays, its index).  The Cornell box is open towards the
    camera, so "behind the camera" would not do - a path that leaves through the front could find it.  The triangle lies outside
    the box behind the middle of the back wall: camera rays that pass the box diverge from that region, and a path that has
    left the box meets nothing that could turn it round."""
    hs = ptmi.HostScene.load(CBOX if which == "cbox" else CBOX_QUADS, 2 if which == "cbox_sub" else 0)
    p = hs.prims()
    tri = np.zeros((1, 4, 3), F)
    tri[0, :3] = [(-0.5, 2.0, -7.0), (0.5, 2.0, -7.0), (0.0, 3.0, -7.0)]
    arrays = (np.append(p["type"], 0).astype(np.int32), np.concatenate([p["verts"], tri]),
              np.concatenate([p["normal"], [[0.0, 0.0, 1.0]]]).astype(F), np.concatenate([p["bsdf"], [[0.9, 0.9, 0.9]]]).astype(F),
              np.concatenate([p["Le"], [[0.0, 0.0, 0.0]]]).astype(F))
    return arrays, len(p["type"])
