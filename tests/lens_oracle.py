"""CPU restatement of the thin lens (include/ptmi.h: "thin lens"), written from the header in numpy float32: the lens block, the
disc map, the lens ray, and the per-lane estimator with it - LensRenderer is PathRenderer (tests/path_oracle.py) with ONE change,
the frame its camera ray is taken over.  The change is a mixin over sample: it makes the two lens draws, puts the per-sample frame
(o, llc_f, hor_f, ver_f) in place of the renderer's and lets the next class draw the jitter and call the sensor's get_ray on it,
so it composes with SmoothRenderer and TexturedSmoothRenderer."""
import ctypes as C

import numpy as np

from nee_oracle import _dot, _unit, f32
from oracle_binding import CameraFrame, camera_frame, oracle_lib
from path_oracle import PathRenderer
from smooth_oracle import SmoothRenderer
from texture_oracle import TexturedSmoothRenderer

TWO23 = 1 << 23


def _length(v):
    return f32(np.sqrt(_dot(v, v)))


def _size_reciprocal(n):
    return f32(f32(1.0) / f32(n)) if 1 <= n <= TWO23 else f32(0.0)


def lens_block(frame12, width, height, radius, focus_distance):
    """THE LENS BLOCK (6, 4) float32 over the frame (org, llc, hor, ver): (llc_f, W) (hor_f, 1/W) (ver_f, H) (org, 1/H) (a, 0) (b, 0)"""
    org, llc, hor, ver = (np.asarray(frame12, f32).reshape(4, 3)[i] for i in range(4))
    f, R = f32(focus_distance), f32(radius)
    with np.errstate(all="ignore"):
        hor_f = (f * hor).astype(f32)
        ver_f = (f * ver).astype(f32)
        llc_f = (org + (f * (llc - org).astype(f32)).astype(f32)).astype(f32)
        a = (f32(R / _length(hor)) * hor).astype(f32)
        b = (f32(R / _length(ver)) * ver).astype(f32)
    iw, ih = _size_reciprocal(width), _size_reciprocal(height)
    if iw == 0 or ih == 0:
        iw = ih = f32(0.0)
    out = np.zeros((6, 4), f32)
    out[0, :3], out[0, 3] = llc_f, f32(width)
    out[1, :3], out[1, 3] = hor_f, iw
    out[2, :3], out[2, 3] = ver_f, f32(height)
    out[3, :3], out[3, 3] = org, ih
    out[4, :3] = a
    out[5, :3] = b
    return out


def disc(r3, r4):
    """(dx, dy) of the two lens draws: rho = sqrtf(r3), phi = (float)(2 pi r4) with the product in binary64, ptmi_sincosf"""
    rho = f32(np.sqrt(f32(r3)))
    phi = f32(2.0 * np.pi * float(f32(r4)))
    s, c = C.c_float(), C.c_float()
    oracle_lib().po_sincosf(phi, C.byref(s), C.byref(c))
    return f32(rho * f32(c.value)), f32(rho * f32(s.value))


def lens_origin(block, r3, r4):
    """o = (org + dx * a) + dy * b"""
    dx, dy = disc(r3, r4)
    return ((block[3, :3] + (dx * block[4, :3]).astype(f32)).astype(f32) + (dy * block[5, :3]).astype(f32)).astype(f32)


def lens_ray(block, x, y, r3, r4, r1, r2):
    """THE LENS RAY (o, d) of pixel (x, y) for the four uniforms, every operation spelled out"""
    block = np.asarray(block, f32)
    o = lens_origin(block, r3, r4)
    u = f32(f32(f32(x) + f32(r1)) / block[0, 3])
    v = f32(f32(f32(y) + f32(r2)) / block[2, 3])
    w = (((block[0, :3] + (u * block[1, :3]).astype(f32)).astype(f32) + (v * block[2, :3]).astype(f32)).astype(f32) - o).astype(f32)
    return o, _unit(w).astype(f32)


def sample_frame(block, o):
    """the per-sample frame (o, llc_f, hor_f, ver_f) as the oracle's CameraFrame"""
    cf = CameraFrame()
    for k in range(3):
        cf.origin[k] = float(o[k]); cf.lower_left_corner[k] = float(block[0, k])
        cf.horizontal[k] = float(block[1, k]); cf.vertical[k] = float(block[2, k])
    return cf


class LensMixin:
    """ONE change over the renderer it is mixed into: a sample starts on the lens.  radius (> 0) and focus_distance are keyword
    arguments; everything else goes on to the next class."""

    def __init__(self, *args, radius, focus_distance, **kw):
        super().__init__(*args, **kw)
        if not radius > 0:
            raise ValueError("radius 0 is the pinhole: use the renderer without the mixin")
        self.block = lens_block(self.cf.as_array(), self.w, self.h, radius, focus_distance)

    def sample(self, x, y, st, max_depth):
        r3 = self._u(st)
        r4 = self._u(st)
        pinhole = self.cf
        self.cf = sample_frame(self.block, lens_origin(self.block, r3, r4))
        try:
            return super().sample(x, y, st, max_depth)      # draws the jitter and takes get_ray over self.cf
        finally:
            self.cf = pinhole


class LensRenderer(LensMixin, PathRenderer):
    """PathRenderer through a thin lens"""


class LensSmoothRenderer(LensMixin, SmoothRenderer):
    """SmoothRenderer (the vertex-normal table is its 5th positional argument) through a thin lens"""


class LensTexturedSmoothRenderer(LensMixin, TexturedSmoothRenderer):
    """TexturedSmoothRenderer (vertex normals and an albedo texture together) through a thin lens"""


def frame_of(cam, width, height):
    """the 12 floats of the oracle's camera frame for cam at width x height"""
    return camera_frame(cam, width, height).as_array()
