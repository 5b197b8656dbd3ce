"""Scenes of the specular-surface tests (include/ptmi.h: "specular surfaces"), as furnace.Scene objects with their kind arrays - no
GPU needed to build them.  Geometry in front of the camera is laid out in the camera's own frame (ptmi.host_camera_frame)."""
import numpy as np

import furnace as FN
import ptmi

F = np.float32
MIRROR, GLASS = 1, 2
BLACK = (0.0, 0.0, 0.0)
WHITE = (1.0, 1.0, 1.0)
# The black furnace's max_depth.  SpecRenderer on black_furnace() at 16 x 16 x 64 spp (16 384 samples, default camera) cuts off
# 0 samples at max_depth 32 (the deepest vertex seen is at depth 6: a ray that enters the cuboid leaves it after a few internal
# reflections); the condition is a share <= 1e-4, so the starting depth stands.  test_specular_host.py checks it.
BLACK_FURNACE_DEPTH = 32


def view_axes(cam, width, height):
    """(origin, forward, right, up) of the camera, binary64 unit vectors: forward through the image centre"""
    f = ptmi.host_camera_frame(cam, width, height).astype(np.float64)
    origin, llc, hor, ver = f[0:3], f[3:6], f[6:9], f[9:12]
    fwd = llc + 0.5 * hor + 0.5 * ver - origin
    unit = lambda v: v / np.linalg.norm(v)
    return origin, unit(fwd), unit(hor), unit(ver)


def pixel_angles(cam, width, height):
    """the angle between the ray through every pixel's centre and the view axis, (height, width), row 0 = bottom"""
    f = ptmi.host_camera_frame(cam, width, height).astype(np.float64)
    origin, llc, hor, ver = f[0:3], f[3:6], f[6:9], f[9:12]
    u = (np.arange(width) + 0.5) / width
    v = (np.arange(height) + 0.5) / height
    d = llc[None, None] + u[None, :, None] * hor + v[:, None, None] * ver - origin
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    fwd = llc + 0.5 * hor + 0.5 * ver - origin
    return np.arccos(np.clip(d @ (fwd / np.linalg.norm(fwd)), -1.0, 1.0))


def cuboid(s, center, a, b, c, le=None, rho=None):
    """a closed box with half-edge vectors a, b, c (right-handed): 12 triangles with outward geometric and stored normals"""
    center, a, b, c = (np.asarray(x, np.float64) for x in (center, a, b, c))
    assert np.dot(np.cross(a, b), c) > 0, "right-handed half-edges"
    first = len(s)
    for n, u, w in ((a, b, c), (b, c, a), (c, a, b)):
        for side in (1.0, -1.0):
            q = [center + side * n - u - w, center + side * n + u - w, center + side * n + u + w, center + side * n - u + w]
            if side < 0:
                q = q[::-1]                                  # cross(u, w) = +n: reverse the winding on the - side
            s.tri(q[0], q[1], q[2], le=le); s.tri(q[0], q[2], q[3], le=le)
    if rho is not None:
        for k in range(first, len(s)):
            s.b[k] = rho
    return list(range(first, len(s)))


def mirror_and_emitter(cam, width, height, tint=(0.5, 0.25, 1.0), le=(1.0, 0.75, 0.5)):
    """A mirror quad at 45 degrees that fills the view, and above it an emitter quad (rho = 0) that catches every reflected ray:
    every pixel's radiance is tint * le at max_depth >= 2"""
    o, fwd, right, up = view_axes(cam, width, height)
    s = FN.Scene(rho=BLACK, le=BLACK)
    c = o + 5.0 * fwd
    along = (fwd + up) / np.sqrt(2.0)                        # in the mirror's plane; its normal (up - fwd) / sqrt 2 faces the camera
    s.quad(c - 10 * right - 10 * along, c + 10 * right - 10 * along, c + 10 * right + 10 * along, c - 10 * right + 10 * along)
    s.b[0] = tint
    e = c + 20.0 * up
    s.quad(e - 100 * right - 100 * fwd, e - 100 * right + 100 * fwd, e + 100 * right + 100 * fwd, e + 100 * right - 100 * fwd, le=le)
    kind = np.array([MIRROR, 0], np.int32)
    return s, kind


def glass_slab(cam, width, height, le, ior_tint=WHITE):
    """A closed thin glass box across the view axis, wider than the view, between the camera and a black emitter wider still;
    nothing behind the camera.  A pixel's expected radiance is le * (1 - F) / (1 + F) with the Fresnel term F at its angle."""
    o, fwd, right, up = view_axes(cam, width, height)
    s = FN.Scene(rho=BLACK, le=BLACK)
    idx = cuboid(s, o + 6.0 * fwd, 40.0 * right, 40.0 * up, -0.05 * fwd, rho=ior_tint)
    e = o + 12.0 * fwd
    s.quad(e - 400 * right - 400 * up, e + 400 * right - 400 * up, e + 400 * right + 400 * up, e - 400 * right + 400 * up, le=le)
    kind = np.zeros(len(s), np.int32); kind[idx] = GLASS
    return s, kind


def black_furnace(le=FN.LE, quads=False, chain=False):
    """furnace.box with rho = 0 and Le = le around the default camera; inside, mirror panels (tint 1) whose stored normals are
    tilted against their planes and a closed glass cuboid (tint 1).  Every path ends on a wall with throughput 1: every pixel's
    expectation is le.  chain: furnace's deep chain outside the box (the stack walk)."""
    s = FN.Scene(rho=BLACK, le=le)
    FN.box(s, quads=quads)
    kind = [0] * len(s)
    rng = np.random.default_rng(9)
    for k in range(4):                                       # panels in front of the camera, seen from both sides by later bounces
        c = np.array([-4.5 + 3.0 * k, 2.0 + 0.7 * k, -2.0 - 1.5 * k])
        n = FN._unit(rng.normal(0, 1, 3) + (0.0, 0.0, 1.5))
        t = FN._unit(np.cross(n, (0.0, 1.0, 0.0))); b = np.cross(n, t)
        stored = FN._unit(n + 0.35 * (np.cos(k) * t + np.sin(k) * b))      # about 19 degrees off the plane normal
        corners = (c - 1.6 * t - 1.6 * b, c + 1.6 * t - 1.6 * b, c + 1.6 * t + 1.6 * b, c - 1.6 * t + 1.6 * b)
        if quads:
            s.quad(*corners, normal=stored, le=BLACK)
        else:
            s.tri(corners[0], corners[1], corners[2], normal=stored, le=BLACK)
            s.tri(corners[0], corners[2], corners[3], normal=stored, le=BLACK)
        while len(kind) < len(s):
            kind.append(MIRROR); s.b[len(kind) - 1] = WHITE
    ax = FN._unit((1.0, 0.2, 0.3)); ay = FN._unit(np.cross((0.0, 1.0, 0.0), ax)); az = np.cross(ax, ay)
    for k in cuboid(s, (1.0, 3.2, 1.0), 1.5 * ax, 0.8 * ay, 1.0 * az, le=BLACK, rho=WHITE):
        kind.append(GLASS)
    if chain:
        n0 = len(s)
        FN._chain(s, quads=quads)
        kind += [0] * (len(s) - n0)
    return s, np.array(kind, np.int32)
