"""Environment maps and open scenes of the environment-lighting tests, built from seeds - no GPU and no library needed.

Maps are (height, width, 3) float32 with row 0 at +y (include/ptmi.h: "environment lighting")."""
import numpy as np

import furnace as FN

F = np.float32


def sky_32x16():
    """the procedural sky of ptmi_scenes.sky at 32 x 16: a gradient, a dark ground and a one-texel sun"""
    import ptmi_scenes
    return ptmi_scenes.sky(32, 16)


def random_map(w, h, seed, lo=0.05, hi=2.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (h, w, 3)).astype(F)


def spike_map(w=8, h=6, seed=3):
    """one texel 1e9 times the rest: the rest of its row, and the other rows, become absorbed CDF steps"""
    m = random_map(w, h, seed, 0.5, 1.0)
    m[2, 5] *= F(1e9)
    return m


def constant_map(value, w=1, h=1):
    return np.broadcast_to(np.asarray(value, F), (h, w, 3)).copy()


HOST_MAPS = {
    "1x1": lambda: constant_map((0.7, 0.8, 0.9)),
    "4x2": lambda: random_map(4, 2, 11),
    "7x5": lambda: random_map(7, 5, 12),
    "32x16": sky_32x16,
    "spike": spike_map,
    "zero": lambda: np.zeros((3, 4, 3), F),
}


def without_box(name):
    """furnace.variant(name) with its enclosing box left out: an open scene.  box() comes first: 12 triangles or 6 quads."""
    s = FN.variant(name)
    n_box = 6 if s.t[0] == 1 else 12
    for lst in (s.t, s.v, s.n, s.b, s.e):
        del lst[:n_box]
    return s


def soup(seed=5, n=200, emitters=True):
    """about 200 triangles in front of the default camera with gaps between them (the certified walk); three emitters, or none"""
    rng = np.random.default_rng(seed)
    centers = np.stack([rng.uniform(-3, 3, n), rng.uniform(0.2, 5.0, n), rng.uniform(-5.5, 0.5, n)], 1)[:, None, :]
    verts = (centers + rng.normal(0, 0.6, (n, 4, 3))).astype(F)
    e1 = verts[:, 1] - verts[:, 0]; e2 = verts[:, 2] - verts[:, 0]
    normal = np.cross(e1, e2); normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    bsdf = rng.uniform(0.2, 0.9, (n, 3)).astype(F)
    Le = np.zeros((n, 3), F)
    if emitters:
        Le[7] = (12.0, 12.0, 12.0); Le[60] = (0.0, 3.0, 0.5); Le[150] = (40.0, 10.0, 2.0)
    return np.zeros(n, np.int32), verts, normal.astype(F), bsdf, Le


def cube(rho, le, center=(0.0, 2.5, 0.0), half=1.5):
    """a closed convex body: 12 triangles with outward geometric (and stored) normals, Kd = rho, Le = le"""
    s = FN.Scene(rho=rho, le=le)
    c = np.asarray(center, np.float64)
    for a in range(3):
        u, w = (a + 1) % 3, (a + 2) % 3
        for side in (-1.0, 1.0):
            def p(du, dw):
                x = np.zeros(3); x[a] = side * half; x[u] = du * half; x[w] = dw * half
                return c + x
            q = [p(-1, -1), p(1, -1), p(1, 1), p(-1, 1)]
            if side < 0:
                q = q[::-1]                                  # cross(e_u, e_w) = +e_a: reverse the winding on the - side
            s.tri(q[0], q[1], q[2]); s.tri(q[0], q[2], q[3])
    return s


def ground_quad(rho, tilt_deg=0.0, half=400.0, y=0.0):
    """one large quad facing up (+y), tilted about the z axis by tilt_deg, Le = 0; large enough to fill the default view's
    lower part and flat, so that a cosine sample from it never returns to it"""
    s = FN.Scene(rho=rho, le=(0.0, 0.0, 0.0))
    th = np.radians(tilt_deg)
    ex = np.array([np.cos(th), np.sin(th), 0.0]); ez = np.array([0.0, 0.0, 1.0])
    c = np.array([0.0, y, 0.0])
    # v00, v10, v11, v01 with cross(v10 - v00, v01 - v00) = cross(ez, ex) * 4 half^2 -> the normal (-sin, cos, 0): up
    s.quad(c - half * ex - half * ez, c - half * ex + half * ez, c + half * ex + half * ez, c + half * ex - half * ez)
    return s


# ------------------------------------------------------------------------------------------------
# the ground quad under a sun: the analytic side, in binary64
# ------------------------------------------------------------------------------------------------
SUN_W, SUN_H, SUN_ROW, SUN_COL = 32, 16, 3, 5
N_GPU = 128 * 128 * 1024                                 # samples of a GPU expectation frame (test_gpu_nee_expectation's constants)
CAP = 0.005                                              # 5 SE <= 0.5 % of the value


def band_edges(h):
    """z_r as the library stores them (float32 of cos(pi r / h)), in binary64"""
    z = np.cos(np.pi * np.arange(h + 1) / h).astype(F).astype(np.float64)
    z[0], z[-1] = 1.0, -1.0
    return z


def form_factors_flat(w=SUN_W, h=SUN_H):
    """F_rj = (1 / pi) * integral of cos(theta) over texel (r, j), for an up-facing surface: (1 / w)(z_r^2 - z_{r+1}^2) on the
    upper rows, 0 below the horizon (closed form)"""
    z = np.maximum(band_edges(h), 0.0)
    return np.repeat(((z[:-1] ** 2 - z[1:] ** 2) / w)[:, None], w, axis=1)


def form_factors_quadrature(normal, rotation_deg, K, w=SUN_W, h=SUN_H):
    """the same for any surface normal and map rotation, by the midpoint rule on K x K cells per texel:
    F_rj = (1 / pi) * integral over the texel of max(0, n . omega) dz dphi, omega = (s cos phi, z, s sin phi), s = sqrt(1 - z^2)"""
    z = band_edges(h)
    n = np.asarray(normal, np.float64); n = n / np.linalg.norm(n)
    t = (np.arange(K) + 0.5) / K
    phi = 2.0 * np.pi * ((np.arange(w)[:, None] + t[None, :]) / w + rotation_deg / 360.0)        # (w, K)
    cp, sp = np.cos(phi), np.sin(phi)
    out = np.zeros((h, w))
    for r in range(h):
        zz = z[r + 1] + t * (z[r] - z[r + 1])                                                    # (K,)
        s = np.sqrt(np.maximum(0.0, 1.0 - zz * zz))
        dot = n[1] * zz[None, :, None] + s[None, :, None] * (n[0] * cp[:, None, :] + n[2] * sp[:, None, :])   # (w, K, K)
        out[r] = np.maximum(dot, 0.0).mean(axis=(1, 2)) * (z[r] - z[r + 1]) * (2.0 * np.pi / w) / np.pi
    return out


def sun_map(radiance, w=SUN_W, h=SUN_H):
    """sky 1 on the upper rows, ground rows 0, one sun texel of `radiance`"""
    m = np.zeros((h, w, 3), F)
    m[: h // 2] = 1.0
    m[SUN_ROW, SUN_COL] = radiance
    return m


def sun_moments(Fm, a):
    """(sum F E, sum F E^2) of sun_map(a) per unit albedo"""
    E = sun_map(a)[..., 0].astype(np.float64)
    return float((Fm * E).sum()), float((Fm * E * E).sum())


def sun_radiance_for_cap(Fm, margin=0.9):
    """The largest sun radiance at which the plain estimator's 5 SE stays at margin x CAP of the value at N_GPU samples:
    per unit albedo V = sum F E and Var = sum F E^2 - V^2 per sample (cosine sampling picks texel (r, j) with probability F_rj),
    so the condition is 5 sqrt(Var / N_GPU) = margin * CAP * V.  Bisection; rounded down to a float32."""
    def excess(a):
        v, m2 = sun_moments(Fm, a)
        return 5.0 * np.sqrt(max(m2 - v * v, 0.0) / N_GPU) - margin * CAP * v
    lo, hi = 1.0, 1.0e4
    assert excess(lo) < 0 < excess(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if excess(mid) < 0 else (lo, mid)
    return float(np.floor(lo))


def tilted_normal(tilt_deg):
    th = np.radians(tilt_deg)
    return np.array([-np.sin(th), np.cos(th), 0.0])


def sun_case(tilt_deg=0.0, rotation_deg=0.0):
    """(map, F, V, Var) of a ground-quad case per unit albedo: the flat case in closed form, any other by quadrature refined
    until doubling K changes V by less than 1e-5 relative"""
    if tilt_deg == 0.0 and rotation_deg == 0.0:
        Fm = form_factors_flat()
    else:
        K, prev = 16, None
        while True:
            Fm = form_factors_quadrature(tilted_normal(tilt_deg), rotation_deg, K)
            v = sun_moments(Fm, 64.0)[0]                 # a fixed probe radiance: the value the refinement watches
            if prev is not None and abs(v - prev) < 1e-5 * abs(v):
                break
            prev, K = v, 2 * K
            assert K <= 1024
    a = sun_radiance_for_cap(Fm)
    v, m2 = sun_moments(Fm, a)
    return sun_map(a), Fm, v, m2 - v * v


def top_down_camera(tilt_deg=0.0, distance=10.0):
    """a camera on the quad's normal looking straight at it: every pixel hits the quad"""
    import ptmi
    n = tilted_normal(tilt_deg)
    cam = ptmi.default_camera()
    cam.origin[:] = tuple(distance * n); cam.lookat[:] = (0.0, 0.0, 0.0); cam.vup[:] = (0.0, 0.0, -1.0)
    cam.orbit = 0
    return cam
