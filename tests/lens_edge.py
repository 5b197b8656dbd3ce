"""The blurred edge of the thin-lens expectation tests (tests/test_gpu_lens_expectation.py, tests/test_lens_host.py) - no GPU needed.

The camera sits at the origin and looks down -z (vup +y, vfov 40, orbit off), so hor runs along +x and the lens disc of radius R
lies in the plane z = 0.  The scene is ONE emitter in the plane z = -z0 that spans x in [-40, 0], y in [-40, 40], and max_depth is
1: a sample is Le if its primary ray meets the emitter and 0 otherwise, for both estimators.  A sample whose focal-plane point has
the abscissa p leaves the lens at x = R dx and crosses z = -z0 at x = R dx k + p z0 / f with k = 1 - z0 / f, which is <= 0 iff
dx <= c (k > 0) or dx >= c (k < 0), c = -p z0 / (f R k).  dx is the abscissa of a uniform point of the unit disc, whose distribution
function is G(c) = 1/2 + (c sqrt(1 - c^2) + asin c) / pi on [-1, 1].  So the sample is lit with probability G(c) for k > 0 and
1 - G(c) for k < 0, and a column's expected value is Le times the mean of that over the column's jitter interval.  y plays no
part: at z0 <= 20 a ray's |y| stays below 9, far inside the emitter.  Everything here is binary64."""
import numpy as np

import furnace as FN
import ptmi

F = np.float32
VFOV = 40.0
RADIUS, FOCUS = 1.0, 10.0
LE = FN.LE
Z_MAX = 5.0                                                    # tests/test_gpu_nee_expectation.py's
SE_FLOOR = 2e-5                                                # its floor on a standard error, as a share of the value


def camera():
    cam = ptmi.default_camera()
    cam.orbit = 0
    cam.origin[:] = (0.0, 0.0, 0.0); cam.lookat[:] = (0.0, 0.0, -1.0); cam.vup[:] = (0.0, 1.0, 0.0)
    cam.vfov_deg = VFOV
    return cam


def scene(z0, quad=True):
    """the emitter alone: (types, verts, normal, bsdf, Le) for load_scene_arrays"""
    s = FN.Scene(rho=(0.5, 0.5, 0.5), le=LE)
    c = [(-40.0, -40.0, -z0), (0.0, -40.0, -z0), (0.0, 40.0, -z0), (-40.0, 40.0, -z0)]
    if quad:
        s.quad(*c)
    else:
        s.tri(c[0], c[1], c[2]); s.tri(c[0], c[2], c[3])
    return s.arrays()


def disc_cdf(c):
    c = np.clip(np.asarray(c, np.float64), -1.0, 1.0)
    return 0.5 + (c * np.sqrt(1.0 - c * c) + np.arcsin(c)) / np.pi


def lit_probability(p, z0, radius=RADIUS, focus=FOCUS):
    """the probability that a sample whose focal-plane abscissa is p meets the emitter; radius 0: the pinhole's step"""
    p = np.asarray(p, np.float64)
    k = 1.0 - z0 / focus
    if radius == 0 or k == 0:
        return (p <= 0).astype(np.float64)
    g = disc_cdf(-p * z0 / (focus * radius * k))
    return g if k > 0 else 1.0 - g


def column_probability(width, height, z0, radius=RADIUS, focus=FOCUS):
    """(width,) the mean lit probability over each column's jitter interval, by a fixed 64-point Gauss rule"""
    half_w = (width / height) * np.tan(np.radians(VFOV) / 2.0) * focus       # the focal plane spans p in [-half_w, half_w]
    x, w = np.polynomial.legendre.leggauss(64)
    out = np.zeros(width)
    for col in range(width):
        u = (col + 0.5 + 0.5 * x) / width
        out[col] = 0.5 * np.dot(w, lit_probability((2.0 * u - 1.0) * half_w, z0, radius, focus))
    return out


def column_z(rad, prob, spp):
    """|column mean - expected| over its standard error, (width, 3).  The standard error is the analytic one - a sample is Le times
    a Bernoulli variable of the column's probability P, so a column of `rows` pixels of spp samples has the variance
    Le^2 P (1 - P) / (rows spp) - with the sibling tests' floor of 2e-5 of Le under it: a sample standard deviation would be 0 in
    the columns of the tails that happen to see no lit sample."""
    rad = np.asarray(rad, np.float64)
    le = np.asarray(LE, np.float64)
    mean = rad.mean(0)
    se = le[None] * np.sqrt(prob * (1.0 - prob) / (rad.shape[0] * spp))[:, None]
    return np.abs(mean - prob[:, None] * le[None]) / np.maximum(se, SE_FLOOR * le[None])


def image_z(rad, prob, spp):
    """the same for the whole-image mean, (3,)"""
    rad = np.asarray(rad, np.float64)
    le = np.asarray(LE, np.float64)
    se = le * np.sqrt((prob * (1.0 - prob)).sum() / (rad.shape[0] * spp)) / rad.shape[1]
    return np.abs(rad.reshape(-1, 3).mean(0) - prob.mean() * le) / np.maximum(se, SE_FLOOR * le)


def check_edge(tag, rad, z0, spp, radius=RADIUS):
    """every column's mean and the image's mean against the expected values, under Z_MAX; returns the probabilities"""
    h, w = rad.shape[:2]
    prob = column_probability(w, h, z0, radius)
    cz, iz = column_z(rad, prob, spp), image_z(rad, prob, spp)
    between = int(((prob > 1e-3) & (prob < 1 - 1e-3)).sum())
    print(f"{tag}: {between} columns carry intermediate values, column |z| max {cz.max():.2f} (column {int(cz.max(1).argmax())}), "
          f"image z {np.array2string(iz, precision=2)}")
    assert (cz < Z_MAX).all(), (tag, np.argwhere(cz >= Z_MAX)[:5], cz.max())
    assert (iz < Z_MAX).all(), (tag, iz)
    return prob
