"""ctypes bindings for the CHECKER libraries under oracle/ (test infrastructure only).

oracle/libptmi_oracle.so  - plain-C CPU restatement (ptmi_oracle.c)
oracle/_ref/libptmi_ref.so - the reference's own geometry headers compiled from
                             /root/reference (present only where it was built)
oracle/_ref/libptmi_ref_solver.so - the reference's radiosity pre-pass (ref_solver_harness.cpp), likewise
"""
import ctypes as C
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SO = os.environ.get("PTMI_ORACLE_LIB") or os.path.join(ROOT, "oracle", "libptmi_oracle.so")   # override: sanitizer builds of the checker
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libptmi_ref.so")
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


class Camera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("lookat", C.c_float * 3), ("vup", C.c_float * 3),
                ("vfov_deg", C.c_float), ("yaw_deg", C.c_float), ("pitch_deg", C.c_float),
                ("orbit", C.c_int)]


def default_camera():
    """AppConfig defaults (application_state.h:285-286) + Sensor yaw/pitch (sensor.h:24-25)."""
    return Camera((0.5, 3.0, 8.5), (0.0, 2.5, 0.0), (0.0, 1.0, 0.0), 40.0, 90.0, 0.0, 1)


class CameraFrame(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("lower_left_corner", C.c_float * 3),
                ("horizontal", C.c_float * 3), ("vertical", C.c_float * 3)]

    def as_array(self):
        return np.array(list(self.origin) + list(self.lower_left_corner) +
                        list(self.horizontal) + list(self.vertical), dtype=np.float32)


class Stats(C.Structure):
    _fields_ = [("seconds", C.c_double), ("samples", C.c_uint64), ("rays", C.c_uint64),
                ("node_visits", C.c_uint64), ("prim_tests", C.c_uint64), ("hits", C.c_uint64)]


class RadiosityParams(C.Structure):
    """RadiosityState / AppConfig defaults (application_state.h:207-209, 290-291)"""
    _fields_ = [("num_iterations", C.c_int), ("mc_samples", C.c_int), ("use_monte_carlo", C.c_int),
                ("enable_filtering", C.c_int), ("use_bilateral", C.c_int),
                ("filter_sigma_spatial", C.c_float), ("filter_sigma_range", C.c_float)]

    def __init__(self, num_iterations=10, mc_samples=64, use_monte_carlo=True, enable_filtering=False, use_bilateral=True,
                 filter_sigma_spatial=1.5, filter_sigma_range=0.3):
        super().__init__(num_iterations, mc_samples, int(use_monte_carlo), int(enable_filtering), int(use_bilateral),
                         filter_sigma_spatial, filter_sigma_range)


class Hit(C.Structure):
    _fields_ = [("hit", C.c_int), ("prim", C.c_int), ("t", C.c_float), ("p", C.c_float * 3),
                ("n", C.c_float * 3), ("bsdf", C.c_float * 3), ("Le", C.c_float * 3),
                ("node_visits", C.c_int), ("prim_tests", C.c_int)]


class RefHit(C.Structure):
    _fields_ = [("hit", C.c_int), ("prim", C.c_int), ("t", C.c_float), ("p", C.c_float * 3),
                ("n", C.c_float * 3), ("bsdf", C.c_float * 3), ("Le", C.c_float * 3)]


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


_oracle = None


def oracle_lib():
    global _oracle
    if _oracle is None:
        if not os.path.exists(ORACLE_SO):
            raise RuntimeError(f"{ORACLE_SO} missing: run `make -C oracle` (or __graft_entry__.build())")
        L = C.CDLL(ORACLE_SO)
        L.po_scene_load.restype = C.c_void_p
        L.po_scene_load.argtypes = [C.c_char_p, C.c_int, C.c_int]
        L.po_scene_from_arrays.restype = C.c_void_p
        L.po_scene_from_arrays.argtypes = [C.c_int] + [C.c_void_p] * 5
        L.po_scene_free.argtypes = [C.c_void_p]
        L.po_scene_num_prims.argtypes = [C.c_void_p]
        L.po_scene_num_nodes.argtypes = [C.c_void_p]
        L.po_scene_get_prims.argtypes = [C.c_void_p] * 6
        L.po_scene_get_bvh.argtypes = [C.c_void_p] * 7
        L.po_camera_frame_setup.argtypes = [C.POINTER(Camera), C.c_int, C.c_int, C.POINTER(CameraFrame)]
        L.po_camera_ray.argtypes = [C.POINTER(CameraFrame), C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        L.po_rng_init.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
        L.po_rng_uniform.restype = C.c_float
        L.po_rng_uniform.argtypes = [C.c_void_p]
        L.po_sincosf.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.po_powf.restype = C.c_float
        L.po_powf.argtypes = [C.c_float, C.c_float]
        L.po_sample_cosine_hemisphere.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p]
        L.po_intersect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.POINTER(Hit)]
        L.po_render.restype = C.c_int
        L.po_scene_set_radiosity_grids.argtypes = [C.c_void_p, C.c_void_p]
        L.po_scene_set_mis_fraction.argtypes = [C.c_void_p, C.c_float]
        L.po_scene_get_cdfs.argtypes = [C.c_void_p, C.c_void_p]
        L.po_scene_set_radiosity.argtypes = [C.c_void_p, C.c_void_p]
        L.po_render_radiosity.restype = C.c_int
        L.po_render_radiosity.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int,
                                          C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.po_acosf.restype = C.c_float; L.po_acosf.argtypes = [C.c_float]
        L.po_expf.restype = C.c_float; L.po_expf.argtypes = [C.c_float]
        L.po_atan2f.restype = C.c_float; L.po_atan2f.argtypes = [C.c_float, C.c_float]
        L.po_math_batch.restype = None; L.po_math_batch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.po_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_uint64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.po_radiosity_solve.restype = C.c_int
        L.po_radiosity_solve.argtypes = [C.c_void_p, C.POINTER(RadiosityParams), C.c_int] + [C.c_void_p] * 6
        vp, f, u32 = C.c_void_p, C.c_float, C.c_uint32
        L.po_xorwow_script.argtypes = [vp, C.c_int, vp]
        L.po_xorwow_next_raw.argtypes = [vp, C.c_int, vp]
        L.po_word_to_uniform.restype = f; L.po_word_to_uniform.argtypes = [u32]
        L.po_sample_cosine_words.argtypes = [vp, vp, C.c_int, vp]
        L.po_mis_power_heuristic.restype = f; L.po_mis_power_heuristic.argtypes = [f, f]
        L.po_grid_sample.argtypes = [vp, vp, vp, C.c_int, vp, vp]
        L.po_grid_pdf.restype = f; L.po_grid_pdf.argtypes = [vp, vp, vp]
        L.po_sample_mis.argtypes = [vp, vp, f, vp, C.c_int, vp, vp, vp]
        L.po_tonemap.argtypes = [vp, vp]; L.po_tonemap.restype = None
        L.po_average.argtypes = [vp, C.c_int, vp]; L.po_average.restype = None
        L.po_scene_apply_grid_filter.restype = C.c_int
        L.po_scene_apply_grid_filter.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        L.po_form_factor_rows.restype = C.c_int
        L.po_form_factor_rows.argtypes = [C.c_void_p, C.POINTER(RadiosityParams), C.c_int, C.c_int] + [C.c_void_p] * 3
        L.po_prim_geometry.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_void_p]
        L.po_prim_sample_uniform.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p]
        L.po_direction_to_grid_index.restype = C.c_int
        L.po_direction_to_grid_index.argtypes = [C.c_void_p, C.c_void_p]
        L.po_visibility_blocked.restype = C.c_int
        L.po_visibility_blocked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int]
        L.po_cdf_layout.argtypes = [C.c_void_p]; L.po_cdf_layout.restype = None
        L.po_grid_constants.argtypes = [C.c_void_p]; L.po_grid_constants.restype = None
        L.po_radiosity_grid_update.argtypes = [C.c_int] + [vp] * 4 + [C.c_int, C.c_int, f, f, vp]
        L.po_filter_pdfs.argtypes = [C.c_int, vp, vp, C.c_int, f, f, vp, vp]
        L.po_cdf_records.argtypes = [C.c_int, vp, vp]
        L.po_form_factor_mc_pair_words.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp]
        _oracle = L
    return _oracle


class OracleScene:
    def __init__(self, handle):
        if not handle:
            raise RuntimeError("oracle: scene load failed")
        self.h = handle
        self.L = oracle_lib()

    @classmethod
    def load(cls, path, subdivision=0, convert_quads=False):
        return cls(oracle_lib().po_scene_load(path.encode(), int(subdivision), int(bool(convert_quads))))

    @classmethod
    def from_arrays(cls, types, verts, normal, bsdf, Le):
        types = np.ascontiguousarray(types, np.int32)
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 4, 3)
        normal, bsdf, Le = (np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (normal, bsdf, Le))
        n = len(types)
        assert verts.shape[0] == n and normal.shape[0] == n
        return cls(oracle_lib().po_scene_from_arrays(n, types.ctypes.data, verts.ctypes.data, normal.ctypes.data,
                                                     bsdf.ctypes.data, Le.ctypes.data))

    def __del__(self):
        try:
            self.L.po_scene_free(self.h)
        except Exception:
            pass

    @property
    def n_prims(self):
        return self.L.po_scene_num_prims(self.h)

    @property
    def n_nodes(self):
        return self.L.po_scene_num_nodes(self.h)

    def prims(self):
        n = self.n_prims
        t = np.zeros(n, np.int32); v = np.zeros((n, 4, 3), np.float32)
        nr = np.zeros((n, 3), np.float32); b = np.zeros((n, 3), np.float32); le = np.zeros((n, 3), np.float32)
        self.L.po_scene_get_prims(self.h, t.ctypes.data, v.ctypes.data, nr.ctypes.data, b.ctypes.data, le.ctypes.data)
        return dict(type=t, verts=v, normal=nr, bsdf=b, Le=le)

    def bvh(self):
        n, m = self.n_nodes, self.n_prims
        bmin = np.zeros((n, 3), np.float32); bmax = np.zeros((n, 3), np.float32)
        left = np.zeros(n, np.int32); right = np.zeros(n, np.int32); count = np.zeros(n, np.int32)
        idx = np.zeros(m, np.int32)
        self.L.po_scene_get_bvh(self.h, bmin.ctypes.data, bmax.ctypes.data, left.ctypes.data, right.ctypes.data,
                                count.ctypes.data, idx.ctypes.data)
        return dict(bmin=bmin, bmax=bmax, left=left, right=right, count=count, indices=idx)

    def intersect(self, o, d, t_min=1e-4, t_max=3.4028234663852886e38, use_bvh=True):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32)
        h = Hit()
        self.L.po_intersect(self.h, o.ctypes.data, d.ctypes.data, t_min, t_max, int(use_bvh), C.byref(h))
        return h

    def set_radiosity_grids(self, rgb):
        """rgb: (n_prims, 256, 3) float32 or None"""
        if rgb is None:
            self.L.po_scene_set_radiosity_grids(self.h, None); return
        rgb = np.ascontiguousarray(rgb, np.float32)
        assert rgb.shape == (self.n_prims, 256, 3)
        self.L.po_scene_set_radiosity_grids(self.h, rgb.ctypes.data)

    def set_radiosity(self, rgb):
        if rgb is None:
            self.L.po_scene_set_radiosity(self.h, None); return
        rgb = np.ascontiguousarray(rgb, np.float32)
        assert rgb.shape == (self.n_prims, 3)
        self.L.po_scene_set_radiosity(self.h, rgb.ctypes.data)

    def render_radiosity(self, cam, width, height, spp, seed_base=2023, y0=0, y1=None, n_threads=0, rng_state=None, reset_rng=True):
        y1 = height if y1 is None else y1
        rgb = np.zeros((height, width, 3), np.uint8); rad = np.zeros((height, width, 3), np.float32)
        rc = self.L.po_render_radiosity(self.h, C.byref(cam), width, height, spp, seed_base, int(reset_rng),
                                        None if rng_state is None else rng_state.ctypes.data, y0, y1, n_threads,
                                        rgb.ctypes.data, rad.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"po_render_radiosity failed: {rc}")
        return rgb, rad

    def radiosity_solve(self, n_threads=0, **params):
        """runSolver + precomputeCDFs (ui_windows.h:185-192); returns dict of the solver's outputs (load order)."""
        n = self.n_prims
        prm = RadiosityParams(**params)
        out = dict(form_factors=np.zeros((n, n), np.float32), radiosity=np.zeros((n, 3), np.float32),
                   unshot=np.zeros((n, 3), np.float32), grid=np.zeros((n, 256), np.float32),
                   radiosity_grid=np.zeros((n, 256, 3), np.float32))
        rays = C.c_uint64(0)
        rc = self.L.po_radiosity_solve(self.h, C.byref(prm), n_threads, out["form_factors"].ctypes.data, out["radiosity"].ctypes.data,
                                       out["unshot"].ctypes.data, out["grid"].ctypes.data, out["radiosity_grid"].ctypes.data,
                                       C.addressof(rays))
        if rc != 0:
            raise RuntimeError(f"po_radiosity_solve failed: {rc}")
        out["rays"] = rays.value
        return out

    def apply_grid_filter(self, use_bilateral=True, sigma_spatial=1.5, sigma_range=0.3):
        """"Apply Filter & Rebuild CDFs" (ui_windows.h:154-167); returns the filtered, normalised (formfactor, radiosity) pdfs"""
        ff = np.zeros((self.n_prims, 256), np.float32); rad = np.zeros((self.n_prims, 256), np.float32)
        rc = self.L.po_scene_apply_grid_filter(self.h, int(use_bilateral), sigma_spatial, sigma_range, ff.ctypes.data, rad.ctypes.data)
        if rc != 0:
            raise RuntimeError("apply_grid_filter: the scene has no radiosity grids")
        return ff, rad

    def form_factor_rows(self, rows, n_threads=0, **params):
        rows = np.ascontiguousarray(rows, np.int32)
        prm = RadiosityParams(**params)
        ff = np.zeros((len(rows), self.n_prims), np.float32); grid = np.zeros((len(rows), 256), np.float32)
        rc = self.L.po_form_factor_rows(self.h, C.byref(prm), n_threads, len(rows), rows.ctypes.data, ff.ctypes.data, grid.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"po_form_factor_rows failed: {rc}")
        return ff, grid

    def mc_pair_words(self, i, j, n_samples, words):
        """po_form_factor_mc_pair_words: dict(F, grid (256), rad_grid (256, 3), used, overrun) of pair (i, j) on scripted raw words."""
        w = np.ascontiguousarray(words, np.uint32)
        F = C.c_float(); over = C.c_int(); grid = np.zeros(256, np.float32); rg = np.zeros((256, 3), np.float32)
        used = self.L.po_form_factor_mc_pair_words(self.h, int(i), int(j), int(n_samples), w.ctypes.data, len(w), C.addressof(F),
                                                   grid.ctypes.data, rg.ctypes.data, C.addressof(over))
        assert used >= 0
        return dict(F=np.float32(F.value), grid=grid, rad_grid=rg, used=np.int32(used), overrun=np.int32(over.value))

    def prim_geometry(self, i):
        a = C.c_float(0); c = np.zeros(3, np.float32)
        self.L.po_prim_geometry(self.h, i, C.byref(a), c.ctypes.data)
        return np.float32(a.value), c

    def sample_uniform(self, i, r1, r2):
        out = np.zeros(3, np.float32)
        self.L.po_prim_sample_uniform(self.h, i, float(r1), float(r2), out.ctypes.data)
        return out

    def set_mis_fraction(self, f):
        self.L.po_scene_set_mis_fraction(self.h, float(f))

    def cdfs(self):
        out = np.zeros((self.n_prims, 530), np.float32)
        return out if self.L.po_scene_get_cdfs(self.h, out.ctypes.data) else None

    def render(self, cam, width, height, spp, max_depth=5, seed_base=2023, y0=0, y1=None, n_threads=0,
               rng_state=None, reset_rng=True, sampling_mode=0):
        y1 = height if y1 is None else y1
        rgb = np.zeros((height, width, 3), np.uint8)
        rad = np.zeros((height, width, 3), np.float32)
        st = Stats()
        rc = self.L.po_render(self.h, C.byref(cam), width, height, spp, max_depth, int(sampling_mode), seed_base, int(reset_rng),
                              None if rng_state is None else rng_state.ctypes.data, y0, y1, n_threads,
                              rgb.ctypes.data, rad.ctypes.data, C.byref(st))
        if rc != 0:
            raise RuntimeError(f"po_render failed: {rc}")
        return rgb, rad, st


def camera_frame(cam, width, height):
    cf = CameraFrame()
    oracle_lib().po_camera_frame_setup(C.byref(cam), width, height, C.byref(cf))
    return cf


def camera_ray(cf, u, v):
    o = np.zeros(3, np.float32); d = np.zeros(3, np.float32)
    oracle_lib().po_camera_ray(C.byref(cf), u, v, o.ctypes.data, d.ctypes.data)
    return o, d


def math_batch(op, a, b=None):
    """po_math_batch: operation `op` (ptmi.Renderer.MATH_* numbers) of the host build of include/ptmi_math.h on the float32 cases
    (a[i], b[i]).  Returns (n, 2) float64, as Renderer.debug_math does for the device build."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1); n = len(a)
    b = np.zeros(n, np.float32) if b is None else np.ascontiguousarray(b, np.float32).reshape(n)
    out = np.zeros((n, 2), np.float64)
    oracle_lib().po_math_batch(int(op), n, a.ctypes.data, b.ctypes.data, out.ctypes.data)
    return out


def oracle_cdf_records(pdfs):
    """po_cdf_records: the (n, 530) PrecomputedCDF records of (n, 256) pdf values."""
    pdfs = np.ascontiguousarray(pdfs, np.float32); assert pdfs.ndim == 2 and pdfs.shape[1] == 256
    out = np.zeros((len(pdfs), 530), np.float32)
    assert oracle_lib().po_cdf_records(len(pdfs), pdfs.ctypes.data, out.ctypes.data) == 0
    return out


def oracle_filter_pdfs(rgb, counts, use_bilateral, sigma_spatial, sigma_range):
    """po_filter_pdfs: (formfactor, radiosity) pdfs of rgb (n, 256, 3) and counts (n, 256) or None."""
    rgb = np.ascontiguousarray(rgb, np.float32); assert rgb.ndim == 3 and rgb.shape[1:] == (256, 3)
    counts = None if counts is None else np.ascontiguousarray(counts, np.float32)
    ff = np.zeros(rgb.shape[:2], np.float32); rad = np.zeros(rgb.shape[:2], np.float32)
    assert oracle_lib().po_filter_pdfs(len(rgb), rgb.ctypes.data, None if counts is None else counts.ctypes.data, int(use_bilateral),
                                       sigma_spatial, sigma_range, ff.ctypes.data, rad.ctypes.data) == 0
    return ff, rad


def oracle_radiosity_grid(centre, normal, form_factors, radiosity, enable_filtering=False, use_bilateral=True, sigma_spatial=1.5,
                          sigma_range=0.3):
    """po_radiosity_grid_update: the (n, 256, 3) grids of a world given by centres, normals, form factors and radiosity."""
    centre, normal, radiosity, form_factors = (np.ascontiguousarray(a, np.float32) for a in (centre, normal, radiosity, form_factors))
    n = len(centre); assert form_factors.shape == (n, n)
    out = np.zeros((n, 256, 3), np.float32)
    assert oracle_lib().po_radiosity_grid_update(n, centre.ctypes.data, normal.ctypes.data, form_factors.ctypes.data, radiosity.ctypes.data,
                                                 int(enable_filtering), int(use_bilateral), sigma_spatial, sigma_range, out.ctypes.data) == 0
    return out


def rng_stream(seed, subsequence, n):
    st = np.zeros(6, np.uint32)
    L = oracle_lib()
    L.po_rng_init(seed, subsequence, st.ctypes.data)
    return np.array([L.po_rng_uniform(st.ctypes.data) for _ in range(n)], np.float32), st


# ---------------------------------------------------------------------------
_ref = None


def ref_available():
    return os.path.exists(REF_SO)


def ref_lib():
    global _ref
    if _ref is None:
        L = C.CDLL(REF_SO)
        L.ref_camera.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                 C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.ref_camera_ray.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        L.ref_scene_create.restype = C.c_void_p
        L.ref_scene_create.argtypes = [C.c_int] + [C.c_void_p] * 5
        L.ref_scene_free.argtypes = [C.c_void_p]
        L.ref_scene_num_nodes.argtypes = [C.c_void_p]
        L.ref_scene_get_bvh.argtypes = [C.c_void_p] * 7
        L.ref_tri_geometric_normal.argtypes = [C.c_void_p] * 4
        L.ref_quad_geometric_normal.argtypes = [C.c_void_p] * 5
        L.ref_centroid.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.ref_unit_vector.argtypes = [C.c_void_p, C.c_void_p]
        L.ref_area.restype = C.c_float
        L.ref_area.argtypes = [C.c_void_p, C.c_int]
        L.ref_sample_uniform.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p]
        L.ref_intersect.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                    C.c_int, C.c_void_p]
        L.ref_layout.argtypes = [C.c_void_p]; L.ref_layout.restype = None
        L.ref_grid_constants.argtypes = [C.c_void_p]; L.ref_grid_constants.restype = None
        _ref = L
    return _ref


class RefScene:
    """The reference's own Primitive[] + BVHBuilder + Scene, fed from arrays."""

    def __init__(self, types, verts, normal, bsdf, Le):
        self.L = ref_lib()
        types = np.ascontiguousarray(types, np.int32)
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 4, 3)
        normal, bsdf, Le = (np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (normal, bsdf, Le))
        self.n = len(types)
        self.h = self.L.ref_scene_create(self.n, types.ctypes.data, verts.ctypes.data, normal.ctypes.data,
                                         bsdf.ctypes.data, Le.ctypes.data)

    def __del__(self):
        try:
            self.L.ref_scene_free(self.h)
        except Exception:
            pass

    def bvh(self):
        n = self.L.ref_scene_num_nodes(self.h)
        bmin = np.zeros((n, 3), np.float32); bmax = np.zeros((n, 3), np.float32)
        left = np.zeros(n, np.int32); right = np.zeros(n, np.int32); count = np.zeros(n, np.int32)
        idx = np.zeros(self.n, np.int32)
        self.L.ref_scene_get_bvh(self.h, bmin.ctypes.data, bmax.ctypes.data, left.ctypes.data, right.ctypes.data,
                                 count.ctypes.data, idx.ctypes.data)
        return dict(bmin=bmin, bmax=bmax, left=left, right=right, count=count, indices=idx)

    def intersect(self, o, d, t_min=1e-4, t_max=3.4028234663852886e38, use_bvh=True):
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3); d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        out = (RefHit * len(o))()
        self.L.ref_intersect(self.h, len(o), o.ctypes.data, d.ctypes.data, t_min, t_max, int(use_bvh), out)
        return out


def ref_camera(cam, width, height):
    out = np.zeros(12, np.float32)
    lf = np.array(list(cam.origin), np.float32); la = np.array(list(cam.lookat), np.float32)
    up = np.array(list(cam.vup), np.float32)
    ref_lib().ref_camera(lf.ctypes.data, la.ctypes.data, up.ctypes.data, cam.vfov_deg, cam.yaw_deg, cam.pitch_deg,
                         cam.orbit, width, height, out.ctypes.data)
    return out


# ---- the reference's PBRT import, compiled (oracle/_ref/libptmi_ref_pbrt.so) -------------------------------------------------
REF_PBRT_SO = os.path.join(os.path.dirname(REF_SO), "libptmi_ref_pbrt.so")
_ref_pbrt = None


def ref_pbrt_available():
    return os.path.exists(REF_PBRT_SO)


def ref_pbrt_load(path):
    """loadPBRT of the reference on `path`: dict(type, verts, normal, bsdf, Le) or None where it fails (returns false / throws)."""
    global _ref_pbrt
    if _ref_pbrt is None:
        L = C.CDLL(REF_PBRT_SO)
        L.ref_pbrt_load.restype = C.c_void_p; L.ref_pbrt_load.argtypes = [C.c_char_p, C.c_int]
        L.ref_pbrt_count.argtypes = [C.c_void_p]; L.ref_pbrt_get.argtypes = [C.c_void_p] * 6; L.ref_pbrt_free.argtypes = [C.c_void_p]
        _ref_pbrt = L
    L = _ref_pbrt
    h = L.ref_pbrt_load(os.fsencode(os.path.abspath(path)), 1)
    if not h:
        return None
    n = L.ref_pbrt_count(h)
    t = np.zeros(n, np.int32); v = np.zeros((n, 4, 3), np.float32)
    nr = np.zeros((n, 3), np.float32); b = np.zeros((n, 3), np.float32); le = np.zeros((n, 3), np.float32)
    L.ref_pbrt_get(h, t.ctypes.data, v.ctypes.data, nr.ctypes.data, b.ctypes.data, le.ctypes.data)
    L.ref_pbrt_free(h)
    return dict(type=t, verts=v, normal=nr, bsdf=b, Le=le)


# ---- the reference's OBJ/MTL loader, compiled (oracle/_ref/libptmi_ref_obj.so; needs NVIDIA's own cuda_runtime.h at build time) ----
REF_OBJ_SO = os.path.join(os.path.dirname(REF_SO), "libptmi_ref_obj.so")
_ref_obj = None


def ref_obj_available():
    return os.path.exists(REF_OBJ_SO)


def ref_obj_load(path):
    """loadOBJ (+ loadMTL) of the reference on `path`: dict(type, verts, normal, bsdf, Le, warnings) or None where it returns false."""
    global _ref_obj
    if _ref_obj is None:
        L = C.CDLL(REF_OBJ_SO)
        L.ref_obj_load.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
        L.ref_obj_warning_count.argtypes = [C.c_void_p]
        L.ref_obj_get.argtypes = [C.c_void_p] * 6; L.ref_obj_free.argtypes = [C.c_void_p]; L.ref_obj_free.restype = None
        _ref_obj = L
    L = _ref_obj
    n = C.c_int(); h = C.c_void_p()
    ok = L.ref_obj_load(os.fsencode(path), C.byref(n), C.byref(h))
    out = None
    if ok:
        t = np.zeros(n.value, np.int32); v = np.zeros((n.value, 4, 3), np.float32)
        nr = np.zeros((n.value, 3), np.float32); b = np.zeros((n.value, 3), np.float32); le = np.zeros((n.value, 3), np.float32)
        if n.value:
            L.ref_obj_get(h, t.ctypes.data, v.ctypes.data, nr.ctypes.data, b.ctypes.data, le.ctypes.data)
        out = dict(type=t, verts=v, normal=nr, bsdf=b, Le=le, warnings=L.ref_obj_warning_count(h))
    L.ref_obj_free(h)
    return out


# ---- the compiled reference's answers, live or recorded ---------------------------------------------------------------------
RECORD_REF_ENV = "PTMI_RECORD_REF_ANSWERS"      # set by tests/golden/make_golden.py --ref-only: the fixture writes its golden file


def sha(a):
    """SHA-256 of an array's bytes (bit-exact equality for answers too bulky to record whole)."""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


class RefAnswers:
    """ref(key, ask): the compiled reference's answer, a dict of arrays.  ask() queries the live library; it is only called where
    that library exists (`live` and `available`), and then its answer must also be the recorded one, bit for bit.  Everywhere
    else the recorded answer is returned."""

    def __init__(self, golden, live, recorded, record):
        self.golden, self.live, self.recorded, self.record, self.fresh = golden, live, recorded, record, {}

    def __call__(self, key, ask, available=True):
        if self.live and available:
            got = {k: np.ascontiguousarray(v) for k, v in ask().items()}
            for k, v in got.items():
                self.fresh[f"{key}/{k}"] = v
                if not self.record:
                    want = self.recorded.get(f"{key}/{k}")
                    assert want is not None, f"{key}/{k} is not in {self.golden}: re-record it"
                    assert want.dtype == v.dtype and want.shape == v.shape and want.tobytes() == v.tobytes(), \
                        f"the compiled reference no longer answers {key}/{k} as recorded in {self.golden}"
            return got
        pre = f"{key}/"
        got = {k[len(pre):]: v for k, v in self.recorded.items() if k.startswith(pre)}
        assert got, f"{key} is not recorded in {self.golden}"
        return got


def recorded_reference(golden, live):
    """Body of a module-scoped fixture: yields the RefAnswers of `golden` (an .npz); in record mode (RECORD_REF_ENV set, the
    live library required) writes what was asked into `golden` when the module is done."""
    record = bool(os.environ.get(RECORD_REF_ENV))
    if record and not live:
        raise RuntimeError(f"{RECORD_REF_ENV} is set but the compiled reference is not built")
    r = RefAnswers(golden, live, {} if record else dict(np.load(golden)), record)
    yield r
    if record:
        np.savez_compressed(golden, **r.fresh)


# ---- the reference's integrator.h + grid.h, compiled (oracle/_ref/libptmi_ref_integrator.so; oracle/ref_integrator_harness.cpp) ----
REF_INT_SO = os.path.join(os.path.dirname(REF_SO), "libptmi_ref_integrator.so")
_ref_int = None


def ref_int_available():
    return os.path.exists(REF_INT_SO)


def ref_int_lib():
    global _ref_int
    if _ref_int is None:
        L = C.CDLL(REF_INT_SO)
        vp, f, i = C.c_void_p, C.c_float, C.c_int
        L.ref_sample_cosine_hemisphere.argtypes = [vp, vp, i, vp]
        L.ref_mis_power_heuristic.restype = f; L.ref_mis_power_heuristic.argtypes = [f, f]
        L.ref_grid_sample.argtypes = [vp, vp, vp, i, vp, vp, vp]
        L.ref_grid_pdf.restype = f; L.ref_grid_pdf.argtypes = [vp, vp, vp]
        L.ref_sample_mis.argtypes = [vp, vp, f, vp, i, vp, vp, vp]
        L.ref_int_scene_create.restype = vp; L.ref_int_scene_create.argtypes = [i] + [vp] * 8 + [f]
        L.ref_int_scene_free.argtypes = [vp]; L.ref_int_scene_free.restype = None
        L.ref_render.argtypes = [vp, vp, i, i, i, i, i, vp]
        L.ref_render_radiosity.argtypes = [vp, vp, i, i, i, i, vp]
        L.ref_radiance.argtypes = [vp, vp, i, i, i, i, i, i, vp]
        if hasattr(L, "ref_grid_record"):
            L.ref_grid_record.argtypes = [i, vp, vp]
        _ref_int = L
    return _ref_int


def _camera13(cam):
    return np.array(list(cam.origin) + list(cam.lookat) + list(cam.vup) + [cam.vfov_deg, cam.yaw_deg, cam.pitch_deg, float(cam.orbit)],
                    np.float32)


def _opt(a, dtype=np.float32):
    return None if a is None else np.ascontiguousarray(a, dtype)


class RefIntegratorScene:
    """The reference's Scene (BVHBuilder) with precomputed_cdfs = `cdfs` (n x 530 words, the oracle's records) or, without
    them, the primitives' raw radiosity grids (initFromRadiosity); per-primitive radiosity for render_radiosity."""

    def __init__(self, types, verts, normal, bsdf, Le, radiosity=None, cdfs=None, rad_grids=None, mis_fraction=0.5):
        self.L = ref_int_lib()
        self.keep = [np.ascontiguousarray(types, np.int32)] + [np.ascontiguousarray(a, np.float32) for a in (verts, normal, bsdf, Le)] + \
                    [_opt(radiosity), _opt(cdfs), _opt(rad_grids)]
        ptrs = [None if a is None else a.ctypes.data for a in self.keep]
        self.h = self.L.ref_int_scene_create(len(self.keep[0]), *ptrs, float(mis_fraction))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.ref_int_scene_free(self.h)
            self.h = None

    def render(self, cam, width, height, spp, mode=0, n_threads=0):
        rgb = np.zeros((height, width, 3), np.uint8)
        self.L.ref_render(self.h, _camera13(cam).ctypes.data, width, height, spp, int(mode), n_threads, rgb.ctypes.data)
        return rgb

    def render_radiosity(self, cam, width, height, spp, n_threads=0):
        rgb = np.zeros((height, width, 3), np.uint8)
        self.L.ref_render_radiosity(self.h, _camera13(cam).ctypes.data, width, height, spp, n_threads, rgb.ctypes.data)
        return rgb

    def radiance(self, cam, width, height, spp, max_depth=5, mode=0, n_threads=0):
        rad = np.zeros((height, width, 3), np.float32)
        self.L.ref_radiance(self.h, _camera13(cam).ctypes.data, width, height, spp, max_depth, int(mode), n_threads, rad.ctypes.data)
        return rad


# ---- the reference's form_factors.h + grid_filter.h, compiled (oracle/_ref/libptmi_ref_solver.so; oracle/ref_solver_harness.cpp) ----
REF_SOL_SO = os.path.join(os.path.dirname(REF_SO), "libptmi_ref_solver.so")
_ref_sol = None


def ref_sol_available():
    return os.path.exists(REF_SOL_SO)


def ref_sol_lib():
    global _ref_sol
    if _ref_sol is None:
        L = C.CDLL(REF_SOL_SO)
        vp, f, i = C.c_void_p, C.c_float, C.c_int
        L.ref_sol_scene_create.restype = vp; L.ref_sol_scene_create.argtypes = [i] + [vp] * 5
        L.ref_sol_scene_free.argtypes = [vp]; L.ref_sol_scene_free.restype = None
        L.ref_sol_scene_num_prims.argtypes = [vp]
        L.ref_sol_scene_get_prims.argtypes = [vp] * 6; L.ref_sol_scene_get_prims.restype = None
        L.ref_sol_grid_index.argtypes = [vp, vp]
        L.ref_sol_visibility.argtypes = [vp, i, i] + [vp] * 6; L.ref_sol_visibility.restype = None
        L.ref_sol_rand_init.argtypes = [i, i, vp, vp]; L.ref_sol_rand_init.restype = None
        L.ref_sol_ff_rows.argtypes = [vp, i, i, i, vp, vp, vp, vp]
        L.ref_sol_mc_pair.argtypes = [vp, i, i, i, vp, i, vp, vp, vp, vp]
        L.ref_sol_update_grid.argtypes = [vp] * 4; L.ref_sol_update_grid.restype = None
        L.ref_sol_iterate.argtypes = [vp] * 6; L.ref_sol_iterate.restype = None
        L.ref_sol_solve.argtypes = [vp, i, i, i, i, i, f, f] + [vp] * 5
        L.ref_sol_filter_grids.argtypes = [i, vp, i, f, f, vp]; L.ref_sol_filter_grids.restype = None
        L.ref_sol_filter_pdfs.argtypes = [i, vp, vp, i, f, f, vp, vp]; L.ref_sol_filter_pdfs.restype = None
        L.ref_sol_subdivide.restype = vp; L.ref_sol_subdivide.argtypes = [vp, i]
        _ref_sol = L
    return _ref_sol


def ref_sol_grid_index(dirs, normals):
    """direction_to_grid_indices_local per call: theta * 16 + phi of each (direction, normal) row."""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3); n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    L = ref_sol_lib()
    return np.array([L.ref_sol_grid_index(d[k].ctypes.data, n[k].ctypes.data) for k in range(len(d))], np.int32)


def ref_sol_rand_init(num_pairs, idx):
    idx = np.ascontiguousarray(idx, np.int32); out = np.zeros((len(idx), 6), np.uint32)
    ref_sol_lib().ref_sol_rand_init(int(num_pairs), len(idx), idx.ctypes.data, out.ctypes.data)
    return out


def ref_sol_filter_grids(rgb, use_bilateral, sigma_spatial, sigma_range):
    rgb = np.ascontiguousarray(rgb, np.float32); assert rgb.ndim == 3 and rgb.shape[1:] == (256, 3)
    out = np.zeros_like(rgb)
    ref_sol_lib().ref_sol_filter_grids(len(rgb), rgb.ctypes.data, int(use_bilateral), sigma_spatial, sigma_range, out.ctypes.data)
    return out


def ref_sol_filter_pdfs(rgb, counts, use_bilateral, sigma_spatial, sigma_range):
    rgb = np.ascontiguousarray(rgb, np.float32); assert rgb.ndim == 3 and rgb.shape[1:] == (256, 3)
    counts = None if counts is None else np.ascontiguousarray(counts, np.float32)
    ff = np.zeros(rgb.shape[:2], np.float32); rad = np.zeros(rgb.shape[:2], np.float32)
    ref_sol_lib().ref_sol_filter_pdfs(len(rgb), rgb.ctypes.data, None if counts is None else counts.ctypes.data, int(use_bilateral),
                                      sigma_spatial, sigma_range, ff.ctypes.data, rad.ctypes.data)
    return ff, rad


class RefSolverScene:
    """The reference's Primitive[] + BVHBuilder tree, fed from arrays, under the reference's own solver kernels."""

    def __init__(self, types=None, verts=None, normal=None, bsdf=None, Le=None, handle=None):
        self.L = ref_sol_lib()
        if handle is not None:
            self.h = handle; return
        types = np.ascontiguousarray(types, np.int32)
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 4, 3)
        normal, bsdf, Le = (np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (normal, bsdf, Le))
        self.h = self.L.ref_sol_scene_create(len(types), types.ctypes.data, verts.ctypes.data, normal.ctypes.data, bsdf.ctypes.data,
                                             Le.ctypes.data)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.ref_sol_scene_free(self.h)
            self.h = None

    @property
    def n(self):
        return self.L.ref_sol_scene_num_prims(self.h)

    def prims(self):
        n = self.n
        t = np.zeros(n, np.int32); v = np.zeros((n, 4, 3), np.float32)
        nr = np.zeros((n, 3), np.float32); b = np.zeros((n, 3), np.float32); le = np.zeros((n, 3), np.float32)
        self.L.ref_sol_scene_get_prims(self.h, t.ctypes.data, v.ctypes.data, nr.ctypes.data, b.ctypes.data, le.ctypes.data)
        return dict(type=t, verts=v, normal=nr, bsdf=b, Le=le)

    def visibility(self, o, d, max_dist, source, target, use_bvh=True):
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3); d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        m = len(o)
        md = np.ascontiguousarray(np.broadcast_to(np.asarray(max_dist, np.float32), (m,)))
        src = np.ascontiguousarray(np.broadcast_to(np.asarray(source, np.int32), (m,)))
        tgt = np.ascontiguousarray(np.broadcast_to(np.asarray(target, np.int32), (m,)))
        out = np.zeros(m, np.int32)
        self.L.ref_sol_visibility(self.h, int(use_bvh), m, o.ctypes.data, d.ctypes.data, md.ctypes.data, src.ctypes.data, tgt.ctypes.data,
                                  out.ctypes.data)
        return out

    def ff_rows(self, rows, use_monte_carlo=True, mc_samples=64):
        rows = np.ascontiguousarray(rows, np.int32); n = self.n
        ff = np.zeros((len(rows), n), np.float32); grid = np.zeros((len(rows), 256), np.float32); rg = np.zeros((len(rows), 256, 3), np.float32)
        rc = self.L.ref_sol_ff_rows(self.h, int(use_monte_carlo), int(mc_samples), len(rows), rows.ctypes.data, ff.ctypes.data,
                                    grid.ctypes.data, rg.ctypes.data)
        assert rc == 0
        return ff, grid, rg

    def mc_pair_words(self, i, j, n_samples, words):
        w = np.ascontiguousarray(words, np.uint32)
        F = C.c_float(); over = C.c_int(); grid = np.zeros(256, np.float32); rg = np.zeros((256, 3), np.float32)
        used = self.L.ref_sol_mc_pair(self.h, int(i), int(j), int(n_samples), w.ctypes.data, len(w), C.addressof(F), grid.ctypes.data,
                                      rg.ctypes.data, C.addressof(over))
        return dict(F=np.float32(F.value), grid=grid, rad_grid=rg, used=np.int32(used), overrun=np.int32(over.value))

    def update_grid(self, form_factors, radiosity):
        n = self.n
        ff = np.ascontiguousarray(form_factors, np.float32); rad = np.ascontiguousarray(radiosity, np.float32)
        assert ff.shape == (n, n) and rad.shape == (n, 3)
        out = np.zeros((n, 256, 3), np.float32)
        self.L.ref_sol_update_grid(self.h, ff.ctypes.data, rad.ctypes.data, out.ctypes.data)
        return out

    def iterate(self, form_factors, radiosity, unshot):
        n = self.n
        ff, rad, un = (np.ascontiguousarray(a, np.float32) for a in (form_factors, radiosity, unshot))
        assert ff.shape == (n, n) and rad.shape == (n, 3) and un.shape == (n, 3)
        o_rad = np.zeros((n, 3), np.float32); o_un = np.zeros((n, 3), np.float32)
        self.L.ref_sol_iterate(self.h, ff.ctypes.data, rad.ctypes.data, un.ctypes.data, o_rad.ctypes.data, o_un.ctypes.data)
        return o_rad, o_un

    def solve(self, **params):
        p = RadiosityParams(**params); n = self.n
        out = dict(form_factors=np.zeros((n, n), np.float32), radiosity=np.zeros((n, 3), np.float32), unshot=np.zeros((n, 3), np.float32),
                   grid=np.zeros((n, 256), np.float32), radiosity_grid=np.zeros((n, 256, 3), np.float32))
        rc = self.L.ref_sol_solve(self.h, p.num_iterations, p.mc_samples, p.use_monte_carlo, p.enable_filtering, p.use_bilateral,
                                  p.filter_sigma_spatial, p.filter_sigma_range, *(out[k].ctypes.data for k in
                                  ("form_factors", "radiosity", "unshot", "grid", "radiosity_grid")))
        assert rc == 0
        return out

    def subdivide(self, levels):
        return RefSolverScene(handle=self.L.ref_sol_subdivide(self.h, int(levels)))
