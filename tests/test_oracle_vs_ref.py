"""oracle/ptmi_oracle.c against the REFERENCE's own geometry headers compiled into oracle/_ref/libptmi_ref.so
(oracle/Makefile, only where the reference tree exists).  Bit-exact: BVHBuilder output, Scene::intersect (BVH and linear),
Sensor, unit_vector, constructor normals.

Every answer of the compiled reference these tests use is recorded in tests/golden/ref_geometry.npz.  Where oracle/_ref is
built, the tests ask it live and also require the recorded answer to be the same bits; everywhere else they compare the
oracle against the recorded answers.  Re-record (where oracle/_ref is built):  python tests/golden/make_golden.py --ref-only
"""
import ctypes
import os

import numpy as np
import pytest

from oracle_binding import (OracleScene, RefHit, RefScene, SCENES, Camera, camera_frame, camera_ray, default_camera,
                            recorded_reference, ref_available, ref_camera, ref_lib, ref_obj_available, ref_obj_load, sha)

F = np.float32
C_HIT_SIZE = ctypes.sizeof(RefHit)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_geometry.npz")


@pytest.fixture(scope="module")
def ref():
    yield from recorded_reference(GOLDEN, ref_available())


HIT = np.dtype([("hit", np.int32), ("prim", np.int32), ("t", F), ("p", F, 3), ("n", F, 3), ("bsdf", F, 3), ("Le", F, 3)])
assert HIT.itemsize == C_HIT_SIZE


def surface_rows(t, p, n, bsdf, Le):
    return np.concatenate([np.asarray(t, F).reshape(-1, 1)] + [np.asarray(a, F).reshape(-1, 3) for a in (p, n, bsdf, Le)], axis=1)


def hits(h):
    """RefScene.intersect's records: hit and prim per ray, and the digest of the hits' t / p / n / bsdf / Le in ray order."""
    a = np.frombuffer(bytes(h), HIT)
    on = a["hit"] != 0
    return dict(hit=np.array(a["hit"]), prim=np.array(a["prim"]), surface=sha(surface_rows(*(a[k][on] for k in ("t", "p", "n", "bsdf", "Le")))))


def bvh_digest(b):
    """The tree's arrays as digests (a leaf's `right` is not part of the tree)."""
    count = np.asarray(b["count"], np.int32)
    return dict(nodes=np.int64(len(count)), count=sha(count), right_inner=sha(np.asarray(b["right"], np.int32)[count == 0]),
                **{k: sha(np.asarray(b[k], np.int32)) for k in ("left", "indices")}, **{k: sha(np.asarray(b[k], F)) for k in ("bmin", "bmax")})


class LazyRef:
    """The reference's Scene over a pair's arrays, built on first use (only where oracle/_ref is built)."""

    def __init__(self, arrs):
        self.arrs, self.scene = arrs, None

    def __call__(self):
        if self.scene is None:
            self.scene = RefScene(*self.arrs)
        return self.scene


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def random_soup(rng, n, quad_frac=0.3, scale=4.0):
    types = (rng.random(n) < quad_frac).astype(np.int32)
    centers = rng.uniform(-scale, scale, (n, 1, 3))
    verts = (centers + rng.normal(0, 0.35, (n, 4, 3))).astype(F)
    # make quads planar-ish parallelograms: v01 = v00 + (v11 - v10)
    q = types == 1
    verts[q, 2] = verts[q, 1] + (verts[q, 3] - verts[q, 0])
    normal = rng.normal(0, 1, (n, 3)); normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    bsdf = rng.uniform(0, 1, (n, 3)); Le = rng.uniform(0, 2, (n, 3)) * (rng.random((n, 1)) < 0.1)
    return types, verts, normal.astype(F), bsdf.astype(F), Le.astype(F)


def scene_pairs():
    out = []
    for name, kw in [("cbox.obj", {}), ("cbox_quads.obj", {}), ("cbox_quads.obj", dict(convert_quads=True)),
                     ("cbox.obj", dict(subdivision=2)), ("cbox_quads.obj", dict(subdivision=1)),
                     ("cbox_quads.obj", dict(subdivision=2, convert_quads=True))]:
        o = OracleScene.load(SCENES + "/" + name, **kw)
        p = o.prims()
        out.append((f"{name}{kw}", o, LazyRef((p["type"], p["verts"], p["normal"], p["bsdf"], p["Le"]))))
    rng = np.random.default_rng(7)
    for n in (1, 3, 5, 64, 1500):
        arrs = random_soup(rng, n)
        out.append((f"soup{n}", OracleScene.from_arrays(*arrs), LazyRef(arrs)))
    # degenerate: many coincident centroids -> "extent < 1e-6" leaf with count > 4, and the
    # empty-partition fallback (bvh.h:185-189, 203-206)
    t = np.zeros(9, np.int32); v = np.tile(rng.normal(0, 1, (1, 4, 3)).astype(F), (9, 1, 1))
    nr = np.tile(np.array([[0, 0, 1]], F), (9, 1)); b = np.full((9, 3), 0.5, F); le = np.zeros((9, 3), F)
    out.append(("coincident9", OracleScene.from_arrays(t, v, nr, b, le), LazyRef((t, v, nr, b, le))))
    return out


@pytest.fixture(scope="module")
def pairs():
    return scene_pairs()


def test_bvh_builder_bit_exact(pairs, ref):
    for name, o, r in pairs:
        bo, br = o.bvh(), ref(f"bvh/{name}", lambda: r().bvh())
        assert len(bo["left"]) == len(br["left"]), name
        for k in ("left", "count", "indices"):
            assert (bo[k] == br[k]).all(), (name, k)
        inner = bo["count"] == 0
        assert (bo["right"][inner] == br["right"][inner]).all(), name
        assert (bits(bo["bmin"]) == bits(br["bmin"])).all() and (bits(bo["bmax"]) == bits(br["bmax"])).all(), name


def _rays_for(o, rng, n):
    """Mix of camera rays, random rays, axis-parallel rays (inv_dir = +-inf), rays starting on
    surfaces (t_min edge) and rays aimed at shared edges/vertices (tie cases)."""
    p = o.prims()
    cf = camera_frame(default_camera(), 64, 64)
    os_, ds = [], []
    for _ in range(n // 4):
        a, b = camera_ray(cf, F(rng.random()), F(rng.random())); os_.append(a); ds.append(b)
    lo = p["verts"].reshape(-1, 3).min(0) - 1; hi = p["verts"].reshape(-1, 3).max(0) + 1
    for _ in range(n // 4):
        os_.append(rng.uniform(lo, hi).astype(F)); d = rng.normal(0, 1, 3); ds.append((d / np.linalg.norm(d)).astype(F))
    for _ in range(n // 8):
        os_.append(rng.uniform(lo, hi).astype(F)); d = np.zeros(3, F); d[rng.integers(3)] = rng.choice([-1.0, 1.0]); ds.append(d)
    for _ in range(n // 8):  # -0.0 components
        os_.append(rng.uniform(lo, hi).astype(F)); d = np.array([-0.0, -0.0, -0.0], F); d[rng.integers(3)] = rng.choice([-1.0, 1.0]); ds.append(d)
    nprim = len(p["type"])
    for _ in range(n // 4):  # from a random point toward a vertex / edge midpoint of a random primitive
        i = rng.integers(nprim); nv = 3 if p["type"][i] == 0 else 4
        a = p["verts"][i, rng.integers(nv)]; b = p["verts"][i, rng.integers(nv)]
        target = (a + b) * F(0.5) if rng.random() < 0.5 else a
        org = rng.uniform(lo, hi).astype(F); d = (target - org).astype(np.float64); d /= max(np.linalg.norm(d), 1e-12)
        os_.append(org); ds.append(d.astype(F))
    return np.array(os_, F), np.array(ds, F)


def test_scene_intersect_bit_exact(pairs, ref):
    rng = np.random.default_rng(11)
    total = hits_ = 0
    for name, o, r in pairs:
        O, D = _rays_for(o, rng, 400)
        for use_bvh in (True, False):
            for (t_min, t_max) in ((1e-4, np.finfo(F).max), (0.5, 6.0)):
                rh = ref(f"intersect/{name}/{use_bvh}/{t_min}", lambda: hits(r().intersect(O, D, t_min, t_max, use_bvh)))
                rows = []
                for i in range(len(O)):
                    oh = o.intersect(O[i], D[i], t_min, t_max, use_bvh)
                    assert oh.hit == rh["hit"][i] and oh.prim == rh["prim"][i], (name, i, use_bvh)
                    total += 1
                    if oh.hit:
                        hits_ += 1
                        rows.append(surface_rows(oh.t, list(oh.p), list(oh.n), list(oh.bsdf), list(oh.Le)))
                # t, p, n, bsdf, Le of every hit, bit for bit
                assert (sha(np.concatenate(rows) if rows else surface_rows(*[np.zeros(0, F)] * 5)) == rh["surface"]).all(), (name, use_bvh, t_min)
    assert hits_ > total // 5


def test_sensor_bit_exact(ref):
    cams = [default_camera(),
            Camera((0.5, 3.0, 8.5), (0, 2.5, 0), (0, 1, 0), 40.0, 37.5, -12.25, 1),
            Camera((0.5, 3.0, 8.5), (0, 2.5, 0), (0, 1, 0), 55.0, 123.0, 20.0, 1),
            Camera((1.0, 2.0, 7.0), (0.2, 2.5, -1), (0, 1, 0), 30.0, 90.0, 0.0, 0),
            Camera((-2.0, 4.0, 3.0), (0, 2.5, -3), (0.1, 1, 0), 70.0, 200.0, -45.0, 1)]
    for c, cam in enumerate(cams):
        for (w, h) in ((1024, 1024), (1920, 1080), (200, 333)):
            rng = np.random.default_rng(3)
            uv = np.array([(F(rng.random()), F(rng.random())) for _ in range(50)], F)

            def ask():
                frame = ref_camera(cam, w, h)
                ro = np.zeros((len(uv), 3), F); rd = np.zeros((len(uv), 3), F)
                for j, (u, v) in enumerate(uv):
                    ref_lib().ref_camera_ray(frame.ctypes.data, u, v, ro[j].ctypes.data, rd[j].ctypes.data)
                return dict(frame=frame, o=ro, d=rd)

            want = ref(f"sensor/{c}/{w}x{h}", ask)
            mine = camera_frame(cam, w, h).as_array()
            assert (bits(mine) == bits(want["frame"])).all(), (list(cam.origin), w, h, mine, want["frame"])
            cf = camera_frame(cam, w, h)
            for j, (u, v) in enumerate(uv):
                o, d = camera_ray(cf, u, v)
                assert (bits(o) == bits(want["o"][j])).all() and (bits(d) == bits(want["d"][j])).all()


def test_constructor_normals_bit_exact(ref):
    """Triangle 4-arg / Quad constructors (triangle.h:23-31, quad.h:23-31) drive convert_quads and
    subdivision normals; compare through a converted + subdivided load."""
    o = OracleScene.load(SCENES + "/cbox_quads.obj", subdivision=1, convert_quads=True)
    p = o.prims()
    assert len(p["type"]) == 16 * 2 * 4 and (p["type"] == 0).all()

    def ask_tri():
        out = np.zeros((len(p["type"]), 3), F)
        for i, v in enumerate(p["verts"]):
            ref_lib().ref_tri_geometric_normal(v[0].ctypes.data, v[1].ctypes.data, v[2].ctypes.data, out[i].ctypes.data)
        return dict(normal=out)
    want = ref("normals/tri", ask_tri)["normal"]
    for i in range(len(p["type"])):
        assert (bits(want[i]) == bits(p["normal"][i])).all(), i
    o = OracleScene.load(SCENES + "/cbox_quads.obj", subdivision=2)
    p = o.prims()
    assert len(p["type"]) == 16 * 16 and (p["type"] == 1).all()

    def ask_quad():
        out = np.zeros((len(p["type"]), 3), F)
        for i in range(len(p["type"])):
            v = np.ascontiguousarray(p["verts"][i])
            ref_lib().ref_quad_geometric_normal(v[0].ctypes.data, v[1].ctypes.data, v[2].ctypes.data, v[3].ctypes.data, out[i].ctypes.data)
        return dict(normal=out)
    want = ref("normals/quad", ask_quad)["normal"]
    for i in range(len(p["type"])):
        assert (bits(want[i]) == bits(p["normal"][i])).all(), i


def test_large_tessellated_scene_bvh_and_intersect(ref):
    """65,536 displaced triangles (the 1 M-triangle stress scene at 1/16 density): the reference's BVHBuilder and
    Scene::intersect on its 4364-byte Primitive records vs the oracle, bit for bit."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda-pathtracer_amd", "python"))
    import ptmi_scenes
    base = OracleScene.load(SCENES + "/cbox_quads.obj").prims()
    sc = ptmi_scenes.tessellated_cornell(base, 64, 32, seed=1)
    assert len(sc["type"]) == 65536
    args = (sc["type"], sc["verts"], sc["normal"], sc["bsdf"], sc["Le"])
    o = OracleScene.from_arrays(*args); r = LazyRef(args)
    bo, br = bvh_digest(o.bvh()), ref("tess64k/bvh", lambda: bvh_digest(r().bvh()))
    assert bo["nodes"] == br["nodes"]
    for k in ("left", "count", "indices", "right_inner", "bmin", "bmax"):
        assert (bo[k] == br[k]).all(), k
    O, D = _rays_for(o, np.random.default_rng(21), 1200)
    rh = ref("tess64k/intersect", lambda: hits(r().intersect(O, D)))
    hits_ = 0; rows = []
    for i in range(len(O)):
        oh = o.intersect(O[i], D[i])
        assert oh.hit == rh["hit"][i] and oh.prim == rh["prim"][i], i
        if oh.hit:
            hits_ += 1
            rows.append(surface_rows(oh.t, list(oh.p), list(oh.n), list(oh.bsdf), list(oh.Le)))
    assert hits_ > 300
    assert (sha(np.concatenate(rows)) == rh["surface"]).all()           # t, p, n, bsdf, Le of every hit, bit for bit


def test_radiosity_prepass_primitive_helpers_bit_exact(pairs, ref):
    """The pieces of the radiosity pre-pass that live in primitive.h - getArea (as the constructors
    computed it), centroid, sampleUniform (triangle barycentric / quad split by area ratio) - against the compiled
    reference.  form_factors.h itself needs <cuda_runtime.h> and is restated only."""
    rng = np.random.default_rng(21)
    for name, o, r in pairs:
        n = o.n_prims
        prims = [int(i) for i in (range(n) if n <= 64 else rng.integers(0, n, 64))]
        us = rng.random((len(prims), 12, 2)).astype(F)
        us[:, 0] = [1.0, 1.0]; us[:, 1] = [2.3283064e-10 / 2, 0.5]; us[:, 2] = [0.5, 1.0]      # curand_uniform's range is (0, 1]

        def ask():
            L = ref_lib()
            area = np.array([L.ref_area(r().h, i) for i in prims], F)
            cen = np.zeros((len(prims), 3), F); smp = np.zeros((len(prims), 12, 3), F)
            for j, i in enumerate(prims):
                L.ref_centroid(r().h, i, cen[j].ctypes.data)
                for k, (r1, r2) in enumerate(us[j]):
                    L.ref_sample_uniform(r().h, i, float(r1), float(r2), smp[j, k].ctypes.data)
            return dict(area=area, centroid=cen, sample_uniform=smp)

        want = ref(f"prim_helpers/{name}", ask)
        for j, i in enumerate(prims):
            area, cen = o.prim_geometry(i)
            assert bits(area) == bits(want["area"][j]), (name, i)
            assert (bits(cen) == bits(want["centroid"][j])).all(), (name, i)
            for k, (r1, r2) in enumerate(us[j]):
                assert (bits(o.sample_uniform(i, r1, r2)) == bits(want["sample_uniform"][j, k])).all(), (name, i, r1, r2)


def test_render_config_layout_and_constants(ref):
    """rendering/render_config.h as the reference's own compiler pass sees it (it reaches ref_harness.cpp through
    triangle.h:7): sizeof / field offsets of PrecomputedCDF (:24-31), GRID_* (:7-9), the SamplingMode values (:38-44), the
    launch block (:51-52) and the grid-step macros (:14-17, doubles because M_PI is the double one) - against the oracle's
    restatement AND the product's record layout (ptmi_host_cdf_record_layout = csrc/device_scene.h kCdf*)."""
    from oracle_binding import oracle_lib
    import ptmi

    def ask():
        lay = np.zeros(22, np.int32); ref_lib().ref_layout(lay.ctypes.data)
        rc = np.zeros(6, np.float64); ref_lib().ref_grid_constants(rc.ctypes.data)
        return dict(layout=lay, grid_constants=rc)
    want = ref("render_config", ask)
    ref_ = want["layout"]
    assert ref_[:7].tolist() == [2120, 0, 1024, 1056, 1088, 2112, 2116]          # "PrecomputedCDF 2120 B"
    assert ref_[7:10].tolist() == [16, 256, 8]
    assert ref_[10:15].tolist() == [0, 1, 2, 3, 4]                                # ptmi_config.sampling_mode values
    assert ref_[15:17].tolist() == [16, 16]
    assert ref_[17:20].tolist() == [4364, 36, 96]                                 # Primitive, BVHNode, SurfaceInteractionRecord
    assert ref_[21] == 8                                                          # GRID_D_THETA is a double expression
    orc = np.zeros(10, np.int32); oracle_lib().po_cdf_layout(orc.ctypes.data)
    assert orc.tolist() == ref_[:10].tolist()
    assert ptmi.host_cdf_record_layout().tolist() == ref_[:10].tolist()
    rc = want["grid_constants"]
    oc = np.zeros(6, np.float64); oracle_lib().po_grid_constants(oc.ctypes.data)
    assert (rc.view(np.uint64) == oc.view(np.uint64)).all(), (rc, oc)
    assert rc[4] == np.pi                                                        # M_PI: the double constant, not math_utils.h's float


@pytest.mark.parametrize("name,n_tris,n_quads,warnings", [("cbox.obj", 32, 0, 0), ("cbox_quads.obj", 0, 16, 20)])
def test_obj_loader_against_the_compiled_reference_loader(ref, name, n_tris, n_quads, warnings):
    """loadOBJ + loadMTL of the reference itself (utils/file_manager.h:39-79, 93-273, compiled unmodified against
    NVIDIA's own cuda_runtime.h) on the two Cornell files: the oracle's C loader and the product's C++ loader return its
    primitives bit for bit - type, vertices, stored normal (first vn or geometric), Kd, Ke - incl. the 20 "malformed face
    vertex token" warnings of cbox_quads.obj:100-112 (trailing '# Top' comments), which must not change the result.
    (oracle/_ref/libptmi_ref_obj.so is built only where <cuda_runtime.h> is found as well: elsewhere the recorded answer.)"""
    import ptmi
    path = os.path.join(SCENES, name)

    def ask():
        got = ref_obj_load(path)
        assert got is not None
        return dict(got, warnings=np.int32(got["warnings"]))
    want = ref(f"obj/{name}", ask, available=ref_obj_available())
    assert ((want["type"] == 0).sum(), (want["type"] == 1).sum(), want["warnings"].item()) == (n_tris, n_quads, warnings)
    for got in (OracleScene.load(path).prims(), ptmi.HostScene.load(path).prims()):
        assert (got["type"] == want["type"]).all()
        tri = got["type"] == 0
        assert (bits(got["verts"][tri][:, :3]) == bits(want["verts"][tri][:, :3])).all() and (bits(got["verts"][~tri]) == bits(want["verts"][~tri])).all()
        for k in ("normal", "bsdf", "Le"):
            assert (bits(got[k]) == bits(want[k])).all(), k
