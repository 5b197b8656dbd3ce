"""Host half of the shaded features (include/ptmi.h, "shaded features"): ptmi_check_feature_shading, and the restatement
(tests/shaded_features_oracle.py) against the feature pass it extends (tests/denoise_oracle.py) where the two must agree bit for
bit, and on a checkered floor where they must not.  No GPU."""
import numpy as np
import pytest

import denoise_oracle as DO
import ptmi
import ptmi_scenes
import shaded_features_oracle as SF
import texture_cases as TC
import texture_oracle as TX
from oracle_binding import OracleScene, default_camera

F = np.float32
KEYS = ("albedo", "normal", "position", "hit_fraction")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    for k in KEYS:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def test_check_accepts_0_to_3_and_refuses_the_rest_with_a_message():
    L = ptmi.lib()
    for flags in range(4):
        assert L.ptmi_check_feature_shading(flags) == 0
        ptmi.check_feature_shading(flags)
    for flags in (-1, 4, 8):
        assert L.ptmi_check_feature_shading(flags) == -1
        assert b"flags must be in [0, 3]" in L.ptmi_last_error()
        with pytest.raises(ptmi.PtmiError, match="feature shading"):
            ptmi.check_feature_shading(flags)
    assert (ptmi.FEATURE_TEXTURED_ALBEDO, ptmi.FEATURE_SHADING_NORMAL) == (1, 2)


@pytest.fixture(scope="module")
def cbox():
    arrays, parts = TC.cornell("cbox")
    scene = OracleScene.from_arrays(*arrays)
    return arrays, parts, scene, DO.features(scene, default_camera(), 9, 7, 2)


def test_flags_0_and_flags_without_tables_are_the_plain_feature_pass(cbox):
    arrays, _, scene, plain = cbox
    n = len(arrays[0])
    table = TX.make_table(TC.image(), TC.random_uvs(n), None, "bilinear")
    same(SF.features(scene, default_camera(), 9, 7, 2), plain)
    tilted = np.asarray(arrays[2], np.float64)[:, None, :] + 0.5 * np.random.default_rng(11).normal(0, 1, (n, 4, 3))
    tilted = (tilted / np.linalg.norm(tilted, axis=2, keepdims=True)).astype(F)           # every primitive smooth
    same(SF.features(scene, default_camera(), 9, 7, 2, flags=0, texture=table, normals=tilted), plain)
    shaded = SF.features(scene, default_camera(), 9, 7, 2, flags=3, texture=table, normals=tilted)
    assert not np.array_equal(bits(shaded["albedo"]), bits(plain["albedo"]))      # and with the flags the tables do show
    assert not np.array_equal(bits(shaded["normal"]), bits(plain["normal"]))
    assert np.array_equal(bits(shaded["position"]), bits(plain["position"]))
    same(SF.features(scene, default_camera(), 9, 7, 2, flags=3), plain)           # no table a flag names
    with pytest.raises(ValueError):
        SF.features(scene, default_camera(), 9, 7, 2, flags=4)


@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_an_image_of_ones_and_the_stored_normals_at_every_corner_change_no_bit(cbox, filt):
    """T = 1 exactly under both filters, and a primitive whose corner normals equal its stored one is flat"""
    arrays, _, scene, plain = cbox
    n = len(arrays[0])
    table = TX.make_table(np.ones((3, 5, 3), F), TC.random_uvs(n), None, filt)
    normals = np.repeat(np.asarray(arrays[2], F)[:, None, :], 4, axis=1)
    same(SF.features(scene, default_camera(), 9, 7, 2, flags=3, texture=table, normals=normals), plain)


def test_a_checkered_floor_has_exactly_the_two_products():
    arrays, parts = TC.cornell("cbox")
    prims = TC.as_prims(arrays)
    scene = OracleScene.from_arrays(*arrays)
    n = len(arrays[0])
    w, h = 48, 40
    textured = np.zeros(n, bool); textured[parts["floor"]] = True
    a, b = F(0.9), F(0.2)
    table = TX.make_table(ptmi_scenes.checker(4, (a,) * 3, (b,) * 3), ptmi_scenes.box_uvs(prims, scale=2.0), textured, "nearest")
    plain = DO.features(scene, default_camera(), w, h, 1)
    got = SF.features(scene, default_camera(), w, h, 1, flags=1, texture=table)
    kd = np.asarray(arrays[3], F)[parts["floor"][0]]
    assert all(np.array_equal(bits(arrays[3][k]), bits(kd)) for k in parts["floor"])
    floor_normal = arrays[2][parts["floor"][0]]
    floor_y = arrays[1][parts["floor"], :3, 1]
    on = (bits(plain["normal"]) == bits(floor_normal)).all(2) & (plain["position"][..., 1] < floor_y.max() + 1e-3)
    assert on.sum() > 100 and (~on).sum() > 500
    values = {tuple(v) for v in bits(got["albedo"][on])}
    assert values == {tuple(bits((kd * a).astype(F))), tuple(bits((kd * b).astype(F)))}
    assert {tuple(v) for v in bits(plain["albedo"][on])} == {tuple(bits(kd))}
    assert np.array_equal(bits(got["albedo"][~on]), bits(plain["albedo"][~on]))
    for k in ("normal", "position", "hit_fraction"):
        assert np.array_equal(bits(got[k]), bits(plain[k])), k
