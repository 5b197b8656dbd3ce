"""The route rule (cuda-pathtracer_amd/host/route_rule.h) without a GPU: which configs the per-lane features refuse, with which
words and in which order, and which runs take the per-lane kernel.  tests/route_rule_shim.cpp is compiled with the host C++
compiler.  The messages below are the literal strings csrc/c_api.cpp held before the table existed; the order is restated here
as a plain loop over feature, then field.  tests/route_rule_check.cpp walks the same table under ASan and UBSan."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATURES = ("next_event", "environment", "surfaces", "vertex normals", "albedo texture", "lens", "medium")   # ptmi_set_config's order
INTEGRATOR, SAMPLING_MODE, FAST_TREE = 0, 1, 2                                                                # ... and a feature's
CONFIGS = list(itertools.product((0, 1), range(5), (0, 1)))                                                   # the 20 configs

# feature -> field -> what ptmi_set_config says when the feature is present (19)
CONFIG_MESSAGES = {
    "next_event": {
        INTEGRATOR: "next_event needs integrator 0 (PathTracing): the Radiosity view traces first hits only",
        SAMPLING_MODE: "next_event needs sampling_mode 0 (BSDF): MIS against the guided modes' grid pdf is not implemented",
        FAST_TREE: "next_event needs fast_tree 0: NEE frames always trace the reference's hits"},
    "environment": {
        INTEGRATOR: "an environment is set: it needs integrator 0 (PathTracing): the Radiosity view traces first hits only",
        SAMPLING_MODE: "an environment is set: it needs sampling_mode 0 (BSDF): the guided modes do not look the environment up",
        FAST_TREE: "an environment is set: it needs fast_tree 0: environment frames always trace the reference's hits"},
    "surfaces": {
        INTEGRATOR: "specular surfaces are set: they need integrator 0 (PathTracing): the Radiosity view traces first hits only",
        SAMPLING_MODE: "specular surfaces are set: they need sampling_mode 0 (BSDF): the guided modes sample a diffuse lobe at every vertex",
        FAST_TREE: "specular surfaces are set: they need fast_tree 0: specular frames always trace the reference's hits"},
    "vertex normals": {
        INTEGRATOR: "vertex normals are set: they need integrator 0 (PathTracing): the Radiosity view shades nothing",
        SAMPLING_MODE: "vertex normals are set: they need sampling_mode 0 (BSDF): the guided modes' grids lie about the stored normal",
        FAST_TREE: "vertex normals are set: they need fast_tree 0: frames with vertex normals always trace the reference's hits"},
    "albedo texture": {
        INTEGRATOR: "an albedo texture is set: it needs integrator 0 (PathTracing): the Radiosity view ignores the texture",
        SAMPLING_MODE: "an albedo texture is set: it needs sampling_mode 0 (BSDF): the guided modes run through the bounce kernels",
        FAST_TREE: "an albedo texture is set: it needs fast_tree 0: textured frames always trace the reference's hits"},
    "lens": {                                                      # (integrator 1 is allowed: the Radiosity view keeps the pinhole)
        SAMPLING_MODE: "a lens is set: it needs sampling_mode 0 (BSDF): the guided modes run through the bounce kernels",
        FAST_TREE: "a lens is set: it needs fast_tree 0: frames through a lens always trace the reference's hits"},
    "medium": {                                                    # (integrator 1 is allowed: the Radiosity view sees vacuum)
        SAMPLING_MODE: "a medium is set: it needs sampling_mode 0 (BSDF): the guided modes run through the bounce kernels",
        FAST_TREE: "a medium is set: it needs fast_tree 0: frames through a medium always trace the reference's hits"},
}
# feature -> field -> what the feature's setter says under a config that has the field set (16; next_event has no setter)
SETTER_MESSAGES = {
    "environment": {
        INTEGRATOR: "environment: the config has integrator 1 (Radiosity), which traces first hits only",
        SAMPLING_MODE: "environment: the config has a guided sampling_mode, which does not look the environment up",
        FAST_TREE: "environment: the config has fast_tree 1; environment frames always trace the reference's hits"},
    "surfaces": {
        INTEGRATOR: "surfaces: the config has integrator 1 (Radiosity), which traces first hits only",
        SAMPLING_MODE: "surfaces: the config has a guided sampling_mode, which samples a diffuse lobe at every vertex",
        FAST_TREE: "surfaces: the config has fast_tree 1; specular frames always trace the reference's hits"},
    "vertex normals": {
        INTEGRATOR: "vertex normals: the config has integrator 1 (Radiosity), which shades nothing",
        SAMPLING_MODE: "vertex normals: the config has a guided sampling_mode, whose grids lie about the stored normal",
        FAST_TREE: "vertex normals: the config has fast_tree 1; frames with vertex normals always trace the reference's hits"},
    "albedo texture": {
        INTEGRATOR: "albedo texture: the config has integrator 1 (Radiosity), which ignores the texture",
        SAMPLING_MODE: "albedo texture: the config has a guided sampling_mode, which runs through the bounce kernels",
        FAST_TREE: "albedo texture: the config has fast_tree 1; textured frames always trace the reference's hits"},
    "lens": {
        SAMPLING_MODE: "lens: the config has a guided sampling_mode, which runs through the bounce kernels",
        FAST_TREE: "lens: the config has fast_tree 1; frames through a lens always trace the reference's hits"},
    "medium": {
        SAMPLING_MODE: "medium: the config has a guided sampling_mode, which runs through the bounce kernels",
        FAST_TREE: "medium: the config has fast_tree 1; frames through a medium always trace the reference's hits"},
}


def first_refusal(messages, features, config):
    """the order, restated: feature by feature, and within one integrator, sampling_mode, fast_tree"""
    for feature in features:
        for field in (INTEGRATOR, SAMPLING_MODE, FAST_TREE):
            if config[field] != 0 and field in messages[feature]:
                return messages[feature][field]
    return ""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("needs a C++ compiler")
    so = str(tmp_path_factory.mktemp("route_rule") / "libroute_rule_shim.so")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(ROOT, "tests", "route_rule_shim.cpp")])
    L = C.CDLL(so)
    L.shim_n_features.restype = C.c_int; L.shim_n_features.argtypes = []
    L.shim_config_refusal.restype = C.c_int; L.shim_config_refusal.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.shim_feature_refusal.restype = C.c_int; L.shim_feature_refusal.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.shim_route.restype = C.c_int; L.shim_route.argtypes = [C.c_uint, C.c_int]
    return L


def message(call, *args):
    buf = C.create_string_buffer(256)
    n = call(*args, buf, len(buf))
    assert n >= 0 and n == len(buf.value), args
    return buf.value.decode()


def test_the_tables_of_this_file():
    assert sum(len(v) for v in CONFIG_MESSAGES.values()) == 19 and sum(len(v) for v in SETTER_MESSAGES.values()) == 16
    assert tuple(CONFIG_MESSAGES) == FEATURES and tuple(SETTER_MESSAGES) == FEATURES[1:]
    every = [m for t in (CONFIG_MESSAGES, SETTER_MESSAGES) for v in t.values() for m in v.values()]
    assert len(set(every)) == 35


def test_config_direction_every_mask_and_config(shim):
    assert shim.shim_n_features() == len(FEATURES)
    refused = 0
    for mask in range(1 << len(FEATURES)):
        present = [f for k, f in enumerate(FEATURES) if mask >> k & 1]
        for config in CONFIGS:
            want = first_refusal(CONFIG_MESSAGES, present, config)
            assert message(shim.shim_config_refusal, mask, *config) == want, (present, config)
            refused += want != ""
    assert 0 < refused < (1 << len(FEATURES)) * len(CONFIGS)


def test_each_config_message_is_reached(shim):
    """one feature, one offending field: the literal message of exactly that pair"""
    for k, f in enumerate(FEATURES):
        for field, value in ((INTEGRATOR, 1), (SAMPLING_MODE, 3), (FAST_TREE, 1)):
            config = [0, 0, 0]; config[field] = value
            assert message(shim.shim_config_refusal, 1 << k, *config) == CONFIG_MESSAGES[f].get(field, ""), (f, field)


def test_setter_direction_every_feature_and_config(shim):
    for k, f in enumerate(FEATURES):
        if f not in SETTER_MESSAGES:
            continue                                               # next_event is a config field: it has no setter
        for config in CONFIGS:
            assert message(shim.shim_feature_refusal, k, *config) == first_refusal(SETTER_MESSAGES, [f], config), (f, config)
        for field, value in ((INTEGRATOR, 1), (SAMPLING_MODE, 4), (FAST_TREE, 1)):
            config = [0, 0, 0]; config[field] = value
            assert message(shim.shim_feature_refusal, k, *config) == SETTER_MESSAGES[f].get(field, ""), (f, field)


def test_route_every_mask_and_integrator(shim):
    for mask in range(1 << len(FEATURES)):
        for integrator in (0, 1):
            per_lane = mask != 0 and integrator == 0               # any feature present, and path tracing
            blocks = integrator == 0                               # the Radiosity view keeps the pinhole and sees vacuum
            assert shim.shim_route(mask, integrator) == (1 if per_lane else 0) | (2 if blocks else 0), (mask, integrator)


def test_a_config_every_feature_accepts_takes_the_per_lane_route(shim):
    for mask in range(1, 1 << len(FEATURES)):
        assert message(shim.shim_config_refusal, mask, 0, 0, 0) == "" and shim.shim_route(mask, 0) & 1


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found (the build needs it too)")
    exe = str(tmp_path_factory.mktemp("route_rule_check") / "route_rule_check")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "route_rule_check.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def test_the_table_under_the_sanitizers(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[-2] == "ok %d" % ((1 << len(FEATURES)) * len(CONFIGS) + (len(FEATURES) - 1) * len(CONFIGS)), r.stdout[-2000:]
    assert not any(ln.startswith("FAILED") for ln in lines), r.stdout[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
