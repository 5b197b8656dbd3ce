"""The route rule (cuda-pathtracer_amd/host/route_rule.h) through the library: for each of the six settable per-lane features, the
config fields it refuses and the configs that refuse it, with their exact messages and nothing changed by a refusal, and the route
a frame takes with the feature on and after everything is cleared.  The messages are tests/test_route_rule.py's literals."""
import numpy as np
import pytest

import env_scenes as ES
import ptmi
from test_route_rule import CONFIG_MESSAGES, FAST_TREE, INTEGRATOR, SAMPLING_MODE, SETTER_MESSAGES

pytestmark = pytest.mark.gpu

F = np.float32
W = H = 8
FIELDS = ((INTEGRATOR, "integrator", 1), (SAMPLING_MODE, "sampling_mode", 3), (FAST_TREE, "fast_tree", 1))


def one_emitter_cube():
    """env_scenes.cube in front of the default camera: 12 triangles, the first of them the only emitter"""
    types, verts, normal, bsdf, Le = ES.cube((0.6, 0.5, 0.4), (4.0, 3.0, 2.0)).arrays()
    Le[1:] = 0.0
    return types, verts, normal, bsdf, Le


ARRAYS = one_emitter_cube()
N = len(ARRAYS[0])


def perturbed_normals():
    table = np.repeat(ARRAYS[2][:, None, :], 4, axis=1).astype(F)
    n = table[0, 0].astype(np.float64) + 0.2 * np.roll(table[0, 0].astype(np.float64), 1) + 0.1
    table[0, 0] = (n / np.linalg.norm(n)).astype(F)
    return table


def mirror_kinds():
    kind = np.zeros(N, np.int32); kind[0] = ptmi.SURFACE_MIRROR
    return kind


def one_textured():
    textured = np.zeros(N, np.int32); textured[0] = 1
    return textured


# feature -> (the smallest input that switches it on, what switches it off, whether *_info reports it on)
FEATURES = {
    "environment": (lambda R: R.set_environment(np.ones((1, 2, 3), F)), lambda R: R.set_environment(None),
                    lambda R: R.environment_info()["width"] != 0),
    "surfaces": (lambda R: R.set_surfaces(mirror_kinds()), lambda R: R.set_surfaces(None),
                 lambda R: R.surfaces_info()["n_mirror"] != 0 or any(R.surface_counts())),
    "vertex normals": (lambda R: R.set_vertex_normals(perturbed_normals()), lambda R: R.set_vertex_normals(None),
                       lambda R: R.vertex_normals_info()["n_smooth"] != 0),
    "albedo texture": (lambda R: R.set_albedo_texture(np.full((1, 1, 3), 0.5, F), np.zeros((N, 4, 2), F), one_textured()),
                       lambda R: R.set_albedo_texture(None, None), lambda R: R.albedo_texture_info()["n_textured"] != 0),
    "lens": (lambda R: R.set_lens(0.1), lambda R: R.set_lens(0.0), lambda R: R.lens()[0] != 0.0),
    "medium": (lambda R: R.set_medium((-2.0, 0.5, -2.0), (2.0, 4.5, 2.0), 0.2), lambda R: R.set_medium(None), lambda R: R.medium() is not None),
}


@pytest.fixture()
def R():
    r = ptmi.Renderer(0)
    r.load_scene_arrays(*ARRAYS)
    r.set_camera(ptmi.default_camera())
    r.update_resolution(W, H)
    r.set_config(spp=1, max_depth=3, sampling_mode=0, integrator=0, fast_tree=False, next_event=False)
    yield r
    r.close()


def frame(R):
    """(the radiance's bits, bounce_launches) of one frame from freshly seeded streams"""
    R.update_resolution(W, H)
    st = R.render_frame()
    return np.ascontiguousarray(R.read_image()[1], F).view(np.uint32), st.bounce_launches


def refused(call, message):
    with pytest.raises(ptmi.PtmiError) as err:
        call()
    assert str(err.value) == "ptmi error %d: %s" % (err.value.code, message)


@pytest.mark.parametrize("feature", list(FEATURES))
def test_refusals_both_ways_and_the_route(R, feature):
    on, off, is_on = FEATURES[feature]
    before, launches = frame(R)
    assert launches > 1 and not is_on(R)                           # the queue loop: two launches are queued before a count is back
    # the feature first: the per-lane route, and each field it refuses is refused with its message and changes nothing
    on(R)
    assert is_on(R)
    with_feature, launches = frame(R)
    assert launches == 1
    for field, name, value in FIELDS:
        if field in CONFIG_MESSAGES[feature]:
            refused(lambda: R.set_config(**{name: value}), CONFIG_MESSAGES[feature][field])
            R.config = ptmi.Config.from_buffer_copy(R.config); setattr(R.config, name, 0)
            again, launches = frame(R)                             # the context's config is what it was: the same frame by the same route
            assert launches == 1 and np.array_equal(again, with_feature), name
        else:
            R.set_config(**{name: value}); R.set_config(**{name: 0})
    # the config first: the feature is refused with its message and stays off
    off(R)
    assert not is_on(R)
    for field, name, value in FIELDS:
        R.set_config(**{name: value})
        if field in SETTER_MESSAGES[feature]:
            refused(lambda: on(R), SETTER_MESSAGES[feature][field])
        else:
            on(R); assert is_on(R); off(R)
        assert not is_on(R), name
        R.set_config(**{name: 0})
    # everything cleared: the queue loop again, and the frame it rendered before
    after, launches = frame(R)
    assert launches > 1 and np.array_equal(after, before)


def test_next_event_refuses_in_the_config_alone(R):
    for field, name, value in FIELDS:
        refused(lambda: R.set_config(next_event=True, **{name: value}), CONFIG_MESSAGES["next_event"][field])
        R.config = ptmi.Config.from_buffer_copy(R.config); R.config.next_event = 0; setattr(R.config, name, 0)
    assert frame(R)[1] > 1
    R.set_config(next_event=True)
    assert frame(R)[1] == 1
