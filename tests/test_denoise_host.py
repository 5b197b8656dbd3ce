"""Host side of the feature buffers and the denoiser (include/ptmi.h: ptmi_render_features, ptmi_denoise) - no GPU needed."""
import ctypes as C
import os
import re

import pytest

import ptmi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_denoise_params():
    p = ptmi.default_denoise_params()
    assert (p.iterations, p.normal_squarings, p.feature_grid, p.demodulate) == (5, 7, 2, 1)
    assert (p.sigma_color, p.color_floor, p.sigma_position) == (4.0, 2.0, 0.0)
    q = ptmi.default_denoise_params(iterations=3, sigma_position=0.25)
    assert (q.iterations, q.sigma_position, q.feature_grid) == (3, 0.25, 2)
    with pytest.raises(TypeError):
        ptmi.default_denoise_params(iteration=3)


def test_denoise_params_struct_matches_the_header():
    header = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*ptmi_denoise_params;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"^\w+\s+", "", d.strip()) for d in body.split(";") if d.strip()]
    assert fields == [f for f, _ in ptmi.DenoiseParams._fields_]
    assert C.sizeof(ptmi.DenoiseParams) == 28
    assert [getattr(ptmi.DenoiseParams, f).offset for f in fields] == [0, 4, 8, 12, 16, 20, 24]


@pytest.mark.parametrize("bad", [dict(iterations=-1), dict(iterations=11), dict(sigma_color=0.0), dict(sigma_color=float("nan")),
                                 dict(sigma_color=2e4), dict(color_floor=0.0), dict(color_floor=float("inf")),
                                 dict(sigma_position=1e-9), dict(sigma_position=float("nan")), dict(normal_squarings=-1),
                                 dict(normal_squarings=11), dict(feature_grid=0), dict(feature_grid=5), dict(demodulate=2)])
def test_denoise_params_are_validated(bad):
    L = ptmi.lib()
    p = ptmi.default_denoise_params(**bad)
    assert L.ptmi_check_denoise_params(C.byref(p)) == -1
    assert list(bad)[0] in L.ptmi_last_error().decode()


def test_valid_denoise_params_pass():
    L = ptmi.lib()
    for ok in (dict(), dict(iterations=0), dict(iterations=10), dict(sigma_position=-1.0), dict(sigma_position=1e-6),
               dict(normal_squarings=0), dict(feature_grid=4), dict(demodulate=0)):
        assert L.ptmi_check_denoise_params(C.byref(ptmi.default_denoise_params(**ok))) == 0, ok


def test_denoise_entry_points_check_their_arguments():
    L = ptmi.lib()
    assert L.ptmi_render_features(None, 2) == -1 and L.ptmi_denoise(None, None) == -1
    assert L.ptmi_read_features(None, None, None, None, None) == -1 and L.ptmi_read_denoised(None, None, None) == -1
    assert L.ptmi_denoise_timing(None, None, None) == -1 and L.ptmi_check_denoise_params(None) == -1
    L.ptmi_default_denoise_params(None)                  # ignored, as ptmi_default_adaptive_params(NULL)
