"""Host side of the temporal accumulation (include/ptmi.h: ptmi_temporal_accumulate) - no GPU needed."""
import ctypes as C
import os
import re

import pytest

import ptmi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_fields(name):
    header = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + ";", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            out += [f.strip() for f in re.sub(r"^\w+\s+", "", decl).split(",")]
    return out


def test_default_temporal_params():
    p = ptmi.default_temporal_params()
    assert (p.max_history, p.feature_grid) == (32, 2)
    assert (p.normal_min, p.sigma_position, p.sigma_albedo) == (ptmi.C.c_float(0.9).value, 0.0, ptmi.C.c_float(0.1).value)
    q = ptmi.default_temporal_params(max_history=4, sigma_position=0.25)
    assert (q.max_history, q.sigma_position, q.feature_grid) == (4, 0.25, 2)
    with pytest.raises(TypeError):
        ptmi.default_temporal_params(history=3)


def test_temporal_structs_match_the_header():
    for cls, name, size, offsets in ((ptmi.TemporalParams, "ptmi_temporal_params", 20, [0, 4, 8, 12, 16]),
                                     (ptmi.TemporalStats, "ptmi_temporal_stats", 40, [0, 8, 16, 24, 32])):
        fields = header_fields(name)
        assert fields == [f for f, _ in cls._fields_]
        assert C.sizeof(cls) == size
        assert [getattr(cls, f).offset for f in fields] == offsets


@pytest.mark.parametrize("bad", [dict(max_history=0), dict(max_history=65537), dict(normal_min=-1.01), dict(normal_min=1.01),
                                 dict(normal_min=float("nan")), dict(sigma_position=1e-9), dict(sigma_position=2e12),
                                 dict(sigma_position=float("nan")), dict(feature_grid=0), dict(feature_grid=5),
                                 dict(sigma_albedo=-0.1), dict(sigma_albedo=2e6), dict(sigma_albedo=float("nan"))])
def test_temporal_params_are_validated(bad):
    L = ptmi.lib()
    p = ptmi.default_temporal_params(**bad)
    assert L.ptmi_check_temporal_params(C.byref(p)) == -1
    assert list(bad)[0] in L.ptmi_last_error().decode()


def test_valid_temporal_params_pass():
    L = ptmi.lib()
    for ok in (dict(), dict(max_history=1), dict(max_history=65536), dict(normal_min=-1.0), dict(normal_min=1.0),
               dict(sigma_position=-1.0), dict(sigma_position=1e-6), dict(sigma_position=1e12), dict(feature_grid=1), dict(feature_grid=4),
               dict(sigma_albedo=0.0), dict(sigma_albedo=1e6)):
        assert L.ptmi_check_temporal_params(C.byref(ptmi.default_temporal_params(**ok))) == 0, ok


def test_temporal_entry_points_check_their_arguments():
    L = ptmi.lib()
    assert L.ptmi_temporal_accumulate(None, None, None) == -1 and L.ptmi_temporal_reset(None) == -1
    assert L.ptmi_read_temporal(None, None, None) == -1 and L.ptmi_read_history_counts(None, None) == -1
    assert L.ptmi_denoise_temporal(None, None) == -1 and L.ptmi_check_temporal_params(None) == -1
    L.ptmi_default_temporal_params(None)                 # ignored, as ptmi_default_denoise_params(NULL)
