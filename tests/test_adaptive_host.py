"""Host side of progressive / adaptive accumulation (include/ptmi.h: ptmi_accum_pass) - no GPU needed."""
import ctypes as C
import os
import re

import pytest

import ptmi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_adaptive_params():
    p = ptmi.default_adaptive_params()
    assert (p.min_passes, p.max_passes) == (4, 64)
    assert abs(p.threshold - 0.02) < 1e-7 and abs(p.floor - 0.01) < 1e-7
    q = ptmi.default_adaptive_params(threshold=0.5, max_passes=9)
    assert (q.min_passes, q.max_passes) == (4, 9) and q.threshold == 0.5
    with pytest.raises(TypeError):
        ptmi.default_adaptive_params(thresold=0.5)


def test_accumulation_structs_match_the_header():
    """the ctypes mirrors carry the header's fields in the header's order"""
    header = open(os.path.join(ROOT, "include", "ptmi.h")).read()

    def fields(name):
        body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + ";", header).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                out += [v.strip() for v in re.sub(r"^\w+\s+", "", decl).split(",")]
        return out
    assert fields("ptmi_adaptive_params") == [f for f, _ in ptmi.AdaptiveParams._fields_]
    assert fields("ptmi_pass_stats") == [f.rstrip("_") for f, _ in ptmi.PassStats._fields_]
    assert C.sizeof(ptmi.AdaptiveParams) == 16
    assert C.sizeof(ptmi.PassStats) == 8 * 15


def test_accumulation_entry_points_check_their_arguments():
    L = ptmi.lib()
    assert L.ptmi_accum_reset(None) == -1 and L.ptmi_accum_pass(None, None, None) == -1
    assert L.ptmi_read_sample_counts(None, None) == -1
    L.ptmi_default_adaptive_params(None)               # ignored, as ptmi_default_radiosity_params(NULL)
