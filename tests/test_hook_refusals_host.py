"""Every test hook (ptmi_debug_*) of libptmi.so refuses a NULL context before it touches a device: the call returns
PTMI_E_INVALID and ptmi_last_error() is the text recorded below, which is what the library answered before the hooks moved into
csrc/c_api_hooks.cpp.  One table row per hook; a hook in ptmi.EXPORTS without a row fails the test, so a new one cannot skip it.
No GPU is needed: the other arguments are small and well formed, and a hook that reached hipSetDevice first would answer
PTMI_E_NO_DEVICE on a machine without one.
"""
import ctypes as C

import numpy as np

import ptmi

PTMI_E_INVALID = -1
NULL_ARGUMENT, CTX_IS_NULL = b"NULL argument", b"ctx is NULL"
ONE_BITS = 0x3f800000

F = np.zeros(4096, np.float32)
D = np.zeros(64, np.float64)
I = np.zeros(1024, np.int32)
U = np.zeros(64, np.uint32)
U64 = np.zeros(4, np.uint64)
B = np.zeros(8 * 8 * 3, np.uint8)
f, d, i, u, u64, b = (a.ctypes.data for a in (F, D, I, U, U64, B))
an_int = lambda: C.byref(C.c_int())
a_u64 = lambda: C.byref(C.c_uint64())
a_u32 = lambda: C.byref(C.c_uint32())

# hook -> (the arguments after the context, the refusal's text)
ROWS = {
    "ptmi_debug_lens_block": ((f,), NULL_ARGUMENT),
    "ptmi_debug_lens_ray": ((1, i, i, f, f), NULL_ARGUMENT),
    "ptmi_debug_medium_call": ((0, 1, f, f), NULL_ARGUMENT),
    "ptmi_debug_place_tiles": ((8, 8, 1, 8, b, f, b, f), CTX_IS_NULL),
    "ptmi_debug_set_traversal": ((-1, 0, an_int()), CTX_IS_NULL),
    "ptmi_debug_get_traversal": ((an_int(),), b"ctx / out_mode is NULL"),
    "ptmi_debug_set_solver_walk": ((-1, 0), CTX_IS_NULL),
    "ptmi_debug_set_packed_min_nodes": ((0, an_int()), CTX_IS_NULL),
    "ptmi_debug_set_packed_top": ((0, an_int(), an_int()), CTX_IS_NULL),
    "ptmi_debug_set_fast_tree": ((2, 1.0, 1.0, 0, an_int(), an_int(), an_int()), CTX_IS_NULL),
    "ptmi_debug_intersect_fast": ((1, f, f, 0.0, 1.0, i, i, f, u64), NULL_ARGUMENT),
    "ptmi_debug_first_hit": ((1, f, f, 0.0, i, i, f), NULL_ARGUMENT),
    "ptmi_debug_intersect": ((1, f, f, 0.0, 1.0, i, i, f, f, f), NULL_ARGUMENT),
    "ptmi_debug_rng": ((0, 1, i, 1, f), NULL_ARGUMENT),
    "ptmi_debug_rcp_check": ((ONE_BITS, 1, a_u64(), a_u32()), NULL_ARGUMENT),
    "ptmi_debug_sqrt_check": ((ONE_BITS, 1, a_u64(), a_u32()), NULL_ARGUMENT),
    "ptmi_debug_ray_inv": ((1, f, i, f), NULL_ARGUMENT),
    "ptmi_debug_sincos_lean_check": ((ONE_BITS, 1, a_u64(), a_u64(), a_u32(), a_u64(), u, an_int()), NULL_ARGUMENT),
    "ptmi_debug_sincos_lean": ((1, f, i, f), NULL_ARGUMENT),
    "ptmi_debug_unit_voted": ((1, f, i, f), NULL_ARGUMENT),
    "ptmi_debug_size_div_check": ((8, ONE_BITS, 1, a_u64(), a_u32(), an_int()), NULL_ARGUMENT),
    "ptmi_debug_cosine_sample": ((1, f, f, f, f), NULL_ARGUMENT),
    "ptmi_debug_guided_sample": ((0, 1, 0, None, None, f, f, u, f, i), NULL_ARGUMENT),
    "ptmi_debug_math": ((0, 1, f, f, d), NULL_ARGUMENT),
    "ptmi_debug_grid_index": ((1, f, f, i), NULL_ARGUMENT),
    "ptmi_debug_nee_call": ((0, 1, f, f, i), NULL_ARGUMENT),
    "ptmi_debug_vertex_normal": ((1, i, f, f), NULL_ARGUMENT),
    "ptmi_debug_albedo": ((1, i, f, f), NULL_ARGUMENT),
    "ptmi_debug_set_temporal_moments": ((f, f, f), NULL_ARGUMENT),
    "ptmi_debug_set_filter_inputs": ((f, f, f, f, f, 2), NULL_ARGUMENT),
    "ptmi_debug_accum_step": ((f, f, f, u, i, 1, None, 1, i, an_int()), NULL_ARGUMENT),
    "ptmi_debug_order_by_cost": ((1, None, u, 1, 0, 1, i, i), NULL_ARGUMENT),
    "ptmi_debug_cdf_records": ((1, 2, f, f), NULL_ARGUMENT),
    "ptmi_debug_filter_pdfs": ((1, f, None, 1, 1.5, 0.3, f, f), NULL_ARGUMENT),
    "ptmi_debug_radiosity_grid": ((1, f, f, f, f, 0, 1, 1.5, 0.3, f), NULL_ARGUMENT),
}


def hooks():
    return [n for n in ptmi.EXPORTS if n.startswith("ptmi_debug_")]


def test_every_hook_has_a_row():
    assert sorted(hooks()) == sorted(ROWS), set(hooks()) ^ set(ROWS)


def test_every_hook_refuses_a_null_context():
    L = ptmi.lib()
    assert len(hooks()) == len(set(hooks())) >= 35
    for name in hooks():
        args, text = ROWS[name]
        assert L.ptmi_check_feature_shading(-1) == PTMI_E_INVALID and b"feature shading" in L.ptmi_last_error()   # another text first
        assert getattr(L, name)(None, *args) == PTMI_E_INVALID, name
        assert L.ptmi_last_error() == text, (name, L.ptmi_last_error())
    for a in (F, D, I, U, U64, B):
        assert not a.any()                                 # and nothing was written
