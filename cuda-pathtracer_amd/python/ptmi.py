"""ctypes binding of libptmi.so (include/ptmi.h) — the product path.

No fallback: if the shared library is missing or no gfx950 device is usable, construction
raises.  Mirrors the reference's three host entry points:

    Renderer.load_scene(path, subdivision, convert_quads)   ~ SceneState::loadScene
    Renderer.update_resolution(w, h, tiling)                 ~ RenderState::updateResolution
    Renderer.render_frame()                                  ~ renderFrame()
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PTMI_LIB") or os.path.join(os.path.dirname(_HERE), "libptmi.so")   # PTMI_LIB: A/B experiments only

EXPORTS = [
    "ptmi_ctx_create", "ptmi_ctx_destroy", "ptmi_last_error", "ptmi_default_camera", "ptmi_default_config",
    "ptmi_default_tiling", "ptmi_load_scene", "ptmi_load_scene_arrays", "ptmi_scene_info", "ptmi_scene_get_prims",
    "ptmi_scene_get_bvh", "ptmi_update_resolution", "ptmi_set_camera", "ptmi_set_config", "ptmi_get_camera_frame",
    "ptmi_local_rows", "ptmi_local_row_map", "ptmi_render_frame", "ptmi_device_image", "ptmi_read_image",
    "ptmi_copy_image_device", "ptmi_set_radiosity_grids", "ptmi_get_precomputed_cdfs", "ptmi_set_radiosity",
           "ptmi_write_png", "ptmi_apply_grid_filter", "ptmi_use_raw_cdfs", "ptmi_get_filtered_pdfs", "ptmi_default_radiosity_params", "ptmi_run_radiosity_solver", "ptmi_get_radiosity_solution",
    "ptmi_debug_intersect", "ptmi_debug_rng", "ptmi_debug_cosine_sample", "ptmi_debug_guided_sample", "ptmi_debug_set_traversal", "ptmi_debug_rcp_check",
    "ptmi_debug_sqrt_check", "ptmi_debug_ray_inv",
    "ptmi_debug_sincos_lean_check", "ptmi_debug_sincos_lean", "ptmi_debug_unit_voted", "ptmi_debug_size_div_check",
    "ptmi_host_scene_load", "ptmi_host_scene_from_arrays", "ptmi_host_scene_free", "ptmi_host_scene_check_extent", "ptmi_host_scene_info",
    "ptmi_host_scene_get_prims", "ptmi_host_scene_get_bvh", "ptmi_host_camera_frame", "ptmi_host_local_row_map",
    "ptmi_host_cdf_record_layout", "ptmi_host_image",
    "ptmi_dist_unique_id", "ptmi_dist_init", "ptmi_dist_finalize", "ptmi_gather_frame", "ptmi_gather_wait", "ptmi_frame_device",
    "ptmi_read_frame", "ptmi_dist_barrier", "ptmi_dist_allreduce_max", "ptmi_debug_place_tiles", "ptmi_debug_set_packed_min_nodes", "ptmi_debug_set_packed_top", "ptmi_render_frames", "ptmi_select_frame",
    "ptmi_debug_set_fast_tree", "ptmi_debug_intersect_fast", "ptmi_debug_first_hit", "ptmi_dist_comm_count", "ptmi_host_fast_tree_build", "ptmi_host_fast_tree_intersect", "ptmi_host_fast_tree_stats",
    "ptmi_debug_set_solver_walk", "ptmi_debug_get_traversal",
    "ptmi_default_adaptive_params", "ptmi_accum_reset", "ptmi_accum_pass", "ptmi_read_sample_counts",
    "ptmi_default_denoise_params", "ptmi_check_denoise_params", "ptmi_render_features", "ptmi_read_features", "ptmi_denoise",
    "ptmi_read_denoised", "ptmi_denoise_timing",
    "ptmi_default_variance_params", "ptmi_check_variance_params", "ptmi_denoise_variance", "ptmi_read_variance",
    "ptmi_variance_timing", "ptmi_read_pass_moments",
    "ptmi_default_temporal_params", "ptmi_check_temporal_params", "ptmi_temporal_reset", "ptmi_temporal_accumulate",
    "ptmi_read_temporal", "ptmi_read_history_counts", "ptmi_denoise_temporal",
    "ptmi_set_temporal_moments", "ptmi_get_temporal_moments", "ptmi_read_temporal_moments", "ptmi_denoise_temporal_variance",
    "ptmi_debug_set_temporal_moments",
    "ptmi_host_emitters",
    "ptmi_debug_math", "ptmi_debug_grid_index", "ptmi_debug_nee_call",
    "ptmi_default_env_params", "ptmi_check_env_params", "ptmi_set_environment", "ptmi_environment_info", "ptmi_host_env_table",
    "ptmi_check_surfaces", "ptmi_set_surfaces", "ptmi_surfaces_info",
    "ptmi_check_surfaces_rough", "ptmi_set_surfaces_rough", "ptmi_surface_counts",
    "ptmi_check_vertex_normals", "ptmi_host_classify_vertex_normals", "ptmi_set_vertex_normals", "ptmi_vertex_normals_info",
    "ptmi_debug_vertex_normal",
    "ptmi_check_albedo_texture", "ptmi_set_albedo_texture", "ptmi_albedo_texture_info", "ptmi_debug_albedo",
    "ptmi_check_feature_shading", "ptmi_set_feature_shading", "ptmi_feature_shading",
    "ptmi_check_lens", "ptmi_set_lens", "ptmi_lens", "ptmi_host_lens_block", "ptmi_debug_lens_block", "ptmi_debug_lens_ray",
    "ptmi_default_medium", "ptmi_check_medium", "ptmi_set_medium", "ptmi_medium_info", "ptmi_host_medium_block", "ptmi_debug_medium_call",
    "ptmi_debug_set_filter_inputs",
    "ptmi_debug_accum_step", "ptmi_debug_order_by_cost",
    "ptmi_debug_cdf_records", "ptmi_debug_filter_pdfs", "ptmi_debug_radiosity_grid",
]

FEATURE_TEXTURED_ALBEDO, FEATURE_SHADING_NORMAL = 1, 2      # PTMI_FEATURE_*


class Medium(C.Structure):
    """ptmi_medium: a homogeneous medium inside the axis-aligned box [lo, hi] (include/ptmi.h: "participating medium")"""
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3), ("sigma_t", C.c_float), ("albedo", C.c_float * 3), ("g", C.c_float)]


MEDIUM_CALL_IN, MEDIUM_CALL_OUT = 20, 8                     # PTMI_MEDIUM_CALL_*
MEDIUM_SEGMENT, MEDIUM_FREE_FLIGHT, MEDIUM_HG_VALUE, MEDIUM_HG_SAMPLE = 0, 1, 2, 3      # ptmi_debug_medium_call's ops


class Camera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("lookat", C.c_float * 3), ("vup", C.c_float * 3),
                ("vfov_deg", C.c_float), ("yaw_deg", C.c_float), ("pitch_deg", C.c_float), ("orbit", C.c_int)]


class Config(C.Structure):
    _fields_ = [("spp", C.c_int), ("max_depth", C.c_int), ("sampling_mode", C.c_int), ("seed_base", C.c_uint64),
                ("segments_per_launch", C.c_int), ("collect_stats", C.c_int), ("wave_tiles", C.c_int), ("streams", C.c_int), ("mis_bsdf_fraction", C.c_float), ("integrator", C.c_int),
                ("download_image", C.c_int), ("fast_tree", C.c_int), ("next_event", C.c_int)]


class Tiling(C.Structure):
    _fields_ = [("n_ranks", C.c_int), ("rank", C.c_int), ("row_block", C.c_int)]


class RadiosityParams(C.Structure):
    _fields_ = [("num_iterations", C.c_int), ("mc_samples", C.c_int), ("use_monte_carlo", C.c_int),
                ("enable_filtering", C.c_int), ("use_bilateral", C.c_int),
                ("filter_sigma_spatial", C.c_float), ("filter_sigma_range", C.c_float)]


class RadiosityStats(C.Structure):
    _fields_ = [("seconds", C.c_double), ("form_factor_ms", C.c_double), ("iteration_ms", C.c_double), ("grid_ms", C.c_double),
                ("pairs", C.c_uint64), ("rays", C.c_uint64), ("cert_chain", C.c_uint64), ("cert_fallback", C.c_uint64), ("walk", C.c_int)]


class Stats(C.Structure):
    _fields_ = [("seconds", C.c_double), ("bounce_kernel_ms", C.c_double), ("bounce_launches", C.c_uint64), ("path_visits", C.c_uint64),
                ("samples", C.c_uint64), ("rays", C.c_uint64), ("node_visits", C.c_uint64),
                ("prim_tests", C.c_uint64), ("hits", C.c_uint64), ("top_node_visits", C.c_uint64),
                ("cert_chain", C.c_uint64), ("cert_fallback", C.c_uint64)]


class AdaptiveParams(C.Structure):
    _fields_ = [("min_passes", C.c_int), ("max_passes", C.c_int), ("threshold", C.c_float), ("floor", C.c_float)]


class PassStats(C.Structure):
    _fields_ = [("pass_", C.c_int), ("active_before", C.c_uint64), ("active_after", C.c_uint64), ("samples", C.c_uint64),
                ("seconds", C.c_double), ("bounce_kernel_ms", C.c_double), ("bounce_launches", C.c_uint64), ("path_visits", C.c_uint64),
                ("rays", C.c_uint64), ("node_visits", C.c_uint64), ("prim_tests", C.c_uint64), ("hits", C.c_uint64),
                ("top_node_visits", C.c_uint64), ("cert_chain", C.c_uint64), ("cert_fallback", C.c_uint64)]


class DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_int), ("sigma_color", C.c_float), ("color_floor", C.c_float), ("sigma_position", C.c_float),
                ("normal_squarings", C.c_int), ("feature_grid", C.c_int), ("demodulate", C.c_int)]


class VarianceParams(C.Structure):
    _fields_ = [("iterations", C.c_int), ("sigma_luminance", C.c_float), ("epsilon", C.c_float), ("sigma_position", C.c_float),
                ("normal_squarings", C.c_int), ("feature_grid", C.c_int), ("demodulate", C.c_int), ("source", C.c_int),
                ("spatial_radius", C.c_int)]


class TemporalParams(C.Structure):
    _fields_ = [("max_history", C.c_int), ("normal_min", C.c_float), ("sigma_position", C.c_float), ("feature_grid", C.c_int),
                ("sigma_albedo", C.c_float)]


class TemporalStats(C.Structure):
    _fields_ = [("accepted", C.c_uint64), ("rejected", C.c_uint64), ("missed", C.c_uint64), ("seconds", C.c_double),
                ("features_ms", C.c_double)]


class EnvParams(C.Structure):
    _fields_ = [("scale", C.c_float), ("rotation_deg", C.c_float), ("select_fraction", C.c_float)]


class PtmiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ptmi error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Loads libptmi.so; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C cuda-pathtracer_amd` "
                               f"(or __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.ptmi_last_error.restype = C.c_char_p
        vp, ip, fp = C.c_void_p, C.POINTER(C.c_int), C.c_void_p
        L.ptmi_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.ptmi_ctx_destroy.argtypes = [vp]; L.ptmi_ctx_destroy.restype = None
        L.ptmi_default_camera.argtypes = [C.POINTER(Camera)]; L.ptmi_default_camera.restype = None
        L.ptmi_default_config.argtypes = [C.POINTER(Config)]; L.ptmi_default_config.restype = None
        L.ptmi_default_tiling.argtypes = [C.POINTER(Tiling)]; L.ptmi_default_tiling.restype = None
        L.ptmi_load_scene.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
        L.ptmi_load_scene_arrays.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
        L.ptmi_scene_info.argtypes = [vp, ip, ip, ip, ip, ip]
        L.ptmi_scene_get_prims.argtypes = [vp] * 6
        L.ptmi_scene_get_bvh.argtypes = [vp] * 7
        L.ptmi_update_resolution.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Tiling)]
        L.ptmi_set_camera.argtypes = [vp, C.POINTER(Camera)]
        L.ptmi_set_config.argtypes = [vp, C.POINTER(Config)]
        L.ptmi_get_camera_frame.argtypes = [vp, fp]
        L.ptmi_local_rows.argtypes = [vp, ip]
        L.ptmi_local_row_map.argtypes = [vp, vp]
        L.ptmi_render_frame.argtypes = [vp, C.POINTER(Stats)]
        L.ptmi_render_frames.argtypes = [vp, C.c_int, C.POINTER(Stats)]
        L.ptmi_select_frame.argtypes = [vp, C.c_int]
        L.ptmi_device_image.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.ptmi_read_image.argtypes = [vp, vp, vp]
        L.ptmi_copy_image_device.argtypes = [vp, vp, vp]
        L.ptmi_set_radiosity_grids.argtypes = [vp, C.c_int, vp]
        L.ptmi_get_precomputed_cdfs.argtypes = [vp, vp]
        L.ptmi_set_radiosity.argtypes = [vp, C.c_int, vp]
        L.ptmi_apply_grid_filter.argtypes = [vp, C.c_int, C.c_float, C.c_float]
        L.ptmi_use_raw_cdfs.argtypes = [vp]
        L.ptmi_get_filtered_pdfs.argtypes = [vp, vp, vp]
        L.ptmi_default_radiosity_params.argtypes = [C.POINTER(RadiosityParams)]
        L.ptmi_default_radiosity_params.restype = None
        L.ptmi_run_radiosity_solver.argtypes = [vp, C.POINTER(RadiosityParams), C.POINTER(RadiosityStats)]
        L.ptmi_get_radiosity_solution.argtypes = [vp] * 6
        L.ptmi_debug_intersect.argtypes = [vp, C.c_int, vp, vp, C.c_float, C.c_float, vp, vp, vp, vp, vp]
        L.ptmi_debug_rng.argtypes = [vp, C.c_uint64, C.c_int, vp, C.c_int, vp]
        L.ptmi_debug_cosine_sample.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        L.ptmi_debug_guided_sample.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
        L.ptmi_debug_math.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
        L.ptmi_debug_grid_index.argtypes = [vp, C.c_int, vp, vp, vp]
        L.ptmi_debug_nee_call.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
        L.ptmi_debug_set_traversal.argtypes = [vp, C.c_int, C.c_int, ip]
        L.ptmi_debug_set_solver_walk.argtypes = [vp, C.c_int, C.c_int]
        L.ptmi_debug_get_traversal.argtypes = [vp, ip]
        L.ptmi_debug_rcp_check.argtypes = [vp, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        if hasattr(L, "ptmi_debug_sqrt_check"):      # an A/B library (PTMI_LIB) built from an older commit has neither
            L.ptmi_debug_sqrt_check.argtypes = [vp, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
            L.ptmi_debug_ray_inv.argtypes = [vp, C.c_int, vp, vp, vp]
        if hasattr(L, "ptmi_debug_sincos_lean_check"):      # likewise
            p64, p32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
            L.ptmi_debug_sincos_lean_check.argtypes = [vp, C.c_uint32, C.c_uint64, p64, p64, p32, p64, vp, ip]
            L.ptmi_debug_sincos_lean.argtypes = [vp, C.c_int, vp, vp, vp]
            L.ptmi_debug_unit_voted.argtypes = [vp, C.c_int, vp, vp, vp]
            L.ptmi_debug_size_div_check.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint64, p64, p32, ip]
        L.ptmi_host_scene_load.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
        L.ptmi_host_scene_from_arrays.argtypes = [C.c_int, vp, vp, vp, vp, vp, C.POINTER(vp)]
        L.ptmi_host_scene_free.argtypes = [vp]; L.ptmi_host_scene_free.restype = None
        L.ptmi_host_scene_info.argtypes = [vp, ip, ip, ip, ip, ip]
        L.ptmi_host_scene_check_extent.argtypes = [vp, vp]
        L.ptmi_host_scene_get_prims.argtypes = [vp] * 6
        L.ptmi_host_scene_get_bvh.argtypes = [vp] * 7
        L.ptmi_host_emitters.argtypes = [vp, ip, vp, vp, vp]
        L.ptmi_host_camera_frame.argtypes = [C.POINTER(Camera), C.c_int, C.c_int, vp]
        L.ptmi_host_local_row_map.argtypes = [C.c_int, C.POINTER(Tiling), ip, vp]
        L.ptmi_write_png.argtypes = [C.c_char_p, C.c_int, C.c_int, vp]
        L.ptmi_host_cdf_record_layout.argtypes = [vp]
        L.ptmi_host_image.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
        L.ptmi_dist_unique_id.argtypes = [vp]
        L.ptmi_dist_init.argtypes = [vp, vp, C.c_int, C.c_int]
        L.ptmi_dist_finalize.argtypes = [vp]
        L.ptmi_gather_frame.argtypes = [vp, C.c_int, C.c_int]
        L.ptmi_gather_wait.argtypes = [vp]
        L.ptmi_frame_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.ptmi_read_frame.argtypes = [vp, vp, vp]
        L.ptmi_dist_barrier.argtypes = [vp]
        L.ptmi_dist_comm_count.argtypes = [vp, ip]
        L.ptmi_dist_allreduce_max.argtypes = [vp, C.POINTER(C.c_double)]
        L.ptmi_debug_set_packed_min_nodes.argtypes = [vp, C.c_int, ip]
        L.ptmi_debug_set_packed_top.argtypes = [vp, C.c_int, ip, ip]
        L.ptmi_debug_place_tiles.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
        L.ptmi_debug_set_fast_tree.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_int, ip, ip, ip]
        L.ptmi_debug_intersect_fast.argtypes = [vp, C.c_int, vp, vp, C.c_float, C.c_float, vp, vp, vp, vp]
        L.ptmi_debug_first_hit.argtypes = [vp, C.c_int, vp, vp, C.c_float, vp, vp, vp]
        L.ptmi_host_fast_tree_build.argtypes = [vp, C.c_int, C.c_float, C.c_float, ip, ip, C.POINTER(C.c_double)]
        L.ptmi_host_fast_tree_stats.argtypes = [vp, vp]
        L.ptmi_host_fast_tree_intersect.argtypes = [vp, C.c_int, vp, vp, C.c_float, C.c_float, vp, vp, vp]
        L.ptmi_default_adaptive_params.argtypes = [C.POINTER(AdaptiveParams)]; L.ptmi_default_adaptive_params.restype = None
        L.ptmi_accum_reset.argtypes = [vp]
        L.ptmi_accum_pass.argtypes = [vp, C.POINTER(AdaptiveParams), C.POINTER(PassStats)]
        L.ptmi_read_sample_counts.argtypes = [vp, vp]
        L.ptmi_default_denoise_params.argtypes = [C.POINTER(DenoiseParams)]; L.ptmi_default_denoise_params.restype = None
        L.ptmi_check_denoise_params.argtypes = [C.POINTER(DenoiseParams)]
        L.ptmi_render_features.argtypes = [vp, C.c_int]
        L.ptmi_read_features.argtypes = [vp, vp, vp, vp, vp]
        L.ptmi_denoise.argtypes = [vp, C.POINTER(DenoiseParams)]
        L.ptmi_read_denoised.argtypes = [vp, vp, vp]
        L.ptmi_denoise_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.ptmi_default_variance_params.argtypes = [C.POINTER(VarianceParams)]; L.ptmi_default_variance_params.restype = None
        L.ptmi_check_variance_params.argtypes = [C.POINTER(VarianceParams)]
        L.ptmi_denoise_variance.argtypes = [vp, C.POINTER(VarianceParams)]
        L.ptmi_read_variance.argtypes = [vp, vp, vp]
        L.ptmi_variance_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.ptmi_read_pass_moments.argtypes = [vp, vp, vp, vp]
        L.ptmi_default_temporal_params.argtypes = [C.POINTER(TemporalParams)]; L.ptmi_default_temporal_params.restype = None
        L.ptmi_check_temporal_params.argtypes = [C.POINTER(TemporalParams)]
        L.ptmi_temporal_reset.argtypes = [vp]
        L.ptmi_temporal_accumulate.argtypes = [vp, C.POINTER(TemporalParams), C.POINTER(TemporalStats)]
        L.ptmi_read_temporal.argtypes = [vp, vp, vp]
        L.ptmi_read_history_counts.argtypes = [vp, vp]
        L.ptmi_denoise_temporal.argtypes = [vp, C.POINTER(DenoiseParams)]
        L.ptmi_default_env_params.argtypes = [C.POINTER(EnvParams)]; L.ptmi_default_env_params.restype = None
        L.ptmi_check_env_params.argtypes = [C.POINTER(EnvParams)]
        L.ptmi_set_environment.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(EnvParams)]
        L.ptmi_environment_info.argtypes = [vp, ip, ip, C.POINTER(C.c_float)]
        L.ptmi_host_env_table.argtypes = [C.c_int, C.c_int, vp, C.POINTER(EnvParams), vp, vp, vp, vp, C.POINTER(C.c_float)]
        L.ptmi_check_surfaces.argtypes = [C.c_int, vp, vp]
        L.ptmi_set_surfaces.argtypes = [vp, C.c_int, vp, vp]
        L.ptmi_surfaces_info.argtypes = [vp, ip, ip]
        L.ptmi_check_surfaces_rough.argtypes = [C.c_int, vp, vp, vp]
        L.ptmi_set_surfaces_rough.argtypes = [vp, C.c_int, vp, vp, vp]
        L.ptmi_surface_counts.argtypes = [vp, vp]
        if hasattr(L, "ptmi_set_vertex_normals"):      # an A/B library (PTMI_LIB) built from an older commit has none of them
            L.ptmi_check_vertex_normals.argtypes = [C.c_int, vp]
            L.ptmi_host_classify_vertex_normals.argtypes = [C.c_int, vp, vp, vp, vp, ip]
            L.ptmi_set_vertex_normals.argtypes = [vp, C.c_int, vp]
            L.ptmi_vertex_normals_info.argtypes = [vp, ip]
            L.ptmi_debug_vertex_normal.argtypes = [vp, C.c_int, vp, vp, vp]
        if hasattr(L, "ptmi_set_albedo_texture"):      # likewise
            L.ptmi_check_albedo_texture.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp]
            L.ptmi_set_albedo_texture.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp]
            L.ptmi_albedo_texture_info.argtypes = [vp, ip, ip, ip, ip]
            L.ptmi_debug_albedo.argtypes = [vp, C.c_int, vp, vp, vp]
        if hasattr(L, "ptmi_set_feature_shading"):     # likewise
            L.ptmi_check_feature_shading.argtypes = [C.c_int]
            L.ptmi_set_feature_shading.argtypes = [vp, C.c_int]
            L.ptmi_feature_shading.argtypes = [vp, ip]
        if hasattr(L, "ptmi_set_lens"):                # likewise
            fp = C.POINTER(C.c_float)
            L.ptmi_check_lens.argtypes = [C.c_float, C.c_float]
            L.ptmi_set_lens.argtypes = [vp, C.c_float, C.c_float]
            L.ptmi_lens.argtypes = [vp, fp, fp]
            L.ptmi_host_lens_block.argtypes = [C.POINTER(Camera), C.c_int, C.c_int, C.c_float, C.c_float, vp]
            L.ptmi_debug_lens_block.argtypes = [vp, vp]
            L.ptmi_debug_lens_ray.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        if hasattr(L, "ptmi_set_medium"):              # likewise
            mp = C.POINTER(Medium)
            L.ptmi_default_medium.argtypes = [mp]; L.ptmi_default_medium.restype = None
            L.ptmi_check_medium.argtypes = [mp]
            L.ptmi_set_medium.argtypes = [vp, mp]
            L.ptmi_medium_info.argtypes = [vp, mp, ip]
            L.ptmi_host_medium_block.argtypes = [mp, vp]
            L.ptmi_debug_medium_call.argtypes = [vp, C.c_int, C.c_int, vp, vp]
        if hasattr(L, "ptmi_set_temporal_moments"):    # likewise
            L.ptmi_set_temporal_moments.argtypes = [vp, C.c_int]
            L.ptmi_get_temporal_moments.argtypes = [vp, ip]
            L.ptmi_read_temporal_moments.argtypes = [vp, vp, vp, vp]
            L.ptmi_denoise_temporal_variance.argtypes = [vp, C.POINTER(VarianceParams)]
            L.ptmi_debug_set_temporal_moments.argtypes = [vp, vp, vp, vp]
        if hasattr(L, "ptmi_debug_set_filter_inputs"): # likewise
            L.ptmi_debug_set_filter_inputs.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int]
        if hasattr(L, "ptmi_debug_accum_step"):        # likewise
            L.ptmi_debug_accum_step.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(AdaptiveParams), C.c_int, vp, ip]
            L.ptmi_debug_order_by_cost.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_uint32, C.c_int, vp, vp]
        if hasattr(L, "ptmi_debug_cdf_records"):       # likewise
            L.ptmi_debug_cdf_records.argtypes = [vp, C.c_int, C.c_int, vp, vp]
            L.ptmi_debug_filter_pdfs.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_float, C.c_float, vp, vp]
            L.ptmi_debug_radiosity_grid.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_float, C.c_float, vp]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise PtmiError(rc, lib().ptmi_last_error().decode(errors="replace"))


class HostScene:
    """Host half of loadScene (parse, convert, subdivide, BVH) - needs no GPU."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def load(cls, filename, subdivision_count=0, convert_quads=False):
        h = C.c_void_p()
        _check(lib().ptmi_host_scene_load(os.fsencode(filename), int(subdivision_count), int(bool(convert_quads)), C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, types, verts, normal, bsdf, Le):
        types = np.ascontiguousarray(types, np.int32)
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 4, 3)
        normal, bsdf, Le = (np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (normal, bsdf, Le))
        h = C.c_void_p()
        _check(lib().ptmi_host_scene_from_arrays(len(types), types.ctypes.data, verts.ctypes.data, normal.ctypes.data,
                                                 bsdf.ctypes.data, Le.ctypes.data, C.byref(h)))
        return cls(h)

    def __del__(self):
        try:
            if self.h and self.h.value:
                lib().ptmi_host_scene_free(self.h)
        except Exception:
            pass

    def check_extent(self, origin=None):
        """Raises what loading this scene onto the device would raise for its extent (edges, coordinates, quad edge x reach);
        origin: a ray origin outside the scene, a camera, held to the same bound."""
        o = None if origin is None else np.ascontiguousarray(origin, np.float32)
        _check(lib().ptmi_host_scene_check_extent(self.h, None if o is None else o.ctypes.data))

    def info(self):
        v = [C.c_int() for _ in range(5)]
        _check(lib().ptmi_host_scene_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("n_prims", "n_tris", "n_quads", "n_bvh_nodes", "bvh_depth"), (x.value for x in v)))

    def prims(self):
        n = self.info()["n_prims"]
        t = np.zeros(n, np.int32); v = np.zeros((n, 4, 3), np.float32)
        nr = np.zeros((n, 3), np.float32); b = np.zeros((n, 3), np.float32); le = np.zeros((n, 3), np.float32)
        _check(lib().ptmi_host_scene_get_prims(self.h, t.ctypes.data, v.ctypes.data, nr.ctypes.data, b.ctypes.data, le.ctypes.data))
        return dict(type=t, verts=v, normal=nr, bsdf=b, Le=le)

    def bvh(self):
        info = self.info(); n, m = info["n_bvh_nodes"], info["n_prims"]
        bmin = np.zeros((n, 3), np.float32); bmax = np.zeros((n, 3), np.float32)
        left = np.zeros(n, np.int32); right = np.zeros(n, np.int32); count = np.zeros(n, np.int32); idx = np.zeros(m, np.int32)
        _check(lib().ptmi_host_scene_get_bvh(self.h, bmin.ctypes.data, bmax.ctypes.data, left.ctypes.data, right.ctypes.data,
                                             count.ctypes.data, idx.ctypes.data))
        return dict(bmin=bmin, bmax=bmax, left=left, right=right, count=count, indices=idx)

    def emitters(self):
        """The emitter table of next-event estimation (include/ptmi.h): load-order index and running sum c_j of every emitter,
        and pdf_area per primitive (load order, 0 where the primitive is not an emitter)."""
        n = C.c_int()
        _check(lib().ptmi_host_emitters(self.h, C.byref(n), None, None, None))
        prim = np.zeros(n.value, np.int32); cdf = np.zeros(n.value, np.float32)
        pdf_area = np.zeros(self.info()["n_prims"], np.float32)
        _check(lib().ptmi_host_emitters(self.h, C.byref(n), prim.ctypes.data, cdf.ctypes.data, pdf_area.ctypes.data))
        return dict(prim=prim, cdf=cdf, pdf_area=pdf_area)


    # --- the opt-in fast tree (csrc/wide_bvh.h), host halves ---
    def fast_tree_build(self, max_leaf=3, c_trav=1.0, c_tri=1.0):
        n = C.c_int(); d = C.c_int(); sah = C.c_double()
        _check(lib().ptmi_host_fast_tree_build(self.h, int(max_leaf), float(c_trav), float(c_tri), C.byref(n), C.byref(d), C.byref(sah)))
        return dict(n_nodes=n.value, depth=d.value, sah=sah.value)

    def fast_tree_stats(self):
        out = np.zeros(13, np.int32)
        _check(lib().ptmi_host_fast_tree_stats(self.h, out.ctypes.data))
        return dict(nodes_by_children=out[:9].tolist(), leaves_by_triangles=out[9:].tolist())

    def fast_tree_intersect(self, o, d, t_min=1e-4, t_max=3.4028234663852886e38):
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3); d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        n = len(o)
        prim = np.zeros(n, np.int32); t = np.zeros(n, np.float32); counts = np.zeros(3, np.uint64)
        _check(lib().ptmi_host_fast_tree_intersect(self.h, n, o.ctypes.data, d.ctypes.data, t_min, t_max, prim.ctypes.data, t.ctypes.data,
                                                   counts.ctypes.data))
        return dict(prim=prim, t=t, node_visits=int(counts[0]), prim_tests=int(counts[1]), max_stack=int(counts[2]))


def host_camera_frame(cam, width, height):
    out = np.zeros(12, np.float32)
    _check(lib().ptmi_host_camera_frame(C.byref(cam), int(width), int(height), out.ctypes.data))
    return out


def host_local_row_map(height, n_ranks, rank, row_block):
    t = Tiling(int(n_ranks), int(rank), int(row_block)); n = C.c_int()
    _check(lib().ptmi_host_local_row_map(int(height), C.byref(t), C.byref(n), None))
    rows = np.zeros(n.value, np.int32)
    if n.value:
        _check(lib().ptmi_host_local_row_map(int(height), C.byref(t), C.byref(n), rows.ctypes.data))
    return rows


def host_cdf_record_layout():
    out = np.zeros(10, np.int32)
    _check(lib().ptmi_host_cdf_record_layout(out.ctypes.data))
    return out


def default_camera():
    c = Camera(); lib().ptmi_default_camera(C.byref(c)); return c


def check_lens(radius, focus_distance):
    """ptmi_check_lens: raises PtmiError with the message of the first rejection; no context and no GPU"""
    _check(lib().ptmi_check_lens(float(radius), float(focus_distance)))


def make_medium(lo, hi, sigma_t, albedo=(1.0, 1.0, 1.0), g=0.0):
    """a Medium of the given numbers; albedo a scalar or three values"""
    m = Medium()
    lib().ptmi_default_medium(C.byref(m))
    a = np.broadcast_to(np.asarray(albedo, np.float32), (3,))
    for k in range(3):
        m.lo[k] = float(lo[k]); m.hi[k] = float(hi[k]); m.albedo[k] = float(a[k])
    m.sigma_t = float(sigma_t); m.g = float(g)
    return m


def check_medium(medium):
    """ptmi_check_medium: raises PtmiError with the message of the first rejection; no context and no GPU"""
    _check(lib().ptmi_check_medium(C.byref(medium)))


def host_medium_block(medium):
    """ptmi_host_medium_block: the three records (3, 4) float32 of a medium - (lo, sigma_t) (hi, g) (albedo, 0); no context and
    no GPU"""
    out = np.zeros((3, 4), np.float32)
    _check(lib().ptmi_host_medium_block(C.byref(medium), out.ctypes.data))
    return out


def host_lens_block(cam, width, height, radius, focus_distance):
    """ptmi_host_lens_block: the six records (6, 4) float32 of a lens over cam at width x height - (llc_f, W) (hor_f, 1 / W)
    (ver_f, H) (org, 1 / H) (a, 0) (b, 0); no context and no GPU"""
    out = np.zeros((6, 4), np.float32)
    _check(lib().ptmi_host_lens_block(C.byref(cam), int(width), int(height), float(radius), float(focus_distance), out.ctypes.data))
    return out


def default_focus_distance(cam):
    """|origin - lookat| of cam in binary32, products summed left to right: the focus distance of a context that was given none"""
    f = np.float32
    d = np.asarray(cam.origin, f) - np.asarray(cam.lookat, f)
    s = f(d[0] * d[0]); s = f(s + f(d[1] * d[1])); s = f(s + f(d[2] * d[2]))
    return float(np.sqrt(s))


def pinhole_centre_ray(frame12, width, height, px, py):
    """The pinhole ray through the centre of pixel (px, py) of the frame (org, llc, hor, ver) in binary32, camera_ray's expressions
    with both jitter numbers 0.5: (o, d) float32"""
    f = np.float32
    org, llc, hor, ver = (np.asarray(frame12, f).reshape(4, 3)[i] for i in range(4))
    u = f(f(f(px) + f(0.5)) / f(width)); v = f(f(f(py) + f(0.5)) / f(height))
    w = (((llc + (u * hor).astype(f)).astype(f) + (v * ver).astype(f)).astype(f) - org).astype(f)
    n2 = f(w[0] * w[0]); n2 = f(n2 + f(w[1] * w[1])); n2 = f(n2 + f(w[2] * w[2]))
    k = f(f(1.0) / f(np.sqrt(n2)))
    return org.copy(), (w * k).astype(f)


def depth_along_axis(frame12, d, t):
    """t * dot(d, axis) in binary64, axis = unit(llc + 0.5 hor + 0.5 ver - org): the depth along the optical axis of the point at
    distance t along the unit direction d - what a focus distance is measured in"""
    org, llc, hor, ver = (np.asarray(frame12, np.float64).reshape(4, 3)[i] for i in range(4))
    axis = llc + 0.5 * hor + 0.5 * ver - org
    axis = axis / np.sqrt(np.dot(axis, axis))
    return float(t) * float(np.dot(np.asarray(d, np.float64), axis))


def default_config():
    c = Config(); lib().ptmi_default_config(C.byref(c)); return c


def default_adaptive_params(**params):
    """ptmi_default_adaptive_params, with any field overridden by keyword (min_passes, max_passes, threshold, floor)."""
    p = AdaptiveParams(); lib().ptmi_default_adaptive_params(C.byref(p))
    for k, v in params.items():
        if k not in dict(AdaptiveParams._fields_):
            raise TypeError(f"unknown adaptive parameter {k}")
        setattr(p, k, type(getattr(p, k))(v))
    return p


def default_denoise_params(**params):
    """ptmi_default_denoise_params, with any field overridden by keyword (iterations, sigma_color, color_floor, sigma_position,
    normal_squarings, feature_grid, demodulate)."""
    p = DenoiseParams(); lib().ptmi_default_denoise_params(C.byref(p))
    for k, v in params.items():
        if k not in dict(DenoiseParams._fields_):
            raise TypeError(f"unknown denoise parameter {k}")
        setattr(p, k, type(getattr(p, k))(v))
    return p


def default_variance_params(**params):
    """ptmi_default_variance_params, with any field overridden by keyword (iterations, sigma_luminance, epsilon, sigma_position,
    normal_squarings, feature_grid, demodulate, source, spatial_radius)."""
    p = VarianceParams(); lib().ptmi_default_variance_params(C.byref(p))
    for k, v in params.items():
        if k not in dict(VarianceParams._fields_):
            raise TypeError(f"unknown variance parameter {k}")
        setattr(p, k, type(getattr(p, k))(v))
    return p


def default_temporal_params(**params):
    """ptmi_default_temporal_params, with any field overridden by keyword (max_history, normal_min, sigma_position,
    feature_grid, sigma_albedo)."""
    p = TemporalParams(); lib().ptmi_default_temporal_params(C.byref(p))
    for k, v in params.items():
        if k not in dict(TemporalParams._fields_):
            raise TypeError(f"unknown temporal parameter {k}")
        setattr(p, k, type(getattr(p, k))(v))
    return p


def default_env_params(**params):
    """ptmi_default_env_params, with any field overridden by keyword (scale, rotation_deg, select_fraction)."""
    p = EnvParams(); lib().ptmi_default_env_params(C.byref(p))
    for k, v in params.items():
        if k not in dict(EnvParams._fields_):
            raise TypeError(f"unknown environment parameter {k}")
        setattr(p, k, float(v))
    return p


def _env_map(rgb):
    rgb = np.ascontiguousarray(rgb, np.float32)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("an environment map is (height, width, 3), row 0 at +y")
    return rgb


def host_env_table(rgb, **params):
    """The sampling table of an environment map (include/ptmi.h: "environment lighting"), host only: z (h + 1), marginal_cdf
    (h), row_cdf (h, w), texel (h, w, 4: scaled rgb and the pdf per solid angle) and total."""
    rgb = _env_map(rgb)
    h, w = rgb.shape[:2]
    p = default_env_params(**params)
    z = np.zeros(h + 1, np.float32); m = np.zeros(h, np.float32); c = np.zeros((h, w), np.float32)
    t = np.zeros((h, w, 4), np.float32); total = C.c_float()
    _check(lib().ptmi_host_env_table(w, h, rgb.ctypes.data, C.byref(p), z.ctypes.data, m.ctypes.data, c.ctypes.data, t.ctypes.data,
                                     C.byref(total)))
    return dict(z=z, marginal_cdf=m, row_cdf=c, texel=t, total=np.float32(total.value))


SURFACE_DIFFUSE, SURFACE_MIRROR, SURFACE_GLASS = 0, 1, 2      # PTMI_SURFACE_*
SURFACE_ROUGH = 3                                             # rough metal: ptmi_set_surfaces_rough only


def _surface_table(kind, ior, roughness=None):
    kind = np.ascontiguousarray(kind, np.int32).reshape(-1)
    if ior is not None:
        ior = np.ascontiguousarray(np.broadcast_to(np.asarray(ior, np.float32), kind.shape))
    if roughness is not None:
        roughness = np.ascontiguousarray(np.broadcast_to(np.asarray(roughness, np.float32), kind.shape))
    return (kind, ior) if roughness is None else (kind, ior, roughness)


def _ptr(a):
    return None if a is None else a.ctypes.data


def check_surfaces(kind, ior=None, roughness=None):
    """ptmi_check_surfaces: raises PtmiError for a table ptmi_set_surfaces would reject on its own account (host only).  With a
    roughness (a scalar or (n_prims,)): ptmi_check_surfaces_rough, which accepts SURFACE_ROUGH."""
    if roughness is None:
        kind, ior = _surface_table(kind, ior)
        _check(lib().ptmi_check_surfaces(len(kind), kind.ctypes.data, _ptr(ior)))
        return
    kind, ior, roughness = _surface_table(kind, ior, roughness)
    _check(lib().ptmi_check_surfaces_rough(len(kind), kind.ctypes.data, _ptr(ior), roughness.ctypes.data))


def _normal_table(normals):
    normals = np.ascontiguousarray(normals, np.float32)
    if normals.ndim != 3 or normals.shape[1:] != (4, 3):
        raise ValueError("vertex normals must be (n_prims, 4, 3)")
    return normals


def check_vertex_normals(normals):
    """ptmi_check_vertex_normals: raises PtmiError for a table ptmi_set_vertex_normals would reject on its own account (host
    only): no primitive, or a NaN or infinite component in corners 0 .. 2.  normals (n_prims, 4, 3)."""
    normals = _normal_table(normals)
    _check(lib().ptmi_check_vertex_normals(len(normals), normals.ctypes.data))


def classify_vertex_normals(types, stored, normals):
    """ptmi_host_classify_vertex_normals: (n_prims,) bool, True where a primitive is smooth - a corner normal that is read differs
    (==) from its stored normal (host only).  types (n_prims,), stored (n_prims, 3), normals (n_prims, 4, 3)."""
    normals = _normal_table(normals)
    types = np.ascontiguousarray(types, np.int32); stored = np.ascontiguousarray(stored, np.float32)
    if types.shape != (len(normals),) or stored.shape != (len(normals), 3):
        raise ValueError("types must be (n_prims,) and stored (n_prims, 3)")
    smooth = np.zeros(len(normals), np.int32); count = C.c_int()
    _check(lib().ptmi_host_classify_vertex_normals(len(normals), types.ctypes.data, stored.ctypes.data, normals.ctypes.data,
                                                   smooth.ctypes.data, C.byref(count)))
    assert count.value == int(smooth.sum())
    return smooth.astype(bool)


TEXTURE_FILTERS = {"nearest": 0, "bilinear": 1}


def _albedo_args(image, uv, textured, filter):
    """(width, height, texels, filter, n_prims, uv, textured or None) as the C entries take them"""
    image = np.ascontiguousarray(image, np.float32)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("the image must be (height, width, 3)")
    uv = np.ascontiguousarray(uv, np.float32)
    if uv.ndim != 3 or uv.shape[1:] != (4, 2):
        raise ValueError("uv must be (n_prims, 4, 2)")
    if textured is not None:
        textured = np.ascontiguousarray(np.asarray(textured) != 0, np.int32)
        if textured.shape != (len(uv),):
            raise ValueError("textured must be (n_prims,)")
    if isinstance(filter, str):
        if filter not in TEXTURE_FILTERS:
            raise ValueError("filter must be 'nearest' or 'bilinear'")
        filter = TEXTURE_FILTERS[filter]
    return image.shape[1], image.shape[0], image, int(filter), len(uv), uv, textured


def check_albedo_texture(image, uv, textured=None, filter="bilinear"):
    """ptmi_check_albedo_texture: raises PtmiError for what ptmi_set_albedo_texture would reject on its own account (host only):
    a side outside 1 .. 4096, a filter other than nearest (0) / bilinear (1), a texel that is not finite or is negative, a UV of
    corners 0 .. 2 of a textured primitive that is not finite or exceeds 65536 in magnitude.  image (h, w, 3), uv (n_prims, 4, 2)."""
    w, h, image, filter, n, uv, textured = _albedo_args(image, uv, textured, filter)
    _check(lib().ptmi_check_albedo_texture(w, h, image.ctypes.data, filter, n, uv.ctypes.data, _ptr(textured)))


def check_feature_shading(flags):
    """ptmi_check_feature_shading: raises PtmiError for flags outside 0 .. 3 (host only)"""
    _check(lib().ptmi_check_feature_shading(int(flags)))


class Renderer:
    """One ApplicationState bound to one GPU."""

    def __init__(self, device_id=0):
        self.L = lib()
        self.h = C.c_void_p()
        self._ck(self.L.ptmi_ctx_create(int(device_id), C.byref(self.h)))
        self.width = self.height = 0
        self.config = default_config()
        self._camera = default_camera()              # what set_lens(radius) takes its default focus distance from

    def _ck(self, rc):
        if rc != 0:
            raise PtmiError(rc, self.L.ptmi_last_error().decode(errors="replace"))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.ptmi_ctx_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- SceneState::loadScene ---
    def load_scene(self, filename, subdivision_count=0, convert_quads=False):
        self._ck(self.L.ptmi_load_scene(self.h, os.fsencode(filename), int(subdivision_count), int(bool(convert_quads))))

    def load_scene_arrays(self, types, verts, normal, bsdf, Le):
        types = np.ascontiguousarray(types, np.int32)
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 4, 3)
        normal, bsdf, Le = (np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (normal, bsdf, Le))
        assert len(verts) == len(types) == len(normal) == len(bsdf) == len(Le)
        self._ck(self.L.ptmi_load_scene_arrays(self.h, len(types), types.ctypes.data, verts.ctypes.data,
                                               normal.ctypes.data, bsdf.ctypes.data, Le.ctypes.data))

    def set_radiosity_grids(self, rgb):
        """rgb: (n_prims, 256, 3) float32 radiosity grids in load order, or None to drop the CDF records."""
        if rgb is None:
            self._ck(self.L.ptmi_set_radiosity_grids(self.h, 0, None)); return
        rgb = np.ascontiguousarray(rgb, np.float32)
        assert rgb.ndim == 3 and rgb.shape[1:] == (256, 3)
        self._ck(self.L.ptmi_set_radiosity_grids(self.h, rgb.shape[0], rgb.ctypes.data))

    def set_radiosity(self, rgb):
        """rgb: (n_prims, 3) float32 per-primitive radiosity in load order, or None (zero)."""
        if rgb is None:
            self._ck(self.L.ptmi_set_radiosity(self.h, 0, None)); return
        rgb = np.ascontiguousarray(rgb, np.float32)
        assert rgb.ndim == 2 and rgb.shape[1] == 3
        self._ck(self.L.ptmi_set_radiosity(self.h, rgb.shape[0], rgb.ctypes.data))

    def apply_grid_filter(self, use_bilateral=True, sigma_spatial=1.5, sigma_range=0.3):
        """"Apply Filter & Rebuild CDFs" (ui_windows.h:154-167); returns the (formfactor, radiosity) filtered pdfs"""
        self._ck(self.L.ptmi_apply_grid_filter(self.h, int(use_bilateral), sigma_spatial, sigma_range))
        n = self.scene_info()["n_prims"]
        ff = np.zeros((n, 256), np.float32); rad = np.zeros((n, 256), np.float32)
        self._ck(self.L.ptmi_get_filtered_pdfs(self.h, ff.ctypes.data, rad.ctypes.data))
        return ff, rad

    def use_raw_cdfs(self):
        self._ck(self.L.ptmi_use_raw_cdfs(self.h))

    def run_radiosity_solver(self, **params):
        """RadiosityState::runSolver + precomputeCDFs + primitive upload (ui_windows.h:185-192).  Keyword arguments are
        the fields of ptmi_radiosity_params; defaults are the reference's."""
        prm = RadiosityParams()
        self.L.ptmi_default_radiosity_params(C.byref(prm))
        for k, v in params.items():
            if k not in dict(RadiosityParams._fields_):
                raise TypeError(f"unknown radiosity parameter {k}")
            setattr(prm, k, type(getattr(prm, k))(v))
        st = RadiosityStats()
        self._ck(self.L.ptmi_run_radiosity_solver(self.h, C.byref(prm), C.byref(st)))
        return st

    def radiosity_solution(self, form_factors=True):
        n = self.scene_info()["n_prims"]
        out = dict(radiosity=np.zeros((n, 3), np.float32), unshot=np.zeros((n, 3), np.float32),
                   grid=np.zeros((n, 256), np.float32), radiosity_grid=np.zeros((n, 256, 3), np.float32))
        if form_factors:
            out["form_factors"] = np.zeros((n, n), np.float32)
        self._ck(self.L.ptmi_get_radiosity_solution(self.h, out["form_factors"].ctypes.data if form_factors else None,
                                                    out["radiosity"].ctypes.data, out["unshot"].ctypes.data,
                                                    out["grid"].ctypes.data, out["radiosity_grid"].ctypes.data))
        return out

    def precomputed_cdfs(self):
        out = np.zeros((self.scene_info()["n_prims"], 530), np.float32)
        self._ck(self.L.ptmi_get_precomputed_cdfs(self.h, out.ctypes.data))
        return out

    def scene_info(self):
        v = [C.c_int() for _ in range(5)]
        self._ck(self.L.ptmi_scene_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("n_prims", "n_tris", "n_quads", "n_bvh_nodes", "bvh_depth"), (x.value for x in v)))

    def scene_prims(self):
        n = self.scene_info()["n_prims"]
        t = np.zeros(n, np.int32); v = np.zeros((n, 4, 3), np.float32)
        nr = np.zeros((n, 3), np.float32); b = np.zeros((n, 3), np.float32); le = np.zeros((n, 3), np.float32)
        self._ck(self.L.ptmi_scene_get_prims(self.h, t.ctypes.data, v.ctypes.data, nr.ctypes.data, b.ctypes.data, le.ctypes.data))
        return dict(type=t, verts=v, normal=nr, bsdf=b, Le=le)

    def scene_bvh(self):
        info = self.scene_info(); n, m = info["n_bvh_nodes"], info["n_prims"]
        bmin = np.zeros((n, 3), np.float32); bmax = np.zeros((n, 3), np.float32)
        left = np.zeros(n, np.int32); right = np.zeros(n, np.int32); count = np.zeros(n, np.int32); idx = np.zeros(m, np.int32)
        self._ck(self.L.ptmi_scene_get_bvh(self.h, bmin.ctypes.data, bmax.ctypes.data, left.ctypes.data, right.ctypes.data,
                                           count.ctypes.data, idx.ctypes.data))
        return dict(bmin=bmin, bmax=bmax, left=left, right=right, count=count, indices=idx)

    # --- RenderState::updateResolution / allocateBuffers ---
    def update_resolution(self, width, height, n_ranks=1, rank=0, row_block=8):
        t = Tiling(int(n_ranks), int(rank), int(row_block))
        self._ck(self.L.ptmi_update_resolution(self.h, int(width), int(height), C.byref(t)))
        self.width, self.height = int(width), int(height)

    def set_camera(self, cam):
        self._ck(self.L.ptmi_set_camera(self.h, C.byref(cam)))
        self._camera = Camera.from_buffer_copy(cam)

    def set_config(self, spp=None, max_depth=None, seed_base=None, segments_per_launch=None, collect_stats=None, wave_tiles=None, streams=None,
                   sampling_mode=None, mis_bsdf_fraction=None, integrator=None, download_image=None, fast_tree=None, next_event=None):
        c = self.config
        if spp is not None: c.spp = int(spp)
        if max_depth is not None: c.max_depth = int(max_depth)
        if seed_base is not None: c.seed_base = int(seed_base)
        if segments_per_launch is not None: c.segments_per_launch = int(segments_per_launch)
        if collect_stats is not None: c.collect_stats = int(bool(collect_stats))
        if wave_tiles is not None: c.wave_tiles = int(bool(wave_tiles))
        if streams is not None: c.streams = int(streams)
        if sampling_mode is not None: c.sampling_mode = int(sampling_mode)
        if mis_bsdf_fraction is not None: c.mis_bsdf_fraction = float(mis_bsdf_fraction)
        if integrator is not None: c.integrator = int(integrator)
        if download_image is not None: c.download_image = int(bool(download_image))
        if fast_tree is not None: c.fast_tree = int(bool(fast_tree))
        if next_event is not None: c.next_event = int(bool(next_event))
        self._ck(self.L.ptmi_set_config(self.h, C.byref(c)))

    def set_environment(self, rgb, **params):
        """The context's environment light: rgb (height, width, 3) float32, row 0 at +y, or None to drop it; keywords scale,
        rotation_deg, select_fraction (include/ptmi.h: ptmi_env_params).  It stays through scene loads."""
        if rgb is None:
            self._ck(self.L.ptmi_set_environment(self.h, 0, 0, None, None))
            return
        rgb = _env_map(rgb)
        p = default_env_params(**params)
        self._ck(self.L.ptmi_set_environment(self.h, rgb.shape[1], rgb.shape[0], rgb.ctypes.data, C.byref(p)))

    def environment_info(self):
        w, h, t = C.c_int(), C.c_int(), C.c_float()
        self._ck(self.L.ptmi_environment_info(self.h, C.byref(w), C.byref(h), C.byref(t)))
        return dict(width=w.value, height=h.value, total=np.float32(t.value))

    host_env_table = staticmethod(host_env_table)

    def set_surfaces(self, kind, ior=None, roughness=None):
        """Mirror and glass (include/ptmi.h: "specular surfaces"): kind (n_prims,) of SURFACE_DIFFUSE / _MIRROR / _GLASS in load
        order, or None to drop the table; ior a scalar or (n_prims,), None: 1.5 everywhere.  A scene load drops the table.
        Rough metal ("rough metal"): with a roughness, a scalar or (n_prims,) in [0.05, 1], the call goes to
        ptmi_set_surfaces_rough and kind may hold SURFACE_ROUGH; without one SURFACE_ROUGH is rejected."""
        if kind is None:
            self._ck(self.L.ptmi_set_surfaces(self.h, 0, None, None))
            return
        if roughness is None:
            kind, ior = _surface_table(kind, ior)
            self._ck(self.L.ptmi_set_surfaces(self.h, len(kind), kind.ctypes.data, _ptr(ior)))
            return
        kind, ior, roughness = _surface_table(kind, ior, roughness)
        self._ck(self.L.ptmi_set_surfaces_rough(self.h, len(kind), kind.ctypes.data, _ptr(ior), roughness.ctypes.data))

    def surface_counts(self):
        """ptmi_surface_counts: the table's primitives of kind 0 .. 3, all 0 without a table"""
        c = np.zeros(4, np.int32)
        self._ck(self.L.ptmi_surface_counts(self.h, c.ctypes.data))
        return [int(v) for v in c]

    def surfaces_info(self):
        m, g = C.c_int(), C.c_int()
        self._ck(self.L.ptmi_surfaces_info(self.h, C.byref(m), C.byref(g)))
        return dict(n_mirror=m.value, n_glass=g.value)

    def set_vertex_normals(self, normals):
        """Smooth shading (include/ptmi.h: "vertex normals"): normals (n_prims, 4, 3), a primitive's corner normals in load order
        and in the corner order of its vertices (a triangle's 4th is ignored), or None to drop the table.  A primitive whose
        corner normals all equal its stored normal stays flat.  A scene load drops the table."""
        if normals is None:
            self._ck(self.L.ptmi_set_vertex_normals(self.h, 0, None))
            return
        normals = _normal_table(normals)
        self._ck(self.L.ptmi_set_vertex_normals(self.h, len(normals), normals.ctypes.data))

    def vertex_normals_info(self):
        """ptmi_vertex_normals_info: the number of smooth primitives, 0 without a table"""
        n = C.c_int()
        self._ck(self.L.ptmi_vertex_normals_info(self.h, C.byref(n)))
        return dict(n_smooth=n.value)

    check_vertex_normals = staticmethod(check_vertex_normals)

    def debug_vertex_normal(self, prim, p):
        """ptmi_debug_vertex_normal: the kernel's shading normal of load-order primitives prim (n,) at the points p (n, 3) on the
        loaded scene and table.  Returns (n, 4) float32: N, then 1.0 where it was interpolated and 0.0 where the vertex keeps
        the stored normal."""
        prim = np.ascontiguousarray(prim, np.int32); p = np.ascontiguousarray(p, np.float32)
        if prim.ndim != 1 or p.shape != (len(prim), 3):
            raise ValueError("prim must be (n,) and p (n, 3)")
        out = np.zeros((len(prim), 4), np.float32)
        self._ck(self.L.ptmi_debug_vertex_normal(self.h, len(prim), prim.ctypes.data, p.ctypes.data, out.ctypes.data))
        return out

    def set_albedo_texture(self, image, uv, textured=None, filter="bilinear"):
        """Albedo texture (include/ptmi.h: "albedo texture"): image (h, w, 3) linear RGB, row 0 at v = 0; uv (n_prims, 4, 2), a
        primitive's corner UVs in load order and in the corner order of its vertices (a triangle's 4th is ignored); textured
        (n_prims,) marks the primitives the image applies to (None: all); filter "nearest" or "bilinear".  image None drops the
        texture.  Kd is multiplied by the image's value at every path vertex on a textured primitive.  A scene load drops it."""
        if image is None:
            self._ck(self.L.ptmi_set_albedo_texture(self.h, 0, 0, None, 0, 0, None, None))
            return
        w, h, image, filter, n, uv, textured = _albedo_args(image, uv, textured, filter)
        self._ck(self.L.ptmi_set_albedo_texture(self.h, w, h, image.ctypes.data, filter, n, uv.ctypes.data, _ptr(textured)))

    def albedo_texture_info(self):
        """ptmi_albedo_texture_info: the number of textured primitives, the image's size and filter; all 0 without a texture"""
        n, w, h, f = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._ck(self.L.ptmi_albedo_texture_info(self.h, C.byref(n), C.byref(w), C.byref(h), C.byref(f)))
        return dict(n_textured=n.value, width=w.value, height=h.value, filter=f.value)

    check_albedo_texture = staticmethod(check_albedo_texture)

    def debug_albedo(self, prim, p):
        """ptmi_debug_albedo: the kernel's lookup for load-order primitives prim (n,) at the points p (n, 3) on the loaded scene
        and texture.  Returns (n, 6) float32: the wrapped (u, v), T, then 1.0 for a textured primitive; (0, 0, 1, 1, 1, 0) for an
        untextured one or without a texture."""
        prim = np.ascontiguousarray(prim, np.int32); p = np.ascontiguousarray(p, np.float32)
        if prim.ndim != 1 or p.shape != (len(prim), 3):
            raise ValueError("prim must be (n,) and p (n, 3)")
        out = np.zeros((len(prim), 6), np.float32)
        self._ck(self.L.ptmi_debug_albedo(self.h, len(prim), prim.ctypes.data, p.ctypes.data, out.ctypes.data))
        return out

    def set_feature_shading(self, albedo=False, normal=False, flags=None):
        """Shaded features (include/ptmi.h: "shaded features"): albedo - the feature albedo is Kd x the albedo texture's value at
        the hit; normal - the feature normal is the interpolated vertex normal there.  A switch whose table is not set has no
        effect.  The context's, kept over scene loads.  A new value invalidates features and variance and empties the temporal
        history; the image and a running accumulation stay.  flags: the PTMI_FEATURE_* bits as an int, instead of the two."""
        if flags is None:
            flags = (FEATURE_TEXTURED_ALBEDO if albedo else 0) | (FEATURE_SHADING_NORMAL if normal else 0)
        self._ck(self.L.ptmi_set_feature_shading(self.h, int(flags)))

    def feature_shading(self):
        """ptmi_feature_shading: dict(albedo, normal, flags) of the context"""
        f = C.c_int()
        self._ck(self.L.ptmi_feature_shading(self.h, C.byref(f)))
        return dict(albedo=bool(f.value & FEATURE_TEXTURED_ALBEDO), normal=bool(f.value & FEATURE_SHADING_NORMAL), flags=f.value)

    check_feature_shading = staticmethod(check_feature_shading)

    # --- thin lens (include/ptmi.h: "thin lens") ---
    def set_lens(self, radius, focus_distance=None):
        """ptmi_set_lens: a thin lens of this radius focused at focus_distance along the optical axis, in scene units.  radius 0 is
        the pinhole.  focus_distance None: |origin - lookat| of the camera as it is now (with radius 0: "no lens", and the focus
        distance follows the camera again).  The context's, kept over scene loads, resolutions and cameras; the feature pass and the
        Radiosity view keep the pinhole.  Changed values restart an accumulation and make the features stale, as set_camera does."""
        if focus_distance is None:
            focus_distance = 0.0 if float(radius) == 0.0 else default_focus_distance(self._camera)
        self._ck(self.L.ptmi_set_lens(self.h, float(radius), float(focus_distance)))

    def lens(self):
        """ptmi_lens: (radius, focus_distance) of the context; without a focus distance of its own, the camera's |origin - lookat|"""
        r, f = C.c_float(), C.c_float()
        self._ck(self.L.ptmi_lens(self.h, C.byref(r), C.byref(f)))
        return r.value, f.value

    def focus_distance_at(self, px, py):
        """The focus distance that brings what pixel (px, py) shows into focus: the first hit of the pinhole ray through the
        pixel's centre (ptmi_debug_first_hit), as a depth along the optical axis, t * dot(d, axis) in binary64.  Raises
        ValueError where the ray hits nothing."""
        if not (0 <= int(px) < self.width and 0 <= int(py) < self.height):
            raise ValueError("pixel (%d, %d) is outside the %d x %d image" % (px, py, self.width, self.height))
        frame = self.camera_frame()
        o, d = pinhole_centre_ray(frame, self.width, self.height, int(px), int(py))
        h = self.debug_first_hit(o[None], d[None])
        if not h["hit"][0]:
            raise ValueError("pixel (%d, %d) shows nothing to focus on" % (px, py))
        return depth_along_axis(frame, d, h["t"][0])

    def debug_lens_block(self):
        """ptmi_debug_lens_block: the context's lens block as the device holds it after deriving it for the camera, resolution and
        lens as they are now, (6, 4) float32"""
        out = np.zeros((6, 4), np.float32)
        self._ck(self.L.ptmi_debug_lens_block(self.h, out.ctypes.data))
        return out

    def debug_lens_ray(self, px, py, r):
        """ptmi_debug_lens_ray: the kernel's lens ray for pixels (px, py) (n,) and the uniforms r (n, 4) = r3 r4 r1 r2 over the
        context's block.  Returns (n, 6) float32: the origin on the lens, then the unit direction."""
        px = np.ascontiguousarray(px, np.int32); py = np.ascontiguousarray(py, np.int32); r = np.ascontiguousarray(r, np.float32)
        if px.ndim != 1 or py.shape != px.shape or r.shape != (len(px), 4):
            raise ValueError("px and py must be (n,) and r (n, 4)")
        out = np.zeros((len(px), 6), np.float32)
        self._ck(self.L.ptmi_debug_lens_ray(self.h, len(px), px.ctypes.data, py.ctypes.data, r.ctypes.data, out.ctypes.data))
        return out

    # --- participating medium (include/ptmi.h: "participating medium") ---
    def set_medium(self, lo, hi=None, sigma_t=0.0, albedo=(1.0, 1.0, 1.0), g=0.0):
        """ptmi_set_medium: a homogeneous medium of extinction sigma_t per scene unit inside the box [lo, hi] (scene coordinates),
        with a single-scattering albedo (a scalar or r, g, b) and the Henyey-Greenstein asymmetry g.  set_medium(None), or sigma_t
        0, drops it.  lo may also be a Medium.  The scene's: a scene load drops it.  The feature pass, the Radiosity view and the
        solver ignore it; a changed medium restarts an accumulation."""
        if lo is None:
            self._ck(self.L.ptmi_set_medium(self.h, None))
            return
        m = lo if isinstance(lo, Medium) else make_medium(lo, hi, sigma_t, albedo, g)
        self._ck(self.L.ptmi_set_medium(self.h, C.byref(m)))

    def medium(self):
        """ptmi_medium_info: the scene's Medium, or None without one"""
        m, on = Medium(), C.c_int()
        self._ck(self.L.ptmi_medium_info(self.h, C.byref(m), C.byref(on)))
        return m if on.value else None

    def debug_medium_call(self, op, inputs):
        """ptmi_debug_medium_call: op (MEDIUM_*) of the kernel's medium functions on the cases inputs (n, MEDIUM_CALL_IN) float32 -
        the block, o, d, t_end, u.  Returns (n, MEDIUM_CALL_OUT) float32."""
        a = np.ascontiguousarray(inputs, np.float32)
        if a.ndim != 2 or a.shape[1] != MEDIUM_CALL_IN:
            raise ValueError("inputs must be (n, %d)" % MEDIUM_CALL_IN)
        out = np.zeros((len(a), MEDIUM_CALL_OUT), np.float32)
        self._ck(self.L.ptmi_debug_medium_call(self.h, int(op), len(a), a.ctypes.data, out.ctypes.data))
        return out

    def camera_frame(self):
        out = np.zeros(12, np.float32)
        self._ck(self.L.ptmi_get_camera_frame(self.h, out.ctypes.data)); return out

    def local_rows(self):
        n = C.c_int(); self._ck(self.L.ptmi_local_rows(self.h, C.byref(n)))
        rows = np.zeros(n.value, np.int32)
        if n.value: self._ck(self.L.ptmi_local_row_map(self.h, rows.ctypes.data))
        return rows

    # --- renderFrame ---
    def render_frame(self, want_stats=True):
        st = Stats()
        self._ck(self.L.ptmi_render_frame(self.h, C.byref(st) if want_stats else None))
        return st

    def render_frames(self, n_frames, want_stats=True):
        """n_frames successive frames as one pipelined run (ptmi_render_frames); the image buffers then hold the last one."""
        st = Stats()
        self._ck(self.L.ptmi_render_frames(self.h, int(n_frames), C.byref(st) if want_stats else None))
        return st

    def select_frame(self, frame):
        self._ck(self.L.ptmi_select_frame(self.h, int(frame)))

    # --- progressive / adaptive accumulation (include/ptmi.h: ptmi_accum_pass) ---
    def accum_reset(self):
        self._ck(self.L.ptmi_accum_reset(self.h))

    def accum_pass(self, params=None):
        """One pass: config.spp more samples for every pixel still active, the stopping test (params: an AdaptiveParams or a
        dict of its fields; None = plain progressive, nothing stops) and the resolve by each pixel's own count.  Returns
        PassStats (the pass number is its `pass_` field)."""
        if isinstance(params, dict):
            params = default_adaptive_params(**params)
        st = PassStats()
        self._ck(self.L.ptmi_accum_pass(self.h, C.byref(params) if params is not None else None, C.byref(st)))
        return st

    def render_adaptive(self, **params):
        """A fresh accumulation run to its end: with keyword parameters (fields of AdaptiveParams over the defaults) passes
        until no pixel is active; without, max_passes plain progressive passes.  Returns the list of PassStats."""
        self.accum_reset()
        prm = default_adaptive_params(**params)
        out = []
        if not params:
            for _ in range(prm.max_passes):
                out.append(self.accum_pass(None))
            return out
        while True:
            out.append(self.accum_pass(prm))
            if out[-1].active_after == 0:
                return out

    def sample_counts(self):
        """Samples per local pixel of the current accumulation, (local rows, width) uint32, rows as read_image returns them."""
        counts = np.zeros((len(self.local_rows()), self.width), np.uint32)
        self._ck(self.L.ptmi_read_sample_counts(self.h, counts.ctypes.data))
        return counts

    # --- feature buffers and the denoiser (include/ptmi.h: ptmi_render_features, ptmi_denoise) ---
    def render_features(self, grid=2):
        self._ck(self.L.ptmi_render_features(self.h, int(grid)))

    def debug_set_filter_inputs(self, radiance, feat, grid=2):
        """ptmi_debug_set_filter_inputs: radiance (local rows, width, 3) and the feature dict of features() become the context's
        image and features, as a finished frame plus a finished feature pass of `grid` would leave them.  Non-finite values
        are passed on as they are."""
        n = len(self.local_rows())
        arrs = [np.ascontiguousarray(radiance, np.float32)] + [np.ascontiguousarray(feat[k], np.float32) for k in ("albedo", "normal", "position")]
        hf = np.ascontiguousarray(feat["hit_fraction"], np.float32)
        if any(a.shape != (n, self.width, 3) for a in arrs) or hf.shape != (n, self.width):
            raise ValueError("radiance, albedo, normal, position must be (%d, %d, 3) and hit_fraction (%d, %d)" % (n, self.width, n, self.width))
        self._ck(self.L.ptmi_debug_set_filter_inputs(self.h, *[a.ctypes.data for a in arrs], hf.ctypes.data, int(grid)))

    def debug_accum_step(self, sums, prev, m2, passes, queue=None, n_queue=None, params=None, first=False):
        """ptmi_debug_accum_step: one stopping test plus resolve on state given BY SLOT - sums (n, 3), prev (n, 4: S_{k-1}.xyz and
        the mean), m2 (n) float32, passes (n) uint32, n = local rows x width; queue: int32 slots (None: the slots 0 .. n_queue - 1,
        n_queue None: all); params: an AdaptiveParams, a dict of its fields or None (progressive).  Returns the next pass's queue."""
        n = len(self.local_rows()) * self.width
        sums = np.ascontiguousarray(sums, np.float32); prev = np.ascontiguousarray(prev, np.float32)
        m2 = np.ascontiguousarray(m2, np.float32); passes = np.ascontiguousarray(passes, np.uint32)
        if sums.shape != (n, 3) or prev.shape != (n, 4) or m2.shape != (n,) or passes.shape != (n,):
            raise ValueError("sums must be (%d, 3), prev (%d, 4), m2 and passes (%d,)" % (n, n, n))
        if queue is not None:
            queue = np.ascontiguousarray(queue, np.int32)
            if queue.ndim != 1 or (n_queue is not None and n_queue != len(queue)):
                raise ValueError("queue must be one-dimensional and n_queue its length")
            n_queue = len(queue)
        elif n_queue is None:
            n_queue = n
        if isinstance(params, dict):
            params = default_adaptive_params(**params)
        out = np.full(max(int(n_queue), 1), -1, np.int32); n_out = C.c_int(-1)
        self._ck(self.L.ptmi_debug_accum_step(self.h, sums.ctypes.data, prev.ctypes.data, m2.ctypes.data, passes.ctypes.data,
                                              queue.ctypes.data if queue is not None else None, int(n_queue),
                                              C.byref(params) if params is not None else None, int(bool(first)), out.ctypes.data, C.byref(n_out)))
        return out[:n_out.value].copy()

    def debug_order_by_cost(self, n, cost, cost_max, classes, queue_in=None):
        """ptmi_debug_order_by_cost: (queue_out (n) int32, hist (512) int32) of the launch order by cost for cost (uint32 per
        entry), cost_max and classes over queue_in (int32, None: 0 .. n - 1)."""
        cost = np.ascontiguousarray(cost, np.uint32)
        if queue_in is not None:
            queue_in = np.ascontiguousarray(queue_in, np.int32)
            if queue_in.shape != (n,):
                raise ValueError("queue_in must hold n entries")
        out = np.full(max(int(n), 1), -2, np.int32); hist = np.full(512, -2, np.int32)
        self._ck(self.L.ptmi_debug_order_by_cost(self.h, int(n), queue_in.ctypes.data if queue_in is not None else None, cost.ctypes.data,
                                                 int(cost.size), int(cost_max), int(classes), out.ctypes.data, hist.ctypes.data))
        return out[:n], hist

    def debug_cdf_records(self, src_kind, src):
        """ptmi_debug_cdf_records: the (n, 530) records of n grids; src (n, 256, 4 | 3) for src_kind 0 | 1, (n, 256) for 2."""
        src = np.ascontiguousarray(src, np.float32)
        want = {0: (256, 4), 1: (256, 3), 2: (256,)}.get(int(src_kind))
        if want is not None and src.shape[1:] != want:
            raise ValueError(f"src_kind {src_kind} takes grids of shape (n,) + {want}")
        out = np.zeros((len(src), 530), np.float32)
        self._ck(self.L.ptmi_debug_cdf_records(self.h, len(src), int(src_kind), src.ctypes.data, out.ctypes.data))
        return out

    def debug_filter_pdfs(self, rgb, counts=None, use_bilateral=True, sigma_spatial=1.5, sigma_range=0.3):
        """ptmi_debug_filter_pdfs: (formfactor, radiosity) pdfs, (n, 256) each, of rgb (n, 256, 3) and counts (n, 256) or None."""
        rgb = np.ascontiguousarray(rgb, np.float32)
        if rgb.ndim != 3 or rgb.shape[1:] != (256, 3):
            raise ValueError("rgb must be (n, 256, 3)")
        if counts is not None:
            counts = np.ascontiguousarray(counts, np.float32)
            if counts.shape != rgb.shape[:2]:
                raise ValueError("counts must be (n, 256)")
        ff = np.zeros(rgb.shape[:2], np.float32); rad = np.zeros(rgb.shape[:2], np.float32)
        self._ck(self.L.ptmi_debug_filter_pdfs(self.h, len(rgb), rgb.ctypes.data, counts.ctypes.data if counts is not None else None,
                                               int(bool(use_bilateral)), sigma_spatial, sigma_range, ff.ctypes.data, rad.ctypes.data))
        return ff, rad

    def debug_radiosity_grid(self, centre, normal, form_factors, radiosity, enable_filtering=False, use_bilateral=True,
                             sigma_spatial=1.5, sigma_range=0.3):
        """ptmi_debug_radiosity_grid: the (n, 256, 3) radiosity grids of a world of n primitives given by centre, normal (n, 3),
        form_factors (n, n) and radiosity (n, 3)."""
        centre, normal, radiosity = (np.ascontiguousarray(a, np.float32) for a in (centre, normal, radiosity))
        form_factors = np.ascontiguousarray(form_factors, np.float32)
        n = len(centre)
        if centre.shape != (n, 3) or normal.shape != (n, 3) or radiosity.shape != (n, 3) or form_factors.shape != (n, n):
            raise ValueError("centre, normal, radiosity must be (n, 3) and form_factors (n, n)")
        out = np.zeros((n, 256, 3), np.float32)
        self._ck(self.L.ptmi_debug_radiosity_grid(self.h, n, centre.ctypes.data, normal.ctypes.data, form_factors.ctypes.data,
                                                  radiosity.ctypes.data, int(bool(enable_filtering)), int(bool(use_bilateral)),
                                                  sigma_spatial, sigma_range, out.ctypes.data))
        return out

    def features(self):
        """The current feature buffers: albedo, normal, position (local rows, width, 3) and hit_fraction (local rows, width),
        float32, rows as read_image returns them."""
        n = len(self.local_rows())
        out = dict(albedo=np.zeros((n, self.width, 3), np.float32), normal=np.zeros((n, self.width, 3), np.float32),
                   position=np.zeros((n, self.width, 3), np.float32), hit_fraction=np.zeros((n, self.width), np.float32))
        self._ck(self.L.ptmi_read_features(self.h, out["albedo"].ctypes.data, out["normal"].ctypes.data, out["position"].ctypes.data,
                                           out["hit_fraction"].ctypes.data))
        return out

    def denoise(self, **params):
        """Denoises the image read_image returns (keyword parameters: fields of DenoiseParams over the defaults); returns the
        result as (rgb8, radiance), shaped like read_image's."""
        p = default_denoise_params(**params)
        self._ck(self.L.ptmi_denoise(self.h, C.byref(p)))
        return self.read_denoised()

    def read_denoised(self):
        n = len(self.local_rows())
        rgb = np.zeros((n, self.width, 3), np.uint8); rad = np.zeros((n, self.width, 3), np.float32)
        self._ck(self.L.ptmi_read_denoised(self.h, rgb.ctypes.data, rad.ctypes.data))
        return rgb, rad

    def denoise_timing(self):
        """(ms of the last feature pass, ms of the last filter run), device time"""
        a = C.c_double(); b = C.c_double()
        self._ck(self.L.ptmi_denoise_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # --- the variance-guided filter (include/ptmi.h: ptmi_denoise_variance) ---
    def denoise_variance(self, **params):
        """The variance-guided a-trous filter over the image read_image returns (keyword parameters: fields of VarianceParams
        over the defaults); returns (rgb8, radiance) like denoise."""
        p = default_variance_params(**params)
        self._ck(self.L.ptmi_denoise_variance(self.h, C.byref(p)))
        return self.read_denoised()

    def variance(self):
        """(variance_in, variance_out) of the last denoise_variance, (local rows, width) float32 each."""
        n = len(self.local_rows())
        vin = np.zeros((n, self.width), np.float32); vout = np.zeros((n, self.width), np.float32)
        self._ck(self.L.ptmi_read_variance(self.h, vin.ctypes.data, vout.ctypes.data))
        return vin, vout

    def variance_timing(self):
        """(ms of the last variance estimate, ms of the last variance-guided filter run), device time"""
        a = C.c_double(); b = C.c_double()
        self._ck(self.L.ptmi_variance_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def pass_moments(self):
        """The stopping test's state of the current accumulation: (mean, M2, passes), (local rows, width) float32, float32,
        uint32."""
        n = len(self.local_rows())
        mean = np.zeros((n, self.width), np.float32); m2 = np.zeros((n, self.width), np.float32)
        passes = np.zeros((n, self.width), np.uint32)
        self._ck(self.L.ptmi_read_pass_moments(self.h, mean.ctypes.data, m2.ctypes.data, passes.ctypes.data))
        return mean, m2, passes

    # --- temporal accumulation with reprojection (include/ptmi.h: ptmi_temporal_accumulate) ---
    def temporal_accumulate(self, **params):
        """Blends the image read_image returns into the history, reprojected from the history's view (keyword parameters:
        fields of TemporalParams over the defaults); returns (rgb8, radiance, TemporalStats), the images shaped like
        read_image's."""
        p = default_temporal_params(**params)
        st = TemporalStats()
        self._ck(self.L.ptmi_temporal_accumulate(self.h, C.byref(p), C.byref(st)))
        rgb, rad = self.read_temporal()
        return rgb, rad, st

    def temporal_reset(self):
        self._ck(self.L.ptmi_temporal_reset(self.h))

    def read_temporal(self):
        n = len(self.local_rows())
        rgb = np.zeros((n, self.width, 3), np.uint8); rad = np.zeros((n, self.width, 3), np.float32)
        self._ck(self.L.ptmi_read_temporal(self.h, rgb.ctypes.data, rad.ctypes.data))
        return rgb, rad

    def history_counts(self):
        """Samples behind each pixel's history, (local rows, width) float32 (0 while the history is empty)."""
        counts = np.zeros((len(self.local_rows()), self.width), np.float32)
        self._ck(self.L.ptmi_read_history_counts(self.h, counts.ctypes.data))
        return counts

    def denoise_temporal(self, **params):
        """The a-trous filter over the history's colour, guided by the history's features (keyword parameters: fields of
        DenoiseParams over the defaults); returns (rgb8, radiance) like denoise."""
        p = default_denoise_params(**params)
        self._ck(self.L.ptmi_denoise_temporal(self.h, C.byref(p)))
        return self.read_denoised()

    # --- the history's luminance statistics (include/ptmi.h: ptmi_set_temporal_moments) ---
    def set_temporal_moments(self, on):
        """ptmi_set_temporal_moments: the history carries (mean, variance, frames) of its luminance.  The context's, kept over
        scene loads; a new value empties the history."""
        self._ck(self.L.ptmi_set_temporal_moments(self.h, int(on)))

    def get_temporal_moments(self):
        on = C.c_int()
        self._ck(self.L.ptmi_get_temporal_moments(self.h, C.byref(on)))
        return on.value

    def temporal_moments(self):
        """(mean, variance, frames) of the history's luminance, (local rows, width) float32 each."""
        shape = (len(self.local_rows()), self.width)
        mean, var, frames = (np.zeros(shape, np.float32) for _ in range(3))
        self._ck(self.L.ptmi_read_temporal_moments(self.h, mean.ctypes.data, var.ctypes.data, frames.ctypes.data))
        return mean, var, frames

    def denoise_temporal_variance(self, **params):
        """The variance-guided a-trous filter over the history's colour, guided by the history's features and steered by the
        history's luminance variance (keyword parameters: fields of VarianceParams over the defaults); returns (rgb8, radiance)
        like denoise; variance() reads the variances."""
        p = default_variance_params(**params)
        self._ck(self.L.ptmi_denoise_temporal_variance(self.h, C.byref(p)))
        return self.read_denoised()

    def debug_set_temporal_moments(self, mean, variance, frames):
        """ptmi_debug_set_temporal_moments: (local rows, width) arrays become the history's (mean, variance, frames), unchecked."""
        shape = (len(self.local_rows()), self.width)
        arrs = [np.ascontiguousarray(a, np.float32) for a in (mean, variance, frames)]
        for a in arrs:
            if a.shape != shape:
                raise ValueError(f"expected arrays of shape {shape}")
        self._ck(self.L.ptmi_debug_set_temporal_moments(self.h, *[a.ctypes.data for a in arrs]))

    def device_image(self):
        a = C.c_void_p(); b = C.c_void_p()
        self._ck(self.L.ptmi_device_image(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def read_image(self, rgb8=True, radiance=True):
        n = len(self.local_rows())
        rgb = np.zeros((n, self.width, 3), np.uint8) if rgb8 else None
        rad = np.zeros((n, self.width, 3), np.float32) if radiance else None
        self._ck(self.L.ptmi_read_image(self.h, rgb.ctypes.data if rgb8 else None, rad.ctypes.data if radiance else None))
        return rgb, rad

    def copy_image_device(self, d_rgb8_ptr=None, d_radiance_ptr=None):
        """D2D copy of the local rows into caller-owned device buffers (raw pointers, e.g. tensor.data_ptr())."""
        self._ck(self.L.ptmi_copy_image_device(self.h, d_rgb8_ptr, d_radiance_ptr))

    def host_image(self):
        """RenderState::h_image: the pinned host copy of the local 8-bit rows that render_frame fills when download_image is set
        (a view, valid until the next update_resolution / close)."""
        p = C.c_void_p(); n = C.c_uint64()
        self._ck(self.L.ptmi_host_image(self.h, C.byref(p), C.byref(n)))
        buf = (C.c_ubyte * n.value).from_address(p.value)
        return np.frombuffer(buf, np.uint8).reshape(-1, self.width, 3)

    # --- multi-GPU frame exchange (RCCL behind the C ABI) ---
    GATHER_RGB8, GATHER_RADIANCE = 1, 2

    @staticmethod
    def dist_unique_id():
        """ncclGetUniqueId: 128 bytes to be shipped from one rank to all ranks (any channel)."""
        buf = C.create_string_buffer(128)
        _check(lib().ptmi_dist_unique_id(buf))
        return buf.raw

    def dist_init(self, unique_id, n_ranks, rank):
        assert len(unique_id) == 128
        self._ck(self.L.ptmi_dist_init(self.h, C.c_char_p(unique_id), int(n_ranks), int(rank)))

    def dist_finalize(self):
        self._ck(self.L.ptmi_dist_finalize(self.h))

    def gather_frame(self, dst_rank=0, what=3):
        """The one exchange step of a frame; only enqueues (see include/ptmi.h)."""
        self._ck(self.L.ptmi_gather_frame(self.h, int(dst_rank), int(what)))

    def gather_wait(self):
        self._ck(self.L.ptmi_gather_wait(self.h))

    def read_frame(self, rgb8=True, radiance=True):
        rgb = np.zeros((self.height, self.width, 3), np.uint8) if rgb8 else None
        rad = np.zeros((self.height, self.width, 3), np.float32) if radiance else None
        self._ck(self.L.ptmi_read_frame(self.h, rgb.ctypes.data if rgb8 else None, rad.ctypes.data if radiance else None))
        return rgb, rad

    def dist_comm_count(self):
        n = C.c_int(); self._ck(self.L.ptmi_dist_comm_count(self.h, C.byref(n))); return n.value

    def dist_barrier(self):
        self._ck(self.L.ptmi_dist_barrier(self.h))

    def dist_allreduce_max(self, value):
        v = C.c_double(float(value))
        self._ck(self.L.ptmi_dist_allreduce_max(self.h, C.byref(v)))
        return v.value

    def debug_place_tiles(self, width, height, n_ranks, row_block, tiles_rgb8=None, tiles_radiance=None):
        """dst-side row placement of the gather alone: tiles concatenated in rank order -> frame."""
        n = width * height * 3
        out_rgb = out_rad = None
        if tiles_rgb8 is not None:
            tiles_rgb8 = np.ascontiguousarray(tiles_rgb8, np.uint8).reshape(-1); assert tiles_rgb8.size == n
            out_rgb = np.zeros((height, width, 3), np.uint8)
        if tiles_radiance is not None:
            tiles_radiance = np.ascontiguousarray(tiles_radiance, np.float32).reshape(-1); assert tiles_radiance.size == n
            out_rad = np.zeros((height, width, 3), np.float32)
        self._ck(self.L.ptmi_debug_place_tiles(self.h, width, height, n_ranks, row_block,
                                               tiles_rgb8.ctypes.data if tiles_rgb8 is not None else None,
                                               tiles_radiance.ctypes.data if tiles_radiance is not None else None,
                                               out_rgb.ctypes.data if out_rgb is not None else None,
                                               out_rad.ctypes.data if out_rad is not None else None))
        return out_rgb, out_rad

    # --- test hooks ---
    SWEEP, LANE, STACK, PHASED, PACKED, WIDE, CERTIFIED = 0, 1, 2, 3, 4, 5, 6

    def set_traversal(self, force_mode=-1, sweep_max_prims=64):
        """Returns the traversal mode in effect for the loaded scene (-1 if none)."""
        m = C.c_int(-1)
        self._ck(self.L.ptmi_debug_set_traversal(self.h, int(force_mode), int(sweep_max_prims), C.byref(m)))
        return m.value

    def traversal(self):
        """The traversal mode in effect for the loaded scene (-1 if none); changes nothing."""
        m = C.c_int(-1)
        self._ck(self.L.ptmi_debug_get_traversal(self.h, C.byref(m)))
        return m.value

    def set_solver_walk(self, force_walk=-1, min_prims=256):
        """Visibility walk of the next radiosity solve: -1 automatic, 0 the reference's tree, 2 certified (identical form factors)."""
        self._ck(self.L.ptmi_debug_set_solver_walk(self.h, int(force_walk), int(min_prims)))

    def set_packed_min_nodes(self, min_nodes=8192):
        """Smallest tree (BVH nodes) that gets the packed layout of traversal mode PACKED; returns the record positions built."""
        n = C.c_int()
        self._ck(self.L.ptmi_debug_set_packed_min_nodes(self.h, int(min_nodes), C.byref(n)))
        return n.value

    def set_packed_top(self, top_records=512):
        """Record positions of the packed tree kept in LDS; returns (n_top, top_depth) built for the loaded scene."""
        a = C.c_int(); b = C.c_int()
        self._ck(self.L.ptmi_debug_set_packed_top(self.h, int(top_records), C.byref(a), C.byref(b)))
        return a.value, b.value

    def debug_rcp_check(self, first_bits, count):
        bad = C.c_uint64(); first = C.c_uint32()
        self._ck(self.L.ptmi_debug_rcp_check(self.h, int(first_bits), int(count), C.byref(bad), C.byref(first)))
        return bad.value, first.value

    def debug_sqrt_check(self, first_bits, count):
        bad = C.c_uint64(); first = C.c_uint32()
        self._ck(self.L.ptmi_debug_sqrt_check(self.h, int(first_bits), int(count), C.byref(bad), C.byref(first)))
        return bad.value, first.value

    def debug_ray_inv(self, d, live=None):
        """The walks' 1 / d of directions d (n, 3); every 64 consecutive cases vote as one wave, live[i] == 0 takes case i out of it."""
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        live = np.ones(len(d), np.int32) if live is None else np.ascontiguousarray(live, np.int32)
        out = np.zeros_like(d)
        self._ck(self.L.ptmi_debug_ray_inv(self.h, len(d), d.ctypes.data, live.ctypes.data, out.ctypes.data))
        return out

    def debug_sincos_lean_check(self, first_bits, count):
        """The cosine sample's voted sincos against ptmi_sincosf over a range of bit patterns: (patterns whose sin differs, whose
        cos differs, the first of them, lanes that raised the ambiguity flag, up to 8 flagged patterns)."""
        bs = C.c_uint64(); bc = C.c_uint64(); first = C.c_uint32(); fl = C.c_uint64(); n = C.c_int()
        kept = np.zeros(8, np.uint32)
        self._ck(self.L.ptmi_debug_sincos_lean_check(self.h, int(first_bits), int(count), C.byref(bs), C.byref(bc), C.byref(first),
                                                     C.byref(fl), kept.ctypes.data, C.byref(n)))
        return bs.value, bc.value, first.value, fl.value, kept[:n.value].copy()

    def _vote_hook(self, fn, x, per_in, per_out, live):
        x = np.ascontiguousarray(x, np.float32).reshape(-1, per_in)
        live = np.ones(len(x), np.int32) if live is None else np.ascontiguousarray(live, np.int32)
        out = np.zeros((len(x), per_out), np.float32)
        self._ck(fn(self.h, len(x), x.ctypes.data, live.ctypes.data, out.ctypes.data))
        return out

    def debug_sincos_lean(self, x, live=None):
        """The voted sincos of x (n,); every 64 consecutive cases vote as one wave, live[i] == 0 takes case i out of it.
        (n, 4): the voted sin and cos, then ptmi_sincosf's."""
        return self._vote_hook(self.L.ptmi_debug_sincos_lean, x, 1, 4, live)

    def debug_unit_voted(self, w, live=None):
        """The voted normalisation of w (n, 3), in waves as debug_sincos_lean.  (n, 6): the voted vector, then unit_vector's."""
        return self._vote_hook(self.L.ptmi_debug_unit_voted, w, 3, 6, live)

    def debug_size_div_check(self, size, first_bits, count):
        """The pixel jitter's a / size against the IEEE division over a range of bit patterns of a: (mismatches, the first, whether
        this size takes the short form)."""
        bad = C.c_uint64(); first = C.c_uint32(); lean = C.c_int()
        self._ck(self.L.ptmi_debug_size_div_check(self.h, int(size), int(first_bits), int(count), C.byref(bad), C.byref(first), C.byref(lean)))
        return bad.value, first.value, bool(lean.value)

    def debug_intersect(self, o, d, t_min=1e-4, t_max=3.4028234663852886e38):
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3); d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        n = len(o)
        hit = np.zeros(n, np.int32); prim = np.zeros(n, np.int32); t = np.zeros(n, np.float32)
        p = np.zeros((n, 3), np.float32); nr = np.zeros((n, 3), np.float32)
        self._ck(self.L.ptmi_debug_intersect(self.h, n, o.ctypes.data, d.ctypes.data, t_min, t_max, hit.ctypes.data,
                                             prim.ctypes.data, t.ctypes.data, p.ctypes.data, nr.ctypes.data))
        return dict(hit=hit, prim=prim, t=t, p=p, n=nr)

    def debug_set_fast_tree(self, max_leaf=3, c_trav=1.0, c_tri=1.0, top_nodes=80):
        n = C.c_int(); d = C.c_int(); t = C.c_int()
        self._ck(self.L.ptmi_debug_set_fast_tree(self.h, int(max_leaf), float(c_trav), float(c_tri), int(top_nodes), C.byref(n), C.byref(d), C.byref(t)))
        return dict(n_nodes=n.value, depth=d.value, n_top=t.value)

    def debug_intersect_fast(self, o, d, t_min=1e-4, t_max=3.4028234663852886e38):
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3); d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        n = len(o)
        hit = np.zeros(n, np.int32); prim = np.zeros(n, np.int32); t = np.zeros(n, np.float32); counts = np.zeros(2, np.uint64)
        self._ck(self.L.ptmi_debug_intersect_fast(self.h, n, o.ctypes.data, d.ctypes.data, t_min, t_max, hit.ctypes.data,
                                                  prim.ctypes.data, t.ctypes.data, counts.ctypes.data))
        return dict(hit=hit, prim=prim, t=t, node_visits=int(counts[0]), prim_tests=int(counts[1]))

    def debug_first_hit(self, o, d, t_min=1e-4):
        """first_hit of the Radiosity view and the feature pass for rays as given, by the walk the loaded scene takes there (the
        certified walk where it has one, else LANE or STACK); t_max is FLT_MAX.  prim: load index or -1."""
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3); d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        n = len(o)
        hit = np.zeros(n, np.int32); prim = np.zeros(n, np.int32); t = np.zeros(n, np.float32)
        self._ck(self.L.ptmi_debug_first_hit(self.h, n, o.ctypes.data, d.ctypes.data, t_min, hit.ctypes.data, prim.ctypes.data, t.ctypes.data))
        return dict(hit=hit, prim=prim, t=t)

    def debug_rng(self, seed_base, pixels, count):
        pixels = np.ascontiguousarray(pixels, np.int32)
        out = np.zeros((len(pixels), count), np.float32)
        self._ck(self.L.ptmi_debug_rng(self.h, int(seed_base), len(pixels), pixels.ctypes.data, int(count), out.ctypes.data))
        return out

    def debug_cosine_sample(self, normals, u, v):
        normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        u = np.ascontiguousarray(u, np.float32); v = np.ascontiguousarray(v, np.float32)
        out = np.zeros_like(normals)
        self._ck(self.L.ptmi_debug_cosine_sample(self.h, len(u), normals.ctypes.data, u.ctypes.data, v.ctypes.data, out.ctypes.data))
        return out

    GUIDED_COSINE, GUIDED_GRID_SAMPLE, GUIDED_GRID_PDF, GUIDED_MIS, GUIDED_MIS_WEIGHT, GUIDED_TONEMAP = range(6)

    def debug_guided_sample(self, op, normals, in3, states, recs=None, rec_idx=None):
        """ptmi_debug_guided_sample: the bounce kernels' guided-sampling functions on n cases.  normals, in3: (n, 3); states:
        (n, 6) uint32 XORWOW states; recs: (m, 530) float32 CDF records and rec_idx: (n,) for the grid ops.
        Returns out (n, 6) float32 and used (n,) int32, the draws each call made."""
        normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3); n = len(normals)
        in3 = np.ascontiguousarray(in3, np.float32).reshape(n, 3)
        states = np.ascontiguousarray(states, np.uint32).reshape(n, 6)
        out = np.zeros((n, 6), np.float32); used = np.zeros(n, np.int32)
        if recs is not None:
            recs = np.ascontiguousarray(recs, np.float32).reshape(-1, 530)
            rec_idx = np.ascontiguousarray(rec_idx, np.int32).reshape(n)
        self._ck(self.L.ptmi_debug_guided_sample(self.h, int(op), n, 0 if recs is None else len(recs),
                                                 None if recs is None else recs.ctypes.data,
                                                 None if recs is None else rec_idx.ctypes.data, normals.ctypes.data,
                                                 in3.ctypes.data, states.ctypes.data, out.ctypes.data, used.ctypes.data))
        return out, used

    (MATH_SINCOS_D, MATH_TAN_D, MATH_LOG_D, MATH_EXP_D, MATH_ATAN2_D, MATH_SINCOSF, MATH_POWF, MATH_EXPF, MATH_ATAN2F, MATH_ACOSF,
     MATH_DIV, MATH_RCP, MATH_SQRT, MATH_ROUND, MATH_TRUNC) = range(15)

    def debug_math(self, op, a, b=None):
        """ptmi_debug_math: operation `op` (MATH_*) of the kernels' build of include/ptmi_math.h on the float32 cases (a[i], b[i]).
        Returns (n, 2) float64; float and int results are promoted, which is exact."""
        a = np.ascontiguousarray(a, np.float32).reshape(-1); n = len(a)
        b = np.zeros(n, np.float32) if b is None else np.ascontiguousarray(b, np.float32).reshape(n)
        out = np.zeros((n, 2), np.float64)
        self._ck(self.L.ptmi_debug_math(self.h, int(op), n, a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    def debug_grid_index(self, dirs, normals):
        """ptmi_debug_grid_index: the form-factor kernel's direction_to_grid_index_local on (n, 3) directions and normals."""
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3); n = len(dirs)
        normals = np.ascontiguousarray(normals, np.float32).reshape(n, 3)
        out = np.zeros(n, np.int32)
        self._ck(self.L.ptmi_debug_grid_index(self.h, n, dirs.ctypes.data, normals.ctypes.data, out.ctypes.data))
        return out

    (NEE_CALL_ENV_LOOKUP, NEE_CALL_ENV_SAMPLE, NEE_CALL_EMITTER_SAMPLE, NEE_CALL_SPECULAR, NEE_CALL_ROUGH_VERTEX, NEE_CALL_ROUGH_EVAL,
     NEE_CALL_ROUGH_SAMPLE, NEE_CALL_LIGHT_WEIGHT) = range(8)
    NEE_CALL_IN, NEE_CALL_OUT_F, NEE_CALL_OUT_I = 16, 16, 4

    def debug_nee_call(self, op, inputs):
        """ptmi_debug_nee_call: op (NEE_CALL_*) of the next-event kernel's light and surface sampling functions on the cases
        inputs (n, k <= 16) float32, against the context's emitter and environment tables.  Returns out_f (n, 16) float32 and
        out_i (n, 4) int32 (include/ptmi.h lists each op's inputs and outputs)."""
        inputs = np.ascontiguousarray(inputs, np.float32)
        inputs = inputs.reshape(len(inputs), -1)
        n = len(inputs)
        a = np.zeros((n, self.NEE_CALL_IN), np.float32)
        a[:, :inputs.shape[1]] = inputs
        out_f = np.zeros((n, self.NEE_CALL_OUT_F), np.float32); out_i = np.zeros((n, self.NEE_CALL_OUT_I), np.int32)
        self._ck(self.L.ptmi_debug_nee_call(self.h, int(op), n, a.ctypes.data, out_f.ctypes.data, out_i.ctypes.data))
        return out_f, out_i


def write_png(path, rgb8):
    """"Save PNG" (ui_windows.h:195-210): rgb8 is (H, W, 3) uint8 with row 0 = bottom row, as read_image returns it."""
    rgb8 = np.ascontiguousarray(rgb8, np.uint8)
    assert rgb8.ndim == 3 and rgb8.shape[2] == 3
    _check(lib().ptmi_write_png(os.fsencode(path), rgb8.shape[1], rgb8.shape[0], rgb8.ctypes.data))


def render_image(scene_path, width, height, spp, max_depth=5, camera=None, device_id=0, **cfg):
    """Convenience: load + allocate + one frame; returns (rgb8, radiance, stats) of the full frame."""
    r = Renderer(device_id)
    r.load_scene(scene_path)
    if camera is not None: r.set_camera(camera)
    r.update_resolution(width, height)
    r.set_config(spp=spp, max_depth=max_depth, **cfg)
    st = r.render_frame()
    rgb, rad = r.read_image()
    r.close()
    return rgb, rad, st
