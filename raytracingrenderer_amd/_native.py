"""ctypes bindings for the two native libraries (include/rtg.h, include/rth.h).

No fallback: if librtg.so / librth.so are missing or fail to load, import of the bindings
raises. Build them with `python -m raytracingrenderer_amd.build` (or __graft_entry__.build()).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")

RTG_MAT_DIFFUSE, RTG_MAT_LAMBERT, RTG_MAT_MIRROR, RTG_MAT_GLASS = 0, 1, 2, 3
RTG_OPT_CULL, RTG_OPT_COUNT, RTG_OPT_TIMING, RTG_OPT_BVH2, RTG_OPT_WAVETIME, RTG_OPT_SERIAL = 1, 2, 4, 8, 16, 32
RTG_OPT_NO_COALESCE = 64
RTG_INTEGRATOR_PATH, RTG_INTEGRATOR_DIRECT, RTG_INTEGRATOR_ALBEDO, RTG_INTEGRATOR_NORMALS = 0, 1, 2, 3
RTG_INTEGRATOR_DIRECT_MIS = 4
RTG_PROBE_TEX_SAMPLE, RTG_PROBE_TEX_ENV, RTG_PROBE_TEX_UNIFORM = 0, 1, 2
RTG_FILTER_NONE, RTG_FILTER_BOX, RTG_FILTER_TENT = 0, 1, 2
RTG_FILTER_MAX_RADIUS = 4.0
RTG_ENV_UNIFORM, RTG_ENV_LUMINANCE = 0, 1
RTG_ENV_MAX_CELLS = 1 << 24
RTG_LIGHTS_UNIFORM, RTG_LIGHTS_POWER = 0, 1
RTG_MATERIALS_REFERENCE, RTG_MATERIALS_PHYSICAL = 0, 1
RTG_PATH_MIS_OFF, RTG_PATH_MIS_POWER = 0, 1
RTG_SAMPLER_PCG, RTG_SAMPLER_SOBOL = 0, 1
RTG_MODEL_REFERENCE, RTG_MODEL_CONDUCTOR, RTG_MODEL_PLASTIC, RTG_MODEL_ORENNAYAR = 0, 1, 2, 3
RTG_MODEL_ROUGH_DIELECTRIC = 5  # (4 is left unassigned)
RTG_ALPHA_DELTA = 0.01

f32p = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)
i32p = C.POINTER(C.c_int32)


class rtg_camera(C.Structure):
    _fields_ = [("inv_proj", C.c_float * 16), ("camera", C.c_float * 16), ("origin", C.c_float * 3),
                ("width", C.c_float), ("height", C.c_float)]


class rtg_camera_proj(C.Structure):
    _fields_ = [("proj", C.c_float * 16), ("camera_to_view", C.c_float * 16), ("view_direction", C.c_float * 3),
                ("a_film", C.c_float)]


class rtg_material(C.Structure):
    _fields_ = [("kind", C.c_int32), ("two_sided", C.c_int32), ("texture", C.c_int32),
                ("int_ior", C.c_float), ("ext_ior", C.c_float), ("emission", C.c_float * 3)]


class rtg_texture(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("texels", f32p)]


class rtg_scene_desc(C.Structure):
    _fields_ = [("n_tris", C.c_uint32), ("positions", f32p), ("normals", f32p), ("uvs", f32p),
                ("material", u32p), ("n_nodes", C.c_uint32), ("node_bounds", f32p),
                ("node_links", i32p), ("n_materials", C.c_uint32),
                ("materials", C.POINTER(rtg_material)), ("n_textures", C.c_uint32),
                ("textures", C.POINTER(rtg_texture)), ("env_texture", C.c_int32),
                ("n_lights", C.c_uint32), ("lights", i32p), ("camera", rtg_camera),
                ("projection", rtg_camera_proj)]


class rtg_stats(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("extension_rays", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64), ("shadow_node_visits", C.c_uint64),
                ("shadow_tri_tests", C.c_uint64), ("extend_launches", C.c_uint64), ("render_ms", C.c_double),
                ("extend_ms", C.c_double), ("shadow_ms", C.c_double), ("shade_ms", C.c_double),
                ("lane_slots", C.c_uint64), ("node_lane_steps", C.c_uint64), ("leaf_lane_steps", C.c_uint64),
                ("leaf_phase_slots", C.c_uint64), ("pops", C.c_uint64), ("cullable_pops", C.c_uint64),
                ("tri_tail_loads", C.c_uint64), ("leafbox_tests", C.c_uint64), ("traced_camera_rays", C.c_uint64),
                ("chunk_samples", C.c_uint64), ("lane_idle_no_ray", C.c_uint64),
                ("lane_idle_last_leaf", C.c_uint64), ("lane_idle_leaf_blocked", C.c_uint64),
                ("lane_idle_retiring", C.c_uint64), ("lane_idle_leaf_popped", C.c_uint64)]


class rtg_denoise_params(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("normal_squarings", C.c_uint32), ("sigma_colour", C.c_float),
                ("sigma_albedo", C.c_float)]


class rtg_camera_sampling(C.Structure):
    _fields_ = [("filter", C.c_int32), ("filter_radius", C.c_float), ("lens_radius", C.c_float),
                ("focal_distance", C.c_float)]


class rtg_light_sampling(C.Structure):
    _fields_ = [("mode", C.c_int32), ("uniform_share", C.c_float)]


class rtg_light_grid(C.Structure):
    _fields_ = [("cells", C.c_uint32)]


class rtg_material_params(C.Structure):
    _fields_ = [("model", C.c_int32), ("alpha", C.c_float), ("sigma", C.c_float), ("eta", C.c_float * 3),
                ("k", C.c_float * 3), ("int_ior", C.c_float), ("ext_ior", C.c_float)]


class rtg_temporal_params(C.Structure):
    _fields_ = [("max_history", C.c_float), ("plane_tolerance", C.c_float), ("normal_cos", C.c_float)]


class rtg_svgf_params(C.Structure):
    _fields_ = [("temporal", rtg_temporal_params), ("iterations", C.c_uint32), ("normal_squarings", C.c_uint32),
                ("sigma_luminance", C.c_float), ("sigma_albedo", C.c_float), ("min_history", C.c_float),
                ("variance_floor", C.c_float)]


class rtg_svgf_illum_params(C.Structure):
    _fields_ = [("svgf", rtg_svgf_params), ("albedo_floor", C.c_float)]


class rth_load_options(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("skip_missing", C.c_int32),
                ("bvh_threads", C.c_int32), ("envmap", C.c_char_p)]


class rth_scene_info(C.Structure):
    _fields_ = [("n_tris", C.c_uint32), ("n_nodes", C.c_uint32), ("n_materials", C.c_uint32),
                ("n_textures", C.c_uint32), ("n_lights", C.c_uint32), ("bvh_depth", C.c_uint32),
                ("width", C.c_int32), ("height", C.c_int32), ("env_in_lights", C.c_int32),
                ("dropped_instances", C.c_uint32), ("load_ms", C.c_double), ("bvh_ms", C.c_double),
                ("bounds_min", C.c_float * 3), ("bounds_max", C.c_float * 3)]


RTG_EXPORTS = [
    ("rtg_abi_version", C.c_int32, []),
    ("rtg_build_id", C.c_char_p, []),
    ("rtg_last_error", C.c_char_p, []),
    ("rtg_device_count", C.c_int, [i32p]),
    ("rtg_create", C.c_int, [C.c_int, C.POINTER(rtg_scene_desc), C.POINTER(C.c_void_p)]),
    ("rtg_destroy", None, [C.c_void_p]),
    ("rtg_set_options", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32]),
    ("rtg_set_integrator", C.c_int, [C.c_void_p, C.c_int]),
    ("rtg_render", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, u32p, C.c_uint32]),
    ("rtg_render_async", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, u32p, C.c_uint32, C.c_void_p]),
    ("rtg_synchronize", C.c_int, [C.c_void_p]),
    ("rtg_render_idle", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    ("rtg_render_light", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64]),
    ("rtg_render_instant_radiosity", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32]),
    ("rtg_render_adaptive", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, u32p]),
    ("rtg_film_read", C.c_int, [C.c_void_p, f32p, u32p]),
    ("rtg_film_copy_device", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtg_film_load", C.c_int, [C.c_void_p, f32p, C.c_uint32]),
    ("rtg_clear", C.c_int, [C.c_void_p]),
    ("rtg_get_stats", C.c_int, [C.c_void_p, C.POINTER(rtg_stats)]),
    ("rtg_launch_times", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_uint32, u32p]),
    ("rtg_launch_rays", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32, u32p]),
    ("rtg_debug_capture", C.c_int, [C.c_void_p, C.c_int]),
    ("rtg_debug_replay", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("rtg_trace_closest", C.c_int, [C.c_void_p, f32p, C.c_uint32, f32p]),
    ("rtg_trace_visible", C.c_int, [C.c_void_p, f32p, C.c_uint32, i32p]),
    ("rtg_probe_bsdf", C.c_int, [f32p, C.c_uint32, f32p]),
    ("rtg_probe_math", C.c_int, [C.c_int, f32p, C.c_uint32, f32p]),
    ("rtg_probe_texture", C.c_int, [C.c_int, f32p, C.c_uint32, C.c_uint32, f32p, C.c_uint32, f32p]),
    ("rtg_probe_connect", C.c_int, [C.c_void_p, f32p, f32p, f32p, C.c_uint32, f32p]),
    # one node, several GPUs (rtg_multi.hip): tile stripes per device + one RCCL film reduce
    ("rtg_tiles_for_rank", C.c_int, [C.c_uint32, C.c_uint32, C.c_int, C.c_int, u32p, u32p]),
    ("rtg_group_create", C.c_int, [i32p, C.c_int, C.POINTER(rtg_scene_desc), C.POINTER(C.c_void_p)]),
    ("rtg_group_destroy", None, [C.c_void_p]),
    ("rtg_group_size", C.c_int, [C.c_void_p]),
    ("rtg_group_handle", C.c_void_p, [C.c_void_p, C.c_int]),
    ("rtg_group_set_options", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32]),
    ("rtg_group_render", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64]),
    ("rtg_group_reduce", C.c_int, [C.c_void_p]),
    ("rtg_group_render_async", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64]),
    ("rtg_group_reduce_async", C.c_int, [C.c_void_p]),
    ("rtg_group_synchronize", C.c_int, [C.c_void_p]),
    ("rtg_group_film_read", C.c_int, [C.c_void_p, f32p, u32p]),
    ("rtg_group_clear", C.c_int, [C.c_void_p]),
    ("rtg_group_reduce_ms", C.c_double, [C.c_void_p]),
    ("rtg_group_uses_rccl", C.c_int, [C.c_void_p]),
    ("rtg_group_setup_ms", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    # own-tile film exchange (rtg_multi.hip)
    ("rtg_tile_pixels", C.c_int, [C.c_uint32, C.c_uint32, u32p, C.c_uint32, u32p, u32p]),
    ("rtg_film_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("rtg_film_scatter", C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    # feature-guided film denoiser (rtg_denoise.hip)
    ("rtg_denoise_defaults", C.c_int, [C.POINTER(rtg_denoise_params)]),
    ("rtg_denoise_images", C.c_int, [C.c_int, C.c_uint32, C.c_uint32, f32p, f32p, f32p, C.POINTER(rtg_denoise_params),
                                     f32p]),
    ("rtg_denoise", C.c_int, [C.c_void_p, C.POINTER(rtg_denoise_params), f32p]),
    ("rtg_denoise_guides", C.c_int, [C.c_void_p, f32p, f32p]),
    ("rtg_denoise_copy_device", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtg_denoise_ms", C.c_double, [C.c_void_p]),
    ("rtg_group_denoise", C.c_int, [C.c_void_p, C.POINTER(rtg_denoise_params), f32p]),
    # camera sampling: pixel-filter jitter and a thin-lens aperture (rtg_render.hip)
    ("rtg_camera_sampling_defaults", C.c_int, [C.POINTER(rtg_camera_sampling)]),
    ("rtg_set_camera_sampling", C.c_int, [C.c_void_p, C.POINTER(rtg_camera_sampling)]),
    ("rtg_get_camera_sampling", C.c_int, [C.c_void_p, C.POINTER(rtg_camera_sampling)]),
    ("rtg_group_set_camera_sampling", C.c_int, [C.c_void_p, C.POINTER(rtg_camera_sampling)]),
    ("rtg_probe_camera_samples", C.c_int, [C.c_void_p, u32p, u32p, C.c_uint32, C.c_uint64, f32p, f32p]),
    # environment light sampling: the luminance alias table (rtg_env.hip)
    ("rtg_env_sampling_check", C.c_int, [C.c_int, C.c_uint32, C.c_uint32]),
    ("rtg_set_env_sampling", C.c_int, [C.c_void_p, C.c_int]),
    ("rtg_get_env_sampling", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    ("rtg_group_set_env_sampling", C.c_int, [C.c_void_p, C.c_int]),
    ("rtg_env_table", C.c_int, [C.c_void_p, u32p, u32p, f32p, C.POINTER(C.c_double)]),
    ("rtg_env_weights", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("rtg_probe_env_samples", C.c_int, [C.c_void_p, u32p, f32p, C.c_uint32, f32p]),
    ("rtg_env_alias_build", C.c_int, [C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double), u32p, f32p]),
    # light selection for NEE: the power-weighted alias table (rtg_light_pick.hip)
    ("rtg_light_sampling_defaults", C.c_int, [C.POINTER(rtg_light_sampling)]),
    ("rtg_set_light_sampling", C.c_int, [C.c_void_p, C.POINTER(rtg_light_sampling)]),
    ("rtg_get_light_sampling", C.c_int, [C.c_void_p, C.POINTER(rtg_light_sampling)]),
    ("rtg_group_set_light_sampling", C.c_int, [C.c_void_p, C.POINTER(rtg_light_sampling)]),
    ("rtg_light_weights", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("rtg_light_table", C.c_int, [C.c_void_p, u32p, f32p, C.POINTER(C.c_double)]),
    ("rtg_light_records", C.c_int, [C.c_void_p, f32p]),
    ("rtg_probe_light_pick", C.c_int, [C.c_void_p, u32p, f32p, C.c_uint32, i32p, f32p]),
    ("rtg_light_pick_build", C.c_int, [C.POINTER(C.c_double), C.c_uint32, C.c_double, C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), u32p, f32p]),
    # per-shading-point light selection: one alias table per grid cell (rtg_light_grid.hip)
    ("rtg_light_grid_defaults", C.c_int, [C.POINTER(rtg_light_grid)]),
    ("rtg_light_grid_check", C.c_int, [C.POINTER(rtg_light_grid), C.c_uint32]),
    ("rtg_set_light_grid", C.c_int, [C.c_void_p, C.POINTER(rtg_light_grid)]),
    ("rtg_get_light_grid", C.c_int, [C.c_void_p, C.POINTER(rtg_light_grid)]),
    ("rtg_group_set_light_grid", C.c_int, [C.c_void_p, C.POINTER(rtg_light_grid)]),
    ("rtg_light_grid_info", C.c_int, [C.c_void_p, u32p, f32p, f32p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    ("rtg_light_grid_table", C.c_int, [C.c_void_p, f32p]),
    ("rtg_probe_light_grid", C.c_int, [C.c_void_p, f32p, u32p, f32p, C.c_uint32, i32p, i32p, f32p]),
    ("rtg_light_grid_build", C.c_int, [f32p, C.c_uint32, C.POINTER(C.c_double), f32p, C.c_uint32, C.c_double, u32p,
                                       f32p, f32p, f32p]),
    # the material model: physical conductor, plastic and Oren-Nayar (rtg_shade_phys.hip)
    ("rtg_material_params_check", C.c_int, [C.POINTER(rtg_material_params), C.c_uint32, C.c_uint32]),
    ("rtg_set_material_params", C.c_int, [C.c_void_p, C.POINTER(rtg_material_params), C.c_uint32]),
    ("rtg_set_material_model", C.c_int, [C.c_void_p, C.c_int]),
    ("rtg_get_material_model", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    ("rtg_group_set_material_params", C.c_int, [C.c_void_p, C.POINTER(rtg_material_params), C.c_uint32]),
    ("rtg_group_set_material_model", C.c_int, [C.c_void_p, C.c_int]),
    ("rtg_probe_material", C.c_int, [f32p, C.c_uint32, f32p]),
    ("rtg_probe_transmission", C.c_int, [f32p, C.c_uint32, f32p]),
    # path-tracer MIS of emitters (rtg_shade_mis.hip)
    ("rtg_path_mis_check", C.c_int, [C.c_int]),
    ("rtg_set_path_mis", C.c_int, [C.c_void_p, C.c_int]),
    ("rtg_get_path_mis", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    ("rtg_group_set_path_mis", C.c_int, [C.c_void_p, C.c_int]),
    ("rtg_probe_mis_weight", C.c_int, [f32p, f32p, C.c_uint32, f32p]),
    ("rtg_probe_env_pdf", C.c_int, [C.c_void_p, f32p, C.c_uint32, f32p]),
    ("rtg_light_of_triangle", C.c_int, [C.c_void_p, i32p]),
    # the sampler: PCG streams or Owen-scrambled Sobol points (rtg_sampler.h)
    ("rtg_sampler_check", C.c_int, [C.c_int]),
    ("rtg_set_sampler", C.c_int, [C.c_void_p, C.c_int]),
    ("rtg_get_sampler", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    ("rtg_sampler_active", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    ("rtg_group_set_sampler", C.c_int, [C.c_void_p, C.c_int]),
    ("rtg_probe_sampler", C.c_int, [C.c_uint64, C.c_uint32, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, u32p]),
    # a movable camera (rtg_api.hip)
    ("rtg_set_camera", C.c_int, [C.c_void_p, C.POINTER(rtg_camera), C.POINTER(rtg_camera_proj)]),
    ("rtg_get_camera", C.c_int, [C.c_void_p, C.POINTER(rtg_camera), C.POINTER(rtg_camera_proj)]),
    ("rtg_group_set_camera", C.c_int, [C.c_void_p, C.POINTER(rtg_camera), C.POINTER(rtg_camera_proj)]),
    # the geometry guide and temporal accumulation by reprojection (rtg_temporal.hip)
    ("rtg_temporal_defaults", C.c_int, [C.POINTER(rtg_temporal_params)]),
    ("rtg_temporal_check", C.c_int, [C.POINTER(rtg_temporal_params)]),
    ("rtg_geometry_guide", C.c_int, [C.c_void_p, f32p, f32p]),
    ("rtg_temporal_accumulate", C.c_int, [C.c_void_p, C.POINTER(rtg_temporal_params), f32p]),
    ("rtg_temporal_history", C.c_int, [C.c_void_p, f32p]),
    ("rtg_temporal_copy_device", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtg_temporal_reset", C.c_int, [C.c_void_p]),
    ("rtg_temporal_ms", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    # variance-guided filtering of the temporal history (rtg_svgf.hip)
    ("rtg_svgf_defaults", C.c_int, [C.POINTER(rtg_svgf_params)]),
    ("rtg_svgf_check", C.c_int, [C.POINTER(rtg_svgf_params)]),
    ("rtg_svgf_accumulate", C.c_int, [C.c_void_p, C.POINTER(rtg_svgf_params), f32p]),
    ("rtg_svgf_variance", C.c_int, [C.c_void_p, f32p]),
    ("rtg_svgf_moments", C.c_int, [C.c_void_p, f32p]),
    ("rtg_svgf_copy_device", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtg_svgf_ms", C.c_int, [C.c_void_p] + [C.POINTER(C.c_double)] * 4),
    # ... its illumination mode (rtg_svgf_illum.hip)
    ("rtg_svgf_illum_defaults", C.c_int, [C.POINTER(rtg_svgf_illum_params)]),
    ("rtg_svgf_illum_check", C.c_int, [C.POINTER(rtg_svgf_illum_params)]),
    ("rtg_svgf_illum_accumulate", C.c_int, [C.c_void_p, C.POINTER(rtg_svgf_illum_params), f32p]),
    ("rtg_svgf_illum_history", C.c_int, [C.c_void_p, f32p]),
    ("rtg_svgf_illum_variance", C.c_int, [C.c_void_p, f32p]),
    ("rtg_svgf_illum_moments", C.c_int, [C.c_void_p, f32p]),
    ("rtg_svgf_illum_guide", C.c_int, [C.c_void_p, f32p, f32p]),
    ("rtg_svgf_illum_copy_device", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtg_svgf_illum_ms", C.c_int, [C.c_void_p] + [C.POINTER(C.c_double)] * 6),
    # the fused first-hit pass (rtg_gbuffer.hip)
    ("rtg_gbuffer", C.c_int, [C.c_void_p, f32p, f32p, f32p, f32p]),
    ("rtg_gbuffer_ms", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
]

RTH_EXPORTS = [
    ("rth_last_error", C.c_char_p, []),
    ("rth_build_id", C.c_char_p, []),
    ("rth_load_scene", C.c_int, [C.c_char_p, C.POINTER(rth_load_options), C.POINTER(C.c_void_p)]),
    ("rth_free_scene", None, [C.c_void_p]),
    ("rth_scene_desc", C.POINTER(rtg_scene_desc), [C.c_void_p]),
    ("rth_scene_get_info", C.c_int, [C.c_void_p, C.POINTER(rth_scene_info)]),
    ("rth_scene_permutation", C.c_int, [C.c_void_p, u32p]),
    ("rth_scene_material_params", C.POINTER(rtg_material_params), [C.c_void_p, u32p]),
    ("rth_scene_material_params_transmissive", C.POINTER(rtg_material_params), [C.c_void_p, u32p]),
    ("rth_camera_look_at", C.c_int, [f32p, f32p, f32p, C.c_float, C.c_int32, C.c_int32, C.c_int32,
                                     C.POINTER(rtg_camera), C.POINTER(rtg_camera_proj)]),
    ("rth_scene_camera_pose", C.c_int, [C.c_void_p, f32p, f32p, f32p, f32p, i32p]),
    ("rth_save_hdr", C.c_int, [C.c_char_p, C.c_int32, C.c_int32, f32p, C.c_uint32]),
    ("rth_write_hdr", C.c_int, [C.c_char_p, C.c_int32, C.c_int32, f32p]),
    ("rth_read_hdr", C.c_int, [C.c_char_p, i32p, i32p, C.POINTER(f32p)]),
    ("rth_read_png", C.c_int, [C.c_char_p, i32p, i32p, i32p, C.POINTER(C.POINTER(C.c_uint8))]),
    ("rth_write_mesh_scene", C.c_int, [C.c_char_p, f32p, C.c_uint32, C.c_int32, C.c_int32]),
    ("rth_read_ldr", C.c_int, [C.c_char_p, i32p, i32p, i32p, C.POINTER(C.POINTER(C.c_uint8))]),
    ("rth_tonemap", C.c_int, [C.c_int32, C.c_int32, f32p, C.c_uint32, C.c_float, C.POINTER(C.c_uint8)]),
    ("rth_save_png", C.c_int, [C.c_char_p, C.c_int32, C.c_int32, f32p, C.c_uint32]),
    ("rth_free", None, [C.c_void_p]),
    ("rth_write_synthetic", C.c_int, [C.c_char_p, C.c_uint32, C.c_uint64, C.c_int32, C.c_int32]),
]


def _bind(lib, exports):
    for name, res, args in exports:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


_rth = None
_rtg = None


def rth():
    global _rth
    if _rth is None:
        path = os.path.join(LIB_DIR, "librth.so")
        if not os.path.exists(path):
            raise ImportError("librth.so not built (run raytracingrenderer_amd.build)")
        _rth = _bind(C.CDLL(path), RTH_EXPORTS)
    return _rth


def rtg():
    """The HIP library. Raises if missing: there is no CPU fallback for the render path."""
    global _rtg
    if _rtg is None:
        path = os.environ.get("RTG_LIB") or os.path.join(LIB_DIR, "librtg.so")  # RTG_LIB: A/B builds
        if not os.path.exists(path):
            raise ImportError("librtg.so not built (run raytracingrenderer_amd.build)")
        _rtg = _bind(C.CDLL(path, mode=C.RTLD_GLOBAL), RTG_EXPORTS)
    return _rtg


def ptr(arr, ctype):
    return arr.ctypes.data_as(C.POINTER(ctype))


def probe_sampler(seed, pixels, samples, n_draws, first_draw=0, stream=0):
    """The Sobol sampler's raw draws as the kernels compute them (rtg_probe_sampler, test surface) on the
    current device: (n, n_draws) uint32, draws first_draw.. of each (pixels[i], samples[i]) under the
    key of (pixel, seed, stream); no rounding of the counter between draws."""
    import numpy as np
    px = np.ascontiguousarray(pixels, np.uint32).ravel()
    sm = np.ascontiguousarray(samples, np.uint32).ravel()
    if len(px) != len(sm):
        raise ValueError("pixels and samples must have the same length")
    out = np.zeros((len(px), int(n_draws)), np.uint32)
    lib = rtg()
    rc = lib.rtg_probe_sampler(int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), ptr(px, C.c_uint32), ptr(sm, C.c_uint32),
                               len(px), int(first_draw), int(n_draws), ptr(out, C.c_uint32))
    if rc != 0:
        from .renderer import NativeError  # (renderer imports this module)
        raise NativeError("%s (code %d)" % (lib.rtg_last_error().decode(errors="replace"), rc))
    return out
