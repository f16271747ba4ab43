"""ctypes view of the C ABI in include/dsrt.h and the PODs of include/dsrt_scene_abi.h.

Nothing here computes anything: it declares the structs field for field (their offsets are asserted against the
reference's in tests/test_host_golden.py::test_abi_matches_reference_layout) and binds the entry points of libdsrt_hip.so.  The library is required:
importing this module without it raises -- there is no Python or CPU fallback for the render path.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DSRT_LIB", os.path.join(_HERE, "libdsrt_hip.so"))


class DsrtF3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class GPUTextureHeader(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("offset", C.c_int)]


class GPUMaterial(C.Structure):
    _fields_ = [("type", C.c_int), ("albedo_tex", C.c_int), ("_pad0", C.c_int), ("_pad1", C.c_int),
                ("albedo", DsrtF3), ("emissive", DsrtF3), ("fuzz", C.c_float), ("ref_idx", C.c_float)]


class GPUSphere(C.Structure):
    _fields_ = [("center", DsrtF3), ("radius", C.c_float), ("material_id", C.c_int), ("_pad", C.c_int)]


class GPUTriangle(C.Structure):
    _fields_ = [("v0", DsrtF3), ("v1", DsrtF3), ("v2", DsrtF3), ("n0", DsrtF3), ("n1", DsrtF3), ("n2", DsrtF3),
                ("uv0", DsrtF3), ("uv1", DsrtF3), ("uv2", DsrtF3), ("material_id", C.c_int), ("albedo_tex", C.c_int)]


class GPUBVHNode(C.Structure):
    _fields_ = [("bbox_min", DsrtF3), ("bbox_max", DsrtF3), ("left", C.c_int), ("right", C.c_int),
                ("tri_offset", C.c_int), ("tri_count", C.c_int)]


class GPURenderParams(C.Structure):
    _fields_ = [("img_width", C.c_int), ("img_height", C.c_int), ("samples_per_pixel", C.c_int), ("max_depth", C.c_int),
                ("use_bvh", C.c_int), ("rng_mode", C.c_int), ("tile_size", C.c_int), ("_pad0", C.c_int),
                ("gamma", C.c_float), ("exposure", C.c_float), ("env_rotation", C.c_float), ("_pad1", C.c_float)]


class GPUCamera(C.Structure):
    _fields_ = [("origin", DsrtF3), ("lower_left_corner", DsrtF3), ("horizontal", DsrtF3), ("vertical", DsrtF3),
                ("u", DsrtF3), ("v", DsrtF3), ("w", DsrtF3), ("lens_radius", C.c_float),
                ("image_width", C.c_int), ("image_height", C.c_int), ("samples_per_pixel", C.c_int), ("max_depth", C.c_int)]


class GPUScene(C.Structure):
    _fields_ = [("spheres", C.c_void_p), ("num_spheres", C.c_int), ("_pad_sph0", C.c_int), ("_pad_sph1", C.c_int),
                ("triangles", C.c_void_p), ("tri_indices", C.c_void_p), ("num_triangles", C.c_int), ("_pad_geo", C.c_int),
                ("bvh_nodes", C.c_void_p), ("num_bvh_nodes", C.c_int),
                ("bvh_tri_indices", C.c_void_p),
                ("materials", C.c_void_p), ("num_materials", C.c_int), ("_pad_mat0", C.c_int), ("_pad_mat1", C.c_int),
                ("textures", C.c_void_p), ("num_textures", C.c_int), ("_pad_tex0", C.c_int), ("_pad_tex1", C.c_int),
                ("texture_pool", C.c_void_p), ("texture_pool_floats", C.c_int), ("_pad_pool0", C.c_int), ("_pad_pool1", C.c_int),
                ("camera", GPUCamera),
                ("sky_type", C.c_int), ("env_tex_id", C.c_int), ("_pad_sky0", C.c_int), ("_pad_sky1", C.c_int),
                ("sky_solid", DsrtF3), ("sky_top", DsrtF3), ("sky_bottom", DsrtF3),
                ("params", GPURenderParams),
                ("seed", C.c_uint64),
                ("sun_enabled", C.c_uint8), ("_pad_sun", C.c_uint8 * 3),
                ("sun_dir", DsrtF3), ("sun_radiance", DsrtF3)]


class DsrtPose(C.Structure):
    _fields_ = [("cam_pos_world", C.c_double * 3), ("model_pos_world", C.c_double * 3), ("model_euler_deg", C.c_float * 3)]


class DsrtFrame(C.Structure):
    _fields_ = [("cam_in_model", C.c_float * 3), ("sun_dir_model", C.c_float * 3), ("sep_m", C.c_double), ("skipped", C.c_int)]


class DsrtRenderDesc(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("spp", C.c_int), ("max_depth", C.c_int), ("gamma", C.c_float),
                ("seed", C.c_uint64), ("rng_mode", C.c_int), ("tile_size", C.c_int), ("shard_rank", C.c_int),
                ("shard_count", C.c_int), ("collect_counters", C.c_int), ("checked", C.c_int), ("stack_entries", C.c_int),
                ("tune", C.c_int * 4), ("math_mode", C.c_int)]


class DsrtStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_float), ("waves_launched", C.c_int), ("device_flags", C.c_uint32), ("lds_stack_entries", C.c_int)] + \
               [(n, C.c_uint64) for n in ("samples", "rays", "primary_hits", "box_fetches", "nodes_entered", "internal_entered", "tri_tests",
                                          "hit_updates", "sphere_tests", "shaded_hits", "tex_fetches", "stack_spills", "max_stack",
                                          "node_slots", "tri_slots", "adv_slots", "adv_active", "idle_at_leaf", "idle_waiting", "idle_done", "visits_depth_lt6", "visits_depth_lt9", "visits_depth_lt12", "tiles_total", "tiles_culled", "wave_ticks", "certificate_fallbacks", "certificate_audited", "certificate_audit_mismatches")] + \
               [(n, C.c_float) for n in ("heavy_queue_empty_ms", "light_queue_empty_ms", "last_wave_exit_ms")] + [("certified_tree_used", C.c_int)]


class DsrtGBuffer(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("t", "range", "depth", "position", "normal", "uv", "albedo", "prim_id", "material_id", "sun_cos", "flags")]


# The G-buffer channels (include/dsrt.h, dsrt_render_gbuffer): name -> (numpy dtype, components per pixel), in DsrtGBuffer's order.
GBUFFER_CHANNELS = {"t": ("<f4", 1), "range": ("<f4", 1), "depth": ("<f4", 1), "position": ("<f4", 3), "normal": ("<f4", 3), "uv": ("<f4", 2),
                    "albedo": ("<f4", 3), "prim_id": ("<i4", 1), "material_id": ("<i4", 1), "sun_cos": ("<f4", 1), "flags": ("u1", 1)}
GB_HIT, GB_FRONT_FACE, GB_SPHERE, GB_SUN_VISIBLE = 1, 2, 4, 8          # DSRT_GB_* of include/dsrt.h


class DsrtRays(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("origins", "dirs", "t_min", "t_max")]


class DsrtRayHits(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("t", "range", "position", "normal", "uv", "albedo", "prim_id", "material_id", "flags")]


class DsrtAccum(C.Structure):
    _fields_ = [("sum", C.c_void_p), ("sum_sq", C.c_void_p)]


class DsrtAdaptive(C.Structure):
    _fields_ = [("passes", C.c_int), ("min_passes", C.c_int), ("rel_tol", C.c_float), ("floor", C.c_float)]


class DsrtAdaptiveStats(C.Structure):
    _fields_ = [("passes_run", C.c_int), ("samples_total", C.c_uint64), ("active", C.c_uint32 * 64)]


class DsrtDenoiseGuides(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("normal", "position", "albedo", "range")]


class DsrtDenoise(C.Structure):
    _fields_ = [("iterations", C.c_int), ("normal_power_log2", C.c_int), ("sigma_l", C.c_float), ("sigma_z", C.c_float), ("sigma_a", C.c_float)]


class DsrtTemporal(C.Structure):
    _fields_ = [("alpha_min", C.c_float), ("normal_cos_min", C.c_float), ("plane_tol", C.c_float), ("min_support", C.c_float)]


class DsrtUpscaleGuides(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("normal", "position", "albedo", "range", "flags")]


class DsrtUpscale(C.Structure):
    _fields_ = [("normal_power_log2", C.c_int), ("sigma_z", C.c_float), ("sigma_a", C.c_float), ("use_sun", C.c_int)]


class DsrtBodyMotion(C.Structure):
    _fields_ = [("bodies", C.c_int), ("first_tri", C.c_void_p), ("num_tris", C.c_void_p), ("poses_prev", C.c_void_p), ("poses_cur", C.c_void_p), ("prim_id", C.c_void_p)]


class DsrtTemporalShading(C.Structure):
    _fields_ = [("flags", C.c_void_p), ("edge_guard", C.c_int)]


class DsrtCoverageDesc(C.Structure):
    _fields_ = [("pattern", C.c_int), ("samples", C.c_int)]


class DsrtCoverageClasses(C.Structure):
    _fields_ = [("count", C.c_int), ("first", C.c_int * 16), ("num", C.c_int * 16)]


class DsrtSensor(C.Structure):
    _fields_ = [("psf", C.c_void_p), ("psf_size", C.c_int), ("mono", C.c_int), ("gain_e", C.c_float), ("prnu", C.c_float), ("dark_e", C.c_float), ("dsnu_e", C.c_float),
                ("read_e", C.c_float), ("full_well_e", C.c_float), ("e_per_dn", C.c_float), ("offset_dn", C.c_float), ("bits", C.c_int), ("noise", C.c_int),
                ("seed", C.c_uint64), ("frame", C.c_uint32)]


class DsrtStars(C.Structure):
    _fields_ = [("count", C.c_int), ("occlusion", C.c_int), ("dir", C.c_void_p), ("flux", C.c_void_p), ("linear_in", C.c_void_p)]


class DsrtStarsOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("layer", "linear_out", "xy", "status")]


# The star field's outputs (include/dsrt.h, POINT SOURCES), in DsrtStarsOut's order: name -> (numpy dtype, per pixel or per star, components).
STAR_OUTPUTS = {"layer": ("<f4", "pixel", 3), "linear_out": ("<f4", "pixel", 3), "xy": ("<f4", "star", 2), "status": ("u1", "star", 1)}
STAR_PROJECTED, STAR_VISIBLE, STAR_INSIDE = 1, 2, 4                     # the bits of the status byte
MAX_STARS = 1 << 22


class DsrtLens(C.Structure):
    _fields_ = ([("src_width", C.c_int), ("src_height", C.c_int)] +
                [(n, C.c_float) for n in ("src_fx", "src_fy", "src_cx", "src_cy", "fx", "fy", "cx", "cy", "k1", "k2", "k3", "p1", "p2", "v1", "v2", "v3")] +
                [("cos4", C.c_int), ("filter", C.c_int), ("channels", C.c_int), ("clamp_zero", C.c_int), ("fill_bits", C.c_uint32)])


class DsrtLensOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("image", "src_xy", "status")]


LENS_NEAREST, LENS_BILINEAR, LENS_CUBIC = 0, 1, 2                       # DSRT_LENS_* of include/dsrt.h: DsrtLens.filter ...
LENS_INVERTED, LENS_ANY_TAP, LENS_ALL_TAPS = 1, 2, 4                    # ... and the bits of the status byte


class DsrtCoverage(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("hits", "alpha", "mask", "sun_hits", "sun_alpha", "sun_mask", "class_hits")] + [("rep", DsrtGBuffer)]


# The coverage pass's own outputs (include/dsrt.h, COVERAGE): name -> numpy dtype, one element per pixel (class_hits: one per pixel and class).
COVERAGE_CHANNELS = {"hits": "u1", "alpha": "<f4", "mask": "<u8", "sun_hits": "u1", "sun_alpha": "<f4", "sun_mask": "<u8", "class_hits": "u1"}
COVERAGE_GRID, COVERAGE_DIAGONAL = 0, 1                                 # DSRT_COVERAGE_* of include/dsrt.h

MAX_BODIES = 16                                                         # DSRT_MAX_BODIES of include/dsrt.h
HISTORY_FLOATS = 16                                                     # per pixel of a temporal history buffer (include/dsrt.h, TEMPORAL ACCUMULATION)

# The ray-query channels (include/dsrt.h, dsrt_trace_rays): name -> (numpy dtype, components per ray), in DsrtRayHits' order.
RAY_HIT_CHANNELS = {n: GBUFFER_CHANNELS[n] for n, _ in DsrtRayHits._fields_}
TRACE_CLOSEST, TRACE_ANY = 0, 1                                         # DSRT_TRACE_* of include/dsrt.h


# numpy record layouts of the reference arrays (for dumping / comparing with goldens)
F3 = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
TRI_DTYPE = np.dtype([("v", "<f4", (3, 3)), ("n", "<f4", (3, 3)), ("uv", "<f4", (3, 3)), ("material_id", "<i4"), ("albedo_tex", "<i4")])
NODE_DTYPE = np.dtype([("bbox_min", "<f4", 3), ("bbox_max", "<f4", 3), ("left", "<i4"), ("right", "<i4"), ("tri_offset", "<i4"), ("tri_count", "<i4")])
MAT_DTYPE = np.dtype([("type", "<i4"), ("albedo_tex", "<i4"), ("_pad", "<i4", 2), ("albedo", "<f4", 3), ("emissive", "<f4", 3), ("fuzz", "<f4"), ("ref_idx", "<f4")])
SPHERE_DTYPE = np.dtype([("center", "<f4", 3), ("radius", "<f4"), ("material_id", "<i4"), ("_pad", "<i4")])
TEXHDR_DTYPE = np.dtype([("width", "<i4"), ("height", "<i4"), ("offset", "<i4")])
assert TRI_DTYPE.itemsize == 116 and NODE_DTYPE.itemsize == 40 and MAT_DTYPE.itemsize == 48 and SPHERE_DTYPE.itemsize == 24

# The ABI version THESE hand-written structs were laid out for (include/dsrt.h, DSRT_ABI_VERSION).  load() requires library == header == this, and compares the sizes
# of the structs above with the library's own (dsrt_sizeof): a header and library bumped without this file are refused, not mis-laid.
ABI_VERSION = 8

EXPORTS = [
    "dsrt_last_error", "dsrt_abi_version", "dsrt_sizeof", "dsrt_microbench_copy", "dsrt_dev_set_experiment", "dsrt_selftest_poke_node_word", "dsrt_ctx_set_certified_tree", "dsrt_ctx_has_certified_tree", "dsrt_dropin_has_certified_tree", "dsrt_host_scene_second_tree_probe",
    "dsrt_host_scene_create", "dsrt_host_scene_destroy", "dsrt_host_scene_add_obj", "dsrt_host_scene_add_world_file",
    "dsrt_host_scene_add_arrays", "dsrt_host_scene_add_texture_file", "dsrt_host_scene_build_bvh", "dsrt_host_scene_build_bvh_sah", "dsrt_host_scene_build_bvh_gpu", "dsrt_host_scene_view", "dsrt_host_scene_bvh_stack_need", "dsrt_host_scene_texture_failures",
    "dsrt_scene_set_frame", "dsrt_read_pose_file", "dsrt_pose_to_frame", "dsrt_pose_points_to_model", "dsrt_pose_dirs_to_model", "dsrt_camera_look_at", "dsrt_decode_image_file", "dsrt_write_ppm", "dsrt_write_png", "dsrt_write_pfm",
    "dsrt_device_count", "dsrt_ctx_create", "dsrt_ctx_destroy", "dsrt_ctx_clone", "dsrt_ctx_device",
    "dsrt_multi_create", "dsrt_multi_destroy", "dsrt_multi_count", "dsrt_multi_uses_rccl", "dsrt_selftest_rccl_gather", "dsrt_multi_scene_upload", "dsrt_multi_render_frame", "dsrt_multi_render_sequence", "dsrt_scene_upload", "dsrt_scene_upload_device",
    "dsrt_scene_set_camera_sun", "dsrt_shard_layout", "dsrt_ctx_scene_bounds", "dsrt_render", "dsrt_render_batch", "dsrt_render_batch_to_host", "dsrt_deinterleave_tiles", "dsrt_deinterleave_batch", "dsrt_render_to_host", "dsrt_render_gbuffer", "dsrt_render_gbuffer_to_host",
    "dsrt_trace_rays", "dsrt_trace_rays_to_host",
    "dsrt_render_accumulate", "dsrt_render_accumulate_to_host", "dsrt_resolve_accumulated", "dsrt_resolve_accumulated_to_host",
    "dsrt_render_accumulate_masked", "dsrt_render_accumulate_masked_to_host", "dsrt_select_unconverged", "dsrt_resolve_accumulated_counts", "dsrt_render_adaptive", "dsrt_render_adaptive_to_host",
    "dsrt_denoise_defaults", "dsrt_denoise_accumulated", "dsrt_denoise_accumulated_to_host", "dsrt_render_denoised_to_host",
    "dsrt_temporal_defaults", "dsrt_denoise_temporal", "dsrt_denoise_temporal_to_host", "dsrt_render_denoised_temporal_to_host",
    "dsrt_upscale_defaults", "dsrt_upscale_guided", "dsrt_upscale_guided_to_host", "dsrt_render_upscaled_to_host",
    "dsrt_host_scene_begin_body", "dsrt_host_scene_body_count", "dsrt_host_scene_body_range", "dsrt_host_scene_build_bvh_bodies", "dsrt_host_scene_set_body_poses",
    "dsrt_scene_upload_bodies", "dsrt_scene_set_body_poses", "dsrt_ctx_body_count", "dsrt_ctx_body_update_ms", "dsrt_selftest_read_scene_words",
    "dsrt_body_motion_host", "dsrt_denoise_temporal_bodies", "dsrt_denoise_temporal_bodies_to_host", "dsrt_ctx_set_temporal_bodies", "dsrt_ctx_temporal_bodies",
    "dsrt_denoise_temporal_shaded", "dsrt_denoise_temporal_shaded_to_host", "dsrt_ctx_set_temporal_shading", "dsrt_ctx_temporal_shading",
    "dsrt_coverage_defaults", "dsrt_render_coverage", "dsrt_render_coverage_to_host", "dsrt_denoise_coverage_alpha_min", "dsrt_denoise_accumulated_coverage",
    "dsrt_denoise_accumulated_coverage_to_host", "dsrt_render_denoised_coverage_to_host",
    "dsrt_upscale_coverage_alpha_min", "dsrt_upscale_guided_coverage", "dsrt_upscale_guided_coverage_to_host", "dsrt_render_upscaled_coverage_to_host",
    "dsrt_sensor_defaults", "dsrt_sensor_psf_gaussian", "dsrt_sensor_apply", "dsrt_sensor_apply_to_host", "dsrt_write_pnm16",
    "dsrt_render_stars", "dsrt_render_stars_to_host", "dsrt_stars_from_catalog", "dsrt_stars_synthetic_catalog",
    "dsrt_lens_defaults", "dsrt_lens_apply", "dsrt_lens_apply_to_host", "dsrt_lens_distort_points", "dsrt_lens_intrinsics_from_camera",
    "dsrt_selftest_read_schedule", "dsrt_selftest_tile_order", "dsrt_selftest_tile_reorder", "dsrt_selftest_batch_table",
    "dsrt_selftest_math", "dsrt_selftest_devkat", "dsrt_selftest_philox", "dsrt_microbench_gather", "dsrt_microbench_valu", "dsrt_microbench_valu_kinds", "dsrt_microbench_valu_kind_name", "gpu_render_scene", "dsrt_build_gpu_scene", "dsrt_free_gpu_scene",
]


def header_abi_version():
    """DSRT_ABI_VERSION as written in include/dsrt.h -- the one place the number lives; the library returns what it was compiled with."""
    import re
    try:
        with open(os.path.join(os.path.dirname(_HERE), "include", "dsrt.h")) as f:
            m = re.search(r"^#define\s+DSRT_ABI_VERSION\s+(\d+)", f.read(), re.M)
    except OSError as e:
        raise ImportError(f"include/dsrt.h cannot be read ({e}): this binding checks the library against the header it was written for") from e
    if not m:
        raise ImportError("include/dsrt.h does not define DSRT_ABI_VERSION")
    return int(m.group(1))


def load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make lib` (or __graft_entry__.build()). "
            "The render path has no fallback; it is the HIP library or nothing.")
    lib = C.CDLL(LIB_PATH)
    P = C.POINTER
    vp = C.c_void_p

    def sig(name, res, args):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args

    sig("dsrt_last_error", C.c_char_p, [])
    sig("dsrt_abi_version", C.c_int, [])
    sig("dsrt_sizeof", C.c_size_t, [C.c_int])
    sig("dsrt_dev_set_experiment", C.c_int, [C.c_uint32])
    sig("dsrt_selftest_poke_node_word", C.c_int, [vp, C.c_size_t, C.c_uint32, P(C.c_uint32)])
    sig("dsrt_microbench_copy", C.c_int, [C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, P(C.c_float), P(C.c_double)])
    sig("dsrt_host_scene_create", vp, [])
    sig("dsrt_host_scene_destroy", None, [vp])
    sig("dsrt_host_scene_add_obj", C.c_int, [vp, C.c_char_p, C.c_double])
    sig("dsrt_host_scene_add_world_file", C.c_int, [vp, C.c_char_p])
    sig("dsrt_host_scene_add_arrays", C.c_int, [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int])
    sig("dsrt_host_scene_add_texture_file", C.c_int, [vp, C.c_char_p, C.c_int])
    sig("dsrt_host_scene_build_bvh", C.c_int, [vp])
    sig("dsrt_host_scene_build_bvh_sah", C.c_int, [vp])
    sig("dsrt_host_scene_build_bvh_gpu", C.c_int, [vp, C.c_int, P(C.c_float), P(C.c_float)])
    sig("dsrt_host_scene_view", C.c_int, [vp, P(GPUScene)])
    sig("dsrt_host_scene_bvh_stack_need", C.c_int, [vp])
    sig("dsrt_host_scene_texture_failures", C.c_int, [vp, C.c_char_p, C.c_size_t])
    sig("dsrt_scene_set_frame", None, [P(GPUScene), P(GPUCamera), P(C.c_float)])
    sig("dsrt_read_pose_file", C.c_int, [C.c_char_p, P(DsrtPose), C.c_int, P(C.c_int)])
    sig("dsrt_pose_to_frame", C.c_int, [P(DsrtPose), P(DsrtFrame)])
    sig("dsrt_pose_points_to_model", C.c_int, [P(DsrtPose), C.c_int, vp, vp])
    sig("dsrt_pose_dirs_to_model", C.c_int, [P(DsrtPose), C.c_int, vp, vp])
    sig("dsrt_camera_look_at", C.c_int, [P(GPUCamera), P(C.c_float), P(C.c_float), C.c_float, C.c_int, C.c_int, C.c_int, C.c_int])
    sig("dsrt_decode_image_file", C.c_int, [C.c_char_p, C.c_int, P(C.c_int), P(C.c_int), vp, C.c_size_t])
    sig("dsrt_write_ppm", C.c_int, [C.c_char_p, vp, C.c_int, C.c_int])
    sig("dsrt_write_png", C.c_int, [C.c_char_p, vp, C.c_int, C.c_int])
    sig("dsrt_write_pfm", C.c_int, [C.c_char_p, vp, C.c_int, C.c_int, C.c_int])
    sig("dsrt_device_count", C.c_int, [])
    sig("dsrt_ctx_create", C.c_int, [C.c_int, P(vp)])
    sig("dsrt_ctx_destroy", None, [vp])
    sig("dsrt_ctx_clone", C.c_int, [vp, P(vp)])
    sig("dsrt_ctx_device", C.c_int, [vp])
    sig("dsrt_ctx_set_certified_tree", C.c_int, [vp, C.c_int])
    sig("dsrt_ctx_has_certified_tree", C.c_int, [vp])
    sig("dsrt_dropin_has_certified_tree", C.c_int, [])
    sig("dsrt_host_scene_second_tree_probe", C.c_int, [vp, P(C.c_int), P(C.c_float), vp, vp, vp, C.c_int, vp, C.c_int])
    sig("dsrt_multi_create", C.c_int, [P(C.c_int), C.c_int, C.c_int, P(vp)])
    sig("dsrt_multi_destroy", None, [vp])
    sig("dsrt_multi_count", C.c_int, [vp])
    sig("dsrt_multi_uses_rccl", C.c_int, [vp])
    sig("dsrt_selftest_rccl_gather", C.c_int, [C.c_int, C.c_size_t])
    sig("dsrt_multi_scene_upload", C.c_int, [vp, P(GPUScene)])
    sig("dsrt_multi_render_frame", C.c_int, [vp, P(DsrtRenderDesc), P(GPUCamera), P(C.c_float), vp, P(C.c_float), P(C.c_double)])
    sig("dsrt_multi_render_sequence", C.c_int, [vp, P(DsrtRenderDesc), P(GPUCamera), P(C.c_float), C.c_int, P(vp), P(C.c_double)])
    sig("dsrt_scene_upload", C.c_int, [vp, P(GPUScene)])
    sig("dsrt_scene_upload_device", C.c_int, [vp, P(GPUScene)])
    sig("dsrt_scene_set_camera_sun", C.c_int, [vp, P(GPUCamera), P(C.c_float)])
    sig("dsrt_shard_layout", C.c_int, [P(DsrtRenderDesc), P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_size_t)])
    sig("dsrt_ctx_scene_bounds", C.c_int, [vp, P(C.c_float), P(C.c_float)])
    sig("dsrt_render", C.c_int, [vp, P(DsrtRenderDesc), vp, vp, vp, P(DsrtStats)])
    sig("dsrt_render_batch", C.c_int, [vp, P(DsrtRenderDesc), C.c_int, P(GPUCamera), P(C.c_float), vp, vp, vp, P(DsrtStats)])
    sig("dsrt_render_batch_to_host", C.c_int, [vp, P(DsrtRenderDesc), C.c_int, P(GPUCamera), P(C.c_float), vp, P(DsrtStats)])
    sig("dsrt_deinterleave_tiles", C.c_int, [vp, P(DsrtRenderDesc), vp, vp, vp])
    sig("dsrt_deinterleave_batch", C.c_int, [vp, P(DsrtRenderDesc), C.c_int, vp, vp, vp])
    sig("dsrt_render_to_host", C.c_int, [vp, P(DsrtRenderDesc), vp, vp, P(DsrtStats)])
    sig("dsrt_render_gbuffer", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtGBuffer), vp, P(DsrtStats)])
    sig("dsrt_render_gbuffer_to_host", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtGBuffer), P(DsrtStats)])
    sig("dsrt_trace_rays", C.c_int, [vp, C.c_int, P(DsrtRays), C.c_int, P(DsrtRayHits), vp, P(DsrtStats)])
    sig("dsrt_trace_rays_to_host", C.c_int, [vp, C.c_int, P(DsrtRays), C.c_int, P(DsrtRayHits), P(DsrtStats)])
    sig("dsrt_render_accumulate", C.c_int, [vp, P(DsrtRenderDesc), C.c_int, C.c_int, C.c_int, P(DsrtAccum), vp, P(DsrtStats)])
    sig("dsrt_render_accumulate_to_host", C.c_int, [vp, P(DsrtRenderDesc), C.c_int, C.c_int, C.c_int, P(DsrtAccum), P(DsrtStats)])
    sig("dsrt_resolve_accumulated", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAccum), C.c_int, vp, vp, vp, vp])
    sig("dsrt_resolve_accumulated_to_host", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAccum), C.c_int, vp, vp, vp])
    sig("dsrt_render_accumulate_masked", C.c_int, [vp, P(DsrtRenderDesc), C.c_int, C.c_int, C.c_int, P(DsrtAccum), vp, vp, vp, P(DsrtStats)])
    sig("dsrt_render_accumulate_masked_to_host", C.c_int, [vp, P(DsrtRenderDesc), C.c_int, C.c_int, C.c_int, P(DsrtAccum), vp, vp, P(DsrtStats)])
    sig("dsrt_select_unconverged", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAccum), vp, C.c_float, C.c_float, C.c_uint32, C.c_uint32, vp, P(C.c_uint32), vp])
    sig("dsrt_resolve_accumulated_counts", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAccum), vp, vp, vp, vp, vp])
    sig("dsrt_render_adaptive", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAdaptive), P(DsrtAccum), vp, vp, vp, vp, vp, P(DsrtAdaptiveStats)])
    sig("dsrt_render_adaptive_to_host", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAdaptive), vp, vp, vp, vp, P(DsrtAdaptiveStats)])
    sig("dsrt_denoise_defaults", None, [P(DsrtDenoise)])
    sig("dsrt_denoise_accumulated", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAccum), C.c_int, vp, P(DsrtDenoiseGuides), P(DsrtDenoise), vp, vp, vp, vp, vp])
    sig("dsrt_denoise_accumulated_to_host", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAccum), C.c_int, vp, P(DsrtDenoiseGuides), P(DsrtDenoise), vp, vp, vp, vp])
    sig("dsrt_render_denoised_to_host", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtDenoise), vp, vp, vp, vp, P(DsrtStats)])
    sig("dsrt_coverage_defaults", None, [P(DsrtCoverageDesc)])
    sig("dsrt_render_coverage", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtCoverageDesc), P(DsrtCoverageClasses), P(DsrtCoverage), vp, P(DsrtStats)])
    sig("dsrt_render_coverage_to_host", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtCoverageDesc), P(DsrtCoverageClasses), P(DsrtCoverage), P(DsrtStats)])
    sig("dsrt_denoise_coverage_alpha_min", C.c_float, [])
    sig("dsrt_denoise_accumulated_coverage", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAccum), C.c_int, vp, P(DsrtDenoiseGuides), vp, C.c_float, P(DsrtDenoise), vp, vp, vp, vp, vp])
    sig("dsrt_denoise_accumulated_coverage_to_host", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAccum), C.c_int, vp, P(DsrtDenoiseGuides), vp, C.c_float, P(DsrtDenoise), vp, vp, vp, vp])
    sig("dsrt_render_denoised_coverage_to_host", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtCoverageDesc), C.c_float, P(DsrtDenoise), vp, vp, vp, vp, vp, P(DsrtStats)])
    sig("dsrt_temporal_defaults", None, [P(DsrtTemporal)])
    sig("dsrt_denoise_temporal", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAccum), C.c_int, vp, P(DsrtDenoiseGuides), P(GPUCamera), vp, vp, P(DsrtTemporal), P(DsrtDenoise),
                                          vp, vp, vp, vp, vp, vp, vp])
    sig("dsrt_denoise_temporal_to_host", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAccum), C.c_int, vp, P(DsrtDenoiseGuides), P(GPUCamera), vp, vp, P(DsrtTemporal), P(DsrtDenoise),
                                                  vp, vp, vp, vp, vp, vp])
    sig("dsrt_render_denoised_temporal_to_host", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtDenoise), P(DsrtTemporal), C.c_int, vp, vp, vp, vp, vp, P(DsrtStats)])
    sig("dsrt_body_motion_host", C.c_int, [P(DsrtBodyMotion), C.c_int, vp, vp, vp, vp])
    sig("dsrt_denoise_temporal_bodies", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAccum), C.c_int, vp, P(DsrtDenoiseGuides), P(DsrtBodyMotion), P(GPUCamera), vp, vp,
                                                 P(DsrtTemporal), P(DsrtDenoise), vp, vp, vp, vp, vp, vp, vp, vp])
    sig("dsrt_denoise_temporal_bodies_to_host", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAccum), C.c_int, vp, P(DsrtDenoiseGuides), P(DsrtBodyMotion), P(GPUCamera), vp, vp,
                                                         P(DsrtTemporal), P(DsrtDenoise), vp, vp, vp, vp, vp, vp, vp])
    sig("dsrt_ctx_set_temporal_bodies", C.c_int, [vp, C.c_int])
    sig("dsrt_ctx_temporal_bodies", C.c_int, [vp])
    sig("dsrt_denoise_temporal_shaded", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAccum), C.c_int, vp, P(DsrtDenoiseGuides), P(DsrtBodyMotion), P(DsrtTemporalShading), P(GPUCamera),
                                                 vp, vp, P(DsrtTemporal), P(DsrtDenoise), vp, vp, vp, vp, vp, vp, vp, vp, vp])
    sig("dsrt_denoise_temporal_shaded_to_host", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtAccum), C.c_int, vp, P(DsrtDenoiseGuides), P(DsrtBodyMotion), P(DsrtTemporalShading),
                                                         P(GPUCamera), vp, vp, P(DsrtTemporal), P(DsrtDenoise), vp, vp, vp, vp, vp, vp, vp, vp])
    sig("dsrt_ctx_set_temporal_shading", C.c_int, [vp, C.c_int])
    sig("dsrt_ctx_temporal_shading", C.c_int, [vp])
    sig("dsrt_upscale_defaults", None, [P(DsrtUpscale)])
    sig("dsrt_upscale_guided", C.c_int, [vp, P(DsrtRenderDesc), C.c_int, C.c_int, vp, vp, P(DsrtUpscaleGuides), P(DsrtUpscaleGuides), P(DsrtUpscale), vp, vp, vp, vp, vp, vp])
    sig("dsrt_upscale_guided_to_host", C.c_int, [vp, P(DsrtRenderDesc), C.c_int, C.c_int, vp, vp, P(DsrtUpscaleGuides), P(DsrtUpscaleGuides), P(DsrtUpscale), vp, vp, vp, vp, vp])
    sig("dsrt_render_upscaled_to_host", C.c_int, [vp, P(DsrtRenderDesc), C.c_int, C.c_int, P(DsrtDenoise), P(DsrtUpscale), vp, vp, vp, vp, vp, P(DsrtStats)])
    sig("dsrt_upscale_coverage_alpha_min", C.c_float, [])
    sig("dsrt_upscale_guided_coverage", C.c_int, [vp, P(DsrtRenderDesc), C.c_int, C.c_int, vp, vp, P(DsrtUpscaleGuides), P(DsrtUpscaleGuides), vp, vp, C.c_float, P(DsrtUpscale),
                                                 vp, vp, vp, vp, vp, vp, vp])
    sig("dsrt_upscale_guided_coverage_to_host", C.c_int, [vp, P(DsrtRenderDesc), C.c_int, C.c_int, vp, vp, P(DsrtUpscaleGuides), P(DsrtUpscaleGuides), vp, vp, C.c_float,
                                                         P(DsrtUpscale), vp, vp, vp, vp, vp, vp])
    sig("dsrt_render_upscaled_coverage_to_host", C.c_int, [vp, P(DsrtRenderDesc), C.c_int, C.c_int, P(DsrtCoverageDesc), P(DsrtCoverageDesc), C.c_float, P(DsrtDenoise),
                                                          P(DsrtUpscale), vp, vp, vp, vp, vp, vp, P(DsrtStats)])
    sig("dsrt_sensor_defaults", None, [P(DsrtSensor)])
    sig("dsrt_sensor_psf_gaussian", C.c_int, [C.c_float, C.c_int, vp])
    sig("dsrt_sensor_apply", C.c_int, [vp, P(DsrtRenderDesc), vp, P(DsrtSensor), vp, vp, vp, vp])
    sig("dsrt_sensor_apply_to_host", C.c_int, [vp, P(DsrtRenderDesc), vp, P(DsrtSensor), vp, vp, vp])
    sig("dsrt_write_pnm16", C.c_int, [C.c_char_p, vp, C.c_int, C.c_int, C.c_int, C.c_int])
    sig("dsrt_render_stars", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtStars), P(DsrtStarsOut), vp, P(DsrtStats)])
    sig("dsrt_render_stars_to_host", C.c_int, [vp, P(DsrtRenderDesc), P(DsrtStars), P(DsrtStarsOut), P(DsrtStats)])
    sig("dsrt_stars_from_catalog", C.c_int, [C.c_int, vp, vp, vp, vp, vp, vp])
    sig("dsrt_stars_synthetic_catalog", C.c_int, [C.c_uint64, C.c_int, C.c_double, C.c_double, vp, vp, vp])
    sig("dsrt_lens_defaults", None, [P(DsrtLens)])
    sig("dsrt_lens_apply", C.c_int, [vp, P(DsrtRenderDesc), vp, P(DsrtLens), P(DsrtLensOut), vp])
    sig("dsrt_lens_apply_to_host", C.c_int, [vp, P(DsrtRenderDesc), vp, P(DsrtLens), P(DsrtLensOut)])
    sig("dsrt_lens_distort_points", C.c_int, [P(DsrtLens), C.c_int, vp, vp, vp])
    sig("dsrt_lens_intrinsics_from_camera", C.c_int, [P(GPUCamera), C.c_int, C.c_int, vp])
    sig("dsrt_host_scene_begin_body", C.c_int, [vp])
    sig("dsrt_host_scene_body_count", C.c_int, [vp])
    sig("dsrt_host_scene_body_range", C.c_int, [vp, C.c_int, P(C.c_int), P(C.c_int)])
    sig("dsrt_host_scene_build_bvh_bodies", C.c_int, [vp])
    sig("dsrt_host_scene_set_body_poses", C.c_int, [vp, C.c_int, C.c_int, vp])
    sig("dsrt_scene_upload_bodies", C.c_int, [vp, vp, P(GPUScene)])
    sig("dsrt_scene_set_body_poses", C.c_int, [vp, C.c_int, C.c_int, vp, vp, P(C.c_float)])
    sig("dsrt_ctx_body_count", C.c_int, [vp])
    sig("dsrt_ctx_body_update_ms", C.c_int, [vp, P(C.c_float)])
    sig("dsrt_selftest_read_scene_words", C.c_int, [vp, C.c_int, C.c_size_t, C.c_size_t, vp])
    sig("dsrt_selftest_math", C.c_int, [vp, C.c_int, vp, C.c_float, vp, C.c_int])
    sig("dsrt_selftest_devkat", C.c_int, [vp, C.c_int, vp, vp, C.c_int])
    sig("dsrt_selftest_philox", C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_int, vp, vp])
    sig("dsrt_selftest_read_schedule", C.c_int, [vp, C.c_int, C.c_size_t, C.c_size_t, vp])
    sig("dsrt_selftest_tile_order", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, vp, vp])
    sig("dsrt_selftest_tile_reorder", C.c_int, [vp, vp, C.c_int, vp, C.c_int, vp])
    sig("dsrt_selftest_batch_table", C.c_int, [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, vp, vp, vp])
    sig("dsrt_microbench_gather", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, P(C.c_float), P(C.c_double)])
    sig("dsrt_microbench_valu", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, P(C.c_float), P(C.c_double), P(C.c_double)])
    sig("dsrt_microbench_valu_kinds", C.c_int, [])
    sig("dsrt_microbench_valu_kind_name", C.c_char_p, [C.c_int])
    sig("gpu_render_scene", None, [P(GPUScene), C.c_int, C.c_int])
    sig("dsrt_build_gpu_scene", C.c_int, [vp, P(GPUCamera), P(C.c_float), P(GPUScene)])
    sig("dsrt_free_gpu_scene", None, [P(GPUScene)])
    have, want = lib.dsrt_abi_version(), header_abi_version()
    if not (have == want == ABI_VERSION):
        raise ImportError(f"ABI mismatch: {LIB_PATH} was built for {have}, include/dsrt.h says {want}, capi.py's structs are laid out for {ABI_VERSION}: "
                          "rebuild with `make lib` / update capi.py")
    for which, struct in enumerate((DsrtRenderDesc, DsrtStats, GPUScene, GPUCamera, DsrtPose, DsrtFrame, DsrtGBuffer, DsrtRays,
                                          DsrtRayHits, DsrtAccum, DsrtAdaptive, DsrtAdaptiveStats, DsrtDenoiseGuides, DsrtDenoise, DsrtTemporal, DsrtUpscaleGuides, DsrtUpscale, None, DsrtBodyMotion, DsrtTemporalShading, DsrtCoverageDesc, DsrtCoverage, DsrtCoverageClasses, None, DsrtSensor, None, DsrtStars, DsrtStarsOut, None, DsrtLens, DsrtLensOut)):      # DSRT_SIZEOF_* of include/dsrt.h, in order (None: an index left unassigned)
        if struct is not None and lib.dsrt_sizeof(which) != C.sizeof(struct):
            raise ImportError(f"capi.py lays {struct.__name__} out in {C.sizeof(struct)} bytes, the library in {lib.dsrt_sizeof(which)}: update capi.py")
    return lib
