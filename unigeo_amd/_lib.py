"""ctypes binding of libunigeo_hip.so (C ABI: include/unigeo_hip.h).

There is deliberately NO fallback: if the shared library is missing or no MI355X is visible
the import / Engine construction raises.  numpy arrays in, numpy arrays out; torch never
crosses this boundary.
"""
import ctypes as C
import dataclasses
import json
import os
import warnings

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UG_LIB_PATH") or os.path.join(_HERE, "csrc", "libunigeo_hip.so")   # UG_LIB_PATH: A/B a second build of the SAME library (tools/ab)

EXPORTS = [
    "ug_unet_config_default", "ug_vae_config_default", "ug_clip_config_default",
    "ug_create", "ug_destroy", "ug_last_error", "ug_workspace_peak",
    "ug_load_tensor", "ug_bind_unet", "ug_bind_vae", "ug_bind_clip",
    "ug_dc_set_inputs", "ug_dc_run", "ug_dc_run_windows", "ug_dc_get_outputs", "ug_dc_device_ptrs", "ug_dc_set_trace", "ug_dc_set_guidance", "ug_unet_forward_pair", "ug_dc_set_inputs_ex", "ug_dc_get_noise", "ug_op_philox_u32", "ug_op_randn", "ug_op_u8_to_frames", "ug_set_vae_encode_fp32", "ug_set_concurrency", "ug_set_coscheduled", "ug_set_fp8_linears", "ug_op_linear_mx8", "ug_set_ff_fused", "ug_op_ff", "ug_op_ln_ff", "ug_bench_ff", "ug_bench_flash", "ug_tune_flash", "ug_tune_ff",
    "ug_eval_depth", "ug_eval_normal", "ug_depth_eval_opts_default", "ug_eval_depth_ex", "ug_eval_depth_global", "ug_op_masked_median", "ug_eval_depth_l1_info", "ug_op_l1_fit", "ug_depth_eval_opts2_default", "ug_eval_depth_ex2", "ug_dc_get_disparity", "ug_clip_embed", "ug_vae_encode", "ug_vae_decode", "ug_unet_forward", "ug_normals_from_depth",
    "ug_op_linear", "ug_op_conv", "ug_op_conv_gn", "ug_op_groupnorm", "ug_op_layernorm", "ug_op_flash_attn",
    "ug_op_temporal_attn", "ug_op_attention_generic", "ug_op_flash_attn_dh", "ug_op_euler_step", "ug_op_flash_cross_attn", "ug_op_temporal_attn_nv",
    "ug_op_groupnorm_ex", "ug_op_layernorm_ex", "ug_op_flash_attn_dh_ex", "ug_op_attention_generic_ex", "ug_op_gemm_batched",
    "ug_op_split_pair", "ug_op_gn32_pair", "ug_op_conv_wide", "ug_op_attn_wide",
    "ug_op_bind_conv", "ug_op_conv_bound", "ug_op_ff_ex", "ug_op_quant_mx8_ex", "ug_op_linear_mx8_ex", "ug_op_linear_engine", "ug_op_linear_ex", "ug_op_conv_epi",
    "ug_op_clip_patchify", "ug_op_prep_video", "ug_op_init_latents", "ug_op_unet_input", "ug_op_euler_step_cfg", "ug_op_window_blend",
    "ug_op_time_conv_out", "ug_op_depth_post", "ug_op_add_grid_nearest", "ug_op_sn_normals_out", "ug_op_clip_assemble",
    "ug_bind_stablenormal", "ug_sn_run", "ug_sn_unet_forward", "ug_sn_dino", "ug_sn_vae_decode", "ug_sn_vae_encode", "ug_resize_bilinear",
    "ug_pcd_opts_default", "ug_pcd_world_points", "ug_eval_pcd", "ug_op_pcd_nn", "ug_op_pcd_select", "ug_op_pcd_knn_normals", "ug_eval_pcd_fps", "ug_op_pcd_fps",
    "ug_eval_pcd_ex", "ug_op_pcd_nn_grid", "ug_op_pcd_knn_normals_grid",
    "ug_pcd_score_opts_default", "ug_eval_pcd_scores", "ug_op_voxel_set",
    "ug_pointmap_opts_default", "ug_pointmap_focal", "ug_pointmap_poses",
    "ug_vis_depth_range", "ug_vis_panels", "ug_prep_resize_frames", "ug_prep_gt", "ug_prep_gt_ex",
    "ug_register_opts_default", "ug_prep_register_depth", "ug_render_opts_default", "ug_prep_render_mesh",
    "ug_gt_normals_opts_default", "ug_prep_gt_normals",
    "ug_tae_opts_default", "ug_eval_tae",
    "ug_profile_begin", "ug_profile_begin_shapes", "ug_profile_end", "ug_bench_gemm", "ug_bench_groupnorm", "ug_bench_mfma_peak", "ug_tune_force",
]


class UNetConfigC(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("num_levels", C.c_int),
                ("block_out_channels", C.c_int * 8), ("num_attention_heads", C.c_int * 8),
                ("down_has_attn", C.c_int * 8),
                ("layers_per_block", C.c_int), ("cross_attention_dim", C.c_int),
                ("addition_time_embed_dim", C.c_int), ("projection_class_embeddings_input_dim", C.c_int),
                ("norm_groups", C.c_int),
                ("eps_cross_attn_blocks", C.c_float), ("eps_plain_down_block", C.c_float),
                ("eps_mid_block", C.c_float), ("eps_up_blocks", C.c_float)]


class VAEConfigC(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("latent_channels", C.c_int),
                ("num_levels", C.c_int), ("block_out_channels", C.c_int * 8),
                ("layers_per_block", C.c_int), ("norm_groups", C.c_int), ("scaling_factor", C.c_float)]


class CLIPConfigC(C.Structure):
    _fields_ = [("hidden_size", C.c_int), ("intermediate_size", C.c_int), ("num_hidden_layers", C.c_int),
                ("num_attention_heads", C.c_int), ("image_size", C.c_int), ("patch_size", C.c_int),
                ("projection_dim", C.c_int), ("layer_norm_eps", C.c_float)]


class DepthEvalOptsC(C.Structure):
    _fields_ = [("alignment", C.c_int), ("max_depth", C.c_float), ("pre_clip_min", C.c_float), ("pre_clip_max", C.c_float),
                ("post_clip_min", C.c_float), ("post_clip_max", C.c_float)]


class DepthEvalOpts2C(C.Structure):
    _fields_ = [("base", DepthEvalOptsC), ("flags", C.c_uint), ("disp_clip_min", C.c_float)]


class PcdOptsC(C.Structure):
    _fields_ = [("threshold", C.c_float), ("max_iteration", C.c_int), ("knn", C.c_int)]


class PcdScoreOptsC(C.Structure):
    _fields_ = [("n_thresholds", C.c_int), ("thresholds", C.c_double * 8), ("n_voxel_sizes", C.c_int), ("voxel_sizes", C.c_double * 4)]


class PointmapOptsC(C.Structure):
    _fields_ = [("reproj_px", C.c_double), ("max_iter", C.c_int), ("max_rounds", C.c_int)]


class RegisterOptsC(C.Structure):
    _fields_ = [("src_focal", C.c_double), ("dst_focal", C.c_double), ("src2dst", C.c_double * 12), ("divisor", C.c_float),
                ("max_valid", C.c_float), ("flags", C.c_uint)]


class RenderOptsC(C.Structure):
    _fields_ = [("znear", C.c_double), ("zfar", C.c_double), ("flags", C.c_uint)]


class GtNormalsOptsC(C.Structure):
    _fields_ = [("radius", C.c_int), ("edge", C.c_double), ("min_count", C.c_int)]


class TaeOptsC(C.Structure):
    _fields_ = [("s", C.c_float), ("t", C.c_float), ("flags", C.c_uint), ("disp_clip_min", C.c_float), ("post_clip_min", C.c_float),
                ("post_clip_max", C.c_float), ("max_depth", C.c_float), ("stride", C.c_int)]


DEPTH_ALIGNMENTS = {"lstsq": 0, "median": 1, "scale": 2, "metric": 3, "l1": 4}    # UG_ALIGN_* of include/unigeo_hip.h
DEPTH_ALIGN_DISPARITY = 1                                                # UG_DEPTH_ALIGN_DISPARITY of include/unigeo_hip.h
PREP_DEPTH_F64, PREP_ZOOMED = 1, 2                                       # UG_PREP_* of include/unigeo_hip.h
REG_DROP_SENTINEL = 1                                                    # UG_REG_* of include/unigeo_hip.h


def _depth_opts(alignment, max_depth, clips):
    """``ug_depth_eval_opts``: ``None`` (no depth bound, a clip that is off) travels as NaN."""
    return DepthEvalOptsC(DEPTH_ALIGNMENTS[alignment], *[float("nan") if v is None else float(v) for v in (max_depth, *clips)])


_lib = None


def _set_argtypes(lib, table):
    """argtypes of entry points that an explicitly selected OLDER build (UG_LIB_PATH, tools/ab A/B runs) may lack, one call per group that arrived together; the in-tree build must have them."""
    try:
        for name, argtypes in table.items():
            getattr(lib, name).argtypes = argtypes
    except AttributeError:
        if not os.environ.get("UG_LIB_PATH"):
            raise


def load_library():
    """dlopen the in-tree library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C unigeo_amd/csrc`).  The MI355X path has no CPU / PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    fp, ip, vp = C.POINTER(C.c_float), C.c_int, C.c_void_p
    lib.ug_create.restype = vp
    lib.ug_create.argtypes = [ip, C.c_size_t, C.c_size_t]
    lib.ug_destroy.argtypes = [vp]
    lib.ug_last_error.restype = C.c_char_p
    lib.ug_last_error.argtypes = [vp]
    lib.ug_workspace_peak.restype = C.c_size_t
    lib.ug_workspace_peak.argtypes = [vp]
    lib.ug_load_tensor.argtypes = [vp, C.c_char_p, ip, ip, C.POINTER(C.c_int64), vp]
    lib.ug_bind_unet.argtypes = [vp, C.POINTER(UNetConfigC)]
    lib.ug_bind_vae.argtypes = [vp, C.POINTER(VAEConfigC)]
    lib.ug_bind_clip.argtypes = [vp, C.POINTER(CLIPConfigC)]
    lib.ug_dc_set_inputs.argtypes = [vp, vp, ip, ip, ip, vp, vp, vp]
    lib.ug_dc_run.argtypes = [vp, ip, ip, ip]
    lib.ug_dc_run_windows.argtypes = [vp, ip, ip, ip, ip, ip]
    lib.ug_dc_get_outputs.argtypes = [vp, vp, vp, vp]
    lib.ug_dc_set_trace.argtypes = [vp, vp, ip]
    lib.ug_set_vae_encode_fp32.argtypes = [vp, ip]
    _set_argtypes(lib, {
        "ug_set_fp8_linears": [vp, ip], "ug_set_concurrency": [vp, ip], "ug_set_coscheduled": [vp, ip], "ug_set_ff_fused": [vp, ip],
        "ug_bench_ff": [vp, ip, ip, ip, ip, vp], "ug_bench_flash": [vp, ip, ip, ip, ip, ip, vp], "ug_tune_flash": [vp, ip], "ug_tune_ff": [vp, ip],
        "ug_op_ff": [vp, vp, ip, ip, vp, vp, vp, vp, vp, C.c_float, C.c_float, ip, vp],
        "ug_op_ln_ff": [vp, vp, ip, ip, vp, vp, C.c_float, vp, ip, vp, vp, vp, vp, C.c_float, C.c_float, ip, vp],
        "ug_op_linear_mx8": [vp, vp, ip, ip, vp, ip, vp, ip, vp, vp, vp]})
    _set_argtypes(lib, {"ug_dc_set_guidance": [vp, C.c_float], "ug_unet_forward_pair": [vp, vp, vp, vp, vp, ip, ip, ip, C.c_float, vp, vp]})
    _set_argtypes(lib, {
        "ug_dc_set_inputs_ex": [vp, vp, ip, ip, ip, ip, vp, vp, C.c_uint64, vp], "ug_dc_get_noise": [vp, vp, vp],
        "ug_op_philox_u32": [vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_long, vp],
        "ug_op_randn": [vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_long, C.c_long, vp], "ug_op_u8_to_frames": [vp, vp, ip, ip, ip, vp]})
    lib.ug_dc_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.ug_eval_depth.argtypes = [vp, vp, vp, vp, C.c_long, C.c_float, vp]
    lib.ug_eval_normal.argtypes = [vp, vp, vp, vp, C.c_long, vp]
    lib.ug_depth_eval_opts_default.restype = None
    lib.ug_depth_eval_opts_default.argtypes = [C.POINTER(DepthEvalOptsC)]
    lib.ug_eval_depth_ex.argtypes = [vp, vp, vp, vp, C.c_long, C.POINTER(DepthEvalOptsC), vp, vp]
    lib.ug_eval_depth_global.argtypes = [vp, vp, vp, vp, vp, vp, vp, ip, ip, ip, C.POINTER(DepthEvalOptsC), vp, vp]
    lib.ug_op_masked_median.argtypes = [vp, vp, vp, C.c_long, C.c_float, C.c_float, C.c_float, vp, C.POINTER(C.c_long)]
    _set_argtypes(lib, {"ug_eval_depth_l1_info": [vp, C.POINTER(C.c_long)],
                        "ug_op_l1_fit": [vp, vp, vp, C.c_long, C.POINTER(DepthEvalOptsC), vp, C.POINTER(C.c_long)]})
    _set_argtypes(lib, {"ug_depth_eval_opts2_default": [C.POINTER(DepthEvalOpts2C)],
                        "ug_eval_depth_ex2": [vp, vp, vp, vp, C.c_long, C.POINTER(DepthEvalOpts2C), vp, vp],
                        "ug_dc_get_disparity": [vp, vp]})
    if hasattr(lib, "ug_depth_eval_opts2_default"):
        lib.ug_depth_eval_opts2_default.restype = None
    lib.ug_pcd_opts_default.restype = None
    _set_argtypes(lib, {"ug_pcd_opts_default": [C.POINTER(PcdOptsC)],
                        "ug_pcd_world_points": [vp, vp, vp, vp, vp, ip, ip, ip, C.POINTER(DepthEvalOptsC), vp, vp],
                        "ug_eval_pcd": [vp, vp, vp, vp, C.c_long, vp, C.c_long, C.POINTER(PcdOptsC), vp, vp, vp],
                        "ug_op_pcd_nn": [vp, vp, C.c_long, vp, C.c_long, vp, vp, vp],
                        "ug_op_pcd_select": [vp, vp, ip, C.c_long, C.c_long, vp],
                        "ug_op_pcd_knn_normals": [vp, vp, C.c_long, ip, vp, vp]})
    _set_argtypes(lib, {"ug_eval_pcd_fps": [vp, vp, vp, vp, C.c_long, C.c_long, C.POINTER(PcdOptsC), vp, vp, vp, vp, vp],
                        "ug_op_pcd_fps": [vp, vp, C.c_long, C.c_long, vp, vp]})
    _set_argtypes(lib, {"ug_eval_pcd_ex": [vp, vp, vp, vp, C.c_long, vp, C.c_long, C.POINTER(PcdOptsC), ip, vp, vp, vp, vp, vp, vp],
                        "ug_op_pcd_nn_grid": [vp, vp, C.c_long, vp, C.c_long, vp, vp, vp, vp],
                        "ug_op_pcd_knn_normals_grid": [vp, vp, C.c_long, ip, vp, vp, vp]})
    _set_argtypes(lib, {"ug_pcd_score_opts_default": [C.POINTER(PcdScoreOptsC)],
                        "ug_eval_pcd_scores": [vp, vp, vp, vp, C.c_long, vp, C.c_long, C.POINTER(PcdOptsC), ip, vp, vp, vp, vp, vp, vp,
                                               C.POINTER(PcdScoreOptsC), vp, vp],
                        "ug_op_voxel_set": [vp, vp, C.c_long, vp, C.c_long, C.c_double, ip, vp]})
    if hasattr(lib, "ug_pcd_score_opts_default"):
        lib.ug_pcd_score_opts_default.restype = None
    _set_argtypes(lib, {"ug_pointmap_opts_default": [C.POINTER(PointmapOptsC)],
                        "ug_pointmap_focal": [vp, vp, ip, ip, C.c_double, C.c_double, vp],
                        "ug_pointmap_poses": [vp, vp, vp, ip, ip, ip, C.c_double, C.c_double, C.c_double, C.POINTER(PointmapOptsC), vp, vp, vp, vp]})
    if hasattr(lib, "ug_pointmap_opts_default"):
        lib.ug_pointmap_opts_default.restype = None
    _set_argtypes(lib, {"ug_vis_depth_range": [vp, vp, C.c_long, vp],
                        "ug_vis_panels": [vp, vp, vp, vp, ip, ip, ip, ip, C.c_float, C.c_float, vp, vp, ip, vp]})
    _set_argtypes(lib, {"ug_prep_resize_frames": [vp, vp, ip, ip, ip, ip, ip, vp, vp, ip, vp, vp, ip, vp],
                        "ug_prep_gt": [vp, vp, C.c_float, vp, vp, vp, ip, ip, ip, vp, ip, vp, ip, C.c_float, vp, vp, vp, vp, vp],
                        "ug_prep_gt_ex": [vp, vp, C.c_float, vp, vp, vp, ip, ip, ip, vp, ip, vp, ip, C.c_float, vp, vp, vp, vp, vp, C.c_uint]})
    _set_argtypes(lib, {"ug_register_opts_default": [C.POINTER(RegisterOptsC)],
                        "ug_prep_register_depth": [vp, vp, ip, ip, ip, C.POINTER(RegisterOptsC), vp]})
    _set_argtypes(lib, {"ug_render_opts_default": [C.POINTER(RenderOptsC)],
                        "ug_prep_render_mesh": [vp, vp, C.c_long, vp, C.c_long, vp, vp, ip, ip, ip, vp, C.POINTER(RenderOptsC), vp, vp, vp]})
    if hasattr(lib, "ug_render_opts_default"):
        lib.ug_render_opts_default.restype = None
    _set_argtypes(lib, {"ug_gt_normals_opts_default": [C.POINTER(GtNormalsOptsC)],
                        "ug_prep_gt_normals": [vp, vp, C.c_float, vp, vp, ip, ip, ip, vp, ip, vp, ip, C.c_float, C.POINTER(GtNormalsOptsC), vp, vp, vp,
                                               C.c_uint]})
    if hasattr(lib, "ug_gt_normals_opts_default"):
        lib.ug_gt_normals_opts_default.restype = None
    _set_argtypes(lib, {"ug_tae_opts_default": [C.POINTER(TaeOptsC)],
                        "ug_eval_tae": [vp, vp, vp, vp, vp, vp, ip, ip, ip, C.POINTER(TaeOptsC), vp, vp, vp, vp]})
    if hasattr(lib, "ug_tae_opts_default"):
        lib.ug_tae_opts_default.restype = None
    lib.ug_clip_embed.argtypes = [vp, vp, ip, ip, ip, vp]
    lib.ug_vae_encode.argtypes = [vp, vp, ip, ip, ip, vp]
    lib.ug_vae_decode.argtypes = [vp, vp, ip, ip, ip, vp]
    lib.ug_unet_forward.argtypes = [vp, vp, ip, ip, ip, C.c_float, vp, vp]
    lib.ug_normals_from_depth.argtypes = [vp, vp, vp, ip, ip, ip, vp]
    lib.ug_op_linear.argtypes = [vp, vp, ip, ip, vp, ip, vp, vp, C.c_float, C.c_float, ip, ip, vp]
    lib.ug_op_conv.argtypes = [vp, vp, ip, vp, ip, ip, ip, ip, vp, vp, ip, ip, ip, ip, ip, ip, ip, vp]
    lib.ug_op_groupnorm.argtypes = [vp, vp, ip, vp, ip, ip, ip, ip, C.c_float, ip, ip, vp, vp, vp]
    lib.ug_op_conv_gn.argtypes = [vp, vp, ip, ip, ip, ip, vp, vp, vp, ip, ip, ip, ip, C.c_float, ip, vp, vp, vp, vp, vp, vp]
    lib.ug_op_layernorm.argtypes = [vp, vp, ip, ip, C.c_float, vp, vp, vp, ip, vp, vp]
    lib.ug_op_flash_attn.argtypes = [vp, vp, ip, ip, ip, vp]
    lib.ug_op_temporal_attn.argtypes = [vp, vp, ip, ip, ip, vp]
    lib.ug_op_attention_generic.argtypes = [vp, vp, ip, ip, ip, ip, vp]
    lib.ug_op_flash_attn_dh.argtypes = [vp, vp, ip, ip, ip, ip, vp]
    lib.ug_op_euler_step.argtypes = [vp, vp, vp, C.c_long, C.c_float, C.c_float]
    _set_argtypes(lib, {"ug_op_flash_cross_attn": [vp, vp, vp, ip, ip, ip, ip, ip, C.c_long, C.c_long, C.c_long, C.c_long, vp],
                        "ug_op_temporal_attn_nv": [vp, vp, ip, ip, ip, ip, vp]})
    _set_argtypes(lib, {"ug_op_flash_attn_dh_ex": [vp, vp, ip, ip, ip, ip, C.c_long, C.c_long, C.c_long, vp],
                        "ug_op_attention_generic_ex": [vp, vp, ip, ip, ip, ip, C.c_long, C.c_long, C.c_long, vp, vp],
                        "ug_op_gemm_batched": [vp, vp, C.c_long, C.c_long, C.c_long, vp, C.c_long, C.c_long, C.c_long, ip, ip, ip, ip, ip, C.c_float, ip,
                                               C.c_long, C.c_long, C.c_long, C.c_long, C.c_long, C.c_long, vp, vp]})
    _set_argtypes(lib, {"ug_op_groupnorm_ex": [vp, vp, ip, vp, ip, ip, ip, ip, C.c_float, ip, ip, vp, vp, ip, C.c_long, vp, vp],
                        "ug_op_layernorm_ex": [vp, vp, ip, ip, C.c_float, vp, vp, vp, ip, C.c_long, ip, C.c_long, vp, vp, vp, vp, vp]})
    _set_argtypes(lib, {
        "ug_op_split_pair": [vp, vp, C.c_long, ip, vp, vp], "ug_op_gn32_pair": [vp, vp, ip, ip, ip, ip, C.c_float, ip, vp, vp, vp, vp],
        "ug_op_conv_wide": [vp, vp, ip, ip, ip, ip, vp, vp, ip, vp, ip, ip, ip, ip, ip, vp], "ug_op_attn_wide": [vp, vp, ip, ip, ip, vp]})
    _set_argtypes(lib, {
        "ug_op_bind_conv": [vp, vp, vp, ip, ip, ip, ip, ip, vp, vp, vp],
        "ug_op_conv_bound": [vp, vp, vp, ip, ip, ip, ip, ip, vp, ip, vp, ip, ip, ip, ip, ip, ip, ip, ip, vp, C.c_float, C.c_float, ip, C.c_long, C.c_long, vp, vp]})
    _set_argtypes(lib, {"ug_op_ff_ex": [vp, vp, ip, ip, vp, vp, vp, vp, vp, ip, vp, C.c_float, C.c_float, C.c_float, vp, vp, C.c_float, vp, ip,
                                        ip, ip, C.c_long, C.c_long, vp, vp]})
    lg, fl = C.c_long, C.c_float
    _set_argtypes(lib, {
        "ug_op_quant_mx8_ex": [vp, vp, ip, ip, lg, lg, lg, vp, vp],
        "ug_op_linear_mx8_ex": [vp, vp, ip, ip, vp, ip, vp, vp, lg, vp, lg, fl, fl, fl, ip, ip, lg, lg, ip, vp, vp, vp, vp],
        "ug_op_linear_engine": [vp, vp, ip, lg, vp, ip, ip, vp, vp, vp, fl, vp, lg, vp, lg, fl, fl, fl, ip, ip, lg, lg, vp, vp]})
    _set_argtypes(lib, {
        "ug_op_linear_ex": [vp, vp, ip, lg, vp, ip, ip, vp, vp, vp, lg, vp, lg, fl, fl, fl, ip, ip, lg, lg, vp, vp],
        "ug_op_conv_epi": [vp, vp, vp, ip, ip, ip, ip, vp, ip, vp, ip, ip, ip, ip, ip, ip, ip, vp, vp, lg, vp, lg, fl, fl, fl, ip, lg, lg, vp, ip, vp, vp, vp]})
    _set_argtypes(lib, {
        "ug_op_clip_patchify": [vp, vp, ip, ip, ip, ip, ip, ip, ip, lg, vp], "ug_op_prep_video": [vp, vp, vp, ip, ip, ip, fl, lg, vp, vp],
        "ug_op_init_latents": [vp, vp, ip, lg, fl, lg, vp], "ug_op_unet_input": [vp, vp, vp, lg, fl, ip, lg, vp],
        "ug_op_euler_step_cfg": [vp, vp, vp, fl, lg, fl, fl, lg, vp], "ug_op_window_blend": [vp, vp, vp, lg, ip, fl, lg, vp, vp],
        "ug_op_time_conv_out": [vp, vp, vp, vp, ip, lg, ip, lg, vp], "ug_op_depth_post": [vp, vp, lg, lg, vp, vp, vp],
        "ug_op_add_grid_nearest": [vp, vp, ip, ip, ip, ip, ip, lg, vp], "ug_op_sn_normals_out": [vp, vp, ip, lg, lg, vp],
        "ug_op_clip_assemble": [vp, vp, vp, vp, ip, ip, ip, lg, vp]})
    lib.ug_bind_stablenormal.argtypes = [vp, C.POINTER(UNetConfigC), C.POINTER(VAEConfigC), C.POINTER(CLIPConfigC)]
    lib.ug_sn_run.argtypes = [vp, vp, ip, ip, ip, vp, C.c_float, ip, vp, vp, vp, vp]
    lib.ug_sn_unet_forward.argtypes = [vp, ip, vp, vp, ip, ip, ip, C.c_float, C.c_float, vp, vp, ip, vp]
    lib.ug_sn_dino.argtypes = [vp, vp, ip, ip, ip, vp]
    lib.ug_sn_vae_decode.argtypes = [vp, vp, ip, ip, ip, vp]
    lib.ug_sn_vae_encode.argtypes = [vp, vp, ip, ip, ip, vp]
    lib.ug_resize_bilinear.argtypes = [vp, vp, ip, ip, ip, ip, ip, ip, ip, vp]
    lib.ug_profile_begin.argtypes = [vp]
    lib.ug_bench_gemm.argtypes = [vp] + [ip] * 16 + [vp]
    lib.ug_bench_groupnorm.argtypes = [vp, ip, ip, ip, ip, ip, ip, ip, vp]
    lib.ug_bench_mfma_peak.argtypes = [vp, ip, vp]
    lib.ug_tune_force.argtypes = [vp, ip, ip]
    lib.ug_profile_begin_shapes.argtypes = [vp]
    lib.ug_profile_end.restype = C.c_char_p
    lib.ug_profile_end.argtypes = [vp]
    _lib = lib
    return lib


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _fill8(dst, vals):
    for i in range(8):
        dst[i] = int(vals[i]) if i < len(vals) else 0


def _unet_c(cfg):
    """ug_unet_config of a UNet config object; a StableNormal (SD) config lacks the SVD-only attributes, which go over as 0."""
    c = UNetConfigC()
    c.in_channels, c.out_channels, c.num_levels = cfg.in_channels, cfg.out_channels, len(cfg.block_out_channels)
    _fill8(c.block_out_channels, cfg.block_out_channels)
    _fill8(c.num_attention_heads, cfg.num_attention_heads)
    _fill8(c.down_has_attn, [int(b) for b in cfg.down_has_attn])
    c.layers_per_block, c.cross_attention_dim, c.norm_groups = cfg.layers_per_block, cfg.cross_attention_dim, cfg.norm_groups
    for name in ("addition_time_embed_dim", "projection_class_embeddings_input_dim",
                 "eps_cross_attn_blocks", "eps_plain_down_block", "eps_mid_block", "eps_up_blocks"):
        setattr(c, name, getattr(cfg, name, 0))
    return c


def _vae_c(cfg):
    c = VAEConfigC()
    c.in_channels, c.out_channels, c.latent_channels = cfg.in_channels, cfg.out_channels, cfg.latent_channels
    c.num_levels = len(cfg.block_out_channels)
    _fill8(c.block_out_channels, cfg.block_out_channels)
    c.layers_per_block, c.norm_groups, c.scaling_factor = cfg.layers_per_block, cfg.norm_groups, cfg.scaling_factor
    return c


def _clip_c(cfg):
    """ug_clip_config of a CLIP / DINOv2 tower config; a DINOv2 config has no projection_dim (0)."""
    c = CLIPConfigC()
    c.hidden_size, c.intermediate_size = cfg.hidden_size, cfg.intermediate_size
    c.num_hidden_layers, c.num_attention_heads = cfg.num_hidden_layers, cfg.num_attention_heads
    c.image_size, c.patch_size, c.layer_norm_eps = cfg.image_size, cfg.patch_size, cfg.layer_norm_eps
    c.projection_dim = getattr(cfg, "projection_dim", 0)
    return c


class Engine:
    """One context = one GPU.  Mirrors, at the C-ABI level, what the reference's pipeline object
    offers at /root/reference/model/depthcrafter.py:24-34,80-90."""

    def __init__(self, device_id=0, workspace_bytes=2 << 30, persist_bytes=1 << 30):
        self.lib = load_library()
        self.ctx = self.lib.ug_create(int(device_id), int(workspace_bytes), int(persist_bytes))
        if not self.ctx:
            raise RuntimeError("ug_create failed: " + self.lib.ug_last_error(None).decode())
        self.device_id = device_id
        self.l1_info = None          # j, k, steps, certified of the last eval_depth(alignment="l1")
        self._l1_warned = False

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.ug_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise RuntimeError("libunigeo_hip: " + self.lib.ug_last_error(self.ctx).decode())

    # ---- weights
    def load_state(self, prefix, state):
        for name, arr in state.items():
            a = np.ascontiguousarray(arr)
            if a.dtype == np.float16:
                dt = 0
            elif a.dtype == np.float32:
                dt = 1
            else:
                a = a.astype(np.float32); dt = 1
            shape = (C.c_int64 * max(a.ndim, 1))(*(a.shape if a.ndim else (1,)))
            self._ck(self.lib.ug_load_tensor(self.ctx, (prefix + name).encode(), dt, max(a.ndim, 1), shape, _ptr(a)))

    def bind_unet(self, cfg):
        self._ck(self.lib.ug_bind_unet(self.ctx, C.byref(_unet_c(cfg))))
        self.unet_cfg = cfg

    def bind_vae(self, cfg):
        self._ck(self.lib.ug_bind_vae(self.ctx, C.byref(_vae_c(cfg))))
        self.vae_cfg = cfg

    def bind_clip(self, cfg):
        self._ck(self.lib.ug_bind_clip(self.ctx, C.byref(_clip_c(cfg))))
        self.clip_cfg = cfg

    # ---- StableNormal
    def bind_stablenormal(self, ucfg, vcfg, dcfg):
        self._ck(self.lib.ug_bind_stablenormal(self.ctx, C.byref(_unet_c(ucfg)), C.byref(_vae_c(vcfg)), C.byref(_clip_c(dcfg))))
        self.sn_cfgs = (ucfg, vcfg, dcfg)

    def sn_run(self, images, prompt_embeds, yoso_t, timesteps, ca, cb):
        f = _f32(images); B, H, W, _ = f.shape
        pe = _f32(prompt_embeds).reshape(77, self.sn_cfgs[0].cross_attention_dim)
        ts, a, b = _f32(timesteps), _f32(ca), _f32(cb)
        out = np.empty((B, H, W, 3), np.float32)
        self._ck(self.lib.ug_sn_run(self.ctx, _ptr(f), B, H, W, _ptr(pe), float(yoso_t), int(ts.size), _ptr(ts), _ptr(a), _ptr(b), _ptr(out)))
        return out

    def sn_unet_forward(self, which, sample, t_unet, prompt_embeds, zimg=None, t_ctrl=0.0, dino_tokens=None, use_ctrl=False):
        s = _f32(sample); B, _, h, w = s.shape
        z = None if zimg is None else _f32(zimg)
        d = None if dino_tokens is None else _f32(dino_tokens)
        pe = _f32(prompt_embeds)
        out = np.empty((B, 4, h, w), np.float32)
        self._ck(self.lib.ug_sn_unet_forward(self.ctx, int(which), _ptr(s), _ptr(z), B, h, w, float(t_unet), float(t_ctrl), _ptr(pe), _ptr(d),
                                             int(bool(use_ctrl)), _ptr(out)))
        return out

    def sn_dino(self, images):
        f = _f32(images); B, H, W, _ = f.shape
        dc = self.sn_cfgs[2]; g = dc.image_size // dc.patch_size
        out = np.empty((B, g * g, dc.hidden_size), np.float32)
        self._ck(self.lib.ug_sn_dino(self.ctx, _ptr(f), B, H, W, _ptr(out)))
        return out

    def sn_vae_decode(self, z):
        z = _f32(z); B, _, h, w = z.shape
        out = np.empty((B, 8 * h, 8 * w, 3), np.float32)
        self._ck(self.lib.ug_sn_vae_decode(self.ctx, _ptr(z), B, h, w, _ptr(out)))
        return out

    def resize_bilinear(self, x_bhwc, Ho, Wo, normalise=False):
        """torch F.interpolate(mode="bilinear", antialias=True, align_corners=False) on the device; [B,Hi,Wi,C<=4] f32 -> [B,Ho,Wo,C]."""
        x = _f32(x_bhwc); B, Hi, Wi, Cc = x.shape
        out = np.empty((B, int(Ho), int(Wo), Cc), np.float32)
        self._ck(self.lib.ug_resize_bilinear(self.ctx, _ptr(x), B, Hi, Wi, Cc, int(Ho), int(Wo), int(bool(normalise)), _ptr(out)))
        return out

    def sn_vae_encode(self, img_m11):
        f = _f32(img_m11); B, H, W, _ = f.shape
        out = np.empty((B, 4, H // 8, W // 8), np.float32)
        self._ck(self.lib.ug_sn_vae_encode(self.ctx, _ptr(f), B, H, W, _ptr(out)))
        return out

    # ---- pipeline
    def set_inputs(self, frames, noise_latents, noise_aug, intrinsics=None):
        f = _f32(frames)
        T, H, W, _ = f.shape
        nl, na = _f32(noise_latents).reshape(T, 4, H // 8, W // 8), _f32(noise_aug).reshape(T, 3, H, W)
        k = None if intrinsics is None else _f32(intrinsics).reshape(T, 3, 3)
        self._ck(self.lib.ug_dc_set_inputs(self.ctx, _ptr(f), T, H, W, _ptr(nl), _ptr(na), _ptr(k)))
        self._shape = (T, H, W)

    FRAMES_F32_THWC, FRAMES_U8_TCHW = 0, 1

    def set_inputs_ex(self, frames, noise_latents=None, noise_aug=None, seed=None, intrinsics=None):
        """The opt-in input modes (``ug_dc_set_inputs_ex``).  ``frames``: a uint8 array is planar ``[T,3,H,W]`` (converted to ``x / 255`` on the
        device), anything else float32 channels-last ``[T,H,W,3]``.  Noise: both host arrays, or neither and a ``seed`` (0 <= seed < 2**64) from
        which the device generates both tensors."""
        f = np.asarray(frames)
        if f.dtype == np.uint8:
            f = np.ascontiguousarray(f); fmt = self.FRAMES_U8_TCHW
            if f.ndim != 4 or f.shape[1] != 3:
                raise ValueError("uint8 frames must be planar [T,3,H,W]")
            T, _, H, W = f.shape
        else:
            f = _f32(f); fmt = self.FRAMES_F32_THWC
            if f.ndim != 4 or f.shape[3] != 3:
                raise ValueError("float frames must be channels-last [T,H,W,3]")
            T, H, W, _ = f.shape
        if (noise_latents is None) != (noise_aug is None):
            raise ValueError("pass both noise arrays, or neither (noise from the seed)")
        if (noise_latents is None) == (seed is None):
            raise ValueError("pass either the two noise arrays or a seed")
        nl = na = None
        if noise_latents is not None:
            nl, na = _f32(noise_latents).reshape(T, 4, H // 8, W // 8), _f32(noise_aug).reshape(T, 3, H, W)
        elif not 0 <= int(seed) < 1 << 64:
            raise ValueError("the noise seed must be in [0, 2**64)")
        k = None if intrinsics is None else _f32(intrinsics).reshape(T, 3, 3)
        self._ck(self.lib.ug_dc_set_inputs_ex(self.ctx, _ptr(f), fmt, T, H, W, _ptr(nl), _ptr(na), int(seed or 0), _ptr(k)))
        self._shape = (T, H, W)

    def get_noise(self):
        """(noise_latents [T,4,H/8,W/8], noise_aug [T,3,H,W]) resident for the current inputs, host arrays or generated from a seed."""
        T, H, W = self._shape
        nl, na = np.empty((T, 4, H // 8, W // 8), np.float32), np.empty((T, 3, H, W), np.float32)
        self._ck(self.lib.ug_dc_get_noise(self.ctx, _ptr(nl), _ptr(na)))
        return nl, na

    def op_philox_u32(self, seed, stream, block_offset, nblocks):
        out = np.empty((int(nblocks), 4), np.uint32)
        self._ck(self.lib.ug_op_philox_u32(self.ctx, int(seed), int(stream), int(block_offset), int(nblocks), _ptr(out)))
        return out

    def op_randn(self, seed, stream, element_offset, n, guard=0, fill=np.nan):
        """n normals of (seed, stream) from ``element_offset`` on, followed by ``guard`` words that went to the device holding ``fill`` and
        came back from it (untouched by the kernel when it writes exactly n values)."""
        buf = np.full(int(n) + int(guard), fill, np.float32)
        self._ck(self.lib.ug_op_randn(self.ctx, int(seed), int(stream), int(element_offset), int(n), int(guard), _ptr(buf)))
        return buf

    def op_u8_to_frames(self, frames_tchw):
        f = np.ascontiguousarray(frames_tchw, dtype=np.uint8)
        T, _, H, W = f.shape
        out = np.empty((T, H, W, 3), np.float32)
        self._ck(self.lib.ug_op_u8_to_frames(self.ctx, _ptr(f), T, H, W, _ptr(out)))
        return out

    def run(self, steps, decode_chunk=8, with_normals=False, window=0, overlap=0):
        if window:
            self._ck(self.lib.ug_dc_run_windows(self.ctx, int(steps), int(decode_chunk), int(bool(with_normals)), int(window), int(overlap)))
        else:
            self._ck(self.lib.ug_dc_run(self.ctx, int(steps), int(decode_chunk), int(bool(with_normals))))

    def set_guidance(self, guidance_scale=1.0):
        """Classifier-free guidance scale of the following runs (``guidance_scale`` of the pipeline call): <= 1 is the unguided path; a
        value that is not finite raises."""
        self._ck(self.lib.ug_dc_set_guidance(self.ctx, float(guidance_scale)))

    def set_coscheduled(self, on=True):
        """This context shares the GPU with another clip in flight (a second context): drop the heuristics that fill the last round of one kernel at the
        price of extra launches / work (fused feed-forward tail split, last-round fill factor of the tile planner)."""
        self._ck(self.lib.ug_set_coscheduled(self.ctx, int(bool(on))))

    def set_concurrency(self, lanes=2):
        """Independent chunks (VAE encode / decode chunks, CLIP tower) in flight on separate HIP streams; 1 = serial.  Bit-identical outputs."""
        self._ck(self.lib.ug_set_concurrency(self.ctx, int(lanes)))

    def set_vae_encode_fp32(self, on=True):
        """True (default) = the reference's float32 VAE encoder (force_upcast); False = fp16 storage like the decoder."""
        self._ck(self.lib.ug_set_vae_encode_fp32(self.ctx, int(bool(on))))

    def bench_flash(self, B, H, S, variant=0, iters=20):
        out = np.zeros(1, np.float32)
        self._ck(self.lib.ug_bench_flash(self.ctx, B, H, S, int(variant), int(iters), _ptr(out)))
        return float(out[0])

    def bench_ff(self, M, C, fused=True, iters=20):
        out = np.zeros(1, np.float32)
        self._ck(self.lib.ug_bench_ff(self.ctx, int(M), int(C), int(bool(fused)), int(iters), _ptr(out)))
        return float(out[0])

    def set_ff_fused(self, on=True, prenorm=True):
        """Fused GEGLU feed-forward kernel of the narrow transformer blocks (on) and its LayerNorm inside the kernel (prenorm); A/B aid."""
        self._ck(self.lib.ug_set_ff_fused(self.ctx, (1 if on else 0) | (2 if on and prenorm else 0)))

    def tune_ff(self, variant=0):
        """Per-context A/B aid: fused feed-forward kernel form, 0 = cross-tile prefetch (default), 1 = without it."""
        self._ck(self.lib.ug_tune_ff(self.ctx, int(variant)))

    def tune_flash(self, variant=-1):
        """Per-context test aid: flash-attention variant mask of this context's launches (-1 = default 23)."""
        self._ck(self.lib.ug_tune_flash(self.ctx, int(variant)))

    def op_ln_ff(self, X, gamma, beta, W1, b1, W2, b2, addvec=None, rows_per_vec=1, eps=1e-5, c0=1.0, c1=1.0, mode=2):
        X = _f32(X); M, Cc = X.shape
        av = None if addvec is None else _f32(addvec)
        out = np.empty((M, Cc), np.float32)
        self._ck(self.lib.ug_op_ln_ff(self.ctx, _ptr(X), M, Cc, _ptr(_f32(gamma)), _ptr(_f32(beta)), float(eps), _ptr(av), int(rows_per_vec),
                                      _ptr(_f32(W1)), _ptr(_f32(b1)), _ptr(_f32(W2)), _ptr(_f32(b2)), float(c0), float(c1), int(mode), _ptr(out)))
        return out

    def op_ff(self, X, W1, b1, W2, b2, R1=None, c0=1.0, c1=1.0, fused=True):
        X = _f32(X); M, Cc = X.shape
        r = None if R1 is None else _f32(R1)
        out = np.empty((M, Cc), np.float32)
        self._ck(self.lib.ug_op_ff(self.ctx, _ptr(X), M, Cc, _ptr(_f32(W1)), _ptr(_f32(b1)), _ptr(_f32(W2)), _ptr(_f32(b2)), _ptr(r),
                                   float(c0), float(c1), int(bool(fused)), _ptr(out)))
        return out

    def op_ff_ex(self, X, W1, b1, W2, b2=None, R1=None, R2=None, c0=1.0, c1=1.0, c2=1.0, gamma=None, beta=None, eps=1e-5, addvec=None, rows_per_vec=1,
                 mode=2, max_wg=0, in_guard=0, out=None, out_guard=0):
        """Every launch form of the feed-forward (ug_op_ff_ex in include/unigeo_hip_test.h).  R1: None, the string "x" (the stream X itself) or an
        array; X, R1 and R2 hold M + in_guard rows and, with in_guard > 0, addvec one vector more than ceil(M / rows_per_vec).  out [M + out_guard, C]
        (None: zeros) goes to the device as given.  Returns (the whole output buffer as the device holds it, (grid, most tiles walked by one
        workgroup, rows the fused kernel took))."""
        X = _f32(X); Cc = X.shape[1]; M = X.shape[0] - in_guard
        r1_is_x = isinstance(R1, str)
        assert not r1_is_x or R1 == "x", R1
        r1 = None if R1 is None or r1_is_x else _f32(R1)
        r2 = None if R2 is None else _f32(R2)
        av = None if addvec is None else _f32(addvec)
        assert M >= 1 and all(a is None or a.shape == X.shape for a in (r1, r2)), (X.shape, in_guard)
        if av is not None:
            assert av.shape == ((M + rows_per_vec - 1) // rows_per_vec + (1 if in_guard else 0), Cc), av.shape
        buf = np.zeros((M + out_guard, Cc), np.float32) if out is None else np.array(out, dtype=np.float32, order="C")
        assert buf.shape == (M + out_guard, Cc), buf.shape
        opt = lambda a: None if a is None else _f32(a)
        info = (C.c_int * 3)()
        self._ck(self.lib.ug_op_ff_ex(self.ctx, _ptr(X), M, Cc, _ptr(_f32(W1)), _ptr(_f32(b1)), _ptr(_f32(W2)), _ptr(opt(b2)), _ptr(r1), int(r1_is_x), _ptr(r2),
                                      float(c0), float(c1), float(c2), _ptr(opt(gamma)), _ptr(opt(beta)), float(eps), _ptr(av), int(rows_per_vec),
                                      int(mode), int(max_wg), int(in_guard), int(out_guard), _ptr(buf), info))
        return buf, tuple(info)

    def set_fp8_linears(self, on=True):
        """MX-fp8 matrix instructions for the UNet transformers' linear layers (BASELINE configs[4]); reduced precision, default off."""
        self._ck(self.lib.ug_set_fp8_linears(self.ctx, int(bool(on))))

    def op_linear_mx8(self, A, W, bias=None, geglu=False, return_quant=False):
        A, W = _f32(A), _f32(W); M, K = A.shape; N = W.shape[0]
        b = None if bias is None else _f32(bias)
        out = np.empty((M, N // 2 if geglu else N), np.float32)
        a8 = np.empty((M, K), np.uint8) if return_quant else None
        sa = np.empty((K // 128, (M + 255) // 256 * 256), np.uint32) if return_quant else None
        self._ck(self.lib.ug_op_linear_mx8(self.ctx, _ptr(A), M, K, _ptr(W), N, _ptr(b), int(bool(geglu)), _ptr(out), _ptr(a8), _ptr(sa)))
        return (out, a8, sa) if return_quant else out

    def op_quant_mx8_ex(self, x, M, K, q, s):
        """launch_quant_mx8 alone (ug_op_quant_mx8_ex in include/unigeo_hip_test.h).  x [M + guard, ldx] float, q [M + guard, K] uint8 and s [K // 128, ld_s]
        uint32 go to the device as given (ldx, guard and ld_s are read off the shapes); returns new arrays with the device's whole q and s."""
        x = _f32(x); q = np.array(q, dtype=np.uint8, order="C"); s = np.array(s, dtype=np.uint32, order="C")
        guard = x.shape[0] - M
        assert guard >= 0 and q.shape == (M + guard, K) and s.ndim == 2 and s.shape[0] == K // 128, (x.shape, q.shape, s.shape)
        self._ck(self.lib.ug_op_quant_mx8_ex(self.ctx, _ptr(x), int(M), int(K), x.shape[1], guard, s.shape[1], _ptr(q), _ptr(s)))
        return q, s

    def op_linear_mx8_ex(self, A, W, bias=None, R1=None, R2=None, c0=1.0, c1=1.0, c2=1.0, act=0, geglu=False, out=None, guard=0, ldo=None, poison=True,
                         return_quant=False):
        """Both quantiser launches and the MX-fp8 GEMM with its whole epilogue (ug_op_linear_mx8_ex).  R1 [M, ldr1] / R2 [M, ldr2] and out [M + guard, ldo]
        (None: zeros, ldo columns) go to the device as given.  Returns (the whole output buffer as the device holds it, (tile pick, group_m))
        (+ the A bytes and its scale dwords [K // 128, round_up(M, 256)] with return_quant)."""
        A, W = _f32(A), _f32(W); M, K = A.shape; N = W.shape[0]; nout = N // 2 if geglu else N
        opt = lambda a: None if a is None else _f32(a)
        b, r1, r2 = opt(bias), opt(R1), opt(R2)
        buf = np.zeros((M + guard, ldo or nout), np.float32) if out is None else np.array(out, dtype=np.float32, order="C")
        assert buf.ndim == 2 and buf.shape[0] == M + guard and all(r is None or (r.ndim == 2 and r.shape[0] == M) for r in (r1, r2)), buf.shape
        a8 = np.empty((M, K), np.uint8) if return_quant else None
        sa = np.empty((K // 128, (M + 255) // 256 * 256), np.uint32) if return_quant else None
        plan = (C.c_int * 2)()
        self._ck(self.lib.ug_op_linear_mx8_ex(self.ctx, _ptr(A), M, K, _ptr(W), N, _ptr(b), _ptr(r1), 0 if r1 is None else r1.shape[1], _ptr(r2),
                                              0 if r2 is None else r2.shape[1], float(c0), float(c1), float(c2), int(act), int(bool(geglu)), buf.shape[1],
                                              int(guard), int(bool(poison)), _ptr(buf), _ptr(a8), _ptr(sa), plan))
        return (buf, tuple(plan), a8, sa) if return_quant else (buf, tuple(plan))

    def op_linear_engine(self, A, W, K=None, bias=None, gamma=None, beta=None, eps=1e-5, R1=None, R2=None, c0=1.0, c1=1.0, c2=1.0, act=0, geglu=False,
                         out=None, guard=0, ldo=None):
        """One linear layer through the engine's quant_lin() and linear() - with gamma / beta, ln_linear() and its pre-quantised hand-off - over a 0xFF-filled
        workspace (ug_op_linear_engine); the path follows the context's fp8_linears.  A [M, lda] with lda >= K (K: W's columns).  Returns (the whole
        output buffer as the device holds it, (MX-fp8 weight bound, MX GEMM ran, the LayerNorm wrote the quantised activation))."""
        A, W = _f32(A), _f32(W); M, lda = A.shape; N, Kw = W.shape; nout = N // 2 if geglu else N
        assert K is None or K == Kw
        opt = lambda a: None if a is None else _f32(a)
        b, g, bt, r1, r2 = opt(bias), opt(gamma), opt(beta), opt(R1), opt(R2)
        buf = np.zeros((M + guard, ldo or nout), np.float32) if out is None else np.array(out, dtype=np.float32, order="C")
        assert buf.ndim == 2 and buf.shape[0] == M + guard and all(r is None or (r.ndim == 2 and r.shape[0] == M) for r in (r1, r2)), buf.shape
        info = (C.c_int * 3)()
        self._ck(self.lib.ug_op_linear_engine(self.ctx, _ptr(A), M, lda, _ptr(W), N, Kw, _ptr(b), _ptr(g), _ptr(bt), float(eps), _ptr(r1),
                                              0 if r1 is None else r1.shape[1], _ptr(r2), 0 if r2 is None else r2.shape[1], float(c0), float(c1), float(c2),
                                              int(act), int(bool(geglu)), buf.shape[1], int(guard), _ptr(buf), info))
        return buf, tuple(info)

    def run_traced(self, steps, decode_chunk=8, with_normals=False):
        """ug_dc_run with the latents after every Euler step copied out: returns [steps, T, 4, h, w] float32."""
        T, H, W = self._shape
        tr = np.zeros((int(steps), T, H // 8, W // 8, 4), np.float32)
        self._ck(self.lib.ug_dc_set_trace(self.ctx, _ptr(tr), int(steps)))
        try:
            self.run(steps, decode_chunk, with_normals)
        finally:
            self.lib.ug_dc_set_trace(self.ctx, None, 0)
        return tr.transpose(0, 1, 4, 2, 3)

    def get_outputs(self, frames=True, depth=True, normals=False):
        T, H, W = self._shape
        fo = np.empty((T, H, W, 3), np.float32) if frames else None
        do = np.empty((T, H, W), np.float32) if depth else None
        no = np.empty((T, H, W, 3), np.float32) if normals else None
        self._ck(self.lib.ug_dc_get_outputs(self.ctx, _ptr(fo), _ptr(do), _ptr(no)))
        return fo, do, no

    def get_disparity(self):
        """The normalised disparity of the last run -> ``[T, H, W]`` float32 in [0, 1] (``ug_dc_get_disparity``): the
        ``x`` the resident depth ``1 / (x + 0.1)`` was made from, produced on the device from the resident frames when it is asked for."""
        shape = getattr(self, "_shape", None)
        if shape is None:
            raise RuntimeError("get_disparity: no clip has been run on this engine")
        out = np.empty(shape, np.float32)
        self._ck(self.lib.ug_dc_get_disparity(self.ctx, _ptr(out)))
        return out

    def device_ptrs(self):
        """(frames, depth, normals) device addresses of the resident outputs + their shapes."""
        f, d, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._ck(self.lib.ug_dc_device_ptrs(self.ctx, C.byref(f), C.byref(d), C.byref(n)))
        T, H, W = self._shape
        return {"frames": (f.value, (T, H, W, 3)), "depth": (d.value, (T, H, W)), "normals": (n.value, (T, H, W, 3))}

    # ---- stages
    def clip_embed(self, frames):
        f = _f32(frames); T, H, W, _ = f.shape
        out = np.empty((T, self.clip_cfg.projection_dim), np.float32)
        self._ck(self.lib.ug_clip_embed(self.ctx, _ptr(f), T, H, W, _ptr(out)))
        return out

    def vae_encode(self, video_m11_thwc):
        f = _f32(video_m11_thwc); T, H, W, _ = f.shape
        out = np.empty((T, self.vae_cfg.latent_channels, H // 8, W // 8), np.float32)
        self._ck(self.lib.ug_vae_encode(self.ctx, _ptr(f), T, H, W, _ptr(out)))
        return out

    def vae_decode(self, z_tchw):
        z = _f32(z_tchw); T, _, h, w = z.shape
        out = np.empty((T, h * 8, w * 8, 3), np.float32)
        self._ck(self.lib.ug_vae_decode(self.ctx, _ptr(z), T, h, w, _ptr(out)))
        return out

    def unet_forward(self, sample_tchw, timestep, clip_emb):
        s = _f32(sample_tchw); T, _, h, w = s.shape
        e = _f32(clip_emb)
        out = np.empty((T, self.unet_cfg.out_channels, h, w), np.float32)
        self._ck(self.lib.ug_unet_forward(self.ctx, _ptr(s), T, h, w, float(timestep), _ptr(e), _ptr(out)))
        return out

    def unet_forward_pair(self, sample_a, emb_a, sample_b, emb_b, timestep):
        """ONE batched UNet pass over two videos (samples [T,Cin,h,w], embeddings [T,cross]) -> (out_a, out_b), each [T,Cout,h,w]."""
        a, b = _f32(sample_a), _f32(sample_b)
        ea, eb = _f32(emb_a), _f32(emb_b)
        T, _, h, w = a.shape
        if b.shape != a.shape or ea.shape != eb.shape or ea.shape[0] != T:
            raise ValueError("unet_forward_pair: both videos need the same shapes")
        oa = np.empty((T, self.unet_cfg.out_channels, h, w), np.float32)
        ob = np.empty_like(oa)
        self._ck(self.lib.ug_unet_forward_pair(self.ctx, _ptr(a), _ptr(ea), _ptr(b), _ptr(eb), T, h, w, float(timestep), _ptr(oa), _ptr(ob)))
        return oa, ob

    def normals_from_depth(self, depth, intrinsics):
        d = _f32(depth); T, H, W = d.shape
        k = _f32(intrinsics).reshape(T, 3, 3)
        out = np.empty((T, H, W, 3), np.float32)
        self._ck(self.lib.ug_normals_from_depth(self.ctx, _ptr(d), _ptr(k), T, H, W, _ptr(out)))
        return out

    # ---- metrics on device (pred=None: use the resident outputs of the last run)
    DEPTH_KEYS = ["Abs Rel", "Sq Rel", "RMSE", "Log RMSE", "delta < 1.", "delta < 1.25", "delta < 1.25^2", "delta < 1.25^3"]
    NORMAL_KEYS = ["normal mean", "normal median", "normal rmse", "angle < 5", "angle < 7.5", "angle < 11.25", "angle < 22.5", "angle < 30"]

    def eval_depth(self, gt, mask=None, pred=None, max_depth=80.0, alignment="lstsq", pre_clip_min=None, pre_clip_max=None,
                   post_clip_min=None, post_clip_max=None, return_error_map=False, space="depth", disp_clip_min=None):
        """Depth metrics on the device -> ``(res, (s, t))``, with ``return_error_map=True`` ``(res, (s, t), error_map)``.
        ``alignment``: "lstsq" | "median" | "scale" | "metric" (``ug_eval_depth_ex``) | "l1" (the exact L1 scale and
        shift; ``l1_info``, None until then, holds j, k, steps, certified, and an uncertified fit warns once); the clip bounds clamp
        the prediction before / after the alignment; ``max_depth=None`` keeps every ``gt > 0``.  The defaults call ``ug_eval_depth``.
        ``space="disparity"`` (``ug_eval_depth_ex2``): the prediction (``pred=None``: the resident DISPARITY of the last
        run, ``get_disparity()``) is aligned against ``1 / gt``, inverted, and scored against ``gt``; ``disp_clip_min`` floors the aligned
        disparity before the inversion."""
        if alignment not in DEPTH_ALIGNMENTS:
            raise ValueError(f"alignment must be one of {sorted(DEPTH_ALIGNMENTS)}, not {alignment!r}")
        from .harness.metrics import check_disp_clip_min
        check_disp_clip_min(space, disp_clip_min, "eval_depth")
        g = _f32(gt); n = g.size
        p = None if pred is None else _f32(pred)
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
        out = np.zeros(11, np.float64)
        clips = (pre_clip_min, pre_clip_max, post_clip_min, post_clip_max)
        emap = None
        if space == "depth" and alignment == "lstsq" and max_depth is not None and not return_error_map and all(c is None for c in clips):
            self._ck(self.lib.ug_eval_depth(self.ctx, _ptr(p), _ptr(g), _ptr(m), n, float(max_depth), _ptr(out)))
        else:
            o = _depth_opts(alignment, max_depth, clips)
            emap = np.empty(g.shape, np.float32) if return_error_map else None
            if space == "depth":
                self._ck(self.lib.ug_eval_depth_ex(self.ctx, _ptr(p), _ptr(g), _ptr(m), n, C.byref(o), _ptr(out), _ptr(emap)))
            else:
                o2 = DepthEvalOpts2C(o, DEPTH_ALIGN_DISPARITY, float("nan") if disp_clip_min is None else float(disp_clip_min))
                self._ck(self.lib.ug_eval_depth_ex2(self.ctx, _ptr(p), _ptr(g), _ptr(m), n, C.byref(o2), _ptr(out), _ptr(emap)))
            if alignment == "l1":
                info = (C.c_long * 4)()
                self._ck(self.lib.ug_eval_depth_l1_info(self.ctx, info))
                self.l1_info = dict(zip(("j", "k", "steps", "certified"), (int(v) for v in info)))
                if not self.l1_info["certified"] and not self._l1_warned:
                    self._l1_warned = True
                    warnings.warn("eval_depth(alignment='l1'): the descent met a cap (64 steps or 4096 tied points) and returned an uncertified "
                                  "vertex; further such fits on this engine are not reported", RuntimeWarning, stacklevel=2)
        res = dict(zip(self.DEPTH_KEYS, out[:8].tolist()))
        res["valid_pixels"] = int(out[8])
        if return_error_map:
            return res, (float(out[9]), float(out[10])), emap
        return res, (float(out[9]), float(out[10]))

    def eval_depth_global(self, gt_depth, gt_radius, cam2world, intrinsics, mask=None, pred=None, max_depth=80.0, pre_clip_min=None,
                          pre_clip_max=None, post_clip_min=None, post_clip_max=None, return_radius_map=False):
        """Depth metrics in global coordinates on the device (``ug_eval_depth_global``) -> ``(res, (s_r, t_r),
        (s_d, t_d))``, with ``return_radius_map=True`` also the aligned radius map ``[T,H,W]``.  ``gt_depth`` / ``gt_radius`` ``[T,H,W]``,
        ``cam2world`` ``[T,4,4]``, ``intrinsics`` ``[T,3,3]``; ``pred=None`` evaluates the resident depth; least squares only."""
        g = _f32(gt_depth)
        if g.ndim != 3:
            raise ValueError("eval_depth_global: gt_depth must be [T,H,W]")
        T, H, W = g.shape
        gr = _f32(gt_radius).reshape(T, H, W)
        pose, k = _f32(cam2world).reshape(T, 4, 4), _f32(intrinsics).reshape(T, 3, 3)
        p = None if pred is None else _f32(pred).reshape(T, H, W)
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8)).reshape(T, H, W)
        o = _depth_opts("lstsq", max_depth, (pre_clip_min, pre_clip_max, post_clip_min, post_clip_max))
        out = np.zeros(13, np.float64)
        rmap = np.empty(g.shape, np.float32) if return_radius_map else None
        self._ck(self.lib.ug_eval_depth_global(self.ctx, _ptr(p), _ptr(g), _ptr(gr), _ptr(pose), _ptr(k), _ptr(m), T, H, W, C.byref(o), _ptr(out),
                                               _ptr(rmap)))
        res = dict(zip(self.DEPTH_KEYS, out[:8].tolist()))
        res["valid_pixels"] = int(out[8])
        fits = (float(out[9]), float(out[10])), (float(out[11]), float(out[12]))
        return (res, *fits, rmap) if return_radius_map else (res, *fits)

    def eval_tae(self, gt, cam2world, intrinsics, fit, mask=None, pred=None, max_depth=80.0, stride=1, space="depth", disp_clip_min=None,
                 post_clip_min=None, post_clip_max=None, return_maps=False):
        """Temporal alignment error on the device (``ug_eval_tae``) -> the dict of
        ``harness.temporal.temporal_alignment_error``: ``TAE``, ``TAE pairs``, ``TAE pairs total``, ``TAE pixels`` and, with
        ``return_maps=True``, ``pair_values`` ``[P,2]``, ``warp`` and ``err`` ``[P,H,W]``.  ``fit`` is the ``(s, t)`` the clip's ``eval_depth``
        returned; ``pred=None`` scores the resident depth of the last run, with ``space="disparity"`` its resident disparity.  The relative
        poses are built on the host by ``harness.temporal.relative_poses``, the function the mirror uses."""
        from .harness.metrics import check_disp_clip_min
        from .harness.temporal import relative_poses
        check_disp_clip_min(space, disp_clip_min, "eval_tae")
        g = _f32(gt)
        if g.ndim != 3:
            raise ValueError("eval_tae: gt must be [T,H,W]")
        T, H, W = g.shape
        stride = int(stride)
        p = None if pred is None else _f32(pred).reshape(T, H, W)
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8)).reshape(T, H, W)
        k = _f32(intrinsics).reshape(T, 3, 3)
        rel = np.ascontiguousarray(relative_poses(cam2world, stride) if stride >= 1 else np.zeros((0, 3, 4)), dtype=np.float64)
        P = rel.shape[0]
        relbuf = rel if P else np.zeros((1, 3, 4), np.float64)      # never a NULL pointer: T <= stride is a result, not an error
        nan = float("nan")
        o = TaeOptsC(float(fit[0]), float(fit[1]), DEPTH_ALIGN_DISPARITY if space == "disparity" else 0,
                     *[nan if v is None else float(v) for v in (disp_clip_min, post_clip_min, post_clip_max, max_depth)], stride)
        out = np.zeros(4, np.float64)
        pairs = np.zeros((P, 2), np.float64) if return_maps else None
        warp = np.zeros((P, H, W), np.float32) if return_maps else None
        err = np.zeros((P, H, W), np.float32) if return_maps else None
        self._ck(self.lib.ug_eval_tae(self.ctx, _ptr(p), _ptr(g), _ptr(m), _ptr(k), _ptr(relbuf), T, H, W, C.byref(o), _ptr(out), _ptr(pairs),
                                      _ptr(warp), _ptr(err)))
        res = {"TAE": float(out[0]), "TAE pairs": int(out[1]), "TAE pairs total": int(out[2]), "TAE pixels": int(out[3])}
        if return_maps:
            res.update({"pair_values": pairs, "warp": warp, "err": err})
        return res

    # ---- point-cloud evaluation on device
    PCD_KEYS = ["acc", "comp", "nc1", "nc2", "acc_med", "comp_med", "nc1_med", "nc2_med"]

    def pcd_world_points(self, gt_depth, cam2world, intrinsics, pred=None, max_depth=80.0, pre_clip_min=None, pre_clip_max=None,
                         post_clip_min=None, post_clip_max=None, return_points=True):
        """World points of the (resident, ``pred=None``) depth (``ug_pcd_world_points``) -> ``(pts float32 [T,H,W,3] or None, (s_d, t_d))``;
        the points stay on the device for ``eval_pcd(None, ...)``."""
        g = _f32(gt_depth)
        if g.ndim != 3:
            raise ValueError("pcd_world_points: gt_depth must be [T,H,W]")
        T, H, W = g.shape
        pose, k = _f32(cam2world).reshape(T, 4, 4), _f32(intrinsics).reshape(T, 3, 3)
        p = None if pred is None else _f32(pred).reshape(T, H, W)
        o = _depth_opts("lstsq", max_depth, (pre_clip_min, pre_clip_max, post_clip_min, post_clip_max))
        fit = np.zeros(2, np.float32)
        pts = np.empty((T, H, W, 3), np.float32) if return_points else None
        self._ck(self.lib.ug_pcd_world_points(self.ctx, _ptr(p), _ptr(g), _ptr(pose), _ptr(k), T, H, W, C.byref(o), _ptr(fit), _ptr(pts)))
        return pts, (float(fit[0]), float(fit[1]))

    def eval_pcd(self, pred_pts, gt_pts, masks, rgbs=None, threshold=0.1, downsample_num=-1, seed=0, knn=30, max_iteration=30,
                 return_clouds=True, sampling="random", search="brute", fscore_thresholds=(), voxel_sizes=()):
        """``pcd_evaluation`` of ``harness/metrics.py`` on the device (``ug_eval_pcd``) -> the same dict.  ``pred_pts=None`` evaluates the
        points that the last ``pcd_world_points`` left resident.  The sampled positions are drawn here, as the host mirror draws them;
        ``sampling="fps"`` picks them on the device instead (``ug_eval_pcd_fps``) and adds ``pred_idx`` / ``gt_idx``.
        ``search="grid"`` (``ug_eval_pcd_ex`` with ``UG_PCD_SEARCH_GRID``) finds the same neighbours through a uniform
        grid - every entry of the dict is bit-equal - and adds ``search_stats``.  ``fscore_thresholds`` / ``voxel_sizes`` (DESIGN.md section
        32), when either is not empty, send the call through ``ug_eval_pcd_scores`` and add the keys of the mirror: ``prec@t`` / ``recall@t`` /
        ``fscore@t`` with ``score_counts``, ``iou@v`` with ``voxel_counts``; the device returns the integer counts, the values are formed
        from them by the mirror's own functions."""
        from .harness.metrics import PCD_MAX_THRESHOLDS, PCD_MAX_VOXEL_SIZES, pcd_sample_indices, pcd_score_names
        taus, tau_names = pcd_score_names(fscore_thresholds, "fscore_thresholds", PCD_MAX_THRESHOLDS)
        vsizes, vsize_names = pcd_score_names(voxel_sizes, "voxel_sizes", PCD_MAX_VOXEL_SIZES)
        score = None
        if taus or vsizes:
            so = PcdScoreOptsC(len(taus), (C.c_double * 8)(*taus), len(vsizes), (C.c_double * 4)(*vsizes))
            score = (so, np.zeros((8, 2), np.int64), np.zeros((4, 6), np.int64), tau_names, vsize_names)
        if sampling not in ("random", "fps"):
            raise ValueError(f"eval_pcd: sampling must be 'random' or 'fps', not {sampling!r}")
        if search not in ("brute", "grid"):
            raise ValueError(f"eval_pcd: search must be 'brute' or 'grid', not {search!r}")
        grid = search == "grid"
        stats = np.zeros(8, np.int64)
        g = _f32(gt_pts).reshape(-1, 3)
        m = np.ascontiguousarray((np.asarray(masks).reshape(-1) > 0).astype(np.uint8))
        p = None if pred_pts is None else _f32(pred_pts).reshape(-1, 3)
        n_mask = int(m.sum())
        if sampling == "fps":
            ns = downsample_num if 0 < downsample_num < n_mask else n_mask
            o = PcdOptsC(float(threshold), int(max_iteration), int(knn))
            out = np.zeros(32, np.float64)
            pc = np.empty((ns, 3), np.float32) if return_clouds else None
            gc = np.empty((ns, 3), np.float32) if return_clouds else None
            ip, ig = np.empty(ns, np.int64), np.empty(ns, np.int64)
            if score is not None:
                self._ck(self.lib.ug_eval_pcd_scores(self.ctx, _ptr(p), _ptr(g), _ptr(m), m.size, None, int(downsample_num), C.byref(o),
                                                     self.PCD_FPS | (self.PCD_SEARCH_GRID if grid else 0), _ptr(out), _ptr(pc), _ptr(gc), _ptr(ip),
                                                     _ptr(ig), _ptr(stats), C.byref(score[0]), _ptr(score[1]), _ptr(score[2])))
            elif grid:
                self._ck(self.lib.ug_eval_pcd_ex(self.ctx, _ptr(p), _ptr(g), _ptr(m), m.size, None, int(downsample_num), C.byref(o),
                                                 self.PCD_FPS | self.PCD_SEARCH_GRID, _ptr(out), _ptr(pc), _ptr(gc), _ptr(ip), _ptr(ig), _ptr(stats)))
            else:
                self._ck(self.lib.ug_eval_pcd_fps(self.ctx, _ptr(p), _ptr(g), _ptr(m), m.size, int(downsample_num), C.byref(o), _ptr(out), _ptr(pc),
                                                  _ptr(gc), _ptr(ip), _ptr(ig)))
            res = self._pcd_result(out, stats if grid else None, score)
            res.update(pred_idx=ip, gt_idx=ig)
            if return_clouds:
                col = np.zeros((n_mask, 3), np.float32) if rgbs is None else _f32(rgbs).reshape(-1, 3)[m > 0]
                res.update(pred_pcd=(pc, col[ip]), gt_pcd=(gc, col[ig]))
            return res
        idx = pcd_sample_indices(n_mask, downsample_num, seed)
        idx = None if idx is None else np.ascontiguousarray(idx.astype(np.int64))
        ns = n_mask if idx is None else len(idx)
        o = PcdOptsC(float(threshold), int(max_iteration), int(knn))
        out = np.zeros(32, np.float64)
        pc = np.empty((ns, 3), np.float32) if return_clouds else None
        gc = np.empty((ns, 3), np.float32) if return_clouds else None
        if score is not None:
            self._ck(self.lib.ug_eval_pcd_scores(self.ctx, _ptr(p), _ptr(g), _ptr(m), m.size, _ptr(idx), 0 if idx is None else len(idx), C.byref(o),
                                                 self.PCD_SEARCH_GRID if grid else 0, _ptr(out), _ptr(pc), _ptr(gc), None, None, _ptr(stats),
                                                 C.byref(score[0]), _ptr(score[1]), _ptr(score[2])))
        elif grid:
            self._ck(self.lib.ug_eval_pcd_ex(self.ctx, _ptr(p), _ptr(g), _ptr(m), m.size, _ptr(idx), 0 if idx is None else len(idx), C.byref(o),
                                             self.PCD_SEARCH_GRID, _ptr(out), _ptr(pc), _ptr(gc), None, None, _ptr(stats)))
        else:
            self._ck(self.lib.ug_eval_pcd(self.ctx, _ptr(p), _ptr(g), _ptr(m), m.size, _ptr(idx), 0 if idx is None else len(idx), C.byref(o),
                                          _ptr(out), _ptr(pc), _ptr(gc)))
        res = self._pcd_result(out, stats if grid else None, score)
        if return_clouds:
            keep = m > 0
            col = np.zeros((n_mask, 3), np.float32) if rgbs is None else _f32(rgbs).reshape(-1, 3)[keep]
            col = col if idx is None else col[idx]
            res.update(pred_pcd=(pc, col), gt_pcd=(gc, col.copy()))
        return res

    PCD_FPS, PCD_SEARCH_GRID = 1, 2      # UG_PCD_FPS, UG_PCD_SEARCH_GRID
    SEARCH_STAT_KEYS = ["settled", "leftover", "gt_cells", "gt_max_cell", "pred_cells", "pred_max_cell", "workspace_peak_bytes"]

    def _pcd_result(self, out, stats=None, score=None):
        res = dict(zip(self.PCD_KEYS, out[:8].tolist()))
        if score is not None:
            from .harness.metrics import pcd_threshold_values, pcd_voxel_values
            _, sc, vc, tau_names, vsize_names = score
            if tau_names:
                res.update(pcd_threshold_values(tau_names, sc[:len(tau_names)], int(out[8])))
                res["score_counts"] = sc[:len(tau_names)].copy()
            if vsize_names:
                res.update(pcd_voxel_values(vsize_names, vc[:len(vsize_names)]))
                res["voxel_counts"] = vc[:len(vsize_names)].copy()
        if stats is not None:
            res["search_stats"] = dict(zip(self.SEARCH_STAT_KEYS, (int(v) for v in stats[:7])))
        res.update(n_points=int(out[8]), icp_iterations=int(out[9]), icp_fitness=float(out[10]), icp_rmse=float(out[11]),
                   transformation=out[12:28].reshape(4, 4).copy(), pred_scale=float(out[28]), gt_scale=float(out[29]),
                   pred_shift_z=float(out[30]), gt_shift_z=float(out[31]))
        return res

    # ---- focal, poses and depth from world point maps
    def pointmap_focal(self, pts0, pp=None):
        """``pointmap_focal`` of ``harness/pointmap.py`` on the device (``ug_pointmap_focal``): the Weiszfeld focal of the point map ``[H,W,3]`` of
        the frame whose camera is the world frame; ``pp`` defaults to ``(W/2, H/2)``."""
        p = _f32(pts0)
        if p.ndim != 3 or p.shape[-1] != 3:
            raise ValueError("pointmap_focal: pts0 must be [H,W,3]")
        H, W = p.shape[:2]
        cx, cy = (W / 2.0, H / 2.0) if pp is None else (float(pp[0]), float(pp[1]))
        out = np.zeros(1, np.float64)
        self._ck(self.lib.ug_pointmap_focal(self.ctx, _ptr(p), H, W, cx, cy, _ptr(out)))
        return float(out[0])

    def pointmap_poses(self, pts, focal, pp=None, mask=None, reproj_px=None, max_iter=None, max_rounds=None):
        """``pointmap_poses`` of ``harness/pointmap.py`` on the device (``ug_pointmap_poses``) -> the same dict: ``extrinsics [T,4,4]`` float64
        world to camera, ``depth [T,H,W]`` float32, ``focal``, per frame ``n_inliers``, ``iterations``, ``reproj_rms``, and ``inliers [T,H,W]``.
        Options left at ``None`` take the library's defaults (``ug_pointmap_opts_default``)."""
        p = _f32(pts)
        if p.ndim != 4 or p.shape[-1] != 3:
            raise ValueError("pointmap_poses: pts must be [T,H,W,3]")
        T, H, W = p.shape[:3]
        cx, cy = (W / 2.0, H / 2.0) if pp is None else (float(pp[0]), float(pp[1]))
        m = None if mask is None else np.ascontiguousarray((np.asarray(mask).reshape(T, H, W) > 0).astype(np.uint8))
        o = PointmapOptsC()
        self.lib.ug_pointmap_opts_default(C.byref(o))
        if reproj_px is not None:
            o.reproj_px = float(reproj_px)
        if max_iter is not None:
            o.max_iter = int(max_iter)
        if max_rounds is not None:
            o.max_rounds = int(max_rounds)
        ext, depth = np.zeros((T, 4, 4), np.float64), np.zeros((T, H, W), np.float32)
        stats, inl = np.zeros((T, 3), np.float64), np.zeros((T, H, W), np.uint8)
        self._ck(self.lib.ug_pointmap_poses(self.ctx, _ptr(p), _ptr(m), T, H, W, float(focal), cx, cy, C.byref(o), _ptr(ext), _ptr(depth),
                                            _ptr(stats), _ptr(inl)))
        return {"extrinsics": ext, "depth": depth, "focal": float(focal), "n_inliers": stats[:, 0].astype(np.int64),
                "iterations": stats[:, 1].astype(np.int64), "reproj_rms": stats[:, 2].copy(), "inliers": inl > 0}

    def op_pcd_fps(self, pts, k):
        """Farthest-point sampling of a float32 cloud ``[n,3]`` alone (``pcd_fps_indices`` of ``harness/metrics.py``) ->
        ``(idx int64 [k], sel_dist float32 [k])``."""
        p = _f32(pts).reshape(-1, 3)
        k = int(k)
        idx, sel = np.empty(max(k, 0), np.int64), np.empty(max(k, 0), np.float32)
        self._ck(self.lib.ug_op_pcd_fps(self.ctx, _ptr(p), len(p), k, _ptr(idx), _ptr(sel)))
        return idx, sel

    def op_pcd_nn(self, query, target, transformation=None):
        """Nearest target of every query (float64 ``[n,3]``; the query first moved by the 4x4) -> ``(distance float64, index int32)``."""
        q = np.ascontiguousarray(np.asarray(query, np.float64).reshape(-1, 3)); t = np.ascontiguousarray(np.asarray(target, np.float64).reshape(-1, 3))
        T = None if transformation is None else np.ascontiguousarray(np.asarray(transformation, np.float64).reshape(4, 4))
        idx, dist = np.empty(len(q), np.int32), np.empty(len(q), np.float64)
        self._ck(self.lib.ug_op_pcd_nn(self.ctx, _ptr(q), len(q), _ptr(t), len(t), _ptr(T), _ptr(idx), _ptr(dist)))
        return dist, idx

    GRID_STAT_KEYS = ["settled", "leftover", "cells", "max_cell"]

    def op_pcd_nn_grid(self, query, target, transformation=None):
        """``op_pcd_nn`` through the uniform grid -> ``(distance, index, stats)``: the same bytes, and how many
        queries the grid settled / left to the brute-force kernels, its cells and the points in its fullest cell."""
        q = np.ascontiguousarray(np.asarray(query, np.float64).reshape(-1, 3)); t = np.ascontiguousarray(np.asarray(target, np.float64).reshape(-1, 3))
        T = None if transformation is None else np.ascontiguousarray(np.asarray(transformation, np.float64).reshape(4, 4))
        idx, dist, st = np.empty(len(q), np.int32), np.empty(len(q), np.float64), np.zeros(4, np.int64)
        self._ck(self.lib.ug_op_pcd_nn_grid(self.ctx, _ptr(q), len(q), _ptr(t), len(t), _ptr(T), _ptr(idx), _ptr(dist), _ptr(st)))
        return dist, idx, dict(zip(self.GRID_STAT_KEYS, (int(v) for v in st)))

    def op_pcd_knn_normals_grid(self, pts, knn=30):
        """``op_pcd_knn_normals`` through the uniform grid -> ``(neighbours, normals, stats)``: the same bytes."""
        p = np.ascontiguousarray(np.asarray(pts, np.float64).reshape(-1, 3))
        nbr, nrm, st = np.empty((len(p), min(knn, len(p))), np.int32), np.empty((len(p), 3), np.float64), np.zeros(4, np.int64)
        self._ck(self.lib.ug_op_pcd_knn_normals_grid(self.ctx, _ptr(p), len(p), int(knn), _ptr(nbr), _ptr(nrm), _ptr(st)))
        return nbr, nrm, dict(zip(self.GRID_STAT_KEYS, (int(v) for v in st)))

    def op_voxel_set(self, a, b, voxel_size, capacity_log2=0):
        """The voxel set of two float64 clouds alone (``ug_op_voxel_set``) -> int64 ``[6]``: cells of ``a``, of ``b``, of
        both, of either, skipped points of ``a``, of ``b`` - the ``counts`` of ``harness.metrics.voxel_iou``.  ``capacity_log2`` forces the
        table size (0: the production rule); a table too small raises."""
        a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, 3)); b = np.ascontiguousarray(np.asarray(b, np.float64).reshape(-1, 3))
        out = np.zeros(6, np.int64)
        self._ck(self.lib.ug_op_voxel_set(self.ctx, _ptr(a) if len(a) else None, len(a), _ptr(b) if len(b) else None, len(b), float(voxel_size),
                                          int(capacity_log2), _ptr(out)))
        return out

    def op_pcd_select(self, values, k):
        """The exact k-th smallest (from 0) of a float32 or float64 array."""
        v = np.ascontiguousarray(np.asarray(values).reshape(-1))
        if v.dtype not in (np.float32, np.float64):
            raise ValueError("op_pcd_select: float32 or float64 values")
        out = np.zeros(1, v.dtype)
        self._ck(self.lib.ug_op_pcd_select(self.ctx, _ptr(v), int(v.dtype == np.float64), v.size, int(k), _ptr(out)))
        return out[0]

    def op_pcd_knn_normals(self, pts, knn=30):
        """KNN lists and covariance normals of a float64 cloud -> ``(neighbours int32 [n, min(knn, n)], normals float64 [n,3])``."""
        p = np.ascontiguousarray(np.asarray(pts, np.float64).reshape(-1, 3))
        nbr, nrm = np.empty((len(p), min(knn, len(p))), np.int32), np.empty((len(p), 3), np.float64)
        self._ck(self.lib.ug_op_pcd_knn_normals(self.ctx, _ptr(p), len(p), int(knn), _ptr(nbr), _ptr(nrm)))
        return nbr, nrm

    def op_l1_fit(self, gt, pred=None, max_depth=80.0, pre_clip_min=None, pre_clip_max=None):
        """The exact L1 scale-and-shift fit alone (``ug_op_l1_fit``) -> ``(s, t, info)`` as ``harness.metrics.l1_fit``
        of the clamped prediction and ``gt`` over the valid ``gt``; ``pred=None`` fits the resident depth."""
        g = _f32(gt).reshape(-1)
        p = None if pred is None else _f32(pred).reshape(-1)
        nan = float("nan")
        o = DepthEvalOptsC(DEPTH_ALIGNMENTS["l1"], nan if max_depth is None else float(max_depth),
                           nan if pre_clip_min is None else float(pre_clip_min), nan if pre_clip_max is None else float(pre_clip_max), nan, nan)
        st = np.zeros(2, np.float64); info = (C.c_long * 4)()
        self._ck(self.lib.ug_op_l1_fit(self.ctx, _ptr(p), _ptr(g), g.size, C.byref(o), _ptr(st), info))
        return float(st[0]), float(st[1]), dict(zip(("j", "k", "steps", "certified"), (int(v) for v in info)))

    def op_masked_median(self, pred, gt, max_depth=80.0, pre_clip_min=None, pre_clip_max=None):
        """The exact masked selection alone -> (lower median of clamp(pred), lower median of gt, count) over the valid ``gt``."""
        p, g = _f32(pred).reshape(-1), _f32(gt).reshape(-1)
        med = np.zeros(2, np.float32); cnt = C.c_long(0)
        nan = float("nan")
        self._ck(self.lib.ug_op_masked_median(self.ctx, _ptr(p), _ptr(g), p.size, nan if max_depth is None else float(max_depth),
                                              nan if pre_clip_min is None else float(pre_clip_min),
                                              nan if pre_clip_max is None else float(pre_clip_max), _ptr(med), C.byref(cnt)))
        return med[0], med[1], int(cnt.value)

    def eval_normal(self, gt, mask=None, pred=None):
        g = _f32(gt); n = g.size // 3
        p = None if pred is None else _f32(pred)
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
        out = np.zeros(8, np.float64)
        self._ck(self.lib.ug_eval_normal(self.ctx, _ptr(p), _ptr(g), _ptr(m), n, _ptr(out)))
        return dict(zip(self.NORMAL_KEYS, out.tolist()))

    # ---- visualisation panels on device (depth / normals None: the resident outputs of the last run)
    VIS_RGB_NONE, VIS_RGB_HOST, VIS_RGB_RESIDENT = 0, 1, 2

    def vis_depth_range(self, depth=None):
        """(vmin, vmax) of the depth as two ``np.float32``, NaN ignored, ``(0, 0)`` for all-NaN or empty input (``ug_vis_depth_range``)."""
        out = np.zeros(2, np.float32)
        if depth is None:
            T, H, W = self._shape
            self._ck(self.lib.ug_vis_depth_range(self.ctx, None, T * H * W, _ptr(out)))
        else:
            d = _f32(depth)
            self._ck(self.lib.ug_vis_depth_range(self.ctx, _ptr(d), d.size, _ptr(out)))
        return out[0], out[1]

    def vis_panels(self, vmin, vmax, lut, depth=None, normals=None, rgbs=None, cbar=None):
        """The reference's visualisation panels composed on the device (``ug_vis_panels``) -> uint8 ``[T,H,Wp,3]``: rgb | normals | depth through
        ``lut`` (float32 ``[256,3]``) over ``vmin..vmax`` | 5 black columns | ``cbar`` (float32 ``[H,Wc,3]``).  ``rgbs``: ``None`` (no rgb section),
        ``"resident"`` (the input frames of the last ``set_inputs*``) or an array ``[T,H,W,3]`` in [0,1]; ``cbar=None`` ends the panel after the
        depth section."""
        d = None if depth is None else _f32(depth)
        n = None if normals is None else _f32(normals)
        if d is not None:
            shape = d.shape
        elif n is not None:
            shape = n.shape[:3]
        else:
            shape = self._shape
        if len(shape) != 3 or (n is not None and n.shape != (*shape, 3)):
            raise ValueError("vis_panels: depth must be [T,H,W] and normals [T,H,W,3]")
        T, H, W = shape
        r, mode = None, self.VIS_RGB_NONE
        if isinstance(rgbs, str):
            if rgbs != "resident":
                raise ValueError('vis_panels: rgbs must be None, "resident" or an array')
            mode = self.VIS_RGB_RESIDENT
        elif rgbs is not None:
            r, mode = _f32(rgbs), self.VIS_RGB_HOST
            if r.shape != (T, H, W, 3):
                raise ValueError("vis_panels: rgbs must be [T,H,W,3]")
        l = _f32(lut)
        if l.shape != (256, 3):
            raise ValueError("vis_panels: lut must be [256,3]")
        cb, Wc = None, 0
        if cbar is not None:
            cb = _f32(cbar)
            if cb.ndim != 3 or cb.shape[0] != H or cb.shape[2] != 3:
                raise ValueError("vis_panels: cbar must be [H,Wc,3]")
            Wc = cb.shape[1]
        Wp = (W if mode else 0) + 2 * W + (5 + Wc if cb is not None else 0)
        out = np.empty((T, H, Wp, 3), np.uint8)
        self._ck(self.lib.ug_vis_panels(self.ctx, _ptr(d), _ptr(n), _ptr(r), mode, T, H, W, float(vmin), float(vmax), _ptr(l), _ptr(cb), Wc, _ptr(out)))
        return out

    # ---- ScanNet++ clip preparation on device
    def prep_resize_frames(self, frames_u8, Ho, Wo, row_taps=None, col_taps=None):
        """The loader's anti-aliased input resize (``harness.scannetpp._resize(order=1, anti_alias=True)``) on the device
        (``ug_prep_resize_frames``): uint8 ``[T,Hi,Wi,3]`` -> float32 ``[T,3,Ho,Wo]``, 0..255.  The per-axis tap tables ``(idx [n_out,K],
        w [n_out,K])`` come from ``harness.scannetpp.resize_taps`` unless given."""
        from .harness.scannetpp import resize_taps
        f = np.asarray(frames_u8)
        if f.dtype != np.uint8 or f.ndim != 4 or f.shape[3] != 3:
            raise ValueError("prep_resize_frames: frames must be uint8 [T,Hi,Wi,3]")
        f = np.ascontiguousarray(f)
        T, Hi, Wi, _ = f.shape
        Ho, Wo = int(Ho), int(Wo)
        tabs = []
        for taps, n_in, n_out in ((row_taps, Hi, Ho), (col_taps, Wi, Wo)):
            idx, w = resize_taps(n_in, n_out) if taps is None else taps
            idx, w = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(w, dtype=np.float64)
            if idx.ndim != 2 or idx.shape != w.shape or idx.shape[0] != n_out:
                raise ValueError("prep_resize_frames: a tap table must be (idx, w), both [n_out, K]")
            tabs.append((idx, w))
        (ri, rw), (ci, cw) = tabs
        out = np.empty((T, 3, Ho, Wo), np.float32)
        self._ck(self.lib.ug_prep_resize_frames(self.ctx, _ptr(f), T, Hi, Wi, Ho, Wo, _ptr(ri), _ptr(rw), ri.shape[1], _ptr(ci), _ptr(cw),
                                                ci.shape[1], _ptr(out)))
        return out

    def prep_gt(self, depth_u16, normals_u8, intrinsics, cam2key, row_idx, col_idx, depth_divisor=1000.0, max_depth=80.0, depth_f64=False,
                zoomed=None):
        """The loader's ground truth at the picked source pixels on the device (``ug_prep_gt_ex``) -> ``(cam_normal, cam_coord, world_normal,
        world_coord, mask)``, float32 ``[T,3,Ho,Wo]`` x 4 and ``[T,Ho,Wo]``.  ``depth_u16`` ``[T,Hi,Wi]``, ``normals_u8`` ``[T,Hi,Wi,3]`` or
        ``None`` (zero normals), ``intrinsics`` ``[T,3,3]``, ``cam2key`` ``[T,4,4]`` (source camera -> key view), ``row_idx`` ``[Ho]`` /
        ``col_idx`` ``[Wo]`` the source row / column of every output row / column (``harness.scannetpp.resize_pick``).  ``depth_f64`` keeps the
        depth in float64 through the back-projection (``UG_PREP_DEPTH_F64``); ``zoomed`` says whether the host's order-0 zoom ran on the
        targets (``UG_PREP_ZOOMED``), ``None`` = it ran iff ``(Ho, Wo) != (Hi, Wi)``, the rule of ``ug_prep_gt``."""
        d = np.asarray(depth_u16)
        if d.dtype != np.uint16 or d.ndim != 3:
            raise ValueError("prep_gt: depth must be uint16 [T,Hi,Wi]")
        d = np.ascontiguousarray(d)
        T, Hi, Wi = d.shape
        n = None
        if normals_u8 is not None:
            n = np.asarray(normals_u8)
            if n.dtype != np.uint8 or n.shape != (T, Hi, Wi, 3):
                raise ValueError("prep_gt: normals must be uint8 [T,Hi,Wi,3]")
            n = np.ascontiguousarray(n)
        k, m = _f32(intrinsics).reshape(T, 3, 3), _f32(cam2key).reshape(T, 4, 4)
        ri, ci = np.ascontiguousarray(row_idx, dtype=np.int32).reshape(-1), np.ascontiguousarray(col_idx, dtype=np.int32).reshape(-1)
        Ho, Wo = ri.size, ci.size
        cn, cc, wn, wc = (np.empty((T, 3, Ho, Wo), np.float32) for _ in range(4))
        mask = np.empty((T, Ho, Wo), np.float32)
        if zoomed is None:
            zoomed = (Ho, Wo) != (Hi, Wi)
        flags = (PREP_DEPTH_F64 if depth_f64 else 0) | (PREP_ZOOMED if zoomed else 0)
        self._ck(self.lib.ug_prep_gt_ex(self.ctx, _ptr(d), float(depth_divisor), _ptr(n), _ptr(k), _ptr(m), T, Hi, Wi, _ptr(ri), Ho, _ptr(ci), Wo,
                                        float(max_depth), _ptr(cn), _ptr(cc), _ptr(wn), _ptr(wc), _ptr(mask), flags))
        return cn, cc, wn, wc, mask

    def prep_gt_normals(self, depth_u16, intrinsics, cam2key, row_idx, col_idx, depth_divisor=1000.0, max_depth=80.0, depth_f64=False,
                        zoomed=None, radius=2, edge=0.05, min_count=None):
        """Normals fitted from the depth at the picked source pixels on the device (``ug_prep_gt_normals``) ->
        ``(cam_normal, world_normal, normal_mask)``, float32 ``[T,3,Ho,Wo]`` x 2 and ``[T,Ho,Wo]``: bit-equal to
        ``harness.normals.fit_normals`` on the full native frame followed by ``world_normals`` and the pick.  The depth, the cameras, the
        tables, ``depth_f64`` and ``zoomed`` are ``prep_gt``'s; ``radius`` (1..8), ``edge`` (``None``: the edge test off) and ``min_count``
        (``None``: the majority of the window) are ``fit_normals``'s, checked here the way it checks them."""
        from .harness.normals import check_fit_options
        radius, edge, min_count = check_fit_options(radius, edge, min_count, "prep_gt_normals")
        d = np.asarray(depth_u16)
        if d.dtype != np.uint16 or d.ndim != 3:
            raise ValueError("prep_gt_normals: depth must be uint16 [T,Hi,Wi]")
        d = np.ascontiguousarray(d)
        T, Hi, Wi = d.shape
        k, m = _f32(intrinsics).reshape(T, 3, 3), _f32(cam2key).reshape(T, 4, 4)
        ri, ci = np.ascontiguousarray(row_idx, dtype=np.int32).reshape(-1), np.ascontiguousarray(col_idx, dtype=np.int32).reshape(-1)
        Ho, Wo = ri.size, ci.size
        cn, wn = (np.empty((T, 3, Ho, Wo), np.float32) for _ in range(2))
        nm = np.empty((T, Ho, Wo), np.float32)
        if zoomed is None:
            zoomed = (Ho, Wo) != (Hi, Wi)
        flags = (PREP_DEPTH_F64 if depth_f64 else 0) | (PREP_ZOOMED if zoomed else 0)
        o = GtNormalsOptsC(radius, -1.0 if edge is None else edge, min_count)
        self._ck(self.lib.ug_prep_gt_normals(self.ctx, _ptr(d), float(depth_divisor), _ptr(k), _ptr(m), T, Hi, Wi, _ptr(ri), Ho, _ptr(ci), Wo,
                                             float(max_depth), C.byref(o), _ptr(cn), _ptr(wn), _ptr(nm), flags))
        return cn, wn, nm

    def prep_register_depth(self, depth_u16, opts=None, invalid="keep"):
        """Raw depth warped into the colour camera on the device (``ug_prep_register_depth``): uint16 ``[T,H,W]`` or
        ``[H,W]`` -> uint16 of the same shape, bit-equal to ``harness.rgbd.register_depth``.  ``opts``: a ``harness.rgbd.RegisterOpts``
        (``None``: the library's defaults, the 7-Scenes calibration); ``invalid="drop"`` sets ``UG_REG_DROP_SENTINEL``."""
        from .harness.rgbd import REGISTER_INVALID
        if invalid not in REGISTER_INVALID:
            raise ValueError(f"prep_register_depth: invalid must be one of {list(REGISTER_INVALID)}, not {invalid!r}")
        d = np.asarray(depth_u16)
        if d.dtype != np.uint16 or d.ndim not in (2, 3):
            raise ValueError("prep_register_depth: depth must be uint16 [T,H,W] or [H,W]")
        clip = np.ascontiguousarray(d if d.ndim == 3 else d[None])
        T, H, W = clip.shape
        o = RegisterOptsC()
        self.lib.ug_register_opts_default(C.byref(o))
        if opts is not None:
            m = np.asarray(opts.src2dst, np.float64).reshape(-1)
            if m.size != 12:
                raise ValueError("prep_register_depth: src2dst holds 12 numbers, the top three rows of the transform")
            o.src_focal, o.dst_focal, o.divisor, o.max_valid = float(opts.src_focal), float(opts.dst_focal), float(opts.divisor), float(opts.max_valid)
            o.src2dst[:] = m.tolist()
        o.flags = REG_DROP_SENTINEL if invalid == "drop" else 0
        out = np.empty((T, H, W), np.uint16)
        self._ck(self.lib.ug_prep_register_depth(self.ctx, _ptr(clip), T, H, W, C.byref(o), _ptr(out)))
        return out if d.ndim == 3 else out[0]

    def prep_render_mesh(self, verts, faces, cam_to_world, K, H, W, masks=None, znear=None, zfar=None, with_index=True):
        """A triangle mesh rendered from T cameras on the device (``ug_prep_render_mesh``): the arguments and the result
        ``(depth_mm uint16 [T,H,W], normal uint8 [T,H,W,3], tri_index int32 [T,H,W])`` of ``harness.render.render_mesh``, byte for byte.
        ``cam_to_world`` is inverted here with ``numpy.linalg.inv``, as the mirror does; ``znear`` / ``zfar`` ``None``: the library's defaults
        (0.05, 20).  ``with_index=False`` passes ``tri_index = NULL`` and returns ``None`` in its place."""
        from .harness.render import check_masks, check_render_args, intrinsics4, world2cam_from
        o = RenderOptsC()
        self.lib.ug_render_opts_default(C.byref(o))
        if znear is not None:
            o.znear = float(znear)
        if zfar is not None:
            o.zfar = float(zfar)
        m = world2cam_from(cam_to_world)
        T = len(m)
        v, f, m, k = check_render_args(verts, faces, m, intrinsics4(K, T), H, W, o.znear, o.zfar, who="prep_render_mesh")
        mk = check_masks(masks, T, H, W, who="prep_render_mesh")
        depth = np.empty((T, H, W), np.uint16); normal = np.empty((T, H, W, 3), np.uint8)
        index = np.empty((T, H, W), np.int32) if with_index else None
        self._ck(self.lib.ug_prep_render_mesh(self.ctx, _ptr(v), len(v), _ptr(f), len(f), _ptr(m), _ptr(k), T, H, W, _ptr(mk), C.byref(o),
                                              _ptr(depth), _ptr(normal), _ptr(index)))
        return depth, normal, index

    # ---- ops (parity tests)
    def op_linear(self, A, W, bias=None, R1=None, c0=1.0, c1=1.0, act=0, geglu=False):
        A, W = _f32(A), _f32(W); M, K = A.shape; N = W.shape[0]
        b = None if bias is None else _f32(bias); r = None if R1 is None else _f32(R1)
        out = np.empty((M, N // 2 if geglu else N), np.float32)
        self._ck(self.lib.ug_op_linear(self.ctx, _ptr(A), M, K, _ptr(W), N, _ptr(b), _ptr(r), c0, c1, act, int(geglu), _ptr(out)))
        return out

    def op_conv(self, x0, weight, bias=None, x1=None, kt=1, k=3, stride=1, pad_t=1, pad_l=1, ups=1):
        x0 = _f32(x0); T, H, W, C0 = x0.shape
        x1a = None if x1 is None else _f32(x1); C1 = 0 if x1 is None else x1a.shape[-1]
        w = _f32(weight); O = w.shape[0]
        b = None if bias is None else _f32(bias)
        Ho, Wo = H * ups // stride, W * ups // stride
        out = np.empty((T, Ho, Wo, O), np.float32)
        self._ck(self.lib.ug_op_conv(self.ctx, _ptr(x0), C0, _ptr(x1a), C1, T, H, W, _ptr(w), _ptr(b), O, kt, k,
                                     stride, pad_t, pad_l, ups, _ptr(out)))
        return out

    def op_groupnorm(self, x0, G, eps, gamma, beta, x1=None, temporal=False, silu=False):
        x0 = _f32(x0); T, HW, C0 = x0.shape
        x1a = None if x1 is None else _f32(x1); C1 = 0 if x1 is None else x1a.shape[-1]
        out = np.empty((T, HW, C0 + C1), np.float32)
        self._ck(self.lib.ug_op_groupnorm(self.ctx, _ptr(x0), C0, _ptr(x1a), C1, T, HW, G, eps, int(temporal), int(silu),
                                          _ptr(_f32(gamma)), _ptr(_f32(beta)), _ptr(out)))
        return out

    def op_conv_gn(self, x, w, b, G, eps, gamma, beta, res=None, kt=1, k=3, temporal=False):
        """conv (+ residual) -> GroupNorm + SiLU with the statistics from a pass over the tensor / from the convolution's epilogue:
        (conv_out, y_pass, y_epi, rows_per_statistics_block)."""
        x = _f32(x); T, H, W, C0 = x.shape; w = _f32(w); O = w.shape[0]
        r = None if res is None else _f32(res)
        co = np.empty((T, H, W, O), np.float32); y1 = np.empty_like(co); y2 = np.empty_like(co)
        rb = C.c_int(0)
        self._ck(self.lib.ug_op_conv_gn(self.ctx, _ptr(x), C0, T, H, W, _ptr(w), _ptr(None if b is None else _f32(b)), _ptr(r), O, kt, k, G, eps, int(temporal),
                                        _ptr(_f32(gamma)), _ptr(_f32(beta)), _ptr(co), _ptr(y1), _ptr(y2), C.byref(rb)))
        return co, y1, y2, rb.value

    def op_layernorm(self, x, eps, gamma, beta, addvec=None, rows_per_vec=1):
        x = _f32(x); M, Cc = x.shape
        out = np.empty((M, Cc), np.float32); xout = np.empty((M, Cc), np.float32)
        av = None if addvec is None else _f32(addvec)
        self._ck(self.lib.ug_op_layernorm(self.ctx, _ptr(x), M, Cc, eps, _ptr(_f32(gamma)), _ptr(_f32(beta)), _ptr(av),
                                          rows_per_vec, _ptr(out), _ptr(xout)))
        return (out, xout) if addvec is not None else out

    def op_groupnorm_ex(self, x0, G, eps, gamma, beta, x1=None, temporal=False, silu=False, mode=0, guard=0, guard_fill=0.0):
        """GroupNorm with the launch scheme forced (mode 1 / 2 / 4 / 6; 0 = the launcher picks).  The output buffer has guard extra rows and is filled with
        guard_fill before it goes to the device.  Returns (out [T*HW + guard, C] as the device holds it, plan) with plan = (scheme launched, slab threads,
        slab VMAX, chunks per frame) - zeros where they do not apply."""
        x0 = _f32(x0); T, HW, C0 = x0.shape
        x1a = None if x1 is None else _f32(x1); C1 = 0 if x1 is None else x1a.shape[-1]
        out = np.full((T * HW + guard, C0 + C1), guard_fill, np.float32)
        plan = (C.c_int * 4)()
        self._ck(self.lib.ug_op_groupnorm_ex(self.ctx, _ptr(x0), C0, _ptr(x1a), C1, T, HW, G, eps, int(temporal), int(silu),
                                             _ptr(_f32(gamma)), _ptr(_f32(beta)), int(mode), int(guard), _ptr(out), plan))
        return out, tuple(plan)

    def op_layernorm_ex(self, x, eps, gamma, beta, addvec=None, rows_per_vec=1, row0=0, form=0, guard=0, guard_fill=0.0, fp8=False):
        """LayerNorm with the pre-add's row offset, the kernel forced (form 1: one wave per row also at C = 320 / 640 / 1280) and reported.  addvec holds
        ceil((M + row0) / rows_per_vec) vectors.  Returns a dict: out [M + guard, C] as the device holds it (filled with guard_fill before the launch),
        form (L of ln40_kernel<L>, or -VPL of ln_kernel<VPL>), xout (with addvec), y8 [M, C] uint8 and s8 [C/128, round_up(M,256)] uint32 (with fp8)."""
        x = _f32(x); M, Cc = x.shape
        out = np.full((M + guard, Cc), guard_fill, np.float32)
        av = None if addvec is None else _f32(addvec)
        if av is not None:
            assert av.shape == ((M + row0 + rows_per_vec - 1) // rows_per_vec, Cc), av.shape
        xout = None if av is None else np.empty((M, Cc), np.float32)
        y8 = np.empty((M, Cc), np.uint8) if fp8 else None
        s8 = np.empty((Cc // 128, (M + 255) // 256 * 256), np.uint32) if fp8 else None
        form_out = C.c_int(0)
        self._ck(self.lib.ug_op_layernorm_ex(self.ctx, _ptr(x), M, Cc, eps, _ptr(_f32(gamma)), _ptr(_f32(beta)), _ptr(av), int(rows_per_vec), int(row0),
                                             int(form), int(guard), _ptr(out), _ptr(xout), _ptr(y8), _ptr(s8), C.byref(form_out)))
        return {"out": out, "form": form_out.value, "xout": xout, "y8": y8, "s8": s8}

    def op_flash_attn(self, qkv, B, H, S):
        q = _f32(qkv); out = np.empty((B * S, H * 64), np.float32)
        self._ck(self.lib.ug_op_flash_attn(self.ctx, _ptr(q), B, H, S, _ptr(out)))
        return out

    def op_temporal_attn(self, qkv, T, HW, H):
        q = _f32(qkv); out = np.empty((T * HW, H * 64), np.float32)
        self._ck(self.lib.ug_op_temporal_attn(self.ctx, _ptr(q), T, HW, H, _ptr(out)))
        return out

    def op_flash_cross_attn(self, q, kv, out_inout, B, H, S, Sk=0, kv_shared=False, guard=0):
        """The d = 64 flash attention with its own key count and row strides (the cross-attention launch form).  q [B*S, ldq], kv [(1 if kv_shared
        else B) * (Sk or S) + guard, ldkv] with K in columns [0, H*64) and V in [H*64, 2*H*64), out_inout [B*S + guard, ldo]: all three are uploaded as
        they are (guard rows and surplus columns too) and a new array with the device's whole out_inout is returned."""
        q, kv, out = _f32(q), _f32(kv), np.array(out_inout, dtype=np.float32, order="C")
        keys = Sk if Sk > 0 else S
        assert q.ndim == kv.ndim == out.ndim == 2 and q.shape[0] == B * S and out.shape[0] == B * S + guard, (q.shape, kv.shape, out.shape)
        assert Sk < 0 or kv.shape[0] == (1 if kv_shared else B) * keys + guard, kv.shape
        self._ck(self.lib.ug_op_flash_cross_attn(self.ctx, _ptr(q), _ptr(kv), B, H, S, Sk, int(bool(kv_shared)), q.shape[1], kv.shape[1], out.shape[1],
                                                 int(guard), _ptr(out)))
        return out

    def op_temporal_attn_nv(self, qkv, nv, T, HW, H):
        q = _f32(qkv); out = np.empty((nv * T * HW, H * 64), np.float32)
        assert q.shape == (nv * T * HW, 3 * H * 64), q.shape
        self._ck(self.lib.ug_op_temporal_attn_nv(self.ctx, _ptr(q), nv, T, HW, H, _ptr(out)))
        return out

    def op_attention_generic(self, qkv, B, S, H, d):
        q = _f32(qkv); out = np.empty((B * S, H * d), np.float32)
        self._ck(self.lib.ug_op_attention_generic(self.ctx, _ptr(q), B, S, H, d, _ptr(out)))
        return out

    def op_flash_attn_dh(self, qkv, B, S, H, d):
        q = _f32(qkv); out = np.empty((B * S, H * d), np.float32)
        self._ck(self.lib.ug_op_flash_attn_dh(self.ctx, _ptr(q), B, S, H, d, _ptr(out)))
        return out

    # the attention paths for head dims other than 64 and the batched GEMMs under the four-launch one (tests/test_attn_general_gpu.py)
    def _attn_general_buffers(self, qkv, out_inout, B, S, guard):
        q, out = _f32(qkv), np.array(out_inout, dtype=np.float32, order="C")
        assert q.ndim == out.ndim == 2 and q.shape[0] == out.shape[0] == B * S + guard, (q.shape, out.shape)
        return q, out

    def op_flash_attn_dh_ex(self, qkv, out_inout, B, S, H, d, guard=0):
        """The fused self-attention for head dims other than 64.  qkv [B*S + guard, ld] with Q | K | V in columns [0, 3*H*d), out_inout [B*S + guard, ldo]:
        both are uploaded as they are (guard rows and surplus columns too) and a new array with the device's whole out_inout is returned."""
        q, out = self._attn_general_buffers(qkv, out_inout, B, S, guard)
        self._ck(self.lib.ug_op_flash_attn_dh_ex(self.ctx, _ptr(q), B, S, H, d, q.shape[1], out.shape[1], int(guard), _ptr(out)))
        return out

    def op_attention_generic_ex(self, qkv, out_inout, B, S, H, d, guard=0):
        """The four-launch attention (Q K^T batched GEMM, row softmax, V transpose, P V batched GEMM) on the same buffers.  Returns (out as the device
        holds it, plan) with plan = ((tile config, split factor) of Q K^T, ... of P V)."""
        q, out = self._attn_general_buffers(qkv, out_inout, B, S, guard)
        plan = (C.c_int * 4)()
        self._ck(self.lib.ug_op_attention_generic_ex(self.ctx, _ptr(q), B, S, H, d, q.shape[1], out.shape[1], int(guard), _ptr(out), plan))
        return out, ((plan[0], plan[1]), (plan[2], plan[3]))

    def op_gemm_batched(self, A, lda, sA, W, ldw, sW, M, N, K, batch, nb_inner, out_inout, ldo, sO, c0=1.0, out_f32=True):
        """One batched GEMM as the four-launch attention runs its two: Out[b] = c0 * A[b] W[b]^T, batch b at element offset (b // nb_inner) * s[0] +
        (b % nb_inner) * s[1] of the flat buffers A, W (fp16 on the device) and out_inout (float32 or fp16 on the device; uploaded as given, returned
        whole).  Returns (out, (tile config, split factor))."""
        A, W, out = _f32(A).ravel(), _f32(W).ravel(), np.array(out_inout, dtype=np.float32, order="C").ravel()
        plan = (C.c_int * 2)()
        self._ck(self.lib.ug_op_gemm_batched(self.ctx, _ptr(A), int(lda), int(sA[0]), int(sA[1]), _ptr(W), int(ldw), int(sW[0]), int(sW[1]), M, N, K,
                                             batch, nb_inner, c0, int(bool(out_f32)), int(ldo), int(sO[0]), int(sO[1]), A.size, W.size, out.size,
                                             _ptr(out), plan))
        return out, (plan[0], plan[1])

    # the float32-grade VAE encoder's kernels: float32 in / out, inputs not rounded to fp16 (tests/test_wide_gpu.py)
    def op_split_pair(self, x):
        x = _f32(x); M, Cc = x.shape
        hi = np.empty((M, Cc), np.float32); lo = np.empty((M, Cc), np.float32)
        self._ck(self.lib.ug_op_split_pair(self.ctx, _ptr(x), M, Cc, _ptr(hi), _ptr(lo)))
        return hi, lo

    def op_gn32_pair(self, x, G, eps, gamma, beta, silu=False):
        x = _f32(x); T, HW, Cc = x.shape
        hi = np.empty((T, HW, Cc), np.float32); lo = np.empty((T, HW, Cc), np.float32)
        self._ck(self.lib.ug_op_gn32_pair(self.ctx, _ptr(x), T, HW, Cc, G, eps, int(silu), _ptr(_f32(gamma)), _ptr(_f32(beta)), _ptr(hi), _ptr(lo)))
        return hi, lo

    def op_conv_wide(self, x, weight, bias=None, res=None, res_in_place=False, k=3, stride=1, pad_t=1, pad_l=1):
        x = _f32(x); T, H, W, Cc = x.shape
        w = _f32(weight); O = w.shape[0]
        b = None if bias is None else _f32(bias); r = None if res is None else _f32(res)
        out = np.empty((T, H // stride, W // stride, O), np.float32)
        self._ck(self.lib.ug_op_conv_wide(self.ctx, _ptr(x), T, H, W, Cc, _ptr(w), _ptr(b), O, _ptr(r), int(bool(res_in_place)), k, stride, pad_t, pad_l, _ptr(out)))
        return out

    # one convolution through the product's own binding (bind_conv) and launch (conv()) code (tests/test_conv_bound_gpu.py)
    def op_bind_conv(self, weight, bias=None, upsampler=False):
        """weight [O, I, kt, k, k] bound on the device.  Returns a dict: w [O, kt*k*k*cinp] (the bound Conv::w, fp16 widened to float32), wphase
        [4, O, 4*cinp] or None (the sub-pixel phase weights of an upsampler), cinp, kchunk (1: both are in the chunk-major K order)."""
        w = _f32(weight); O, I, kt, k, _ = w.shape
        b = None if bias is None else _f32(bias)
        cinp = (I + 7) // 8 * 8
        wo = np.empty((O, kt * k * k * cinp), np.float32); wp = np.full((4, O, 4 * cinp), np.nan, np.float32)
        info = (C.c_int * 3)()
        self._ck(self.lib.ug_op_bind_conv(self.ctx, _ptr(w), _ptr(b), I, O, kt, k, int(bool(upsampler)), _ptr(wo), _ptr(wp), info))
        assert info[0] == cinp, (info[0], cinp)
        return {"w": wo, "wphase": wp if info[2] else None, "cinp": info[0], "kchunk": info[1]}

    def op_conv_bound(self, x0, weight, bias=None, x1=None, stride=1, pad_t=1, pad_l=1, ups=1, upsampler=False, R1=None, c0=1.0, c1=1.0, act=0,
                      ldo=0, guard=0, fill=0.0):
        """weight [O, I, kt, k, k] bound on the device and launched by the engine's conv() on x0 [T,H,W,C0] (+ x1 [T,H,W,C1]), C0 + C1 == I (I % 8 != 0:
        one source, padded on the device).  The output buffer [rows + guard, ldo] (ldo 0: O) is filled with `fill` before it goes to the device.
        Returns (out as the device holds it, plan) with plan = ((tile config, split factor), ...) of the launches as the planner gave them."""
        x0 = _f32(x0); T, H, W, C0 = x0.shape
        x1a = None if x1 is None else _f32(x1); C1 = 0 if x1 is None else x1a.shape[-1]
        w = _f32(weight); O, I, kt, k, _ = w.shape
        b = None if bias is None else _f32(bias)
        rows = T * (H * ups // stride) * (W * ups // stride)
        r = None if R1 is None else _f32(R1).reshape(rows, O)
        ldo = ldo or O
        out = np.full((rows + guard, ldo), fill, np.float32)
        plan = (C.c_int * 9)()
        self._ck(self.lib.ug_op_conv_bound(self.ctx, _ptr(w), _ptr(b), I, O, kt, k, int(bool(upsampler)), _ptr(x0), C0, _ptr(x1a), C1, T, H, W,
                                           stride, pad_t, pad_l, ups, _ptr(r), c0, c1, act, int(ldo), int(guard), _ptr(out), plan))
        return out, tuple((plan[1 + 2 * i], plan[2 + 2 * i]) for i in range(plan[0]))

    # the epilogue operands of the graphs on linear() / conv() (tests/test_epilogue_forms_gpu.py).  Residuals are [rows, ld] arrays (ld >= the output width),
    # the output buffer [rows + guard, ldo] is filled with `fill` (or given as `out`) before it goes to the device and comes back whole.
    STAT_SENTINEL = 0x7FC5A5A5      # a quiet NaN with a payload no kernel produces: the bit pattern of an untouched statistics word

    def op_linear_ex(self, A, W, bias=None, bias2=None, R1=None, R2=None, c0=1.0, c1=1.0, c2=1.0, act=0, geglu=False, K=None, ldo=0, guard=0, fill=0.0):
        """A [M, lda] (lda >= K = W's columns), W [N, K]: act(c0 * f(A[:, :K] W^T + bias + bias2) + c1 * R1 + c2 * R2) through the engine's fp16 linear()
        (ug_op_linear_ex).  Returns (out [M + guard, ldo] as the device holds it, (tile config launched, split factor))."""
        A, W = _f32(A), _f32(W); M, lda = A.shape; N, Kw = W.shape; nout = N // 2 if geglu else N
        assert K is None or K == Kw
        opt = lambda a: None if a is None else _f32(a)
        b, b2, r1, r2 = opt(bias), opt(bias2), opt(R1), opt(R2)
        assert all(v is None or v.shape == (N,) for v in (b, b2)) and all(r is None or (r.ndim == 2 and r.shape[0] == M) for r in (r1, r2))
        out = np.full((M + guard, ldo or nout), fill, np.float32)
        plan = (C.c_int * 2)()
        self._ck(self.lib.ug_op_linear_ex(self.ctx, _ptr(A), M, lda, _ptr(W), N, Kw, _ptr(b), _ptr(b2), _ptr(r1), 0 if r1 is None else r1.shape[1],
                                          _ptr(r2), 0 if r2 is None else r2.shape[1], float(c0), float(c1), float(c2), int(act), int(bool(geglu)),
                                          out.shape[1], int(guard), _ptr(out), plan))
        return out, tuple(plan)

    def op_conv_epi(self, x0, weight, bias=None, x1=None, stride=1, pad_t=1, pad_l=1, bias2=None, R1=None, R2=None, c0=1.0, c1=1.0, c2=1.0, act=0,
                    ldo=0, guard=0, fill=0.0, stats=False):
        """weight [O, I, kt, k, k] bound on the device and launched by the engine's conv() on x0 [T,H,W,C0] (+ x1 [T,H,W,C1]) with the whole epilogue
        (ug_op_conv_epi).  Returns (out [rows + guard, ldo], (tile config launched, split factor)), and with stats=True also (rb, part): the rows per
        statistics block the launch reported (0: declined) and the statistics area [ceil(rows / 48), O, 2] float32 (sum, sum of squares), which went to the
        device filled with STAT_SENTINEL."""
        x0 = _f32(x0); T, H, W, C0 = x0.shape
        x1a = None if x1 is None else _f32(x1); C1 = 0 if x1 is None else x1a.shape[-1]
        w = _f32(weight); O, I, kt, k, _ = w.shape
        opt = lambda a: None if a is None else _f32(a)
        b, b2, r1, r2 = opt(bias), opt(bias2), opt(R1), opt(R2)
        rows = T * (H // stride) * (W // stride)
        assert all(v is None or v.shape == (O,) for v in (b, b2)) and all(r is None or (r.ndim == 2 and r.shape[0] == rows) for r in (r1, r2))
        out = np.full((rows + guard, ldo or O), fill, np.float32)
        part = np.full(((rows + 47) // 48, O, 2), self.STAT_SENTINEL, np.uint32).view(np.float32) if stats else None
        plan = (C.c_int * 2)(); rb = C.c_int(0)
        self._ck(self.lib.ug_op_conv_epi(self.ctx, _ptr(w), _ptr(b), I, O, kt, k, _ptr(x0), C0, _ptr(x1a), C1, T, H, W, stride, pad_t, pad_l,
                                         _ptr(b2), _ptr(r1), 0 if r1 is None else r1.shape[1], _ptr(r2), 0 if r2 is None else r2.shape[1],
                                         float(c0), float(c1), float(c2), int(act), out.shape[1], int(guard), _ptr(out), int(bool(stats)), _ptr(part),
                                         C.cast(C.byref(rb), C.c_void_p), plan))
        return (out, tuple(plan), int(rb.value), part) if stats else (out, tuple(plan))

    def op_attn_wide(self, qkv, T, S):
        q = _f32(qkv); Cc = q.shape[1] // 3
        out = np.empty((T * S, Cc), np.float32)
        self._ck(self.lib.ug_op_attn_wide(self.ctx, _ptr(q), T, S, Cc, _ptr(out)))
        return out

    def op_euler_step(self, v, lat, sigma, sigma_next):
        v = _f32(v); l = _f32(lat).copy()
        self._ck(self.lib.ug_op_euler_step(self.ctx, _ptr(v), _ptr(l), l.size, sigma, sigma_next))
        return l

    # the pipeline glue of kernels/misc.hip one launch at a time (tests/test_glue_gpu.py).  Every output is a new array of the whole device buffer:
    # guard extra rows (or elements) filled with `fill` before the launch - an fp16-representable value where the buffer is fp16 on the device.
    @staticmethod
    def _out(shape, fill):
        return np.full(shape, fill, np.float32)

    def op_clip_patchify(self, video_m11, S, P, Kpad, imagenet_norm=False, guard=0, fill=-777.0):
        """video_m11 [T,H,W,3] -> [T*(S/P)^2 + guard, Kpad]; columns [3*P*P, Kpad) keep `fill`."""
        v = _f32(video_m11); T, H, W, _ = v.shape
        out = self._out((T * (S // P) ** 2 + guard, Kpad), fill)
        self._ck(self.lib.ug_op_clip_patchify(self.ctx, _ptr(v), T, H, W, S, P, Kpad, int(bool(imagenet_norm)), int(guard), _ptr(out)))
        return out

    def op_prep_video(self, frames, noise, aug, guard=0, fill=-777.0):
        """frames [T,H,W,3], noise [T,3,H,W] -> (clip_src [T*H*W + guard, 3], vae_in [T*H*W + guard, 8])."""
        f, nz = _f32(frames), _f32(noise); T, H, W, _ = f.shape
        assert nz.shape == (T, 3, H, W), nz.shape
        src = self._out((T * H * W + guard, 3), fill); vin = self._out((T * H * W + guard, 8), fill)
        self._ck(self.lib.ug_op_prep_video(self.ctx, _ptr(f), _ptr(nz), T, H, W, float(aug), int(guard), _ptr(src), _ptr(vin)))
        return src, vin

    def op_init_latents(self, noise_tchw, sigma0, guard=0, fill=-777.0):
        """noise [T,4,h,w] -> latents [T*h*w + guard, 4] (channels-last)."""
        nz = _f32(noise_tchw); T, ch, h, w = nz.shape
        assert ch == 4, nz.shape
        lat = self._out((T * h * w + guard, 4), fill)
        self._ck(self.lib.ug_op_init_latents(self.ctx, _ptr(nz), T, h * w, float(sigma0), int(guard), _ptr(lat)))
        return lat

    def op_unet_input(self, lat, cond, den, guided=False, guard=0, fill=-777.0):
        """lat, cond [pixels,4] -> [pixels + guard, 8]; guided: [2*pixels + guard, 8], conditional video first."""
        l, cn = _f32(lat), _f32(cond); px = l.shape[0]
        assert l.shape == cn.shape == (px, 4), (l.shape, cn.shape)
        out = self._out(((2 if guided else 1) * px + guard, 8), fill)
        self._ck(self.lib.ug_op_unet_input(self.ctx, _ptr(l), _ptr(cn), px, float(den), int(bool(guided)), int(guard), _ptr(out)))
        return out

    def op_euler_step_cfg(self, vc, vu, g, lat, sigma, sigma_next, guard=0, fill=-777.0):
        a, b, l = _f32(vc).ravel(), _f32(vu).ravel(), _f32(lat).ravel()
        assert a.size == b.size == l.size
        out = np.concatenate([l, self._out(guard, fill)])
        self._ck(self.lib.ug_op_euler_step_cfg(self.ctx, _ptr(a), _ptr(b), float(g), l.size, float(sigma), float(sigma_next), int(guard), _ptr(out)))
        return out

    def op_window_blend(self, prev, cur, overlap, coef, guard=0, fill=-777.0):
        """prev, cur [overlap, frame_elems]: (prev + coef * cur, the cross-fade of cur into prev), each [overlap * frame_elems + guard]."""
        p, cu = _f32(prev), _f32(cur)
        assert p.shape == cu.shape and p.shape[0] == overlap, (p.shape, cu.shape)
        rn = np.concatenate([cu.ravel(), self._out(guard, fill)]); fd = np.concatenate([p.ravel(), self._out(guard, fill)])
        self._ck(self.lib.ug_op_window_blend(self.ctx, _ptr(p), _ptr(cu), p.shape[1], int(overlap), float(coef), int(guard), _ptr(rn), _ptr(fd)))
        return rn, fd

    def op_time_conv_out(self, x, w, b, guard=0, fill=-777.0):
        """x [T,HW,Cs], w [3,3,3] (out, in, tap), b [3] -> [T*HW + guard, 3] float32."""
        xa, wa, ba = _f32(x), _f32(w), _f32(b); T, HW, Cs = xa.shape
        assert wa.shape == (3, 3, 3) and ba.shape == (3,)
        out = self._out((T * HW + guard, 3), fill)
        self._ck(self.lib.ug_op_time_conv_out(self.ctx, _ptr(xa), _ptr(wa), _ptr(ba), T, HW, Cs, int(guard), _ptr(out)))
        return out

    def op_depth_post(self, frames, guard=0, fill=-777.0):
        """frames [n,3] -> (depth [n + guard], disparity [n + guard], (min, max) decoded from the ordered-integer words)."""
        f = _f32(frames); n = f.shape[0]
        depth = self._out(n + guard, fill); disp = self._out(n + guard, fill); mm = np.zeros(2, np.float32)
        self._ck(self.lib.ug_op_depth_post(self.ctx, _ptr(f), n, int(guard), _ptr(depth), _ptr(disp), _ptr(mm)))
        return depth, disp, mm

    def op_add_grid_nearest(self, x, grid, guard=0, fill=-777.0):
        """x [B,h,w,C] += grid [B,g,g,C] gathered at (y*g // h, x*g // w) -> [B*h*w + guard, C]."""
        xa, ga = _f32(x), _f32(grid); B, h, w, Cc = xa.shape; g = ga.shape[1]
        assert ga.shape == (B, g, g, Cc), ga.shape
        out = np.concatenate([xa.reshape(-1, Cc), self._out((guard, Cc), fill)])
        self._ck(self.lib.ug_op_add_grid_nearest(self.ctx, _ptr(ga), B, h, w, g, Cc, int(guard), _ptr(out)))
        return out

    def op_sn_normals_out(self, dec, guard=0, fill=-777.0):
        """dec [pixels, ldd] -> [pixels + guard, 3] float32."""
        d = _f32(dec); px, ldd = d.shape
        out = self._out((px + guard, 3), fill)
        self._ck(self.lib.ug_op_sn_normals_out(self.ctx, _ptr(d), ldd, px, int(guard), _ptr(out)))
        return out

    def op_clip_assemble(self, patches, cls, pos, T, guard=0, fill=-777.0):
        """patches [T*np, d], cls [d], pos [np+1, d] -> tokens [T*(np+1) + guard, d]."""
        p, cl, po = _f32(patches), _f32(cls), _f32(pos); d = p.shape[1]; npp = p.shape[0] // T
        assert p.shape == (T * npp, d) and cl.shape == (d,) and po.shape == (npp + 1, d), (p.shape, cl.shape, po.shape)
        out = self._out((T * (npp + 1) + guard, d), fill)
        self._ck(self.lib.ug_op_clip_assemble(self.ctx, _ptr(p), _ptr(cl), _ptr(po), T, npp, d, int(guard), _ptr(out)))
        return out

    def bench_gemm(self, M=0, N=0, K=0, conv=None, cfg=-1, split=0, iters=20):
        """conv = dict(T,H,W,C0,C1,kt,k,stride,ups) or None (dense).  Returns (ms, TFLOP/s, cfg, split)."""
        out = np.zeros(8, np.float32)
        cv = conv or {}
        self._ck(self.lib.ug_bench_gemm(self.ctx, M, N, K, int(conv is not None), cv.get("T", 0), cv.get("H", 0), cv.get("W", 0),
                                        cv.get("C0", 0), cv.get("C1", 0), cv.get("kt", 1), cv.get("k", 1), cv.get("stride", 1),
                                        cv.get("ups", 1), cfg, split, iters, _ptr(out)))
        Mr, Kr = float(out[3]), float(out[4])
        return float(out[0]), 2.0 * Mr * N * Kr / (out[0] * 1e-3) / 1e12, int(out[1]), int(out[2])

    def bench_mfma_peak(self, iters=20000):
        """Calibration: chip-wide fp16 MFMA TFLOP/s with operands in registers (kernels/probe.hip)."""
        out = np.zeros(1, np.float32)
        self._ck(self.lib.ug_bench_mfma_peak(self.ctx, int(iters), _ptr(out)))
        return float(out[0])

    def tune_force(self, cfg=-1, split=-1):
        """Test / A-B aid, per context: force a GEMM tile config + split-K factor ((-1, -1) = planner); cfg = -100 - mask sets the knob mask."""
        self._ck(self.lib.ug_tune_force(self.ctx, int(cfg), int(split)))

    def bench_groupnorm(self, C0, C1, T, HW, temporal, mode, iters=20):
        out = np.zeros(1, np.float32)
        self._ck(self.lib.ug_bench_groupnorm(self.ctx, C0, C1, T, HW, int(temporal), mode, iters, _ptr(out)))
        return float(out[0])

    # ---- profiling
    def profile_begin(self, shapes=False):
        self._ck((self.lib.ug_profile_begin_shapes if shapes else self.lib.ug_profile_begin)(self.ctx))

    def profile_end(self):
        prof = json.loads(self.lib.ug_profile_end(self.ctx).decode())
        self.last_profile_order = prof.pop("__order__", None)      # shapes=True: [[name, algorithmic bytes], ...] of the GEMM launches, in order
        return prof

    def workspace_peak(self):
        return int(self.lib.ug_workspace_peak(self.ctx))
