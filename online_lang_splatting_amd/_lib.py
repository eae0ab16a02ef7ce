"""Loads libolsr.so (the HIP kernels + C-ABI of include/olsr.h, include/olsr_single_stage.h, include/olsr_frame_ingest.h,
include/olsr_map_io.h and include/olsr_clip_trunk.h) and declares its prototypes.

There is no fallback: if the library is missing or a symbol is absent this raises, loudly.
"""
import ctypes as C
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# (OLSR_LIB: another build of the same library, for kernel experiments; the compiled torch binding always links libolsr.so)
LIB_PATH = os.environ.get("OLSR_LIB") or os.path.join(_HERE, "libolsr.so")

# every symbol include/olsr.h declares
EXPORTS = (
    "olsr_geometry_bytes", "olsr_image_bytes", "olsr_binning_bytes", "olsr_backward_scratch_bytes", "olsr_last_forward_token", "olsr_live_rows", "olsr_forward", "olsr_forward_async", "olsr_forward_async_loss", "olsr_fused_loss_scratch_bytes",
    "olsr_backward", "olsr_accumulate_gradients", "olsr_sparse_exchange_mask", "olsr_sparse_exchange_scratch_ints", "olsr_sparse_exchange_pack", "olsr_sparse_exchange_unpack", "olsr_mapping_loss", "olsr_mapping_loss_scratch_bytes", "olsr_tracking_loss", "olsr_refinement_loss", "olsr_refinement_loss_scratch_bytes", "olsr_lang_ae_scratch_bytes", "olsr_lang_ae_train_step", "olsr_lang_ae_encode", "olsr_lang_ae_decode", "olsr_lang_query_scratch_bytes", "olsr_lang_query_sims", "olsr_lang_query_relevancy", "olsr_lang_encoder_encode", "olsr_hr_net_workspace_bytes", "olsr_hr_net_forward", "olsr_tsdf_init", "olsr_tsdf_integrate", "olsr_tsdf_surface_scratch_bytes", "olsr_tsdf_surface_plan", "olsr_tsdf_surface_emit", "olsr_tsdf_mesh_scratch_bytes", "olsr_tsdf_mesh_plan", "olsr_tsdf_mesh_emit", "olsr_emd_scratch_bytes", "olsr_emd_cost", "olsr_chamfer_scratch_bytes", "olsr_chamfer", "olsr_mask_smooth", "olsr_query_eval_scratch_bytes", "olsr_query_eval", "olsr_image_psnr_scratch_bytes", "olsr_image_psnr", "olsr_pose_step", "olsr_pose_step_gated", "olsr_window_pose_step", "olsr_knn_mean_dist2", "olsr_knn_scratch_bytes", "olsr_adam_step", "olsr_adam_step_sum", "olsr_adam_step_masked", "olsr_adam_step_groups", "olsr_adam_step_groups_reg", "olsr_isotropic_reg_scratch_bytes", "olsr_isotropic_reg", "olsr_map_edit_scratch_bytes", "olsr_map_edit_plan", "olsr_map_edit_apply", "olsr_keyframe_seed_scratch_bytes", "olsr_keyframe_seed_plan", "olsr_keyframe_seed_finish", "olsr_frontend_scratch_bytes", "olsr_grad_mask", "olsr_median_depth", "olsr_covisibility", "olsr_keyframe_decide", "olsr_bucket_add", "olsr_mark_visible", "olsr_geometry_field", "olsr_binning_field", "olsr_image_field",
    "olsr_set_profiling", "olsr_get_stage_times", "olsr_debug_sort_timing", "olsr_debug_sort_plan", "olsr_debug_sort_knobs", "olsr_debug_sort_small", "olsr_debug_sort_compact", "olsr_debug_sort_threads", "olsr_debug_composite_stamps", "olsr_debug_sync_fault", "olsr_debug_rows_ratio", "olsr_debug_backward_ordered", "olsr_debug_backward_ordered_scratch_bytes", "olsr_debug_exp_sweep", "olsr_debug_activate", "olsr_debug_carve_log", "olsr_debug_carve_log_read", "olsr_debug_sort_status_room", "olsr_live_rows_wait", "olsr_live_rows_overwritten", "olsr_backward_rows", "olsr_last_error", "olsr_version",
)

# every symbol include/olsr_single_stage.h declares (the same library)
EXPORTS_SINGLE_STAGE = ("olsr_ss_encoder_encode", "olsr_ss_query_sims")

# every symbol include/olsr_frame_ingest.h declares (the same library)
EXPORTS_FRAME_INGEST = ("olsr_frame_ingest",)

# every symbol include/olsr_map_io.h declares (the same library)
EXPORTS_MAP_IO = ("olsr_map_ply_width", "olsr_map_ply_pack", "olsr_map_ply_unpack")

# every symbol include/olsr_clip_trunk.h declares (the same library)
EXPORTS_CLIP_TRUNK = ("olsr_convnext_block_workspace_bytes", "olsr_convnext_block", "olsr_clip_trunk_workspace_bytes",
                      "olsr_clip_trunk_packed_floats", "olsr_clip_trunk_launches", "olsr_clip_trunk_forward")

_lib = None


class OlsrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"olsr error {code}: {msg}")
        self.code = code


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m online_lang_splatting_amd.build` "
            "(hipcc, gfx950).  There is no CPU or PyTorch fallback for the rasterizer.")
    L = C.CDLL(LIB_PATH)
    missing = [s for s in EXPORTS + EXPORTS_SINGLE_STAGE + EXPORTS_FRAME_INGEST + EXPORTS_MAP_IO + EXPORTS_CLIP_TRUNK if not hasattr(L, s)]
    if missing:
        raise ImportError(f"{LIB_PATH} lacks symbols {missing}; rebuild it")
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    scene_p = C.POINTER(_abi.OlsrScene)
    L.olsr_geometry_bytes.argtypes, L.olsr_geometry_bytes.restype = [i32, i32], sz
    L.olsr_image_bytes.argtypes, L.olsr_image_bytes.restype = [i32, i32, i32], sz
    L.olsr_binning_bytes.argtypes, L.olsr_binning_bytes.restype = [i64, i32], sz
    L.olsr_forward.argtypes = [scene_p, _abi.ALLOC_FN, vp, _abi.ALLOC_FN, vp, _abi.ALLOC_FN, vp,
                               vp, vp, vp, vp, vp, vp, C.POINTER(i32), vp]
    L.olsr_forward.restype = C.c_int
    L.olsr_forward_async.argtypes = [scene_p, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.olsr_forward_async.restype = C.c_int
    L.olsr_forward_async_loss.argtypes = [scene_p, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                          C.POINTER(_abi.OlsrLossFusion), vp]
    L.olsr_forward_async_loss.restype = C.c_int
    L.olsr_fused_loss_scratch_bytes.argtypes, L.olsr_fused_loss_scratch_bytes.restype = [i32, i32, i32], sz
    L.olsr_backward_scratch_bytes.argtypes, L.olsr_backward_scratch_bytes.restype = [i64, i32], sz
    L.olsr_last_forward_token.argtypes, L.olsr_last_forward_token.restype = [], i32
    L.olsr_live_rows.argtypes, L.olsr_live_rows.restype = [i32, i32], i64
    L.olsr_live_rows_wait.argtypes, L.olsr_live_rows_wait.restype = [i32, i32, i32], i64
    L.olsr_live_rows_overwritten.argtypes, L.olsr_live_rows_overwritten.restype = [i32], i32
    L.olsr_backward_rows.argtypes, L.olsr_backward_rows.restype = [i32, i32, i64, i32], i64
    L.olsr_backward.argtypes = ([scene_p, vp, vp, i32, vp, vp, _abi.ALLOC_FN, vp, i32, vp, i64] + [vp] * 3 + [vp] * 13
                                + [C.POINTER(_abi.OlsrGradBucket), vp, vp])
    L.olsr_backward.restype = C.c_int
    L.olsr_accumulate_gradients.argtypes = [i32, i32, i32, i32] + [vp] * 12
    L.olsr_accumulate_gradients.restype = C.c_int
    L.olsr_sparse_exchange_mask.argtypes, L.olsr_sparse_exchange_mask.restype = [i32, i32] + [vp] * 5, C.c_int
    L.olsr_sparse_exchange_scratch_ints.argtypes, L.olsr_sparse_exchange_scratch_ints.restype = [i32], i64
    L.olsr_sparse_exchange_pack.argtypes, L.olsr_sparse_exchange_pack.restype = [i32, i32, i32] + [vp] * 10, C.c_int
    L.olsr_sparse_exchange_unpack.argtypes, L.olsr_sparse_exchange_unpack.restype = [i32, i32, i32] + [vp] * 5, C.c_int
    L.olsr_mapping_loss_scratch_bytes.argtypes, L.olsr_mapping_loss_scratch_bytes.restype = [i32, i32], sz
    L.olsr_mapping_loss.argtypes = [C.POINTER(_abi.OlsrLossParams)] + [vp] * 14
    L.olsr_mapping_loss.restype = C.c_int
    L.olsr_tracking_loss.argtypes = [C.POINTER(_abi.OlsrLossParams)] + [vp] * 13
    L.olsr_tracking_loss.restype = C.c_int
    L.olsr_refinement_loss_scratch_bytes.argtypes, L.olsr_refinement_loss_scratch_bytes.restype = [i32, i32], sz
    L.olsr_refinement_loss.argtypes, L.olsr_refinement_loss.restype = [i32, i32, C.c_float] + [vp] * 6, C.c_int
    L.olsr_lang_ae_scratch_bytes.argtypes, L.olsr_lang_ae_scratch_bytes.restype = [i32], sz
    L.olsr_lang_ae_train_step.argtypes = [C.POINTER(_abi.OlsrLangAeParams), i32] + [vp] * 10
    L.olsr_lang_ae_train_step.restype = C.c_int
    L.olsr_lang_ae_encode.argtypes, L.olsr_lang_ae_encode.restype = [i32, vp, vp, i32, vp, vp], C.c_int
    L.olsr_lang_ae_decode.argtypes, L.olsr_lang_ae_decode.restype = [i32, vp, vp, i32, vp, vp], C.c_int
    qp = C.POINTER(_abi.OlsrLangQueryParams)
    L.olsr_lang_query_scratch_bytes.argtypes, L.olsr_lang_query_scratch_bytes.restype = [qp], sz
    L.olsr_lang_query_sims.argtypes, L.olsr_lang_query_sims.restype = [qp] + [vp] * 6, C.c_int
    L.olsr_lang_query_relevancy.argtypes, L.olsr_lang_query_relevancy.restype = [qp] + [vp] * 11, C.c_int
    L.olsr_lang_encoder_encode.argtypes = [C.POINTER(_abi.OlsrLangEncoderParams), i32] + [vp] * 6
    L.olsr_lang_encoder_encode.restype = C.c_int
    L.olsr_ss_encoder_encode.argtypes = [C.POINTER(_abi.OlsrSsEncoderParams), i32] + [vp] * 4
    L.olsr_ss_encoder_encode.restype = C.c_int
    L.olsr_ss_query_sims.argtypes, L.olsr_ss_query_sims.restype = [qp] + [vp] * 5, C.c_int
    L.olsr_hr_net_workspace_bytes.argtypes, L.olsr_hr_net_workspace_bytes.restype = [i32] * 6, sz
    L.olsr_hr_net_forward.argtypes, L.olsr_hr_net_forward.restype = [C.POINTER(_abi.OlsrHrNetParams)] + [vp] * 7, C.c_int
    tv = C.POINTER(_abi.OlsrTsdfVolume)
    L.olsr_tsdf_init.argtypes, L.olsr_tsdf_init.restype = [tv, vp], C.c_int
    L.olsr_tsdf_integrate.argtypes, L.olsr_tsdf_integrate.restype = [tv, i32, C.POINTER(_abi.OlsrTsdfView), vp], C.c_int
    L.olsr_tsdf_surface_scratch_bytes.argtypes, L.olsr_tsdf_surface_scratch_bytes.restype = [i32, i32, i32], sz
    L.olsr_tsdf_surface_plan.argtypes, L.olsr_tsdf_surface_plan.restype = [tv, C.c_float, vp, vp, vp], C.c_int
    L.olsr_tsdf_surface_emit.argtypes, L.olsr_tsdf_surface_emit.restype = [tv, C.c_float, vp, i32, vp, vp, vp, vp], C.c_int
    L.olsr_tsdf_mesh_scratch_bytes.argtypes, L.olsr_tsdf_mesh_scratch_bytes.restype = [i32, i32, i32], sz
    L.olsr_tsdf_mesh_plan.argtypes, L.olsr_tsdf_mesh_plan.restype = [tv, C.c_float, vp, vp, vp], C.c_int
    L.olsr_tsdf_mesh_emit.argtypes, L.olsr_tsdf_mesh_emit.restype = [tv, C.c_float, vp, i32, i32, vp, vp, vp, vp, vp, vp], C.c_int
    L.olsr_emd_scratch_bytes.argtypes, L.olsr_emd_scratch_bytes.restype = [i32, i64, i64], sz
    L.olsr_emd_cost.argtypes, L.olsr_emd_cost.restype = [i32, vp, vp, i32, i32] + [vp] * 7, C.c_int
    L.olsr_chamfer_scratch_bytes.argtypes, L.olsr_chamfer_scratch_bytes.restype = [i32, i64, i64], sz
    L.olsr_chamfer.argtypes, L.olsr_chamfer.restype = [i32, vp, vp, i32, i32] + [vp] * 10, C.c_int
    L.olsr_mask_smooth.argtypes, L.olsr_mask_smooth.restype = [i32, i32, i32, vp, vp, vp], C.c_int
    L.olsr_query_eval_scratch_bytes.argtypes, L.olsr_query_eval_scratch_bytes.restype = [i32, i32, i32], sz
    L.olsr_query_eval.argtypes, L.olsr_query_eval.restype = [i32, i32, i32] + [vp] * 10, C.c_int
    L.olsr_image_psnr_scratch_bytes.argtypes, L.olsr_image_psnr_scratch_bytes.restype = [], sz
    L.olsr_image_psnr.argtypes, L.olsr_image_psnr.restype = [i32, i32, i32] + [vp] * 5, C.c_int
    L.olsr_pose_step.argtypes = [C.POINTER(_abi.OlsrPoseParams)] + [vp] * 6
    L.olsr_pose_step.restype = C.c_int
    L.olsr_pose_step_gated.argtypes = [C.POINTER(_abi.OlsrPoseParams)] + [vp] * 7
    L.olsr_pose_step_gated.restype = C.c_int
    L.olsr_adam_step.argtypes = [i32, i32, i32, C.POINTER(_abi.OlsrAdamParams)] + [vp] * 10
    L.olsr_adam_step.restype = C.c_int
    L.olsr_adam_step_sum.argtypes = [i32, i32, i32, C.POINTER(_abi.OlsrAdamParams), i32, C.POINTER(vp)] + [vp] * 9
    L.olsr_adam_step_sum.restype = C.c_int
    L.olsr_adam_step_masked.argtypes = [i32, i32, i32, C.POINTER(_abi.OlsrAdamParams), i32, C.POINTER(vp), C.POINTER(vp)] + [vp] * 9
    L.olsr_adam_step_masked.restype = C.c_int
    L.olsr_adam_step_groups.argtypes = [i32, i32, i32, C.POINTER(_abi.OlsrAdamGroupParams), i32, C.POINTER(vp), C.POINTER(vp)] + [vp] * 9
    L.olsr_adam_step_groups.restype = C.c_int
    L.olsr_adam_step_groups_reg.argtypes = ([i32, i32, i32, C.POINTER(_abi.OlsrAdamGroupParams), i32, C.POINTER(vp), C.POINTER(vp)]
                                            + [vp] * 8 + [C.POINTER(_abi.OlsrAdamReg), vp])
    L.olsr_adam_step_groups_reg.restype = C.c_int
    L.olsr_isotropic_reg_scratch_bytes.argtypes, L.olsr_isotropic_reg_scratch_bytes.restype = [i32], sz
    L.olsr_isotropic_reg.argtypes, L.olsr_isotropic_reg.restype = [i32, vp, i32, C.c_double, vp, vp, vp, vp], C.c_int
    L.olsr_window_pose_step.argtypes = [C.POINTER(_abi.OlsrPoseParams), i32, C.POINTER(i32)] + [vp] * 7
    L.olsr_window_pose_step.restype = C.c_int
    L.olsr_map_edit_scratch_bytes.argtypes, L.olsr_map_edit_scratch_bytes.restype = [i32], sz
    mb, mp = C.POINTER(_abi.OlsrMapBuffers), C.POINTER(_abi.OlsrMapEditParams)
    L.olsr_map_edit_plan.argtypes, L.olsr_map_edit_plan.restype = [i32, mp, mb, vp, vp, vp, vp], C.c_int
    L.olsr_map_edit_apply.argtypes = [i32, i32, i32, mp, mb, vp, mb, vp, vp, i32, i32, mb, vp, vp]
    L.olsr_map_edit_apply.restype = C.c_int
    ks = C.POINTER(_abi.OlsrKeyframeSeedParams)
    L.olsr_keyframe_seed_scratch_bytes.argtypes, L.olsr_keyframe_seed_scratch_bytes.restype = [i32, i32], sz
    L.olsr_keyframe_seed_plan.argtypes, L.olsr_keyframe_seed_plan.restype = [ks, vp, vp, vp, vp, mb, vp, vp, vp, vp, vp], C.c_int
    L.olsr_keyframe_seed_finish.argtypes, L.olsr_keyframe_seed_finish.restype = [ks, i32, mb, vp, vp, vp, vp], C.c_int
    L.olsr_frontend_scratch_bytes.argtypes, L.olsr_frontend_scratch_bytes.restype = [i64], sz
    L.olsr_grad_mask.argtypes, L.olsr_grad_mask.restype = [i32, i32, i64, i32, C.c_float, vp, vp, vp, vp], C.c_int
    L.olsr_median_depth.argtypes, L.olsr_median_depth.restype = [i64] + [vp] * 7, C.c_int
    L.olsr_covisibility.argtypes, L.olsr_covisibility.restype = [i64, vp, C.POINTER(_abi.OlsrCovisViews), vp, vp, vp], C.c_int
    L.olsr_keyframe_decide.argtypes = [C.POINTER(_abi.OlsrKeyframeDecideParams)] + [vp] * 6
    L.olsr_keyframe_decide.restype = C.c_int
    L.olsr_frame_ingest.argtypes = [C.POINTER(_abi.OlsrFrameIngestParams)] + [vp] * 5
    L.olsr_frame_ingest.restype = C.c_int
    L.olsr_map_ply_width.argtypes, L.olsr_map_ply_width.restype = [i32, i32], C.c_int
    L.olsr_map_ply_pack.argtypes, L.olsr_map_ply_pack.restype = [i32, i32, i32, mb, vp, vp], C.c_int
    L.olsr_map_ply_unpack.argtypes, L.olsr_map_ply_unpack.restype = [i32, i32, i32, i32, C.POINTER(i32), vp, mb, vp], C.c_int
    L.olsr_convnext_block_workspace_bytes.argtypes, L.olsr_convnext_block_workspace_bytes.restype = [i32, i32, i32], sz
    L.olsr_convnext_block.argtypes, L.olsr_convnext_block.restype = [C.POINTER(_abi.OlsrConvnextBlockParams)] + [vp] * 5, C.c_int
    tp = C.POINTER(_abi.OlsrClipTrunkParams)
    L.olsr_clip_trunk_workspace_bytes.argtypes, L.olsr_clip_trunk_workspace_bytes.restype = [tp], sz
    L.olsr_clip_trunk_packed_floats.argtypes, L.olsr_clip_trunk_packed_floats.restype = [tp], sz
    L.olsr_clip_trunk_launches.argtypes, L.olsr_clip_trunk_launches.restype = [tp], i32
    L.olsr_clip_trunk_forward.argtypes, L.olsr_clip_trunk_forward.restype = [tp] + [vp] * 7, C.c_int
    L.olsr_bucket_add.argtypes, L.olsr_bucket_add.restype = [i32, i32] + [vp] * 9, C.c_int
    L.olsr_knn_scratch_bytes.argtypes, L.olsr_knn_scratch_bytes.restype = [i32], sz
    L.olsr_knn_mean_dist2.argtypes, L.olsr_knn_mean_dist2.restype = [i32, vp, vp, vp, vp], C.c_int
    L.olsr_mark_visible.argtypes, L.olsr_mark_visible.restype = [i32, vp, vp, vp, vp, vp], C.c_int
    L.olsr_geometry_field.argtypes, L.olsr_geometry_field.restype = [vp, i32, i32, C.c_char_p], vp
    L.olsr_binning_field.argtypes, L.olsr_binning_field.restype = [vp, i64, i32, C.c_char_p], vp
    L.olsr_image_field.argtypes, L.olsr_image_field.restype = [vp, i32, i32, i32, C.c_char_p], vp
    L.olsr_set_profiling.argtypes, L.olsr_set_profiling.restype = [C.c_int], None
    L.olsr_get_stage_times.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]
    L.olsr_get_stage_times.restype = C.c_int
    L.olsr_debug_sort_plan.argtypes = [i64, C.c_int, C.POINTER(i32), C.POINTER(i32)]
    L.olsr_debug_sort_plan.restype = C.c_int
    L.olsr_debug_sort_knobs.argtypes = [C.c_int, C.c_int, C.c_int]
    L.olsr_debug_sort_knobs.restype = None
    L.olsr_debug_sort_small.argtypes, L.olsr_debug_sort_small.restype = [C.c_int], None
    L.olsr_debug_sort_compact.argtypes, L.olsr_debug_sort_compact.restype = [C.c_int], None
    L.olsr_debug_sort_threads.argtypes, L.olsr_debug_sort_threads.restype = [C.c_int], C.c_int
    L.olsr_debug_composite_stamps.argtypes, L.olsr_debug_composite_stamps.restype = [vp, C.c_int], None
    L.olsr_debug_sync_fault.argtypes = [C.c_int, C.c_int]
    L.olsr_debug_sync_fault.restype = None
    L.olsr_debug_rows_ratio.argtypes, L.olsr_debug_rows_ratio.restype = [i32, C.c_float, C.POINTER(i32)], C.c_float
    L.olsr_debug_backward_ordered_scratch_bytes.argtypes, L.olsr_debug_backward_ordered_scratch_bytes.restype = [i64, i32], sz
    L.olsr_debug_backward_ordered.argtypes = [scene_p, vp, i32, vp, vp] + [vp] * 3 + [vp] + [vp] * 6 + [i32, vp]
    L.olsr_debug_backward_ordered.restype = C.c_int
    L.olsr_debug_exp_sweep.argtypes, L.olsr_debug_exp_sweep.restype = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)], C.c_int
    L.olsr_debug_activate.argtypes, L.olsr_debug_activate.restype = [i32, i32] + [vp] * 3 + [vp] * 3 + [vp], C.c_int
    L.olsr_debug_carve_log.argtypes, L.olsr_debug_carve_log.restype = [C.c_int], None
    L.olsr_debug_carve_log_read.argtypes, L.olsr_debug_carve_log_read.restype = [C.POINTER(C.c_uint64), C.c_int], C.c_int
    L.olsr_debug_sort_status_room.argtypes, L.olsr_debug_sort_status_room.restype = [i64, C.c_int], i64
    L.olsr_last_error.argtypes, L.olsr_last_error.restype = [], C.c_char_p
    L.olsr_version.argtypes, L.olsr_version.restype = [], C.c_char_p
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise OlsrError(rc, lib().olsr_last_error().decode())


def stage_times(max_entries=1 << 16):
    """[(stage name, milliseconds)] for every stage issued on this thread since
    olsr_set_profiling(1), in issue order."""
    names = (C.c_char_p * max_entries)()
    ms = (C.c_float * max_entries)()
    n = lib().olsr_get_stage_times(names, ms, max_entries)
    return [(names[i].decode(), float(ms[i])) for i in range(n)]


def exp_sweep(first_bits, count):
    """olsr_debug_exp_sweep: (scalar, packed, swapped) mismatch counts and the lowest mismatching pattern (None: none)."""
    out = (C.c_uint64 * 4)()
    check(lib().olsr_debug_exp_sweep(first_bits, count, out))
    return int(out[0]), int(out[1]), int(out[2]), (None if out[3] == 2**64 - 1 else int(out[3]))


def debug_activate(activations, opacities=None, scales=None, rotations=None):
    """olsr_debug_activate on the current stream: the kernels' own sigmoid / exp / normalize of the raw arrays whose _abi.ACT_*
    bit is set in `activations`, copies of the others (contiguous float32 on the GPU; None: left out).  Returns the three
    activated arrays (None where None was given)."""
    import torch
    given = [t for t in (opacities, scales, rotations) if t is not None]
    for t in given:
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("debug_activate: inputs must be contiguous fp32 tensors on the GPU")
    if not given:
        return None, None, None
    P = given[0].shape[0]
    for t, per in ((opacities, 1), (scales, 3), (rotations, 4)):
        if t is not None and t.numel() != P * per:
            raise RuntimeError("debug_activate: opacities [P(,1)], scales [P,3] and rotations [P,4] of one P")
    out = [None if t is None else torch.empty_like(t) for t in (opacities, scales, rotations)]
    from ._host import ptr, stream_ptr
    check(lib().olsr_debug_activate(P, int(activations), ptr(opacities), ptr(scales), ptr(rotations), ptr(out[0]), ptr(out[1]),
                                    ptr(out[2]),
                                    stream_ptr(given[0].device)))
    return tuple(out)


def carve_log(enable):
    """olsr_debug_carve_log: clear this thread's carve log and switch it on or off."""
    lib().olsr_debug_carve_log(1 if enable else 0)


def carve_log_read():
    """[(base, offset, bytes)] of every Carver::take since carve_log(True) on this thread (base 0: a sizing carve)."""
    n = lib().olsr_debug_carve_log_read(None, 0)
    out = (C.c_uint64 * (3 * max(n, 1)))()
    n = min(n, lib().olsr_debug_carve_log_read(out, n))
    return [(int(out[3 * i]), int(out[3 * i + 1]), int(out[3 * i + 2])) for i in range(n)]


def set_profiling(enable):
    lib().olsr_set_profiling(1 if enable else 0)
