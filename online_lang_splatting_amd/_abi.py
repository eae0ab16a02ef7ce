"""ctypes mirror of include/olsr.h (struct olsr_scene, callback type, constants).

Pure declarations: importing this module loads no native code.
"""
import ctypes as C

OLSR_OK = 0
OLSR_ERR_ARG = -1
OLSR_ERR_DEVICE = -2
OLSR_ERR_ALLOC = -3
OLSR_ERR_CAPACITY = -4

BWD_REFERENCE = 0
BWD_EXACT = 1

ACT_OPACITY_SIGMOID = 1      # OLSR_ACT_*: the array holds the raw parameter, the kernels apply the activation
ACT_SCALE_EXP = 2
ACT_ROTATION_NORMALIZE = 4
ACT_ALL = 7
FLAG_ORACLE_KEEP_ZERO_DET = 0x100  # OLSR_FLAG_ORACLE_KEEP_ZERO_DET: oracle only; the library rejects it
FLAG_SIGNED_EMPTY_RADII = 1  # OLSR_FLAG_SIGNED_EMPTY_RADII: radii = -radius for a bounding square that covers no tile
FLAG_FWD_ACCUM_WEIGHT = 4    # OLSR_FLAG_FWD_ACCUM_WEIGHT: fma(alpha T, f, C) on the vector ALU (images to ~1e-7)
FLAG_FRAMES_IN_FLIGHT = 8    # OLSR_FLAG_FRAMES_IN_FLIGHT: several frames in flight on several streams -> four-wave radix blocks
FLAG_FWD_ACCUM_MFMA = 2      # OLSR_FLAG_FWD_ACCUM_MFMA: the forward's feature accumulation on the matrix cores (images to ~1e-7)

BINNING_RECT = 0     # every tile of the reference's bounding square (bit-identical instance lists)
BINNING_ELLIPSE = 1  # only tiles the alpha >= 1/255 ellipse reaches (identical outputs, shorter lists)

# olsr_debug_exp_sweep: the arguments the composites' exp can be handed and consume — float32 bit patterns, inclusive:
# -0 ... -90 (below the -87 clamp) and +0 ... +88 — and the specials every form must agree on as well
EXP_SWEEP_RANGES = ((0x80000000, 0xC2B40000), (0x00000000, 0x42B00000))
EXP_SWEEP_SPECIALS = (0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0xFFFFFFFF, 0xF149F2CA)  # +-inf, NaNs, -1e30

SUPPORTED_F = (0, 3, 15, 16, 32)
SUPPORTED_TILES = (15, 16)

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)

_fp = C.c_void_p  # device (or, for the oracle, host) float pointers travel as raw addresses


class OlsrScene(C.Structure):
    """struct olsr_scene, include/olsr.h."""

    _fields_ = [
        ("P", C.c_int32),
        ("D", C.c_int32),
        ("M", C.c_int32),
        ("F", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("tile", C.c_int32),
        ("prefiltered", C.c_int32),
        ("debug", C.c_int32),
        ("bwd_mode", C.c_int32),
        ("tan_fovx", C.c_float),
        ("tan_fovy", C.c_float),
        ("scale_modifier", C.c_float),
        ("binning", C.c_int32),
        ("background", _fp),
        ("means3D", _fp),
        ("shs", _fp),
        ("colors_precomp", _fp),
        ("language_precomp", _fp),
        ("opacities", _fp),
        ("scales", _fp),
        ("rotations", _fp),
        ("cov3D_precomp", _fp),
        ("viewmatrix", _fp),
        ("projmatrix", _fp),
        ("projmatrix_raw", _fp),
        ("cam_pos", _fp),
        ("activations", C.c_int32),
        ("flags", C.c_int32),
        ("tile_depth_cut", _fp),
        ("backward_row_capacity", C.c_int64),
        ("depth_order_carry", _fp),
    ]


class OlsrGradBucket(C.Structure):
    """struct olsr_grad_bucket, include/olsr.h."""

    _fields_ = [("flat", _fp), ("densify", _fp), ("max_radii", _fp), ("assign", C.c_int32), ("_pad0", C.c_int32),
                ("row_mask", _fp)]


class OlsrAdamParams(C.Structure):
    """struct olsr_adam_params, include/olsr.h."""

    _fields_ = [(n, C.c_double) for n in ("lr_xyz", "lr_sh_dc", "lr_sh_rest", "lr_opacity", "lr_scale", "lr_rotation",
                                           "lr_language", "beta1", "beta2", "eps")] + [("step", C.c_int32), ("_pad0", C.c_int32)]


class OlsrAdamGroupParams(C.Structure):
    """struct olsr_adam_group_params, include/olsr.h (group order: OLSR_ADAM_GROUP_*)."""

    _fields_ = [("base", OlsrAdamParams), ("group_step", C.c_int32 * 7), ("skip_mask", C.c_int32)]


class OlsrAdamReg(C.Structure):
    """struct olsr_adam_reg, include/olsr.h."""

    _fields_ = [("isotropic_weight", C.c_double), ("activations", C.c_int32), ("P_total", C.c_int32)]


# olsr_window_pose_step (OLSR_WINDOW_*)
WINDOW_MAX_VIEWS, WINDOW_OPT_POSE, WINDOW_OPT_EXPOSURE = 32, 1, 2

# OLSR_ADAM_GROUP_*: the reference's parameter groups (gaussian_model.py training_setup) in bucket-column order
ADAM_GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "f_language")

MAP_EDIT_DENSIFY, MAP_EDIT_MASK = 0, 1


class OlsrMapBuffers(C.Structure):
    """struct olsr_map_buffers, include/olsr.h."""

    _fields_ = [(n, _fp) for n in ("means3D", "shs", "opacities", "scales", "rotations", "language", "exp_avg", "exp_avg_sq",
                                   "kf_id", "n_obs", "stats", "max_radii")]


class OlsrMapEditParams(C.Structure):
    """struct olsr_map_edit_params, include/olsr.h."""

    _fields_ = [("mode", C.c_int32), ("n_append", C.c_int32), ("append_kf_id", C.c_int32), ("screen_size_term", C.c_int32),
                ("max_grad", C.c_float), ("min_opacity", C.c_float), ("clone_max_scale", C.c_float), ("big_scale", C.c_float)]


class OlsrKeyframeSeedParams(C.Structure):
    """struct olsr_keyframe_seed_params, include/olsr.h."""

    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("plane_stride", C.c_int64), ("M", C.c_int32), ("downsample", C.c_int32),
                ("seed", C.c_uint32), ("_pad0", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("rgb_boundary_threshold", C.c_float), ("depth_trunc", C.c_float),
                ("point_size", C.c_double), ("adaptive_pointsize", C.c_int32), ("capacity", C.c_int32)]


# the front end's frame step (OLSR_GRAD_MASK_*, OLSR_COVIS_*, OLSR_KEYFRAME_RECORD_*)
GRAD_MASK_BLOCKS, GRAD_MASK_GLOBAL, GRAD_MASK_MAX_BLOCK_PIXELS = 0, 1, 8192
COVIS_MAX_VIEWS, COVIS_COUNTS, KEYFRAME_RECORD_FLOATS, KEYFRAME_RECORD_BYTES = 16, 33, 40, 192


class OlsrCovisViews(C.Structure):
    """struct olsr_covis_views, include/olsr.h."""

    _fields_ = [("K", C.c_int32), ("_pad0", C.c_int32), ("vis", C.c_void_p * COVIS_MAX_VIEWS)]


class OlsrKeyframeDecideParams(C.Structure):
    """struct olsr_keyframe_decide_params, include/olsr.h."""

    _fields_ = [(n, C.c_int32) for n in ("window_len", "window_size", "check_time", "single_thread")] + [
        (n, C.c_float) for n in ("kf_translation", "kf_min_translation", "kf_overlap", "kf_cutoff")]


class OlsrPoseParams(C.Structure):
    """struct olsr_pose_params, include/olsr.h."""

    _fields_ = [(n, C.c_double) for n in ("lr_rot", "lr_trans", "lr_exposure", "beta1", "beta2", "eps",
                                           "converged_threshold")] + [("step", C.c_int32), ("_pad0", C.c_int32)]


BATCHNORM_FIELDS = ("weight", "bias", "running_mean", "running_var")


def _mlp_state(prefix, widths, stride, batchnorm):
    """The state_dict entries of an nn.Sequential of Linear layers `widths`, `stride` modules per layer (Linear, [BatchNorm1d,]
    activation), as ((name, shape), ...) in state_dict order, without num_batches_tracked."""
    out = []
    for k, (i, o) in enumerate(zip(widths, widths[1:])):
        out += [(f"{prefix}.{stride * k}.weight", (o, i)), (f"{prefix}.{stride * k}.bias", (o,))]
        if batchnorm and k < len(widths) - 2:   # BatchNorm1d on the layer's output, ahead of the ReLU
            out += [(f"{prefix}.{stride * k + 1}.{n}", (o,)) for n in BATCHNORM_FIELDS]
    return tuple(out)


def set_widths(p, widths):
    """Fills the n_widths / widths[] pair of a parameter struct; returns the struct."""
    p.n_widths = len(widths)
    p.widths[:len(widths)] = widths
    return p


# the online language autoencoder (OLSR_LANG_AE_*): compiled-in sizes, the flat parameter array in state_dict order
LANG_AE_IN, LANG_AE_HIDDEN, LANG_AE_CODE, LANG_AE_PARAMS = 32, 24, 15, 2351
LANG_AE_CODES_ROWS, LANG_AE_CODES_CHANNELS = 0, 1   # codes as [N,15] rows / as [15,N] = low_dim.T
LANG_AE_STATE = (_mlp_state("encoder", (LANG_AE_IN, LANG_AE_HIDDEN, LANG_AE_CODE), 2, False)
                 + _mlp_state("decoder", (LANG_AE_CODE, LANG_AE_HIDDEN, LANG_AE_IN), 2, False))


class OlsrLangAeParams(C.Structure):
    """struct olsr_lang_ae_params, include/olsr.h."""

    _fields_ = [(n, C.c_double) for n in ("lr", "beta1", "beta2", "eps")] + [
        (n, C.c_int32) for n in ("step", "code_layout", "in_dim", "hidden_dim", "code_dim", "_pad0")]


# text queries on a rendered language map (OLSR_LANG_QUERY_*): the general decoder AutoencoderMLP.decoder in state_dict order
LANG_QUERY_MAX_LAYERS, LANG_QUERY_MAX_PHRASES, LANG_QUERY_FEATURE_DIM, LANG_QUERY_DECODER_PARAMS = 8, 64, 768, 745536
LANG_QUERY_WANT_MASK, LANG_QUERY_WANT_LABELS = 1, 2
LANG_QUERY_WIDTHS = (32, 192, 256, 384, 512, 768)
LANG_QUERY_STATE = _mlp_state("decoder", LANG_QUERY_WIDTHS, 2, False)


class OlsrLangQueryParams(C.Structure):
    """struct olsr_lang_query_params, include/olsr.h."""

    _fields_ = [("n_widths", C.c_int32), ("widths", C.c_int32 * LANG_QUERY_MAX_LAYERS)] + [
        (n, C.c_int32) for n in ("K", "n_pos", "n_labels", "in_width", "in_height", "dec_width", "dec_height", "out_width",
                                 "out_height")] + [("thresh", C.c_float), ("flags", C.c_uint32)]


# the general language encoder (OLSR_LANG_ENCODER_*): AutoencoderMLP.encoder in state_dict order, without num_batches_tracked
LANG_ENCODER_PARAMS = 572128
LANG_ENCODER_IN_ROWS, LANG_ENCODER_IN_CHANNELS = 0, 1   # features as [N,768] rows / as [768] planes of a [1,768,h,w] map
LANG_ENCODER_WIDTHS = (768, 512, 256, 128, 64, 32)


LANG_ENCODER_STATE = _mlp_state("encoder", LANG_ENCODER_WIDTHS, 3, True)

# struct olsr_lang_encoder_params and struct olsr_ss_encoder_params declare the same members
_ENCODER_PARAMS_FIELDS = [("n_widths", C.c_int32), ("widths", C.c_int32 * 8), ("in_layout", C.c_int32), ("code_layout", C.c_int32),
                          ("plane_stride", C.c_int64), ("bn_eps", C.c_double)]


class OlsrLangEncoderParams(C.Structure):
    """struct olsr_lang_encoder_params, include/olsr.h."""

    _fields_ = _ENCODER_PARAMS_FIELDS


# the single-stage chain 768 -> 15 -> 768 (include/olsr_single_stage.h): one AutoencoderMLP, no online autoencoder
SS_ENCODER_PARAMS, SS_DECODER_PARAMS = 396927, 542544
SS_ENCODER_WIDTHS = (768, 384, 192, 96, 48, 24, 15)
SS_DECODER_WIDTHS = (15, 24, 48, 96, 192, 384, 384, 768)


SS_ENCODER_STATE = _mlp_state("encoder", SS_ENCODER_WIDTHS, 3, True)
SS_DECODER_STATE = _mlp_state("decoder", SS_DECODER_WIDTHS, 2, False)


# a frame's ingest (include/olsr_frame_ingest.h)
INGEST_DEPTH_U16, INGEST_DEPTH_F32 = 0, 1


class OlsrFrameIngestParams(C.Structure):
    """struct olsr_frame_ingest_params, include/olsr_frame_ingest.h."""

    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("depth_type", C.c_int32), ("_pad0", C.c_int32),
                ("plane_stride", C.c_int64), ("depth_scale", C.c_double)]


# the map's point_cloud.ply record (include/olsr_map_io.h, OLSR_MAP_PLY_*)
MAP_PLY_MAX_M, MAP_PLY_MAX_F, MAP_PLY_MAX_WIDTH, MAP_PLY_BLOCK_ROWS, MAP_PLY_MAX_COLS = 16, 32, 94, 64, 6016


class OlsrSsEncoderParams(C.Structure):
    """struct olsr_ss_encoder_params, include/olsr_single_stage.h."""

    _fields_ = _ENCODER_PARAMS_FIELDS


# the high-resolution language feature net (OLSR_HR_NET_*): HighResLanguageFeatureNet's layers in forward order as
# (module path, kind, out, in, BatchNorm path or None); kind "conv1" / "conv3" is nn.Conv2d [out,in,k,k], "convT" is
# nn.ConvTranspose2d(4, 2, 1) [in,out,4,4].  The packed array holds, per layer, taps x [out][in] | bias | BatchNorm [4][out].
HR_NET_PARAMS = 19890816
HR_NET_LAUNCHES = 13
HR_NET_CHANNELS = (768, 384, 192, 768)   # fv, f3, f2, out
HR_NET_TAPS = {"conv1": 1, "conv3": 9, "convT": 16}
HR_NET_LAYERS = (
    ("initial_conv.0", "conv3", 512, 768, "initial_conv.1"),
    ("upsample1.0", "convT", 512, 512, "upsample1.1"),
    ("attention_fusion1.low_res_align", "conv1", 512, 384, None),
    ("attention_fusion1.fusion.0", "conv3", 512, 1024, "attention_fusion1.fusion.1"),
    ("attention_fusion1.attention.0", "conv3", 512, 512, "attention_fusion1.attention.1"),
    ("attention_fusion1.attention.3", "conv1", 512, 512, None),
    ("upsample2.0", "convT", 256, 512, "upsample2.1"),
    ("attention_fusion2.low_res_align", "conv1", 256, 192, None),
    ("attention_fusion2.fusion.0", "conv3", 256, 512, "attention_fusion2.fusion.1"),
    ("attention_fusion2.attention.0", "conv3", 256, 256, "attention_fusion2.attention.1"),
    ("attention_fusion2.attention.3", "conv1", 256, 256, None),
    ("upsample3.0", "convT", 128, 256, "upsample3.1"),
    ("final_conv", "conv1", 768, 128, None),
)
HR_NET_BN_FIELDS = BATCHNORM_FIELDS


def _hr_net_state():
    out = []
    for path, kind, o, i, bn in HR_NET_LAYERS:
        k = {"conv1": 1, "conv3": 3, "convT": 4}[kind]
        out += [(f"{path}.weight", (i, o, k, k) if kind == "convT" else (o, i, k, k)), (f"{path}.bias", (o,))]
        if bn:
            out += [(f"{bn}.{n}", (o,)) for n in HR_NET_BN_FIELDS]
    return tuple(out)


HR_NET_STATE = _hr_net_state()   # state_dict order of the module, without num_batches_tracked


class OlsrHrNetParams(C.Structure):
    """struct olsr_hr_net_params, include/olsr.h."""

    _fields_ = [(n, C.c_int32) for n in ("h", "w", "h3", "w3", "h2", "w2", "c_fv", "c_f3", "c_f2", "c_out")] + [
        ("launches", C.c_uint32), ("_pad0", C.c_int32)] + [
        (n, C.c_int64) for n in ("fv_stride", "f3_stride", "f2_stride", "out_stride")] + [
        ("bn_eps", C.c_double), ("workspace_bytes", C.c_uint64)]


# the CLIP ConvNeXt image tower (include/olsr_clip_trunk.h, OLSR_CLIP_TRUNK_*)
CLIP_TRUNK_FUSED_MAX_C, CLIP_TRUNK_MAX_LAUNCHES, CLIP_TRUNK_MAX_DIM = 256, 128, 4096
CLIP_TRUNK_DEPTHS, CLIP_TRUNK_DIMS, CLIP_TRUNK_EMBED = (3, 3, 27, 3), (192, 384, 768, 1536), 768   # convnext_large_d_320
CLIP_PIXEL_MEAN = (122.7709383, 116.7460125, 104.09373615)   # language/sed/config.py:67-68
CLIP_PIXEL_STD = (68.5005327, 66.6321579, 70.3231630)
CLIP_LN_EPS = 1e-6


class OlsrConvnextBlockParams(C.Structure):
    """struct olsr_convnext_block_params, include/olsr_clip_trunk.h."""

    _fields_ = [("C", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("_pad0", C.c_int32), ("ln_eps", C.c_double),
                ("workspace_bytes", C.c_uint64)]


class OlsrClipTrunkParams(C.Structure):
    """struct olsr_clip_trunk_params, include/olsr_clip_trunk.h."""

    _fields_ = [("depths", C.c_int32 * 4), ("dims", C.c_int32 * 4), ("embed_dim", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("R", C.c_int32), ("mean", C.c_float * 3), ("std", C.c_float * 3), ("_pad0", C.c_int32),
                ("_pad1", C.c_int32), ("ln_eps", C.c_double), ("launches", C.c_uint64 * 2), ("workspace_bytes", C.c_uint64)]


def clip_block_state(prefix, c):
    """((state_dict name, shape), ...) of one ConvNeXt block of c channels, in the packed order."""
    return ((f"{prefix}.conv_dw.weight", (c, 1, 7, 7)), (f"{prefix}.conv_dw.bias", (c,)), (f"{prefix}.norm.weight", (c,)),
            (f"{prefix}.norm.bias", (c,)), (f"{prefix}.mlp.fc1.weight", (4 * c, c)), (f"{prefix}.mlp.fc1.bias", (4 * c,)),
            (f"{prefix}.mlp.fc2.weight", (c, 4 * c)), (f"{prefix}.mlp.fc2.bias", (c,)), (f"{prefix}.gamma", (c,)))


def clip_trunk_state(depths, dims, embed_dim, root="visual."):
    """((state_dict name, shape), ...) of the tower in the packed order: the names of open_clip's TimmModel around timm's
    ConvNeXt, restated from memory (timm is not a dependency and no checkpoint was at hand: unverified)."""
    t = root + "trunk."
    out = [(t + "stem.0.weight", (dims[0], 3, 4, 4)), (t + "stem.0.bias", (dims[0],)), (t + "stem.1.weight", (dims[0],)),
           (t + "stem.1.bias", (dims[0],))]
    for i in range(4):
        s = f"{t}stages.{i}."
        if i > 0:
            out += [(s + "downsample.0.weight", (dims[i - 1],)), (s + "downsample.0.bias", (dims[i - 1],)),
                    (s + "downsample.1.weight", (dims[i], dims[i - 1], 2, 2)), (s + "downsample.1.bias", (dims[i],))]
        for j in range(depths[i]):
            out += clip_block_state(f"{s}blocks.{j}", dims[i])
    out += [(t + "head.norm.weight", (dims[3],)), (t + "head.norm.bias", (dims[3],)),
            (root + "head.proj.weight", (embed_dim, dims[3]))]
    return tuple(out)


# point-cloud metrics (OLSR_CLOUD_*)
CLOUD_MAX_SEGMENTS = 32767

# scoring text queries (OLSR_QUERY_EVAL_*); the columns of olsr_query_eval's result
QUERY_EVAL_MAX_PLANES, QUERY_EVAL_MAX_EXTENT = 65535, 1 << 20
QUERY_EVAL_RESULT = ("intersection", "union", "n_max", "hit")

# TSDF fusion (OLSR_TSDF_*)
TSDF_MAX_VIEWS = 16
TSDF_FEAT_FLOAT, TSDF_FEAT_PACKED_RGB = 0, 1
TSDF_IMAGE_CHANNELS, TSDF_IMAGE_ROWS = 0, 1   # a view's features as [F,H,W] (what the rasteriser returns) / as [H,W,F]


class OlsrTsdfVolume(C.Structure):
    """struct olsr_tsdf_volume, include/olsr.h."""

    _fields_ = [(n, C.c_int32) for n in ("X", "Y", "Z", "F", "feat_mode")] + [
        ("voxel_size", C.c_float), ("trunc_margin", C.c_float), ("origin", C.c_float * 3),
        ("tsdf", _fp), ("weight", _fp), ("feat", _fp)]


class OlsrTsdfView(C.Structure):
    """struct olsr_tsdf_view, include/olsr.h."""

    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy")] + [("pose", C.c_float * 16), ("obs_weight", C.c_float),
                ("min_opacity", C.c_float), ("H", C.c_int32), ("W", C.c_int32), ("feat_layout", C.c_int32), ("_pad0", C.c_int32),
                ("depth", _fp), ("feat", _fp), ("opacity", _fp)]


class OlsrLossParams(C.Structure):
    """struct olsr_loss_params, include/olsr.h."""

    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("F", C.c_int32), ("lang_width", C.c_int32),
                ("lang_height", C.c_int32), ("initialization", C.c_int32), ("alpha", C.c_float),
                ("rgb_boundary_threshold", C.c_float), ("lamda_lang", C.c_float), ("one_minus_alpha", C.c_float)]


class OlsrLossFusion(C.Structure):
    """struct olsr_loss_fusion, include/olsr.h: the loss evaluated in the forward composite's epilogue."""

    _fields_ = [("params", OlsrLossParams), ("tracking", C.c_int32), ("skip_images", C.c_int32), ("gt_image", _fp),
                ("gt_depth", _fp), ("gt_language", _fp), ("exposure", _fp), ("grad_mask", _fp), ("dL_dimage", _fp),
                ("dL_ddepth", _fp), ("dL_dlanguage", _fp), ("loss", _fp), ("dL_dexposure", _fp), ("scratch", _fp)]


def ptr(t):
    """data_ptr of a tensor, or None for an absent (None / empty) one — the reference maps
    empty tensors to nullptr the same way (contiguous().data<float>() of a 0-element tensor,
    tested with `!= nullptr` in CR/forward.cu:320,356)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def make_scene(*, P, D, M, F, width, height, tile, prefiltered, debug, bwd_mode, tan_fovx, tan_fovy,
               scale_modifier, binning=BINNING_RECT, activations=0, flags=0, background, means3D, shs, colors_precomp, language_precomp, opacities,
               scales, rotations, cov3D_precomp, viewmatrix, projmatrix, projmatrix_raw, cam_pos, tile_depth_cut=None,
               backward_row_capacity=0, depth_order_carry=None):
    s = OlsrScene()
    s.P, s.D, s.M, s.F = int(P), int(D), int(M), int(F)
    s.width, s.height, s.tile = int(width), int(height), int(tile)
    s.prefiltered, s.debug, s.bwd_mode = int(bool(prefiltered)), int(bool(debug)), int(bwd_mode)
    s.tan_fovx, s.tan_fovy, s.scale_modifier = float(tan_fovx), float(tan_fovy), float(scale_modifier)
    s.binning = int(binning)
    s.activations = int(activations)
    s.flags = int(flags)
    s.background = ptr(background)
    s.means3D = ptr(means3D)
    s.shs = ptr(shs)
    s.colors_precomp = ptr(colors_precomp)
    s.language_precomp = ptr(language_precomp)
    s.opacities = ptr(opacities)
    s.scales = ptr(scales)
    s.rotations = ptr(rotations)
    s.cov3D_precomp = ptr(cov3D_precomp)
    s.viewmatrix = ptr(viewmatrix)
    s.projmatrix = ptr(projmatrix)
    s.projmatrix_raw = ptr(projmatrix_raw)
    s.cam_pos = ptr(cam_pos)
    s.tile_depth_cut = ptr(tile_depth_cut)
    s.backward_row_capacity = int(backward_row_capacity)
    s.depth_order_carry = ptr(depth_order_carry)
    return s
