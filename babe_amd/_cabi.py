"""The C-ABI of libbabe_hip.so as ctypes sees it: one mirror of every struct of include/babe_hip.h that crosses the boundary and ONE
table of every entry point Python calls (the package, tools/, tests/).  A function called without argtypes gets its Python ints
converted to 32-bit C ints - a device pointer passed that way is silently truncated - so nothing reaches the library except
through this table: `bind` applies all of it when the library is loaded, and the object it returns has no other babe_* name.
The table is checked against the header, and the structs against a C compiler's layout, by tests/test_cabi_exports.py; a new
entry point is one line here."""
import ctypes as C


class ConvArgs(C.Structure):
    """babe_conv_args"""
    _fields_ = [
        ("in_", C.c_void_p), ("in_bs", C.c_long), ("in_cs", C.c_long),
        ("in2", C.c_void_p), ("in2_bs", C.c_long), ("in2_cs", C.c_long), ("cin_split", C.c_int),
        ("w_packed", C.c_void_p),
        ("out", C.c_void_p), ("out_bs", C.c_long), ("out_cs", C.c_long),
        ("res", C.c_void_p), ("res_bs", C.c_long), ("res_cs", C.c_long),
        ("in_scale", C.c_void_p), ("oscale", C.c_void_p),
        ("alpha", C.c_float), ("rbeta", C.c_float),
        ("B", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("F", C.c_int), ("T", C.c_int),
        ("KH", C.c_int), ("KW", C.c_int), ("dil", C.c_int),
        # optional reduction fused into the F(4,5) kernels' epilogue (include/babe_hip.h; zero = off)
        ("stat_mode", C.c_int), ("stat_cg", C.c_int), ("stat_x", C.c_void_p), ("stat_scale", C.c_void_p), ("stat_part", C.c_void_p),
        ("fbias", C.c_void_p),                          # [Cout][F] bias per channel and frequency row (the (1,1) fp32 kernels)
    ]


class WgradArgs(C.Structure):
    """babe_wgrad_args: operands of the conv weight gradient."""
    _fields_ = [("x", C.c_void_p), ("x_bs", C.c_long), ("x_cs", C.c_long),
                ("x2", C.c_void_p), ("x2_bs", C.c_long), ("x2_cs", C.c_long), ("cin_split", C.c_int),
                ("g", C.c_void_p), ("g_bs", C.c_long), ("g_cs", C.c_long),
                ("B", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("F", C.c_int), ("T", C.c_int),
                ("KH", C.c_int), ("KW", C.c_int), ("dil", C.c_int)]


class CPackedConv(C.Structure):
    """babe_packed_conv: the images of one ops.PackedConv (its `desc`), for babe_conv2d_auto and the UNet plan."""
    _fields_ = [("Cout", C.c_int), ("Cin", C.c_int), ("KH", C.c_int), ("KW", C.c_int), ("nt", C.c_int), ("splits", C.c_int),
                ("fwd", C.c_void_p), ("bwd", C.c_void_p), ("fwd_wino", C.c_void_p), ("bwd_wino", C.c_void_p),
                ("fwd_wino4", C.c_void_p), ("bwd_wino4", C.c_void_p), ("fwd_wino45", C.c_void_p), ("bwd_wino45", C.c_void_p),
                ("w_raw", C.c_void_p), ("fwd_wino85", C.c_void_p), ("bwd_wino85", C.c_void_p)]


class PackedConvLayout(C.Structure):
    """babe_packed_conv_layout: babe_packed_conv_plan's answer; bytes in the order of IMAGE_SLOTS"""
    _fields_ = [("nt", C.c_int), ("splits", C.c_int), ("raw", C.c_int), ("bytes", C.c_long * 10)]


IMAGE_SLOTS = ("fwd", "bwd", "fwd_wino", "bwd_wino", "fwd_wino4", "bwd_wino4", "fwd_wino45", "bwd_wino45", "fwd_wino85", "bwd_wino85")


class CAttn(C.Structure):
    """babe_unet_attn: the time-attention branch of a block (networks/unet_engine.py::_Attn)."""
    _fields_ = [("H", C.c_int), ("F", C.c_int), ("scale", C.c_float),
                ("proj_in", CPackedConv), ("qk", CPackedConv), ("proj_out", CPackedConv),
                ("gamma", C.c_void_p), ("film_aff", C.c_int), ("film_gate", C.c_int),
                ("qk_bias", C.c_void_p), ("emb", C.c_void_p), ("num_buckets", C.c_int), ("max_distance", C.c_int)]


class AttnBucketThr(C.Structure):
    """babe_attn_bucket_thr: the host data of the bucket-table kernel (babe_attn_bucket_thresholds)."""
    _fields_ = [("half", C.c_int), ("max_distance", C.c_int), ("thr", C.c_int * 32)]


class CBlock(C.Structure):
    """babe_unet_block"""
    _fields_ = [("N", C.c_int), ("nd", C.c_int), ("k53", C.c_int),
                ("proj_in", CPackedConv), ("res_conv", CPackedConv), ("proj_out", CPackedConv), ("H", CPackedConv * 8),
                ("gamma", C.c_void_p * 8), ("film_aff", C.c_int * 8), ("film_gate", C.c_int * 8),
                ("fb_proj_in", C.c_void_p), ("fb_res_conv", C.c_void_p), ("attn", C.POINTER(CAttn))]


class PwArgs(C.Structure):
    """babe_pw_args: the operands of one fused (1,1) ResnetBlock pass (csrc/pw_block.hip)."""
    _fields_ = [("B", C.c_int), ("F", C.c_int), ("T", C.c_int), ("S", C.c_int), ("plan_splits", C.c_int),
                ("z", C.c_void_p), ("z_bs", C.c_long), ("z_cs", C.c_long),
                ("x", C.c_void_p), ("x_bs", C.c_long), ("x_cs", C.c_long),
                ("out", C.c_void_p), ("out_bs", C.c_long), ("out_cs", C.c_long),
                ("add", C.c_void_p), ("add_bs", C.c_long), ("add_cs", C.c_long),
                ("part", C.c_void_p), ("film", C.c_void_p), ("film_bs", C.c_long), ("gate", C.c_void_p),
                ("stats", C.c_void_p), ("scale", C.c_void_p)]


class CPlanDesc(C.Structure):
    """babe_unet_plan_desc"""
    _fields_ = [("nocts", C.c_int), ("bpo", C.c_int), ("Ns", C.c_int * 8),
                ("init_blk", CBlock * 8), ("main_blk", CBlock * 8), ("up_out", CBlock * 8), ("up_blk", CBlock * 8),
                ("mid_blk", CBlock), ("mid_out", CBlock), ("pyr_conv", CPackedConv * 8), ("attn_core", C.c_int)]


# babe_unet_plan_desc.attn_core / babe_model_options.attention, by the attention core's name (UnetEngine.attn_core)
ATTN_CORES = {None: 0, "f32": 1, "bf16": 2}


class CqtBands(C.Structure):
    """babe_cqt_bands"""
    _fields_ = [("nbands", C.c_int), ("L", C.c_int), ("KX", C.c_int),
                ("c", C.c_void_p), ("M", C.c_void_p), ("woff", C.c_void_p), ("log2T", C.c_void_p),
                ("oct", C.c_void_p), ("binoct", C.c_void_p), ("tw4096", C.c_void_p),
                ("nocts", C.c_int), ("binsoct", C.c_int), ("coef", C.c_void_p * 8),
                ("wg_first", C.c_void_p), ("wg_count", C.c_void_p), ("nwg", C.c_int),
                ("wg_rec", C.c_void_p), ("band_rec", C.c_void_p), ("reserved", C.c_int),
                ("max_wg_count", C.c_int), ("min_log2T", C.c_int), ("max_log2T", C.c_int),
                ("sum_T", C.c_long), ("sum_M", C.c_long), ("sum_TlogT", C.c_double),
                ("kdeg", C.c_int), ("kpoly", C.c_float * 12)]


class FitCfg(C.Structure):
    """babe_fit_cfg"""
    _fields_ = [("mu_fc", C.c_float), ("mu_A", C.c_float), ("tol_fc", C.c_float), ("tol_A", C.c_float),
                ("fcmin", C.c_float), ("fcmax", C.c_float), ("Amin", C.c_float), ("Amax", C.c_float),
                ("max_iter", C.c_int), ("clamp_fc", C.c_int), ("clamp_A", C.c_int), ("only_negative_A", C.c_int),
                ("weighting", C.c_int), ("kernel", C.c_int)]


class EvalDesc(C.Structure):
    """babe_eval_desc"""
    _fields_ = [("unet_plan", C.c_void_p), ("unet_state", C.c_void_p), ("cqt_plan", C.c_void_p), ("L", C.c_int),
                ("rff_freq", C.c_void_p), ("rff_n", C.c_int),
                ("emb_W", C.c_void_p * 3), ("emb_b", C.c_void_p * 3), ("emb_dim", C.c_int * 4),
                ("film_W", C.c_void_p), ("film_b", C.c_void_p), ("film_J", C.c_int),
                ("nfft", C.c_int), ("fs", C.c_float), ("env_inv", C.c_void_p), ("tw4096", C.c_void_p), ("K", C.c_int),
                ("fit", FitCfg), ("blind", C.c_int), ("shared", C.c_int), ("hpf", C.c_int),
                ("xi", C.c_float), ("score_mode", C.c_int), ("audio_len_norm", C.c_float),
                ("mask", C.c_void_p), ("mask_bs", C.c_long), ("dc_mask", C.c_void_p), ("dc_y", C.c_void_p),
                # the known observation model (all zero: the STFT filter) and the classic replacement step
                ("obs_kind", C.c_int), ("taps", C.c_void_p), ("ntaps", C.c_int),
                ("b", C.c_void_p), ("a", C.c_void_p), ("order", C.c_int), ("clamp", C.c_int),
                ("obs_mask", C.c_void_p), ("obs_mask_bs", C.c_long), ("clip_value", C.c_float), ("dc_classic", C.c_int)]


# babe_eval_desc.obs_kind
OBS_STFT, OBS_FIR, OBS_IIR, OBS_MASK, OBS_CLIP = range(5)


class SampleStep(C.Structure):
    """babe_sample_step"""
    _fields_ = [("t_hat", C.c_float), ("inject", C.c_float), ("t_next", C.c_float), ("h", C.c_float), ("heun", C.c_int),
                ("c1", C.c_float * 4), ("c2", C.c_float * 4)]


class SampleDesc(C.Structure):
    """babe_sample_desc"""
    _fields_ = [("eval", EvalDesc), ("T", C.c_int), ("steps", C.POINTER(SampleStep)), ("t0", C.c_float), ("warm_start", C.c_int),
                ("skip_zero_inject", C.c_int)]


class RecordingDesc(C.Structure):
    """babe_recording_desc"""
    _fields_ = [("eval", EvalDesc), ("T", C.c_int), ("t0", C.c_float), ("warm_start", C.c_int),
                ("steps_blind", C.POINTER(SampleStep)), ("steps_known", C.POINTER(SampleStep)),
                ("n_blind", C.c_int), ("blind_starts", C.c_long * 16), ("init_params", C.c_void_p),
                ("target_std", C.c_float), ("overlap", C.c_long), ("discard_end", C.c_long),
                ("inpaint_dc", C.c_int), ("dc_size", C.c_int), ("dc_window", C.c_void_p), ("std_dev", C.c_void_p)]


class DnConvArgs(C.Structure):
    """babe_dnconv_args"""
    _fields_ = [("in_", C.c_void_p), ("in_bs", C.c_long), ("in_cs", C.c_long), ("IH", C.c_int), ("IW", C.c_int),
                ("bias", C.c_void_p),
                ("out", C.c_void_p), ("out_bs", C.c_long), ("out_cs", C.c_long), ("out_H", C.c_int), ("out_W", C.c_int),
                ("out_hstep", C.c_int), ("out_h0", C.c_int), ("out_wstep", C.c_int), ("out_w0", C.c_int),
                ("res", C.c_void_p), ("res_bs", C.c_long), ("res_cs", C.c_long),
                ("B", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("OH", C.c_int), ("OW", C.c_int),
                ("KH", C.c_int), ("KW", C.c_int), ("stride", C.c_int), ("pad_t", C.c_int), ("pad_l", C.c_int),
                ("pad_mode", C.c_int), ("act", C.c_int), ("ksplit", C.c_int), ("ws", C.c_void_p)]


class ModelEntry(C.Structure):
    """babe_model_entry"""
    _fields_ = [("name", C.c_char_p), ("ndim", C.c_int), ("shape", C.c_long * 4), ("data", C.c_void_p)]


class ModelKV(C.Structure):
    """babe_model_kv"""
    _fields_ = [("key", C.c_char_p), ("str", C.c_char_p), ("num", C.c_double)]


class ModelOptions(C.Structure):
    """babe_model_options"""
    _fields_ = [("precision", C.c_int), ("attention", C.c_int), ("reserved", C.c_int * 6)]


class ModelSummary(C.Structure):
    """babe_model_summary"""
    _fields_ = [("L", C.c_int), ("fs", C.c_float), ("nocts", C.c_int), ("bpo", C.c_int), ("Ns", C.c_int * 8),
                ("params", C.c_long), ("device_bytes", C.c_long), ("cqt_device_bytes", C.c_long), ("device", C.c_int),
                ("load_ms", C.c_double * 3)]


class DenoiserSummary(C.Structure):
    """babe_denoiser_summary"""
    _fields_ = [("depth", C.c_int), ("num_tfc", C.c_int), ("num_stages", C.c_int), ("use_SAM", C.c_int), ("use_fencoding", C.c_int),
                ("f_dim", C.c_int), ("sample_rate", C.c_int), ("win", C.c_int), ("hop", C.c_int), ("segment", C.c_long),
                ("params", C.c_long), ("device_bytes", C.c_long), ("device", C.c_int), ("load_ms", C.c_double * 3)]


class SincTable(C.Structure):
    """babe_sinc_table"""
    _fields_ = [("kernel", C.c_void_p), ("krange", C.c_void_p), ("width", C.c_int), ("orig", C.c_int), ("new_", C.c_int)]


class FileDesc(C.Structure):
    """babe_file_desc"""
    _fields_ = [("rec", RecordingDesc), ("denoiser", C.c_void_p), ("conv", SincTable * 2), ("lengths", C.c_long * 3)]


class OptTensor(C.Structure):
    """babe_opt_tensor"""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("ema", C.c_void_p), ("n", C.c_long)]


class OptChunk(C.Structure):
    """babe_opt_chunk"""
    _fields_ = [("off", C.c_long), ("t", C.c_int), ("n", C.c_int)]


# header struct name -> mirror (the layout test compiles a probe for each of them)
STRUCTS = {"babe_conv_args": ConvArgs, "babe_wgrad_args": WgradArgs, "babe_packed_conv": CPackedConv,
           "babe_packed_conv_layout": PackedConvLayout, "babe_unet_block": CBlock, "babe_pw_args": PwArgs,
           "babe_unet_plan_desc": CPlanDesc, "babe_cqt_bands": CqtBands, "babe_fit_cfg": FitCfg, "babe_eval_desc": EvalDesc,
           "babe_dnconv_args": DnConvArgs, "babe_sample_step": SampleStep, "babe_sample_desc": SampleDesc,
           "babe_recording_desc": RecordingDesc,
           "babe_model_entry": ModelEntry, "babe_model_kv": ModelKV, "babe_model_summary": ModelSummary,
           "babe_denoiser_summary": DenoiserSummary, "babe_sinc_table": SincTable, "babe_file_desc": FileDesc,
           "babe_opt_tensor": OptTensor, "babe_opt_chunk": OptChunk,
           "babe_unet_attn": CAttn, "babe_attn_bucket_thr": AttnBucketThr, "babe_model_options": ModelOptions}

# C type -> ctypes: void* (and every data pointer; hipStream_t), long, int, float, double, const char*; None = void
_P, _L, _I, _F, _D, _S = C.c_void_p, C.c_long, C.c_int, C.c_float, C.c_double, C.c_char_p

# name -> (restype, [argtypes]), in the header's order
SIGS = {
    "babe_version": (_S, []),
    "babe_last_error": (_S, []),
    "babe_conv2d_wino85_stat_slots": (_I, [C.POINTER(ConvArgs)]),
    "babe_conv_packed_size": (_L, [_I, _I, _I, _I, _I]),
    "babe_conv_pack_weights_nt": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "babe_conv_pack_weights_bf16": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "babe_conv_packed_size_bf16": (_L, [_I, _I, _I, _I, _I, _I]),
    "babe_units_size": (_L, [_I, _I, _I]),
    "babe_scale_gelu_units": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "babe_conv2d_bf16_units_supported": (_I, [C.POINTER(ConvArgs)]),
    "babe_conv2d_bf16_units": (_I, [C.POINTER(ConvArgs), _P, _P]),
    "babe_conv2d_wino_supported": (_I, [C.POINTER(ConvArgs)]),
    "babe_conv_pack_weights_wino": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "babe_conv_packed_size_wino": (_L, [_I, _I, _I, _I]),
    "babe_conv2d_wino4_supported": (_I, [C.POINTER(ConvArgs)]),
    "babe_conv_pack_weights_wino4": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "babe_conv_packed_size_wino4": (_L, [_I, _I, _I, _I]),
    "babe_conv2d_wino45": (_I, [C.POINTER(ConvArgs), _P, _P]),
    "babe_conv2d_wino45_supported": (_I, [C.POINTER(ConvArgs)]),
    "babe_conv2d_wino45_preferred": (_I, [C.POINTER(ConvArgs)]),
    "babe_conv2d_fewco_supported": (_I, [C.POINTER(ConvArgs)]),
    "babe_conv_pack_weights_wino45": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "babe_conv_packed_size_wino45": (_L, [_I, _I, _I]),
    "babe_prof_nslots": (_I, []),
    "babe_prof_slot_name": (_S, [_I]),
    "babe_prof_enable": (_I, [_I]),
    "babe_prof_conv_slot": (_I, [_I]),
    "babe_prof_read": (_I, [_P, _P, _P, _P, _P]),
    "babe_prof_dispatch_counts": (_I, [_P, _I]),
    "babe_prof_timeline": (_L, [_P, _P, _P, _P, _P, _L]),
    "babe_prof_pending": (_L, []),
    "babe_gn_splits": (_L, [_L]),
    "babe_gn_partial": (_I, [_P, _P, _I, _I, _L, _I, _P]),
    "babe_gn_stats": (_I, [_P, _P, _P, _P, _P, _L, _P, _P, _I, _I, _I, _L, _I, _F, _P]),
    "babe_gn_finalize": (_I, [_P, _P, _P, _L, _P, _P, _I, _I, _I, _L, _I, _F, _P]),
    "babe_scale_gelu_fin": (_I, [_P, _P, _P, _P, _L, _P, _P, _P, _I, _I, _I, _L, _I, _F, _P]),
    "babe_scale_gelu": (_I, [_P, _P, _P, _I, _I, _L, _P]),
    "babe_gn_bwd_partial": (_I, [_P, _P, _P, _P, _I, _I, _I, _L, _I, _P]),
    "babe_gn_bwd_apply": (_I, [_P, _P, _P, _P, _P, _P, _P, _F, _I, _I, _I, _L, _I, _F, _P]),
    "babe_gn_bwd_apply_merge": (_I, [_P, _P, _P, _P, _P, _P, _P, _F, _I, _I, _I, _L, _I, _F, _P, _P, _F, _F]),
    "babe_gn_bwd_partial_nogelu": (_I, [_P, _P, _P, _P, _I, _I, _I, _L, _I, _P]),
    "babe_gn_bwd_apply_nogelu": (_I, [_P, _P, _P, _P, _P, _P, _P, _F, _I, _I, _I, _L, _I, _F, _P]),
    "babe_resample": (_I, [_P, _L, _L, _P, _L, _L, _I, _I, _I, _I, _I, _F, _F, _P]),
    "babe_resample_res": (_I, [_P, _L, _L, _P, _L, _L, _P, _L, _L, _I, _I, _I, _I, _I, _F, _F, _P]),
    "babe_resample_sinc": (_I, [_P, _L, _P, _L, _I, _L, _L, _P, _P, _I, _I, _I, _P]),
    "babe_resample_sinc_adjoint": (_I, [_P, _L, _P, _L, _I, _L, _L, _P, _P, _I, _I, _I, _P]),
    "babe_iir_workspace": (_L, [_I, _L, _I]),
    "babe_iir_filter": (_I, [_P, _L, _P, _L, _I, _L, _P, _P, _I, _I, _I, _P, _L, _P, _L, _P]),
    "babe_decimate": (_I, [_P, _L, _P, _L, _I, _L, _L, _I, _I, _P]),
    "babe_clip_residual": (_I, [_P, _L, _P, _L, _F, _P, _L, _P, _L, _P, _I, _I, _L, _P]),
    "babe_clip_fwd": (_I, [_P, _L, _F, _P, _L, _I, _L, _P]),
    "babe_clip_adj": (_I, [_P, _L, _P, _L, _P, _L, _I, _L, _P]),
    "babe_specnorm_workspace": (_L, [_I, _I, _I]),
    "babe_specnorm_seed": (_I, [_P, _L, _I, _I, _I, _P, _L, _I, _P, _L, _P]),
    "babe_stft_mag_workspace": (_L, [_I, _I, _I]),
    "babe_stft_mag_fwd": (_I, [_P, _L, _L, _P, _I, _I, _P, _P, _I, _I, _P, _P]),
    "babe_stft_mag_vjp": (_I, [_P, _P, _P, _I, _I, _P, _L, _L, _I, _I, _P, _P, _L, _P]),
    "babe_conv_packed_size_wino85": (_L, [_I, _I, _I]),
    "babe_conv_pack_weights_wino85": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "babe_conv2d_wino85_supported": (_I, [C.POINTER(ConvArgs)]),
    "babe_conv2d_wino85_preferred": (_I, [C.POINTER(ConvArgs)]),
    "babe_conv2d_wino85": (_I, [C.POINTER(ConvArgs), _P, _P]),
    "babe_conv2d_wino85_set_waves": (_I, [_I]),
    "babe_packed_conv_plan": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(PackedConvLayout)]),
    "babe_conv_splits_for": (_I, [_I, _I, _I, _I, _I, _I]),
    "babe_conv2d_bf16_units_shape": (_I, [C.POINTER(CPackedConv), _I]),
    "babe_packed_conv_pack": (_I, [C.POINTER(CPackedConv), _P, _P]),
    "babe_conv2d_auto": (_I, [C.POINTER(ConvArgs), C.POINTER(CPackedConv), _I, _P]),
    "babe_unet_plan_create": (_P, [C.POINTER(CPlanDesc)]),
    "babe_unet_plan_destroy": (None, [_P]),
    "babe_unet_state_create": (_P, []),
    "babe_unet_state_destroy": (None, [_P]),
    "babe_unet_workspace_bytes": (_L, [_P, _I, C.POINTER(_I)]),
    "babe_unet_fwd": (_I, [_P, _P, C.POINTER(_P), _P, _L, _I, C.POINTER(_I), _P, _L, C.POINTER(_P), _P]),
    "babe_unet_vjp": (_I, [_P, _P, C.POINTER(_P), C.POINTER(_P), _P]),
    "babe_unet_form_get": (_I, [_I]),
    "babe_unet_form_set": (_I, [_I, _I]),
    "babe_pw_block_enable": (_I, [_I]),
    "babe_pw_block_supported": (_I, [C.POINTER(CBlock), C.POINTER(PwArgs), _I]),
    "babe_pw_block_fwd": (_I, [C.POINTER(CBlock), C.POINTER(PwArgs), _P]),
    "babe_axpby4d": (_I, [_P, _L, _L, _P, _L, _L, _I, _I, _I, _I, _F, _F, _P]),
    "babe_fill4d": (_I, [_P, _L, _L, _I, _I, _I, _I, _F, _P]),
    "babe_axpby2_4d": (_I, [_P, _L, _L, _P, _L, _L, _P, _L, _L, _I, _I, _I, _I, _F, _F, _P]),
    "babe_linear": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "babe_rff": (_I, [_P, _P, _P, _I, _I, _P]),
    "babe_rfft_mixed": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _I, _P, _P, _P, _I, _P]),
    "babe_fft_twiddle_transpose": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "babe_cqt_band_analysis": (_I, [C.POINTER(CqtBands), _P, _P, _I, _P]),
    "babe_cqt_band_synthesis": (_I, [C.POINTER(CqtBands), _P, _P, _L, _I, _P]),
    "babe_cqt_gather": (_I, [_P, _L, _P, _P, _P, _P, _I, _I, _F, _P, _I, _P]),
    "babe_spec_scale": (_I, [_P, _P, _P, _P, _I, _I, _F, _F, _I, _P]),
    "babe_cqt_design_create": (_P, [_D, _I, _I, _I, _D]),
    "babe_cqt_design_create_ex": (_P, [_D, _I, _I, _I, _D, _I]),
    "babe_cqt_design_destroy": (None, [_P]),
    "babe_cqt_design_get": (_L, [_P, _S, _P, _L]),
    "babe_cqt_plan_create": (_P, [_D, _I, _I, _I, _D]),
    "babe_cqt_plan_create_ex": (_P, [_D, _I, _I, _I, _D, _I]),
    "babe_cqt_plan_destroy": (None, [_P]),
    "babe_cqt_workspace_bytes": (_L, [_P, _I]),
    "babe_cqt_fwd": (_I, [_P, _P, _P, _P, _I, _P]),
    "babe_cqt_bwd": (_I, [_P, _P, _P, _P, _I, _P]),
    "babe_cqt_fwd_adjoint": (_I, [_P, _P, _P, _P, _I, _P]),
    "babe_cqt_bwd_adjoint": (_I, [_P, _P, _P, _P, _I, _P]),
    "babe_cqt_hpf": (_I, [_P, _P, _P, _P, _I, _P]),
    "babe_stft_fwd": (_I, [_P, _L, _I, _P, _P, _I, _I, _I, _P, _P]),
    "babe_spec_filter_istft": (_I, [_P, _P, _L, _P, _I, _I, _I, _P, _P]),
    "babe_ola": (_I, [_P, _P, _P, _L, _P, _L, _P, _I, _I, _I, _I, _I, _P]),
    "babe_residual_seed": (_I, [_P, _L, _P, _I, _P, _P, _L, _I, _I, _P]),
    "babe_stft_mag_stats": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "babe_design_filter": (_I, [_P, _P, _I, _I, _I, _F, _I, _P]),
    "babe_filter_fit": (_I, [_P, _P, _P, _I, _I, _I, _F, _I, C.POINTER(FitCfg), _P]),
    "babe_filter_loss_grad": (_I, [_P, _L, _P, _P, _I, _I, _I, _F, _I, C.POINTER(FitCfg), _P]),
    "babe_fir_same": (_I, [_P, _L, _P, _I, _P, _L, _I, _I, _I, _P]),
    "babe_fir_sqerr_fwd": (_I, [_P, _L, _P, _L, _P, _I, _P, _P, _I, _I, _P]),
    "babe_fir_sqerr_bwd": (_I, [_P, _L, _P, _P, _I, _P, _I, _I, _P]),
    "babe_plane_bin_energy": (_I, [_P, _P, _I, _I, _I, _P]),
    "babe_lsd_num_frames": (_L, [_I, _I, _I]),
    "babe_lsd_frames": (_I, [_P, _L, _P, _L, _I, _I, _I, _I, _I, _I, _F, _P, _P, _P]),
    "babe_lincomb3": (_I, [_P, _F, _P, _F, _P, _F, _P, _L, _P]),
    "babe_add_obs_noise": (_I, [_P, _L, _P, _L, _F, _I, _L, _P]),
    "babe_mask_blend": (_I, [_P, _P, _L, _P, _P, _I, _L, _P]),
    "babe_sumsq_partial": (_I, [_P, _L, _P, _I, _I, _L, _P]),
    "babe_stft_dist_partial": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "babe_stft_dist_grad": (_I, [_P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "babe_cos_partial": (_I, [_P, _L, _P, _L, _P, _I, _I, _L, _P]),
    "babe_residual_seed_alt": (_I, [_P, _L, _P, _L, _P, _I, _P, _P, _L, _I, _I, _I, _F, _P]),
    "babe_score_direction": (_I, [_P, _P, _P, _P, _I, _P, _F, _F, _F, _I, _I, _I, _L, _P]),
    "babe_eval_workspace_bytes": (_L, [C.POINTER(EvalDesc), _I]),
    "babe_score_eval": (_I, [C.POINTER(EvalDesc), _P, _F, _F, _F, _F, _F, _P, _P, _P, _P, _P, _P, _P, _L, _I, _P]),
    "babe_philox4x32": (_I, [_P, _P, _P]),
    "babe_randn": (_I, [_P, _L, _I, _L, _L, _L, _L, _P]),
    "babe_rand_bits": (_I, [_P, _L, _I, _L, _L, _L, _L, _P]),
    "babe_sample_workspace_bytes": (_L, [C.POINTER(SampleDesc), _I]),
    "babe_sample_bwe": (_I, [C.POINTER(SampleDesc), _P, _P, _P, _P, _L, _L, _P, _P, _P, _L, _I, _P]),
    "babe_edm_steps": (_I, [C.POINTER(SampleStep), _P, _I, _I, _D, _D, _D, _D, _D, _D, _D, _D, _D]),
    "babe_firwin_kaiser": (_I, [_I, _D, _D, _D, _I, _P]),
    "babe_iir_check": (_I, [_P, _P, _I]),
    "babe_recording_plan": (_L, [_L, _L, _L, _L, _P, _P, _L]),
    "babe_recording_workspace_bytes": (_L, [C.POINTER(RecordingDesc)]),
    "babe_restore_recording": (_I, [C.POINTER(RecordingDesc), _P, _L, _P, _P, _P, _L, _L, _P, _L, _P]),
    "babe_row_std": (_I, [_P, _L, _I, _L, _P, _P, _P]),
    "babe_segment_cut": (_I, [_P, _L, _P, _L, _P]),
    "babe_scale_dev": (_I, [_P, _P, _L, _F, _P, _I, _P]),
    "babe_edge_masks": (_I, [_P, _P, _L, _L, _I, _P, _P]),
    "babe_dn_conv2d": (_I, [C.POINTER(DnConvArgs), _P, _P]),
    "babe_dn_pack_weights": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "babe_dn_packed_size": (_L, [_I, _I, _I, _I]),
    "babe_dn_upsample_add": (_I, [_P, _L, _L, _P, _L, _L, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "babe_dn_sam_gate": (_I, [_P, _P, _P, _L, _L, _P, _L, _L, _I, _I, _L, _P]),
    "babe_dn_fill_input": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "babe_dn_stft": (_I, [_P, _L, _I, _P, _I, _I, _I, _I, _P, _P]),
    "babe_dn_istft": (_I, [_P, _P, _P, _L, _I, _I, _I, _I, _I, _P, _P]),
    "babe_attn_buckets": (_I, [_P, _I, _I, _I]),
    "babe_attn_bucket_thresholds": (_I, [C.POINTER(AttnBucketThr), _I, _I]),
    "babe_attn_bucket_table": (_I, [C.POINTER(AttnBucketThr), _I, _P, _P]),
    "babe_attn_fwd": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _F, _P]),
    "babe_attn_vjp": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P]),
    "babe_attn_fwd_bf16": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _F, _P]),
    "babe_attn_vjp_bf16": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P]),
    "babe_conv_wgrad_workspace": (_L, [C.POINTER(WgradArgs)]),
    "babe_conv_wgrad_rows": (_I, [C.POINTER(WgradArgs), _P, _P, _F, _P, _P, _L, _F, _P, _L, _P]),
    "babe_conv_wgrad_bf16_workspace": (_L, [C.POINTER(WgradArgs)]),
    "babe_conv_wgrad_bf16_rows": (_I, [C.POINTER(WgradArgs), _P, _P, _F, _P, _P, _L, _F, _P, _L, _P]),
    "babe_rows_sum": (_I, [_P, _L, _I, _L, _P, _F, _P]),
    "babe_gn_param_grad": (_I, [_P, _P, _P, _P, _P, _P, _L, _F, _P, _L, _P, _L, _I, _I, _I, _L, _P]),
    "babe_linear_bwd_workspace": (_L, [_I, _I, _I]),
    "babe_linear_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _P]),
    "babe_fenc_bias": (_I, [_P, _P, _P, _I, _I, _P]),
    "babe_fenc_wgrad_rows": (_I, [_P, _L, _L, _P, _F, _P, _L, _I, _I, _I, _I, _I, _P]),
    "babe_attn_qk_wgrad_workspace": (_L, [_I, _I, _I]),
    "babe_attn_qk_wgrad": (_I, [_P, _P, _P, _P, _I, _I, _I, _F, _F, _P]),
    "babe_attn_param_vjp_workspace": (_L, [_I, _I, _I, _I]),
    "babe_attn_param_vjp": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _L, _P, _L, _I, _I, _I, _I, _F, _P]),
    "babe_attn_qk_wgrad_bf16_workspace": (_L, [_I, _I, _I]),
    "babe_attn_qk_wgrad_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _F, _F, _P]),
    "babe_attn_param_vjp_bf16_workspace": (_L, [_I, _I, _I, _I]),
    "babe_attn_param_vjp_bf16": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _L, _P, _L, _I, _I, _I, _I, _F, _P]),
    "babe_gn_param_grad_nogelu": (_I, [_P, _P, _P, _P, _P, _L, _F, _P, _L, _P, _L, _I, _I, _I, _L, _P]),
    "babe_scale_channels": (_I, [_P, _P, _P, _I, _I, _L, _P]),
    "babe_model_load": (_P, [_S, _P]),
    "babe_model_create": (_P, [C.POINTER(ModelEntry), _I, C.POINTER(ModelKV), _I, _P]),
    "babe_model_load_ex": (_P, [_S, _I, _P]),
    "babe_model_create_ex": (_P, [C.POINTER(ModelEntry), _I, C.POINTER(ModelKV), _I, _I, _P]),
    "babe_model_load_opt": (_P, [_S, C.POINTER(ModelOptions), _P]),
    "babe_model_create_opt": (_P, [C.POINTER(ModelEntry), _I, C.POINTER(ModelKV), _I, C.POINTER(ModelOptions), _P]),
    "babe_model_precision": (_I, [_P]),
    "babe_model_attention": (_I, [_P]),
    "babe_model_destroy": (None, [_P]),
    "babe_model_info": (_I, [_P, C.POINTER(ModelSummary)]),
    "babe_model_setting": (_I, [_P, _S, C.POINTER(_D)]),
    "babe_model_unet_plan": (_P, [_P]),
    "babe_model_cqt_plan": (_P, [_P]),
    "babe_model_eval_desc": (_I, [_P, _P, C.POINTER(EvalDesc)]),
    "babe_resample_sinc_table_size": (_L, [_L, _L, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "babe_resample_sinc_table": (_I, [_L, _L, _P, _P]),
    "babe_resampled_length": (_L, [_L, _L, _L]),
    "babe_denoiser_load": (_P, [_S, _P]),
    "babe_denoiser_create": (_P, [C.POINTER(ModelEntry), _I, C.POINTER(ModelKV), _I, _P]),
    "babe_denoiser_destroy": (None, [_P]),
    "babe_denoiser_info": (_I, [_P, C.POINTER(DenoiserSummary)]),
    "babe_dn_ksplit": (_I, [C.POINTER(DnConvArgs)]),
    "babe_denoiser_workspace_bytes": (_L, [_P, _I, _I, _I]),
    "babe_denoiser_fwd": (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _I, _P]),
    "babe_denoise_signal_plan": (_L, [_L, _L, _L, _P, _L]),
    "babe_denoise_signal_workspace_bytes": (_L, [_P, _I, _L]),
    "babe_denoise_signal": (_I, [_P, _P, _L, _P, _L, _I, _L, _P, _L, _P]),
    "babe_dn_segment_pad": (_I, [_P, _L, _L, _P, _L, _L, _I, _P]),
    "babe_dn_fade_add": (_I, [_P, _L, _P, _L, _I, _L, _L, _P, _I, _I, _I, _P]),
    "babe_restore_file_plan": (_I, [_L, _L, _L, _L, _P]),
    "babe_restore_file_workspace_bytes": (_L, [C.POINTER(FileDesc)]),
    "babe_restore_file": (_I, [C.POINTER(FileDesc), _P, _L, _P, _P, _P, _P, _L, _L, _P, _L, _P]),
    "babe_opt_chunks": (_L, [_P, _L, _L, _P, _L]),
    "babe_grad_sqnorm": (_I, [_P, _P, _L, _P, _P, _P]),
    "babe_adam_ema_step": (_I, [_P, _P, _L, _P, _D, _D, _D, _D, _D, _D, _D, _D, _P]),
}


class _Bound:
    """The declared entry points as plain attributes (the ctypes function objects themselves: a call costs what it costs on a
    CDLL); any other babe_* name is an error instead of a call with guessed argument types."""

    def __init__(self, cdll):
        for name, (restype, argtypes) in SIGS.items():
            fn = getattr(cdll, name)
            fn.restype, fn.argtypes = restype, argtypes
            setattr(self, name, fn)

    def __getattr__(self, name):                        # reached only for names that are not attributes: undeclared ones
        raise AttributeError(f"{name} is not declared in babe_amd/_cabi.py::SIGS: add its signature there "
                             "(an undeclared function would be called with 32-bit pointer arguments)")


def bind(path):
    """Load the library at `path` and declare every entry point of SIGS."""
    return _Bound(C.CDLL(path))
