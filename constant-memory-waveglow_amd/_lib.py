"""ctypes binding of csrc/libwgflow.so (the C ABI declared in include/wgflow.h).

There is NO fallback: if the shared library is missing or a tensor is not on a HIP device the call
raises.  Build with `python -c "import __graft_entry__ as g; g.build()"` (or `python build.py`).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WGFLOW_LIB") or os.path.join(_HERE, "csrc", "libwgflow.so")   # WGFLOW_LIB: developer A/B builds
_LIB = None

ABI_VERSION = 10         # include/wgflow.h WG_ABI_VERSION (10: the BatchNorm statistics of wg_mg_bn_* in double)
ABI_SYMBOLS = [
    "wg_strerror", "wg_abi_version", "wg_param_count", "wg_packed_bytes", "wg_workspace_bytes",
    "wg_wn_param_count", "wg_wn_packed_bytes", "wg_coupling_workspace_bytes", "wg_invconv_workspace_bytes",
    "wg_workspace_init", "wg_pack_weights", "wg_wn_pack_weights", "wg_forward", "wg_inverse", "wg_backward",
    "wg_nll_loss", "wg_nll_loss_backward", "wg_invconv_apply", "wg_invconv_backward", "wg_coupling_apply",
    "wg_coupling_backward", "wg_upsample", "wg_wn_apply", "wg_wsr_cond", "wg_wsr_cond_backward", "wg_adam_step",
    "wg_wf_param_count", "wg_wf_packed_bytes", "wg_wf_workspace_bytes", "wg_wf_tape_bytes", "wg_wf_pack_weights", "wg_wf_upsample", "wg_wf_forward",
    "wg_wf_inverse", "wg_wf_backward", "wg_melspec_frames", "wg_melspec", "wg_lowpass_workspace_bytes", "wg_lowpass", "wg_train_step",
    "wg_nll_scratch_floats", "wg_train_scratch_floats",
    "wg_timer_create", "wg_timer_attach", "wg_timer_count", "wg_timer_read", "wg_timer_read_info", "wg_timer_destroy", "wg_stat_wgrad16t_launches",
    "wg_stat_layer_launches", "wg_layer_workspace_bytes", "wg_layer_apply", "wg_wf_wn_apply",
    "wg_timer_read_name", "wg_box_probe_bytes", "wg_box_probe", "wg_stat_layerg_launches", "wg_stat_gate_split_launches",
    "wg_wf_wn_backward", "wg_layer_backward_workspace_bytes", "wg_layer_backward", "wg_affine_apply", "wg_affine_backward",
    "wg_reload_env", "wg_stat_gate_part_launches", "wg_wsr_cond_pre",
    "wg_mg_gemm_workspace_bytes", "wg_mg_gemm", "wg_mg_bn_stats", "wg_mg_bn_update", "wg_mg_bn_tanh", "wg_mg_bn_tanh_backward", "wg_mg_weight_norm",
    "wg_mg_weight_norm_backward", "wg_lvc_check", "wg_lvc_forward", "wg_lvc_backward_data", "wg_lvc_backward_weight", "wg_lvc_gate_backward",
    "wg_mr_haar_split", "wg_mr_haar_merge", "wg_mr_upsample", "wg_mr_upsample_backward", "wg_mr_pack", "wg_mr_unpack",
    "wg_mg_check", "wg_mg_param_count", "wg_mg_packed_bytes", "wg_mg_workspace_bytes", "wg_mg_pack_weights", "wg_mg_forward", "wg_mg_inverse",
    "wg_stat_mg_pass_calls", "wg_stat_mg_layer_launches", "wg_mg_layer_apply", "wg_mg_predictor_apply",
    "wg_mr_check", "wg_mr_param_count", "wg_mr_packed_bytes", "wg_mr_workspace_bytes", "wg_mr_pack_weights", "wg_mr_forward", "wg_mr_inverse",
    "wg_stat_mr_pass_calls", "wg_mr_plane_geo", "wg_mr_plane_split", "wg_mr_plane_merge", "wg_mr_plane_upsample",
]
K_CONV_STORE, K_CONV_GATE, K_CONV_RESSKIP, K_CONV_DGATE, K_WGRAD, K_LAYER, K_THIN = range(7)


class WgConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_flows", "n_group", "n_early_every", "n_early_size", "n_mels",
        "up_stride", "up_kernel", "up_pad", "res_ch", "dil_ch", "skip_ch", "depth", "radix", "precision", "reverse_mode", "keep_activations",
        "bias")]


class WgWfConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("flows", "n_group", "n_mels", "res_ch", "dil_ch", "skip_ch", "precision", "use_conv1x1", "bias")]


class WgWnDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("in_ch", "aux_ch", "res_ch", "dil_ch", "skip_ch", "depth", "radix", "precision", "bias")]


class WgLayerDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("res_ch", "dil_ch", "skip_ch", "radix", "dilation", "last_layer", "h_dilation", "rows")]


class WgMgGemmDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("M", "N", "K", "batch", "N1", "K1")] + \
               [(n, C.c_int64) for n in ("a_m", "a_k", "a_k2", "a_b", "b_k", "b_k2", "b_n", "b_n2", "b_b", "c_m", "c_n", "c_n2", "c_b")] + \
               [("alpha", C.c_float), ("beta", C.c_float)]


class WgLvcDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("res_ch", "dil_ch", "radix", "dilation")]


class WgMgConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("flows", "n_group", "n_early_every", "n_early_size", "hop", "n_mels", "depth", "res_ch", "dil_ch",
                                         "skip_ch", "radix", "pred_ch", "pred_layers", "reverse_mode")]


class WgMrConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("prior_flows", "flows", "levels", "n_group", "hop_size", "n_mels", "super_resolution", "reverse_mode",
                                         "dilation_channels", "residual_channels", "skip_channels", "depth", "radix", "bias", "precision")]


PREC_F32, PREC_BF16X3, PREC_BF16X3_PLANES = 0, 1, 2


def default_precision():
    """WG_PRECISION=f32|bf16x3|bf16x3p selects the arithmetic of the MFMA contractions (include/wgflow.h, WG_PREC_*)."""
    v = os.environ.get("WG_PRECISION", "bf16x3p").lower()
    if v in ("f32", "fp32", "0"):
        return PREC_F32
    if v in ("bf16x3", "1"):
        return PREC_BF16X3
    if v in ("bf16x3p", "bf16x3_planes", "2"):
        return PREC_BF16X3_PLANES
    raise WgError("WG_PRECISION must be f32 or bf16x3 (got %r)" % v)


class WgError(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise WgError("HIP extension %s is missing -- build it first (python build.py); "
                      "this package has no CPU or eager fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, sz, i, f = C.c_void_p, C.c_size_t, C.c_int, C.c_float
    cfgp, wnp = C.POINTER(WgConfig), C.POINTER(WgWnDims)
    L.wg_strerror.restype = C.c_char_p
    L.wg_strerror.argtypes = [i]
    L.wg_abi_version.restype = i
    if L.wg_abi_version() != ABI_VERSION:
        raise WgError("%s implements ABI revision %d, this package binds revision %d (include/wgflow.h WG_ABI_VERSION): rebuild it"
                      % (LIB_PATH, L.wg_abi_version(), ABI_VERSION))
    L.wg_param_count.argtypes = [cfgp]
    L.wg_packed_bytes.restype = sz
    L.wg_packed_bytes.argtypes = [cfgp]
    L.wg_workspace_bytes.restype = sz
    L.wg_workspace_bytes.argtypes = [cfgp, i, i, i]
    L.wg_wn_param_count.argtypes = [wnp]
    L.wg_wn_packed_bytes.restype = sz
    L.wg_wn_packed_bytes.argtypes = [wnp]
    L.wg_coupling_workspace_bytes.restype = sz
    L.wg_coupling_workspace_bytes.argtypes = [wnp, i, i, i]
    L.wg_invconv_workspace_bytes.restype = sz
    L.wg_invconv_workspace_bytes.argtypes = [i, i, i]
    L.wg_workspace_init.argtypes = [vp, sz, vp]
    L.wg_pack_weights.argtypes = [cfgp, vp, vp, vp]
    L.wg_wn_pack_weights.argtypes = [wnp, vp, vp, vp]
    L.wg_forward.argtypes = [cfgp, vp, vp, vp, i, i, i, vp, vp, vp, sz, vp]
    L.wg_inverse.argtypes = [cfgp, vp, vp, vp, i, i, i, vp, vp, vp, sz, vp]
    L.wg_backward.argtypes = [cfgp, vp, vp, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, vp, sz, vp, vp]
    L.wg_nll_scratch_floats.restype = sz
    L.wg_nll_scratch_floats.argtypes = [i]
    L.wg_train_scratch_floats.restype = sz
    L.wg_train_scratch_floats.argtypes = [i, i]
    L.wg_nll_loss.argtypes = [vp, vp, i, i, f, i, vp, vp, vp, vp]
    L.wg_nll_loss_backward.argtypes = [vp, i, i, f, i, vp, vp, vp, vp]
    L.wg_invconv_apply.argtypes = [vp, i, vp, i, i, i, vp, vp, vp, sz, vp]
    L.wg_invconv_backward.argtypes = [vp, i, vp, vp, vp, i, i, i, vp, vp, vp, vp, sz, vp]
    L.wg_coupling_apply.argtypes = [wnp, vp, vp, vp, i, i, i, vp, vp, vp, sz, vp]
    L.wg_coupling_backward.argtypes = [wnp, vp, vp, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, vp, sz, vp]
    L.wg_upsample.argtypes = [cfgp, vp, vp, i, i, i, vp, vp]
    L.wg_wn_apply.argtypes = [wnp, vp, vp, vp, i, i, vp, vp, vp, sz, vp]
    L.wg_wsr_cond.argtypes = [vp, i, i, vp, vp, vp, vp]
    L.wg_wsr_cond_backward.argtypes = [vp, i, i, vp, vp, vp, vp]
    L.wg_wsr_cond_pre.argtypes = [vp, i, i, vp, vp, vp]
    L.wg_adam_step.argtypes = [vp, vp, vp, vp, sz, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, i, vp]
    wfp = C.POINTER(WgWfConfig)
    L.wg_wf_param_count.argtypes = [wfp]
    L.wg_wf_packed_bytes.restype = sz
    L.wg_wf_packed_bytes.argtypes = [wfp]
    L.wg_wf_workspace_bytes.restype = sz
    L.wg_wf_workspace_bytes.argtypes = [wfp, i, i, i]
    L.wg_wf_tape_bytes.restype = sz
    L.wg_wf_tape_bytes.argtypes = [wfp, i, i]
    L.wg_wf_pack_weights.argtypes = [wfp, vp, vp, vp]
    L.wg_wf_upsample.argtypes = [wfp, vp, vp, vp, i, i, i, vp, vp]
    L.wg_wf_forward.argtypes = [wfp, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, sz, vp]
    L.wg_wf_inverse.argtypes = [wfp, vp, vp, vp, vp, i, i, i, vp, vp, vp, sz, vp]
    L.wg_wf_wn_apply.argtypes = [wfp, vp, vp, vp, vp, i, i, i, vp, vp, vp, sz, vp]
    L.wg_wf_wn_backward.argtypes = [wfp, vp, vp, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, sz, vp]
    L.wg_wf_backward.argtypes = [wfp, vp, vp, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, sz, vp]
    L.wg_melspec_frames.argtypes = [i, i, i]
    L.wg_melspec.argtypes = [vp, i, i, i, i, i, C.c_double, C.c_double, i, vp, vp, vp]
    L.wg_lowpass_workspace_bytes.restype = sz
    L.wg_lowpass_workspace_bytes.argtypes = [i, i, i, i]
    L.wg_lowpass.argtypes = [vp, i, i, i, i, i, i, vp, vp, sz, vp]
    L.wg_train_step.argtypes = [cfgp, vp, vp, vp, vp, i, i, i, f, i, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp]
    L.wg_timer_create.restype = vp
    L.wg_timer_create.argtypes = [i, i]
    L.wg_timer_attach.argtypes = [vp]
    L.wg_timer_attach.restype = None
    L.wg_timer_count.argtypes = [vp]
    L.wg_timer_read.argtypes = [vp, vp, i]
    L.wg_timer_read_info.argtypes = [vp, vp, i]
    L.wg_stat_wgrad16t_launches.restype = C.c_longlong
    L.wg_stat_wgrad16t_launches.argtypes = []
    L.wg_stat_layer_launches.restype = C.c_longlong
    L.wg_stat_layer_launches.argtypes = []
    L.wg_layer_workspace_bytes.restype = sz
    L.wg_layer_workspace_bytes.argtypes = [C.POINTER(WgLayerDims), i, i]
    L.wg_layer_apply.argtypes = [C.POINTER(WgLayerDims), vp, vp, vp, i, i, vp, vp, vp, sz, vp]
    L.wg_layer_backward_workspace_bytes.restype = C.c_size_t
    L.wg_layer_backward_workspace_bytes.argtypes = [C.POINTER(WgLayerDims), i, i]
    L.wg_layer_backward.argtypes = [C.POINTER(WgLayerDims), vp, vp, vp, vp, vp, i, i, vp, vp, vp, vp, sz, vp]
    L.wg_affine_apply.argtypes = [vp, vp, vp, sz, i, vp, vp]
    L.wg_affine_backward.argtypes = [vp, vp, vp, vp, vp, sz, i, vp, vp, vp, vp, vp]
    L.wg_timer_destroy.argtypes = [vp]
    L.wg_timer_destroy.restype = None
    L.wg_timer_read_name.argtypes = [vp, i, C.c_char_p, i]
    L.wg_box_probe_bytes.restype = C.c_size_t
    L.wg_box_probe_bytes.argtypes = []
    L.wg_box_probe.argtypes = [vp, i, vp, vp]
    L.wg_stat_layerg_launches.restype = C.c_longlong
    L.wg_stat_gate_split_launches.restype = C.c_longlong
    L.wg_stat_gate_part_launches.restype = C.c_longlong
    L.wg_reload_env.restype = None
    L.wg_reload_env.argtypes = []
    L.wg_mg_gemm_workspace_bytes.restype = sz
    L.wg_mg_gemm_workspace_bytes.argtypes = [C.POINTER(WgMgGemmDesc)]
    L.wg_mg_gemm.argtypes = [C.POINTER(WgMgGemmDesc), vp, vp, vp, vp, vp, sz, vp]
    L.wg_mg_bn_stats.argtypes = [vp, i, i, f, i, vp, vp, vp, vp, vp, vp]
    L.wg_mg_bn_update.argtypes = [vp, vp, vp, vp, vp, i, f, vp]
    L.wg_mg_bn_tanh.argtypes = [vp, i, i, vp, vp, vp, vp, vp, vp, vp, vp]
    L.wg_mg_bn_tanh_backward.argtypes = [vp, vp, vp, i, i, vp, vp, vp, i, vp, vp, vp, vp]
    L.wg_mg_weight_norm.argtypes = [vp, vp, i, i, vp, vp]
    L.wg_mg_weight_norm_backward.argtypes = [vp, vp, vp, i, i, vp, vp, vp]
    lvcp = C.POINTER(WgLvcDims)
    L.wg_lvc_check.argtypes = [lvcp, i, i, i]
    L.wg_lvc_forward.argtypes = [lvcp, vp, vp, i, i, i, vp, vp, vp]
    L.wg_lvc_backward_data.argtypes = [lvcp, vp, vp, vp, i, i, i, vp, vp]
    L.wg_lvc_backward_weight.argtypes = [lvcp, vp, vp, i, i, i, vp, vp]
    L.wg_lvc_gate_backward.argtypes = [vp, vp, i, i, i, vp, vp]
    i64 = C.c_int64
    L.wg_mr_haar_split.argtypes = [vp, i64, i64, i64, i, i, i, i, vp, vp, vp, i, vp]
    L.wg_mr_haar_merge.argtypes = [vp, vp, i, vp, i, i, i, i, vp, i64, i64, i64, vp]
    L.wg_mr_upsample.argtypes = [vp, vp, i, i, i, i, i, vp, i, i, vp]
    L.wg_mr_upsample_backward.argtypes = [vp, i, i, i, i, i, i, i, vp, vp]
    L.wg_mr_pack.argtypes = [vp, i, i, i, i, i, vp, vp]
    L.wg_mr_unpack.argtypes = [vp, i, i, i, i, i, vp, vp]
    mgp = C.POINTER(WgMgConfig)
    L.wg_mg_check.argtypes = [mgp, i, i, i]
    L.wg_mg_param_count.argtypes = [mgp]
    L.wg_mg_packed_bytes.restype = sz
    L.wg_mg_packed_bytes.argtypes = [mgp]
    L.wg_mg_workspace_bytes.restype = sz
    L.wg_mg_workspace_bytes.argtypes = [mgp, i, i]
    L.wg_mg_pack_weights.argtypes = [mgp, vp, vp, vp, vp]
    L.wg_mg_forward.argtypes = [mgp, vp, vp, vp, i, i, i, vp, vp, vp, sz, vp]
    L.wg_mg_inverse.argtypes = [mgp, vp, vp, vp, i, i, i, vp, vp, vp, sz, vp]
    L.wg_stat_mg_pass_calls.restype = C.c_longlong
    L.wg_stat_mg_pass_calls.argtypes = []
    L.wg_stat_mg_layer_launches.restype = C.c_longlong
    L.wg_stat_mg_layer_launches.argtypes = []
    L.wg_mg_layer_apply.argtypes = [lvcp, i, i, i, vp, vp, vp, i, i, i, vp, vp, vp]
    L.wg_mg_predictor_apply.argtypes = [mgp, vp, i, vp, i, i, i, vp, vp, sz, vp]
    mrp, ip = C.POINTER(WgMrConfig), C.POINTER(C.c_int)
    L.wg_mr_check.argtypes = [mrp, i, i, i]
    L.wg_mr_param_count.argtypes = [mrp]
    L.wg_mr_packed_bytes.restype = sz
    L.wg_mr_packed_bytes.argtypes = [mrp]
    L.wg_mr_workspace_bytes.restype = sz
    L.wg_mr_workspace_bytes.argtypes = [mrp, i, i]
    L.wg_mr_pack_weights.argtypes = [mrp, vp, vp, vp]
    L.wg_mr_forward.argtypes = [mrp, vp, vp, vp, i, i, i, vp, vp, vp, sz, vp]
    L.wg_mr_inverse.argtypes = [mrp, vp, vp, vp, i, i, i, vp, vp, vp, sz, vp]
    L.wg_stat_mr_pass_calls.restype = C.c_longlong
    L.wg_stat_mr_pass_calls.argtypes = []
    L.wg_mr_plane_geo.argtypes = [i, i, ip, ip]
    L.wg_mr_plane_split.argtypes = [vp, vp, i, i, i, i, i, vp, i, i, vp, i, vp, i, i, vp]
    L.wg_mr_plane_merge.argtypes = [vp, i, vp, i, i, i, i, i, i, vp, i, vp, vp]
    L.wg_mr_plane_upsample.argtypes = [vp, i, i, i, i, i, i, i, vp, ip, ip, vp]
    _LIB = L
    return L


def check(rc, what):
    if rc != 0:
        raise WgError("%s failed: %s (code %d)" % (what, lib().wg_strerror(rc).decode(), rc))
