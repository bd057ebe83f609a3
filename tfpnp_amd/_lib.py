"""ctypes binding of libpnpx.so (the C ABI declared in include/pnpx.h).

There is NO CPU or PyTorch fallback anywhere in this package: if the HIP library is missing or a call
fails, a RuntimeError is raised.
"""
import ctypes as C
import os
import threading

import torch  # noqa: F401  -- must come first: libpnpx.so has to bind to the HIP runtime PyTorch already loaded

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PNPX_LIB", os.path.join(_HERE, "libpnpx.so"))   # PNPX_LIB: A/B builds of the same ABI

_lib = None
_lock = threading.Lock()

c_float_p = C.POINTER(C.c_float)
c_void_p = C.c_void_p


class PnpxError(RuntimeError):
    pass


PNPX_ERR_RANGE = 6      # include/pnpx.h: half-split range guard tripped (pnpx_ctx_status)


class ConvHsProbeDesc(C.Structure):
    """include/pnpx.h: pnpx_conv_hs_probe_desc (field for field)."""
    _fields_ = ([(n, c_void_p) for n in ("w", "bias", "outc_w", "outc_b", "first_w", "first_b", "in0", "in1", "res", "dmask", "out", "pool_out",
                                         "x_in", "first_x", "first_sigma", "out_img", "out_pre")] +
                [(n, C.c_int) for n in ("cin", "cout", "G0", "G1", "B", "H", "W")] + [("slope", C.c_float)] +
                [(n, C.c_int) for n in ("taps", "in0_groups", "wreg", "share", "ups_h", "ups_w", "critic_epi")] + [("alpha", C.c_float)] +
                [("res_groups", C.c_int), ("first_sigma_stride", C.c_int), ("first_slope", C.c_float), ("want_range_flag", C.c_int),
                 ("range_flag_out", C.POINTER(C.c_uint))])
PNPX_CONV_HS_PLAN_INTS = 12


class VjpGlueProbeDesc(C.Structure):
    """include/pnpx.h: pnpx_vjp_glue_probe_desc (field for field)."""
    _fields_ = ([(n, C.c_int) for n in ("op", "family", "form", "B", "C", "H", "W", "Ccat", "c_off", "Ht", "Wt")] +
                [(n, c_void_p) for n in ("g", "act", "g_pool", "pre", "w", "g_res", "sc", "out", "out_res", "part", "gsigma", "bits")])


class FwdGlueProbeDesc(C.Structure):
    """include/pnpx.h: pnpx_fwd_glue_probe_desc (field for field)."""
    _fields_ = ([(n, C.c_int) for n in ("op", "family", "form", "B", "C", "H", "W", "Ht", "Wt", "sigma_stride", "k")] + [("slope", C.c_float)] +
                [(n, c_void_p) for n in ("src", "src2", "x", "sigma", "pre", "sc", "w", "bias", "out", "out_pre", "part", "gsigma")])


class NetTrainProbeDesc(C.Structure):
    """include/pnpx.h: pnpx_net_train_probe_desc (field for field)."""
    _fields_ = ([(n, C.c_int) for n in ("op", "B", "G", "h", "w", "cout", "K", "cin", "Cp", "kind", "Gg", "Xg", "resG", "mG", "n_det", "spi", "update")] +
                [(n, C.c_float) for n in ("momentum", "thr", "boost", "inv_w", "inv_b")] +
                [(n, c_void_p) for n in ("z0", "z1", "g", "act", "res", "x", "m", "st0", "st1", "gv", "slot", "fin", "fin2", "params", "din", "din2",
                                         "alpha_src", "out", "out2", "dy_out", "grad", "coef", "fout", "fout2", "dout", "flag")])


class RadonGeom(C.Structure):
    """include/pnpx.h: pnpx_radon_geom (field for field)."""
    _fields_ = [("kind", C.c_int), ("n_view", C.c_int), ("det_count", C.c_int), ("source_distance", C.c_float),
                ("det_distance", C.c_float), ("det_spacing", C.c_float)]
PNPX_GEOM_PARALLEL, PNPX_GEOM_FAN = 0, 1
PNPX_FAN_W_ADJOINT, PNPX_FAN_W_FBP = 0, 1


# name -> (restype, argtypes); mirrors include/pnpx.h one to one
_P = c_void_p  # device pointers travel as integers
_SIGNATURES = {
    "pnpx_version": (C.c_char_p, []),
    "pnpx_last_error": (C.c_char_p, []),
    "pnpx_ctx_create": (C.c_int, [C.c_int, C.POINTER(c_void_p)]),
    "pnpx_ctx_destroy": (C.c_int, [c_void_p]),
    "pnpx_ctx_reserve": (C.c_int, [c_void_p, C.c_int, C.c_int, C.c_int]),
    "pnpx_ctx_set_option": (C.c_int, [c_void_p, C.c_char_p, C.c_int]),
    "pnpx_ctx_get_option": (C.c_int, [c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    "pnpx_ctx_status": (C.c_int, [c_void_p]),
    "pnpx_ctx_bytes": (C.c_size_t, [c_void_p]),
    "pnpx_unet_num_params": (C.c_size_t, []),
    "pnpx_unet_load": (C.c_int, [c_void_p, c_void_p, C.c_size_t]),
    "pnpx_drunet_num_params": (C.c_size_t, [C.c_int]),
    "pnpx_drunet_load": (C.c_int, [c_void_p, c_void_p, C.c_size_t, C.c_int]),
    "pnpx_unet_denoise": (C.c_int, [c_void_p, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_unet_denoise_backward": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_unet_denoise_train": (C.c_int, [c_void_p, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_unet_denoise_backward_ticket": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int,
                                                    C.c_ulonglong, c_void_p]),
    "pnpx_policy_num_params": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "pnpx_policy_load": (C.c_int, [c_void_p, c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int]),
    "pnpx_policy_load_device": (C.c_int, [c_void_p, _P, C.c_size_t, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_policy_params": (C.c_int, [c_void_p, _P, C.c_size_t, c_void_p]),
    "pnpx_policy_forward": (C.c_int, [c_void_p, _P, _P, _P, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_policy_forward_train": (C.c_int, [c_void_p, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, c_void_p]),
    "pnpx_policy_num_bn_channels": (C.c_size_t, []),
    "pnpx_policy_bn_stats": (C.c_int, [c_void_p, _P, _P, C.c_size_t, c_void_p]),
    "pnpx_policy_param_grad": (C.c_int, [c_void_p, _P, _P, _P, _P, C.c_size_t, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_policy_forward_train_keep": (C.c_int, [c_void_p, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, c_void_p]),
    "pnpx_policy_param_grad_kept": (C.c_int, [c_void_p, _P, _P, _P, C.c_size_t, c_void_p]),
    "pnpx_policy_adam_step": (C.c_int, [c_void_p, _P, C.c_size_t] + [C.c_float] * 5 + [_P, c_void_p]),
    "pnpx_policy_optim_state": (C.c_int, [c_void_p, _P, _P, C.c_size_t, C.POINTER(C.c_longlong), c_void_p]),
    "pnpx_policy_optim_reset": (C.c_int, [c_void_p]),
    "pnpx_policy_frozen_ranges": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_int]),
    "pnpx_critic_num_params": (C.c_size_t, [C.c_int]),
    "pnpx_critic_load": (C.c_int, [c_void_p, c_void_p, C.c_size_t, C.c_int]),
    "pnpx_critic_load_device": (C.c_int, [c_void_p, _P, C.c_size_t, C.c_int, c_void_p]),
    "pnpx_critic_soft_update": (C.c_int, [c_void_p, _P, C.c_size_t, C.c_float, C.c_float, c_void_p]),
    "pnpx_critic_params": (C.c_int, [c_void_p, _P, C.c_size_t, c_void_p]),
    "pnpx_critic_forward": (C.c_int, [c_void_p, _P, _P, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_critic_backward": (C.c_int, [c_void_p, _P, _P, _P, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_critic_param_grad": (C.c_int, [c_void_p, _P, _P, _P, C.c_size_t, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_critic_value_loss_grad": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, C.c_size_t, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_critic_adam_step": (C.c_int, [c_void_p, _P, C.c_size_t] + [C.c_float] * 5 + [_P, c_void_p]),
    "pnpx_critic_optim_state": (C.c_int, [c_void_p, _P, _P, C.c_size_t, C.POINTER(C.c_longlong), c_void_p]),
    "pnpx_critic_optim_reset": (C.c_int, [c_void_p]),
    "pnpx_mddpg_policy_loss": (C.c_int, [c_void_p] + [_P] * 6 + [C.c_float] * 3 + [C.c_int] + [_P] * 7 + [c_void_p]),
    "pnpx_unet_profile": (C.c_int, [c_void_p, _P, _P, _P, C.c_int, C.c_int, C.c_int, c_void_p, C.c_int,
                                    c_float_p, C.POINTER(C.c_double), C.POINTER(C.c_char_p), C.POINTER(C.c_int)]),
    "pnpx_fft2": (C.c_int, [c_void_p, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_cdp_forward": (C.c_int, [c_void_p, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_cdp_backward": (C.c_int, [c_void_p, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_spi_inverse": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_psnr": (C.c_int, [c_void_p, _P, _P, _P, C.c_int, C.c_int, c_void_p]),
    "pnpx_rows_gather": (C.c_int, [c_void_p, C.c_int, C.POINTER(c_void_p), C.POINTER(c_void_p), C.POINTER(C.c_size_t), _P,
                                   C.c_int, c_void_p]),
    "pnpx_rows_scatter": (C.c_int, [c_void_p, C.c_int, C.POINTER(c_void_p), C.POINTER(c_void_p), C.POINTER(C.c_size_t), _P,
                                    C.c_int, c_void_p]),
    "pnpx_ring_store": (C.c_int, [c_void_p, C.c_int, C.POINTER(c_void_p), C.POINTER(c_void_p), C.POINTER(C.c_size_t),
                                  C.c_int64, C.c_int64, C.c_int, c_void_p]),
    "pnpx_live_compact": (C.c_int, [c_void_p, _P, _P, C.c_int, _P, C.POINTER(C.c_int), c_void_p]),
    "pnpx_policy_ob_pack": (C.c_int, [c_void_p, C.c_int, C.POINTER(c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), _P,
                                      C.c_int, C.c_int, C.c_int, _P, c_void_p]),
    "pnpx_policy_ob_unpack": (C.c_int, [c_void_p, C.c_int, C.POINTER(c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.c_int, C.c_int, C.c_int, _P, c_void_p]),
    "pnpx_csmri_admm": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 + [c_void_p]),
    "pnpx_csmri_admm_train": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 +
                              [_P, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_csmri_admm_backward": (C.c_int, [c_void_p, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P] + [C.c_int] * 4 +
                                 [C.c_ulonglong, c_void_p]),
    "pnpx_csmri_hqs_train": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 +
                             [_P, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_csmri_hqs_backward": (C.c_int, [c_void_p, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P] + [C.c_int] * 4 +
                                [C.c_ulonglong, c_void_p]),
    "pnpx_csmri_hqs": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 + [c_void_p]),
    "pnpx_csmri_amp": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 + [c_void_p]),
    "pnpx_csmri_pg_train": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 +
                            [_P, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_csmri_pg_backward": (C.c_int, [c_void_p, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P] + [C.c_int] * 4 +
                               [C.c_ulonglong, c_void_p]),
    "pnpx_csmri_pg": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 + [c_void_p]),
    "pnpx_csmri_apg_train": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 +
                             [_P, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_csmri_apg_backward": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P] + [C.c_int] * 4 +
                                [C.c_ulonglong, c_void_p]),
    "pnpx_csmri_apg": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 + [c_void_p]),
    "pnpx_csmri_redadmm_train": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 +
                                 [_P, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_csmri_redadmm_backward": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P] +
                                    [C.c_int] * 4 + [C.c_ulonglong, c_void_p]),
    "pnpx_csmri_redadmm": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 + [c_void_p]),
    "pnpx_pr_iadmm_train": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P, _P] + [C.c_int] * 6 +
                            [_P, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_pr_iadmm_backward": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 +
                               [C.c_ulonglong, c_void_p]),
    "pnpx_pr_iadmm": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P, _P] + [C.c_int] * 6 + [c_void_p]),
    "pnpx_pr_pg_train": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P] + [C.c_int] * 6 +
                         [_P, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_pr_pg_backward": (C.c_int, [c_void_p, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 +
                            [C.c_ulonglong, c_void_p]),
    "pnpx_pr_pg": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P] + [C.c_int] * 6 + [c_void_p]),
    "pnpx_spi_admm_train": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 +
                            [_P, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_spi_admm_backward": (C.c_int, [c_void_p, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P] + [C.c_int] * 4 +
                               [C.c_ulonglong, c_void_p]),
    "pnpx_spi_admm": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 + [c_void_p]),
    "pnpx_spi_pg_step": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_spi_pg_train": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 +
                          [_P, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_spi_pg_backward": (C.c_int, [c_void_p, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P] + [C.c_int] * 4 +
                             [C.c_ulonglong, c_void_p]),
    "pnpx_spi_pg": (C.c_int, [c_void_p, _P, _P, _P, _P, _P, _P] + [C.c_int] * 5 + [c_void_p]),
    "pnpx_radon_det_count": (C.c_int, [C.c_int]),
    "pnpx_radon_forward": (C.c_int, [c_void_p, _P, _P, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_radon_backprojection": (C.c_int, [c_void_p, _P, _P, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_ct_iadmm_train": (C.c_int, [c_void_p, _P, _P, _P, C.c_int, C.c_float, _P, _P, _P] + [C.c_int] * 4 +
                            [_P, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_ct_iadmm_backward": (C.c_int, [c_void_p, C.c_int, C.c_float, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P] +
                               [C.c_int] * 3 + [C.c_ulonglong, c_void_p]),
    "pnpx_ct_pg_train": (C.c_int, [c_void_p, _P, _P, _P, C.c_int, C.c_float, _P, _P] + [C.c_int] * 4 +
                         [_P, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_ct_pg_backward": (C.c_int, [c_void_p, C.c_int, C.c_float, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P] +
                            [C.c_int] * 3 + [C.c_ulonglong, c_void_p]),
    "pnpx_ct_iadmm": (C.c_int, [c_void_p, _P, _P, _P, C.c_int, C.c_float, _P, _P, _P] + [C.c_int] * 4 + [c_void_p]),
    "pnpx_ct_pg": (C.c_int, [c_void_p, _P, _P, _P, C.c_int, C.c_float, _P, _P] + [C.c_int] * 4 + [c_void_p]),
    "pnpx_fan_det_count": (C.c_int, [C.c_int, C.c_float, C.c_float, C.c_float]),
    "pnpx_fan_forward": (C.c_int, [c_void_p, _P, _P, C.POINTER(RadonGeom), C.c_int, C.c_int, c_void_p]),
    "pnpx_fan_backprojection": (C.c_int, [c_void_p, _P, _P, C.POINTER(RadonGeom), C.c_int, C.c_int, c_void_p]),
    "pnpx_fan_tables": (C.c_int, [C.POINTER(RadonGeom), C.c_int, c_float_p, c_float_p, C.POINTER(C.c_int)]),
    "pnpx_ct_hqs_train": (C.c_int, [c_void_p, _P, _P, _P, C.POINTER(RadonGeom), C.c_int, C.c_float, _P, _P] + [C.c_int] * 4 +
                          [_P, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_ct_hqs_backward": (C.c_int, [c_void_p, C.POINTER(RadonGeom), C.c_int, C.c_float, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P] +
                             [C.c_int] * 3 + [C.c_ulonglong, c_void_p]),
    "pnpx_ct_hqs": (C.c_int, [c_void_p, _P, _P, _P, C.POINTER(RadonGeom), C.c_int, C.c_float, _P, _P] + [C.c_int] * 4 + [c_void_p]),
    "pnpx_radon_filter": (C.c_int, [c_void_p, _P, _P, C.POINTER(RadonGeom), C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_fan_backprojection_w": (C.c_int, [c_void_p, _P, _P, C.POINTER(RadonGeom), C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_fan_fbp": (C.c_int, [c_void_p, _P, _P, C.POINTER(RadonGeom), C.c_int, C.c_int, c_void_p]),
    "pnpx_ct_iadmm_geom": (C.c_int, [c_void_p, _P, _P, _P, C.POINTER(RadonGeom), C.c_int, C.c_float, _P, _P, _P] + [C.c_int] * 4 +
                           [c_void_p]),
    "pnpx_ct_iadmm_geom_train": (C.c_int, [c_void_p, _P, _P, _P, C.POINTER(RadonGeom), C.c_int, C.c_float, _P, _P, _P] + [C.c_int] * 4 +
                                 [_P, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_ct_iadmm_geom_backward": (C.c_int, [c_void_p, C.POINTER(RadonGeom), C.c_int, C.c_float, _P, _P, _P, C.c_int] + [_P] * 7 +
                                    [C.c_int] * 3 + [C.c_ulonglong, c_void_p]),
    "pnpx_ct_pg_geom": (C.c_int, [c_void_p, _P, _P, _P, C.POINTER(RadonGeom), C.c_int, C.c_float, _P, _P] + [C.c_int] * 4 + [c_void_p]),
    "pnpx_ct_pg_geom_train": (C.c_int, [c_void_p, _P, _P, _P, C.POINTER(RadonGeom), C.c_int, C.c_float, _P, _P] + [C.c_int] * 4 +
                              [_P, C.POINTER(C.c_ulonglong), c_void_p]),
    "pnpx_ct_pg_geom_backward": (C.c_int, [c_void_p, C.POINTER(RadonGeom), C.c_int, C.c_float, _P, _P, C.c_int] + [_P] * 6 +
                                 [C.c_int] * 3 + [C.c_ulonglong, c_void_p]),
    "pnpx_winof4_matrices": (None, [c_void_p, c_void_p, c_void_p]),
    "pnpx_winof4_pack": (C.c_int, [c_void_p, C.c_int, C.c_int, c_void_p]),
    "pnpx_conv3x3_probe": (C.c_int, [c_void_p, C.c_int, c_void_p, c_void_p, C.c_int, _P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_float, _P,
                                     C.c_int, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_conv3x3_probe_plan": (C.c_int, [C.c_int] * 7),
    "pnpx_upsample2x_probe": (C.c_int, [c_void_p, _P, _P, C.c_int, C.c_int, C.c_int, c_void_p]),
    "pnpx_conv_f32_entry_plan": (C.c_int, [C.c_int] * 9),
    "pnpx_conv_f32_forward_plan": (C.c_int, [C.c_int] * 9),
    "pnpx_winof4_c32_pack": (C.c_int, [c_void_p, C.c_int, C.c_int, c_void_p]),
    "pnpx_winof4_halo_plan": (C.c_int, [C.c_int] * 3 + [c_void_p] * 7),
    "pnpx_conv_hs_probe": (C.c_int, [c_void_p, c_void_p, c_void_p]),
    "pnpx_conv_hs_probe_plan": (C.c_int, [c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "pnpx_vjp_glue_probe": (C.c_int, [c_void_p, c_void_p, c_void_p]),
    "pnpx_vjp_glue_probe_plan": (C.c_int, [c_void_p]),
    "pnpx_fwd_glue_probe": (C.c_int, [c_void_p, c_void_p, c_void_p]),
    "pnpx_fwd_glue_probe_plan": (C.c_int, [c_void_p]),
    "pnpx_net_train_probe": (C.c_int, [c_void_p, c_void_p, c_void_p]),
    "pnpx_net_train_probe_plan": (C.c_int, [c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """The loaded library; raises loudly when it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise PnpxError(
                        f"{LIB_PATH} not found: the HIP library has not been built "
                        "(run `make -C tfpnp_amd/csrc` or __graft_entry__.build()). There is no CPU fallback.")
                l = C.CDLL(LIB_PATH)
                missing = []
                for name, (res, args) in _SIGNATURES.items():
                    try:
                        fn = getattr(l, name)  # AttributeError if the .so lacks a declared symbol
                    except AttributeError:
                        if "PNPX_LIB" in os.environ:   # A/B run against an older build of the ABI (tools/ only)
                            missing.append(name)
                            continue
                        raise
                    fn.restype = res
                    fn.argtypes = args
                if missing:
                    import warnings
                    warnings.warn(f"PNPX_LIB={LIB_PATH} lacks {len(missing)} symbol(s) of include/pnpx.h: "
                                  + ", ".join(missing) + " -- calls to them will fail with AttributeError")
                _lib = l
    return _lib


def check(status):
    if status != 0:
        msg = lib().pnpx_last_error().decode("utf-8", "replace")
        raise PnpxError(f"pnpx call failed (status {status}): {msg}")
