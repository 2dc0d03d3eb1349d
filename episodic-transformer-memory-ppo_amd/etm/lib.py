"""ctypes loader for libetm_hip.so.  Fails loudly: there is no CPU or eager fallback for the kernels."""
import ctypes
import os

import torch  # noqa: F401  -- MUST precede the dlopen below: torch ships its own libamdhip64; loading ours first would put a
#                             second HIP runtime in the process (kernels would then launch on a runtime with no device)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libetm_hip.so")     # (diagnostic tools that load another build assign this before load())
ABI_VERSION = 61

_lib = None

_P = ctypes.c_void_p
_I = ctypes.c_int
_L = ctypes.c_int64
_F = ctypes.c_float
_D = ctypes.c_double

class RolloutGroup(ctypes.Structure):
    """etm_rollout_group of include/etm_hip.h (one worker group of the native rollout driver)."""
    _fields_ = [("graph_exec", ctypes.c_void_p), ("stream", ctypes.c_void_p), ("ready", ctypes.c_void_p), ("n_procs", ctypes.c_int32),
                ("ready_stride", ctypes.c_int32), ("lo", ctypes.c_int32), ("hi", ctypes.c_int32), ("obs_src", ctypes.c_void_p),
                ("stage_dst", ctypes.c_void_p), ("ss_dst", ctypes.c_void_p)]


# name -> (restype, argtypes); mirrors include/etm_hip.h one to one
SIGNATURES = {
    "etm_abi_version": (_I, []),
    "etm_error_string": (ctypes.c_char_p, [_I]),
    "etm_mha_fwd": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "etm_mha_bwd_workspace_bytes": (_L, [_I, _I, _I]),
    "etm_mha_bwd": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                         _P, _L, _I, _I, _I, _I, _P]),
    "etm_attn_cached": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "etm_reset_rows": (_I, [_P, _P, _P, _I, _L, _P]),
    "etm_rollout_window": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _P]),
    "etm_rollout_sample": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "etm_rollout_sample_branched": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P]),
    "etm_rollout_sample_gaussian": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "etm_add_layernorm": (_I, [_P, _P, _I, _P, _P, _P, _F, _P, _I, _I, _P]),
    "etm_conv_relu": (_I, [_P, _P, _L, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "etm_upload": (_I, [_P, _P, _L, _P]),
    "etm_graph_launch": (_I, [_P, _P]),
    "etm_host_direct_write_init": (_I, [_I]),
    "etm_host_store_fence": (_I, [_I]),
    "etm_host_register": (_I, [_P, _L]),
    "etm_host_unregister": (_I, [_P]),
    "etm_rollout_drive": (_I, [_P, _I, _I, _I, _I, _L, _L, _P, _P, _P, _P, _L, _P, _L, _P, _P, _I, _I, _D, _P, _P]),
    "etm_comm_unique_id": (_I, [_P]),
    "etm_comm_init": (_I, [_P, _I, _I, ctypes.POINTER(ctypes.c_void_p)]),
    "etm_allreduce_f32": (_I, [_P, _P, _P, _L, _P]),
    "etm_comm_destroy": (_I, [_P]),
    "etm_rollout_policy": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "etm_rollout_policy_branched": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _I, _P]),
    "etm_rollout_policy_gaussian": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "etm_conv_pack_weights": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "etm_gather_rows": (_I, [_P, _P, _P, _I, _P, _L, _L, _P]),
    "etm_group_norms": (_I, [_P, _P, _P, _I, _P, _I, _P, _P, _P]),
    "etm_step_head": (_I, [_P, _P, _P, _I, _P, _I, _P, _L, _L, _P, _P, _P, _P]),
    "etm_group_norms_step": (_I, [_P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _I, _P, _I, _P, _P]),
    "etm_step_end": (_I, [_P, _I, _P, _I, _P, _P]),
    "etm_relu_bwd_colsum_workspace_bytes": (_L, [_I, _I]),
    "etm_relu_bwd_colsum": (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _P]),
    "etm_host_copier_create": (_P, [_I]),
    "etm_host_copier_destroy": (None, [_P]),
    "etm_host_copier_set_spin": (_I, [_P, _I]),
    "etm_host_copy": (_I, [_P, _P, _P, _L]),
    "etm_rollout_trxl_team": (_I, [_I]),
    "etm_rollout_trxl_set_placement": (_I, [_I]),
    "etm_rollout_trxl_grid": (_I, [_I, _I]),
    "etm_rollout_trxl_supported": (_I, [_I, _I, _I, _I, _I, _I]),
    "etm_rollout_trxl_gate_merged": (_I, [_I, _I]),
    "etm_rollout_trxl_scratch_bytes": (_L, [_I, _I, _I, _I]),
    "etm_rollout_trxl_group_supported": (_I, [_I] * 8),
    "etm_rollout_trxl_supported_branched": (_I, [_I, _I, _I, _I, _P, _I, _I]),
    "etm_rollout_trxl_supported_gaussian": (_I, [_I] * 6),
    "etm_rollout_trxl_group_supported_gaussian": (_I, [_I] * 8),
    "etm_rollout_trxl_group_supported_branched": (_I, [_I, _I, _I, _I, _P, _I, _I, _I, _I]),
    "etm_rollout_trxl_group_grid": (_I, []),
    "etm_rollout_trxl_group_scratch_bytes": (_L, [_I]),
    "etm_window_set_skip_masked": (_I, [_I]),
    "etm_rollout_hidden_splits": (_I, [_I]),
    "etm_rollout_hidden_partial": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "etm_rollout_conv3_hidden_supported": (_I, [_I, _I, _I, _I, _I, _I, _I, _I]),
    "etm_rollout_conv3_hidden": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "etm_rollout_heads": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "etm_gru_gate_rz": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "etm_gru_gate_out": (_I, [_P, _P, _P, _P, _P, _I, _I, _P]),
    "etm_block_row_groups": (_I, [_I]),
    "etm_ln_train_fwd": (_I, [_P, _P, _I, _P, _P, _P, _F, _P, _P, _P, _I, _I, _P]),
    "etm_ln_train_bwd_workspace_bytes": (_L, [_I, _I]),
    "etm_ln_train_bwd_partial_rows": (_I, [_I]),
    "etm_relu_bwd_colsum_partial_rows": (_I, [_I]),
    "etm_colsum_reduce_max_problems": (_I, []),
    "etm_colsum_reduce_grouped": (_I, [_P, _P, _P, _P, _P, _I, _P]),
    "etm_ln_train_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _L, _I, _I, _P]),
    "etm_gate_train_rz": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "etm_gate_train_out": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "etm_gate_train_bwd_workspace_bytes": (_L, [_I, _I]),
    "etm_gate_train_bwd_partial_rows": (_I, [_I]),
    "etm_gate_train_bwd1": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _P]),
    "etm_gate_train_bwd2": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "etm_conv_train_fwd": (_I, [_P, _P, _L, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "etm_conv_train_set_fwd_lds": (_I, [_I]),
    "etm_conv_train_set_wgrad_lds": (_I, [_I]),
    "etm_conv_train_set_dgrad_lds": (_I, [_I]),
    "etm_conv_pack_weights_grouped": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "etm_conv_train_wgrad_slices": (_I, [_I] * 8),
    "etm_conv_wgrad_reduce_grouped": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "etm_conv_train_dgrad": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "etm_conv_train_wgrad_workspace_bytes": (_L, [_I, _I, _I, _I, _I, _I, _I, _I]),
    "etm_conv_train_wgrad": (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "etm_relu_mask": (_I, [_P, _P, _P, _L, _P]),
    "etm_conv_b3_pack": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "etm_conv_b3_fwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "etm_conv_b3_dgrad": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "etm_conv_b3_wgrad_slices": (_I, [_I] * 8),
    "etm_conv_b3_wgrad": (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "etm_bytes_to_unit": (_I, [_P, _P, _P, _L, _L, _P]),
    "etm_conv_relu_u8": (_I, [_P, _P, _L, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "etm_conv_b3_fwd_u8": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "etm_conv_b3_wgrad_u8": (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "etm_grouped_dw_supported": (_I, [_I, _I, _I, _I, _I, _I]),
    "etm_grouped_dw_max_problems": (_I, []),
    "etm_grouped_dw": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "etm_grouped_dw_tile_map": (_I, [_I, _P]),
    "etm_grouped_dw_tail_max_problems": (_I, []),
    "etm_grouped_dw_tail": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _I, _P]),
    "etm_grad_sqnorm": (_I, [_P, _L, _P, _I, _P, _P]),
    "etm_adamw_clip": (_I, [_P, _P, _P, _P, _L, _P, _I, _P, _P, _D, _D, _D, _D, _F, _F, _P, _P]),
    "etm_grad_sqnorm_gated": (_I, [_P, _L, _P, _I, _P, _P, _F, _P, _P, _P]),
    "etm_adamw_clip_gated": (_I, [_P, _P, _P, _P, _L, _P, _I, _P, _P, _D, _D, _D, _D, _F, _F, _P, _P, _P]),
    "etm_grad_sqnorm_adaptive": (_I, [_P, _L, _P, _I, _P, _P, _P, _F, _F, _F, _F, _F, _P, _F, _P, _P, _P]),
    "etm_arena_digest": (_I, [_P, _L, _P, _I, _P, _P]),
    "etm_gae": (_I, [_P, _P, _P, _P, _F, _F, _P, _I, _I, _P]),
    "etm_gae_truncated": (_I, [_P, _P, _P, _P, _P, _P, _F, _F, _P, _I, _I, _P]),
    "etm_obs_stats_supported": (_I, [_I]),
    "etm_obs_stats_workspace_bytes": (_L, [_I, _I]),
    "etm_obs_stats_update": (_I, [_P, _I, _I, _P, _P, _P, _D, _P, _L, _P]),
    "etm_obs_normalize": (_I, [_P, _P, _P, _P, _F, _P, _L, _I, _P]),
    "etm_return_scale_workspace_bytes": (_L, [_I]),
    "etm_return_scale": (_I, [_P, _P, _P, _P, _D, _D, _F, _P, _I, _I, _P, _L, _P]),
    "etm_adv_stats": (_I, [_P, _I, _P, _P]),
    "etm_adv_stats_workspace_bytes": (_L, [_I]),
    "etm_adv_stats_ws": (_I, [_P, _I, _P, _P, _L, _P]),
    "etm_ppo_loss_workspace_bytes": (_L, [_I]),
    "etm_heads_loss_supported": (_I, [_I, _I, _I]),
    "etm_heads_loss_row_floats": (_I, [_I, _I]),
    "etm_heads_loss_workspace_bytes": (_L, [_I, _I, _I]),
    "etm_heads_loss": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _L, _P, _P, _P, _D, _F, _F, _F, _F, _F, _P, _P, _P, _P, _P, _P, _P, _P, _L,
                            _I, _I, _I, _P]),
    "etm_heads_loss_supported_branched": (_I, [_I, _I, _P, _I]),
    "etm_heads_loss_supported_gaussian": (_I, [_I, _I, _I]),
    "etm_heads_loss_gaussian_row_floats": (_I, [_I, _I]),
    "etm_heads_loss_gaussian_workspace_bytes": (_L, [_I, _I, _I]),
    "etm_heads_loss_gaussian": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _L, _P, _P, _P, _D, _F, _F, _F, _F, _F, _P, _P, _P, _P, _P, _P,
                                     _P, _P, _L, _I, _I, _I, _P]),
    "etm_heads_loss_branched": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _L, _P, _P, _P, _D, _F, _F, _F, _F, _F, _P, _P, _P, _P, _P, _P, _P,
                                     _P, _L, _I, _I, _P, _I, _P]),
    "etm_window_fwd": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _F, _P, _L, _L, _P, _P, _L, _L, _P, _I, _I, _I, _I, _I, _P]),
    "etm_window_ln_grad_rows": (_I, [_I]),
    "etm_window_ln_grad": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _P, _I, _I, _I, _I, _P]),
    "etm_window_ln_grad_from_outputs": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _P, _I, _I, _I, _I, _P]),
    "etm_window_ln_grad_guarded": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _P, _P, _F, _P, _I, _I, _I, _I, _P]),
    "etm_ln_row_stats": (_I, [_P, _F, _P, _L, _I, _P]),
    "etm_window_bwd": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _P, _P, _L, _L, _I, _I, _I, _I, _P]),
    "etm_window_dx": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "etm_profile_enable": (_I, [_I]),
    "etm_profile_set_tag": (_I, [_I]),
    "etm_profile_kernel_count": (_I, []),
    "etm_profile_kernel_name": (ctypes.c_char_p, [_I]),
    "etm_profile_collect": (_I, [_P, _P]),
    "etm_ppo_loss": (_I, [_P, _P, _L, _P, _L, _P, _P, _P, _P, _D, _F, _F, _F, _F, _F, _I, _P, _P, _P, _P, _L, _P, _I, _I, _P]),
}
# the step kernel (etm_rollout_trxl*, worker and group form alike): the shared head (h_in ... bv) and middle (host_flag ... hid) of its
# argument lists; between them lie the draw arguments up to host_actions -- uniforms + 7 pointers (categorical) or log_std, normals + 7
# (Box) --, behind them (A, stage_W), (stage_W, branch_sizes, n_branches) or (A, stage_W, low, high), and the stream
_STEP_HEAD = [_P, _P, _P, _P, _I, _P, _L, _L] + [_P] * 9
_STEP_MIDDLE = [_P, _P, _F, _P, _L] + [_P] * 5 + [_L] * 3 + [_P, _I] + [_P] * 10 + [_I] * 8
for _name in ("etm_rollout_trxl", "etm_rollout_trxl_group"):
    SIGNATURES[_name] = (_I, _STEP_HEAD + [_P] * 8 + _STEP_MIDDLE + [_I, _I, _P])
    SIGNATURES[_name + "_branched"] = (_I, _STEP_HEAD + [_P] * 8 + _STEP_MIDDLE + [_I, _P, _I, _P])
    SIGNATURES[_name + "_gaussian"] = (_I, _STEP_HEAD + [_P] * 9 + _STEP_MIDDLE + [_I, _I, _P, _P, _P])
# invalid-action masks (ABI 58): the masked twins take the arguments of their entry with the mask word array in front of the stream
for _name, _extra in (("etm_rollout_sample_branched", [_P]), ("etm_rollout_policy_branched", [_P]), ("etm_rollout_trxl_branched", [_P]),
                      ("etm_rollout_trxl_group_branched", [_P]), ("etm_heads_loss", [_P]), ("etm_heads_loss_branched", [_P]),
                      ("etm_ppo_loss", [_P, _I])):
    _res, _args = SIGNATURES[_name]
    SIGNATURES[_name + "_masked"] = (_res, _args[:-1] + _extra + _args[-1:])
# the exact Gaussian KL (ABI 61): the four Gaussian sampling entries with the means' staging table in front of the stream, and the
# Gaussian heads + loss pass with old_mean, its row stride and old_log_std there
for _name, _extra in (("etm_rollout_sample_gaussian", [_P]), ("etm_rollout_policy_gaussian", [_P]), ("etm_rollout_trxl_gaussian", [_P]),
                      ("etm_rollout_trxl_group_gaussian", [_P])):
    _res, _args = SIGNATURES[_name]
    SIGNATURES[_name + "_means"] = (_res, _args[:-1] + _extra + _args[-1:])
_res, _args = SIGNATURES["etm_heads_loss_gaussian"]
SIGNATURES["etm_heads_loss_gaussian_kl"] = (_res, _args[:-1] + [_P, _L, _P] + _args[-1:])
SIGNATURES["etm_heads_loss_gaussian_kl_row_floats"] = (_I, [_I, _I])
SIGNATURES["etm_heads_loss_gaussian_kl_workspace_bytes"] = (_L, [_I, _I, _I])
# the exact categorical KL (`exact_kl: true`; added with the ABI left at 61 -- no signature above changes): the four categorical sampling
# entries' *_logps forms take their masked twin's arguments (the mask optional) and the log-probs' staging table in front of the stream;
# the loss entries their masked twin's (the mask optional) and old_logps, its row stride (etm_ppo_loss_kl: and the branch's first
# column) there
for _name in ("etm_rollout_sample_branched", "etm_rollout_policy_branched", "etm_rollout_trxl_branched", "etm_rollout_trxl_group_branched"):
    _res, _args = SIGNATURES[_name + "_masked"]
    SIGNATURES[_name + "_logps"] = (_res, _args[:-1] + [_P] + _args[-1:])
for _name, _twin, _extra in (("etm_heads_loss_kl", "etm_heads_loss_masked", [_P, _L]),
                             ("etm_heads_loss_branched_kl", "etm_heads_loss_branched_masked", [_P, _L]),
                             ("etm_ppo_loss_kl", "etm_ppo_loss_masked", [_P, _L, _I])):
    _res, _args = SIGNATURES[_twin]
    SIGNATURES[_name] = (_res, _args[:-1] + _extra + _args[-1:])
SIGNATURES["etm_heads_loss_kl_row_floats"] = (_I, [_I, _I])
SIGNATURES["etm_heads_loss_kl_workspace_bytes"] = (_L, [_I, _I, _I])
# the KL penalty (`kl_penalty`; the ABI stays at 61 -- no signature above changes): each loss entry is its *_kl twin's argument list with
# kl_coef, one device float32, in front of the stream
for _name in ("etm_heads_loss_kl", "etm_heads_loss_branched_kl", "etm_heads_loss_gaussian_kl", "etm_ppo_loss_kl"):
    _res, _args = SIGNATURES[_name]
    SIGNATURES[_name + "_penalty"] = (_res, _args[:-1] + [_P] + _args[-1:])
# previous_step_input (csrc/prev_input.hip; the ABI stays at 61 -- no signature above changes): the table's rows as an addend of
# lin_hidden's pre-activation, and the table's gradient
SIGNATURES["etm_prev_input_supported"] = (_I, [_I, _I])
SIGNATURES["etm_prev_input_rows"] = (_I, [_P, _I, _I, _P, _L, _P, _I, _P, _P, _P, _P, _L, _L, _P])
SIGNATURES["etm_prev_input_grad_chunk"] = (_I, [])
SIGNATURES["etm_prev_input_grad_partial_rows"] = (_I, [_L])
SIGNATURES["etm_prev_input_grad_workspace_bytes"] = (_L, [_L, _I, _I])
SIGNATURES["etm_prev_input_grad"] = (_I, [_P, _L, _P, _L, _P, _I, _P, _P, _I, _I, _L, _P, _L, _P])
# obs_reconstruction (csrc/obs_recon.hip; the ABI stays at 61): the decoder's last layer fused with the sigmoid cross-entropy and its
# gradient, and that layer's data gradient (its weight gradient is etm_conv_train_wgrad with the roles exchanged)
SIGNATURES["etm_obs_recon_supported"] = (_I, [_I, _I, _I])
SIGNATURES["etm_obs_recon_workspace_bytes"] = (_L, [_L, _I, _I, _I])
SIGNATURES["etm_obs_recon_fwd_loss"] = (_I, [_P, _P, _P, _P, _I, _P, _L, _P, _P, _P, _P, _P, _L, _L, _I, _I, _I, _P])
SIGNATURES["etm_obs_recon_dgrad"] = (_I, [_P, _P, _P, _P, _L, _I, _I, _I, _P])
# device-resident environments (csrc/device_env.hip; the ABI stays at 61): CueRoom stepped, auto-reset and rendered by one launch
SIGNATURES["etm_cue_room_supported"] = (_I, [_I, _I])
SIGNATURES["etm_cue_room_state_bytes"] = (_L, [_I])
SIGNATURES["etm_cue_room_reset"] = (_I, [_P, _P, _L, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _L, _P])
SIGNATURES["etm_cue_room_step"] = (_I, [_P, _P, _L, _P, _L, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _L, _P])
# CommandRoom, the second device-resident task (same file, same shape of entry; one more rule word: K, show_steps, gap_steps)
SIGNATURES["etm_command_room_supported"] = (_I, [_I, _I, _I])
SIGNATURES["etm_command_room_state_bytes"] = (_L, [_I])
SIGNATURES["etm_command_room_reset"] = (_I, [_P, _P, _L, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _L, _P])
SIGNATURES["etm_command_room_step"] = (_I, [_P, _P, _L, _P, _L, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _L, _P])
# PathRoom, the third (same file, same shape of entry; the rule words are G, P, M, max_steps)
SIGNATURES["etm_path_room_supported"] = (_I, [_I, _I, _I])
SIGNATURES["etm_path_room_state_bytes"] = (_L, [_I])
SIGNATURES["etm_path_room_reset"] = (_I, [_P, _P, _L, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _L, _P])
SIGNATURES["etm_path_room_step"] = (_I, [_P, _P, _L, _P, _L, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _L, _P])
# SpotRoom, the fourth (the rule words are G, P, N, light_steps, spot_period, health, max_steps)
SIGNATURES["etm_spot_room_supported"] = (_I, [_I, _I, _I, _I])
SIGNATURES["etm_spot_room_state_bytes"] = (_L, [_I])
SIGNATURES["etm_spot_room_reset"] = (_I, [_P, _P, _L, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _L, _P])
SIGNATURES["etm_spot_room_step"] = (_I, [_P, _P, _L, _P, _L, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _L, _P])
# attention statistics (csrc/attn_stats.hip; the ABI stays at 61): att [N, H, L] and the window mask -> sums per head, added to a table
ATTN_STATS_WORDS = 264
SIGNATURES["etm_attn_stats_workspace_bytes"] = (_L, [_I, _I, _I])
SIGNATURES["etm_attn_stats"] = (_I, [_P, _P, _P, _P, _L, _I, _I, _I, _P])
del _twin
del _name, _extra, _res, _args


def load():
    """Return the loaded library (cached).  Raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the MI355X kernels are not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C episodic-transformer-memory-ppo_amd/csrc`. There is no CPU fallback for this path.")
    if os.path.basename(LIB_PATH) != "libetm_hip.so":
        print(f"[etm] using the library build {LIB_PATH}", flush=True)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.etm_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libetm_hip.so ABI {lib.etm_abi_version()} != expected {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().etm_error_string(rc)
        raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")


def profile_collect():
    """{(tag, kernel_name): (total_ms, launches)} for everything recorded since the last call."""
    import numpy as np
    lib = load()
    k = lib.etm_profile_kernel_count()
    ms = np.zeros(2 * k, dtype=np.float64)
    cnt = np.zeros(2 * k, dtype=np.int64)
    check(lib.etm_profile_collect(ms.ctypes.data, cnt.ctypes.data), "etm_profile_collect")
    out = {}
    for tag in (0, 1):
        for i in range(k):
            if cnt[tag * k + i]:
                out[(tag, lib.etm_profile_kernel_name(i).decode())] = (float(ms[tag * k + i]), int(cnt[tag * k + i]))
    return out
