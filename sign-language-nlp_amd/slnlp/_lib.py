"""ctypes binding of libslnlp.so (C ABI in include/slnlp.h).

The library is the product path: there is NO CPU fallback.  Loading works
without a GPU (symbols / layout queries only); any compute entry point needs a
MI355X and raises ``RuntimeError`` with ``slnlp_last_error()`` on failure.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SLNLP_PROBE_LIB=k: load lib/libslnlp_probe<k>.so instead (tools/probes only: `make PROBE=k` builds it with agent-scope fences
# around every kernel, csrc/common.hpp); the product never sets it
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib",
                        f"libslnlp_probe{os.environ['SLNLP_PROBE_LIB']}.so" if os.environ.get("SLNLP_PROBE_LIB") else "libslnlp.so")

i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class GemmArgs(C.Structure):
    _fields_ = [("A", vp), ("lda", i64), ("a_kmajor", i32),
                ("B", vp), ("ldb", i64), ("b_kmajor", i32),
                ("C", vp), ("ldc", i64),
                ("M", i32), ("N", i32), ("K", i32),
                ("bias", vp), ("relu", i32),
                ("gate", vp), ("ldg", i64), ("gate_scale", f32),
                ("drop_p", f32), ("drop_site", i32), ("rng", vp),
                ("resid", vp), ("ldr", i64),
                ("rowsum_a", vp), ("precision", i32), ("gate_mode", i32),
                ("A_hi", vp), ("A_lo", vp), ("lda_p", i64), ("B_hi", vp), ("B_lo", vp), ("ldb_p", i64),
                ("C_hi", vp), ("C_lo", vp), ("ldc_p", i64), ("drop_head_dim", i32),
                ("col_scale", vp), ("C_q8", vp),
                ("batch", i32), ("batch_stride_a", i64), ("batch_stride_b", i64), ("batch_stride_c", i64)]


class TimedLaunch(C.Structure):
    _fields_ = [("blocks", i32), ("njobs", i32), ("geometry", i32), ("us", f32)]


class TfConfig(C.Structure):
    _fields_ = [("E", i32), ("H", i32), ("N", i32), ("F", i32), ("Vs", i32), ("Vt", i32),
                ("B", i32), ("S", i32), ("pad_src", i32), ("pad_tgt", i32),
                ("dropout", f32), ("precision", i32)]


class TfBuffers(C.Structure):
    _fields_ = [("params", vp), ("grads", vp), ("momentum", vp), ("pe", vp), ("workspace", vp),
                ("rng", vp), ("lr", vp), ("scalars", vp)]


class RnnConfig(C.Structure):
    _fields_ = [("lstm", i32), ("E", i32), ("Hd", i32), ("N", i32), ("Vs", i32), ("Vt", i32), ("B", i32), ("S", i32),
                ("pad_src", i32), ("pad_tgt", i32), ("bos_idx", i32), ("dropout", f32), ("precision", i32)]


class RnnCellDir(C.Structure):
    _fields_ = [("xproj", vp), ("hproj", vp), ("h", vp), ("c", vp), ("hprev_save", vp), ("cprev_save", vp),
                ("acts", vp), ("hn_save", vp), ("out", vp), ("t", i32), ("out_row0", i32), ("out_col0", i32)]


class RnnStepDir(C.Structure):
    _fields_ = [("h_in", vp), ("h_out", vp), ("w_hh", vp), ("b_hh", vp), ("xproj", vp), ("c", vp), ("cprev_save", vp),
                ("acts", vp), ("hn_save", vp), ("out", vp), ("t", i32), ("out_row0", i32), ("out_col0", i32)]


class RnnLayerDir(C.Structure):
    _fields_ = [("hprev", vp), ("h_final", vp), ("w_hh", vp), ("b_hh", vp), ("xproj", vp), ("c", vp), ("cprev", vp),
                ("acts", vp), ("hn", vp), ("out", vp), ("out_col0", i32), ("reverse", i32)]


class RnnCellBwdDir(C.Structure):
    _fields_ = [("dh_state", vp), ("dc_state", vp), ("dout", vp), ("acts", vp), ("cprev_save", vp),
                ("hprev_save", vp), ("hn_save", vp), ("dgx", vp), ("dgh", vp), ("carry", vp),
                ("t", i32), ("out_row0", i32), ("out_col0", i32),
                ("dh_extra", vp), ("extra_stride", i64), ("n_extra", i32)]


class RnnStepBwdDir(C.Structure):
    _fields_ = [("cell", RnnCellBwdDir), ("dgh_next", vp), ("w_hh", vp)]


class LnReduceEntry(C.Structure):
    _fields_ = [("partial", vp), ("dgamma", vp), ("dbeta", vp), ("nblk", i32), ("E", i32)]


class LnPartialEntry(C.Structure):
    _fields_ = [("dy", vp), ("x", vp), ("stats", vp), ("partial", vp), ("dec", i32), ("pad", i32)]


class XmemDmemLayer(C.Structure):
    _fields_ = [("probs", vp), ("dsc", vp), ("dmbar", vp), ("qk", vp), ("dcp", vp), ("dbv", vp), ("drop_site", i32), ("pad", i32)]


# name -> (restype, argtypes).  Every symbol include/slnlp.h declares is listed;
# tests/test_abi.py checks the header and this table agree.
SIGNATURES = {
    "slnlp_last_error": (C.c_char_p, []),
    "slnlp_abi_version": (i32, []),
    "slnlp_gemm": (i32, [C.POINTER(GemmArgs), vp]),
    "slnlp_gemm_group_scratch_bytes": (i64, [C.POINTER(GemmArgs), C.POINTER(i32), i32]),
    "slnlp_set_rnn_step_tile": (i32, [i32]),
    "slnlp_gemm_group": (i32, [C.POINTER(GemmArgs), C.POINTER(i32), i32, vp, i64, vp]),
    "slnlp_gemm_wd": (i32, [C.POINTER(GemmArgs), C.POINTER(GemmArgs), vp, i64, vp]),
    "slnlp_gemm_wd_plan": (i32, [C.POINTER(GemmArgs), C.POINTER(GemmArgs), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "slnlp_gemm_rows": (i32, [C.POINTER(GemmArgs), vp]),
    "slnlp_gemm_rows_ln": (i32, [C.POINTER(GemmArgs), vp, i64, vp, vp, f32, vp, vp, vp, vp, i64, vp]),
    "slnlp_gemm_rows_bwd": (i32, [C.POINTER(GemmArgs), C.POINTER(GemmArgs), vp]),
    "slnlp_set_rows_tile": (i32, [i32]),
    "slnlp_quant_rows_fp8": (i32, [vp, i64, i32, i32, vp, i64, vp, vp]),
    "slnlp_split_planes": (i32, [vp, i64, i32, i32, vp, vp, i64, vp]),
    "slnlp_embed_fwd": (i32, [vp, i64, i32, i32, i32, i32, vp, vp, vp, f32, f32, i32, vp, i64, vp]),
    "slnlp_embed_bwd_scratch_bytes": (i64, [i32, i32, i32]),
    "slnlp_embed_bwd": (i32, [vp, i64, i32, i32, i32, i32, vp, vp, f32, i64, f32, i32, vp, vp, vp]),
    "slnlp_embed_fwd_ex": (i32, [vp, i64, i32, i32, i32, i32, vp, vp, vp, f32, f32, i32, vp, i64, vp, vp, vp, vp]),
    "slnlp_embed_bwd_ex": (i32, [vp, i64, i32, i32, i32, i32, vp, vp, f32, i64, f32, i32, vp, vp, vp, vp]),
    "slnlp_attn_self_fwd": (i32, [vp, vp, i64, i64, i32, i32, i32, i32, i32, vp, vp, f32, i32, vp, vp]),
    "slnlp_attn_self_bwd": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, f32, i32, vp, vp]),
    "slnlp_attn_long_scratch_bytes": (i64, [i32, i32, i32]),
    "slnlp_attn_self_bwd_long": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, f32, i32, vp, vp]),
    "slnlp_attn_cross_fwd": (i32, [vp, vp, i64, i32, i32, i32, i32, vp, vp, f32, i32, vp, vp]),
    "slnlp_attn_cross_bwd": (i32, [vp, vp, i64, vp, vp, i32, i32, i32, i32, vp, vp, i64, f32, i32, vp, vp]),
    "slnlp_attn_self_fwd_ex": (i32, [vp, vp, i64, i64, i32, i32, i32, i32, i32, vp, vp, f32, i32, vp, vp, vp, vp, vp]),
    "slnlp_attn_self_bwd_ex": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, f32, i32, vp, vp, vp, vp, vp]),
    "slnlp_attn_cross_bwd_ex": (i32, [vp, vp, i64, vp, vp, i32, i32, i32, i32, vp, vp, i64, f32, i32, vp, vp, vp, vp]),
    "slnlp_attn_mem_fwd": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, f32, i32, vp, vp]),
    "slnlp_attn_mem_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, f32, i32, vp, vp]),
    "slnlp_attn_mem_dmem_all": (i32, [vp, i32, i32, i32, i32, i32, vp, f32, vp, vp]),
    "slnlp_set_xmem_heads": (i32, [i32]),
    "slnlp_layernorm_fwd": (i32, [vp, vp, vp, i32, i32, f32, vp, vp, vp]),
    "slnlp_layernorm_bwd": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, f32, i32, vp, vp, C.POINTER(i32), vp]),
    "slnlp_ln_param_reduce": (i32, [vp, i32, i32, vp]),
    "slnlp_layernorm_fwd_ex": (i32, [vp, vp, vp, i32, i32, f32, vp, vp, vp, vp, vp]),
    "slnlp_layernorm_bwd_ex": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, f32, i32, vp, vp, C.POINTER(i32), i32, vp, vp, vp, vp, vp]),
    "slnlp_ln_param_partial": (i32, [vp, i32, i32, i32, i32, i32, i32, vp]),
    "slnlp_lsm_nll": (i32, [vp, i64, vp, i32, i32, i64, vp, vp, vp, i64, vp, vp]),
    "slnlp_lsm_nll_ex": (i32, [vp, i64, vp, i32, i32, i64, vp, f32, i32, vp, vp, vp, i64, vp, vp]),
    "slnlp_lsm_bwd": (i32, [vp, vp, i32, i32, vp, i64, vp]),
    "slnlp_clip_sgd_step": (i32, [vp, vp, vp, i64, vp, f32, f32, vp, vp, vp, vp]),
    "slnlp_clip_adam_step": (i32, [vp, vp, vp, vp, i64, vp, f32, f32, f32, f32, f32, vp, vp, vp, vp]),
    "slnlp_clip_sgd_step_ex": (i32, [vp, vp, vp, i64, vp, f32, f32, f32, i32, f32, vp, vp, vp, i64, i64, vp]),
    "slnlp_clip_adamw_step": (i32, [vp, vp, vp, vp, i64, vp, f32, f32, f32, f32, f32, vp, vp, vp, i64, i64, vp]),
    "slnlp_param_groups_create": (i32, [i64, i32, vp, vp, i32, vp, vp, C.POINTER(vp)]),
    "slnlp_param_groups_destroy": (None, [vp]),
    "slnlp_clip_sgd_step_groups": (i32, [vp, vp, vp, i64, vp, vp, f32, f32, i32, f32, vp, vp, vp, i64, i64, vp]),
    "slnlp_clip_adam_step_groups": (i32, [vp, vp, vp, vp, i64, vp, vp, f32, f32, f32, i32, f32, vp, vp, vp, i64, i64, vp]),
    "slnlp_average_step": (i32, [vp, vp, i64, vp, i32, f32, i64, i64, vp]),
    "slnlp_swap_arenas": (i32, [vp, vp, i64, vp]),
    "slnlp_score_rows": (i32, [vp, i64, vp, i64, i32, vp, vp, vp, vp, vp]),
    "slnlp_fit_temperature_scratch_bytes": (i64, [i64]),
    "slnlp_fit_temperature": (i32, [vp, i64, vp, i64, i64, vp, vp, i64, vp]),
    "slnlp_scale_logp": (i32, [vp, i64, i64, i64, vp, vp, i64, vp]),
    "slnlp_fit_bias_temperature_scratch_bytes": (i64, [i64, i64]),
    "slnlp_fit_bias_temperature": (i32, [vp, i64, vp, i64, i64, C.c_double, C.c_double, vp, vp, vp, i64, vp]),
    "slnlp_fit_priors_scratch_bytes": (i64, [i64, i64]),
    "slnlp_fit_priors": (i32, [vp, i64, i64, i64, vp, vp, i32, C.c_double, vp, vp, vp, i64, vp]),
    "slnlp_shift_logp": (i32, [vp, i64, i64, i64, vp, vp, vp, i64, vp]),
    "slnlp_reliability_rows": (i32, [vp, i64, vp, i64, i64, i32, vp, vp, vp, vp]),
    "slnlp_topk_rows": (i32, [vp, i64, i64, i64, i32, vp, vp, vp, vp]),
    "slnlp_confusion_matrix": (i32, [vp, vp, i64, i64, vp, vp]),
    "slnlp_confusion_pairs_workspace_bytes": (i64, [i64, i32]),
    "slnlp_confusion_pairs": (i32, [vp, i64, i32, vp, vp, i64, vp]),
    "slnlp_bootstrap_scores": (i32, [vp, vp, vp, vp, i64, i32, i64, i32, i32, i32, C.c_uint64, vp, vp, vp]),
    "slnlp_ensemble_rows": (i32, [vp, vp, vp, vp, i32, i64, i64, i32, vp, i64, vp, vp]),
    "slnlp_ranking_rows": (i32, [vp, i64, vp, i64, i64, vp, vp, vp]),
    "slnlp_conformal_rows": (i32, [vp, i64, vp, i64, i64, vp, i32, C.c_double, i32, i32, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp]),
    "slnlp_conformal_quantile": (i32, [vp, vp, i64, C.c_double, vp, vp]),
    "slnlp_conformal_summary": (i32, [vp, vp, i64, i64, vp, vp]),
    "slnlp_selective_rows": (i32, [vp, i64, vp, i64, i64, i32, vp, vp, vp, vp, vp]),
    "slnlp_selective_counts": (i32, [vp, vp, i64, vp, i32, vp, i32, vp, vp, vp]),
    "slnlp_label_audit": (i32, [vp, i64, vp, i64, i64, vp, i32, vp, i64, vp]),
    "slnlp_scatter_logp": (i32, [vp, i64, i64, i64, vp, vp, vp, i64, i64, vp]),
    "slnlp_train_dynamics_state_bytes": (i64, [i64]),
    "slnlp_train_dynamics_reset": (i32, [vp, i64, i64, vp]),
    "slnlp_train_dynamics_epoch": (i32, [vp, i64, vp, vp, i64, i64, i64, i64, vp, i64, vp, i64, vp]),
    "slnlp_occlude_rows": (i32, [vp, vp, vp, i64, i64, vp, i64, i32, i64, i64, i64, i64, vp, i64, i64, vp, vp, vp, vp]),
    "slnlp_attribution_rows": (i32, [vp, i64, vp, i64, vp, vp, i64, i64, i64, i32, vp, i64, vp, vp, vp]),
    "slnlp_attribution_summary": (i32, [vp, i64, vp, vp, vp, i64, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "slnlp_edit_distances": (i32, [vp, i64, vp, i64, vp, i64, vp, i64, vp, vp]),
    "slnlp_edit_knn_scratch_bytes": (i64, [i64, i64]),
    "slnlp_edit_knn_rows": (i32, [vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, i64, vp, i64, vp, vp, vp, vp]),
    "slnlp_edit_knn_logp": (i32, [vp, vp, vp, vp, vp, i64, i64, i64, i64, i32, C.c_double, i32, C.c_double, vp, vp, i64, vp, vp]),
    "slnlp_edit_long_distances": (i32, [vp, i64, vp, i64, vp, i64, vp, i64, i64, vp, vp]),
    "slnlp_edit_long_knn_scratch_bytes": (i64, [i64, i64]),
    "slnlp_edit_long_knn_rows": (i32, [vp, i64, vp, i64, vp, i64, vp, i64, i64, vp, i64, i64, vp, i64, vp, vp, vp, vp]),
    "slnlp_edit_long_knn_logp": (i32, [vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i32, C.c_double, i32, C.c_double, vp, vp, i64, vp, vp]),
    "slnlp_field_distances": (i32, [vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, vp, vp]),
    "slnlp_field_knn_scratch_bytes": (i64, [i64, i64]),
    "slnlp_field_knn_rows": (i32, [vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, vp, i64, i64, vp, i64, vp, vp, vp, vp]),
    "slnlp_field_knn_logp": (i32, [vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i32, C.c_double, i32, C.c_double, vp, vp, i64, vp, vp]),
    "slnlp_field_distances_w": (i32, [vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, i64, vp, i64, vp, vp]),
    "slnlp_field_knn_rows_w": (i32, [vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, i64, vp, i64, vp, i64, i64, vp, i64, vp, vp, vp, vp]),
    "slnlp_loo_objective": (i32, [vp, i64, vp, i64, i64, vp, i64, i64, vp]),
    "slnlp_dup_groups_begin": (i32, [vp, vp, i64, vp, vp]),
    "slnlp_dup_groups_link": (i32, [vp, i32, i64, i64, i64, i64, vp, vp, vp, vp]),
    "slnlp_dup_groups_finish": (i32, [vp, i64, vp, vp, vp]),
    "slnlp_gloss_structure_begin": (i32, [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp]),
    "slnlp_gloss_structure_rows": (i32, [vp, i32, i64, i64, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]),
    "slnlp_gloss_structure_finish": (i32, [vp, vp, vp, i64, i64, vp, vp, vp]),
    "slnlp_dropout_mask": (i32, [vp, i32, i32, f32, i32, vp, vp]),
    "slnlp_balance_plan_create": (i32, [vp, i64, i32, vp, C.POINTER(vp)]),
    "slnlp_balance_plan_rows": (i64, [vp]),
    "slnlp_balance_plan_destroy": (None, [vp]),
    "slnlp_balanced_order": (i32, [vp, vp, C.c_uint64, i64, vp, vp, vp]),
    "slnlp_augment_rows": (i32, [vp, vp, i64, i64, i64, i64, f32, f32, C.c_uint64, i64, vp, vp, vp]),
    "slnlp_gather_batch": (i32, [vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp]),
    "slnlp_rnn_cell_fwd": (i32, [i32, C.POINTER(RnnCellDir), i32, i32, i32, vp, f32, i64, f32, i32, vp, vp]),
    "slnlp_rnn_layer_fwd": (i32, [i32, C.POINTER(RnnLayerDir), i32, i32, i32, i32, vp, f32, i64, f32, i32, vp, i32, vp,
                                  C.POINTER(i32), vp]),
    "slnlp_rnn_step_fwd": (i32, [i32, C.POINTER(RnnStepDir), i32, i32, i32, vp, f32, i64, f32, i32, vp, i32, vp]),
    "slnlp_rnn_cell_bwd": (i32, [i32, C.POINTER(RnnCellBwdDir), i32, i32, i32, vp, i64, f32, i32, vp, vp]),
    "slnlp_rnn_step_bwd": (i32, [i32, C.POINTER(RnnStepBwdDir), i32, i32, i32, vp, i64, f32, i32, vp, i32, vp]),
    "slnlp_bahdanau_fwd": (i32, [vp, vp, vp, vp, vp, i64, i64, i32, i32, i32, vp, vp, vp]),
    "slnlp_bahdanau_bwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
    "slnlp_rnn_num_params": (i32, [C.POINTER(RnnConfig)]),
    "slnlp_rnn_param_info": (i32, [C.POINTER(RnnConfig), i32, C.c_char_p, C.POINTER(i64 * 2), C.POINTER(i32),
                                   C.POINTER(i64)]),
    "slnlp_rnn_arena_floats": (i64, [C.POINTER(RnnConfig)]),
    "slnlp_rnn_workspace_bytes": (i64, [C.POINTER(RnnConfig)]),
    "slnlp_rnn_create": (i32, [C.POINTER(RnnConfig), C.POINTER(TfBuffers), C.POINTER(vp)]),
    "slnlp_rnn_destroy": (None, [vp]),
    "slnlp_rnn_forward": (i32, [vp, vp, vp, vp, i32, i32, vp, vp]),
    "slnlp_rnn_seed_dlogp": (i32, [vp, vp, vp]),
    "slnlp_rnn_backward": (i32, [vp, vp]),
    "slnlp_rnn_optim": (i32, [vp, f32, f32, vp]),
    "slnlp_rnn_optim_adam": (i32, [vp, vp, f32, f32, f32, f32, f32, vp]),
    "slnlp_rnn_set_destroy_sync": (i32, [vp, i32]),
    "slnlp_rnn_set_criterion": (i32, [vp, vp, f32, i32, vp]),
    "slnlp_rnn_set_update": (i32, [vp, i32, f32, f32, i32]),
    "slnlp_rnn_set_param_groups": (i32, [vp, i32, vp, vp, i32, vp, vp, vp]),
    "slnlp_rnn_set_averaging": (i32, [vp, vp, vp, i32, f32]),
    "slnlp_rnn_train_step": (i32, [vp, vp, vp, vp, i32, f32, f32, vp, vp]),
    "slnlp_rnn_graph_capture_train": (i32, [vp, vp, vp, vp, i32, f32, f32, vp, vp]),
    "slnlp_rnn_graph_launch": (i32, [vp, i32, vp]),
    "slnlp_rnn_set_persistent": (i32, [vp, i32]),
    "slnlp_rnn_set_fused_backward": (i32, [vp, i32]),
    "slnlp_rnn_health": (i32, [vp, C.POINTER(i32)]),
    "slnlp_rnn_tap": (i32, [vp, C.c_char_p, vp, i64, C.POINTER(i64), vp]),
    "slnlp_tf_num_params": (i32, [C.POINTER(TfConfig)]),
    "slnlp_tf_param_info": (i32, [C.POINTER(TfConfig), i32, C.c_char_p, C.POINTER(i64 * 2), C.POINTER(i32),
                                  C.POINTER(i64)]),
    "slnlp_tf_arena_floats": (i64, [C.POINTER(TfConfig)]),
    "slnlp_tf_workspace_bytes": (i64, [C.POINTER(TfConfig)]),
    "slnlp_tf_create": (i32, [C.POINTER(TfConfig), C.POINTER(TfBuffers), C.POINTER(vp)]),
    "slnlp_tf_destroy": (None, [vp]),
    "slnlp_tf_forward": (i32, [vp, vp, vp, i32, i32, vp, vp]),
    "slnlp_tf_seed_dlogp": (i32, [vp, vp, vp]),
    "slnlp_tf_backward": (i32, [vp, vp]),
    "slnlp_tf_optim": (i32, [vp, f32, f32, vp]),
    "slnlp_tf_train_step": (i32, [vp, vp, vp, i32, f32, f32, vp, vp]),
    "slnlp_tf_graph_capture_train": (i32, [vp, vp, vp, i32, f32, f32, vp, vp]),
    "slnlp_tf_graph_launch": (i32, [vp, i32, vp]),
    "slnlp_tf_tap": (i32, [vp, C.c_char_p, vp, i64, C.POINTER(i64), vp]),
    "slnlp_tf_params_changed": (i32, [vp]),
    "slnlp_tf_optim_adam": (i32, [vp, vp, f32, f32, f32, f32, f32, vp]),
    "slnlp_tf_debug_layout": (i32, [vp, C.c_char_p, i64]),
    "slnlp_tf_set_destroy_sync": (i32, [vp, i32]),
    "slnlp_tf_set_criterion": (i32, [vp, vp, f32, i32, vp]),
    "slnlp_tf_set_update": (i32, [vp, i32, f32, f32, i32]),
    "slnlp_tf_set_param_groups": (i32, [vp, i32, vp, vp, i32, vp, vp, vp]),
    "slnlp_tf_set_averaging": (i32, [vp, vp, vp, i32, f32]),
    "slnlp_tf_set_dmem_batched": (i32, [vp, i32]),
    "slnlp_tf_set_dec_ln_fused": (i32, [vp, i32]),
    "slnlp_set_stream_policy": (i32, [i32]),
    "slnlp_set_thread_stream_policy": (i32, [i32]),
    "slnlp_set_backward_passes": (i32, [i32, i32]),
    "slnlp_get_backward_passes": (i32, [C.POINTER(i32), C.POINTER(i32)]),
    "slnlp_launch_timer_start": (i32, [i32]),
    "slnlp_launch_timer_stop": (i32, [C.POINTER(TimedLaunch), i32]),
    "slnlp_set_plane_tile": (i32, [i32]),
    "slnlp_plane_geo": (i32, [vp, vp, i32]),
    "slnlp_set_gemm_ks": (i32, [i32]),
    "slnlp_set_fp8_tile": (i32, [i32]),
    "slnlp_tf_lockstep_workspace_bytes": (i64, [vp, i32]),
    "slnlp_tf_lockstep_create": (i32, [vp, i32, vp, i64, vp, vp]),
    "slnlp_tf_lockstep_destroy": (None, [vp]),
    "slnlp_tf_lockstep_set_data": (i32, [vp, i32, vp, vp, i64, vp, vp, vp]),
    "slnlp_tf_lockstep_step": (i32, [vp, i32, i64, i32, i32, i32, C.c_float, C.c_float, vp]),
    "slnlp_tf_lockstep_epoch": (i32, [vp, i32, i32, i32, C.c_float, C.c_float, vp]),
    "slnlp_tf_lockstep_num_launches": (i32, [vp, i32, i32, i32]),
    "slnlp_tf_lockstep_set_adam": (i32, [vp, vp, f32, f32, f32, f32]),
    "slnlp_tf_lockstep_set_lr_table": (i32, [vp, vp, i32, vp]),
    "slnlp_tf_lockstep_set_order": (i32, [vp, i32, vp, i64, vp]),
    "slnlp_tf_lockstep_set_averaging": (i32, [vp, vp, vp, i32, f32]),
    "slnlp_tf_lockstep_set_destroy_sync": (i32, [vp, i32]),
    "slnlp_rnn_lockstep_workspace_bytes": (i64, [vp, i32]),
    "slnlp_rnn_lockstep_create": (i32, [vp, i32, vp, i64, vp, vp]),
    "slnlp_rnn_lockstep_destroy": (None, [vp]),
    "slnlp_rnn_lockstep_set_data": (i32, [vp, i32, vp, vp, vp, i64, vp, vp, vp]),
    "slnlp_rnn_lockstep_step": (i32, [vp, i32, i64, i32, i32, i32, C.c_float, C.c_float, vp]),
    "slnlp_rnn_lockstep_epoch": (i32, [vp, i32, i32, i32, C.c_float, C.c_float, vp]),
    "slnlp_rnn_lockstep_num_launches": (i32, [vp, i32, i32, i32]),
    "slnlp_rnn_lockstep_set_adam": (i32, [vp, vp, f32, f32, f32, f32]),
    "slnlp_rnn_lockstep_set_lr_table": (i32, [vp, vp, i32, vp]),
    "slnlp_rnn_lockstep_set_order": (i32, [vp, i32, vp, i64, vp]),
    "slnlp_rnn_lockstep_set_averaging": (i32, [vp, vp, vp, i32, f32]),
    "slnlp_rnn_lockstep_set_destroy_sync": (i32, [vp, i32]),
}

_lib = None


def load():
    """Load libslnlp.so (once).  Raises if the in-tree build is missing --
    run ``python -c 'import __graft_entry__ as g; g.build()'`` or ``make`` in
    sign-language-nlp_amd/."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libslnlp.so not built at {LIB_PATH}: the HIP extension is the "
                               "only compute path (no CPU fallback)")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("SLNLP_PROBE_LIB") and not hasattr(lib, name):
                continue              # an A / B library built from an older tree (tools/ab_bench.py) lacks the newer entry points
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = load().slnlp_last_error().decode(errors="replace")
        raise RuntimeError(f"libslnlp {what} failed (code {rc}): {msg}")


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("slnlp: no MI355X visible -- the HIP path is the only compute path "
                           "(there is deliberately no CPU fallback)")


REDUCTIONS = {"mean": 0, "sum": 1}             # CrossEntropyLoss reductions the fused criterion implements
UPDATE_KINDS = {"sgd": 0, "adam": 1, "adamw": 2}  # SLNLP_UPDATE_*
AVERAGE_KINDS = {"swa": 0, "ema": 1}            # SLNLP_AVG_*
CALIBRATION_REASONS = {1: "flat", 2: "bound", 3: "gradient", 4: "step", 5: "cap"}   # SLNLP_CAL_* of slnlp_fit_temperature
BIAS_CALIBRATION_REASONS = {**CALIBRATION_REASONS, 6: "pivot"}   # ... of slnlp_fit_bias_temperature: SLNLP_CAL_PIVOT too
BIAS_CAL_MAX_V = 512                            # SLNLP_BIAS_CAL_MAX_V
PRIOR_REASONS = {1: "tol", 2: "cap", 3: "empty"}   # SLNLP_PRIOR_*
PRIOR_MAX_ITER = 1024                           # SLNLP_PRIOR_MAX_ITER
REL_MAX_BINS = 64                               # SLNLP_REL_MAX_BINS
RANK_CHUNK = 2048                               # SLNLP_RANK_CHUNK
RANK_MAX_ROWS = 67108863                        # SLNLP_RANK_MAX_ROWS
TOPK_MAX = 64                                   # SLNLP_TOPK_MAX
CONFORMAL_MAX_V = 1024                          # SLNLP_CONFORMAL_MAX_V
CONFORMAL_METHODS = {"lac": 0, "aps": 1}        # SLNLP_CONFORMAL_LAC / _APS
CONFORMAL_STAGE = 0x636F6E66                    # SLNLP_CONFORMAL_STAGE
SEL_SCORES = {"max_prob": 0, "margin": 1, "neg_entropy": 2}    # SLNLP_SEL_MAX_PROB / _MARGIN / _NEG_ENTROPY
SEL_CHUNK = 2048                                # SLNLP_SEL_CHUNK
SEL_MAX_LEVELS = 8                              # SLNLP_SEL_MAX_LEVELS
SEL_TABLE_HEAD = 40                             # SLNLP_SEL_TABLE_HEAD
SEL_MAX_ROWS = 1048576                          # SLNLP_SEL_MAX_ROWS
AUDIT_HEAD_BYTES = 64                           # SLNLP_AUDIT_HEAD_BYTES
DYN_HEAD_BYTES = 64                             # SLNLP_DYN_HEAD_BYTES
DYN_FRAC_BITS = 20                              # SLNLP_DYN_FRAC_BITS
DYN_VISIT_BITS = 23                             # SLNLP_DYN_VISIT_BITS
OCCLUDE_KINDS = ("mask", "drop", "substitute")  # SLNLP_OCCLUDE_MASK / _DROP / _SUBSTITUTE
ATTR_MAX_BINS = 64                              # SLNLP_ATTR_MAX_BINS
ATTR_HEAD_BYTES = 64                            # SLNLP_ATTR_HEAD_BYTES
ATTR_TARGETS = ("label", "pred")                # target 0: the label; 1: the base row's arg-max
EDIT_MAX_LEN = 64                               # SLNLP_EDIT_MAX_LEN
EDIT_LONG_MAX_LEN = 512                         # SLNLP_EDIT_LONG_MAX_LEN
EDIT_MAX_K = 64                                 # SLNLP_EDIT_MAX_K
EDIT_MAX_ROWS = 2 ** 30                         # SLNLP_EDIT_MAX_ROWS
EDIT_MAX_PAIRS = 2 ** 31                        # SLNLP_EDIT_MAX_PAIRS
EDIT_HEAD_BYTES = 64                            # SLNLP_EDIT_HEAD_BYTES
EDIT_WEIGHTS = ("uniform", "distance")          # SLNLP_EDIT_UNIFORM / _DISTANCE
FIELD_MAX_FIELDS = 16                           # SLNLP_FIELD_MAX_FIELDS
FIELD_MAX_WEIGHT = 16                           # SLNLP_FIELD_MAX_WEIGHT
LOO_SLOT_BYTES = 32                             # SLNLP_LOO_SLOT_BYTES
LOO_MAX_SLOTS = 65536                           # SLNLP_LOO_MAX_SLOTS
DUP_HEAD_BYTES = 64                             # SLNLP_DUP_HEAD_BYTES
GLOSS_HEAD_BYTES = 64                           # SLNLP_GLOSS_HEAD_BYTES
GLOSS_MAX_CLASSES = 1024                        # SLNLP_GLOSS_MAX_CLASSES
CONFUSION_MAX_V = 4096                          # SLNLP_CONFUSION_MAX_V
PAIRS_MAX = 64                                  # SLNLP_PAIRS_MAX
BOOT_MAX_REPLICATES = 65536                     # SLNLP_BOOT_MAX_REPLICATES
BOOT_MAX_VALUES = 8                             # SLNLP_BOOT_MAX_VALUES
BOOT_FIXED = 9                                  # SLNLP_BOOT_FIXED
BOOT_STAGE = 0x626F6F74                         # SLNLP_BOOT_STAGE
ENSEMBLE_MAX_MEMBERS = 32                       # SLNLP_ENSEMBLE_MAX_MEMBERS
VOTING = {"soft": 0, "log": 1}                  # SLNLP_VOTE_*


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else t.data_ptr()


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream
