"""ctypes binding of libpfn_hip.so (the C ABI declared in include/pfn_hip.h).

PyTorch-ROCm is only plumbing here: it owns device memory and streams; every arithmetic step of
the hot path runs in the hand-written gfx950 kernels behind this boundary.  There is NO fallback:
if the shared library is missing (or was built for another ABI version) every product entry
point raises, it never silently routes to PyTorch ops.
"""
import ctypes
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libpfn_hip.so')
ABI_VERSION = 10

MAX_FEATURES = 1022      # pfn_model_desc.num_features (include/pfn_hip.h): wider encoders are refused when the model is built
PREC_BF16 = 0
PREC_F32 = 1
PREC_FP16 = 2      # fp16 MFMA operands under a device-side loss scale (include/pfn_hip.h): the timed path that holds the north star's 1e-3
PRECISIONS = {'bf16': PREC_BF16, 'f32': PREC_F32, 'fp32': PREC_F32, 'fp16': PREC_FP16, 'f16': PREC_FP16}
SCHED_TOP_LAYER_ALL_ROWS, SCHED_FUSE_LN_WIDE, SCHED_SEPARATE_LNBWD, SCHED_DETERMINISTIC, SCHED_NO_KEY_CENTERING, SCHED_FUSE_Q_PROJECTION, SCHED_KEY_CENTERING, SCHED_F32_RESIDUAL = 1, 2, 4, 8, 16, 32, 64, 128     # pfn_model_desc.schedule bits (include/pfn_hip.h)
NUTS_ADAPT_MASS, NUTS_KEEP_WARMUP, NUTS_MAX_WINDOWS, NUTS_INV_MASS_OFFSET = 1, 2, 16, 256      # PFN_NUTS_* (include/pfn_hip.h)

# GEMM epilogue flags (csrc/pfn_kernels.h)
EPI_BIAS, EPI_GELU, EPI_GELU_BWD, EPI_RESID, EPI_OUT_F32, EPI_OUT_T, EPI_OUT2_T, EPI_ACCUM, EPI_RESID_T = 1, 2, 4, 8, 16, 32, 64, 128, 256


class HipExtensionError(RuntimeError):
    pass


class ModelDesc(ctypes.Structure):
    _fields_ = [('num_features', ctypes.c_int32), ('emsize', ctypes.c_int32), ('nhead', ctypes.c_int32),
                ('nhid', ctypes.c_int32), ('nlayers', ctypes.c_int32), ('n_out', ctypes.c_int32),
                ('precision', ctypes.c_int32), ('ln_eps', ctypes.c_float), ('dropout', ctypes.c_float), ('schedule', ctypes.c_int32)]

    def key(self):
        return (self.num_features, self.emsize, self.nhead, self.nhid, self.nlayers, self.n_out, self.precision, self.ln_eps, self.dropout, self.schedule)


HOST_CALLBACK = ctypes.CFUNCTYPE(None, ctypes.c_void_p)     # pfn_host_callback

_lib = None

_c = ctypes
_P, _I, _L, _F, _U64 = _c.c_void_p, _c.c_int, _c.c_int64, _c.c_float, _c.c_uint64
_D = _c.POINTER(ModelDesc)

# name -> (restype, argtypes).  This table is the Python mirror of include/pfn_hip.h; the not-gpu
# test suite checks that the library exports every one of these symbols.
SIGNATURES = {
    'pfn_abi_version': (_I, []),
    'pfn_last_error_string': (_c.c_char_p, []),
    'pfn_set_tuning': (_I, [_I, _I]),
    'pfn_default_schedule': (_I, []),
    'pfn_profile_enable': (_I, [_I]),
    'pfn_profile_read': (_I, [_I, _c.POINTER(_c.c_double), _c.POINTER(_L)]),
    'pfn_param_layout': (_I, [_D, _c.POINTER(_L), _c.POINTER(_L), _I]),
    'pfn_param_count': (_L, [_D]),
    'pfn_shadow_bytes': (_L, [_D]),
    'pfn_prepare_params': (_I, [_D, _P, _P, _P]),
    'pfn_workspace_bytes': (_L, [_D, _I, _I]),
    'pfn_top_layer_rows': (_L, [_D, _I, _I, _I, _I]),
    'pfn_stack_forward': (_I, [_D, _P, _P, _P, _L, _L, _P, _L, _L, _P, _I, _I, _I, _P, _L, _P, _P]),
    'pfn_stack_backward': (_I, [_D, _P, _P, _P, _L, _L, _P, _L, _L, _I, _I, _I, _P, _L, _P, _P, _P, _P]),
    'pfn_stack_forward_dropout': (_I, [_D, _P, _P, _P, _L, _L, _P, _L, _L, _P, _I, _I, _I, _P, _L, _P, _P, _U64]),
    'pfn_stack_backward_split': (_I, [_D, _P, _P, _P, _L, _L, _P, _L, _L, _I, _I, _I, _P, _L, _P, _P, _P, _P, _I, _P, _P, _I, _U64]),
    # (d, params, shadow, x, x_st, x_sb, y, y_st, y_sb, B, S, sep_of, row_off, sep_min, sep_max, test_rows, ws, ws_bytes, logits, stream, use_dropout, seed)
    'pfn_stack_forward_ragged': (_I, [_D, _P, _P, _P, _L, _L, _P, _L, _L, _I, _I, _P, _P, _I, _I, _L, _P, _L, _P, _P, _I, _U64]),
    # (..., ws, ws_bytes, dlogits, grads, stream, first_group_layers, callback, user, use_dropout, seed)
    'pfn_stack_backward_ragged': (_I, [_D, _P, _P, _P, _L, _L, _P, _L, _L, _I, _I, _P, _P, _I, _I, _L, _P, _L, _P, _P, _P, _I, _P, _P, _I, _U64]),
    'pfn_context_bytes': (_L, [_D, _I, _I]),
    # (d, params, shadow, x, x_st, x_sb, y, y_st, y_sb, B, sep, ws, ws_bytes, context, context_bytes, stream)
    'pfn_stack_condition': (_I, [_D, _P, _P, _P, _L, _L, _P, _L, _L, _I, _I, _P, _L, _P, _L, _P]),
    'pfn_predict_workspace_bytes': (_L, [_D, _I, _I]),
    # (d, params, shadow, context, context_bytes, sep, x, x_st, x_sb, B, n, ws, ws_bytes, logits, stream)
    'pfn_stack_predict': (_I, [_D, _P, _P, _P, _L, _I, _P, _L, _L, _I, _I, _P, _L, _P, _P]),
    'pfn_predict_grad_workspace_bytes': (_L, [_D, _I, _I]),
    # (same arguments as pfn_stack_predict; the workspace of pfn_predict_grad_workspace_bytes)
    'pfn_stack_predict_saved': (_I, [_D, _P, _P, _P, _L, _I, _P, _L, _L, _I, _I, _P, _L, _P, _P]),
    # (d, params, shadow, context, context_bytes, sep, B, n, ws, ws_bytes, dlogits, dx, dx_st, dx_sb, stream)
    'pfn_stack_predict_backward': (_I, [_D, _P, _P, _P, _L, _I, _I, _I, _P, _L, _P, _P, _L, _L, _P]),
    # a different train-row count per dataset (ABI 10, additive): `sep` -> sep_max, sep_of [B] int32 on the device
    # (d, params, shadow, x, x_st, x_sb, y, y_st, y_sb, B, sep_max, sep_of, ws, ws_bytes, context, context_bytes, stream)
    'pfn_stack_condition_ragged': (_I, [_D, _P, _P, _P, _L, _L, _P, _L, _L, _I, _I, _P, _P, _L, _P, _L, _P]),
    # (d, params, shadow, context, context_bytes, sep_max, sep_of, x, x_st, x_sb, B, n, ws, ws_bytes, logits, stream)
    'pfn_stack_predict_ragged': (_I, [_D, _P, _P, _P, _L, _I, _P, _P, _L, _L, _I, _I, _P, _L, _P, _P]),
    'pfn_stack_predict_saved_ragged': (_I, [_D, _P, _P, _P, _L, _I, _P, _P, _L, _L, _I, _I, _P, _L, _P, _P]),
    # (d, params, shadow, context, context_bytes, sep_max, sep_of, B, n, ws, ws_bytes, dlogits, dx, dx_st, dx_sb, stream)
    'pfn_stack_predict_backward_ragged': (_I, [_D, _P, _P, _P, _L, _I, _P, _I, _I, _P, _L, _P, _P, _L, _L, _P]),
    # (d, params, B, S, sep, ws, ws_bytes, dx, dx_st, dx_sb, dy, dy_st, dy_sb, stream)
    'pfn_stack_input_grads': (_I, [_D, _P, _I, _I, _I, _P, _L, _P, _L, _L, _P, _L, _L, _P]),
    'pfn_bar_nll_forward': (_I, [_P, _L, _P, _P, _L, _I, _I, _P, _P, _P, _P]),
    'pfn_bar_nll_backward': (_I, [_P, _L, _P, _P, _P, _L, _I, _P, _P]),
    'pfn_bar_mean': (_I, [_P, _L, _P, _L, _I, _I, _P, _P]),
    # (logits, ld, borders, R, nbars, full_support, mean, gout, dlogits, stream)
    'pfn_bar_mean_backward': (_I, [_P, _L, _P, _L, _I, _I, _P, _P, _P, _P]),
    # (logits, ld, borders, R, nbars, full_support, kinds [host int32], K, args, arg_ld, out, stream)      -- ABI 10, additive
    'pfn_bar_stats': (_I, [_P, _L, _P, _L, _I, _I, _P, _I, _P, _L, _P, _P]),
    # (logits, ld, borders, R, nbars, full_support, kinds, K, args, arg_ld, out, gout, dlogits, stream)
    'pfn_bar_stats_backward': (_I, [_P, _L, _P, _L, _I, _I, _P, _I, _P, _L, _P, _P, _P, _P]),
    # (logits, ld, borders, R, nbars, full_support, n_samples, seed, out, stream)
    'pfn_bar_sample': (_I, [_P, _L, _P, _L, _I, _I, _I, _U64, _P, _P]),
    'pfn_clip_adam_step': (_I, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _F, _I, _I, _P, _P]),
    'pfn_gp_workspace_bytes': (_L, [_I, _I]),
    'pfn_gp_prior_sample': (_I, [_P, _P, _P, _P, _L, _P, _P, _P, _I, _I, _I, _I, _I, _I, _U64, _U64, _P, _P]),
    'pfn_gp_posterior': (_I, [_P, _P, _P, _L, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    # GP hyper-parameter fit (ABI 10, additive).  (x, y, n_of, theta, prior, P, S, nf, kernel, flags, ws, ws_bytes, value, grad, info, stream)
    'pfn_gp_fit_workspace_bytes': (_L, [_I, _I]),
    'pfn_gp_mll_grad': (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _L, _P, _P, _P, _P]),
    # (x, y, n_of, theta, prior, P, S, nf, kernel, x_test, m, ws, ws_bytes, mean, var, info, stream)
    'pfn_gp_fit_predict': (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _L, _P, _P, _P, _P]),
    # batched NUTS (ABI 10, additive).  (ws, ws_bytes, C, D, ld, max_tree_depth, num_warmup, num_samples, flags, window_ends [host int32], n_windows, window_start,
    #  step_size, target_accept, seed, chain_ids, theta0, inv_mass0, trial, done_count, stream)
    'pfn_nuts_workspace_bytes': (_L, [_I, _I, _I]),
    'pfn_nuts_init': (_I, [_P, _L, _I, _I, _L, _I, _I, _I, _I, _P, _I, _I, _F, _F, _U64, _P, _P, _P, _P, _P, _P]),
    # (ws, ws_bytes, C, D, ld, max_tree_depth, num_warmup, num_samples, value, grad, info, scale, shift, trial, samples, stats, warm, done_count, stream)
    'pfn_nuts_advance': (_I, [_P, _L, _I, _I, _L, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    # BNN posterior target (ABI 10, additive).  (x, y, n_of, theta, ld, P, K, S, F, H, activation, value, grad, stream)
    'pfn_bnn_logp_grad': (_I, [_P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    # (x_test, theta, ld, P, K, m, F, H, activation, prob1, stream)
    'pfn_bnn_predict': (_I, [_P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P]),
    # SVI on the BNN (ABI 10, additive).  (x, y, n_of, state, ld, P, S, F, H, activation, num_particles, step0, num_steps, lr, beta1, beta2, eps, seed, problem_ids, loss, stream)
    'pfn_bnn_svi_steps': (_I, [_P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _L, _I, _F, _F, _F, _F, _U64, _P, _P, _P]),
    # SVGD on the BNN (ABI 10, additive).  (P, num_particles, F, H)
    'pfn_bnn_svgd_workspace_bytes': (_L, [_I, _I, _I, _I]),
    # (x, y, n_of, state, ld, P, S, F, H, activation, num_particles, step0, num_steps, lr, beta1, beta2, eps, bandwidth_factor, workspace, workspace_bytes, potential,
    #  bandwidth, stream)
    'pfn_bnn_svgd_steps': (_I, [_P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _L, _I, _F, _F, _F, _F, _F, _P, _L, _P, _P, _P]),
    # tabular study (ABI 10, additive).  (X, y, starts, N, F, F_out, W, bptt, sep, rescale, mode, x_out, y_out, stream)
    'pfn_tabular_windows': (_I, [_P, _P, _P, _L, _I, _I, _I, _I, _I, _F, _I, _P, _P, _P]),
    # (scores, labels, T, C, counts, stream)
    'pfn_auc_counts': (_I, [_P, _P, _I, _I, _P, _P]),
    # (train, labels, test, fold, P, n, T, F, cv_correct, test_pos, test_nbr, stream)
    'pfn_knn_cv': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    # logistic regression with its grid search (ABI 10, additive).  (train, labels, test, fold, cand_C, cand_kind, P, n, T, F, NC, n_splits, cv_correct, test_z, status,
    #  coef, stream)
    'pfn_logistic_cv': (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    # BNN classifier with its grid search (ABI 10, additive).  (train, labels, test, fold, cand_H (host), cand_lr (host), P, n, T, F, NC, n_splits, state, ld, step0,
    #  num_steps, beta1, beta2, eps, num_pred_samples, seed, problem_ids, loss, cv_prob, test_prob, cv_draw, test_draw, status, stream)
    'pfn_bnn_cv': (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _L, _L, _I, _F, _F, _F, _I, _U64, _P, _P, _P, _P, _P, _P, _P, _P]),
    # Gradient-boosted trees with their grid search (ABI 10, additive).  (train, labels, test, fold, cand_depth, cand_lr, cand_mcw, cand_subsample, cand_colsample,
    # cand_ids, P, n, T, F, NC, n_splits, num_rounds, seed, problem_ids, order, cv_margin, test_margin, status, tree_feature, tree_threshold, tree_leaf, stream)
    'pfn_xgb_cv': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _U64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    # Oblivious boosted trees with their grid search (ABI 10, additive).  (train, labels, test, fold, cand_depth, cand_lr, cand_l2, cand_ids, checkpoints, P, n, T, F,
    # NC, NK, num_rounds, seed, problem_ids, order, hold_margin, test_margin, status, tree_feature, tree_threshold, tree_leaf, stream)
    'pfn_catboost_cv': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _U64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    # GP classifier with its grid search (ABI 10, additive).  (theta, train, labels, fold, P, n, F, NC, n_splits, value, grad, status, stream)
    'pfn_gpc_lml_grad': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    # (theta, train, labels, test, fold, P, n, T, F, NC, n_splits, cv_f, test_f, test_var, status, stream)
    'pfn_gpc_predict': (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    # stroke prior of the few-shot study (ABI 10, additive).  (segs, n_strokes, width, noise, N, size, normalize, image_stride, seed, offset, x, raw, img, stream)
    'pfn_stroke_render': (_I, [_P, _P, _P, _P, _L, _I, _I, _L, _U64, _U64, _P, _P, _P, _P]),
    # (labels, B, T, num_classes, size, normalize, strokes_lo, strokes_hi, len_lo, len_hi, start_lo, start_hi, width_lo, width_hi, max_offset, max_target_offset, seed, offset,
    #  first_dataset, x, cls_n, cls_len, cls_start, cls_dir, segs, width, raw, img, status, stream)
    'pfn_stroke_prior_sample': (_I, [_P] + [_I] * 15 + [_U64] * 3 + [_P] * 11),
    # class-label embedding of the few-shot study (ABI 10, additive).  (B, S, F, E, C, prec)
    'pfn_class_embed_workspace_bytes': (_L, [_I] * 6),
    # (x, x_st, x_sb, labels, l_st, l_sb, wx, bx, table, B, S, F, E, C, sep, prec, flags, workspace, workspace_bytes, src_sbe, status, stream)
    'pfn_class_embed_forward': (_I, [_P, _L, _L, _P, _L, _L, _P, _P, _P] + [_I] * 8 + [_P, _L, _P, _P, _P]),
    # (dsrc_sbe, wx, B, S, F, E, C, sep, prec, flags, workspace, workspace_bytes, dwx, dbx, dtable, stream)
    'pfn_class_embed_backward': (_I, [_P, _P] + [_I] * 8 + [_P, _L, _P, _P, _P, _P]),
    # Omniglot episode loader of the few-shot study (ABI 10, additive).  (bank, table, n_classes, n_img, size, src, rot, shift_in, N, translate, image_stride, seed,
    #  offset, first_image, x, bbox, shift, status, stream)
    'pfn_episode_gather': (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _L, _I, _L, _U64, _U64, _U64, _P, _P, _P, _P, _P]),
    # (bank, table, n_classes, n_img, size, B, n_way, k_shot, mode, train, translate, pool_lo, pool_hi, alphabet_offsets, n_alphabets, seed, offset, first_dataset,
    #  x, labels, targets, classes, rotations, src, shift, bbox, status, stream)
    'pfn_episode_sample': (_I, [_P, _P] + [_I] * 11 + [_P, _I] + [_U64] * 3 + [_P] * 10),
    'pfn_mlp_prior_forward': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _U64, _U64, _P]),
    'pfn_op_gemm_nt': (_I, [_P, _L, _P, _L, _I, _I, _I, _I, _P, _P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _I, _P]),
    'pfn_op_gemm_tn': (_I, [_P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _P]),
    'pfn_op_gemm_tn_group': (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    'pfn_op_gemm_ln': (_I, [_P, _L, _P, _L, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _I, _P]),
    'pfn_op_gemm_lnbwd': (_I, [_P, _L, _P, _L, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    'pfn_op_attention_fwd': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'pfn_op_attention_bwd_ws_bytes': (_L, [_I, _I, _I, _I]),
    'pfn_op_attention_fwd_from': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    'pfn_op_attention_bwd_from': (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    'pfn_op_gather_rows': (_I, [_P, _P, _I, _I, _L, _I, _P]),
    'pfn_op_scatter_rows': (_I, [_P, _P, _I, _I, _L, _I, _I, _P]),
    'pfn_op_attention_bwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    # (test only, ABI 10, additive) the pair above with dropout on the probabilities: (..., prec[, parts], p_drop, site seed, stream)
    'pfn_op_attention_fwd_dropout': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _c.c_uint32, _P]),
    'pfn_op_attention_bwd_dropout': (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _c.c_uint32, _P]),
    'pfn_op_layernorm_fwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _F, _I, _P]),
    'pfn_op_layernorm_bwd': (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _P]),
    'pfn_op_cast': (_I, [_P, _P, _L, _I, _P]),
    'pfn_op_qkv_projection': (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _P]),
}


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 into libpfn_hip.so (in-tree). hipcc cross-compiles without a GPU."""
    script = os.path.join(_HERE, 'csrc', 'build.sh')
    res = subprocess.run(['bash', script], capture_output=True, text=True)
    if res.returncode != 0 or not os.path.exists(LIB_PATH):
        raise HipExtensionError('building libpfn_hip.so failed:\n' + res.stdout[-4000:] + res.stderr[-8000:])
    if verbose:
        print(res.stdout[-2000:])
    return LIB_PATH


def lib():
    """The loaded library (import torch first so libamdhip64 is already resident)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipExtensionError(
                f'{LIB_PATH} not found. Build it with `python -c "import __graft_entry__ as g; g.build()"` '
                f'(or transformerscandobayesianinference_amd/csrc/build.sh). There is no CPU / PyTorch fallback for the hot path.')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise HipExtensionError(f'libpfn_hip.so does not export {name}') from e
            fn.restype = res
            fn.argtypes = args
        if handle.pfn_abi_version() != ABI_VERSION:
            raise HipExtensionError(f'libpfn_hip.so ABI {handle.pfn_abi_version()} != binding ABI {ABI_VERSION}; rebuild')
        _lib = handle
    return _lib


def check(rc, what):
    if rc < 0:
        msg = lib().pfn_last_error_string()
        raise HipExtensionError(f'{what} failed with code {rc}: {msg.decode() if msg else ""}')
    return rc


def stream_ptr(device=None):
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


def require_gpu_tensor(t, name):
    if not t.is_cuda:
        raise HipExtensionError(
            f'{name} lives on {t.device}: the PFN hot path only runs on an MI355X through libpfn_hip.so; '
            f'move the model and data to a cuda device (there is no CPU fallback in the product path).')
