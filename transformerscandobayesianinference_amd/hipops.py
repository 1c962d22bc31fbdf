"""Tensor-level wrappers around the C-ABI entry points that take plain buffers (include/pfn_hip.h), on the current stream: the single-op entry points of the
transformer stack (`pfn_op_*`: one kernel launch per call; the per-kernel parity tests tests/test_gpu_ops.py, bench.py's kernel table, tools/) and the
studies' entry points with their tensor checks -- the GP hyper-parameter fit, NUTS, the BNN's potential, SVI and SVGD step loops, the tabular study's windows,
AUC counts, kNN, logistic-regression and GP-classifier grid searches, the stroke prior and the Omniglot episode loader -- which the study modules (mcmc.py, tabular.py, priors/) build on."""
import collections
import ctypes
import math

import torch

from transformerscandobayesianinference_amd import _hip

TDT = {_hip.PREC_BF16: torch.bfloat16, _hip.PREC_F32: torch.float32, _hip.PREC_FP16: torch.float16}
PREC_OF = {v: k for k, v in TDT.items()}      # operand precision of a tensor's dtype
MANGLED_OPERAND = {_hip.PREC_BF16: 'DF16b', _hip.PREC_FP16: 'DF16_', _hip.PREC_F32: 'f'}      # Itanium mangling of the kernels' operand-type template argument


def sp():
    return _hip.stream_ptr()


def gemm_nt(A, B, flags, prec, bias=None, aux=None, resid=None, out_f32=None, out_t=None, out2_t=None):
    M, K = A.shape
    N = B.shape[0]
    p = _hip.ptr
    ld = lambda t: 0 if t is None else t.stride(0)
    _hip.check(_hip.lib().pfn_op_gemm_nt(p(A), A.stride(0), p(B), B.stride(0), M, N, K, flags, p(bias), p(aux), ld(aux),
                                         p(resid), ld(resid), p(out_f32), ld(out_f32), p(out_t), ld(out_t), p(out2_t), ld(out2_t),
                                         prec, sp()), 'pfn_op_gemm_nt')


def gemm_tn(A, B, C, prec, atomic=1):
    M, P = A.shape
    Q = B.shape[1]
    _hip.check(_hip.lib().pfn_op_gemm_tn(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), C.data_ptr(), C.stride(0), M, P, Q,
                                         atomic, prec, sp()), 'pfn_op_gemm_tn')


def gemm_tn_group(problems, splits=0):
    """problems: list of (A[M,P], B[M,Q], C[P,Q], colsum[P] or None), all operands of ONE 16-bit dtype (bf16 / fp16) with the same M."""
    import ctypes
    n = len(problems)
    M = problems[0][0].shape[0]
    VP, L, I = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int32 * n
    A = VP(*[p[0].data_ptr() for p in problems]); lda = L(*[p[0].stride(0) for p in problems])
    B = VP(*[p[1].data_ptr() for p in problems]); ldb = L(*[p[1].stride(0) for p in problems])
    C = VP(*[p[2].data_ptr() for p in problems]); ldc = L(*[p[2].stride(0) for p in problems])
    P = I(*[p[0].shape[1] for p in problems]); Q = I(*[p[1].shape[1] for p in problems])
    cs = VP(*[(p[3].data_ptr() if p[3] is not None else None) for p in problems])
    _hip.check(_hip.lib().pfn_op_gemm_tn_group(n, A, lda, B, ldb, C, ldc, P, Q, cs, M, splits, PREC_OF[problems[0][0].dtype], sp()), 'pfn_op_gemm_tn_group')


SUMS_16BIT = 256      # include/pfn_hip.h PFN_OP_SUMS_16BIT


def gemm_ln(A, B, bias, gamma, beta, eps, resid=None, prev=None, out=None, sums16=False):
    """prev = (ry, rmean, rrstd, rgamma, rbeta) when the residual is the previous LayerNorm's (recomputed) output.
    out = (y[M+2,N], x_t, mean, rstd) pre-allocated buffers (timing loops).
    sums16 (fp16 operands): y leaves -- and prev's ry arrives -- in operand precision (PFN_OP_SUMS_16BIT: what the stack does for fp16 models)."""
    M, K = A.shape
    N = B.shape[0]
    dev = A.device
    if out is None:
        y = torch.full((M + 2, N), float('nan'), dtype=A.dtype if sums16 else torch.float32, device=dev)
        x_t = torch.empty(M, N, dtype=A.dtype, device=dev)
        mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
    else:
        y, x_t, mean, rstd = out
    p = _hip.ptr
    pv = prev if prev is not None else (None,) * 5
    assert y.dtype == (A.dtype if sums16 else torch.float32) and (pv[0] is None or pv[0].dtype == y.dtype)
    _hip.check(_hip.lib().pfn_op_gemm_ln(p(A), A.stride(0), p(B), B.stride(0), M, N, K, p(bias), p(resid), p(pv[0]), p(pv[1]), p(pv[2]), p(pv[3]), p(pv[4]),
                                         p(gamma), p(beta), eps, p(y), p(mean), p(rstd), p(x_t), PREC_OF[A.dtype] | (SUMS_16BIT if sums16 else 0), sp()), 'pfn_op_gemm_ln')
    if out is None:
        assert torch.isnan(y[M:]).all()
    return y[:M], x_t, mean, rstd


def attention_fwd(qkv, H, sep, prec, q_begin=0, out=None, p_drop=0.0, drop_seed=0):
    """q_begin > 0: the queries below it (rounded down to a multiple of 256) are skipped -- their ctx / lse rows keep the NaN fill
    (or whatever `out` = (ctx, lse) held: timing loops pass buffers so that no fill kernel runs between the launches).
    p_drop > 0 (tests): dropout on the probabilities with the site seed drop_seed (pfn_op_attention_fwd_dropout; not with q_begin)."""
    B, S, E3 = qkv.shape
    E = E3 // 3
    if p_drop:
        if q_begin:
            raise _hip.HipExtensionError('attention_fwd: no entry point combines q_begin with dropout')
        ctx = torch.full((B, S, E), float('nan'), dtype=qkv.dtype, device=qkv.device)      # (tests only: a row the kernel skipped shows)
        lse = torch.full((B, H, S), float('nan'), dtype=torch.float32, device=qkv.device)
        _hip.check(_hip.lib().pfn_op_attention_fwd_dropout(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), B, S, E, H, sep, prec, p_drop, drop_seed, sp()), 'attn fwd')
        return ctx, lse
    if q_begin:
        if out is not None:
            ctx, lse = out
        else:
            ctx = torch.full((B, S, E), float('nan'), dtype=qkv.dtype, device=qkv.device)
            lse = torch.full((B, H, S), float('nan'), dtype=torch.float32, device=qkv.device)
        _hip.check(_hip.lib().pfn_op_attention_fwd_from(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), B, S, E, H, sep, q_begin, prec, sp()), 'attn fwd')
        return ctx, lse
    ctx = torch.empty(B, S, E, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=qkv.device)
    _hip.check(_hip.lib().pfn_op_attention_fwd(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), B, S, E, H, sep, prec, sp()), 'attn fwd')
    return ctx, lse


def gather_rows(src, sep, out=None):
    """[B, S, W] -> the compact test rows [(S - sep) * B, W] in the decoder's order (row (t - sep) * B + b)."""
    B, S, W = src.shape
    dst = out if out is not None else torch.empty((S - sep) * B, W, dtype=src.dtype, device=src.device)
    _hip.check(_hip.lib().pfn_op_gather_rows(src.data_ptr(), dst.data_ptr(), B, S, W * src.element_size(), sep, sp()), 'gather rows')
    return dst


def scatter_rows(src, B, S, sep, zero_from, fill=float('nan'), out=None):
    """the inverse: rows >= sep from the compact rows, zeros in [zero_from, sep), `fill` (untouched) below"""
    W = src.shape[1]
    dst = out if out is not None else torch.full((B, S, W), fill, dtype=src.dtype, device=src.device)
    _hip.check(_hip.lib().pfn_op_scatter_rows(src.data_ptr(), dst.data_ptr(), B, S, W * src.element_size(), sep, zero_from, sp()), 'scatter rows')
    return dst


def gemm_lnbwd(A, B, aux, y, mean, rstd, gamma, out=None):
    """dx_t, dgamma, dbeta of  v = A . B^T + aux  pushed back through the LayerNorm (y, mean, rstd, gamma)  (pfn_op_gemm_lnbwd).
    y in operand precision (fp16) selects PFN_OP_SUMS_16BIT."""
    M, K = A.shape
    N = B.shape[0]
    if out is None:
        out = (torch.full((M + 2, N), float('nan'), dtype=A.dtype, device=A.device), torch.zeros(N, device=A.device), torch.zeros(N, device=A.device))
    dx_t, dgamma, dbeta = out
    p = _hip.ptr
    _hip.check(_hip.lib().pfn_op_gemm_lnbwd(p(A), A.stride(0), p(B), B.stride(0), M, N, K, p(aux), p(y), p(mean), p(rstd), p(gamma),
                                            p(dx_t), p(dgamma), p(dbeta), PREC_OF[A.dtype] | (SUMS_16BIT if y.dtype == A.dtype else 0), sp()), 'pfn_op_gemm_lnbwd')
    return dx_t, dgamma, dbeta


# (name, rocprofv3 kernel name, `parts` bit, algorithmic product units, executed product units) of every launch of the attention
# backward; one unit = one [S x keys x head-dim] product over all heads (the backward's algorithmic work is 4: dV, dP, dK, dQ;
# it executes 5, the forward's S being recomputed once)
ATTENTION_BWD_PARTS = [
    # (rocprofv3 prints these kernels by their mangled names: its demangler does not know the __bf16 template argument)
    ('attn_bwd: delta = rowsum(dO * O)', '_ZN3pfn17attn_delta_kernelI{T}EEvNS_8AttnArgsEi', 1, 0.0, 0.0),
    ('attn_bwd: key-block pass (S, dP, dV, dK products; stores dS^T)', '_ZN3pfn18attn_bwd_kv_kernelI{T}Li{D}ELi0ELb0', 2, 3.0, 4.0),
    ('attn_bwd: query-block pass (dQ = dS K from the stored dS^T)', '_ZN3pfn18attn_bwd_dq_kernelI{T}Li{D}ELb0', 4, 1.0, 1.0),      # (...ELb0: the variant without the dropout masks)
]
ATTENTION_FWD_ROCPROF = '_ZN3pfn15attn_fwd_kernelI{T}Li{D}ELb0'
# (round 2: head dim 256 ran the key-block pass as two launches with one more S product -- {256: 5.0}; round 3: one pass everywhere)
ATTENTION_BWD_KV_EXECUTED_UNITS = {}
_bwd_scratch = {}


def attention_bwd(qkv, ctx, lse, dctx, H, sep, prec, parts=0, q_begin=0, p_drop=0.0, drop_seed=0):
    """parts = 0: the whole backward (outputs start as NaN so a skipped element shows).  parts != 0 (timing): only the selected
    launches, into cached scratch buffers (the skipped launches' products must exist from an earlier full call with the same
    shapes for the numbers to mean anything).  p_drop > 0 (tests): the forward's dropout (pfn_op_attention_bwd_dropout; not with q_begin)."""
    B, S, E3 = qkv.shape
    E = E3 // 3
    key = (tuple(qkv.shape), qkv.dtype, qkv.device, H)
    if key not in _bwd_scratch:
        _bwd_scratch.clear()
        ws = _hip.check(_hip.lib().pfn_op_attention_bwd_ws_bytes(B, S, H, prec), 'attn bwd ws')
        _bwd_scratch[key] = (torch.zeros_like(qkv), torch.zeros(2, B, H, S, dtype=torch.float32, device=qkv.device),     # [delta | lse in log2 units]
                             torch.empty(ws, dtype=torch.uint8, device=qkv.device))
    dqkv, delta, ds = _bwd_scratch[key]
    if not parts:
        dqkv = torch.full_like(qkv, float('nan'))
        ds.fill_(0xff)                                 # NaN patterns: a dS^T element the key-block pass skipped would show in dQ
    if p_drop:
        if q_begin:
            raise _hip.HipExtensionError('attention_bwd: no entry point combines q_begin with dropout')
        _hip.check(_hip.lib().pfn_op_attention_bwd_dropout(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), dctx.data_ptr(), dqkv.data_ptr(),
                                                           delta.data_ptr(), ds.data_ptr(), B, S, E, H, sep, prec, parts, p_drop, drop_seed, sp()), 'attn bwd')
        return dqkv
    if q_begin:
        _hip.check(_hip.lib().pfn_op_attention_bwd_from(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), dctx.data_ptr(), dqkv.data_ptr(),
                                                        delta.data_ptr(), ds.data_ptr(), B, S, E, H, sep, q_begin, prec, parts, sp()), 'attn bwd')
        return dqkv
    _hip.check(_hip.lib().pfn_op_attention_bwd(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), dctx.data_ptr(), dqkv.data_ptr(),
                                               delta.data_ptr(), ds.data_ptr(), B, S, E, H, sep, prec, parts, sp()), 'attn bwd')
    return dqkv


def layernorm_fwd(x, gamma, beta, eps, prec):
    rows, E = x.shape
    y32 = torch.empty_like(x)
    yt = torch.empty(rows, E, dtype=TDT[prec], device=x.device)
    mean = torch.empty(rows, device=x.device)
    rstd = torch.empty(rows, device=x.device)
    _hip.check(_hip.lib().pfn_op_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y32.data_ptr(), yt.data_ptr(),
                                               mean.data_ptr(), rstd.data_ptr(), rows, E, eps, prec, sp()), 'ln fwd')
    return y32, yt, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, prec, want_f32=True):
    """dy: f32, or the operand dtype of `prec` (the form the backward schedule uses; then usually want_f32=False)."""
    rows, E = x.shape
    dy_is_t = int(dy.dtype != torch.float32)
    dx32 = torch.empty_like(x) if want_f32 else None
    dxt = torch.empty(rows, E, dtype=TDT[prec], device=x.device)
    dg = torch.zeros(E, device=x.device)
    db = torch.zeros(E, device=x.device)
    dbias = torch.zeros(E, device=x.device)
    _hip.check(_hip.lib().pfn_op_layernorm_bwd(dy.data_ptr(), dy_is_t, x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                               dx32.data_ptr() if want_f32 else 0, dxt.data_ptr(), dg.data_ptr(), db.data_ptr(), dbias.data_ptr(),
                                               rows, E, prec, sp()), 'ln bwd')
    return dx32, dxt, dg, db, dbias


def qkv_projection(x, w_in, b_in, sep, center=True, sep_of=None):
    """x [B, S, E], w_in [3E, E] (one 16-bit dtype), b_in [3E] f32 -> (qkv [B, S, 3E], kshift [B, E] f32): the encoder layer's packed projection with the keys of every
    dataset centred on a sample mean of its train rows (pfn_op_qkv_projection; center=False: the plain projection)."""
    B, S, E = x.shape
    qkv = torch.full((B, S, 3 * E), float('nan'), dtype=x.dtype, device=x.device)
    ks = torch.full((B, E), float('nan'), dtype=torch.float32, device=x.device)
    _hip.check(_hip.lib().pfn_op_qkv_projection(x.data_ptr(), w_in.data_ptr(), b_in.data_ptr(), qkv.data_ptr(), ks.data_ptr(), B, S, E, sep,
                                                _hip.ptr(sep_of), int(center), PREC_OF[x.dtype], sp()), 'pfn_op_qkv_projection')
    return qkv, ks


# ---- GP hyper-parameter fit (csrc/gp_fit.hip; include/pfn_hip.h "GP hyper-parameter fit") ----
def gp_fit_workspace(P, S, device):
    """The caller-owned workspace of pfn_gp_mll_grad / pfn_gp_fit_predict for P problems of S rows; reusable across calls of the same shape."""
    return torch.empty(int(_hip.lib().pfn_gp_fit_workspace_bytes(P, S)), dtype=torch.uint8, device=device)


def _gp_fit_inputs(x, y, theta, prior, n_of):
    _hip.require_gpu_tensor(x, 'x')
    P, S, F = x.shape
    assert S % 4 == 0, 'S must be a multiple of 4 (pad and mask the padding through n_of)'
    assert y.shape == (P, S) and theta.shape == (P, F + 3) and prior.shape == (8,)
    for t in (x, y, theta, prior):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.device == x.device
    if n_of is not None:
        assert n_of.dtype == torch.int32 and n_of.shape == (P,) and n_of.is_contiguous() and n_of.device == x.device
    return P, S, F


def gp_mll_grad(x, y, theta, prior, kernel, n_of=None, flags=0, want_grad=True, ws=None):
    """J(theta) and dJ/dtheta of the MAP-II objective per problem (pfn_gp_mll_grad).  x [P,S,F], y [P,S], theta [P,F+3], prior [8], n_of [P] int32 or None:
    contiguous f32 / int32 tensors on the GPU.  Returns (value [P], grad [P,F+3] or None, info [P])."""
    P, S, F = _gp_fit_inputs(x, y, theta, prior, n_of)
    ws = gp_fit_workspace(P, S, x.device) if ws is None else ws
    value = torch.empty(P, dtype=torch.float32, device=x.device)
    grad = torch.empty(P, F + 3, dtype=torch.float32, device=x.device) if want_grad else None
    info = torch.empty(P, dtype=torch.int32, device=x.device)
    _hip.check(_hip.lib().pfn_gp_mll_grad(x.data_ptr(), y.data_ptr(), _hip.ptr(n_of), theta.data_ptr(), prior.data_ptr(), P, S, F, int(kernel), int(flags),
                                          ws.data_ptr(), ws.numel(), value.data_ptr(), _hip.ptr(grad), info.data_ptr(), _hip.stream_ptr(x.device)), 'pfn_gp_mll_grad')
    return value, grad, info


def gp_fit_predict(x, y, theta, prior, kernel, x_test, n_of=None, ws=None):
    """Posterior of the GP with parameters theta at x_test [P,m,F] (pfn_gp_fit_predict).  Returns (mean [P,m], var [P,m] with observation noise, info [P])."""
    P, S, F = _gp_fit_inputs(x, y, theta, prior, n_of)
    m = x_test.shape[1]
    assert x_test.shape == (P, m, F) and x_test.dtype == torch.float32 and x_test.is_contiguous() and x_test.device == x.device
    ws = gp_fit_workspace(P, S, x.device) if ws is None else ws
    mean = torch.empty(P, m, dtype=torch.float32, device=x.device)
    var = torch.empty(P, m, dtype=torch.float32, device=x.device)
    info = torch.empty(P, dtype=torch.int32, device=x.device)
    _hip.check(_hip.lib().pfn_gp_fit_predict(x.data_ptr(), y.data_ptr(), _hip.ptr(n_of), theta.data_ptr(), prior.data_ptr(), P, S, F, int(kernel), x_test.data_ptr(), m,
                                             ws.data_ptr(), ws.numel(), mean.data_ptr(), var.data_ptr(), info.data_ptr(), _hip.stream_ptr(x.device)), 'pfn_gp_fit_predict')
    return mean, var, info


# ---- batched NUTS (csrc/gp_mcmc.hip; include/pfn_hip.h "batched NUTS") ----
def nuts_workspace(C, D, max_tree_depth, device):
    """The caller-owned workspace of pfn_nuts_init / pfn_nuts_advance for C chains of D coordinates."""
    nbytes = int(_hip.lib().pfn_nuts_workspace_bytes(C, D, max_tree_depth))
    if nbytes < 0:
        raise _hip.HipExtensionError(f'pfn_nuts_workspace_bytes({C}, {D}, {max_tree_depth}): need C >= 1, 1 <= D <= 128, 1 <= max_tree_depth <= 10')
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _nuts_f32(t, shape, name, device):
    assert t.dtype == torch.float32 and t.is_contiguous() and t.device == device and tuple(t.shape) == tuple(shape), f'{name}: want contiguous f32 {tuple(shape)} on {device}'


def nuts_init(ws, theta0, D, max_tree_depth, num_warmup, num_samples, seed, trial, done_count, flags=0, window_start=0, window_ends=(), step_size=0.1, target_accept=0.8,
              chain_ids=None, inv_mass=None):
    """pfn_nuts_init: lays the state of C = theta0.shape[0] chains out in `ws` and writes the start points to trial [C, ld] (ld = theta0.shape[1] >= D)."""
    _hip.require_gpu_tensor(theta0, 'theta0')
    C, ld = theta0.shape
    dev = theta0.device
    _nuts_f32(theta0, (C, ld), 'theta0', dev)
    _nuts_f32(trial, (C, ld), 'trial', dev)
    assert done_count.dtype == torch.int32 and done_count.numel() == 1 and done_count.device == dev
    if chain_ids is not None:
        assert chain_ids.dtype == torch.int64 and chain_ids.shape == (C,) and chain_ids.is_contiguous() and chain_ids.device == dev
    if inv_mass is not None:
        _nuts_f32(inv_mass, (C, D), 'inv_mass', dev)
    ends = (ctypes.c_int32 * max(1, len(window_ends)))(*[int(e) for e in window_ends])
    _hip.check(_hip.lib().pfn_nuts_init(ws.data_ptr(), ws.numel(), C, int(D), ld, int(max_tree_depth), int(num_warmup), int(num_samples), int(flags),
                                        ctypes.cast(ends, ctypes.c_void_p), len(window_ends), int(window_start), float(step_size), float(target_accept), int(seed) & (2 ** 64 - 1),
                                        _hip.ptr(chain_ids), theta0.data_ptr(), _hip.ptr(inv_mass), trial.data_ptr(), done_count.data_ptr(), _hip.stream_ptr(dev)), 'pfn_nuts_init')


def nuts_advance(ws, D, max_tree_depth, value, grad, trial, samples, stats, done_count, info=None, scale=None, shift=None, warm=None):
    """pfn_nuts_advance: consumes value [C], grad [C, ld] (and info [C] int32) at `trial`, advances every chain by one leapfrog and writes the next trial points;
    samples [C, N, D], stats [C, W+N, 8], warm [C, W, D] receive the rows of the transitions that finished in this call.  N and W are read off the shapes of
    `samples` and `stats` and handed to the kernel, which does nothing unless they are the ones `nuts_init` was given: buffers of another size are never written."""
    C, ld = trial.shape
    dev = trial.device
    _nuts_f32(value, (C,), 'value', dev)
    _nuts_f32(grad, (C, ld), 'grad', dev)
    N = samples.shape[1]
    W = stats.shape[1] - N
    assert N >= 1 and W >= 0, 'samples [C, N, D] and stats [C, W+N, 8]'
    _nuts_f32(samples, (C, N, D), 'samples', dev)
    _nuts_f32(stats, (C, W + N, 8), 'stats', dev)
    if info is not None:
        assert info.dtype == torch.int32 and info.shape == (C,) and info.is_contiguous() and info.device == dev
    if scale is not None:
        _nuts_f32(scale, (C,), 'scale', dev)
    if shift is not None:
        _nuts_f32(shift, (D,), 'shift', dev)
    if warm is not None:
        _nuts_f32(warm, (C, W, D), 'warm', dev)
    _hip.check(_hip.lib().pfn_nuts_advance(ws.data_ptr(), ws.numel(), C, int(D), ld, int(max_tree_depth), W, N, value.data_ptr(), grad.data_ptr(), _hip.ptr(info),
                                           _hip.ptr(scale), _hip.ptr(shift), trial.data_ptr(), samples.data_ptr(), stats.data_ptr(), _hip.ptr(warm), done_count.data_ptr(),
                                           _hip.stream_ptr(dev)), 'pfn_nuts_advance')


def nuts_inv_mass(ws, C, D):
    """The chains' current inverse mass [C, D]: a view of the workspace at PFN_NUTS_INV_MASS_OFFSET."""
    return ws[_hip.NUTS_INV_MASS_OFFSET:_hip.NUTS_INV_MASS_OFFSET + 4 * C * D].view(torch.float32).view(C, D)


# ---- BNN posterior target (csrc/bnn_mcmc.hip; include/pfn_hip.h "BNN posterior target") ----
BNN_ACTIVATIONS = {'identity': 0, 'tanh': 1, 0: 0, 1: 1}


def bnn_num_params(F, H):
    """D = H (F + 3) + 2: W1 [H,F], b1 [H], W2 [2,H], b2 [2]."""
    return int(H) * (int(F) + 3) + 2


def _bnn_f32(x, *tensors):
    """The tensor checks of the bnn_* wrappers, written once: x and every given tensor is f32, contiguous and on x's device."""
    for t in (x,) + tensors:
        assert t.dtype == torch.float32 and t.is_contiguous() and t.device == x.device


def _bnn_n_of(n_of, P, x):
    assert n_of is None or (n_of.dtype == torch.int32 and n_of.shape == (P,) and n_of.is_contiguous() and n_of.device == x.device), 'n_of [P] int32'


def bnn_logp_grad(x, y, theta, H, K=None, n_of=None, activation=0, want_grad=True, value=None, grad=None):
    """Potential and gradient of the two-layer BNN for every chain (pfn_bnn_logp_grad).  x [P,S,F], y [P,S], theta [P K, ld >= D] contiguous f32 on the GPU,
    n_of [P] int32 or None; chain c belongs to problem c // K (K defaults to theta.shape[0] // P).  Returns (value [P K], grad [P K, ld] or None); only the
    first D columns of `grad` are written (a fresh one is zero-filled; a caller-owned one keeps its tail)."""
    _hip.require_gpu_tensor(x, 'x')
    P, S, F = x.shape
    C, ld = theta.shape
    K = C // P if K is None else int(K)
    assert C == P * K and y.shape == (P, S), 'theta [P K, ld], y [P, S]'
    _bnn_f32(x, y, theta)
    _bnn_n_of(n_of, P, x)
    value = torch.empty(C, dtype=torch.float32, device=x.device) if value is None else value
    if want_grad and grad is None:
        grad = torch.zeros(C, ld, dtype=torch.float32, device=x.device)
    if not want_grad:
        grad = None
    assert value.shape == (C,) and (grad is None or grad.shape == (C, ld))
    _bnn_f32(x, value, *(() if grad is None else (grad,)))
    _hip.check(_hip.lib().pfn_bnn_logp_grad(x.data_ptr(), y.data_ptr(), _hip.ptr(n_of), theta.data_ptr(), ld, P, K, S, F, int(H), BNN_ACTIVATIONS[activation],
                                            value.data_ptr(), _hip.ptr(grad), _hip.stream_ptr(x.device)), 'pfn_bnn_logp_grad')
    return value, grad


def bnn_predict(x_test, theta, H, K=None, activation=0):
    """Class-1 probability of every chain at x_test [P,m,F] (pfn_bnn_predict): theta [P K, ld] -> prob1 [P K, m]."""
    _hip.require_gpu_tensor(x_test, 'x_test')
    P, m, F = x_test.shape
    C, ld = theta.shape
    K = C // P if K is None else int(K)
    assert C == P * K, 'theta [P K, ld]'
    _bnn_f32(x_test, theta)
    prob1 = torch.empty(C, m, dtype=torch.float32, device=x_test.device)
    _hip.check(_hip.lib().pfn_bnn_predict(x_test.data_ptr(), theta.data_ptr(), ld, P, K, m, F, int(H), BNN_ACTIVATIONS[activation], prob1.data_ptr(),
                                          _hip.stream_ptr(x_test.device)), 'pfn_bnn_predict')
    return prob1


# ---- SVI on the BNN (csrc/bnn_svi.hip; include/pfn_hip.h "SVI on the BNN") ----
SVI_ROWS = ('loc', 'u', 'm_loc', 'v_loc', 'm_u', 'v_u')      # the rows of a guide's state


def bnn_svi_state(P, F, H, device, loc0=None, init_scale=0.1):
    """The state of P mean-field Gaussian guides at step 0: [P, 6, D] f32 with loc = loc0 ([P, D] or None: zeros), u = softplus^-1(init_scale) (the guide's
    scale is softplus(u)) and zero Adam moments."""
    D = bnn_num_params(F, H)
    assert init_scale > 0
    state = torch.zeros(int(P), 6, D, dtype=torch.float32, device=device)
    if loc0 is not None:
        assert tuple(loc0.shape) == (int(P), D), 'loc0 [P, D]'
        state[:, 0] = loc0.to(device=device, dtype=torch.float32)
    state[:, 1] = math.log(math.expm1(float(init_scale)))
    return state


def bnn_svi_steps(x, y, state, H, num_steps, step0=0, num_particles=1, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=0, n_of=None, activation=0, problem_ids=None,
                  loss=None):
    """`num_steps` steps of SVI (noise -> ELBO gradient -> Adam) on the guides of P problems in one launch (pfn_bnn_svi_steps).  x [P,S,F], y [P,S],
    state [P, 6, ld >= D] contiguous f32 on the GPU (updated in place; bnn_svi_state), n_of [P] int32 or None, problem_ids [P] int64 or None (the noise
    stream of problem p: its index).  The launch covers the absolute steps step0 .. step0 + num_steps - 1.  Returns loss [P, num_steps] (a fresh tensor
    unless given): the ELBO loss of every step before its update."""
    _hip.require_gpu_tensor(x, 'x')
    P, S, F = x.shape
    num_steps, step0, K = int(num_steps), int(step0), int(num_particles)
    assert state.dim() == 3 and state.shape[:2] == (P, 6) and y.shape == (P, S), 'state [P, 6, ld], y [P, S]'
    ld = state.shape[2]
    _bnn_f32(x, y, state)
    _bnn_n_of(n_of, P, x)
    if problem_ids is not None:
        assert problem_ids.dtype == torch.int64 and problem_ids.shape == (P,) and problem_ids.is_contiguous() and problem_ids.device == x.device
    if loss is None:
        loss = torch.empty(P, max(num_steps, 0), dtype=torch.float32, device=x.device)
    assert loss.shape == (P, num_steps)
    _bnn_f32(x, loss)
    _hip.check(_hip.lib().pfn_bnn_svi_steps(x.data_ptr(), y.data_ptr(), _hip.ptr(n_of), state.data_ptr(), ld, P, S, F, int(H), BNN_ACTIVATIONS[activation], K, step0,
                                            num_steps, float(lr), float(betas[0]), float(betas[1]), float(eps), int(seed), _hip.ptr(problem_ids), loss.data_ptr(),
                                            _hip.stream_ptr(x.device)), 'pfn_bnn_svi_steps')
    return loss


# ---- SVGD on the BNN (csrc/bnn_svgd.hip; include/pfn_hip.h "SVGD on the BNN") ----
SVGD_ROWS = ('particles', 'm', 'v')      # the row blocks of a particle state
SVGD_MAX_PARTICLES = 64                  # PFN_BNN_SVGD_MAX_PARTICLES


def bnn_svgd_state(P, N, F, H, device, particles0=None):
    """The state of N Stein particles per problem at step 0: [P, 3, N, D] f32 with the particles particles0 ([P, N, D]) and zero Adam moments.  None leaves
    the particles at zero for the caller to fill: coincident particles have no bandwidth (h = 0) and a step from them is non-finite."""
    D = bnn_num_params(F, H)
    state = torch.zeros(int(P), 3, int(N), D, dtype=torch.float32, device=device)
    if particles0 is not None:
        assert tuple(particles0.shape) == (int(P), int(N), D), 'particles0 [P, N, D]'
        state[:, 0] = particles0.to(device=device, dtype=torch.float32)
    return state


def bnn_svgd_steps(x, y, state, H, num_steps, step0=0, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, bandwidth_factor=1.0, n_of=None, activation=0, potential=None,
                   bandwidth=None):
    """`num_steps` steps of SVGD (grad U -> per-coordinate median bandwidth -> Stein direction -> Adam) on the particles of P problems in one launch
    (pfn_bnn_svgd_steps).  x [P,S,F], y [P,S], state [P, 3, N, ld >= D] contiguous f32 on the GPU (updated in place; bnn_svgd_state), n_of [P] int32 or None.
    The launch covers the absolute steps step0 .. step0 + num_steps - 1.  Returns (potential [P, num_steps], bandwidth [P, ld]) (fresh tensors unless given):
    the mean over particles of U before every step's update, and h of the last step in the first D columns (untouched when num_steps = 0)."""
    _hip.require_gpu_tensor(x, 'x')
    P, S, F = x.shape
    num_steps, step0 = int(num_steps), int(step0)
    assert state.dim() == 4 and state.shape[:2] == (P, 3) and y.shape == (P, S), 'state [P, 3, N, ld], y [P, S]'
    N, ld = state.shape[2], state.shape[3]
    _bnn_f32(x, y, state)
    _bnn_n_of(n_of, P, x)
    if potential is None:
        potential = torch.empty(P, max(num_steps, 0), dtype=torch.float32, device=x.device)
    if bandwidth is None:
        bandwidth = torch.zeros(P, ld, dtype=torch.float32, device=x.device)
    assert potential.shape == (P, num_steps) and bandwidth.shape == (P, ld)
    _bnn_f32(x, potential, bandwidth)
    lib = _hip.lib()
    ws_bytes = int(lib.pfn_bnn_svgd_workspace_bytes(P, N, F, int(H)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes > 0 else None      # negative (bad shapes): the call below names what is wrong
    _hip.check(lib.pfn_bnn_svgd_steps(x.data_ptr(), y.data_ptr(), _hip.ptr(n_of), state.data_ptr(), ld, P, S, F, int(H), BNN_ACTIVATIONS[activation], N, step0,
                                      num_steps, float(lr), float(betas[0]), float(betas[1]), float(eps), float(bandwidth_factor), _hip.ptr(ws), max(ws_bytes, 0),
                                      potential.data_ptr(), bandwidth.data_ptr(), _hip.stream_ptr(x.device)), 'pfn_bnn_svgd_steps')
    return potential, bandwidth


# ---- Tabular study (csrc/tabular.hip; include/pfn_hip.h "Tabular study") ----
TAB_NORM_WITH_TEST, TAB_NORM_TRAIN_ONLY = 0, 1      # PFN_TAB_NORM_*
TAB_MAX_FEATURES = 1024
AUC_MAX_ROWS = 4096
KNN_MAX_K, KNN_MAX_FOLDS = 5, 5
KNN_LIMITS = dict(n=(4, 128), T=(1, 128), F=(1, 128))


def tabular_windows_check(N, F, F_out, W, bptt, sep, rescale, mode, starts):
    """The shape rules of pfn_tabular_windows plus the one the kernel can only answer with NaN columns: every window lies inside the table.  Host only."""
    if mode not in (TAB_NORM_WITH_TEST, TAB_NORM_TRAIN_ONLY):
        raise ValueError(f'unknown mode {mode!r} (TAB_NORM_WITH_TEST, TAB_NORM_TRAIN_ONLY)')
    if not (1 <= F <= TAB_MAX_FEATURES and F_out >= F):
        raise ValueError(f'F {F} outside 1 .. {TAB_MAX_FEATURES} or F_out {F_out} < F')
    if not (N >= 1 and W >= 1 and 1 <= sep <= bptt and (sep < bptt or mode == TAB_NORM_TRAIN_ONLY) and rescale > 0):
        raise ValueError(f'need N {N} >= 1, W {W} >= 1, 1 <= sep {sep} {"<" if mode == TAB_NORM_WITH_TEST else "<="} bptt {bptt}, rescale {rescale} > 0')
    if min(starts) < 0 or max(starts) + bptt > N:
        raise ValueError(f'a window of {bptt} rows starting at {min(starts)} .. {max(starts)} leaves the table of {N} rows')


def tabular_windows(X, y, starts, bptt, sep, F_out=None, rescale=1.0, mode=TAB_NORM_WITH_TEST):
    """Every window of an eval position gathered from the table X [N,F], y [N] and normalised, in one launch (pfn_tabular_windows).  `starts`: the windows'
    first rows, a host sequence or CPU tensor (checked against the table here).  WITH_TEST returns x [sep+1, W T, F_out], y [sep, W T] -- column w T + t is
    window w's train rows and its test row t, normalised over those sep + 1 rows and divided by `rescale`; TRAIN_ONLY returns x [bptt, W, F_out], y [bptt, W]
    normalised by the train rows' statistics."""
    starts = [int(s) for s in (starts.tolist() if torch.is_tensor(starts) else starts)]
    if X.dim() != 2 or y.shape != X.shape[:1]:
        raise ValueError('X [N, F], y [N]')
    N, F = X.shape
    F_out = F if F_out is None else int(F_out)
    bptt, sep, W = int(bptt), int(sep), len(starts)
    tabular_windows_check(N, F, F_out, W, bptt, sep, float(rescale), mode, starts or [0])
    _hip.require_gpu_tensor(X, 'X')
    _bnn_f32(X, y)
    T = bptt - sep
    dev = X.device
    st = torch.tensor(starts, dtype=torch.int32).to(dev)
    if mode == TAB_NORM_WITH_TEST:
        x_out = torch.empty(sep + 1, W * T, F_out, dtype=torch.float32, device=dev)
        y_out = torch.empty(sep, W * T, dtype=torch.float32, device=dev)
    else:
        x_out = torch.empty(bptt, W, F_out, dtype=torch.float32, device=dev)
        y_out = torch.empty(bptt, W, dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().pfn_tabular_windows(X.data_ptr(), y.data_ptr(), st.data_ptr(), N, F, F_out, W, bptt, sep, float(rescale), int(mode), x_out.data_ptr(),
                                              y_out.data_ptr(), _hip.stream_ptr(dev)), 'pfn_tabular_windows')
    return x_out, y_out


def auc_counts(scores, labels):
    """Per column of scores [T,C] / labels [T,C] (positive = label > 0.5): int64 [C,4] = (positives, negatives, pairs won, pairs tied) (pfn_auc_counts)."""
    if scores.dim() != 2 or labels.shape != scores.shape:
        raise ValueError('scores [T, C], labels [T, C]')
    T, C = scores.shape
    if not (1 <= T <= AUC_MAX_ROWS and C >= 1):
        raise ValueError(f'T {T} outside 1 .. {AUC_MAX_ROWS} or C {C} < 1')
    _hip.require_gpu_tensor(scores, 'scores')
    _bnn_f32(scores, labels)
    counts = torch.empty(C, 4, dtype=torch.int64, device=scores.device)
    _hip.check(_hip.lib().pfn_auc_counts(scores.data_ptr(), labels.data_ptr(), T, C, counts.data_ptr(), _hip.stream_ptr(scores.device)), 'pfn_auc_counts')
    return counts


def auc_from_counts(counts):
    """AUC = (2 gt + eq) / (2 P Nn) in f64 on the host, NaN where a column has one class only.  counts [C,4] -> numpy [C]."""
    import numpy as np
    c = counts.cpu().numpy().astype(np.int64).reshape(-1, 4)
    pairs = (c[:, 0] * c[:, 1]).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(pairs > 0, (2 * c[:, 2] + c[:, 3]).astype(np.float64) / (2. * pairs), np.nan)


def _limits_check(prefix, limits, **sizes):
    """The limits of a fold-based launch (KNN_LIMITS, LOGIT_LIMITS, GPC_LIMITS), raised as ValueError in the order given.  Host only."""
    for name, v in sizes.items():
        lo, hi = limits[name]
        if not lo <= v <= hi:
            raise ValueError(f'{prefix}: {name} = {v} outside {lo} .. {hi}')


def _fold_args(check, train, labels, fold, test=None, NC=None, splits=None, also_f32=(), layout='train [P, n, F], labels [P, n], test [P, T, F], fold [P, n]'):
    """What knn_cv, logistic_cv and the gpc_* wrappers check alike, ValueErrors first and the device after: the shapes (`layout` is their message), the launch's
    limits (`check`, with NC where the call has candidates), P >= 1 and splits = (n_splits, most folds) where the call has n_splits, then train on the GPU, train /
    labels / test / `also_f32` f32 and contiguous there, fold int32.  A call without test rows counts as T = 1.  Returns (P, n, T, F)."""
    if train.dim() != 3 or labels.shape != train.shape[:2] or fold.shape != train.shape[:2] or \
            (test is not None and (test.dim() != 3 or test.shape[0] != train.shape[0] or test.shape[2] != train.shape[2])):
        raise ValueError(layout)
    P, n, F = train.shape
    T = 1 if test is None else test.shape[1]
    check(n, T, F, *(() if NC is None else (NC,)))
    if P < 1 or (splits is not None and not 2 <= int(splits[0]) <= splits[1]):
        raise ValueError('P >= 1' if splits is None else f'P >= 1, 2 <= n_splits = {splits[0]} <= {splits[1]}')
    _hip.require_gpu_tensor(train, 'train')
    _bnn_f32(train, labels, *(() if test is None else (test,)), *also_f32)
    assert fold.dtype == torch.int32 and fold.is_contiguous() and fold.device == train.device, 'fold [P, n] int32'
    return P, n, T, F


def knn_cv_check(n, T, F):
    _limits_check('knn_cv', KNN_LIMITS, n=n, T=T, F=F)


def knn_cv(train, labels, test, fold):
    """Neighbour lists for the kNN grid search of every problem in one launch (pfn_knn_cv): train [P,n,F], labels [P,n], test [P,T,F] f32 and fold [P,n] int32
    (the CV test fold of each train row, 0 .. 4) on the GPU.  Returns int32 (cv_correct [P,5,5], test_pos [P,T,5], test_nbr [P,T,5])."""
    P, n, T, F = _fold_args(knn_cv_check, train, labels, fold, test)
    dev = train.device
    cv_correct = torch.empty(P, KNN_MAX_K, KNN_MAX_FOLDS, dtype=torch.int32, device=dev)
    test_pos = torch.empty(P, T, KNN_MAX_K, dtype=torch.int32, device=dev)
    test_nbr = torch.empty(P, T, KNN_MAX_K, dtype=torch.int32, device=dev)
    _hip.check(_hip.lib().pfn_knn_cv(train.data_ptr(), labels.data_ptr(), test.data_ptr(), fold.data_ptr(), P, n, T, F, cv_correct.data_ptr(), test_pos.data_ptr(),
                                     test_nbr.data_ptr(), _hip.stream_ptr(dev)), 'pfn_knn_cv')
    return cv_correct, test_pos, test_nbr


# ---- Logistic regression with its grid search (csrc/logistic.hip; include/pfn_hip.h "Logistic regression") ----
LOGIT_NONE, LOGIT_L1, LOGIT_L2, LOGIT_FIT_INTERCEPT = 0, 1, 2, 4      # PFN_LOGIT_*: cand_kind = penalty code | fit-intercept bit
LOGIT_PENALTIES = {'none': LOGIT_NONE, None: LOGIT_NONE, 'l1': LOGIT_L1, 'l2': LOGIT_L2}
LOGIT_FOLDS, LOGIT_SLOTS, LOGIT_MAX_CANDIDATES = 5, 6, 64
LOGIT_UNUSED, LOGIT_CONVERGED, LOGIT_STALLED, LOGIT_CAPPED, LOGIT_ONE_CLASS, LOGIT_NONFINITE = 0, 1, 2, 3, 4, 5      # status[..., 0]
LOGIT_LIMITS = dict(n=(4, 128), T=(1, 128), F=(1, 128), NC=(1, LOGIT_MAX_CANDIDATES))


def logistic_cv_check(n, T, F, NC=1):
    _limits_check('logistic_cv', LOGIT_LIMITS, n=n, T=T, F=F, NC=NC)


def logistic_cv(train, labels, test, fold, n_splits, cand_C, cand_kind, return_coef=False):
    """Every fit of a logistic-regression grid search in one launch (pfn_logistic_cv): train [P,n,F], labels [P,n], test [P,T,F] f32 and fold [P,n] int32 (the
    CV test fold of each train row) on the GPU; cand_C / cand_kind: the NC candidates' C and penalty code | LOGIT_FIT_INTERCEPT (host sequences).  Slot
    s < n_splits of a candidate is the fit without fold s, slot n_splits the refit on all rows.  Returns (cv_correct [P,NC,5] int32, test_z [P,NC,T] f32,
    status [P,NC,6,2] int32 = (LOGIT_* exit reason, iterations), coef [P,NC,6,F+1] f32 or None)."""
    cand_C, cand_kind = [float(v) for v in cand_C], [int(v) for v in cand_kind]
    NC = len(cand_C)
    if len(cand_kind) != NC or any((k & 3) == 3 or not 0 <= k < 8 for k in cand_kind) or not all(v > 0 for v in cand_C):
        raise ValueError('cand_C [NC] > 0, cand_kind [NC] = LOGIT_NONE / LOGIT_L1 / LOGIT_L2, optionally | LOGIT_FIT_INTERCEPT')
    P, n, T, F = _fold_args(logistic_cv_check, train, labels, fold, test, NC=NC, splits=(n_splits, LOGIT_FOLDS))
    dev = train.device
    c_dev = torch.tensor(cand_C, dtype=torch.float32).to(dev)
    k_dev = torch.tensor(cand_kind, dtype=torch.int32).to(dev)
    cv_correct = torch.empty(P, NC, LOGIT_FOLDS, dtype=torch.int32, device=dev)
    test_z = torch.empty(P, NC, T, dtype=torch.float32, device=dev)
    status = torch.empty(P, NC, LOGIT_SLOTS, 2, dtype=torch.int32, device=dev)
    coef = torch.empty(P, NC, LOGIT_SLOTS, F + 1, dtype=torch.float32, device=dev) if return_coef else None
    _hip.check(_hip.lib().pfn_logistic_cv(train.data_ptr(), labels.data_ptr(), test.data_ptr(), fold.data_ptr(), c_dev.data_ptr(), k_dev.data_ptr(), P, n, T, F, NC,
                                          int(n_splits), cv_correct.data_ptr(), test_z.data_ptr(), status.data_ptr(), _hip.ptr(coef), _hip.stream_ptr(dev)),
               'pfn_logistic_cv')
    return cv_correct, test_z, status, coef


# ---- BNN classifier with its grid search (csrc/bnn_cv.hip; include/pfn_hip.h "BNN classifier with its grid search") ----
BNN_CV_FOLDS, BNN_CV_SLOTS, BNN_CV_MAX_CANDIDATES = 5, 6, 64      # PFN_BNN_CV_*
BNN_CV_UNUSED, BNN_CV_DONE, BNN_CV_NONFINITE = 0, 1, 2            # status
BNN_CV_LIMITS = dict(n=(4, 128), T=(1, 128), F=(1, 128), NC=(1, BNN_CV_MAX_CANDIDATES), H=(1, 64))
BnnCvOut = collections.namedtuple('BnnCvOut', 'loss cv_prob test_prob cv_draw test_draw status')


def bnn_cv_check(n, T, F, cand_H):
    """The limits of a pfn_bnn_cv launch, raised as ValueError before any launch.  cand_H: the candidates' widths.  Host only."""
    cand_H = [int(h) for h in cand_H]
    _limits_check('bnn_cv', BNN_CV_LIMITS, n=n, T=T, F=F, NC=len(cand_H))
    for h in cand_H:
        _limits_check('bnn_cv', BNN_CV_LIMITS, H=h)


def bnn_cv_state(P, cand_H, F, device, loc0=None, init_scale=0.1):
    """The state of every fit of a grid search at step 0: [P, NC, 6 slots, 6 rows, ld] f32 with ld the largest candidate's D; loc = loc0 ([P, NC, 6, ld] or None:
    zeros; a candidate's columns beyond its own D are never read), u = softplus^-1(init_scale) and zero Adam moments, as bnn_svi_state."""
    cand_H = [int(h) for h in cand_H]
    ld = max(bnn_num_params(F, h) for h in cand_H)
    assert init_scale > 0
    state = torch.zeros(int(P), len(cand_H), BNN_CV_SLOTS, 6, ld, dtype=torch.float32, device=device)
    if loc0 is not None:
        assert tuple(loc0.shape) == (int(P), len(cand_H), BNN_CV_SLOTS, ld), 'loc0 [P, NC, 6, ld]'
        state[:, :, :, 0] = loc0.to(device=device, dtype=torch.float32)
    state[:, :, :, 1] = math.log(math.expm1(float(init_scale)))
    return state


def bnn_cv(train, labels, test, fold, n_splits, cand_H, cand_lr, state, num_steps, step0=0, num_pred_samples=0, seed=0, problem_ids=None, want_loss=False,
           sample_obs=False, betas=(0.9, 0.999), eps=1e-8):
    """The SVI steps and the predictive of every fit of a BNN grid search in one launch (pfn_bnn_cv): train [P,n,F], labels [P,n], test [P,T,F] f32 and fold [P,n]
    int32 on the GPU; cand_H / cand_lr: the NC candidates' widths and learning rates (host sequences); state [P,NC,6,6,ld] f32 on the GPU, updated in place
    (bnn_cv_state).  Slot s < n_splits of a candidate is the fit without fold s, slot n_splits the refit on all rows.  The launch covers the absolute steps
    step0 .. step0 + num_steps - 1 and then, with num_pred_samples > 0, the predictive.  Returns BnnCvOut(loss [P,NC,6,num_steps] with want_loss (NaN in the unused slots), cv_prob [P,NC,n]
    (written at the held-out rows of the slots in use; NaN elsewhere) and test_prob [P,NC,T] with num_pred_samples > 0, cv_draw / test_draw of the same shapes
    with sample_obs, status [P,NC,6] int32); what was not asked for is None."""
    import numpy as np
    cand_H, cand_lr = [int(h) for h in cand_H], [float(v) for v in cand_lr]
    NC = len(cand_H)
    if len(cand_lr) != NC or not all(math.isfinite(v) and v >= 0 for v in cand_lr):
        raise ValueError('cand_H [NC], cand_lr [NC] finite and >= 0')
    num_steps, step0, S = int(num_steps), int(step0), int(num_pred_samples)
    P, n, T, F = _fold_args(lambda n, T, F, NC: bnn_cv_check(n, T, F, cand_H), train, labels, fold, test, NC=NC, splits=(n_splits, BNN_CV_FOLDS), also_f32=(state,))
    if not (0 <= step0 <= 1 << 40 and num_steps >= 0 and 0 <= S <= 1 << 20):
        raise ValueError('0 <= step0 <= 2^40, num_steps >= 0, 0 <= num_pred_samples <= 2^20')
    ld = state.shape[-1]
    if tuple(state.shape) != (P, NC, BNN_CV_SLOTS, 6, ld) or ld < max(bnn_num_params(F, h) for h in cand_H):
        raise ValueError('state [P, NC, 6, 6, ld] with ld >= the largest D')
    dev = train.device
    if problem_ids is not None:
        assert problem_ids.dtype == torch.int64 and problem_ids.shape == (P,) and problem_ids.is_contiguous() and problem_ids.device == dev
    new = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=dev)
    loss = new(P, NC, BNN_CV_SLOTS, num_steps) if want_loss else None      # (the unused slots stay NaN)
    cv_prob, test_prob = (new(P, NC, n), new(P, NC, T)) if S > 0 else (None, None)
    cv_draw, test_draw = (new(P, NC, n), new(P, NC, T)) if S > 0 and sample_obs else (None, None)
    status = torch.zeros(P, NC, BNN_CV_SLOTS, dtype=torch.int32, device=dev)
    h_host, lr_host = np.asarray(cand_H, dtype=np.int32), np.asarray(cand_lr, dtype=np.float32)      # read before the call returns
    _hip.check(_hip.lib().pfn_bnn_cv(train.data_ptr(), labels.data_ptr(), test.data_ptr(), fold.data_ptr(), h_host.ctypes.data, lr_host.ctypes.data, P, n, T, F, NC,
                                     int(n_splits), state.data_ptr(), ld, step0, num_steps, float(betas[0]), float(betas[1]), float(eps), S, int(seed),
                                     _hip.ptr(problem_ids), _hip.ptr(loss), _hip.ptr(cv_prob), _hip.ptr(test_prob), _hip.ptr(cv_draw), _hip.ptr(test_draw),
                                     status.data_ptr(), _hip.stream_ptr(dev)), 'pfn_bnn_cv')
    return BnnCvOut(loss, cv_prob, test_prob, cv_draw, test_draw, status)


# ---- Gradient-boosted trees with their grid search (csrc/xgb_cv.hip; include/pfn_hip.h "Gradient-boosted trees with their grid search") ----
XGB_CV_FOLDS, XGB_CV_SLOTS, XGB_CV_MAX_CANDIDATES, XGB_CV_MAX_DEPTH, XGB_CV_MAX_ROUNDS = 5, 6, 64, 2, 4096      # PFN_XGB_CV_*
XGB_CV_UNUSED, XGB_CV_DONE, XGB_CV_NONFINITE = 0, 1, 2            # status
XGB_CV_LIMITS = dict(n=(4, 128), T=(1, 128), F=(1, 128), NC=(1, XGB_CV_MAX_CANDIDATES), max_depth=(1, XGB_CV_MAX_DEPTH), num_rounds=(0, XGB_CV_MAX_ROUNDS))
XgbCvOut = collections.namedtuple('XgbCvOut', 'cv_margin test_margin status tree_feature tree_threshold tree_leaf')


def xgb_cv_check(n, T, F, cand_depth, num_rounds=0):
    """The limits of a pfn_xgb_cv launch, raised as ValueError before any launch.  cand_depth: the candidates' max_depth.  Host only."""
    cand_depth = [int(d) for d in cand_depth]
    _limits_check('xgb_cv', XGB_CV_LIMITS, n=n, T=T, F=F, NC=len(cand_depth), num_rounds=int(num_rounds))
    for d in cand_depth:
        _limits_check('xgb_cv', XGB_CV_LIMITS, max_depth=d)


def xgb_cv(train, labels, test, fold, n_splits, cand_depth, cand_lr, cand_mcw, cand_subsample, cand_colsample, num_rounds, seed=0, problem_ids=None,
           want_trees=False, cand_ids=None):
    """Every boosting round of every fit of a gradient-boosting grid search in one launch (pfn_xgb_cv, after a small launch that sorts the columns): train [P,n,F],
    labels [P,n], test [P,T,F] f32 and fold [P,n] int32 on the GPU; cand_*: the NC candidates' max_depth, learning_rate, min_child_weight, subsample and
    colsample_bytree (host sequences), cand_ids their ids in the noise addressing (None: 0 .. NC-1).  Slot s < n_splits of a candidate is the fit without fold
    s, slot n_splits the refit on all rows.  Returns XgbCvOut(cv_margin [P,NC,n] (written at the held-out rows of the slots in use; NaN elsewhere), test_margin
    [P,NC,T], status [P,NC,6] int32, and with want_trees tree_feature int32 / tree_threshold f32 [P,NC,6,num_rounds,3] and tree_leaf [P,NC,6,num_rounds,4], else
    None)."""
    import numpy as np
    cand_depth, cand_lr = [int(d) for d in cand_depth], [float(v) for v in cand_lr]
    cand_mcw, cand_subsample, cand_colsample = ([float(v) for v in seq] for seq in (cand_mcw, cand_subsample, cand_colsample))
    NC, num_rounds = len(cand_depth), int(num_rounds)
    cand_ids = list(range(NC)) if cand_ids is None else [int(v) for v in cand_ids]
    if not all(len(seq) == NC for seq in (cand_lr, cand_mcw, cand_subsample, cand_colsample, cand_ids)) or \
            not all(math.isfinite(v) and v > 0 for v in cand_lr) or not all(math.isfinite(v) and v >= 0 for v in cand_mcw) or \
            not all(0 < v <= 1 for v in cand_subsample + cand_colsample) or not all(0 <= v < XGB_CV_MAX_CANDIDATES for v in cand_ids):
        raise ValueError('cand_depth, cand_lr > 0, cand_mcw >= 0, cand_subsample and cand_colsample in (0, 1], cand_ids in 0 .. 63: [NC] each, all finite')
    P, n, T, F = _fold_args(lambda n, T, F, NC: xgb_cv_check(n, T, F, cand_depth, num_rounds), train, labels, fold, test, NC=NC, splits=(n_splits, XGB_CV_FOLDS))
    dev = train.device
    if problem_ids is not None:
        assert problem_ids.dtype == torch.int64 and problem_ids.shape == (P,) and problem_ids.is_contiguous() and problem_ids.device == dev
    new = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=dev)
    cv_margin, test_margin = new(P, NC, n), new(P, NC, T)
    status = torch.zeros(P, NC, XGB_CV_SLOTS, dtype=torch.int32, device=dev)
    order = torch.zeros(P, F, n, dtype=torch.uint8, device=dev)
    tree_feature = torch.full((P, NC, XGB_CV_SLOTS, num_rounds, 3), -1, dtype=torch.int32, device=dev) if want_trees else None
    tree_threshold, tree_leaf = (new(P, NC, XGB_CV_SLOTS, num_rounds, 3), new(P, NC, XGB_CV_SLOTS, num_rounds, 4)) if want_trees else (None, None)
    host = [np.asarray(cand_depth, dtype=np.int32), np.asarray(cand_lr, dtype=np.float32), np.asarray(cand_mcw, dtype=np.float64),
            np.asarray(cand_subsample, dtype=np.float64), np.asarray(cand_colsample, dtype=np.float64), np.asarray(cand_ids, dtype=np.int32)]      # read before the call returns
    _hip.check(_hip.lib().pfn_xgb_cv(train.data_ptr(), labels.data_ptr(), test.data_ptr(), fold.data_ptr(), *(h.ctypes.data for h in host), P, n, T, F, NC, int(n_splits),
                                     num_rounds, int(seed), _hip.ptr(problem_ids), order.data_ptr(), cv_margin.data_ptr(), test_margin.data_ptr(), status.data_ptr(),
                                     _hip.ptr(tree_feature), _hip.ptr(tree_threshold), _hip.ptr(tree_leaf), _hip.stream_ptr(dev)), 'pfn_xgb_cv')
    return XgbCvOut(cv_margin, test_margin, status, tree_feature, tree_threshold, tree_leaf)


# ---- Oblivious boosted trees with their grid search (csrc/catboost_cv.hip; include/pfn_hip.h "Oblivious boosted trees with their grid search") ----
CATBOOST_CV_SLOTS, CATBOOST_CV_MAX_CANDIDATES, CATBOOST_CV_MAX_DEPTH, CATBOOST_CV_MAX_LEAVES = 2, 64, 7, 128      # PFN_CATBOOST_CV_*
CATBOOST_CV_MAX_ROUNDS, CATBOOST_CV_MAX_CHECKPOINTS = 1024, 8
CATBOOST_CV_DONE, CATBOOST_CV_NONFINITE, CATBOOST_CV_ONE_CLASS = 1, 2, 3      # status
CATBOOST_CV_LIMITS = dict(n=(4, 128), T=(1, 128), F=(1, 128), NC=(1, CATBOOST_CV_MAX_CANDIDATES), depth=(1, CATBOOST_CV_MAX_DEPTH),
                          num_rounds=(1, CATBOOST_CV_MAX_ROUNDS))
CatboostCvOut = collections.namedtuple('CatboostCvOut', 'hold_margin test_margin status tree_feature tree_threshold tree_leaf')


def catboost_cv_check(n, T, F, cand_depth, num_rounds=1):
    """The limits of a pfn_catboost_cv launch, raised as ValueError before any launch.  cand_depth: the candidates' depths.  Host only."""
    cand_depth = [int(d) for d in cand_depth]
    _limits_check('catboost_cv', CATBOOST_CV_LIMITS, n=n, T=T, F=F, NC=len(cand_depth), num_rounds=int(num_rounds))
    for d in cand_depth:
        _limits_check('catboost_cv', CATBOOST_CV_LIMITS, depth=d)


def catboost_cv(train, labels, test, fold, cand_depth, cand_lr, cand_l2, num_rounds, checkpoints=None, seed=0, problem_ids=None, want_trees=False, cand_ids=None):
    """Every tree of every fit of an oblivious-tree grid search in one launch (pfn_catboost_cv, after a small launch that sorts the columns): train [P,n,F],
    labels [P,n], test [P,T,F] f32 and fold [P,n] int32 (0: held out of the search fit) on the GPU; cand_*: the NC candidates' depth, learning_rate and
    l2_leaf_reg (host sequences), cand_ids their ids in the noise addressing (None: 0 .. NC-1); checkpoints: ascending tree counts, the last num_rounds (None:
    num_rounds alone).  Slot 0 of a candidate learns on the rows with fold != 0, slot 1 on all rows.  Returns CatboostCvOut(hold_margin [P,NC,NK,n] (written at
    the rows with fold == 0; NaN elsewhere), test_margin [P,NC,NK,T], status [P,NC,2] int32, and with want_trees tree_feature int32 / tree_threshold f32
    [P,NC,2,num_rounds,7] and tree_leaf [P,NC,2,num_rounds,128], else None).  A fit whose status is not CATBOOST_CV_DONE leaves its margins NaN."""
    import numpy as np
    cand_depth, cand_lr, cand_l2 = [int(d) for d in cand_depth], [float(v) for v in cand_lr], [float(v) for v in cand_l2]
    NC, num_rounds = len(cand_depth), int(num_rounds)
    cand_ids = list(range(NC)) if cand_ids is None else [int(v) for v in cand_ids]
    checkpoints = [num_rounds] if checkpoints is None else [int(k) for k in checkpoints]
    if not all(len(seq) == NC for seq in (cand_lr, cand_l2, cand_ids)) or not all(math.isfinite(v) and v > 0 for v in cand_lr) or \
            not all(math.isfinite(v) and v >= 0 for v in cand_l2) or not all(0 <= v < CATBOOST_CV_MAX_CANDIDATES for v in cand_ids):
        raise ValueError('cand_depth, cand_lr > 0, cand_l2 >= 0, cand_ids in 0 .. 63: [NC] each, all finite')
    NK = len(checkpoints)
    if not 1 <= NK <= CATBOOST_CV_MAX_CHECKPOINTS or checkpoints[0] < 1 or any(b <= a for a, b in zip(checkpoints, checkpoints[1:])) or checkpoints[-1] != num_rounds:
        raise ValueError(f'checkpoints: 1 .. {CATBOOST_CV_MAX_CHECKPOINTS} ascending tree counts >= 1, the last equal to num_rounds = {num_rounds}')
    P, n, T, F = _fold_args(lambda n, T, F, NC: catboost_cv_check(n, T, F, cand_depth, num_rounds), train, labels, fold, test, NC=NC)
    dev = train.device
    if problem_ids is not None:
        assert problem_ids.dtype == torch.int64 and problem_ids.shape == (P,) and problem_ids.is_contiguous() and problem_ids.device == dev
    new = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=dev)
    hold_margin, test_margin = new(P, NC, NK, n), new(P, NC, NK, T)
    status = torch.zeros(P, NC, CATBOOST_CV_SLOTS, dtype=torch.int32, device=dev)
    order = torch.zeros(P, F, n, dtype=torch.uint8, device=dev)
    tree_feature = torch.full((P, NC, CATBOOST_CV_SLOTS, num_rounds, CATBOOST_CV_MAX_DEPTH), -1, dtype=torch.int32, device=dev) if want_trees else None
    tree_threshold = new(P, NC, CATBOOST_CV_SLOTS, num_rounds, CATBOOST_CV_MAX_DEPTH) if want_trees else None
    tree_leaf = new(P, NC, CATBOOST_CV_SLOTS, num_rounds, CATBOOST_CV_MAX_LEAVES) if want_trees else None
    host = [np.asarray(cand_depth, dtype=np.int32), np.asarray(cand_lr, dtype=np.float32), np.asarray(cand_l2, dtype=np.float32),
            np.asarray(cand_ids, dtype=np.int32), np.asarray(checkpoints, dtype=np.int32)]      # read before the call returns
    _hip.check(_hip.lib().pfn_catboost_cv(train.data_ptr(), labels.data_ptr(), test.data_ptr(), fold.data_ptr(), *(h.ctypes.data for h in host), P, n, T, F, NC, NK,
                                          num_rounds, int(seed), _hip.ptr(problem_ids), order.data_ptr(), hold_margin.data_ptr(), test_margin.data_ptr(),
                                          status.data_ptr(), _hip.ptr(tree_feature), _hip.ptr(tree_threshold), _hip.ptr(tree_leaf), _hip.stream_ptr(dev)),
               'pfn_catboost_cv')
    return CatboostCvOut(hold_margin, test_margin, status, tree_feature, tree_threshold, tree_leaf)


# ---- GP classifier with its grid search (csrc/gpc.hip; include/pfn_hip.h "GP classifier") ----
GPC_FOLDS, GPC_SLOTS, GPC_MAX_CANDIDATES, GPC_MAX_N, GPC_MAX_NEWTON = 5, 6, 64, 112, 100
GPC_UNUSED, GPC_CONVERGED, GPC_CAPPED, GPC_ONE_CLASS, GPC_NONPOSITIVE, GPC_NONFINITE = 0, 1, 2, 3, 4, 5      # status[..., 0]
GPC_LIMITS = dict(n=(4, GPC_MAX_N), T=(1, 128), F=(1, 128), NC=(1, GPC_MAX_CANDIDATES))


def gpc_check(n, T, F, NC=1):
    _limits_check('gpc', GPC_LIMITS, n=n, T=T, F=F, NC=NC)


def _gpc_args(theta, train, labels, fold, n_splits, test=None):
    layout = 'theta [P, NC, 6, 2], train [P, n, F], labels [P, n], fold [P, n], test [P, T, F]'
    if theta.dim() != 4 or theta.shape[:1] != train.shape[:1] or tuple(theta.shape[2:]) != (GPC_SLOTS, 2):
        raise ValueError(layout)
    NC = theta.shape[1]
    P, n, _, F = _fold_args(gpc_check, train, labels, fold, test, NC=NC, splits=(n_splits, GPC_FOLDS), also_f32=(theta,), layout=layout)
    return P, n, F, NC


def gpc_lml_grad(theta, train, labels, fold, n_splits):
    """-Z and -dZ/dtheta of the Laplace approximation of every fit of a GP-classifier grid search in one launch (pfn_gpc_lml_grad): theta [P,NC,6,2] f32 =
    (log c, log l) per (problem, candidate, slot), train [P,n,F], labels [P,n] f32, fold [P,n] int32 on the GPU.  Slot s < n_splits is the fit without fold s,
    slot n_splits the refit on all rows.  Returns (value [P,NC,6], grad [P,NC,6,2], status [P,NC,6,2] int32 = (GPC_* exit reason, Newton iterations))."""
    P, n, F, NC = _gpc_args(theta, train, labels, fold, n_splits)
    dev = train.device
    value = torch.empty(P, NC, GPC_SLOTS, dtype=torch.float32, device=dev)
    grad = torch.empty(P, NC, GPC_SLOTS, 2, dtype=torch.float32, device=dev)
    status = torch.empty(P, NC, GPC_SLOTS, 2, dtype=torch.int32, device=dev)
    _hip.check(_hip.lib().pfn_gpc_lml_grad(theta.data_ptr(), train.data_ptr(), labels.data_ptr(), fold.data_ptr(), P, n, F, NC, int(n_splits), value.data_ptr(),
                                           grad.data_ptr(), status.data_ptr(), _hip.stream_ptr(dev)), 'pfn_gpc_lml_grad')
    return value, grad, status


def gpc_predict(theta, train, labels, test, fold, n_splits):
    """The decision values of every fit of a GP-classifier grid search at its theta in one launch (pfn_gpc_predict); arguments as gpc_lml_grad plus test
    [P,T,F].  Returns (cv_f [P,NC,n,2], test_f [P,NC,T,2], test_var [P,NC,T], status [P,NC,6,2]): a decision value is the pair (m, e), f* = m exp(-e), to be
    formed in f64; cv_f holds row i's pair from the fit that held it out (NaN-filled where no fit did), test_f / test_var are the refit's."""
    P, n, F, NC = _gpc_args(theta, train, labels, fold, n_splits, test)
    T = test.shape[1]
    dev = train.device
    cv_f = torch.full((P, NC, n, 2), float('nan'), dtype=torch.float32, device=dev)
    test_f = torch.empty(P, NC, T, 2, dtype=torch.float32, device=dev)
    test_var = torch.empty(P, NC, T, dtype=torch.float32, device=dev)
    status = torch.empty(P, NC, GPC_SLOTS, 2, dtype=torch.int32, device=dev)
    _hip.check(_hip.lib().pfn_gpc_predict(theta.data_ptr(), train.data_ptr(), labels.data_ptr(), test.data_ptr(), fold.data_ptr(), P, n, T, F, NC, int(n_splits),
                                          cv_f.data_ptr(), test_f.data_ptr(), test_var.data_ptr(), status.data_ptr(), _hip.stream_ptr(dev)), 'pfn_gpc_predict')
    return cv_f, test_f, test_var, status


# ---- stroke prior of the few-shot study (csrc/stroke_prior.hip; include/pfn_hip.h PFN_STROKE_*) ----
STROKE_MAX_STROKES, STROKE_MAX_CLASSES, STROKE_MAX_WIDTH, STROKE_MAX_PASSES, STROKE_COORD_LIMIT = 8, 16, 64, 256, 4096
STROKE_MIN_SIZE, STROKE_MAX_SIZE = 8, 64


def stroke_check(size, n_strokes_hi=0, width_hi=0, num_classes=1):
    """The limits of the stroke kernels, raised as ValueError before the device is asked for anything."""
    if not STROKE_MIN_SIZE <= size <= STROKE_MAX_SIZE:
        raise ValueError(f'stroke: size = {size} outside {STROKE_MIN_SIZE} .. {STROKE_MAX_SIZE} (one lane per row, a row\'s mask in 64 bits)')
    if not 0 <= n_strokes_hi <= STROKE_MAX_STROKES:
        raise ValueError(f'stroke: strokes = {n_strokes_hi} outside 0 .. {STROKE_MAX_STROKES}')
    if not 0 <= width_hi <= STROKE_MAX_WIDTH:
        raise ValueError(f'stroke: width = {width_hi} outside 0 .. {STROKE_MAX_WIDTH}')
    if not 1 <= num_classes <= STROKE_MAX_CLASSES:
        raise ValueError(f'stroke: num_classes = {num_classes} outside 1 .. {STROKE_MAX_CLASSES}')


def stroke_render(segs, n_strokes, width, size, noise=None, normalize=False, out=None, seed=0, offset=0, want_bytes=False, check=True):
    """N glyphs from explicit parameters (pfn_stroke_render): segs [N,8,4] int32 = (x0, y0, x1, y1), n_strokes [N], width [N] int32, noise [N,size^2] uint8 or
    None (drawn on the device) on the GPU.  Returns x [N,size^2] f32 -- or writes image n to out[n] when `out` ([N, >= size^2] f32, rows contiguous) is given --
    and with `want_bytes` (x, raw, img): the uint8 image before and after the blur.  `check` reads back the largest stroke count and width first (one
    synchronisation) and raises ValueError beyond 8 / 64; without it the kernel clamps them."""
    stroke_check(size)
    if segs.dim() != 3 or tuple(segs.shape[1:]) != (STROKE_MAX_STROKES, 4) or n_strokes.shape != segs.shape[:1] or width.shape != segs.shape[:1]:
        raise ValueError('segs [N, 8, 4], n_strokes [N], width [N]')
    N, px = segs.shape[0], size * size
    if noise is not None and (tuple(noise.shape) != (N, px) or noise.dtype != torch.uint8):
        raise ValueError('noise [N, size^2] uint8')
    _hip.require_gpu_tensor(segs, 'segs')
    dev = segs.device
    for t, name in ((segs, 'segs'), (n_strokes, 'n_strokes'), (width, 'width')):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.device == dev, f'{name}: contiguous int32 on {dev}'
    assert noise is None or (noise.is_contiguous() and noise.device == dev), 'noise: contiguous on the same device'
    if check and N:
        n_lo, n_hi, w_lo, w_hi = (int(v) for v in torch.stack([n_strokes.min(), n_strokes.max(), width.min(), width.max()]).tolist())
        stroke_check(size, n_hi if n_lo >= 0 else n_lo, w_hi if w_lo >= 0 else w_lo)
    if out is None:
        out = torch.empty(N, px, dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and out.device == dev and out.dim() == 2 and out.shape[0] == N and out.shape[1] >= px and (N == 0 or out.stride(1) == 1), \
        'out: [N, >= size^2] f32 with contiguous rows'
    raw = torch.empty(N, px, dtype=torch.uint8, device=dev) if want_bytes else None
    img = torch.empty(N, px, dtype=torch.uint8, device=dev) if want_bytes else None
    _hip.check(_hip.lib().pfn_stroke_render(segs.data_ptr(), n_strokes.data_ptr(), width.data_ptr(), _hip.ptr(noise), N, size, int(bool(normalize)),
                                            out.stride(0) if N > 1 else out.shape[1], int(seed) & (2 ** 64 - 1), int(offset), out.data_ptr(), _hip.ptr(raw),
                                            _hip.ptr(img), _hip.stream_ptr(dev)), 'pfn_stroke_render')
    return (out, raw, img) if want_bytes else out


def stroke_prior_sample(labels, size, bounds, num_classes, seed, offset=0, first_dataset=0, normalize=False, want_bytes=False):
    """One batch of the stroke prior (pfn_stroke_prior_sample): labels [B,T] int32 on the GPU; bounds: a dict of inclusive integer ranges strokes, len, start,
    width = (lo, hi) and offset, jitter = (-m, m), as priors.stroke.integer_bounds gives.  Returns a dict: x [T,B,size^2] f32, cls_n [B,C], cls_len [B,C,8],
    cls_start [B,C,8,2] int32, cls_dir [B,C,8] f64, segs [B,T,8,4], width [B,T] int32, status [B] int32 (class strokes that hit the retry cap) and, with
    `want_bytes`, raw / img [B,T,size^2] uint8."""
    if labels.dim() != 2:
        raise ValueError('labels [B, T]')
    B, T = labels.shape
    C, px = int(num_classes), size * size
    (s_lo, s_hi), (l_lo, l_hi), (p_lo, p_hi), (w_lo, w_hi) = bounds['strokes'], bounds['len'], bounds['start'], bounds['width']
    stroke_check(size, s_hi, w_hi, C)
    if bounds['offset'][0] != -bounds['offset'][1] or bounds['jitter'][0] != -bounds['jitter'][1]:
        raise ValueError('offset and jitter ranges are symmetric: (-m, m)')
    _hip.require_gpu_tensor(labels, 'labels')
    dev = labels.device
    assert labels.dtype == torch.int32 and labels.is_contiguous(), 'labels [B, T]: contiguous int32'
    i32 = dict(dtype=torch.int32, device=dev)
    r = dict(x=torch.empty(T, B, px, dtype=torch.float32, device=dev), cls_n=torch.empty(B, C, **i32), cls_len=torch.empty(B, C, STROKE_MAX_STROKES, **i32),
             cls_start=torch.empty(B, C, STROKE_MAX_STROKES, 2, **i32), cls_dir=torch.empty(B, C, STROKE_MAX_STROKES, dtype=torch.float64, device=dev),
             segs=torch.empty(B, T, STROKE_MAX_STROKES, 4, **i32), width=torch.empty(B, T, **i32), status=torch.empty(B, **i32))
    if want_bytes:
        r['raw'] = torch.empty(B, T, px, dtype=torch.uint8, device=dev)
        r['img'] = torch.empty(B, T, px, dtype=torch.uint8, device=dev)
    _hip.check(_hip.lib().pfn_stroke_prior_sample(labels.data_ptr(), B, T, C, size, int(bool(normalize)), s_lo, s_hi, l_lo, l_hi, p_lo, p_hi, w_lo, w_hi,
                                                  bounds['offset'][1], bounds['jitter'][1], int(seed) & (2 ** 64 - 1), int(offset), int(first_dataset),
                                                  r['x'].data_ptr(), r['cls_n'].data_ptr(), r['cls_len'].data_ptr(), r['cls_start'].data_ptr(), r['cls_dir'].data_ptr(),
                                                  r['segs'].data_ptr(), r['width'].data_ptr(), _hip.ptr(r.get('raw')), _hip.ptr(r.get('img')), r['status'].data_ptr(),
                                                  _hip.stream_ptr(dev)), 'pfn_stroke_prior_sample')
    return r


# ---- Omniglot episode loader of the few-shot study (csrc/episode.hip; include/pfn_hip.h PFN_EPISODE_*) ----
EPISODE_MIN_SIZE, EPISODE_MAX_SIZE, EPISODE_MAX_WAY, EPISODE_MAX_IMAGES = 8, 64, 16, 64
EPISODE_STANDARD, EPISODE_JONAS = 0, 1
EPISODE_MODES = {'standard': EPISODE_STANDARD, 'jonas': EPISODE_JONAS}


def episode_lds_bytes(size):
    """Dynamic LDS of one block of the image kernel: the 256-entry table and four images with rows padded to the odd stride size | 1."""
    return (256 + 4 * size * (size | 1)) * 4


def episode_check(size, n_img=1, n_classes=1, n_way=1, k_shot=None, pool=None, alphabet_offsets=None):
    """The limits of the episode kernels, raised as ValueError before the device is asked for anything.  pool: (lo, hi) of standard mode; alphabet_offsets: the
    HOST list [A + 1] of jonas mode (the kernel gets them as a device array and cannot refuse them)."""
    if not EPISODE_MIN_SIZE <= size <= EPISODE_MAX_SIZE:
        raise ValueError(f'episode: size = {size} outside {EPISODE_MIN_SIZE} .. {EPISODE_MAX_SIZE} (one lane per row, a row\'s mask in 64 bits)')
    if not 1 <= n_img <= EPISODE_MAX_IMAGES:
        raise ValueError(f'episode: n_img = {n_img} outside 1 .. {EPISODE_MAX_IMAGES}')
    if n_classes < 1 or n_classes * n_img >= 2 ** 31:
        raise ValueError(f'episode: n_classes = {n_classes} below 1, or n_classes n_img >= 2^31')
    if not 1 <= n_way <= EPISODE_MAX_WAY:
        raise ValueError(f'episode: n_way = {n_way} outside 1 .. {EPISODE_MAX_WAY}')
    if k_shot is not None and not 1 <= k_shot < n_img:
        raise ValueError(f'episode: k_shot = {k_shot} outside 1 .. n_img - 1 = {n_img - 1}')
    if pool is not None and not (0 <= pool[0] and pool[1] <= n_classes and pool[1] - pool[0] >= n_way):
        raise ValueError(f'episode: the pool [{pool[0]}, {pool[1]}) must lie in [0, {n_classes}) and hold at least n_way = {n_way} classes')
    if alphabet_offsets is not None:
        o = [int(v) for v in alphabet_offsets]
        if len(o) < 2 or o[0] < 0 or o[-1] > n_classes or any(b - a < n_way for a, b in zip(o, o[1:])):
            raise ValueError(f'episode: alphabet offsets {o} must ascend inside [0, {n_classes}] with at least n_way = {n_way} classes per alphabet')


def _episode_bank(bank, table=None):
    """(images [C, n_img, size, size] on the GPU, table or None) of an ImageBank-like object (fields images, table) or of a plain tensor."""
    images = getattr(bank, 'images', bank)
    table = getattr(bank, 'table', table)
    if images.dim() != 4 or images.shape[2] != images.shape[3] or images.dtype not in (torch.uint8, torch.float32):
        raise ValueError('bank [n_classes, n_img, size, size], uint8 (with a table) or float32')
    if (images.dtype == torch.uint8) != (table is not None):
        raise ValueError('a uint8 bank needs its 256-entry f32 table, an f32 bank takes none')
    episode_check(images.shape[2], images.shape[1], images.shape[0])
    assert images.is_contiguous(), 'bank: contiguous'
    if table is not None:
        assert table.dtype == torch.float32 and tuple(table.shape) == (256,) and table.is_contiguous() and table.device == images.device, 'table: [256] f32 beside the bank'
    return images, table


def episode_gather(bank, src, rot=None, shift=None, table=None, out=None, seed=0, offset=0, first_image=0, check=True, want_status=True):
    """N images of the bank, rotated and shifted (pfn_episode_gather): src [N] (class * n_img + image), rot [N] quarter turns or None, int32 on the GPU;
    shift: None (no shift), 'draw' (the kernel draws it inside each image's range from Philox at counter first_image + n) or [N, 2] int32 = (tx, ty).  Returns a
    dict: x [N, size^2] f32 -- image n written to out[n] when `out` ([N, >= size^2] f32, rows contiguous) is given --, bbox [N, 4] = (c0, c1, r0, r1), shift
    [N, 2] as used, status [1] (images without content; None without `want_status`, which saves the counting launch).  `check` reads back the range of src
    and rot first (one synchronisation) and raises ValueError outside the bank / 0 .. 3; without it the kernel clamps them."""
    images, table = _episode_bank(bank, table)
    C, n_img, size = images.shape[0], images.shape[1], images.shape[2]
    dev, px = images.device, size * size
    if src.dim() != 1 or (rot is not None and rot.shape != src.shape):
        raise ValueError('src [N], rot [N]')
    N = src.shape[0]
    draw = isinstance(shift, str)
    if draw and shift != 'draw':
        raise ValueError("shift: None, 'draw' or [N, 2] int32")
    shift_in = None if (draw or shift is None) else shift
    if shift_in is not None and tuple(shift_in.shape) != (N, 2):
        raise ValueError('shift [N, 2]')
    _hip.require_gpu_tensor(images, 'bank')
    for t, name in ((src, 'src'), (rot, 'rot'), (shift_in, 'shift')):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.device == dev), f'{name}: contiguous int32 on {dev}'
    if check and N:
        probe = [src.min(), src.max()] + ([rot.min(), rot.max()] if rot is not None else [])
        lo_hi = [int(v) for v in torch.stack(probe).tolist()]
        if lo_hi[0] < 0 or lo_hi[1] >= C * n_img:
            raise ValueError(f'episode: src outside 0 .. {C * n_img - 1}')
        if rot is not None and (lo_hi[2] < 0 or lo_hi[3] > 3):
            raise ValueError('episode: rot outside 0 .. 3')
    if out is None:
        out = torch.empty(N, px, dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and out.device == dev and out.dim() == 2 and out.shape[0] == N and out.shape[1] >= px and (N == 0 or out.stride(1) == 1), \
        'out: [N, >= size^2] f32 with contiguous rows'
    i32 = dict(dtype=torch.int32, device=dev)
    r = dict(x=out, bbox=torch.empty(N, 4, **i32), shift=torch.empty(N, 2, **i32), status=torch.zeros(1, **i32) if want_status else None)
    _hip.check(_hip.lib().pfn_episode_gather(images.data_ptr(), _hip.ptr(table), C, n_img, size, src.data_ptr(), _hip.ptr(rot), _hip.ptr(shift_in), N, int(draw),
                                             out.stride(0) if N > 1 else out.shape[1], int(seed) & (2 ** 64 - 1), int(offset), int(first_image), out.data_ptr(),
                                             r['bbox'].data_ptr(), r['shift'].data_ptr(), _hip.ptr(r['status']), _hip.stream_ptr(dev)), 'pfn_episode_gather')
    return r


def episode_sample(bank, B, n_way, k_shot, mode, train, translate, seed, offset=0, first_dataset=0, num_classes_used=None):
    """One batch of the episode loader (pfn_episode_sample) from an ImageBank (priors.omniglot.ImageBank: images, table, n_train_classes and the alphabet
    offsets of both splits, on the host and on the device).  mode: 'standard' or 'jonas'.  standard: the train pool is [0, num_classes_used) (default:
    n_train_classes), the test pool [n_train_classes, n_classes).  Returns a dict: x [T, B, size^2] f32, labels, targets [B, T], classes, rotations [B, n_way],
    src [B, T], shift [B, T, 2], bbox [B, T, 4], status [B], the integers int32."""
    images, table = _episode_bank(bank)
    C, n_img, size = images.shape[0], images.shape[1], images.shape[2]
    mode_id = EPISODE_MODES[mode] if isinstance(mode, str) else int(mode)
    pool, offsets, offsets_host = (0, 0), None, None
    if mode_id == EPISODE_STANDARD:
        pool = (0, min(int(bank.n_train_classes if num_classes_used is None else num_classes_used), C)) if train else (int(bank.n_train_classes), C)
    else:
        offsets = bank.train_alphabet_offsets if train else bank.test_alphabet_offsets
        offsets_host = bank.alphabet_offsets_host(train)
        if offsets is None:
            raise ValueError('episode: jonas mode needs the alphabet offsets of the split (ImageBank.from_arrays(..., train_alphabet_offsets, test_alphabet_offsets))')
        assert offsets.dtype == torch.int32 and offsets.is_contiguous() and offsets.device == images.device and offsets.numel() == len(offsets_host)
    episode_check(size, n_img, C, n_way, k_shot, pool if mode_id == EPISODE_STANDARD else None, offsets_host)
    T, dev, px = n_way * k_shot + 1, images.device, size * size
    if B < 0 or B * T >= 2 ** 31:
        raise ValueError(f'episode: B = {B} below 0 or B T >= 2^31')
    _hip.require_gpu_tensor(images, 'bank')
    i32 = dict(dtype=torch.int32, device=dev)
    r = dict(x=torch.empty(T, B, px, dtype=torch.float32, device=dev), labels=torch.empty(B, T, **i32), targets=torch.empty(B, T, **i32),
             classes=torch.empty(B, n_way, **i32), rotations=torch.empty(B, n_way, **i32), src=torch.empty(B, T, **i32), shift=torch.empty(B, T, 2, **i32),
             bbox=torch.empty(B, T, 4, **i32), status=torch.empty(B, **i32))
    _hip.check(_hip.lib().pfn_episode_sample(images.data_ptr(), _hip.ptr(table), C, n_img, size, B, n_way, k_shot, mode_id, int(bool(train)), int(bool(translate)),
                                             pool[0], pool[1], _hip.ptr(offsets), 0 if offsets is None else offsets.numel() - 1, int(seed) & (2 ** 64 - 1), int(offset),
                                             int(first_dataset), r['x'].data_ptr(), r['labels'].data_ptr(), r['targets'].data_ptr(), r['classes'].data_ptr(),
                                             r['rotations'].data_ptr(), r['src'].data_ptr(), r['shift'].data_ptr(), r['bbox'].data_ptr(), r['status'].data_ptr(),
                                             _hip.stream_ptr(dev)), 'pfn_episode_sample')
    return r


# ---- class-label embedding of the few-shot study (csrc/class_embed.hip; include/pfn_hip.h pfn_class_embed_*) ----
CLASS_EMBED_MAX_FEATURES, CLASS_EMBED_MAX_CLASSES = _hip.MAX_FEATURES, 1024


def class_embed_supported(F, E, C):
    """The shape limits of pfn_class_embed_* (include/pfn_hip.h)."""
    return 1 <= F <= CLASS_EMBED_MAX_FEATURES and 1 <= C <= CLASS_EMBED_MAX_CLASSES and E >= 8 and E % 8 == 0


def class_embed_check(x, labels, weight, bias, table, sep, precision):
    """The argument checks of `class_embed`, raised as ValueError before the device is asked for anything.  Returns (S, B, F, E, C, sep, PFN_PREC_*)."""
    if x.dim() != 3 or labels.dim() != 2 or tuple(labels.shape) != tuple(x.shape[:2]):
        raise ValueError(f'class_embed: x [S, B, F] and labels [S, B], got {tuple(x.shape)} and {tuple(labels.shape)}')
    if weight.dim() != 2 or table.dim() != 2 or bias is None or bias.dim() != 1:
        raise ValueError('class_embed: weight [E, F], bias [E], table [C, E]')
    S, B, F = x.shape
    E, C = weight.shape[0], table.shape[0]
    if weight.shape[1] != F or bias.shape[0] != E or table.shape[1] != E:
        raise ValueError(f'class_embed: weight {tuple(weight.shape)}, bias {tuple(bias.shape)}, table {tuple(table.shape)} do not fit x with F = {F} (weight [E, F], bias [E], table [C, E])')
    if not class_embed_supported(F, E, C):
        raise ValueError(f'class_embed: F = {F} outside 1 .. {CLASS_EMBED_MAX_FEATURES}, C = {C} outside 1 .. {CLASS_EMBED_MAX_CLASSES}, or E = {E} below 8 / no multiple of 8')
    if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
        raise ValueError(f'class_embed: labels are class indices, got {labels.dtype}')
    sep = int(sep)
    if not 0 <= sep <= S:
        raise ValueError(f'class_embed: sep = {sep} outside 0 .. S = {S}')
    if isinstance(precision, str):
        if precision not in _hip.PRECISIONS:
            raise ValueError(f'class_embed: precision {precision!r} is none of {sorted(_hip.PRECISIONS)}')
        precision = _hip.PRECISIONS[precision]
    if precision not in TDT:
        raise ValueError(f'class_embed: precision {precision!r} is no PFN_PREC_* value')
    return S, B, F, E, C, sep, precision


def _f32_aligned(t, align=4):
    t = t.detach()
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    return t.clone() if t.data_ptr() % align else t


class _ClassEmbedFunction(torch.autograd.Function):
    """src = class embedding (pfn_class_embed_forward); its backward is pfn_class_embed_backward.  With `model` the gradients are accumulated straight into the
    parameters' .grad -- views of the model's flat gradient buffer, as the stack's are -- and autograd is handed None; without it they are returned."""

    @staticmethod
    def forward(ctx, x, labels, weight, bias, table, dims, deterministic, status, model):
        S, B, F, E, C, sep, prec = dims
        lib = _hip.lib()
        dev = x.device
        stream = _hip.stream_ptr(dev)
        if x.dtype != torch.float32 or x.stride(-1) != 1 or x.data_ptr() % 4:
            x = x.float().contiguous()
        labels = labels.to(dev)
        if labels.dtype != torch.int64:
            labels = labels.long()
        wx, bx, tb = _f32_aligned(weight), _f32_aligned(bias, 16), _f32_aligned(table)
        ws_bytes = _hip.check(lib.pfn_class_embed_workspace_bytes(B, S, F, E, C, prec), 'pfn_class_embed_workspace_bytes')
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        src = torch.empty((S, B, E), dtype=torch.float32, device=dev)
        flags = 1 if deterministic else 0
        _hip.check(lib.pfn_class_embed_forward(x.data_ptr(), x.stride(0), x.stride(1), labels.data_ptr(), labels.stride(0), labels.stride(1), wx.data_ptr(), bx.data_ptr(),
                                               tb.data_ptr(), B, S, F, E, C, sep, prec, flags, ws.data_ptr(), ws_bytes, src.data_ptr(), _hip.ptr(status), stream),
                   'pfn_class_embed_forward')
        ctx.state = (ws, dims, flags, model, wx, (weight, bias, table))
        return src

    @staticmethod
    def backward(ctx, dsrc):
        ws, (S, B, F, E, C, sep, prec), flags, model, wx, params = ctx.state
        ctx.state = None
        dev = ws.device
        need = ctx.needs_input_grad[2:5]
        dsrc = _f32_aligned(dsrc, 16)
        if model is not None:
            model._attach_grads()
            outs = [p.grad if n else None for p, n in zip(params, need)]
        else:
            outs = [torch.zeros(p.shape, dtype=torch.float32, device=dev) if n else None for p, n in zip(params, need)]
        _hip.check(_hip.lib().pfn_class_embed_backward(dsrc.data_ptr(), wx.data_ptr(), B, S, F, E, C, sep, prec, flags, ws.data_ptr(), ws.numel(), _hip.ptr(outs[0]),
                                                       _hip.ptr(outs[1]), _hip.ptr(outs[2]), _hip.stream_ptr(dev)), 'pfn_class_embed_backward')
        if model is not None:
            outs = [None, None, None]
        return (None, None, outs[0], outs[1], outs[2], None, None, None, None)


def class_embed(x, labels, weight, bias, table, sep, precision, deterministic=False, status=None, _model=None):
    """The embedding of a (Linear, CanEmb) model on the matrix cores: src [S, B, E] f32 with
        src[t, b] = weight . x[t, b] + bias + (table[labels[t, b]] if t < sep else 0)
    for x [S, B, F] f32 (any strides over S and B), labels [S, B] of an integer dtype, weight [E, F], bias [E], table [C, E].  `precision`: 'fp16' / 'bf16' / 'f32'
    (or a PFN_PREC_* value), the operand type of the GEMMs.  Differentiable in weight, bias and table -- not in x.  deterministic=True: the weight-gradient GEMM
    runs without token splits, two runs give bit-equal gradients.  status: an int32 tensor [2] on the device that the kernels add to -- [0] train-row labels
    outside [0, C) (the row gets no class row, the table no gradient from it), [1] values beyond +-65504 stored saturated under fp16."""
    dims = class_embed_check(x, labels, weight, bias, table, sep, precision)
    if status is not None and (status.dtype != torch.int32 or status.numel() != 2 or not status.is_contiguous()):
        raise ValueError('class_embed: status is a contiguous int32 tensor of two elements')
    _hip.require_gpu_tensor(x, 'x')
    for t, name in ((weight, 'weight'), (bias, 'bias'), (table, 'table')) + (((status, 'status'),) if status is not None else ()):
        _hip.require_gpu_tensor(t, name)
    return _ClassEmbedFunction.apply(x, labels, weight, bias, table, dims, bool(deterministic), status, _model)
