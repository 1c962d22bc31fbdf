"""TransformerModel: the PFN encoder-only transformer, running on hand-written gfx950 kernels.

API and state-dict parity with the reference `transformer.py` (constructor :14, forward :55-91,
init :43-53); the call `self.transformer_encoder(src, src_mask)` (:84) and everything around it
(embedding :66-74, decoder :85, test-row slice :91) is replaced by ONE autograd node that drives
libpfn_hip.so through the C ABI (`pfn_stack_forward` / `pfn_stack_backward`).

PyTorch's role here is plumbing only: it owns the parameter / gradient / activation memory and the
stream.  All parameters are views into one flat f32 buffer (and their .grad into one flat gradient
buffer) so the optimizer and the data-parallel all-reduce touch a single contiguous range.
There is no PyTorch fallback: CPU tensors or a missing library raise `HipExtensionError`.
"""
import ctypes

import torch
from torch import nn

from transformerscandobayesianinference_amd import _hip, encoders, hipops
from transformerscandobayesianinference_amd.positional_encodings import NoPositionalEncoding
from transformerscandobayesianinference_amd.utils import SeqBN

_ALIGN = 64  # elements; must match make_layout() in csrc/pfn_api.hip


class _SelfAttentionParams(nn.Module):
    """Parameter container with the key names of torch.nn.MultiheadAttention
    (`in_proj_weight`, `in_proj_bias`, `out_proj.{weight,bias}`) and its default initialisation."""

    def __init__(self, emsize):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * emsize, emsize))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * emsize))
        self.out_proj = nn.Linear(emsize, emsize)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)


class _EncoderLayerParams(nn.Module):
    """Parameter container with the key names of torch.nn.TransformerEncoderLayer."""

    def __init__(self, emsize, nhid):
        super().__init__()
        self.self_attn = _SelfAttentionParams(emsize)
        self.linear1 = nn.Linear(emsize, nhid)
        self.linear2 = nn.Linear(nhid, emsize)
        self.norm1 = nn.LayerNorm(emsize, eps=1e-5)
        self.norm2 = nn.LayerNorm(emsize, eps=1e-5)


class _EncoderParams(nn.Module):
    def __init__(self, emsize, nhid, nlayers):
        super().__init__()
        self.layers = nn.ModuleList([_EncoderLayerParams(emsize, nhid) for _ in range(nlayers)])


class _StackFunction(torch.autograd.Function):
    """logits = stack(x, y | src); one node for embedding + L layers + decoder."""

    @staticmethod
    def forward(ctx, flat_params, model, x, y, src, sep, inference, ragged=None):
        lib = _hip.lib()
        dev = flat_params.device
        stream = _hip.stream_ptr(dev)
        # `inference` is decided by the caller: grad mode is always off inside Function.forward, so it cannot be read here
        desc, shadow = model._operands(stream, inference)
        if src is not None:
            src = src.contiguous().float()
            if src.data_ptr() % 16:      # (a contiguous view keeps its storage offset; the kernel loads src 16 bytes at a time)
                src = src.clone()
            S, B = src.shape[0], src.shape[1]
            xs = ys = None
            x_ptr = y_ptr = 0
            x_st = x_sb = y_st = y_sb = 0
        else:
            if x.dtype != torch.float32 or x.stride(-1) != 1:
                x = x.float().contiguous()
            if y.dtype != torch.float32:
                y = y.float()
            S, B = x.shape[0], x.shape[1]
            x_ptr, y_ptr = x.data_ptr(), y.data_ptr()
            x_st, x_sb = x.stride(0), x.stride(1)
            y_st, y_sb = y.stride(0), y.stride(1)
        ws_bytes = lib.pfn_workspace_bytes(ctypes.byref(desc), B, S)
        _hip.check(ws_bytes, 'pfn_workspace_bytes')
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        ctx.ragged = ragged
        if ragged is not None:
            # a ragged batch (forward_batches): per-dataset eval positions, compact test rows dataset-major -- one launch set for several micro-batches
            sep_of, row_off, sep_min, sep_max, test_rows = ragged
            logits = torch.empty((test_rows, desc.n_out or desc.emsize), dtype=torch.float32, device=dev)
            ctx.dropout_seed = model._next_dropout_seed() if (model.training and desc.dropout > 0) else None
            _hip.check(lib.pfn_stack_forward_ragged(ctypes.byref(desc), flat_params.data_ptr(), shadow.data_ptr(), x_ptr, x_st, x_sb, y_ptr, y_st, y_sb, B, S,
                                                    sep_of.data_ptr(), row_off.data_ptr(), sep_min, sep_max, test_rows, ws.data_ptr(), ws_bytes, logits.data_ptr(), stream,
                                                    int(ctx.dropout_seed is not None), ctx.dropout_seed or 0), 'pfn_stack_forward_ragged')
            ctx.model, ctx.ws, ctx.dims = model, ws, (B, S, sep_max)
            ctx.operands = (desc, shadow)
            ctx.inputs = (x, y, None)
            ctx.src_needs_grad = False
            return logits
        logits = torch.empty((S - sep, B, desc.n_out or desc.emsize), dtype=torch.float32, device=dev)   # n_out 0: the encoder's test rows
        # dropout (reference train.py:22 default 0.2; TransformerEncoderLayer's four sites): live in training mode only.  Every pass
        # takes its own 64-bit seed; the masks are counter-based functions of it, regenerated by the backward (include/pfn_hip.h)
        ctx.dropout_seed = None
        if model.training and desc.dropout > 0:
            ctx.dropout_seed = model._next_dropout_seed()
            _hip.check(lib.pfn_stack_forward_dropout(ctypes.byref(desc), flat_params.data_ptr(), shadow.data_ptr(),
                                                     x_ptr, x_st, x_sb, y_ptr, y_st, y_sb, _hip.ptr(src), B, S, sep,
                                                     ws.data_ptr(), ws_bytes, logits.data_ptr(), stream, ctx.dropout_seed), 'pfn_stack_forward_dropout')
        else:
            _hip.check(lib.pfn_stack_forward(ctypes.byref(desc), flat_params.data_ptr(), shadow.data_ptr(),
                                             x_ptr, x_st, x_sb, y_ptr, y_st, y_sb, _hip.ptr(src), B, S, sep,
                                             ws.data_ptr(), ws_bytes, logits.data_ptr(), stream), 'pfn_stack_forward')
        ctx.model, ctx.ws, ctx.dims = model, ws, (B, S, sep)
        ctx.operands = (desc, shadow)      # the backward reads the workspace in the layout THIS descriptor's precision wrote
        ctx.inputs = (x, y, src)
        ctx.src_needs_grad = src is not None and ctx.needs_input_grad[4]
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        lib = _hip.lib()
        model, ws = ctx.model, ctx.ws
        B, S, sep = ctx.dims
        x, y, src = ctx.inputs
        dev = ws.device
        stream = _hip.stream_ptr(dev)
        desc, shadow = ctx.operands
        if desc is not model._desc:
            raise RuntimeError('backward through an inference-precision forward: the forward of this graph ran the eval_precision kernels')
        model._attach_grads()
        dlogits = dlogits.contiguous().float()
        dsrc = None
        if src is not None:
            dsrc = torch.empty_like(src)
            args = (0, 0, 0, 0, 0, 0)
        else:
            args = (x.data_ptr(), x.stride(0), x.stride(1), y.data_ptr(), y.stride(0), y.stride(1))
        hook = model._first_group_hook
        split = hook is not None and hook.armed()
        if ctx.ragged is not None:
            sep_of, row_off, sep_min, sep_max, test_rows = ctx.ragged
            cb = _hip.HOST_CALLBACK(lambda user: hook.first_group_launched()) if split else None
            _hip.check(lib.pfn_stack_backward_ragged(ctypes.byref(desc), model._flat.data_ptr(), shadow.data_ptr(), *args, B, S,
                                                     sep_of.data_ptr(), row_off.data_ptr(), sep_min, sep_max, test_rows, ws.data_ptr(), ws.numel(), dlogits.data_ptr(),
                                                     model._flat_grad.data_ptr(), stream, hook.first_group_layers if split else 0, cb, None,
                                                     int(ctx.dropout_seed is not None), ctx.dropout_seed or 0), 'pfn_stack_backward_ragged')
            ctx.ws = None
            return None, None, None, None, None, None, None, None
        if split or ctx.dropout_seed is not None:
            # data-parallel runs (dp.OverlappedGradientReducer): the top layers' weight gradients are launched early and the hook
            # records an event right behind them, so their all-reduce can run under the rest of this backward.
            # dropout: the backward regenerates the forward's masks from its seed.
            cb = _hip.HOST_CALLBACK(lambda user: hook.first_group_launched()) if split else None
            _hip.check(lib.pfn_stack_backward_split(ctypes.byref(desc), model._flat.data_ptr(), shadow.data_ptr(), *args,
                                                    B, S, sep, ws.data_ptr(), ws.numel(), dlogits.data_ptr(),
                                                    model._flat_grad.data_ptr(), _hip.ptr(dsrc), stream,
                                                    hook.first_group_layers if split else 0, cb, None,
                                                    int(ctx.dropout_seed is not None), ctx.dropout_seed or 0),
                       'pfn_stack_backward_split')
        else:
            _hip.check(lib.pfn_stack_backward(ctypes.byref(desc), model._flat.data_ptr(), shadow.data_ptr(), *args,
                                              B, S, sep, ws.data_ptr(), ws.numel(), dlogits.data_ptr(),
                                              model._flat_grad.data_ptr(), _hip.ptr(dsrc), stream), 'pfn_stack_backward')
        dx = dy = None
        if src is None and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3]):
            # input gradients of the fused embedding from the d(src) the backward left in its workspace (pfn_stack_input_grads): x for every row, y for the train rows
            dx = torch.empty((S, B, x.shape[2]), dtype=torch.float32, device=dev)
            dy = torch.empty((S, B), dtype=torch.float32, device=dev) if ctx.needs_input_grad[3] else None
            if sep == S:      # no test row: nothing reaches the embedding
                dx.zero_()
                if dy is not None:
                    dy.zero_()
            else:
                _hip.check(lib.pfn_stack_input_grads(ctypes.byref(desc), model._flat.data_ptr(), B, S, sep, ws.data_ptr(), ws.numel(),
                                                     dx.data_ptr(), dx.stride(0), dx.stride(1), _hip.ptr(dy), B, 1, stream),
                           'pfn_stack_input_grads')
        ctx.ws = None
        return (None, None, dx if ctx.needs_input_grad[2] else None, dy, (dsrc if ctx.src_needs_grad else None), None, None, None)


class _PredictFunction(torch.autograd.Function):
    """One chunk of `TransformerModel.predict` that keeps its per-layer activations (pfn_stack_predict_saved) for pfn_stack_predict_backward:
    the gradient reaches x_test only -- the context and the parameters are constants here."""

    @staticmethod
    def forward(ctx, x, model, context, desc, shadow):
        lib = _hip.lib()
        dev = x.device
        stream = _hip.stream_ptr(dev)
        n, B, _ = x.shape
        ws_bytes = _hip.check(lib.pfn_predict_grad_workspace_bytes(ctypes.byref(desc), B, n), 'pfn_predict_grad_workspace_bytes')
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty((n, B, desc.n_out or desc.emsize), dtype=torch.float32, device=dev)
        if context.lengths is not None:      # a ragged context: every dataset against its own train rows
            _hip.check(lib.pfn_stack_predict_saved_ragged(ctypes.byref(desc), model._flat.data_ptr(), shadow.data_ptr(), context.buffer.data_ptr(),
                                                          context.buffer.numel(), context.sep, context.sep_of.data_ptr(), x.data_ptr(), x.stride(0), x.stride(1),
                                                          B, n, ws.data_ptr(), ws_bytes, out.data_ptr(), stream), 'pfn_stack_predict_saved_ragged')
        else:
            _hip.check(lib.pfn_stack_predict_saved(ctypes.byref(desc), model._flat.data_ptr(), shadow.data_ptr(), context.buffer.data_ptr(), context.buffer.numel(),
                                                   context.sep, x.data_ptr(), x.stride(0), x.stride(1), B, n, ws.data_ptr(), ws_bytes, out.data_ptr(), stream),
                       'pfn_stack_predict_saved')
        ctx.state = (model, context, desc, shadow, ws, x.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        model, context, desc, shadow, ws, (n, B, F) = ctx.state
        lib = _hip.lib()
        dout = dout.contiguous().float()
        dx = torch.empty((n, B, F), dtype=torch.float32, device=dout.device)
        if context.lengths is not None:
            _hip.check(lib.pfn_stack_predict_backward_ragged(ctypes.byref(desc), model._flat.data_ptr(), shadow.data_ptr(), context.buffer.data_ptr(),
                                                             context.buffer.numel(), context.sep, context.sep_of.data_ptr(), B, n, ws.data_ptr(), ws.numel(),
                                                             dout.data_ptr(), dx.data_ptr(), dx.stride(0), dx.stride(1), _hip.stream_ptr(dout.device)),
                       'pfn_stack_predict_backward_ragged')
        else:
            _hip.check(lib.pfn_stack_predict_backward(ctypes.byref(desc), model._flat.data_ptr(), shadow.data_ptr(), context.buffer.data_ptr(), context.buffer.numel(),
                                                      context.sep, B, n, ws.data_ptr(), ws.numel(), dout.data_ptr(), dx.data_ptr(), dx.stride(0), dx.stride(1),
                                                      _hip.stream_ptr(dout.device)), 'pfn_stack_predict_backward')
        ctx.state = None
        return dx, None, None, None, None


def ragged_layout(T, widths, single_eval_positions):
    """Host side of a ragged batch (pfn_stack_forward_ragged): batch k has widths[k] datasets at eval position single_eval_positions[k] (negative positions count
    from the end, as slicing does in the reference).  Returns (clamped positions per batch, eval position per dataset [B], first compact test row per dataset
    [B + 1]): dataset b's test rows are row_off[b] + (t - sep_of[b]) for t >= sep_of[b], batches and datasets in order."""
    seps = []
    for sep in single_eval_positions:
        sep = int(sep)
        seps.append(max(0, min(T, sep + T if sep < 0 else sep)))
    per_dataset = [s for s, w in zip(seps, widths) for _ in range(w)]
    offs = [0]
    for s in per_dataset:
        offs.append(offs[-1] + T - s)
    return seps, per_dataset, offs


def check_train_lengths(train_lengths, B, sep_max):
    """`condition(src, train_lengths=...)`: one train-row count per dataset, as a sequence or an integer tensor [B], each within [0, sep_max] (the rows of the
    padded src).  Returns them as a tuple of ints; anything else raises ValueError.  (Host side only: the kernels clamp what they read, they do not report it.)"""
    if isinstance(train_lengths, torch.Tensor):
        if train_lengths.dim() != 1 or train_lengths.dtype.is_floating_point or train_lengths.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise ValueError(f'train_lengths: expected an integer tensor [B], got {train_lengths.dtype} of shape {tuple(train_lengths.shape)}')
        train_lengths = train_lengths.tolist()
    lengths = []
    for v in train_lengths:
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f'train_lengths: {v!r} is not an integer')
        lengths.append(int(v))
    if len(lengths) != B:
        raise ValueError(f'train_lengths has {len(lengths)} entries, the batch has B={B} datasets')
    for b, v in enumerate(lengths):
        if v < 0 or v > sep_max:
            raise ValueError(f'train_lengths[{b}] = {v} is outside [0, {sep_max}] (the rows of the padded training set)')
    return tuple(lengths)


def pad_datasets(datasets):
    """[(x_b [s_b, F], y_b [s_b]), ...] -> (x [sep_max, B, F], y [sep_max, B], lengths): the datasets side by side, zero-filled behind their own rows (the values
    there reach nothing: `TransformerModel.condition(src, train_lengths)`), sep_max = the longest.  Pure tensor code, on whatever device the datasets live."""
    if len(datasets) == 0:
        raise ValueError('pad_datasets: no dataset')
    x0 = datasets[0][0]
    if x0.dim() != 2:
        raise ValueError(f'pad_datasets: x of dataset 0 has shape {tuple(x0.shape)}, expected [s, F]')
    F = x0.shape[1]
    lengths = []
    for b, (xb, yb) in enumerate(datasets):
        if xb.dim() != 2 or xb.shape[1] != F or tuple(yb.shape) != (xb.shape[0],):
            raise ValueError(f'pad_datasets: dataset {b} has x {tuple(xb.shape)} and y {tuple(yb.shape)}, expected [s, {F}] and [s]')
        lengths.append(xb.shape[0])
    sep_max = max(lengths)
    x = x0.new_zeros((sep_max, len(datasets), F))
    y = datasets[0][1].new_zeros((sep_max, len(datasets)))
    for b, (xb, yb) in enumerate(datasets):
        x[:lengths[b], b] = xb
        y[:lengths[b], b] = yb
    return x, y, tuple(lengths)


class PredictContext:
    """A conditioned training set (`TransformerModel.condition`): every layer's keys and values of the train rows in one device buffer
    (include/pfn_hip.h pfn_context_bytes), with what they were made from -- the parameter version, the descriptor, B, F, sep and the device.
    `TransformerModel.predict` refuses a context whose model has changed since.
    A ragged context (`condition(src, train_lengths)`) also carries `lengths` (host tuple, one train-row count per dataset) and `sep_of` (the same as int32 on
    the device); `sep` is then their padded maximum.  Both are None for a uniform context."""

    def __init__(self, buffer, param_version, desc_key, B, F, sep, device, lengths=None, sep_of=None):
        self.buffer, self.param_version, self.desc_key = buffer, param_version, desc_key
        self.B, self.F, self.sep, self.device = B, F, sep, device
        self.lengths, self.sep_of = lengths, sep_of

    def __repr__(self):
        ragged = '' if self.lengths is None else f', lengths {min(self.lengths)}..{max(self.lengths)}'
        return f'PredictContext(B={self.B}, F={self.F}, sep={self.sep}{ragged}, {self.buffer.numel()} bytes on {self.device})'


class TransformerModel(nn.Module):
    requires_gpu = True   # train() checks this before building anything (the host-plumbing tests substitute a CPU stand-in)
    # (Linear, CanEmb) models -- the few-shot study's -- embed on the matrix cores (hipops.class_embed); False restores the PyTorch embedding of custom encoders
    fuse_class_embedding = True

    def __init__(self, encoder, n_out, ninp, nhead, nhid, nlayers, dropout=0.0, y_encoder=None, pos_encoder=None,
                 decoder=None, input_normalization=False, precision='fp16', eval_precision='f32', deterministic=False):
        super().__init__()
        self.model_type = 'Transformer'
        self.transformer_encoder = _EncoderParams(ninp, nhid, nlayers)
        self.ninp, self.nhead, self.nhid, self.nlayers, self.n_out = ninp, nhead, nhid, nlayers, n_out
        self.dropout = dropout
        self.encoder = encoder
        self.y_encoder = y_encoder
        self.pos_encoder = pos_encoder
        # reference :23: a decoder generator replaces the default MLP.  The default runs inside the HIP stack; a custom module
        # (decoders.ScaledDecoder ...) runs in PyTorch on the encoder's test rows, which the stack then returns instead of logits.
        self._custom_decoder = decoder is not None
        self.decoder = decoder(ninp, nhid, n_out) if decoder is not None else nn.Sequential(nn.Linear(ninp, nhid), nn.GELU(), nn.Linear(nhid, n_out))
        self.input_ln = SeqBN(ninp) if input_normalization else None
        if self._fused_embedding() and encoder.in_features > _hip.MAX_FEATURES:
            raise ValueError(f'{encoder.in_features} features: the fused embedding takes at most {_hip.MAX_FEATURES} (include/pfn_hip.h num_features)')
        # `precision`: operand type of the TRAINING path ('fp16', the default and the benchmarked mode since round 6: fp16 MFMA operands under a device-side loss
        # scale, saturating stores, keys centred, pre-LayerNorm sums in fp16; 'bf16' = rounds 1-5's path, same rate; 'f32' = exact-f32 parity mode).
        # `eval_precision`: operand type of INFERENCE passes -- model.eval() under torch.no_grad(), i.e. everything that produces
        # posterior-predictive outputs (validate / run_test / criterion.mean).  Default 'f32': the same kernels on the f32 matrix
        # instructions, so the outputs match the reference's CPU path to 1e-6 where 16-bit operands leave 2e-3 (fp16) to 5e-2 (bf16) on a TRAINED model
        # (profiles/r03_trained_*.json); a forward-only pass is not the throughput path.  None = as in training.
        self.precision = precision
        self.eval_precision = eval_precision
        self._flat = self._flat_grad = self._shadow = None
        self.schedule = None               # pfn_model_desc.schedule bits (_hip.SCHED_*); None = the library's defaults at the time the model is packed
        # deterministic=True: bit-reproducible gradients (PFN_SCHED_DETERMINISTIC: one writer per gradient element and launch, ordered partial sums;
        # the micro-batch / alternating streams of train() are switched off for such a model) -- the reference's CPU loop is deterministic (train.py:58-110)
        if deterministic:
            self.schedule = _hip.SCHED_DETERMINISTIC
        self._shadow_version = None
        self._desc = None
        self._eval_desc = self._eval_shadow = self._eval_shadow_version = None
        self._first_group_hook = None      # set by dp.OverlappedGradientReducer
        self._views = []
        self.init_weights()
        # a state dict loaded into a model that has already run keeps the flat views but changes their contents
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.mark_params_updated())

    # ---- reference helpers kept for API parity (host-side, unused by the kernels) ----
    @staticmethod
    def generate_square_subsequent_mask(sz):
        allowed = torch.tril(torch.ones(sz, sz, dtype=torch.bool))
        return torch.zeros(sz, sz).masked_fill(~allowed, float('-inf'))

    @staticmethod
    def generate_D_q_matrix(sz, query_size):
        """0/-inf mask: key j visible to query i iff j < sz - query_size or i == j (reference :34-41).
        The kernels never build it -- they take the integer `single_eval_pos`."""
        train_size = sz - query_size
        allowed = torch.zeros(sz, sz, dtype=torch.bool)
        allowed[:, :train_size] = True
        allowed |= torch.eye(sz, dtype=torch.bool)
        return torch.zeros(sz, sz).masked_fill(~allowed, float('-inf'))

    @classmethod
    def _check_src_mask(cls, src_mask, T, sep):
        """An explicit `src_mask` (reference :60-65 uses it in place of the one it would build) is accepted when it IS the mask the reference builds for this
        eval position -- generate_D_q_matrix(T, T - sep), as a 0/-inf float mask or as torch's boolean `True = masked` form: that is what the kernels
        implement from the integer.  Any other mask has no kernel here and raises (no caller on the path named by north_star passes one)."""
        want = cls.generate_D_q_matrix(T, T - sep).to(src_mask.device) == 0              # True = visible
        if tuple(src_mask.shape) != (T, T):
            raise ValueError(f'src_mask has shape {tuple(src_mask.shape)}, expected ({T}, {T})')
        visible = ~src_mask if src_mask.dtype == torch.bool else src_mask == 0
        finite_ok = src_mask.dtype == torch.bool or bool(((src_mask == 0) | (src_mask == float('-inf'))).all())
        if not finite_ok or not torch.equal(visible, want):
            raise NotImplementedError('src_mask differs from generate_D_q_matrix(len(x), len(x) - single_eval_pos): the kernels implement exactly that mask '
                                      '(keys below single_eval_pos + the query itself); arbitrary additive masks are not supported')

    @property
    def deterministic(self):
        return bool((self.__dict__.get('_schedule') or 0) & _hip.SCHED_DETERMINISTIC)

    @property
    def schedule(self):
        return self.__dict__.get('_schedule')

    @schedule.setter
    def schedule(self, bits):
        # the descriptor is cached when the parameters are packed: a change of the schedule after the first forward rebuilds it (it was silently
        # ignored).  The schedule does not touch the parameter layout, so the flat buffers (and any optimizer holding them) stay as they are.
        changed = bits != self.__dict__.get('_schedule')
        self.__dict__['_schedule'] = bits
        if changed and self.__dict__.get('_flat') is not None:
            self._desc = self._make_desc()
            if self._eval_desc is not None:
                self._eval_desc = self._make_desc(self.eval_precision)

    def init_weights(self):
        """Zero the two residual-branch output projections of every layer (reference :43-53)."""
        for layer in self.transformer_encoder.layers:
            nn.init.zeros_(layer.linear2.weight)
            nn.init.zeros_(layer.linear2.bias)
            nn.init.zeros_(layer.self_attn.out_proj.weight)
            nn.init.zeros_(layer.self_attn.out_proj.bias)

    # ---- flat parameter storage ----
    def _fused_embedding(self):
        return (type(self.encoder) is nn.Linear and type(self.y_encoder) is nn.Linear and self.input_ln is None
                and (self.pos_encoder is None or isinstance(self.pos_encoder, NoPositionalEncoding)))

    def _fused_class_embedding(self):
        """True for the few-shot study's model: an nn.Linear x-encoder and a plain encoders.CanEmb over one label feature (what `get_Canonical` builds), no SeqBN,
        no positional encoding, a shape inside the limits of pfn_class_embed_* (include/pfn_hip.h) -- and `fuse_class_embedding` left True.  Such a model's
        embedding runs in csrc/class_embed.hip; its parameters stay "extras" of the flat buffers (`_flatten`)."""
        y = self.y_encoder
        return (bool(self.fuse_class_embedding) and type(self.encoder) is nn.Linear and type(y) is encoders.CanEmb and self.encoder.bias is not None
                and self.encoder.out_features == self.ninp and y.embedding_dim == self.ninp and y.padding_idx is None and y.max_norm is None
                and not y.scale_grad_by_freq and not y.sparse and self.input_ln is None
                and (self.pos_encoder is None or isinstance(self.pos_encoder, NoPositionalEncoding))
                and hipops.class_embed_supported(self.encoder.in_features, self.ninp, y.num_embeddings))

    def class_embedding_status(self):
        """(train-row labels outside [0, C), values stored saturated under fp16) counted by the class embedding's kernels since the model was built -- the one
        place that synchronises.  Such a label gets no class row and gives the table no gradient (include/pfn_hip.h pfn_class_embed_forward)."""
        status = self.__dict__.get('_class_embed_status')
        return (0, 0) if status is None else tuple(int(v) for v in status.tolist())

    def _class_embed_counters(self, device):
        status = self.__dict__.get('_class_embed_status')
        if status is None or status.device != device:      # (a plain attribute, not a buffer: the state dict stays the reference's; a moved model carries its counts along)
            status = torch.zeros(2, dtype=torch.int32, device=device) if status is None else status.to(device)
            self.__dict__['_class_embed_status'] = status
        return status

    def _stack_parameters(self):
        """Parameters in the order of pfn_param_layout (state-dict order of the reference model)."""
        ps = []
        if self._fused_embedding():
            ps += [self.encoder.weight, self.encoder.bias, self.y_encoder.weight, self.y_encoder.bias]
        else:
            ps += [None, None, None, None]
        for l in self.transformer_encoder.layers:
            ps += [l.self_attn.in_proj_weight, l.self_attn.in_proj_bias, l.self_attn.out_proj.weight, l.self_attn.out_proj.bias,
                   l.linear1.weight, l.linear1.bias, l.linear2.weight, l.linear2.bias,
                   l.norm1.weight, l.norm1.bias, l.norm2.weight, l.norm2.bias]
        if not self._custom_decoder:
            ps += [self.decoder[0].weight, self.decoder[0].bias, self.decoder[2].weight, self.decoder[2].bias]
        return ps

    def _make_desc(self, precision=None):
        nf = self.encoder.in_features if self._fused_embedding() else 1
        prec = _hip.PRECISIONS[precision or self.precision]
        # schedule: the library's defaults (0) unless a test / profiling run changed them (pfn_set_tuning) or the model carries its own bits; fixed per
        # descriptor, so a forward and the backward that reads its workspace always agree about the buffer layout (ABI 6)
        sched = getattr(self, 'schedule', None)       # (a model pickled whole before ABI 6 has no such attribute: ADVICE r4)
        schedule = sched if sched is not None else _hip.lib().pfn_default_schedule()
        return _hip.ModelDesc(nf, self.ninp, self.nhead, self.nhid, self.nlayers, 0 if self._custom_decoder else self.n_out, prec, 1e-5, float(self.dropout or 0.0), schedule)

    def _is_flat(self):
        if self._flat is None:
            return False
        stack = [p for p in self._stack_parameters() if p is not None]
        first, last = stack[0], stack[-1]
        lo, hi = self._flat.data_ptr(), self._flat.data_ptr() + self._flat.numel() * 4
        return all(p.is_cuda and p.device == self._flat.device and lo <= p.data_ptr() < hi for p in (first, last))

    def _flatten(self, device):
        """(Re)pack every parameter into one flat f32 buffer; parameters become views of it."""
        lib = _hip.lib()
        desc = self._make_desc()
        n = _hip.check(lib.pfn_param_layout(ctypes.byref(desc), None, None, 0), 'pfn_param_layout')
        offs = (ctypes.c_int64 * n)()
        nums = (ctypes.c_int64 * n)()
        _hip.check(lib.pfn_param_layout(ctypes.byref(desc), offs, nums, n), 'pfn_param_layout')
        stack = self._stack_parameters()
        assert len(stack) == n
        total = lib.pfn_param_count(ctypes.byref(desc))
        placed = {id(p) for p in stack if p is not None}
        extras, cursor = [], total
        for p in self.parameters():
            if id(p) not in placed:
                extras.append((p, cursor))
                placed.add(id(p))
                cursor = (cursor + p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        flat = torch.zeros(cursor, dtype=torch.float32, device=device)
        grad = torch.zeros(cursor, dtype=torch.float32, device=device)
        with torch.no_grad():
            for p, off, num in list(zip(stack, offs, nums)) + [(p, o, p.numel()) for p, o in extras]:
                if p is None:
                    continue
                assert p.numel() == num, f'parameter of {p.numel()} elements does not fit its slot of {num}'
                old_grad = p.grad
                flat[off:off + num].copy_(p.detach().reshape(-1).to(device))
                p.data = flat[off:off + num].view(p.shape)
                if old_grad is not None:
                    grad[off:off + num].copy_(old_grad.reshape(-1).to(device))
                p.grad = grad[off:off + num].view(p.shape)
        self._flat, self._flat_grad, self._desc = flat, grad, desc
        self._views = [(p, off, num) for p, off, num in list(zip(stack, offs, nums)) + [(p, o, p.numel()) for p, o in extras] if p is not None]
        self._stack_numel = total
        self._shadow = torch.empty(lib.pfn_shadow_bytes(ctypes.byref(desc)), dtype=torch.uint8, device=device)
        self._shadow_version = None
        self._eval_desc = self._eval_shadow = self._eval_shadow_version = None
        if self.eval_precision not in (None, self.precision) and self._make_desc(self.eval_precision).precision != desc.precision:
            self._eval_desc = self._make_desc(self.eval_precision)        # its operand copies are allocated at the first inference pass
            if lib.pfn_shadow_bytes(ctypes.byref(self._eval_desc)) < 0:   # shape outside that precision's kernels:
                self._eval_desc = None                                    # inference then runs in the training precision

    def _attach_grads(self):
        """Point every .grad at its slice of the flat gradient buffer (after zero_grad(set_to_none=True)
        the buffer is cleared first, so stale values are not re-used)."""
        first = self._views[0][0]
        if first.grad is not None and first.grad.data_ptr() == self._flat_grad.data_ptr() + self._views[0][1] * 4:
            return
        if first.grad is None:
            self._flat_grad.zero_()
        for p, off, num in self._views:
            if p.grad is not None and p.grad.data_ptr() != self._flat_grad.data_ptr() + off * 4:
                self._flat_grad[off:off + num].add_(p.grad.reshape(-1))
            p.grad = self._flat_grad[off:off + num].view(p.shape)

    def mark_params_updated(self):
        """Called by whoever writes the parameters behind autograd's back: optimizers that update the flat buffer
        through raw pointers (FusedClipAdam), or code that assigns through `p.data` (which bumps no version counter)."""
        self._shadow_version = None
        self._eval_shadow_version = None
        self._param_updates = getattr(self, '_param_updates', 0) + 1      # (what a PredictContext compares: writes through raw pointers bump no version)

    def _param_version(self):
        """Every Parameter is a view of the flat buffer with its OWN version counter (`p.data = flat[...]` detaches
        it from the buffer's), so in-place updates through the parameters -- `load_state_dict`, `torch.optim.*`,
        `p.copy_()` -- are only visible there; updates of the flat buffer itself only on the buffer."""
        return (self._flat._version, sum(p._version for p, _, _ in self._views))

    def _refresh_shadow(self, stream):
        version = self._param_version()
        if self._shadow_version != version:
            _hip.check(_hip.lib().pfn_prepare_params(ctypes.byref(self._desc), self._flat.data_ptr(), self._shadow.data_ptr(), stream),
                       'pfn_prepare_params')
            self._shadow_version = version

    def _inference_pass(self):
        """True when this forward produces outputs only (eval mode, autograd off) and a separate inference precision is configured.
        Must be evaluated in `forward`, OUTSIDE the autograd Function (inside `Function.forward` grad mode is always off): an eval-mode
        forward that is differentiated afterwards (fine-tuning under eval(), input gradients) has to run the training-precision
        kernels, whose workspace layout the backward reads."""
        return self._eval_desc is not None and not self.training and not torch.is_grad_enabled()

    def _operands(self, stream, inference):
        """(model descriptor, operand copies of the weights) of a pass, refreshed if the parameters changed."""
        if not inference:
            self._refresh_shadow(stream)
            return self._desc, self._shadow
        lib = _hip.lib()
        if self._eval_shadow is None:
            self._eval_shadow = torch.empty(lib.pfn_shadow_bytes(ctypes.byref(self._eval_desc)), dtype=torch.uint8, device=self._flat.device)
        version = self._param_version()
        if self._eval_shadow_version != version:
            _hip.check(lib.pfn_prepare_params(ctypes.byref(self._eval_desc), self._flat.data_ptr(), self._eval_shadow.data_ptr(), stream), 'pfn_prepare_params')
            self._eval_shadow_version = version
        return self._eval_desc, self._eval_shadow

    def _next_dropout_seed(self):
        """A fresh 64-bit seed per training pass, derived from torch's global seed (rank-distinct under data parallelism) and a counter."""
        self._dropout_calls = getattr(self, '_dropout_calls', 0) + 1
        self._last_dropout_seed = (torch.initial_seed() * 0x9E3779B97F4A7C15 + self._dropout_calls * 0xD1B54A32D192ED03) & (2 ** 64 - 1)
        return self._last_dropout_seed

    def layer_offset(self, layer):
        """Offset (in elements) of encoder layer `layer`'s first parameter in the flat buffers: everything from there to the end of the
        buffer belongs to that layer, the layers above it and the decoder (state-dict order)."""
        self.flat_parameters()
        first = self.transformer_encoder.layers[layer].self_attn.in_proj_weight
        return next(off for p, off, _ in self._views if p is first)

    def flat_parameters(self):
        """(flat f32 parameter buffer, flat f32 gradient buffer); packs the model on first use."""
        if not self._is_flat():
            dev = next(self.parameters()).device
            _hip.require_gpu_tensor(next(self.parameters()), 'model parameters')
            self._flatten(dev)
        self._attach_grads()
        return self._flat, self._flat_grad

    # ---- several micro-batches in one launch set ----
    def can_forward_batches(self):
        return self._fused_embedding() and not self._custom_decoder

    def forward_batches(self, batches, single_eval_positions):
        """`model((x_k, y_k), single_eval_pos=sep_k)` for several batches at once: batches = [(x_k[T, b_k, F], y_k[T, b_k]), ...] with one T, one eval position
        per batch.  Returns the list of logits [T - sep_k, b_k, n_out] -- the tensors the separate calls would return -- from ONE launch set in which every
        dataset carries its own eval position (pfn_stack_forward_ragged).  The reference runs the k batches of an optimizer step one after the other
        (train.py:66-97); a batch of 4 datasets fills a fraction of the chip.  Losses formed per batch and summed give the reference's accumulated gradient."""
        assert self.can_forward_batches(), 'forward_batches needs the built-in linear encoders and decoder'
        assert len(batches) == len(single_eval_positions) and len(batches) > 0
        x = torch.cat([b[0] for b in batches], 1)
        y = torch.cat([b[1].to(x.device) for b in batches], 1)
        _hip.require_gpu_tensor(x, 'x')
        _hip.require_gpu_tensor(next(self.parameters()), 'model parameters')
        T = x.shape[0]
        for xb, _ in batches:
            assert xb.shape[0] == T, 'forward_batches: every batch needs the same sequence length'
        widths = [xb.shape[1] for xb, _ in batches]
        seps, per_dataset, offs = ragged_layout(T, widths, single_eval_positions)
        meta = torch.tensor(per_dataset + offs, dtype=torch.int64)          # one host-to-device copy for both arrays
        sep_of = meta[:len(per_dataset)].to(torch.int32).to(x.device, non_blocking=True)
        row_off = meta[len(per_dataset):].to(x.device, non_blocking=True)
        if not self._is_flat():
            self._flatten(x.device)
        flat = self._flat
        inference = self._inference_pass()
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            flat = flat.detach().requires_grad_(True)
        logits = _StackFunction.apply(flat, self, x, y, None, max(seps), inference, (sep_of, row_off, min(seps), max(seps), offs[-1]))
        # (torch.split: its backward is ONE concatenation of the per-batch gradients; slicing would zero-fill and add a full-size tensor per batch)
        parts = torch.split(logits, [w * (T - sep) for sep, w in zip(seps, widths)])
        return [p.view(w, T - sep, logits.shape[1]).transpose(0, 1) for p, sep, w in zip(parts, seps, widths)]      # dataset-major rows -> the reference's [T - sep, b, n_out]

    # ---- condition once, predict many ----
    _PREDICT_ROWS = 1 << 15      # rows (test rows x datasets) per pfn_stack_predict call: bounds its workspace, any n is chunked to it

    def _check_predict_model(self):
        if self.pos_encoder is not None and not isinstance(self.pos_encoder, NoPositionalEncoding):
            raise NotImplementedError('condition / predict: a positional encoding makes a row\'s output depend on its index in the sequence, so cached train rows '
                                      'cannot serve test rows at other positions')
        if self.input_ln is not None:
            raise NotImplementedError('condition / predict: SeqBN normalises over the whole sequence, so the train rows\' activations depend on the test rows')
        if not self._fused_embedding():
            raise NotImplementedError('condition / predict need the fused embedding (Linear x / y encoders, no positional encoding, no SeqBN)')

    def _predict_operands(self, stream):
        if not self._is_flat():
            self._flatten(next(self.parameters()).device)
        return self._operands(stream, self._eval_desc is not None)      # eval_precision when the model has one, else precision (as an inference forward)

    def _predict_version(self):
        return (self._param_version(), getattr(self, '_param_updates', 0))

    @torch.no_grad()
    def condition(self, src, train_lengths=None):
        """Run the training set src = (x_train [sep, B, F], y_train [sep, B]) once and keep every layer's keys and values: the returned PredictContext
        serves any number of `predict` calls (pfn_stack_condition).

        train_lengths (a sequence or integer tensor [B], 0 <= value <= sep): dataset b has only its first train_lengths[b] rows; the rows behind them are padding
        whose values reach no output (pfn_stack_condition_ragged).  Column b of every later `predict` is then what the dataset's own rows alone would give --
        tabular tasks or optimisation runs of different sizes as one batch, instead of one B = 1 call each."""
        self._check_predict_model()
        x, y = src
        lengths = None if train_lengths is None else check_train_lengths(train_lengths, x.shape[1], x.shape[0])
        _hip.require_gpu_tensor(x, 'x')
        _hip.require_gpu_tensor(next(self.parameters()), 'model parameters')
        sep, B, F = x.shape
        y = y.to(x.device)
        if x.dtype != torch.float32 or x.stride(-1) != 1:
            x = x.float().contiguous()
        if y.dtype != torch.float32:
            y = y.float()
        lib = _hip.lib()
        stream = _hip.stream_ptr(x.device)
        desc, shadow = self._predict_operands(stream)
        nbytes = _hip.check(lib.pfn_context_bytes(ctypes.byref(desc), B, sep), 'pfn_context_bytes')
        buf = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        if lengths is not None:
            sep_of = torch.tensor(lengths, dtype=torch.int32).to(x.device)
            if sep > 0:
                ws_bytes = _hip.check(lib.pfn_workspace_bytes(ctypes.byref(desc), B, sep), 'pfn_workspace_bytes')
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
                _hip.check(lib.pfn_stack_condition_ragged(ctypes.byref(desc), self._flat.data_ptr(), shadow.data_ptr(), x.data_ptr(), x.stride(0), x.stride(1),
                                                          y.data_ptr(), y.stride(0), y.stride(1), B, sep, sep_of.data_ptr(), ws.data_ptr(), ws_bytes,
                                                          buf.data_ptr(), nbytes, stream), 'pfn_stack_condition_ragged')
            return PredictContext(buf, self._predict_version(), desc.key(), B, F, sep, x.device, lengths, sep_of)
        if sep > 0:
            ws_bytes = _hip.check(lib.pfn_workspace_bytes(ctypes.byref(desc), B, sep), 'pfn_workspace_bytes')
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
            _hip.check(lib.pfn_stack_condition(ctypes.byref(desc), self._flat.data_ptr(), shadow.data_ptr(), x.data_ptr(), x.stride(0), x.stride(1),
                                               y.data_ptr(), y.stride(0), y.stride(1), B, sep, ws.data_ptr(), ws_bytes, buf.data_ptr(), nbytes, stream),
                       'pfn_stack_condition')
        return PredictContext(buf, self._predict_version(), desc.key(), B, F, sep, x.device)

    def condition_datasets(self, datasets):
        """`condition` for datasets of different sizes given one by one: [(x_b [s_b, F], y_b [s_b]), ...] on the model's device, zero-padded to the longest
        (`pad_datasets`) and conditioned with their own lengths."""
        x, y, lengths = pad_datasets(datasets)
        return self.condition((x, y), train_lengths=lengths)

    def predict(self, context, x_test):
        """Posterior-predictive logits [n, B, n_out] of the test rows x_test [n, B, F] given the conditioned training set: what model.eval() under
        torch.no_grad() returns for model((cat(x_train, x_test), cat(y_train, anything)), single_eval_pos=sep), computed from the cached keys and values
        (pfn_stack_predict).  Rows are independent; any n, in chunks of the caller's choosing.

        Differentiable in x_test: with grad mode on and x_test.requires_grad, every chunk keeps its layers' test-row activations
        (pfn_stack_predict_saved) and the output's backward is pfn_stack_predict_backward -- what botorch's optimize_acqf needs of an acquisition
        function built on the PFN (reference acquisition_functions.py).  Gradients go to x_test ONLY: the parameters get none, and neither do the
        train rows behind the context (both are constants of the cached keys and values).  The kept workspace is linear in nlayers and independent
        of sep: about 1.8 GB in fp16 and 2.9 GB in f32 for 256 test rows x 64 datasets of the configs[1] model (emsize 512, nhid 1024, 6 layers).
        Otherwise (grad mode off, or x_test not requiring grad) the pass is the plain pfn_stack_predict and nothing is kept."""
        if not (torch.is_grad_enabled() and x_test.requires_grad):
            with torch.no_grad():
                return self._predict(context, x_test, False)
        return self._predict(context, x_test, True)

    def _predict(self, context, x_test, grad):
        self._check_predict_model()
        _hip.require_gpu_tensor(x_test, 'x_test')
        _hip.require_gpu_tensor(next(self.parameters()), 'model parameters')
        n, B, F = x_test.shape
        if (B, F) != (context.B, context.F):
            raise ValueError(f'predict: x_test has B={B}, F={F}; the context was conditioned on B={context.B}, F={context.F}')
        if x_test.device != context.device:
            raise ValueError(f'predict: x_test is on {x_test.device}, the context on {context.device}')
        lib = _hip.lib()
        stream = _hip.stream_ptr(x_test.device)
        if not self._is_flat() or self._predict_version() != context.param_version:
            raise RuntimeError('predict: the model parameters changed after condition() (optimizer step, load_state_dict, mark_params_updated); condition again')
        desc, shadow = self._predict_operands(stream)
        if desc.key() != context.desc_key:
            raise RuntimeError('predict: the model descriptor (precision / schedule) changed after condition(); condition again')
        if x_test.dtype != torch.float32 or x_test.stride(-1) != 1:
            x_test = x_test.float().contiguous()
        if grad and n > 0:      # one autograd node per chunk, each with its saved workspace
            chunk = max(1, self._PREDICT_ROWS // B)
            parts = [_PredictFunction.apply(x_test[t0:t0 + chunk], self, context, desc, shadow) for t0 in range(0, n, chunk)]
            out = parts[0] if len(parts) == 1 else torch.cat(parts, 0)
            return self.decoder(out) if self._custom_decoder else out
        width = desc.n_out or desc.emsize
        out = torch.empty((n, B, width), dtype=torch.float32, device=x_test.device)
        chunk = max(1, self._PREDICT_ROWS // B)
        ws = None
        for t0 in range(0, n, chunk):
            m = min(chunk, n - t0)
            ws_bytes = _hip.check(lib.pfn_predict_workspace_bytes(ctypes.byref(desc), B, m), 'pfn_predict_workspace_bytes')
            if ws is None or ws.numel() < ws_bytes:
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x_test.device)
            xc = x_test[t0:t0 + m]
            if context.lengths is not None:
                _hip.check(lib.pfn_stack_predict_ragged(ctypes.byref(desc), self._flat.data_ptr(), shadow.data_ptr(), context.buffer.data_ptr(),
                                                        context.buffer.numel(), context.sep, context.sep_of.data_ptr(), xc.data_ptr(), xc.stride(0), xc.stride(1),
                                                        B, m, ws.data_ptr(), ws.numel(), out[t0:t0 + m].data_ptr(), stream), 'pfn_stack_predict_ragged')
            else:
                _hip.check(lib.pfn_stack_predict(ctypes.byref(desc), self._flat.data_ptr(), shadow.data_ptr(), context.buffer.data_ptr(), context.buffer.numel(),
                                                 context.sep, xc.data_ptr(), xc.stride(0), xc.stride(1), B, m, ws.data_ptr(), ws.numel(), out[t0:t0 + m].data_ptr(),
                                                 stream), 'pfn_stack_predict')
        return self.decoder(out) if self._custom_decoder else out

    # ---- forward ----
    def forward(self, src, src_mask=None, single_eval_pos=None):
        assert single_eval_pos is not None, 'Single eval pos is required now.'
        assert isinstance(src, tuple), 'pass src as an (x, y) tuple together with single_eval_pos (the fuse_x_y path of the reference is dead code: transformer.py:56-59)'
        x_src, y_src = src
        _hip.require_gpu_tensor(x_src, 'x')
        _hip.require_gpu_tensor(next(self.parameters()), 'model parameters')
        T = x_src.shape[0]
        sep = int(single_eval_pos)
        if sep < 0:
            sep += T  # negative positions work through slicing in the reference
        sep = max(0, min(T, sep))
        if src_mask is not None:
            self._check_src_mask(src_mask, T, sep)
        if not self._is_flat():
            self._flatten(x_src.device)
        flat = self._flat
        inference = self._inference_pass()
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            flat = flat.detach().requires_grad_(True)  # connects the node to autograd; grads go to the flat buffer directly
        if self._fused_embedding():
            out = _StackFunction.apply(flat, self, x_src, y_src.to(x_src.device), None, sep, inference)
            return self.decoder(out) if self._custom_decoder else out
        if self._fused_class_embedding() and not (torch.is_grad_enabled() and x_src.requires_grad):
            # (Linear, CanEmb): the embedding as one GEMM on the matrix cores, its gradients accumulated into the flat gradient buffer (csrc/class_embed.hip); in the
            # precision of the pass, as the stack.  An x that asks for its own gradient keeps the PyTorch embedding below.
            prec = self.eval_precision if inference else self.precision
            emb = hipops.class_embed(x_src, y_src.to(x_src.device), self.encoder.weight, self.encoder.bias, self.y_encoder.weight, sep, prec,
                                     deterministic=self.deterministic, status=self._class_embed_counters(x_src.device), _model=self)
            out = _StackFunction.apply(flat, self, None, None, emb, sep, inference)
            return self.decoder(out) if self._custom_decoder else out
        # custom encoders / positional encodings / SeqBN: PyTorch computes the embedding, HIP runs the stack
        x_emb = self.encoder(x_src)
        y_emb = self.y_encoder(y_src.unsqueeze(-1))
        emb = torch.cat([x_emb[:sep] + y_emb[:sep], x_emb[sep:]], 0)
        if self.input_ln is not None:
            emb = self.input_ln(emb)
        if self.pos_encoder is not None:
            emb = self.pos_encoder(emb)
        out = _StackFunction.apply(flat, self, None, None, emb, sep, inference)
        return self.decoder(out) if self._custom_decoder else out
