"""Host-side checks of condition once / predict many (include/pfn_hip.h, ABI 9): the context and workspace sizes, the argument checks that return before
anything is launched, and the models the split into two calls refuses.  No GPU needed."""
import ctypes

import pytest
import torch

from transformerscandobayesianinference_amd import _hip, encoders, positional_encodings
from transformerscandobayesianinference_amd.transformer import TransformerModel


def _desc(precision, emsize=128, nhead=4, nlayers=2, schedule=0, n_out=100):
    return _hip.ModelDesc(5, emsize, nhead, 256, nlayers, n_out, precision, 1e-5, 0.0, schedule)


def _align(v):
    return (v + 255) // 256 * 256


def _formula(d, B, sep):
    es = 4 if d.precision == _hip.PREC_F32 else 2
    centred = d.emsize % 64 == 0 and ((d.precision == _hip.PREC_FP16 and not d.schedule & _hip.SCHED_NO_KEY_CENTERING) or
                                      (d.precision == _hip.PREC_BF16 and d.schedule & _hip.SCHED_KEY_CENTERING))
    if sep == 0:
        return 0
    return d.nlayers * (_align(B * sep * 2 * d.emsize * es) + (_align(B * d.emsize * 4) if centred else 0))


@pytest.mark.parametrize('precision,schedule,centred', [
    (_hip.PREC_F32, 0, False),
    (_hip.PREC_BF16, 0, False),
    (_hip.PREC_BF16, _hip.SCHED_KEY_CENTERING, True),
    (_hip.PREC_FP16, 0, True),
    (_hip.PREC_FP16, _hip.SCHED_NO_KEY_CENTERING, False),
])
def test_context_bytes_follow_the_layout(precision, schedule, centred):
    lib = _hip.lib()
    for B, sep, nlayers in [(1, 1, 1), (3, 437, 2), (64, 2000, 6), (2, 0, 3)]:
        d = _desc(precision, nlayers=nlayers, schedule=schedule)
        got = lib.pfn_context_bytes(ctypes.byref(d), B, sep)
        assert got == _formula(d, B, sep), (precision, schedule, B, sep, nlayers, got)
        es = 4 if precision == _hip.PREC_F32 else 2
        if sep > 0:      # the formula's two parts: the K | V rows, and the key shift exactly when the keys are centred
            assert got == nlayers * (_align(B * sep * 2 * 128 * es) + (_align(B * 128 * 4) if centred else 0))
    assert lib.pfn_context_bytes(ctypes.byref(_desc(precision)), 0, 10) < 0
    assert lib.pfn_context_bytes(ctypes.byref(_desc(precision)), 1, -1) < 0


def test_predict_workspace_does_not_grow_with_depth():
    lib = _hip.lib()
    for precision in (_hip.PREC_F32, _hip.PREC_BF16, _hip.PREC_FP16):
        for B, n in [(1, 1), (1, 16), (64, 256), (1, 2048), (8, 300)]:
            sizes = {lib.pfn_predict_workspace_bytes(ctypes.byref(_desc(precision, emsize=512, nlayers=L)), B, n) for L in (1, 2, 6, 12)}
            assert len(sizes) == 1 and min(sizes) > 0, (precision, B, n, sizes)
        # ... and per row it is a small fraction of the training workspace a full forward at sep + n rows carves
        d = _desc(precision, emsize=512, nlayers=6)
        assert lib.pfn_predict_workspace_bytes(ctypes.byref(d), 64, 256) * 4 < lib.pfn_workspace_bytes(ctypes.byref(d), 64, 256)


def test_argument_errors_return_before_any_launch():
    """Every case below is refused by host-side checks: the pointers are never dereferenced (nothing runs on a device here)."""
    lib = _hip.lib()
    d = _desc(_hip.PREC_FP16)
    B, sep, n = 2, 100, 7
    fake = 4096       # a non-NULL address that is never touched
    ctx_bytes = lib.pfn_context_bytes(ctypes.byref(d), B, sep)
    ws_c = lib.pfn_workspace_bytes(ctypes.byref(d), B, sep)
    ws_p = lib.pfn_predict_workspace_bytes(ctypes.byref(d), B, n)
    assert ctx_bytes > 0 and ws_c > 0 and ws_p > 0

    def condition(ctx=fake, nbytes=ctx_bytes, B=B, sep=sep, ws_bytes=ws_c):
        return lib.pfn_stack_condition(ctypes.byref(d), fake, fake, fake, B, 1, fake, B, 1, B, sep, fake, ws_bytes, ctx, nbytes, None)

    def predict(ctx=fake, nbytes=ctx_bytes, B=B, n=n, sep=sep, ws_bytes=ws_p, x=fake, logits=fake):
        return lib.pfn_stack_predict(ctypes.byref(d), fake, fake, ctx, nbytes, sep, x, B * 5, 5, B, n, fake, ws_bytes, logits, None)

    ERR = -4      # PFN_ERR_ARGUMENT
    assert condition(ctx=None) == ERR                       # NULL context with sep > 0
    assert condition(nbytes=ctx_bytes - 1) == ERR           # context smaller than pfn_context_bytes
    assert condition(B=0) == ERR and condition(sep=-1) == ERR
    assert condition(ws_bytes=ws_c - 1) == ERR              # the train rows' forward workspace
    assert predict(ctx=None) == ERR
    assert predict(nbytes=ctx_bytes - 1) == ERR
    assert predict(B=0) == ERR and predict(n=-1) == ERR and predict(sep=-1) == ERR
    assert predict(ws_bytes=ws_p - 1) == ERR
    assert predict(x=None) == ERR and predict(logits=None) == ERR
    # sep = 0: no context at all, and nothing to condition
    assert lib.pfn_context_bytes(ctypes.byref(d), B, 0) == 0
    assert lib.pfn_stack_condition(ctypes.byref(d), fake, fake, fake, B, 1, fake, B, 1, B, 0, fake, ws_c, None, 0, None) == 0
    assert predict(ctx=None, nbytes=0, sep=0, n=0) == 0     # n = 0: nothing to do


def _model(pos_encoder=None, input_normalization=False):
    F, E = 5, 64
    return TransformerModel(encoders.Linear(F, E), 10, E, 4, 128, 2, y_encoder=encoders.Linear(1, E), pos_encoder=pos_encoder,
                            input_normalization=input_normalization)


def test_condition_and_predict_refuse_sequence_dependent_models():
    x, y = torch.rand(20, 2, 5), torch.rand(20, 2)
    m = _model(pos_encoder=positional_encodings.PositionalEncoding(64))
    with pytest.raises(NotImplementedError, match='positional encoding'):
        m.condition((x, y))
    with pytest.raises(NotImplementedError, match='positional encoding'):
        m.predict(None, x)
    m = _model(input_normalization=True)
    with pytest.raises(NotImplementedError, match='SeqBN'):
        m.condition((x, y))
    with pytest.raises(NotImplementedError, match='SeqBN'):
        m.predict(None, x)


def test_condition_refuses_cpu_tensors():
    m = _model()
    with pytest.raises(_hip.HipExtensionError):
        m.condition((torch.rand(20, 2, 5), torch.rand(20, 2)))
