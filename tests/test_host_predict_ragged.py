"""Host-side checks of condition / predict with a different training-set size per dataset (include/pfn_hip.h: the four pfn_stack_*_ragged entry points, ABI 10
additive): the argument checks that return before anything is launched, the padding helper and the validation of `train_lengths`.  No GPU needed."""
import ctypes

import pytest
import torch

from transformerscandobayesianinference_amd import _hip
from transformerscandobayesianinference_amd.transformer import check_train_lengths, pad_datasets

ERR = -4      # PFN_ERR_ARGUMENT
FAKE = 4096   # a non-NULL address that is never touched


def _desc(precision, emsize=128, nhead=4, nlayers=2, schedule=0, n_out=100):
    return _hip.ModelDesc(5, emsize, nhead, 256, nlayers, n_out, precision, 1e-5, 0.0, schedule)


@pytest.mark.parametrize('precision', [_hip.PREC_FP16, _hip.PREC_F32])
def test_argument_errors_return_before_any_launch(precision):
    """Every case below is refused by host-side checks: the pointers are never dereferenced (nothing runs on a device here)."""
    lib = _hip.lib()
    d = _desc(precision)
    B, sep_max, n = 2, 100, 7
    ctx_bytes = lib.pfn_context_bytes(ctypes.byref(d), B, sep_max)
    ws_c = lib.pfn_workspace_bytes(ctypes.byref(d), B, sep_max)
    ws_p = lib.pfn_predict_workspace_bytes(ctypes.byref(d), B, n)
    ws_g = lib.pfn_predict_grad_workspace_bytes(ctypes.byref(d), B, n)
    assert ctx_bytes > 0 and ws_c > 0 and ws_p > 0 and ws_g > 0

    def condition(ctx=FAKE, nbytes=ctx_bytes, B=B, sep_max=sep_max, sep_of=FAKE, ws_bytes=ws_c):
        return lib.pfn_stack_condition_ragged(ctypes.byref(d), FAKE, FAKE, FAKE, B, 1, FAKE, B, 1, B, sep_max, sep_of, FAKE, ws_bytes, ctx, nbytes, None)

    def predict(fn, ws_full, ctx=FAKE, nbytes=ctx_bytes, B=B, n=n, sep_max=sep_max, sep_of=FAKE, ws_bytes=None):
        return fn(ctypes.byref(d), FAKE, FAKE, ctx, nbytes, sep_max, sep_of, FAKE, B * 5, 5, B, n, FAKE, ws_full if ws_bytes is None else ws_bytes, FAKE, None)

    def backward(ctx=FAKE, nbytes=ctx_bytes, B=B, n=n, sep_max=sep_max, sep_of=FAKE, ws_bytes=ws_g):
        return lib.pfn_stack_predict_backward_ragged(ctypes.byref(d), FAKE, FAKE, ctx, nbytes, sep_max, sep_of, B, n, FAKE, ws_bytes, FAKE, FAKE, B * 5, 5, None)

    assert condition(sep_of=None) == ERR                    # NULL sep_of
    assert condition(B=0) == ERR and condition(sep_max=-1) == ERR
    assert condition(nbytes=ctx_bytes - 1) == ERR           # context one byte short
    assert condition(ws_bytes=ws_c - 1) == ERR              # workspace one byte short
    assert condition(ctx=None) == ERR                       # NULL context with sep_max > 0
    for fn, ws_full in ((lib.pfn_stack_predict_ragged, ws_p), (lib.pfn_stack_predict_saved_ragged, ws_g)):
        assert predict(fn, ws_full, sep_of=None) == ERR
        assert predict(fn, ws_full, B=0) == ERR and predict(fn, ws_full, sep_max=-1) == ERR and predict(fn, ws_full, n=-1) == ERR
        assert predict(fn, ws_full, nbytes=ctx_bytes - 1) == ERR
        assert predict(fn, ws_full, ws_bytes=ws_full - 1) == ERR
        assert predict(fn, ws_full, ctx=None) == ERR
        assert predict(fn, ws_full, n=0) == 0                                     # n = 0: nothing to do
        assert predict(fn, ws_full, ctx=None, nbytes=0, sep_max=0, n=0) == 0      # sep_max = 0: no context at all
    assert backward(sep_of=None) == ERR
    assert backward(B=0) == ERR and backward(sep_max=-1) == ERR and backward(n=-1) == ERR
    assert backward(nbytes=ctx_bytes - 1) == ERR
    assert backward(ws_bytes=ws_g - 1) == ERR
    assert backward(ctx=None) == ERR
    assert backward(n=0) == 0
    assert backward(ctx=None, nbytes=0, sep_max=0, n=0) == 0
    # sep_max = 0: nothing to condition, as the uniform call at sep = 0
    assert condition(ctx=None, nbytes=0, sep_max=0) == 0


def test_pad_datasets():
    g = torch.Generator().manual_seed(0)
    sizes = [5, 0, 9, 1]
    datasets = [(torch.randn(s, 3, generator=g), torch.randn(s, generator=g)) for s in sizes]
    x, y, lengths = pad_datasets(datasets)
    assert lengths == tuple(sizes)
    assert x.shape == (9, 4, 3) and y.shape == (9, 4) and x.dtype == torch.float32
    for b, (xb, yb) in enumerate(datasets):
        assert torch.equal(x[:sizes[b], b], xb) and torch.equal(y[:sizes[b], b], yb)
        assert not x[sizes[b]:, b].any() and not y[sizes[b]:, b].any()      # zero fill behind the dataset's own rows
    # every dataset empty: sep_max = 0
    x, y, lengths = pad_datasets([(torch.zeros(0, 3), torch.zeros(0))] * 2)
    assert x.shape == (0, 2, 3) and y.shape == (0, 2) and lengths == (0, 0)
    with pytest.raises(ValueError):
        pad_datasets([])
    with pytest.raises(ValueError):
        pad_datasets([(torch.zeros(4, 3), torch.zeros(4)), (torch.zeros(4, 2), torch.zeros(4))])      # another F
    with pytest.raises(ValueError):
        pad_datasets([(torch.zeros(4, 3), torch.zeros(5))])                                            # y of another length


def test_train_lengths_are_validated_on_the_host():
    assert check_train_lengths([3, 0, 10], 3, 10) == (3, 0, 10)
    assert check_train_lengths(torch.tensor([3, 0, 10], dtype=torch.int32), 3, 10) == (3, 0, 10)
    assert check_train_lengths((), 0, 0) == ()
    with pytest.raises(ValueError, match='entries'):
        check_train_lengths([3, 0], 3, 10)             # wrong count
    with pytest.raises(ValueError, match='outside'):
        check_train_lengths([3, -1, 10], 3, 10)        # negative
    with pytest.raises(ValueError, match='outside'):
        check_train_lengths([3, 11, 10], 3, 10)        # above sep_max
    with pytest.raises(ValueError):
        check_train_lengths(torch.tensor([1.0, 2.0, 3.0]), 3, 10)
    with pytest.raises(ValueError):
        check_train_lengths([1.5, 2, 3], 3, 10)


def test_condition_validates_train_lengths_before_touching_a_device():
    """condition(train_lengths=...) raises ValueError for bad lengths even on CPU tensors (the device check comes after)"""
    from transformerscandobayesianinference_amd import encoders
    from transformerscandobayesianinference_amd.transformer import TransformerModel
    m = TransformerModel(encoders.Linear(5, 64), 10, 64, 4, 128, 2, y_encoder=encoders.Linear(1, 64))
    x, y = torch.rand(20, 3, 5), torch.rand(20, 3)
    for bad in ([1, 2], [1, -1, 2], [1, 21, 2]):
        with pytest.raises(ValueError):
            m.condition((x, y), train_lengths=bad)
    with pytest.raises(_hip.HipExtensionError):      # valid lengths: the usual refusal of CPU tensors
        m.condition((x, y), train_lengths=[1, 20, 0])
