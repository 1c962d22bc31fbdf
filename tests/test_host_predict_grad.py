"""Host-side checks of the input-gradient entry points (include/pfn_hip.h, ABI 10): they are declared, exported and bound; the size of the predict workspace that
keeps a backward's activations; the argument checks that return before anything is launched.  No GPU needed."""
import ctypes
import os
import re

from transformerscandobayesianinference_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pfn_predict_grad_workspace_bytes', 'pfn_stack_predict_saved', 'pfn_stack_predict_backward', 'pfn_stack_input_grads', 'pfn_bar_mean_backward')
ERR = -4      # PFN_ERR_ARGUMENT


def _desc(precision, emsize=128, nhead=4, nlayers=2, n_out=100):
    return _hip.ModelDesc(5, emsize, nhead, 256, nlayers, n_out, precision, 1e-5, 0.0, 0)


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    lib = _hip.lib()
    assert _hip.ABI_VERSION == 10 and lib.pfn_abi_version() == 10
    for name in NEW:
        assert re.search(r'\b' + name + r'\(', header), name
        assert name in _hip.SIGNATURES, name
        assert hasattr(lib, name), name


def test_grad_workspace_is_linear_in_depth_and_independent_of_sep():
    lib = _hip.lib()
    for precision in (_hip.PREC_F32, _hip.PREC_BF16, _hip.PREC_FP16):
        for B, n in [(1, 1), (3, 7), (64, 256), (8, 300)]:
            sizes = [lib.pfn_predict_grad_workspace_bytes(ctypes.byref(_desc(precision, emsize=512, nlayers=L)), B, n) for L in (1, 2, 3, 6)]
            assert all(s > 0 for s in sizes), sizes
            per_layer = sizes[1] - sizes[0]
            assert per_layer > 0 and sizes[2] - sizes[1] == per_layer and sizes[3] - sizes[2] == 3 * per_layer, (precision, B, n, sizes)
            for L in (1, 6):
                d = _desc(precision, emsize=512, nlayers=L)
                assert lib.pfn_predict_grad_workspace_bytes(ctypes.byref(d), B, n) >= lib.pfn_predict_workspace_bytes(ctypes.byref(d), B, n)
        # the size takes no sep at all: the context holds the train rows
    d = _desc(_hip.PREC_FP16)
    assert lib.pfn_predict_grad_workspace_bytes(ctypes.byref(d), 0, 4) == -1
    assert lib.pfn_predict_grad_workspace_bytes(ctypes.byref(d), 2, -1) == -1
    bad = _hip.ModelDesc(5, 100, 3, 256, 2, 10, _hip.PREC_FP16, 1e-5, 0.0, 0)      # emsize not divisible by nhead
    assert lib.pfn_predict_grad_workspace_bytes(ctypes.byref(bad), 2, 4) == -1


def test_predict_backward_and_input_grads_refuse_bad_arguments_before_any_launch():
    """Every call below is refused by host checks: the pointers are never dereferenced (nothing runs on a device here)."""
    lib = _hip.lib()
    d = _desc(_hip.PREC_FP16)
    B, sep, n, S = 2, 100, 7, 50
    fake = 4096
    ctx_bytes = lib.pfn_context_bytes(ctypes.byref(d), B, sep)
    ws_g = lib.pfn_predict_grad_workspace_bytes(ctypes.byref(d), B, n)
    ws_t = lib.pfn_workspace_bytes(ctypes.byref(d), B, S)
    assert ctx_bytes > 0 and ws_g > 0 and ws_t > 0

    def backward(ctx=fake, nbytes=ctx_bytes, B=B, n=n, sep=sep, ws_bytes=ws_g, dlogits=fake, dx=fake):
        return lib.pfn_stack_predict_backward(ctypes.byref(d), fake, fake, ctx, nbytes, sep, B, n, fake, ws_bytes, dlogits, dx, B * 5, 5, None)

    def saved(ctx=fake, nbytes=ctx_bytes, ws_bytes=ws_g, x=fake):
        return lib.pfn_stack_predict_saved(ctypes.byref(d), fake, fake, ctx, nbytes, sep, x, B * 5, 5, B, n, fake, ws_bytes, fake, None)

    def input_grads(ws_bytes=ws_t, dx=fake, S=S, sep=30):
        return lib.pfn_stack_input_grads(ctypes.byref(d), fake, B, S, sep, fake, ws_bytes, dx, B * 5, 5, fake, B, 1, None)

    assert backward(ws_bytes=ws_g - 1) == ERR                 # short workspace
    assert backward(ws_bytes=lib.pfn_predict_workspace_bytes(ctypes.byref(d), B, n)) == ERR      # the plain predict workspace is not enough
    assert backward(dx=None) == ERR and backward(dlogits=None) == ERR
    assert backward(nbytes=ctx_bytes - 1) == ERR and backward(ctx=None) == ERR
    assert backward(B=0) == ERR and backward(n=-1) == ERR and backward(sep=-1) == ERR
    assert backward(ctx=None, nbytes=0, sep=0, n=0) == 0      # n = 0: nothing to do
    assert saved(ws_bytes=ws_g - 1) == ERR and saved(x=None) == ERR and saved(nbytes=ctx_bytes - 1) == ERR
    assert input_grads(ws_bytes=ws_t - 1) == ERR
    assert input_grads(dx=None) == ERR
    assert input_grads(sep=S + 1) == ERR and input_grads(S=0) == ERR
    assert lib.pfn_bar_mean_backward(None, 10, fake, 4, 10, 0, fake, fake, fake, None) == ERR
    assert lib.pfn_bar_mean_backward(fake, 10, fake, 4, 10, 0, fake, fake, None, None) == ERR
