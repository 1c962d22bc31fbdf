"""Host-side checks of the class-label embedding (csrc/class_embed.hip, hipops.class_embed, TransformerModel._fused_class_embedding): the C ABI and the build,
the torch restatement (tests/class_embed_f64.py) against torch's own modules under autograd, the kernels' descriptor budgets, which models take the path, and the
argument checks that must answer without a GPU.  No GPU."""
import os
import re
import sys

import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_embed_f64 as R      # noqa: E402

from transformerscandobayesianinference_amd import _hip, encoders, hipops, positional_encodings      # noqa: E402
from transformerscandobayesianinference_amd.transformer import TransformerModel      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc')
PFN_ERR_UNSUPPORTED, PFN_ERR_ALIGNMENT, PFN_ERR_ARGUMENT = -1, -2, -4
SYMBOLS = (('pfn_class_embed_workspace_bytes', 6), ('pfn_class_embed_forward', 22), ('pfn_class_embed_backward', 16))


def test_the_symbols_are_declared_exported_and_bound_at_abi_10():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    source = open(os.path.join(CSRC, 'class_embed.hip')).read()      # the entry points stand beside their kernels
    lib = _hip.lib()
    for symbol, nargs in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % symbol, header), symbol
        assert symbol in _hip.SIGNATURES and hasattr(lib, symbol) and len(_hip.SIGNATURES[symbol][1]) == nargs, symbol
        assert re.search(r'^int(64_t)? %s\s*\(' % symbol, source, re.M), symbol
    assert _hip.ABI_VERSION == 10 and lib.pfn_abi_version() == 10 and '#define PFN_ABI_VERSION 10' in header
    build = open(os.path.join(CSRC, 'build.sh')).read()
    assert 'class_embed.hip' in build and '../_build/class_embed.o' in build      # compiled and linked
    assert re.search(r'\blaunch_gemm_nt\s*\(', source) and re.search(r'\blaunch_gemm_tn\s*\(', source)      # the GEMMs are the stack's
    assert callable(hipops.class_embed) and (hipops.CLASS_EMBED_MAX_FEATURES, hipops.CLASS_EMBED_MAX_CLASSES) == (1022, 1024)


@pytest.mark.parametrize('S,B,F,E,C,sep', [(3, 1, 1, 8, 1, 2), (11, 3, 7, 64, 5, 10), (5, 7, 33, 72, 37, 0), (5, 7, 33, 72, 37, 5), (4, 2, 9, 16, 3, 1)])
def test_the_restatement_is_torchs_linear_canemb_and_cat_in_f64(S, B, F, E, C, sep):
    g = torch.Generator().manual_seed(S * 1000 + F)
    x = torch.randn(S, B, F, dtype=torch.float64, generator=g)
    labels = torch.randint(0, C, (S, B), generator=g)
    enc, emb = nn.Linear(F, E).double(), encoders.CanEmb(1, C, E).double()
    x_emb, y_emb = enc(x), emb(labels.unsqueeze(-1))      # the four lines of TransformerModel.forward (reference transformer.py:68-74)
    src = torch.cat([x_emb[:sep] + y_emb[:sep], x_emb[sep:]], 0)
    dsrc = torch.randn(S, B, E, dtype=torch.float64, generator=g)
    src.backward(dsrc)
    wx, bx, table = enc.weight.detach(), enc.bias.detach(), emb.weight.detach()
    mine = R.forward(x, labels, wx, bx, table, sep)
    dwx, dbx, dtable = R.backward(x, labels, C, sep, dsrc)
    table_grad = emb.weight.grad if emb.weight.grad is not None else torch.zeros_like(table)      # (sep = 0: the table is not on the graph)
    for name, got, want in (('src', mine, src.detach()), ('dWx', dwx, enc.weight.grad), ('dbx', dbx, enc.bias.grad), ('dtable', dtable, table_grad)):
        assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name
    # the rounded variant in f32 "rounds" nothing a float32 run would not; in fp16 it differs from the plain one by about the unit round-off
    e = R.error(R.rounded_forward(x, labels, wx, bx, table, sep, 'fp16'), mine)
    assert 0 < e < 16 * R.UNIT_ROUNDOFF['fp16']
    # a label outside [0, C) on a train row selects no class row; on a test row it is never looked at
    bad = labels.clone()
    bad[sep:] = -100
    assert torch.equal(R.forward(x, bad, wx, bx, table, sep), mine)
    if sep > 0:
        bad[0, 0] = C
        assert torch.equal(R.forward(x, bad, wx, bx, table, sep)[0, 0], (x @ wx.t() + bx)[0, 0])


def test_the_loss_scale_of_the_rounded_backward_is_a_power_of_two():
    d = torch.tensor([[[3e-7, -1.1e-9, 0.0, 2.5e-8]]], dtype=torch.float64)
    r = R.round_scaled(d, 'fp16')
    assert R.error(r, d) < R.UNIT_ROUNDOFF['fp16'] and float(r[0, 0, 1]) != 0      # without the scale 1.1e-9 is below fp16's smallest subnormal
    assert float(R.round_to(d, 'fp16')[0, 0, 1]) == 0
    assert torch.equal(R.round_scaled(d, 'bf16'), R.round_to(d, 'bf16'))


def test_the_kernels_keep_their_register_and_scratch_budgets(tmp_path):
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    asm = str(tmp_path / 'class_embed.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-munsafe-fp-atomics', '-S', '--cuda-device-only', os.path.join(CSRC, 'class_embed.hip'), '-o', asm],
                   check=True, capture_output=True)
    found = dict(re.findall(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', open(asm).read(), re.S))
    count = lambda part: sum(part in k for k in found)
    # the two packs in three operand types, the d(src) cast in the two 16-bit ones, one scatter
    assert len(found) == 9 and count('class_embed_pack_kernel') == 3 and count('class_embed_pack_w_kernel') == 3 and count('class_embed_cast_kernel') == 2 and \
        count('class_embed_scatter_kernel') == 1, sorted(found)
    for name, body in found.items():
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name      # no scratch
        assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 128, name      # four waves per SIMD
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1)) == 0, name      # no LDS: nothing here is reused


def model(y_encoder=None, encoder=None, **kw):
    E = 64
    return TransformerModel(encoder or encoders.Linear(784, E), 5, E, 2, 128, 2, 0.0, y_encoder=y_encoder or encoders.get_Canonical(5)(1, E), **kw)


def test_which_models_take_the_class_embedding():
    m = model()
    assert m._fused_class_embedding() and not m._fused_embedding() and m.fuse_class_embedding is True and m.class_embedding_status() == (0, 0)
    m.fuse_class_embedding = False
    assert not m._fused_class_embedding()
    E = 64
    excluded = {
        'padding_idx': model(encoders.CanEmb(1, 5, E, padding_idx=0)),
        'max_norm': model(encoders.CanEmb(1, 5, E, max_norm=1.0)),
        'scale_grad_by_freq': model(encoders.CanEmb(1, 5, E, scale_grad_by_freq=True)),
        'sparse': model(encoders.CanEmb(1, 5, E, sparse=True)),
        'SeqBN': model(input_normalization=True),
        'positional encoding': model(pos_encoder=positional_encodings.PositionalEncoding(E, 64)),
        '(Linear, Linear)': model(encoders.Linear(1, E)),
        'two label features': model(encoders.CanEmb(2, 5, E)),
        'a subclass of CanEmb': model(type('Mine', (encoders.CanEmb,), {})(1, 5, E)),
        'an MLP x-encoder': model(encoder=nn.Sequential(nn.Linear(784, E))),
        'a table wider than the limit': model(encoders.CanEmb(1, 1025, E)),
        'no bias': model(encoder=nn.Linear(784, E, bias=False)),
    }
    for name, m in excluded.items():
        assert not m._fused_class_embedding(), name
    assert excluded['(Linear, Linear)']._fused_embedding()
    assert model(pos_encoder=positional_encodings.NoPositionalEncoding(E, 64))._fused_class_embedding()
    assert model(encoders.CanEmb(1, 1024, E), encoder=encoders.Linear(1022, E))._fused_class_embedding()      # the widest table and encoder
    # the parameters of such a model are where the state dict of the reference has them
    assert [k for k in model().state_dict() if 'encoder' in k and 'transformer' not in k] == ['encoder.weight', 'encoder.bias', 'y_encoder.weight']


def test_argument_errors_return_before_any_launch():
    lib = _hip.lib()
    buf = torch.zeros(1 << 16)      # host memory: a refused call never looks at it
    p = buf.data_ptr()
    assert p % 16 == 0

    def fwd(B=2, S=3, F=4, E=8, C=2, sep=1, prec=2, ws=p, ws_bytes=1 << 18, x=p, labels=p, wx=p, bx=p, table=p, src=p, status=p):
        return lib.pfn_class_embed_forward(x, 4, 12, labels, 2, 1, wx, bx, table, B, S, F, E, C, sep, prec, 0, ws, ws_bytes, src, status, 0)

    def bwd(B=2, S=3, F=4, E=8, C=2, sep=1, prec=2, ws=p, ws_bytes=1 << 18, dsrc=p, dwx=p, dbx=p, dtable=p):
        return lib.pfn_class_embed_backward(dsrc, p, B, S, F, E, C, sep, prec, 0, ws, ws_bytes, dwx, dbx, dtable, 0)
    for kw in (dict(F=0), dict(F=1023), dict(C=0), dict(C=1025), dict(E=0), dict(E=4), dict(E=12), dict(prec=3), dict(prec=-1)):
        assert fwd(**kw) == PFN_ERR_UNSUPPORTED and bwd(**kw) == PFN_ERR_UNSUPPORTED, kw
        assert lib.pfn_class_embed_workspace_bytes(2, 3, kw.get('F', 4), kw.get('E', 8), kw.get('C', 2), kw.get('prec', 2)) == PFN_ERR_UNSUPPORTED, kw
        assert b'class_embed' in lib.pfn_last_error_string()
    for kw in (dict(B=-1), dict(S=-1), dict(sep=-1), dict(sep=4), dict(ws=0), dict(ws_bytes=64)):
        assert fwd(**kw) == PFN_ERR_ARGUMENT and bwd(**kw) == PFN_ERR_ARGUMENT, kw
    for kw in (dict(x=0), dict(labels=0), dict(wx=0), dict(bx=0), dict(table=0), dict(src=0)):
        assert fwd(**kw) == PFN_ERR_ARGUMENT, kw
    assert bwd(dsrc=0) == PFN_ERR_ARGUMENT
    for kw in (dict(ws=p + 8), dict(src=p + 4), dict(bx=p + 8), dict(x=p + 2), dict(labels=p + 4), dict(status=p + 2)):
        assert fwd(**kw) == PFN_ERR_ALIGNMENT, kw
    for kw in (dict(ws=p + 8), dict(dsrc=p + 4), dict(dwx=p + 2), dict(dtable=p + 1)):
        assert bwd(**kw) == PFN_ERR_ALIGNMENT, kw
    assert fwd(F=0, x=0) == PFN_ERR_UNSUPPORTED      # the shape first, before any pointer is looked at
    assert lib.pfn_class_embed_workspace_bytes(-1, 3, 4, 8, 2, 2) == PFN_ERR_ARGUMENT
    # nothing to do: nothing launched, whatever the pointers are
    assert fwd(B=0, x=0, ws=0) == 0 and fwd(S=0, sep=0, src=0) == 0 and bwd(B=0, dsrc=0) == 0
    # the workspace holds A_aug, W_aug, the d(src) copy (16-bit), dW_aug and its column sums; Kp = F + C rounded up to 64
    n16, n32 = lib.pfn_class_embed_workspace_bytes(1000, 26, 784, 1024, 5, 2), lib.pfn_class_embed_workspace_bytes(1000, 26, 784, 1024, 5, 1)
    Kp = 832
    assert 26000 * Kp * 2 + 1024 * Kp * 2 + 26000 * 1024 * 2 + 1024 * Kp * 4 + 4096 <= n16 < 1.01 * (26000 * Kp * 2 + 1024 * Kp * 2 + 26000 * 1024 * 2 + 1024 * Kp * 4 + 4096)
    assert 26000 * Kp * 4 + 1024 * Kp * 8 <= n32 < 1.01 * (26000 * Kp * 4 + 1024 * Kp * 8 + 4096)
    assert lib.pfn_class_embed_workspace_bytes(2, 2, 60, 1024, 1024, 0) == lib.pfn_class_embed_workspace_bytes(2, 2, 60, 1024, 1024, 2)


def test_python_checks_raise_before_the_device_is_asked_for():
    x, labels = torch.zeros(3, 2, 4), torch.zeros(3, 2, dtype=torch.int64)
    w, b, t = torch.zeros(8, 4), torch.zeros(8), torch.zeros(5, 8)
    bad = [
        (dict(sep=4), 'sep = 4'), (dict(sep=-1), 'sep = -1'), (dict(precision='fp8'), 'precision'), (dict(precision=7), 'precision'),
        (dict(labels=torch.zeros(3, 2)), 'class indices'), (dict(labels=torch.zeros(2, 3, dtype=torch.int64)), r'labels \[S, B\]'),
        (dict(weight=torch.zeros(8, 5)), 'do not fit'), (dict(bias=torch.zeros(7)), 'do not fit'), (dict(table=torch.zeros(5, 16)), 'do not fit'),
        (dict(weight=torch.zeros(12, 4), bias=torch.zeros(12), table=torch.zeros(5, 12)), 'multiple of 8'),
        (dict(table=torch.zeros(1025, 8)), 'C = 1025'), (dict(x=torch.zeros(3, 2, 1023), weight=torch.zeros(8, 1023)), 'F = 1023'),
        (dict(status=torch.zeros(2)), 'status'), (dict(status=torch.zeros(3, dtype=torch.int32)), 'status'), (dict(bias=None), 'bias'),
    ]
    for kw, match in bad:
        args = dict(x=x, labels=labels, weight=w, bias=b, table=t, sep=1, precision='fp16')
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            hipops.class_embed(**args)
    # with sound arguments the op asks for the GPU: there is no CPU fall-back
    with pytest.raises(_hip.HipExtensionError):
        hipops.class_embed(x, labels, w, b, t, 1, 'f32')
    with pytest.raises(_hip.HipExtensionError):
        model()((torch.zeros(11, 2, 784), torch.zeros(11, 2, dtype=torch.int64)), single_eval_pos=10)
