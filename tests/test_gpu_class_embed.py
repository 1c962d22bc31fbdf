"""The class-label embedding on the device (csrc/class_embed.hip, hipops.class_embed, TransformerModel's (Linear, CanEmb) path) against its f64 restatement
(tests/class_embed_f64.py): forward and the three gradients per tensor in fp16 / bf16 / f32 at the smallest shapes where packing, padding and tile edges can
go wrong; the op's properties (test-row labels, out-of-range labels, saturation, accumulation, determinism); the notebook's model both ways.

Bounds (README), the error being max |error| over max |f64 value| of a tensor: 16-bit 3 max(e, u), e the error of the operand-rounded
restatement, u the format's unit round-off; f32 4 max(e, 2^-23), e the float32 CPU run's.  The measured values are on record in
profiles/r21_class_embed_bounds_measured.json (PFN_RECORD_BOUNDS)."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_embed_f64 as R      # noqa: E402
from bounds import within      # noqa: E402

from oracle import pfn_oracle      # noqa: E402
from transformerscandobayesianinference_amd import _hip, encoders, hipops, priors      # noqa: E402
from transformerscandobayesianinference_amd.priors import stroke      # noqa: E402
from transformerscandobayesianinference_amd.transformer import TransformerModel      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PRECISIONS = ('fp16', 'bf16', 'f32')
# (S, B, F, E, C): the smallest shape; a plain one; Kp padding past one 64 block; 260 tokens, across a 256-row tile; the widest F; the widest table
SHAPES = [(3, 1, 1, 8, 1), (11, 3, 7, 64, 5), (5, 7, 33, 72, 37), (26, 10, 784, 64, 5), (4, 65, 1022, 128, 2), (2, 2, 60, 1024, 1024)]
TOKENS_260 = SHAPES[3]
CASES = [(shape, sep) for shape in SHAPES for sep in sorted({0, 1, shape[0] - 1, shape[0]})]
NAMES = ('src', 'dWx', 'dbx', 'dtable')


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


_refs = {}


def reference(shape, sep):
    """Inputs (f32, on the CPU) and what f64 makes of them, computed once per (shape, sep) and left alone: x as the transposed view of a [B, S, F] tensor -- how
    get_batch returns it -- labels int64 with strides of their own, d(src) small enough that fp16 needs its loss scale."""
    key = (shape, sep)
    if key not in _refs:
        S, B, F, E, C = shape
        g = torch.Generator().manual_seed(hash(key) % (2 ** 31))
        x = torch.randn(B, S, F, generator=g).transpose(0, 1)
        labels = torch.randint(0, C, (S, 2 * B + 1), generator=g)[:, 1::2]
        assert x.stride() == (F, S * F, 1) and labels.stride() == (2 * B + 1, 2) and labels.shape == (S, B)
        wx, bx, table = torch.randn(E, F, generator=g) / math.sqrt(F), 0.1 * torch.randn(E, generator=g), torch.randn(C, E, generator=g)
        dsrc = 1e-4 * torch.randn(S, B, E, generator=g)
        d = [t.double() for t in (x, wx, bx, table, dsrc)]
        want = (R.forward(d[0], labels, d[1], d[2], d[3], sep),) + R.backward(d[0], labels, C, sep, d[4])
        f32 = (R.forward(x, labels, wx, bx, table, sep),) + R.backward(x, labels, C, sep, dsrc)
        e = {'f32': [R.error(a, b) for a, b in zip(f32, want)]}
        for p in ('fp16', 'bf16'):
            rounded = (R.rounded_forward(d[0], labels, d[1], d[2], d[3], sep, p),) + R.rounded_backward(d[0], labels, C, sep, d[4], p)
            e[p] = [R.error(a, b) for a, b in zip(rounded, want)]
        _refs[key] = dict(x=x, labels=labels, wx=wx, bx=bx, table=table, dsrc=dsrc, want=want, e=e)
    return _refs[key]


def run_op(ref, sep, precision, labels=None, x=None, deterministic=False, status=None):
    """(src, dWx, dbx, dtable) of hipops.class_embed on the reference's inputs, strides kept."""
    xg = (ref['x'] if x is None else x)
    xg = xg.transpose(0, 1).contiguous().to(DEV).transpose(0, 1)
    lab = ref['labels'] if labels is None else labels
    wide = torch.zeros(lab.shape[0], 2 * lab.shape[1] + 1, dtype=torch.int64)
    wide[:, 1::2] = lab
    lab = wide.to(DEV)[:, 1::2]
    assert xg.stride() == ref['x'].stride() and lab.stride() == ref['labels'].stride()
    w, b, t = (ref[k].to(DEV).requires_grad_(True) for k in ('wx', 'bx', 'table'))
    src = hipops.class_embed(xg, lab, w, b, t, sep, precision, deterministic=deterministic, status=status)
    src.backward(ref['dsrc'].to(DEV))
    return src.detach(), w.grad, b.grad, t.grad


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('shape,sep', CASES, ids=[f'S{s[0]}-B{s[1]}-F{s[2]}-E{s[3]}-C{s[4]}-sep{sep}' for s, sep in CASES])
def test_forward_and_gradients_per_tensor_vs_f64(shape, sep, precision):
    ref = reference(shape, sep)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    got = run_op(ref, sep, precision, status=status)
    assert tuple(got[0].shape) == (shape[0], shape[1], shape[3]) and status.tolist() == [0, 0]
    for name, g, want, e in zip(NAMES, got, ref['want'], ref['e'][precision]):
        err, bound = R.error(g.cpu(), want), R.bound(precision, e)
        print(f'{name}: error {err:.3e}, e {e:.3e}, bound {bound:.3e}')
        within(f'{precision} {name}', err, bound)
    if sep == 0:
        assert not got[3].any()      # no train row: the table's gradient is not touched


# ---- properties of the op -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('shape,sep,deterministic', [(SHAPES[1], 7, False), (TOKENS_260, 25, True)])      # 33 tokens: one token split, one writer even by default
def test_labels_of_test_rows_do_not_matter(shape, sep, deterministic, precision):
    ref = reference(shape, sep)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    base = run_op(ref, sep, precision, deterministic=deterministic, status=status)
    for junk in (-100, 10 ** 6):
        labels = ref['labels'].clone()
        labels[sep:] = junk
        other = run_op(ref, sep, precision, labels=labels, deterministic=deterministic, status=status)
        for name, a, b in zip(NAMES, base, other):
            assert torch.equal(bits(a), bits(b)), (name, junk)
    assert status.tolist() == [0, 0]


@pytest.mark.parametrize('precision', PRECISIONS)
def test_out_of_range_train_labels_are_counted_and_select_no_class_row(precision):
    shape, sep = SHAPES[2], 4
    ref = reference(shape, sep)
    S, B, F, E, C = shape
    labels = ref['labels'].clone()
    bad = [(0, 0, -1), (1, 3, C), (3, 6, 10 ** 12), (2, 2, -2 ** 40)]
    for t, b, v in bad:
        labels[t, b] = v
    labels[sep, 1] = C + 5      # a test row: not counted
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    got = run_op(ref, sep, precision, labels=labels, status=status)
    torch.cuda.synchronize()      # nothing faulted
    assert status.tolist() == [len(bad), 0]
    alone = run_op(ref, 0, precision)[0]      # the x-embedding alone
    for t, b, _ in bad:
        assert torch.equal(bits(got[0][t, b]), bits(alone[t, b])), (t, b)
    assert not torch.equal(bits(got[0][0, 1]), bits(alone[0, 1]))      # (a sound train row does carry its class row)
    d = [ref[k].double() for k in ('x', 'dsrc')]
    want = R.backward(d[0], labels, C, sep, d[1])      # the restatement leaves those rows out of the table's gradient
    rounded = R.rounded_backward(d[0], labels, C, sep, d[1], precision) if precision != 'f32' else R.backward(ref['x'], labels, C, sep, ref['dsrc'])
    for name, g, w, r in zip(NAMES[1:], got[1:], want, rounded):
        within(f'{precision} {name}', R.error(g.cpu(), w), R.bound(precision, R.error(r, w)))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_fp16_saturation_is_counted(precision):
    shape, sep = SHAPES[1], 7
    ref = reference(shape, sep)
    x = ref['x'].clone()
    x[2, 1, 3], x[9, 0, 0] = 1e6, -1e6
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    src = run_op(ref, sep, precision, x=x, status=status)[0]
    assert status.tolist() == [0, 2 if precision == 'fp16' else 0] and torch.isfinite(src).all()
    if precision == 'fp16':      # stored as +-65504: the row is what the restatement makes of the clamped x
        want = R.rounded_forward(x.double(), ref['labels'], ref['wx'].double(), ref['bx'].double(), ref['table'].double(), sep, 'fp16')
        assert R.error(src.cpu()[2, 1], want[2, 1]) < 1e-5


@pytest.mark.parametrize('precision', PRECISIONS)
def test_two_backward_calls_accumulate_and_nothing_is_written_past_an_output(precision):
    """Integers only, small enough to be exact in every operand format and in the f32 accumulators: the gradients equal the f64 ones exactly, twice them after
    a second call; -7 sentinels behind src, the workspace and the three gradients stay."""
    S, B, F, E, C = SHAPES[2]
    sep, prec = 4, _hip.PRECISIONS[precision]
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (B, S, F), generator=g).float().transpose(0, 1)
    labels = torch.randint(0, C, (S, B), generator=g)
    wx, bx, table = (torch.randint(-2, 3, s, generator=g).float() for s in ((E, F), (E,), (C, E)))
    dsrc = torch.randint(-4, 5, (S, B, E), generator=g).float()
    dsrc[0, 0, 0] = 4      # max |d(src)| a power of two
    want = (R.forward(x.double(), labels, wx.double(), bx.double(), table.double(), sep),) + R.backward(x.double(), labels, C, sep, dsrc.double())
    lib, stream = _hip.lib(), _hip.stream_ptr()
    ws_bytes = lib.pfn_class_embed_workspace_bytes(B, S, F, E, C, prec)
    assert ws_bytes > 0 and ws_bytes % 16 == 0

    def guarded(n, fill=0.0):
        t = torch.full((n + 64,), -7.0, device=DEV)
        t[:n] = fill
        return t
    ws = torch.full((ws_bytes + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    src, dwx, dbx, dtable = guarded(S * B * E, float('nan')), guarded(E * F), guarded(E), guarded(C * E)
    xd, ld, wd, bd, td, dd = (t.to(DEV) for t in (x.transpose(0, 1).contiguous(), labels, wx, bx, table, dsrc))
    _hip.check(lib.pfn_class_embed_forward(xd.data_ptr(), F, S * F, ld.data_ptr(), B, 1, wd.data_ptr(), bd.data_ptr(), td.data_ptr(), B, S, F, E, C, sep, prec, 0,
                                           ws.data_ptr(), ws_bytes, src.data_ptr(), 0, stream), 'pfn_class_embed_forward')
    assert torch.equal(src[:S * B * E].cpu().double().view(S, B, E), want[0])
    for call in (1, 2):
        _hip.check(lib.pfn_class_embed_backward(dd.data_ptr(), wd.data_ptr(), B, S, F, E, C, sep, prec, 0, ws.data_ptr(), ws_bytes, dwx.data_ptr(), dbx.data_ptr(),
                                                dtable.data_ptr(), stream), 'pfn_class_embed_backward')
        for name, got, w in zip(NAMES[1:], (dwx, dbx, dtable), want[1:]):
            assert torch.equal(got[:w.numel()].cpu().double().view(w.shape), call * w), (name, call)
    for name, t in (('src', src), ('dwx', dwx), ('dbx', dbx), ('dtable', dtable)):
        assert (t[-64:] == -7.0).all(), name
    assert (ws[ws_bytes:] == 0xA5).all()
    # sep = 0: the x-embedding alone, and the table's gradient is left as it was
    _hip.check(lib.pfn_class_embed_forward(xd.data_ptr(), F, S * F, 0, 0, 0, wd.data_ptr(), bd.data_ptr(), td.data_ptr(), B, S, F, E, C, 0, prec, 0,
                                           ws.data_ptr(), ws_bytes, src.data_ptr(), 0, stream), 'pfn_class_embed_forward')
    _hip.check(lib.pfn_class_embed_backward(dd.data_ptr(), wd.data_ptr(), B, S, F, E, C, 0, prec, 0, ws.data_ptr(), ws_bytes, dwx.data_ptr(), dbx.data_ptr(),
                                            dtable.data_ptr(), stream), 'pfn_class_embed_backward')
    assert torch.equal(src[:S * B * E].cpu().double().view(S, B, E), x.double() @ wx.double().t() + bx.double())
    assert torch.equal(dtable[:C * E].cpu().double().view(C, E), 2 * want[3]) and torch.equal(dwx[:E * F].cpu().double().view(E, F), 3 * want[1])


@pytest.mark.parametrize('precision', PRECISIONS)
def test_the_deterministic_flag_gives_bit_equal_gradients(precision):
    ref = reference(TOKENS_260, 25)
    first, second = run_op(ref, 25, precision, deterministic=True), run_op(ref, 25, precision, deterministic=True)
    for name, a, b in zip(NAMES, first, second):
        assert torch.equal(bits(a), bits(b)), name
    for name, g, want, e in zip(NAMES, first, ref['want'], ref['e'][precision]):
        within(f'{precision} {name}', R.error(g.cpu(), want), R.bound(precision, e))


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------------------
E_, H_, NHID_, L_, T_, SEP_, B_, C_ = 64, 2, 128, 2, 11, 10, 6, 5
_model_data = {}


def batch():
    """One batch of stroke images at the notebook's model shape, and the f64 logits and gradients of the notebook's model on it: the f64 restatement of the
    embedding followed by oracle.pfn_oracle (fed the embedding through an identity encoder), cross-entropy on the test rows."""
    if not _model_data:
        labels, targets = stroke.draw_labels(B_, T_, C_, only_train_for_last_idx=True, generator=torch.Generator().manual_seed(3))      # [B, T]
        drawn = hipops.stroke_prior_sample(labels.to(torch.int32).contiguous().to(DEV), 28, stroke.integer_bounds(28), C_, 20260, offset=1, normalize=True)
        x, y, target = drawn['x'], labels.t().contiguous().to(DEV), targets.t().contiguous().to(DEV)      # what get_batch returns, at a fixed seed and offset
        assert tuple(x.shape) == (T_, B_, 784) and (target[:-1] == -100).all()
        sd = {k: v.detach().cpu().clone() for k, v in build('f32', True).state_dict().items()}
        p64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        emb = R.forward(x.cpu().double(), y.cpu(), p64['encoder.weight'], p64['encoder.bias'], p64['y_encoder.weight'], SEP_)
        fed = {k: v for k, v in p64.items() if not k.startswith(('encoder.', 'y_encoder.'))}
        fed.update({'encoder.weight': torch.eye(E_, dtype=torch.float64), 'encoder.bias': torch.zeros(E_, dtype=torch.float64),
                    'y_encoder.weight': torch.zeros(E_, 1, dtype=torch.float64), 'y_encoder.bias': torch.zeros(E_, dtype=torch.float64)})
        logits = pfn_oracle.forward(fed, emb, torch.zeros(T_, B_, dtype=torch.float64), SEP_, H_)
        Fn.cross_entropy(logits.reshape(-1, C_), target[SEP_:].cpu().reshape(-1)).backward()
        _model_data.update(x=x, y=y, target=target, sd=sd, logits=logits.detach(), grads={k: v.grad for k, v in p64.items()})
        assert all(g is not None and g.abs().max() > 0 for g in _model_data['grads'].values())
    return _model_data


def build(precision, fuse, deterministic=False, sd=None):
    torch.manual_seed(0)
    m = TransformerModel(encoders.Linear(784, E_), C_, E_, H_, NHID_, L_, 0.0, y_encoder=encoders.get_Canonical(C_)(1, E_), precision=precision, deterministic=deterministic)
    with torch.no_grad():      # (the zero-initialised residual branches would hide every gradient below them: SURVEY section 4)
        for layer in m.transformer_encoder.layers:
            layer.linear2.weight.normal_(0, 0.05)
            layer.self_attn.out_proj.weight.normal_(0, 0.05)
    if sd is not None:
        m.load_state_dict(sd)
    m.fuse_class_embedding = fuse
    return m.to(DEV).train()


def step(m, d, x=None):
    for p in m.parameters():
        if p.grad is not None:
            p.grad.zero_()
    logits = m((d['x'] if x is None else x, d['y']), single_eval_pos=SEP_)
    Fn.cross_entropy(logits.reshape(-1, C_), d['target'][SEP_:].reshape(-1).to(logits.device)).backward()
    return logits.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize('precision', ['f32', 'fp16'])
def test_model_agrees_with_the_pytorch_embedding(precision, monkeypatch):
    d = batch()
    calls = []
    real = hipops.class_embed
    monkeypatch.setattr(hipops, 'class_embed', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    fused, torch_branch = build(precision, True, sd=d['sd']), build(precision, False, sd=d['sd'])
    assert fused._fused_class_embedding() and not torch_branch._fused_class_embedding()
    logits_t, grads_t = step(torch_branch, d)
    assert not calls
    logits_f, grads_f = step(fused, d)
    assert len(calls) == 1 and fused.class_embedding_status() == (0, 0)
    # the three embedding gradients live inside the flat gradient buffer (FusedClipAdam and the data-parallel all-reduce find them there)
    lo, hi = fused._flat_grad.data_ptr(), fused._flat_grad.data_ptr() + 4 * fused._flat_grad.numel()
    for p in (fused.encoder.weight, fused.encoder.bias, fused.y_encoder.weight):
        assert lo <= p.grad.data_ptr() and p.grad.data_ptr() + 4 * p.grad.numel() <= hi
        assert p.grad.data_ptr() - lo == p.data_ptr() - fused._flat.data_ptr()      # the gradient's slot is the parameter's
    pairs = [('logits', logits_f, logits_t, d['logits'])] + [(k, grads_f[k], grads_t[k], d['grads'][k]) for k in grads_t]
    for name, f, t, want in pairs:
        scale = float(want.abs().max())
        e = R.error(t.cpu(), want)      # the PyTorch embedding's own error against f64
        err = float((f - t).abs().max()) / scale
        bound = R.bound(precision, e)
        print(f'{name}: fused vs PyTorch embedding {err:.3e}, the latter against f64 {e:.3e}, bound {bound:.3e}')
        within(f'{precision} {name}', err, bound)


def test_deterministic_model_gives_bit_equal_embedding_gradients():
    d = batch()
    m = build('fp16', True, deterministic=True, sd=d['sd'])
    (_, a), (_, b) = step(m, d), step(m, d)
    for k in ('encoder.weight', 'encoder.bias', 'y_encoder.weight'):
        assert torch.equal(bits(a[k]), bits(b[k])) and a[k].abs().max() > 0, k


def test_an_x_that_requires_grad_keeps_the_pytorch_embedding(monkeypatch):
    d = batch()
    m = build('f32', True, sd=d['sd'])

    def refuse(*a, **k):
        raise AssertionError('the fused class embedding has no gradient for x')
    monkeypatch.setattr(hipops, 'class_embed', refuse)
    x = d['x'].clone().requires_grad_(True)
    step(m, d, x=x)
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    x64 = d['x'].cpu().double().requires_grad_(True)      # dx through the PyTorch embedding is d(src) . Wx: check it against autograd of the restatement at f64's d(src)
    sd = {k: v.double() for k, v in d['sd'].items()}
    emb = R.forward(x64, d['y'].cpu(), sd['encoder.weight'], sd['encoder.bias'], sd['y_encoder.weight'], SEP_)
    fed = {k: v for k, v in sd.items() if not k.startswith(('encoder.', 'y_encoder.'))}
    fed.update({'encoder.weight': torch.eye(E_, dtype=torch.float64), 'encoder.bias': torch.zeros(E_, dtype=torch.float64),
                'y_encoder.weight': torch.zeros(E_, 1, dtype=torch.float64), 'y_encoder.bias': torch.zeros(E_, dtype=torch.float64)})
    Fn.cross_entropy(pfn_oracle.forward(fed, emb, torch.zeros(T_, B_, dtype=torch.float64), SEP_, H_).reshape(-1, C_), d['target'][SEP_:].cpu().reshape(-1)).backward()
    assert R.error(x.grad.cpu(), x64.grad) < 1e-4
    with torch.no_grad():      # without autograd on x the fused path is asked for again
        with pytest.raises(AssertionError, match='no gradient for x'):
            m((x, d['y']), single_eval_pos=SEP_)


def test_the_notebooks_training_call_takes_the_fused_path(monkeypatch):
    from transformerscandobayesianinference_amd.train import Losses, train
    calls = []
    real = hipops.class_embed
    monkeypatch.setattr(hipops, 'class_embed', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    torch.manual_seed(0)
    loss, positional, model = train(priors.stroke.DataLoader, Losses.ce, encoders.Linear, y_encoder_generator=encoders.get_Canonical(C_), bptt=T_, single_eval_pos_gen=SEP_,
                                    emsize=E_, nhead=H_, nhid=NHID_, nlayers=L_, batch_size=B_, epochs=1, steps_per_epoch=4, verbose=False,
                                    extra_prior_kwargs_dict={'num_features': 784, 'num_outputs': C_, 'only_train_for_last_idx': True})
    print(f'loss {loss:.4f}, {len(calls)} fused embeddings')
    assert math.isfinite(loss) and 0 < loss < 2 * math.log(5)
    assert len(calls) >= 4 and model._fused_class_embedding() and model.class_embedding_status() == (0, 0)
    assert all(torch.isfinite(p).all() for p in model.parameters())
