"""Condition and predict with a different training-set size per dataset (TransformerModel.condition(src, train_lengths) / .condition_datasets / .predict;
the four pfn_stack_*_ragged entry points, ABI 10 additive) on the MI355X.  Column b of a ragged predict is what dataset b's own train rows alone give -- against
the B = 1 inference forward and the f64 oracle per dataset, in every operand format and head dim and in every state of the cached-K/V attention kernels that a
per-dataset key count adds (empty key-range splits, a dataset without train rows inside a batch, a partial last tile in a middle split); equal lengths are the
uniform call bit for bit; the padded rows reach nothing; input gradients.  The bounds are those of the uniform path, whose arithmetic this shares
(tests/test_gpu_predict.py BOUND, tests/test_gpu_predict_grad.py BOUND).  The maxima of this file have not been measured on a GPU yet: record them with
PFN_RECORD_BOUNDS=profiles/r10_predict_ragged_bounds_measured.json; a case above its bound is a bug to find, not a bound to widen."""
import pytest
import torch

from oracle import pfn_oracle
from bounds import within
from test_gpu_predict import BOUND, data, make, relerr
from test_gpu_predict_grad import BOUND as GRAD_BOUND, oracle_input_grads, predict_vjp
from transformerscandobayesianinference_amd import _hip, decoders, evaluation
from transformerscandobayesianinference_amd.optim import FusedClipAdam
from transformerscandobayesianinference_amd.transformer import TransformerModel, pad_datasets

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def alone(model, x, y, b, length, sep_max):
    """dataset b on its own: the B = 1 inference forward on its first `length` train rows followed by its test rows"""
    xs = torch.cat([x[:length, b:b + 1], x[sep_max:, b:b + 1]])
    ys = torch.cat([y[:length, b:b + 1], y[sep_max:, b:b + 1]])
    with torch.no_grad():
        return model((xs, ys), single_eval_pos=length)


def seeded_lengths(B, hi, seed=11):
    """B integers in [0, hi] that contain both ends"""
    v = torch.randint(0, hi + 1, (B,), generator=torch.Generator().manual_seed(seed)).tolist()
    v[0], v[1] = 0, hi
    return tuple(v)


# (operand format, inference format, emsize, heads, lengths, n): the smallest shapes that reach each state of the kernels
CASES = [
    ('f32', 'same', 128, 4, (437, 0, 64, 33, 1), 7),       # D 32: 14 splits of one 32-key tile, empty splits, a dataset without train rows, partial tiles
    ('f32', 'same', 256, 1, (63, 200, 0), 7),              # D 256: two V slices with ragged key counts
    ('f32', 'same', 256, 2, (2000, 31), 1),                # D 128: one long and one short dataset
    ('f32', 'same', 128, 4, seeded_lengths(32, 64), 260),  # >= 256 workgroups: one split, no merge
    ('fp16', 'same', 256, 2, (437, 0, 64, 65, 1), 7),      # 64-key tiles; per-dataset key shift, zero shift for the empty dataset
    ('fp16', 'same', 512, 4, (63, 300, 5), 300),           # several query blocks per dataset
    ('bf16', 'same', 128, 4, (437, 64, 0), 7),             # bf16 at D 32
    ('bf16', 'same', 256, 1, (437, 100), 7),               # bf16 at D 256
    ('fp16', 'f32', 256, 2, (437, 12, 0), 7),              # an fp16 model's default inference: the exact-f32 kernels
]


@pytest.mark.parametrize('precision,eval_precision,E,H,lengths,n', CASES, ids=[f'{c[0]}-{c[1]}-E{c[2]}-H{c[3]}-B{len(c[4])}-n{c[5]}' for c in CASES])
def test_ragged_predict_equals_each_dataset_alone(precision, eval_precision, E, H, lengths, n):
    B, sep_max = len(lengths), max(lengths)
    model = make(E, H, precision, eval_precision)
    x, y = data(sep_max, n, B)      # (the rows behind a dataset's own are whatever the generator drew: they must not matter)
    ctx = model.condition((x[:sep_max], y[:sep_max]), train_lengths=lengths)
    assert ctx.lengths == tuple(lengths) and ctx.sep == sep_max and ctx.sep_of.dtype == torch.int32 and ctx.sep_of.tolist() == list(lengths)
    got = model.predict(ctx, x[sep_max:])
    assert got.shape == (n, B, 100) and not got.requires_grad
    fmt = precision if eval_precision == 'same' else eval_precision
    for b, length in enumerate(lengths):
        want = alone(model, x, y, b, length, sep_max)
        within(f'{fmt} logits rel l2 vs the dataset alone', relerr(got[:, b:b + 1], want), BOUND[fmt])
    assert model.predict(ctx, x[sep_max:sep_max]).shape == (0, B, 100)


@pytest.mark.parametrize('sep', [437, 0])
@pytest.mark.parametrize('precision', ['f32', 'fp16'])
def test_equal_lengths_are_the_uniform_call_bit_for_bit(precision, sep):
    B, n = 3, 7
    model = make(256, 2, precision)
    x, y = data(sep, n, B)
    R = torch.randn(n, B, 100, generator=torch.Generator().manual_seed(7)).to(DEV)
    uni = model.condition((x[:sep], y[:sep]))
    rag = model.condition((x[:sep], y[:sep]), train_lengths=[sep] * B)
    assert uni.lengths is None and rag.lengths == (sep,) * B
    with torch.no_grad():
        assert torch.equal(model.predict(rag, x[sep:]), model.predict(uni, x[sep:]))
    out_u, dx_u = predict_vjp(model, uni, x[sep:], R)
    out_r, dx_r = predict_vjp(model, rag, x[sep:], R)
    assert torch.equal(out_r, out_u) and torch.equal(dx_r, dx_u)


@pytest.mark.parametrize('precision', ['f32', 'fp16', 'bf16'])
def test_padding_reaches_nothing(precision):
    """the same datasets conditioned with zeros and with large finite values behind their own rows: the same bits out"""
    lengths, n = (437, 0, 64), 7
    B, sep_max = len(lengths), max(lengths)
    model = make(256, 2, precision)
    x, y = data(sep_max, n, B)
    g = torch.Generator().manual_seed(3)
    xz, yz, xg, yg = x[:sep_max].clone(), y[:sep_max].clone(), x[:sep_max].clone(), y[:sep_max].clone()
    for b, length in enumerate(lengths):
        xz[length:, b] = 0
        yz[length:, b] = 0
        xg[length:, b] = (torch.randn(sep_max - length, x.shape[2], generator=g) * 1e3).to(DEV)
        yg[length:, b] = (torch.randint(0, 2, (sep_max - length,), generator=g).float() * 2e3 - 1e3).to(DEV)
    R = torch.randn(n, B, 100, generator=torch.Generator().manual_seed(7)).to(DEV)
    out_z, dx_z = predict_vjp(model, model.condition((xz, yz), train_lengths=lengths), x[sep_max:], R)
    out_g, dx_g = predict_vjp(model, model.condition((xg, yg), train_lengths=lengths), x[sep_max:], R)
    assert torch.isfinite(out_z).all() and torch.isfinite(dx_z).all()
    assert torch.equal(out_g, out_z)
    assert torch.equal(dx_g, dx_z)


@pytest.mark.parametrize('E,H,F', [(128, 4, 5), (1024, 4, 18)])
def test_ragged_predict_vs_oracle(E, H, F):
    """the batch and the bounds of test_predict_vs_oracle; test rows = the last n = 7 rows of every dataset, train rows = its first len_b <= 100 - n (one dataset
    keeps 99: train and test rows may overlap, they are just data)"""
    T, B, nbars, n = 100, 8, 100, 7
    lengths = (81, 99, 1, 0, 50, 64, 33, T - n)
    sep_max = max(lengths)
    model = make(E, H, 'f32', L=2, F=F, seed=3)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    params = {k: v for k, v in sd.items() if not k.startswith('criterion.')}
    gen = torch.Generator().manual_seed(5)
    x, y, _ = pfn_oracle.get_batch_fast_gp(B, T, F, {'noise': 1e-4, 'outputscale': 1., 'lengthscale': .6}, gen)
    ctx = model.condition((x[:sep_max].to(DEV), y[:sep_max].to(DEV)), train_lengths=lengths)
    lg = model.predict(ctx, x[T - n:].to(DEV))
    m_h = model.criterion.mean(lg)
    for b, length in enumerate(lengths):
        xs, ys = torch.cat([x[:length, b:b + 1], x[T - n:, b:b + 1]]), torch.cat([y[:length, b:b + 1], y[T - n:, b:b + 1]])
        lo = pfn_oracle.forward(params, xs, ys, length, H)
        within('logits rel l2 vs oracle', relerr(lg[:, b:b + 1], lo), 1e-4)
        m_o = pfn_oracle.bar_mean(lo, sd['criterion.borders'])
        within('means max / target range', ((m_h[:, b:b + 1].double().cpu() - m_o).abs().max() / (y.max() - y.min())).item(), 1e-5)
        within('means rel l2 (own norm)', relerr(m_h[:, b:b + 1], m_o), 1e-4)


@pytest.mark.parametrize('E,H,n', [(128, 4, 7), (256, 1, 7), (128, 2, 60)], ids=['D32-n7', 'D256-n7', 'D64-n60'])
@pytest.mark.parametrize('precision', ['f32', 'fp16', 'bf16'])
def test_ragged_input_gradients_vs_oracle(precision, E, H, n):
    lengths = (437, 0, 33)
    B, sep_max = len(lengths), max(lengths)
    model = make(E, H, precision, 'same')
    x, y = data(sep_max, n, B)
    R = torch.randn(n, B, 100, generator=torch.Generator().manual_seed(7)).to(DEV)
    ctx = model.condition((x[:sep_max], y[:sep_max]), train_lengths=lengths)
    before = ctx.buffer.clone()
    out, dx = predict_vjp(model, ctx, x[sep_max:], R)
    torch.cuda.synchronize()
    assert torch.equal(ctx.buffer, before)      # the backward leaves the context alone
    with torch.no_grad():
        assert torch.equal(out.detach(), model.predict(ctx, x[sep_max:]))
    for b, length in enumerate(lengths):
        xs = torch.cat([x[:length, b:b + 1], x[sep_max:, b:b + 1]])
        ys = torch.cat([y[:length, b:b + 1], y[sep_max:, b:b + 1]])
        _, dxo, _ = oracle_input_grads(model, xs, ys, length, H, R[:, b:b + 1])
        within(f'{precision} dx rel l2 vs oracle', relerr(dx[:, b:b + 1], dxo[length:]), GRAD_BOUND[precision])


def test_condition_datasets_is_condition_on_the_padded_batch():
    model = make(128, 4, 'f32')
    g = torch.Generator().manual_seed(2)
    sizes = (120, 0, 437, 1)
    datasets = [(torch.randn(s, 5, generator=g).to(DEV), torch.randn(s, generator=g).to(DEV)) for s in sizes]
    xt = torch.randn(9, len(sizes), 5, generator=g).to(DEV)
    a = model.condition_datasets(datasets)
    xp, yp, lengths = pad_datasets(datasets)
    assert lengths == sizes and xp.device == xt.device
    b = model.condition((xp, yp), train_lengths=torch.tensor(lengths))
    assert a.lengths == b.lengths == sizes and a.sep == 437
    assert torch.equal(model.predict(a, xt), model.predict(b, xt))


def test_chunks_equal_one_call(monkeypatch):
    model = make(128, 4, 'f32')
    lengths = (437, 0, 64)
    x, y = data(437, 50, 3)
    ctx = model.condition((x[:437], y[:437]), train_lengths=lengths)
    one = model.predict(ctx, x[437:])
    monkeypatch.setattr(TransformerModel, '_PREDICT_ROWS', 3 * 7)      # 7 rows x 3 datasets per chunk, the last one short
    within('f32 chunked vs one call rel l2', relerr(model.predict(ctx, x[437:]), one), 1e-6)
    parts = torch.cat([model.predict(ctx, x[437 + a:437 + b]) for a, b in ((0, 1), (1, 20), (20, 50))])
    within('f32 caller-side chunks vs one call rel l2', relerr(parts, one), 1e-6)


def test_custom_decoder():
    model = make(128, 4, 'f32', decoder=decoders.FixedScaledDecoder)
    lengths = (300, 0, 17)
    x, y = data(300, 50, 3)
    got = model.predict(model.condition((x[:300], y[:300]), train_lengths=lengths), x[300:])
    assert got.shape == (50, 3, 100)
    for b, length in enumerate(lengths):
        within('custom decoder: rel l2 vs the dataset alone', relerr(got[:, b:b + 1], alone(model, x, y, b, length, 300)), BOUND['f32'])


def test_a_stale_ragged_context_is_refused():
    model = make(128, 4, 'fp16', 'f32')
    lengths = (100, 37)
    x, y = data(100, 20, 2)
    ctx = model.condition((x[:100], y[:100]), train_lengths=lengths)
    model.predict(ctx, x[100:])
    with pytest.raises(ValueError):
        model.predict(ctx, x[100:, :1])          # another B
    with pytest.raises(ValueError):
        model.predict(ctx, x[100:, :, :4])       # another F
    with pytest.raises(_hip.HipExtensionError):
        model.predict(ctx, x[100:].cpu())
    with pytest.raises(ValueError):
        model.condition((x[:100], y[:100]), train_lengths=(100, 101))
    opt = FusedClipAdam(model, lr=1e-3)          # an optimizer step (writes the flat buffer through raw pointers)
    model.train()
    logits = model((x, y), single_eval_pos=100)
    model.criterion(logits.reshape(-1, 100), y[100:].flatten()).mean().backward()
    opt.step(zero_grad=True)
    model.eval()
    with pytest.raises(RuntimeError, match='changed after condition'):
        model.predict(ctx, x[100:])
    ctx = model.condition((x[:100], y[:100]), train_lengths=lengths)
    model.predict(ctx, x[100:])
    model.mark_params_updated()
    with pytest.raises(RuntimeError, match='changed after condition'):
        model.predict(ctx, x[100:])
    ctx = model.condition((x[:100], y[:100]), train_lengths=lengths)
    model.schedule = _hip.SCHED_TOP_LAYER_ALL_ROWS      # another descriptor
    with pytest.raises(RuntimeError, match='descriptor'):
        model.predict(ctx, x[100:])


def test_learning_curve():
    """NLL and posterior mean of row p given rows [:p] from one ragged condition and one predict equal the per-position forwards (f32; both tensors [P, B] in rel l2)"""
    T, B, positions = 60, 2, (1, 17, 32, 59)
    model = make(128, 4, 'f32')
    x, y = data(T, 0, B)
    nll, mean = evaluation.learning_curve(model, x, y, positions)
    assert nll.shape == mean.shape == (len(positions), B)
    want_nll, want_mean = [], []
    with torch.no_grad():
        for p in positions:
            logits = model((x[:p + 1], y[:p + 1]), single_eval_pos=p)
            want_nll.append(model.criterion(logits[0], y[p]))
            want_mean.append(model.criterion.mean(logits)[0])
    within('learning curve: nll rel l2 vs per-position forwards', relerr(nll, torch.stack(want_nll)), BOUND['f32'])
    within('learning curve: means rel l2 vs per-position forwards', relerr(mean, torch.stack(want_mean)), BOUND['f32'])
