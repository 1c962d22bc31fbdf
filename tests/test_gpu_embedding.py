"""The embedding stage, one tensor at a time: (x, y, single_eval_pos) -> src and the four gradients encoder.weight / encoder.bias / y_encoder.weight /
y_encoder.bias back out, against the f64 oracle (oracle/pfn_oracle.py) on every backward form the dispatch can pick:

  * f32: the register kernel embed_bwd_kernel<NF8> (nf + 2 <= 32, NF8 = 8 / 16 / 24 / 32) and the wide kernel (nf + 2 > 32);
  * 16-bit: the GEMM form (embed_fwd -> xaug_t, launch_gemm_tn -> embacc, embed_grad_scatter) with emb_aug_width 32 / 64 / 128, and the wide kernel past it;
  * each of them under the default and the deterministic schedule, for a single eval position and for forward_batches' per-dataset ones.

Inside a whole model these tensors are a percent or less of the global gradient norm, which is all the 16-bit model tests assert.  B*T = 390 is a multiple of
neither EMB_TOK (16) nor EMBB_TOK (128), so every kernel sees a ragged last tile.  Bounds are twice the largest value measured on the MI355X over the matrix
(profiles/embedding_parity_measured.json, recorded with PFN_RECORD_BOUNDS).
"""
import pytest
import torch
from torch import nn

from oracle import pfn_oracle
from bounds import within
from transformerscandobayesianinference_amd import bar_distribution, encoders
from transformerscandobayesianinference_amd.transformer import TransformerModel

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
T, B, E, H, NHID, L, NBARS = 130, 3, 128, 4, 256, 1, 20
NFS = [1, 6, 7, 14, 15, 22, 23, 30, 31, 62, 63, 100, 126, 127, 200, 1000]      # both sides of every NF8 template and aug width, nf + 2 == aug, the wide kernel
SEPS = (1, 64, 129)
EMB = ('encoder.weight', 'encoder.bias', 'y_encoder.weight', 'y_encoder.bias')
PRECISIONS = ('f32', 'bf16', 'fp16')


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# (f32, bf16, fp16) per quantity: <= 2 x the largest value measured on the MI355X over both oracle tests below (profiles/embedding_parity_measured.json)
BOUNDS = {'logits': (1.3e-6, 9.5e-3, 1.1e-3),
          'encoder.weight': (1.2e-6, 1.2e-2, 1.8e-3),
          'encoder.weight worst column': (1.9e-6, 3.8e-2, 3.4e-3),
          'encoder.bias': (1.2e-6, 1.1e-2, 1.5e-3),
          'y_encoder.weight': (2.1e-6, 2.3e-2, 3.3e-3),
          'y_encoder.bias': (1.7e-6, 1.4e-2, 1.8e-3)}


def bound(precision, what):
    return BOUNDS[what][PRECISIONS.index(precision)]


def col_exponents(nf):
    """a power-of-two scale per feature column, 2^-16 .. 2^16: x's column is multiplied by it and encoder.weight's column divided by it (the logits do not
    change; in fp16 the small columns reach the subnormals and the large ones pass 65504 -- where an unscaled operand of the weight gradient goes wrong)"""
    g = torch.Generator().manual_seed(1000 + nf)
    return torch.randint(-16, 17, (nf,), generator=g).double()


def make_model(nf, precision, deterministic=False, pos_encoder=None, column_scales=True):
    torch.manual_seed(nf)
    borders = torch.sort(torch.randn(NBARS + 1) * 1.5)[0]
    m = TransformerModel(encoders.Linear(nf, E), NBARS, E, H, NHID, L, 0.0, y_encoder=encoders.Linear(1, E), pos_encoder=pos_encoder,
                         precision=precision, eval_precision=precision, deterministic=deterministic)
    m.criterion = bar_distribution.FullSupportBarDistribution(borders)
    with torch.no_grad():
        for layer in m.transformer_encoder.layers:      # un-zero the residual branches
            layer.linear2.weight.normal_(0, 0.03)
            layer.self_attn.out_proj.weight.normal_(0, 0.03)
        if column_scales:
            m.encoder.weight.mul_(torch.exp2(-col_exponents(nf)).float())
    return m


def make_data(nf, seed=0, column_scales=True):
    g = torch.Generator().manual_seed(seed * 7919 + nf)
    x = torch.randn(T, B, nf, generator=g)
    if column_scales:
        x = x * torch.exp2(col_exponents(nf)).float()
    y = torch.randn(T, B, generator=g)
    return x, y


_oracle = {}


def oracle(nf, sep, sd, x, y):
    key = (nf, sep)
    if key not in _oracle:
        _oracle[key] = pfn_oracle.loss_and_grads(sd, x, y, y, sep, H, sd['criterion.borders'])
    return _oracle[key]


def run(model, x, y, sep):
    model.zero_grad()
    logits = model((x, y), single_eval_pos=sep)
    loss = model.criterion(logits.reshape(-1, NBARS), y[sep:].to(DEV).float().reshape(-1)).mean()
    loss.backward()
    return logits.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def worst_column(got, want):
    return max(relerr(got[:, f], want[:, f]) for f in range(want.shape[1]))


def check_embedding(precision, logits, grads, logits_o, grads_o):
    within(f'{precision} logits rel l2', relerr(logits, logits_o), bound(precision, 'logits'))
    for k in EMB:
        within(f'{precision} {k} grad rel l2', relerr(grads[k], grads_o[k]), bound(precision, k))
    within(f'{precision} encoder.weight grad worst column rel l2', worst_column(grads['encoder.weight'], grads_o['encoder.weight']),
           bound(precision, 'encoder.weight worst column'))


# ---- A. the oracle matrix ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('deterministic', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('nf', NFS)
def test_embedding_gradients_per_tensor_vs_oracle(nf, precision, deterministic):
    model = make_model(nf, precision, deterministic)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    x, y = make_data(nf)
    for sep in SEPS:
        _, logits_o, grads_o = oracle(nf, sep, sd, x, y)
        logits, grads = run(model, x.to(DEV), y.to(DEV), sep)
        check_embedding(precision, logits, grads, logits_o, grads_o)


@pytest.mark.parametrize('deterministic', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('nf', [5, 23, 60, 100, 200])
def test_forward_batches_embedding_gradients_vs_oracle(nf, precision, deterministic):
    """per-dataset eval positions (the sep_of branch of every embedding kernel): the sum of the per-batch losses against the sum of the per-batch oracle gradients"""
    seps = [0, 77, 129]
    model = make_model(nf, precision, deterministic)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    x, y = make_data(nf, seed=1)
    want = [pfn_oracle.loss_and_grads(sd, x[:, b:b + 1], y[:, b:b + 1], y[:, b:b + 1], s, H, sd['criterion.borders']) for b, s in enumerate(seps)]
    grads_o = {k: sum(w[2][k] for w in want) for k in want[0][2]}
    xd, yd = x.to(DEV), y.to(DEV)
    model.zero_grad()
    outs = model.forward_batches([(xd[:, b:b + 1], yd[:, b:b + 1]) for b in range(B)], seps)
    loss = sum(model.criterion(o.reshape(-1, NBARS), yd[s:, b:b + 1].reshape(-1)).mean() for b, (o, s) in enumerate(zip(outs, seps)))
    loss.backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    logits = torch.cat([o.reshape(-1) for o in outs])
    logits_o = torch.cat([w[1].reshape(-1) for w in want])
    check_embedding(precision, logits, grads, logits_o, grads_o)


# ---- B. exact scale equivariance ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('nf', [5, 60, 100])
def test_input_scale_moves_into_the_encoder_weights_bit_for_bit(nf, precision):
    """x * 2^k with encoder.weight * 2^-k, y (the input, not the targets) * 2^k with y_encoder.weight * 2^-k: every product of the embedding is the same, so
    under the deterministic schedule the logits and every other gradient are bit-identical, and the two rescaled weights' gradients are 2^k times the k = 0
    ones exactly (16-bit operands included: each column of the weight-gradient operand carries its own power of two)"""
    model = make_model(nf, precision, deterministic=True).to(DEV).train()
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    x, y = make_data(nf, seed=2)
    x, y = x.to(DEV), y.to(DEV)
    sep = 64

    def run_k(k):
        sd = dict(sd0)
        sd['encoder.weight'] = sd0['encoder.weight'] * 2.0 ** -k
        sd['y_encoder.weight'] = sd0['y_encoder.weight'] * 2.0 ** -k
        model.load_state_dict(sd)
        model.zero_grad()
        logits = model((x * 2.0 ** k, y * 2.0 ** k), single_eval_pos=sep)
        loss = model.criterion(logits.reshape(-1, NBARS), y[sep:].reshape(-1)).mean()
        loss.backward()
        return logits.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}

    logits0, grads0 = run_k(0)
    assert torch.isfinite(logits0).all() and all(torch.isfinite(g).all() for g in grads0.values())
    for k in (-24, -10, 10, 24):
        logits, grads = run_k(k)
        assert torch.equal(logits, logits0), (k, relerr(logits, logits0))
        for n, g in grads.items():
            want = grads0[n] * 2.0 ** k if n in ('encoder.weight', 'y_encoder.weight') else grads0[n]
            assert torch.equal(g, want), (k, n, relerr(g, want))


# ---- C. caller layouts --------------------------------------------------------------------------------------------------------------------------------------
def _layouts(x, y):
    """(name, x as passed, y as passed): each holds the values of the contiguous f32 (x.float().contiguous(), y.float().contiguous()) of itself"""
    F = x.shape[2]
    bt = torch.empty(B, T, F, device=DEV)
    bt.copy_(x.transpose(0, 1))
    big = torch.zeros(T, B, F + 2, device=DEV)
    big[..., 1:F + 1] = x
    y2 = torch.zeros(T, B, 2, device=DEV)
    y2[..., 1] = y
    cases = [('x [B,T,F] transposed', bt.transpose(0, 1), y),
             ('x feature slice', big[..., 1:F + 1], y),
             ('x expanded over the batch', x[:, :1].expand(T, B, F), y),
             ('y column of [T,B,2]', x, y2[..., 1]),
             ('y expanded', x, y[:, :1].expand(T, B)),
             ('float64', x.double(), y.double()),
             ('float16', x.half(), y.half())]
    assert cases[1][1].data_ptr() % 16 != 0 and cases[2][1].stride(1) == 0 and cases[4][2].stride(1) == 0
    return cases


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('nf', [5, 60])
def test_caller_layouts_give_the_contiguous_result_bit_for_bit(nf, precision):
    model = make_model(nf, precision, deterministic=True, column_scales=False).to(DEV).train()
    x, y = make_data(nf, seed=3, column_scales=False)      # (the float16 copy must hold the values)
    x, y = x.to(DEV), y.to(DEV)
    for name, xv, yv in _layouts(x, y):
        want_logits, want = run(model, xv.float().contiguous(), yv.float().contiguous(), 64)
        logits, grads = run(model, xv, yv, 64)
        assert torch.equal(logits, want_logits), name
        for n in want:
            assert torch.equal(grads[n], want[n]), (name, n)


# ---- D. gradient ingress ------------------------------------------------------------------------------------------------------------------------------------
class _MisalignedGradient(torch.autograd.Function):
    """identity whose backward hands on the incoming gradient as a contiguous view 4 bytes past a 16-byte boundary (as torch.cat's backward does for the
    second part when rows * n_out is not a multiple of 4)"""
    seen = []

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        n = g.numel()
        buf = torch.empty(n + 4, dtype=g.dtype, device=g.device)
        out = buf[1:1 + n].view(g.shape)
        out.copy_(g)
        _MisalignedGradient.seen.append(out.data_ptr() % 16)
        return out


@pytest.mark.parametrize('precision', PRECISIONS)
def test_misaligned_incoming_gradient(precision):
    nf, sep = 5, 64
    model = make_model(nf, precision, deterministic=True).to(DEV).train()
    x, y = make_data(nf, seed=4)
    x, y = x.to(DEV), y.to(DEV)
    _, want = run(model, x, y, sep)
    model.zero_grad()
    _MisalignedGradient.seen.clear()
    logits = _MisalignedGradient.apply(model((x, y), single_eval_pos=sep))
    model.criterion(logits.reshape(-1, NBARS), y[sep:].reshape(-1)).mean().backward()
    assert _MisalignedGradient.seen == [4]
    for n, p in model.named_parameters():
        assert torch.equal(p.grad, want[n]), n


class _OffsetPositions(nn.Module):
    """a positional encoding that returns its input as a contiguous view one float past a 16-byte boundary (offset=True) or at the boundary"""
    def __init__(self, offset):
        super().__init__()
        self.offset, self.seen = offset, []

    def forward(self, emb):
        o = 1 if self.offset else 0
        buf = torch.zeros(emb.numel() + 4, dtype=emb.dtype, device=emb.device)
        view = buf[o:o + emb.numel()].view(emb.shape)
        view.copy_(emb)
        self.seen.append(view.data_ptr() % 16)
        return view


@pytest.mark.parametrize('precision', PRECISIONS)
def test_misaligned_pre_embedded_src(precision):
    """a custom positional encoding makes the stack take src [S,B,E] from PyTorch; a contiguous view at an offset is aligned on the host before any launch"""
    nf, sep = 5, 64
    x, y = make_data(nf, seed=5)
    x, y = x.to(DEV), y.to(DEV)
    out = {}
    for offset in (False, True):
        pos = _OffsetPositions(offset)
        model = make_model(nf, precision, deterministic=True, pos_encoder=pos).to(DEV).train()
        out[offset] = run(model, x, y, sep)
        assert pos.seen == [4 if offset else 0]
    assert torch.equal(out[True][0], out[False][0])
    for n in out[False][1]:
        assert torch.equal(out[True][1][n], out[False][1][n]), n


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('nf', [5, 60, 200])
def test_no_train_rows_leave_the_y_encoder_gradients_zero(nf, precision):
    model = make_model(nf, precision).to(DEV).train()
    x, y = make_data(nf, seed=6)
    _, grads = run(model, x.to(DEV), y.to(DEV), 0)
    assert torch.count_nonzero(grads['y_encoder.weight']) == 0 and torch.count_nonzero(grads['y_encoder.bias']) == 0
    assert torch.count_nonzero(grads['encoder.weight']) > 0 and all(torch.isfinite(g).all() for g in grads.values())


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('nf', [5, 60, 200])
def test_no_test_rows_leave_every_gradient_zero(nf, precision):
    model = make_model(nf, precision).to(DEV).train()
    x, y = make_data(nf, seed=7)
    model.zero_grad()
    logits = model((x.to(DEV), y.to(DEV)), single_eval_pos=T)
    assert logits.shape == (0, B, NBARS)
    logits.sum().backward()
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.count_nonzero(p.grad) == 0, n
