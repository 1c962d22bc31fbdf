"""Input gradients on the MI355X (ABI 10): d(predict(context, x_test))/d(x_test) through the cached train rows (pfn_stack_predict_saved /
pfn_stack_predict_backward), d(x) and d(y) of the full forward (pfn_stack_input_grads), and the differentiable posterior mean (pfn_bar_mean_backward).
The oracle is oracle.pfn_oracle.forward in f64 on cat(x_train, x_test), differentiated by torch.autograd.  Bounds at 2 x measured (tests/bounds.py;
profiles/r08_predict_grad_bounds_measured.json)."""
import pytest
import torch

from oracle import pfn_oracle
from bounds import within
from transformerscandobayesianinference_amd import _hip, bar_distribution, decoders, encoders
from transformerscandobayesianinference_amd.transformer import TransformerModel

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PFN_TUNE_ATTN_CACHE_SPLITS = 17


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def make(E, H, precision='f32', eval_precision='same', L=2, F=5, nbars=100, seed=0, schedule=None, decoder=None):
    torch.manual_seed(seed)
    m = TransformerModel(encoders.Linear(F, E), nbars, E, H, 2 * E, L, 0.0, y_encoder=encoders.Linear(1, E), decoder=decoder, precision=precision,
                         eval_precision=precision if eval_precision == 'same' else eval_precision)
    m.criterion = bar_distribution.FullSupportBarDistribution(torch.sort(torch.randn(nbars + 1) * 1.5)[0])
    with torch.no_grad():
        for layer in m.transformer_encoder.layers:      # un-zero the residual branches
            for t in (layer.linear2.weight, layer.self_attn.out_proj.weight):
                t.normal_(0, 0.03)
    if schedule is not None:
        m.schedule = schedule
    return m.to(DEV).eval()


def data(sep, n, B, F=5, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(sep + n, B, F, generator=g).to(DEV), torch.randn(sep + n, B, generator=g).to(DEV)


def params_of(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if not k.startswith('criterion.')}


def oracle_input_grads(model, x, y, sep, H, R):
    """f64 oracle: logits of cat(x_train, x_test) and d((logits * R).sum()) / d(x), d(y)"""
    xo = x.detach().cpu().double().requires_grad_(True)
    yo = y.detach().cpu().double().requires_grad_(True)
    lo = pfn_oracle.forward(params_of(model), xo, yo, sep, H)
    dx, dy = torch.autograd.grad((lo * R.cpu().double()).sum(), (xo, yo))
    return lo, dx, dy


def predict_vjp(model, ctx, xt, R):
    xt = xt.detach().clone().requires_grad_(True)
    out = model.predict(ctx, xt)
    assert out.requires_grad
    (dx,) = torch.autograd.grad((out * R).sum(), xt)
    return out, dx


class split_cap:
    """PFN_TUNE_ATTN_CACHE_SPLITS for the duration of a block (0 = the rule), restored afterwards"""

    def __init__(self, cap):
        self.cap = cap

    def __enter__(self):
        _hip.check(_hip.lib().pfn_set_tuning(PFN_TUNE_ATTN_CACHE_SPLITS, self.cap), 'pfn_set_tuning')

    def __exit__(self, *exc):
        _hip.check(_hip.lib().pfn_set_tuning(PFN_TUNE_ATTN_CACHE_SPLITS, 0), 'pfn_set_tuning')


# (emsize, heads, sep, n, B): head dims 32 / 64 / 128 / 256; sep in {0, 1, 437}, n in {1, 7, 60}, B in {1, 3}
CASES = [
    (128, 4, 437, 7, 3),     # D 32
    (128, 4, 1, 60, 1),
    (128, 2, 0, 7, 3),       # D 64, no train rows
    (128, 2, 437, 60, 3),
    (256, 2, 437, 1, 1),     # D 128
    (256, 2, 1, 7, 3),
    (256, 1, 437, 7, 3),     # D 256
    (512, 2, 0, 60, 1),
]
BOUND = {'f32': 2e-6, 'fp16': 1.7e-3, 'bf16': 1.4e-2}      # measured 8.8e-7 / 8.1e-4 / 7.0e-3 (the issue's ceilings: 1e-4 / 5e-3 / 2e-2)


@pytest.mark.parametrize('cap', [0, 1], ids=['splits', 'one_pass'])
@pytest.mark.parametrize('E,H,sep,n,B', CASES)
def test_predict_vjp_vs_oracle_f32(E, H, sep, n, B, cap):
    model = make(E, H, 'f32', 'f32')
    x, y = data(sep, n, B)
    R = torch.randn(n, B, 100, generator=torch.Generator().manual_seed(7)).to(DEV)
    lo, dxo, _ = oracle_input_grads(model, x, y, sep, H, R)
    with split_cap(cap):
        ctx = model.condition((x[:sep], y[:sep]))
        out, dx = predict_vjp(model, ctx, x[sep:], R)
        with torch.no_grad():
            plain = model.predict(ctx, x[sep:])
    assert torch.equal(out.detach(), plain)      # the saved pass returns the plain pass's bits
    within('f32 logits rel l2 vs oracle', relerr(out, lo), 2e-6)
    within('f32 dx rel l2 vs oracle', relerr(dx, dxo[sep:]), BOUND['f32'])


@pytest.mark.parametrize('precision', ['fp16', 'bf16'])
@pytest.mark.parametrize('E,H,sep,n,B', [(128, 4, 437, 7, 3), (256, 2, 1, 60, 3), (256, 1, 437, 7, 1), (128, 2, 0, 60, 3)])
def test_predict_vjp_vs_oracle_16bit(precision, E, H, sep, n, B):
    model = make(E, H, precision, 'same')
    x, y = data(sep, n, B)
    R = torch.randn(n, B, 100, generator=torch.Generator().manual_seed(7)).to(DEV)
    lo, dxo, _ = oracle_input_grads(model, x, y, sep, H, R)
    ctx = model.condition((x[:sep], y[:sep]))
    out, dx = predict_vjp(model, ctx, x[sep:], R)
    with torch.no_grad():
        assert torch.equal(out.detach(), model.predict(ctx, x[sep:]))
    within(f'{precision} dx rel l2 vs oracle', relerr(dx, dxo[sep:]), BOUND[precision])


def full_forward_input_grads(model, x, y, sep, R, train=False):
    xg, yg = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    model.train(train)
    out = model((xg, yg), single_eval_pos=sep)
    dx, dy = torch.autograd.grad((out * R).sum(), (xg, yg))
    model.eval()
    return out, dx, dy


def test_long_context_vs_the_full_forward_input_gradient():
    """sep 2000, n 300, B 8 (beyond the f64 oracle's reach): predict's dx equals the test rows of the f32 full forward's dx, with and without key splits"""
    model = make(256, 2, 'f32', 'f32')
    sep, n, B = 2000, 300, 8
    x, y = data(sep, n, B)
    R = torch.randn(n, B, 100, generator=torch.Generator().manual_seed(7)).to(DEV)
    _, dxf, _ = full_forward_input_grads(model, x, y, sep, R)
    for cap in (0, 1):
        with split_cap(cap):
            ctx = model.condition((x[:sep], y[:sep]))
            _, dx = predict_vjp(model, ctx, x[sep:], R)
        within('f32 dx rel l2 vs full forward, sep 2000', relerr(dx, dxf[sep:]), 1.2e-6)


def test_context_and_gradients_untouched():
    model = make(128, 4, 'f32', 'f32')
    x, y = data(437, 60, 3)
    ctx = model.condition((x[:437], y[:437]))
    before = ctx.buffer.clone()
    flat_grad = model.flat_parameters()[1]
    flat_grad.zero_()
    predict_vjp(model, ctx, x[437:], torch.randn(60, 3, 100, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(ctx.buffer, before)
    assert not flat_grad.any()
    assert all(p.grad is None or not p.grad.any() for p in model.parameters())


def test_chunks_give_the_same_gradient(monkeypatch):
    model = make(128, 4, 'f32', 'f32')
    x, y = data(437, 60, 3)
    R = torch.randn(60, 3, 100, device=DEV)
    ctx = model.condition((x[:437], y[:437]))
    out1, dx1 = predict_vjp(model, ctx, x[437:], R)
    monkeypatch.setattr(TransformerModel, '_PREDICT_ROWS', 3 * 7)     # 7 rows x 3 datasets per chunk: 9 chunks, the last one short
    out2, dx2 = predict_vjp(model, ctx, x[437:], R)
    assert torch.equal(out1, out2)
    within('chunked dx rel l2 vs one call', relerr(dx2, dx1), 1e-6)


def test_custom_decoder_chains_its_gradient():
    model = make(128, 4, 'f32', 'f32', decoder=decoders.ScaledDecoder)
    sep, n, B = 437, 7, 3
    x, y = data(sep, n, B)
    ctx = model.condition((x[:sep], y[:sep]))
    xt = x[sep:].detach().clone().requires_grad_(True)
    out = model.predict(ctx, xt)
    R = torch.randn_like(out)
    (dx,) = torch.autograd.grad((out * R).sum(), xt)
    # the same decoder on the full forward's encoder rows
    xg = x.detach().clone().requires_grad_(True)
    full = model((xg, y), single_eval_pos=sep)
    (dxf,) = torch.autograd.grad((full * R).sum(), xg)
    within('custom decoder dx rel l2 vs full forward', relerr(dx, dxf[sep:]), 1e-6)


def test_fp16_loss_scale_with_large_cotangents():
    m16 = make(128, 4, 'fp16', 'same')
    m32 = make(128, 4, 'fp16', 'f32')
    sep, n, B = 437, 60, 3
    x, y = data(sep, n, B)
    R = 3e4 * torch.randn(n, B, 100, generator=torch.Generator().manual_seed(7)).to(DEV)
    _, dx16 = predict_vjp(m16, m16.condition((x[:sep], y[:sep])), x[sep:], R)
    _, dx32 = predict_vjp(m32, m32.condition((x[:sep], y[:sep])), x[sep:], R)
    assert torch.isfinite(dx16).all()
    within('fp16 dx rel l2 vs f32, large dlogits', relerr(dx16, dx32), 1.6e-3)


def test_bayesian_optimisation_quantities_vs_oracle():
    """grad_x of the expected improvement and of the posterior mean -- what optimize_acqf climbs -- against the same functions of the oracle's logits"""
    model = make(128, 4, 'f32', 'f32')
    sep, n, B, H = 437, 60, 3, 4
    x, y = data(sep, n, B)
    crit = model.criterion.to(DEV)
    ctx = model.condition((x[:sep], y[:sep]))
    xo = x.detach().cpu().double().requires_grad_(True)
    lo = pfn_oracle.forward(params_of(model), xo, y.cpu().double(), sep, H)
    for name, fn_h, fn_o in [
        ('ei', lambda lg: crit.ei(lg, 0.5).sum(), lambda lg: crit.ei(lg.to(DEV), 0.5).sum()),
        ('mean', lambda lg: crit.mean(lg).sum(), lambda lg: pfn_oracle.bar_mean(lg, crit.borders.cpu()).sum()),
    ]:
        xt = x[sep:].detach().clone().requires_grad_(True)
        val = fn_h(model.predict(ctx, xt))
        assert val.requires_grad, name
        (dx,) = torch.autograd.grad(val, xt)
        (dxo,) = torch.autograd.grad(fn_o(lo), xo, retain_graph=True)
        within(f'{name} dx rel l2 vs oracle', relerr(dx, dxo[sep:]), 1.2e-6)


def test_bar_mean_gradient():
    crit = bar_distribution.FullSupportBarDistribution(torch.sort(torch.randn(101) * 1.5)[0]).to(DEV)
    logits = torch.randn(50, 100, device=DEV, requires_grad=True)
    with torch.no_grad():
        assert torch.equal(crit.mean(logits), crit.mean(logits.detach()))
    g = torch.randn(50, device=DEV)
    (d,) = torch.autograd.grad((crit.mean(logits) * g).sum(), logits)
    lo = logits.detach().cpu().double().requires_grad_(True)
    (do,) = torch.autograd.grad((pfn_oracle.bar_mean(lo, crit.borders.cpu()) * g.cpu().double()).sum(), lo)
    within('bar mean dlogits rel l2 vs f64', relerr(d, do), 2e-7)


@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('precision', ['f32', 'fp16'])
def test_full_forward_input_grads(precision, train):
    sep, n, B, H = 437, 60, 3, 4
    model = make(128, H, precision, 'same', schedule=_hip.SCHED_DETERMINISTIC)
    x, y = data(sep, n, B)
    R = torch.randn(n, B, 100, generator=torch.Generator().manual_seed(7)).to(DEV)
    _, dxo, dyo = oracle_input_grads(model, x, y, sep, H, R)
    flat_grad = model.flat_parameters()[1]
    flat_grad.zero_()
    _, dx, dy = full_forward_input_grads(model, x, y, sep, R, train)
    with_inputs = flat_grad.clone()
    bound = {'f32': 1.1e-6, 'fp16': 1.7e-3}[precision]      # measured 5.3e-7 / 8.1e-4
    within(f'{precision} full forward dx rel l2 vs oracle', relerr(dx, dxo), bound)
    within(f'{precision} full forward dy rel l2 vs oracle', relerr(dy[:sep], dyo[:sep]), bound)
    assert not dy[sep:].any()
    # parameter gradients: the same bits as a backward that asks for no input gradient (deterministic schedule)
    flat_grad.zero_()
    model.train(train)
    out = model((x, y), single_eval_pos=sep)
    (out * R).sum().backward()
    model.eval()
    assert torch.equal(flat_grad, with_inputs)
    if precision == 'f32':      # the test rows' dx of the full forward and of predict's backward
        ctx = model.condition((x[:sep], y[:sep]))
        _, dxp = predict_vjp(model, ctx, x[sep:], R)
        within('f32 predict dx vs full forward dx', relerr(dxp, dx[sep:]), 1e-5)
