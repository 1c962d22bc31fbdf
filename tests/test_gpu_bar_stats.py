"""Posterior summaries and draws of the bar distribution on the MI355X (pfn_bar_stats / pfn_bar_stats_backward / pfn_bar_sample) against the f64
reference tests/bar_f64.py.  Every bound is 2 x the largest value measured on the MI355X (tests/bounds.py; profiles/r09_bar_stats_bounds_measured.json).

Two remarks on what the figures mean:
  * the ICDF walks the cumulative sums from the left in f32, so a level is resolved to about 1e-7 ABSOLUTE in probability: the residual |F(Q) - u| is
    small everywhere, but at u = 1 - 1e-6 the remaining mass 1e-6 is known to a few per cent only, and so is the density there -- the gradient of that
    column is recorded under its own label ('extreme levels') next to the central levels, and the VJP over all columns is recorded as the issue asks;
  * dQ/dlogits jumps where u meets a cumulative sum C_k (the density changes from bucket k to k + 1) and f32 / f64 can land on different sides of such
    a tie (all-equal rows: C_k = (k + 1) / n meets .5, .025, ... exactly).  Q itself is continuous there and stays checked; the cotangent of such a
    (row, level) pair is set to zero on both sides in the VJP comparison (`ties`)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bar_f64  # noqa: E402
from bounds import within  # noqa: E402
from oracle import pfn_oracle  # noqa: E402
from transformerscandobayesianinference_amd import _hip, bar_distribution, encoders  # noqa: E402
from transformerscandobayesianinference_amd.transformer import TransformerModel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

U = [1e-6, .025, .159, .5, .841, .975, 1 - 1e-6]
KIND = dict(mean=0, variance=1, mode=2, cdf=3, icdf=4, ei_max=5, ei_min=6)
NAMES16 = ['mean', 'variance', 'mode', 'cdf', 'cdf', 'ei_max', 'ei_min'] + ['icdf'] * 7 + ['cdf', 'ei_max']
ICDF0 = 7                                                     # columns 7 .. 13: the levels U in order
YSLOTS = [j for j, nm in enumerate(NAMES16) if nm in ('cdf', 'ei_max', 'ei_min')]

# 2 x the largest value measured on the MI355X (profiles/r09_bar_stats_bounds_measured.json)
BOUNDS = {
    'mean rel': 1.8e-7, 'variance rel': 2.3e-7, 'cdf rel': 5.2e-7, 'ei rel': 5.2e-7,                    # measured 8.8e-8, 1.14e-7, 2.6e-7, 2.6e-7
    'icdf probability residual': 7.7e-4,                                                                 # 3.8e-4: one f32 step of Q in a bucket of width 1.3e-3 that holds all the mass
    'icdf probability residual beyond the f32 neighbours of Q': 7.0e-7,                                  # 3.5e-7
    'icdf vs quantile, rel span': 6.6e-6,                                                                # 3.3e-6
    'vjp rel l2, all columns': 2.7e-2, 'vjp rel l2, icdf extreme levels': 4.9e-1,                        # 1.3e-2, 2.4e-1 (u = 1 - 1e-6: see the module docstring)
    'vjp rel l2, without icdf': 2.0e-5, 'vjp rel l2, icdf central levels': 1.2e-4,                       # 9.7e-6, 5.8e-5
    'sample ecdf': 0.06,                                                                                 # the issue's figure (DKW); measured 1.3e-2
    'e2e f32 dx rel l2': 2.1e-6, 'e2e fp16 dx rel l2': 1.9e-3,                                           # 1.0e-6, 9.0e-4
}


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def make_borders(n, gen):
    w = torch.rand(n + 1, generator=gen) + 0.1
    b = torch.cumsum(w, 0)
    return ((b - b[0]) / (b[-1] - b[0]) * 6.5 - 3.0).float()      # uneven widths over [-3, 3.5]


def make_rows(R, n, gen, first_type=0):
    """row r is of type (first_type + r) % 4: smooth / all equal / nearly one-hot (one logit + 50) / half the logits -1e4 (those p_i are exactly 0)"""
    rows = []
    for r in range(R):
        t = (first_type + r) % 4
        if t == 0:
            row = 3 * torch.sin(torch.linspace(0, 3.1, n) + 0.37 * r) + 0.3 * torch.randn(n, generator=gen)
        elif t == 1:
            row = torch.full((n,), 0.7)
        elif t == 2:
            row = 0.5 * torch.randn(n, generator=gen)
            row[[0, n - 1, n // 2, (7 * r) % n][(r // 4) % 4]] += 50.
        else:
            row = torch.randn(n, generator=gen)
            dead = torch.randperm(n, generator=gen)[:n // 2]
            row[dead] = -1e4
        rows.append(row)
    return torch.stack(rows).float()


def y_values(b):
    n = len(b) - 1
    w = b[1:] - b[:-1]
    j = n // 3
    return torch.stack([b[0], b[min(1, n)], b[n // 2], b[j] + 0.3 * w[j], b[0] - 0.7 * w[0], b[n] + 1.3 * w[n - 1], b[0] + 0.4 * w[0],
                        b[n - 1] + 0.6 * w[n - 1], b[n]]).float()      # borders exactly, inside a bucket, outside the support, inside both tail buckets


def place(t, ld, misaligned):
    """t [R, n] on the device with row stride ld; misaligned: the first row starts 4 bytes past a 16-byte boundary.  Padding holds NaN."""
    R, n = t.shape
    buf = torch.full((R * ld + 8,), float('nan'), device=DEV)
    off = 1 if misaligned else 0
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + R * ld].view(R, ld)
    view[:, :n] = t.to(DEV)
    assert (view.data_ptr() % 16 != 0) == misaligned
    return buf, view


def c_kinds(names):
    return (ctypes.c_int32 * len(names))(*[KIND[nm] for nm in names])


def raw_stats(view, n, borders, full, names, args, arg_ld):
    R, ld = view.shape
    out = torch.full((R, len(names)), float('nan'), device=DEV)
    ck = c_kinds(names)
    _hip.check(_hip.lib().pfn_bar_stats(view.data_ptr(), ld, borders.data_ptr(), R, n, int(full), ctypes.addressof(ck), len(names), args.data_ptr(), arg_ld,
                                        out.data_ptr(), _hip.stream_ptr(view.device)), 'pfn_bar_stats')
    return out


def raw_backward(view, n, borders, full, names, args, arg_ld, out, gout, misaligned):
    R, ld = view.shape
    dbuf, dview = place(torch.zeros(R, n), ld, misaligned)
    dview[:, :n] = float('inf')      # every element must be written
    ck = c_kinds(names)
    _hip.check(_hip.lib().pfn_bar_stats_backward(view.data_ptr(), ld, borders.data_ptr(), R, n, int(full), ctypes.addressof(ck), len(names), args.data_ptr(), arg_ld,
                                                 out.data_ptr(), gout.data_ptr(), dview.data_ptr(), _hip.stream_ptr(view.device)), 'pfn_bar_stats_backward')
    torch.cuda.synchronize()
    # nothing outside [R, n] was touched: the padding columns and the words around the buffer still hold NaN
    inside = torch.zeros_like(dbuf, dtype=torch.bool)
    off = 1 if misaligned else 0
    inside[off:off + R * ld].view(R, ld)[:, :n] = True
    assert torch.isnan(dbuf[~inside]).all()
    return dview[:, :n].clone()


def run_config(n, full, R, ld_extra, misaligned, per_row, names, gen, first_type=0, arg_set=0):
    """one launch of the forward and the backward through the C ABI, every assertion of the issue on it"""
    cls = 'full' if full else 'bounded'
    b = make_borders(n, gen)
    logits = make_rows(R, n, gen, first_type)
    span = (b[-1] - b[0]).double().item()
    ys = y_values(b)
    K = len(names)
    # arguments: f32 values, [K] shared or [R, K + 2] per row
    argm = torch.zeros(R, K)
    for j, nm in enumerate(names):
        if nm == 'icdf':
            argm[:, j] = U[(j - ICDF0) % 7] if K == 16 else U[(arg_set + 3) % 7]
        elif nm in ('cdf', 'ei_max', 'ei_min'):
            rows = torch.arange(R) if per_row else torch.zeros(R, dtype=torch.long)
            argm[:, j] = ys[(j + 6 * arg_set + rows) % len(ys)]
    if per_row:
        args = torch.full((R, K + 2), float('nan'))
        args[:, :K] = argm
        arg_ld = K + 2
    else:
        args, arg_ld = argm[0].clone(), 0
    args = args.to(DEV)
    bd = b.to(DEV)
    _, view = place(logits, n + ld_extra, misaligned)
    out = raw_stats(view, n, bd, full, names, args, arg_ld)
    torch.cuda.synchronize()
    got = out.cpu().double()
    assert torch.isfinite(got).all()

    lg64 = logits.double().requires_grad_(True)
    spec = [(nm, argm[:, j].double()) if nm in ('cdf', 'icdf', 'ei_max', 'ei_min') else (nm,) for j, nm in enumerate(names)]
    ref = bar_f64.stats(lg64, b, full, spec)
    scale = {'mean': span, 'variance': span * span, 'cdf': 1., 'ei_max': span, 'ei_min': span}
    crit = (bar_distribution.FullSupportBarDistribution if full else bar_distribution.BarDistribution)(b.clone())
    icdf_cols = [j for j, nm in enumerate(names) if nm == 'icdf']
    for j, nm in enumerate(names):
        if nm in scale:
            err = ((got[:, j] - ref[:, j].detach()).abs() / ref[:, j].detach().abs().clamp_min(scale[nm])).max().item()
            within(f'{cls} {nm.split("_")[0]} rel', err, BOUNDS[f'{nm.split("_")[0]} rel'])
        elif nm == 'mode':
            want = bar_distribution.BarDistribution.bucket_means(crit)[logits.argmax(-1)]      # the reference's definition, in its f32 arithmetic
            assert torch.equal(out[:, j].cpu(), want)
        else:
            q = got[:, j]
            res = (bar_f64.cdf(logits, b, full, q) - argm[:, j].double()).abs().max().item()
            within(f'{cls} icdf probability residual', res, BOUNDS['icdf probability residual'])
            # the part of it that is not the f32 grid of Q: the mass between the two f32 neighbours of Q is what no f32 answer can resolve
            q32 = out[:, j].cpu()
            up, down = torch.nextafter(q32, torch.full_like(q32, float('inf'))).double(), torch.nextafter(q32, torch.full_like(q32, float('-inf'))).double()
            grid = bar_f64.cdf(logits, b, full, up) - bar_f64.cdf(logits, b, full, down)
            beyond = ((bar_f64.cdf(logits, b, full, q) - argm[:, j].double()).abs() - grid).clamp_min(0).max().item()
            within(f'{cls} icdf probability residual beyond the f32 neighbours of Q', beyond, BOUNDS['icdf probability residual beyond the f32 neighbours of Q'])
            if not full:
                assert (out[:, j].cpu() >= b[0]).all() and (out[:, j].cpu() <= b[-1]).all()
    if K == 16:
        q = out[:, ICDF0:ICDF0 + 7].cpu()
        assert (q[:, 1:] >= q[:, :-1]).all(), 'Q is not monotone in u'
        if not full:      # against the existing quantile, on the rows where that is the quantile (tests/test_host_bar_stats.py::reference_wraps)
            p = torch.softmax(logits.double(), -1)
            for center, lo_col, hi_col in ((.682, 2, 4), (.95, 1, 5)):
                side = (1 - center) / 2
                old = crit.to(DEV).quantile(logits.to(DEV), center_prob=center).double()
                ok = torch.stack([p[:, 0] < side * (1 - 1e-4), p[:, -1] < side * (1 - 1e-4)], -1)
                new = torch.stack([got[:, ICDF0 + lo_col], got[:, ICDF0 + hi_col]], -1)
                if ok.any():
                    within('bounded icdf vs quantile, rel span', ((new - old).abs()[ok] / span).max().item(), BOUNDS['icdf vs quantile, rel span'])

    # backward: VJP with a random cotangent against autograd through the f64 reference
    gout = torch.randn(R, K, generator=gen)
    cum = torch.cumsum(torch.softmax(logits.double(), -1), -1)
    ties = 0
    for j in icdf_cols:
        u = argm[:, j].double()
        tie = ((cum - u[:, None]).abs().min(-1).values < 1e-5 * torch.minimum(u, 1 - u))
        gout[tie, j] = 0.
        ties += int(tie.sum())
    mode_cols = [j for j, nm in enumerate(names) if nm == 'mode']
    groups = {'all columns': list(range(K)),
              'without icdf': [j for j in range(K) if j not in icdf_cols],
              'icdf central levels': [j for j in icdf_cols if 1e-3 < argm[0, j] < 1 - 1e-3],
              'icdf extreme levels': [j for j in icdf_cols if not 1e-3 < argm[0, j] < 1 - 1e-3]}
    for label, cols in groups.items():
        if not cols:
            continue
        g = torch.zeros_like(gout)
        g[:, cols] = gout[:, cols]
        if not g.any():
            continue
        dl = raw_backward(view, n, bd, full, names, args, arg_ld, out, g.to(DEV), misaligned).cpu()
        assert torch.isfinite(dl).all()
        (want,) = torch.autograd.grad((ref * g.double()).sum(), lg64, retain_graph=True)
        if want.norm() == 0:      # a single bucket (p = 1 whatever the logit) or only zero-gradient columns: f32 round-off of O(span^2) terms at the most
            assert dl.abs().max().item() <= 1e-5 * max(span * span, 1.) * g.abs().max().item()
        else:
            within(f'{cls} vjp rel l2, {label}', relerr(dl, want), BOUNDS[f'vjp rel l2, {label}'])
    if mode_cols:      # the MODE column contributes exactly 0
        g = torch.zeros(R, K)
        g[:, mode_cols] = 3.
        dl = raw_backward(view, n, bd, full, names, args, arg_ld, out, g.to(DEV), misaligned)
        assert torch.count_nonzero(dl).item() == 0
    return ties


NBARS = [2, 7, 100, 1000, 1003, 5000]


# (a full-support distribution has two tail buckets: nbars = 1 is PFN_ERR_ARGUMENT there, tests/test_host_bar_stats.py)
@pytest.mark.parametrize('n,full', [(1, False)] + [(n, f) for n in NBARS for f in (False, True)])
def test_stats_and_backward_vs_f64(n, full):
    gen = torch.Generator().manual_seed(100 * n + full)
    for arg_set in (0, 1):      # together the two sets put every y value in a CDF and in an EI slot
        run_config(n, full, R=5, ld_extra=0, misaligned=False, per_row=False, names=NAMES16, gen=gen, arg_set=arg_set)
        run_config(n, full, R=5, ld_extra=3, misaligned=True, per_row=True, names=NAMES16, gen=gen, first_type=1, arg_set=arg_set)
    for t, nm in enumerate(['mean', 'variance', 'mode', 'cdf', 'icdf', 'ei_max', 'ei_min']):      # K = 1, R = 1
        run_config(n, full, R=1, ld_extra=3 * (t % 2), misaligned=bool(t % 2), per_row=bool(t & 2), names=[nm], gen=gen, first_type=t, arg_set=t)


@pytest.mark.parametrize('full', [False, True], ids=['bounded', 'full'])
@pytest.mark.parametrize('n', [7, 100])
def test_many_rows(n, full):
    gen = torch.Generator().manual_seed(7 * n + full)
    run_config(n, full, R=4097, ld_extra=3, misaligned=True, per_row=True, names=NAMES16, gen=gen)
    run_config(n, full, R=4097, ld_extra=0, misaligned=False, per_row=False, names=['icdf'], gen=gen, arg_set=2)


def test_python_api_matches_the_c_abi_and_differentiates():
    """stats / variance / cdf / icdf / median / pi / ucb: spec parsing, broadcasting of tensor arguments, leading dimensions, autograd"""
    gen = torch.Generator().manual_seed(3)
    n = 100
    b = make_borders(n, gen)
    crit = bar_distribution.FullSupportBarDistribution(b.clone()).to(DEV)
    logits = make_rows(12, n, gen).view(4, 3, n).to(DEV)
    best = torch.tensor([0.1, -0.4, 1.2], device=DEV)      # one per dataset: broadcasts over the leading dimension
    spec = [('mean',), 'variance', ('icdf', .159), ('icdf', .841), ('ei', best), ('ei', 0.3, False), ('cdf', torch.full((4, 3), 0.25, device=DEV)), ('mode',)]
    lg = logits.clone().requires_grad_(True)
    s = crit.stats(lg, spec)
    assert s.shape == (4, 3, 8) and s.requires_grad
    flat = logits.reshape(12, n).cpu()
    ref_spec = [('mean',), ('variance',), ('icdf', .159), ('icdf', .841), ('ei_max', best.cpu().repeat(4)), ('ei_min', 0.3), ('cdf', 0.25), ('mode',)]
    lg64 = flat.double().requires_grad_(True)
    ref = bar_f64.stats(lg64, b, True, [(sp[0], torch.as_tensor(sp[1]).float().double()) if len(sp) > 1 else sp for sp in ref_spec])
    within('api forward rel l2', relerr(s.reshape(12, 8), ref), 1e-5)      # ~100 f32 eps: sums over 100 buckets
    g = torch.randn(4, 3, 8, generator=gen)
    (d,) = torch.autograd.grad((s * g.to(DEV)).sum(), lg)
    (want,) = torch.autograd.grad((ref * g.reshape(12, 8).double()).sum(), lg64)
    within('api vjp rel l2', relerr(d.reshape(12, n), want), 1e-4)
    with torch.no_grad():
        assert torch.equal(crit.stats(logits, spec), s.detach())
        assert torch.equal(crit.variance(logits), s[..., 1].detach()) and torch.equal(crit.icdf(logits, .159), s[..., 2].detach())
        assert torch.equal(crit.ucb(logits, rest_prob=.159), crit.icdf(logits, 1 - .159)) and torch.equal(crit.ucb(logits, .159, maximize=False), s[..., 2].detach())
        assert torch.equal(crit.median(logits), crit.icdf(logits, .5))
        assert torch.equal(crit.cdf(logits, 0.25), s[..., 6].detach())
        assert torch.equal(crit.pi(logits, 0.25), 1 - crit.cdf(logits, 0.25)) and torch.equal(crit.pi(logits, 0.25, maximize=False), crit.cdf(logits, 0.25))
        assert torch.equal(crit.stats(logits, [('mean',)])[..., 0], s[..., 0].detach())
        assert crit.stats(logits[:0], spec[:2]).shape == (0, 3, 2) and crit.sample(logits[:0], 5, seed=1).shape == (5, 0, 3)
    with pytest.raises(ValueError):
        crit.stats(logits, [('cdf', torch.zeros(4, 3, device=DEV, requires_grad=True))])
    with pytest.raises(ValueError):
        crit.stats(logits, [('mean',)] * 17)
    with pytest.raises(ValueError):
        crit.stats(logits, [('skewness',)])
    with pytest.raises(ValueError):
        crit.stats(logits, [('icdf',)])


# ---- draws ---------------------------------------------------------------------------------------------------------------------------------------------
def uniforms(seed, R, n_samples):
    """u[s, r] of pfn_bar_sample, restated from include/pfn_hip.h with the oracle's mix32"""
    M = 0xFFFFFFFF
    mix = pfn_oracle._mix32
    r = np.arange(R, dtype=np.uint64)
    s = np.arange(n_samples, dtype=np.uint64)
    a = mix(np.uint64(seed & M) ^ ((r & np.uint64(M)) * np.uint64(0x9E3779B1) & np.uint64(M)))
    b = mix(a ^ np.uint64(seed >> 32) ^ (((r >> np.uint64(32)) * np.uint64(0x85EBCA77)) & np.uint64(M)))
    h = mix(b[None, :] ^ ((s * np.uint64(0xC2B2AE35)) & np.uint64(M))[:, None])
    u = ((h >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    assert (u.astype(np.float32).astype(np.float64) == u).all() and u.min() > 0 and u.max() < 1
    return torch.from_numpy(u.astype(np.float32))


@pytest.mark.parametrize('full', [False, True], ids=['bounded', 'full'])
@pytest.mark.parametrize('n', [7, 1000, 5000])
def test_sample_is_the_icdf_at_the_documented_uniforms(n, full):
    gen = torch.Generator().manual_seed(n + full)
    b = make_borders(n, gen)
    crit = (bar_distribution.FullSupportBarDistribution if full else bar_distribution.BarDistribution)(b).to(DEV)
    logits = make_rows(9, n, gen).to(DEV)
    seed, S = 0x9E3779B97F4A7C15, 70      # both halves of the seed in use; more draws than lanes
    got = crit.sample(logits, S, seed=seed)
    assert got.shape == (S, 9) and torch.isfinite(got).all()
    u = uniforms(seed, 9, S).to(DEV)
    for s0 in range(0, S, 16):
        want = crit.stats(logits, [('icdf', u[s]) for s in range(s0, min(S, s0 + 16))])
        assert torch.equal(got[s0:s0 + 16].T, want), s0
    assert torch.equal(crit.sample(logits, S, seed=seed), got)
    other = crit.sample(logits, S, seed=seed + 1)
    assert not torch.equal(other, got) and (other != got).float().mean() > 0.9
    assert torch.equal(crit.sample(logits.view(3, 3, n), S, seed=seed), got.view(S, 3, 3))
    torch.manual_seed(11)
    a1 = crit.sample(logits, 4)
    torch.manual_seed(11)
    assert torch.equal(crit.sample(logits, 4), a1) and not torch.equal(crit.sample(logits, 4), a1)      # seed=None: from torch's generator


@pytest.mark.parametrize('full', [False, True], ids=['bounded', 'full'])
def test_sample_distribution(full):
    """8 rows x 4096 draws: the empirical CDF at every border and four tail points within 0.06 of the f64 F -- by the Dvoretzky-Kiefer-Wolfowitz bound
    2 exp(-2 * 4096 * 0.06^2) < 1e-12 per row for a correct sampler, and deterministic once it passes (fixed seed) -- and the sample mean within 6 standard errors."""
    gen = torch.Generator().manual_seed(17 + full)
    n, S = 100, 4096
    b = make_borders(n, gen)
    crit = (bar_distribution.FullSupportBarDistribution if full else bar_distribution.BarDistribution)(b).to(DEV)
    logits = make_rows(8, n, gen)
    x = crit.sample(logits.to(DEV), S, seed=2024).cpu().double()      # [S, 8]
    assert torch.isfinite(x).all()
    w = (b[1:] - b[:-1]).double()
    pts = torch.cat([b.double(), torch.stack([b[0] - 2 * w[0], b[0] - 0.5 * w[0], b[-1] + 0.5 * w[-1], b[-1] + 2 * w[-1]]).double()])
    worst = 0.
    for y in pts:
        ecdf = (x <= y).double().mean(0)
        worst = max(worst, (ecdf - bar_f64.cdf(logits, b, full, y.item())).abs().max().item())
    within(f'{"full" if full else "bounded"} sample ecdf', worst, BOUNDS['sample ecdf'])
    mean, var = bar_f64.mean(logits, b, full), bar_f64.variance(logits, b, full)
    assert ((x.mean(0) - mean).abs() < 6 * (var / S).sqrt()).all()


# ---- end to end: grad_x of acquisition values through predict ---------------------------------------------------------------------------------------------
def make_model(E, H, precision, nbars=100):
    torch.manual_seed(0)
    m = TransformerModel(encoders.Linear(5, E), nbars, E, H, 2 * E, 2, 0.0, y_encoder=encoders.Linear(1, E), precision=precision, eval_precision=precision)
    m.criterion = bar_distribution.FullSupportBarDistribution(torch.sort(torch.randn(nbars + 1) * 1.5)[0])
    with torch.no_grad():
        for layer in m.transformer_encoder.layers:
            for t in (layer.linear2.weight, layer.self_attn.out_proj.weight):
                t.normal_(0, 0.03)
    return m.to(DEV).eval()


@pytest.mark.parametrize('precision', ['f32', 'fp16'])
@pytest.mark.parametrize('E,H,sep,n,B', [(128, 4, 437, 7, 3), (256, 2, 1, 60, 3)])      # two shapes of tests/test_gpu_predict_grad.py
def test_acquisition_gradient_through_predict(E, H, sep, n, B, precision):
    model = make_model(E, H, precision)
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(sep + n, B, 5, generator=g).to(DEV), torch.randn(sep + n, B, generator=g).to(DEV)
    crit = model.criterion
    best = 0.5
    spec = [('ei', best), ('icdf', .9), ('variance',)]
    ctx = model.condition((x[:sep], y[:sep]))
    xt = x[sep:].detach().clone().requires_grad_(True)
    val = crit.stats(model.predict(ctx, xt), spec)
    assert val.shape == (n, B, 3) and val.requires_grad
    (dx,) = torch.autograd.grad(val.sum(-1).sum(), xt)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if not k.startswith('criterion.')}
    xo = x.detach().cpu().double().requires_grad_(True)
    lo = pfn_oracle.forward(sd, xo, y.cpu().double(), sep, H)
    vo = bar_f64.stats(lo.reshape(n * B, -1), crit.borders.cpu(), True, [('ei_max', best), ('icdf', float(np.float32(.9))), ('variance',)])
    (dxo,) = torch.autograd.grad(vo.sum(-1).sum(), xo)
    within(f'e2e {precision} dx rel l2', relerr(dx, dxo[sep:]), BOUNDS[f'e2e {precision} dx rel l2'])
    # without grad: the fused kernels only (no PyTorch softmax anywhere), and the same bits
    with torch.no_grad(), torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        plain = crit.stats(model.predict(ctx, x[sep:]), spec)
    assert torch.equal(plain, val.detach())
    assert not [e.name for e in prof.events() if 'softmax' in e.name.lower()]
