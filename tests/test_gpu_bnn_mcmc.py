"""The BNN posterior target on the device (csrc/bnn_mcmc.hip: pfn_bnn_logp_grad, pfn_bnn_predict) and what is built on it
(mcmc_svi_transformer_on_bayesian.sample_bnn_posterior / eval_mcmc) against the f64 restatement (tests/bnn_f64.py, verified on the host in
tests/test_host_bnn_mcmc.py), the f64 emulation of the NUTS state machine (tests/nuts_f64.py) and self-normalised importance sampling from the prior.

Bounds on continuous outputs: <= 2 x the value measured on the MI355X (profiles/r13_bnn_mcmc_bounds_measured.json), and never above 1e-3.  Errors of a
chain's value are relative to |value|, of its gradient to the gradient's norm; probabilities and sampled points are compared absolutely."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnn_f64 as ref      # noqa: E402
import bounds      # noqa: E402
import nuts_f64 as emu      # noqa: E402

from transformerscandobayesianinference_amd import hipops, mcmc      # noqa: E402
from transformerscandobayesianinference_amd import mcmc_svi_transformer_on_bayesian as study      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CAP = 1e-3
MARGIN = 1e-4
S = 100

# (H, F, P, K, activation, n_of): every H of {1, 5, 8, 9, 16, 33, 64}, F of {1, 3, 16}, n of {0, 1, 2, 63, 64, 65, 100}, P of {1, 3}, K of {1, 3, 9}; every
# Hp (8: H 1 / 5 / 8, 16: H 9 / 16, 32: H 33, 64: H 64) with every K, which leaves a partly filled last wave and last block for each.  F = 8 and 5 are the
# third width of the kernel's row registers (Fp = 8), exact and padded.
CASES = {
    'H1': (1, 1, 1, 1, 'identity', (100,)),
    'H5': (5, 3, 3, 3, 'tanh', (0, 63, 100)),
    'H8': (8, 16, 3, 9, 'identity', (1, 64, 65)),
    'H9': (9, 3, 3, 1, 'tanh', (2, 65, 100)),
    'H16a': (16, 1, 1, 3, 'identity', (64,)),
    'H16b': (16, 16, 3, 9, 'tanh', (0, 1, 63)),
    'H33a': (33, 3, 1, 1, 'identity', (65,)),
    'H33b': (33, 1, 3, 3, 'tanh', (2, 100, 64)),
    'H33c': (33, 16, 1, 9, 'identity', (100,)),
    'H64a': (64, 16, 3, 1, 'tanh', (63, 0, 2)),
    'H64b': (64, 3, 1, 3, 'identity', (1,)),
    'H64c': (64, 1, 3, 9, 'tanh', (65, 100, 64)),
    'F8': (11, 8, 3, 3, 'tanh', (100, 63, 1)),
    'F5': (5, 5, 1, 9, 'identity', (65,)),
}
# measured on the MI355X (profiles/r13_bnn_mcmc_bounds_measured.json): (value, gradient), each <= 2 x measured
VALUE_GRAD_BOUNDS = {
    'H1': (1.2e-7, 2.4e-7),
    'H5': (3.1e-7, 3.7e-7),
    'H8': (3.6e-7, 5.7e-7),
    'H9': (3.1e-7, 3.4e-7),
    'H16a': (2.9e-7, 3.2e-7),
    'H16b': (1.5e-7, 4.2e-7),
    'H33a': (7.3e-8, 2.9e-7),
    'H33b': (1.8e-7, 3.3e-7),
    'H33c': (2.4e-7, 4.8e-7),
    'H64a': (3.5e-8, 3.9e-7),
    'H64b': (6.7e-8, 4.8e-8),
    'H64c': (2.4e-7, 5.0e-7),
    'F8': (1.0e-7, 3.2e-7),
    'F5': (2.2e-7, 3.8e-7),
}
RANGE_BOUNDS = {'identity': (3.5e-7, 5.7e-7), 'tanh': (3.5e-7, 1.4e-6)}      # theta x 30
PREDICT_BOUNDS = {1: 3.0e-7, 64: 9.2e-7, 65: 9.2e-7}      # by m
POISON_BOUNDS = (2.1e-7, 3.5e-7)
NUTS_BOUNDS = (3.6e-6, 6.9e-6)      # kept point, mean accept probability
assert all(b <= CAP for v in list(VALUE_GRAD_BOUNDS.values()) + list(RANGE_BOUNDS.values()) + [POISON_BOUNDS, NUTS_BOUNDS] for b in v) and all(b <= CAP for b in PREDICT_BOUNDS.values())


def problem(H, F, P, K, seed, scale=1.):
    """x [P,S,F], y [P,S] in {0, 1}, theta [P K, D] ~ scale N(0, 1), all f32 (the f64 side reads the same numbers)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, S, F, generator=g)
    y = (torch.rand(P, S, generator=g) > 0.5).float()
    theta = torch.randn(P * K, ref.num_params(F, H), generator=g) * scale
    return x, y, theta


def f64_value_grad(x, y, theta, n_of, F, H, K, activation):
    out = [ref.value_and_grad(theta[c], x[c // K], y[c // K], int(n_of[c // K]), F, H, activation) for c in range(theta.shape[0])]
    return np.array([o[0] for o in out]), torch.stack([o[1] for o in out])


@functools.lru_cache(maxsize=None)
def case(label):
    """Inputs and the f64 value / gradient of a case (computed once, shared by the tests that need it)."""
    H, F, P, K, activation, n_of = CASES[label]
    x, y, theta = problem(H, F, P, K, 1000 + sum(map(ord, label)))
    return x, y, theta, f64_value_grad(x, y, theta, n_of, F, H, K, activation)


def errors(value, grad, want):
    """(max over chains of |value - f64| / |f64|, of |grad - f64| / |f64 grad|)."""
    U64, g64 = want
    v = value.double().cpu().numpy()
    g = grad.double().cpu()[:, :g64.shape[1]]
    return float(np.max(np.abs(v - U64) / np.abs(U64))), float(((g - g64).norm(dim=1) / g64.norm(dim=1)).max())


def run(x, y, theta, H, K, n_of, activation, **kw):
    n = None if n_of is None else torch.tensor(n_of, dtype=torch.int32, device=DEV)
    return hipops.bnn_logp_grad(x.to(DEV), y.to(DEV), theta.to(DEV), H, K=K, n_of=n, activation=activation, **kw)


@pytest.mark.parametrize('label', list(CASES))
def test_value_and_gradient_against_f64(label):
    H, F, P, K, activation, n_of = CASES[label]
    x, y, theta, want = case(label)
    value, grad = run(x, y, theta, H, K, n_of, activation)
    assert bool(torch.isfinite(value).all()) and bool(torch.isfinite(grad).all())
    e_value, e_grad = errors(value, grad, want)
    print(f'{label}: H {H} F {F} P {P} K {K} {activation} n_of {n_of}: value {e_value:.3e}, gradient {e_grad:.3e}')
    bounds.within(f'{label} value', e_value, VALUE_GRAD_BOUNDS[label][0])
    bounds.within(f'{label} gradient', e_grad, VALUE_GRAD_BOUNDS[label][1])
    only_value, none = run(x, y, theta, H, K, n_of, activation, want_grad=False)      # a NULL grad: the same value
    assert none is None and torch.equal(only_value, value)
    if all(n == S for n in n_of):      # a NULL n_of means all S rows
        value_all, grad_all = run(x, y, theta, H, K, None, activation)
        assert torch.equal(value_all, value) and torch.equal(grad_all, grad)
    if all(n == 0 for n in n_of[:1]) and label == 'H5':      # n = 0 is the prior: |theta|^2 / 2 + (D / 2) log 2 pi, gradient theta
        D = ref.num_params(F, H)
        prior = 0.5 * (theta[:K].double() ** 2).sum(1) + 0.5 * D * math.log(2 * math.pi)
        assert float(((value[:K].double().cpu() - prior).abs() / prior).max()) < 1e-6 and torch.equal(grad[:K].cpu(), theta[:K])


def test_rows_beyond_n_and_columns_beyond_d_are_never_touched():
    H, F, P, K, activation = 5, 3, 3, 3, 'tanh'
    n_of = (0, 63, 99)
    D = ref.num_params(F, H)
    x, y, theta = problem(H, F, P, K, 77)
    want = f64_value_grad(x, y, theta, n_of, F, H, K, activation)
    xp, yp = x.clone(), y.clone()
    for p, n in enumerate(n_of):
        xp[p, n:], yp[p, n:] = float('nan'), float('nan')
    ld = D + 3
    tp = torch.full((P * K, ld), float('nan'))
    tp[:, :D] = theta
    grad = torch.full((P * K, ld), -777., device=DEV)
    value, grad = run(xp, yp, tp, H, K, n_of, activation, grad=grad)
    assert bool(torch.isfinite(value).all()) and bool(torch.isfinite(grad[:, :D]).all()) and bool((grad[:, D:] == -777.).all())
    e_value, e_grad = errors(value, grad, want)
    print(f'poisoned tails: value {e_value:.3e}, gradient {e_grad:.3e}')
    bounds.within('poisoned value', e_value, POISON_BOUNDS[0])
    bounds.within('poisoned gradient', e_grad, POISON_BOUNDS[1])
    clean_value, clean_grad = run(x, y, theta, H, K, n_of, activation)      # the same bits as from clean, unpadded inputs
    assert torch.equal(clean_value, value) and torch.equal(clean_grad, grad[:, :D])
    prob = hipops.bnn_predict(x[:, :7].contiguous().to(DEV), tp.to(DEV), H, K=K, activation=activation)
    assert bool(torch.isfinite(prob).all()) and torch.equal(prob, hipops.bnn_predict(x[:, :7].contiguous().to(DEV), theta.to(DEV), H, K=K, activation=activation))


@pytest.mark.parametrize('H,F,activation', [(5, 3, 'tanh'), (9, 16, 'identity'), (33, 8, 'tanh'), (64, 1, 'identity')])
def test_a_chain_is_a_bitwise_function_of_its_own_inputs(H, F, activation):
    """Chain c of a P = 3, K = 9 call against the same chain alone (P = 1, K = 1): value, gradient and predictive, bit for bit; one H per Hp."""
    P, K = 3, 9
    n_of = (65, 7, 100)
    x, y, theta = problem(H, F, P, K, 300 + H)
    value, grad = run(x, y, theta, H, K, n_of, activation)
    xt = x[:, :66].contiguous()
    prob = hipops.bnn_predict(xt.to(DEV), theta.to(DEV), H, K=K, activation=activation)
    for c in (0, 4, 8, 13, 22, 26):
        p = c // K
        v1, g1 = run(x[p:p + 1], y[p:p + 1], theta[c:c + 1], H, 1, n_of[p:p + 1], activation)
        assert torch.equal(v1[0], value[c]) and torch.equal(g1[0], grad[c]), c
        assert torch.equal(hipops.bnn_predict(xt[p:p + 1].to(DEV), theta[c:c + 1].to(DEV), H, K=1, activation=activation)[0], prob[c]), c
    # ... and of K: the chains of problem 1 as a P = 1, K = 9 call
    v9, g9 = run(x[1:2], y[1:2], theta[K:2 * K], H, K, n_of[1:2], activation)
    assert torch.equal(v9, value[K:2 * K]) and torch.equal(g9, grad[K:2 * K])


@pytest.mark.parametrize('activation', ['identity', 'tanh'])
def test_large_logits_stay_finite_and_a_nan_chain_stays_alone(activation):
    H, F, P, K = 5, 3, 3, 3
    n_of = (100, 63, 2)
    x, y, theta = problem(H, F, P, K, 55, scale=30.)
    want = f64_value_grad(x, y, theta, n_of, F, H, K, activation)
    o = torch.stack([ref.logits(theta[c].double(), x[c // K].double(), F, H, activation) for c in range(P * K)])
    assert float(o.abs().max()) > 80.      # the logits reach +-80 and beyond
    value, grad = run(x, y, theta, H, K, n_of, activation)
    assert bool(torch.isfinite(value).all()) and bool(torch.isfinite(grad).all())
    e_value, e_grad = errors(value, grad, want)
    print(f'theta x 30 ({activation}): largest |logit| {float(o.abs().max()):.0f}, value {e_value:.3e}, gradient {e_grad:.3e}')
    bounds.within(f'range {activation} value', e_value, RANGE_BOUNDS[activation][0])
    bounds.within(f'range {activation} gradient', e_grad, RANGE_BOUNDS[activation][1])
    bad = theta.clone()
    bad[4, 7] = float('nan')
    value_bad, grad_bad = run(x, y, bad, H, K, n_of, activation)
    assert not bool(torch.isfinite(value_bad[4]))
    keep = [c for c in range(P * K) if c != 4]
    assert torch.equal(value_bad[keep], value[keep]) and torch.equal(grad_bad[keep], grad[keep])
    bad[4, 7] = float('inf')
    assert not bool(torch.isfinite(run(x, y, bad, H, K, n_of, activation)[0][4]))


@pytest.mark.parametrize('m', [1, 64, 65])
def test_predict_against_f64(m):
    e = 0.
    for H, F, activation in ((5, 3, 'identity'), (9, 16, 'tanh'), (33, 1, 'identity'), (64, 8, 'tanh')):
        P, K = 3, 3
        x, _, theta = problem(H, F, P, K, 500 + H)
        xt = x[:, :m].contiguous()
        prob = hipops.bnn_predict(xt.to(DEV), theta.to(DEV), H, K=K, activation=activation)
        assert prob.shape == (P * K, m) and bool(((prob >= 0) & (prob <= 1)).all())
        want = torch.stack([ref.predict(theta[c], xt[c // K], F, H, activation) for c in range(P * K)])
        e = max(e, float((prob.double().cpu() - want).abs().max()))
    print(f'predict m {m}: |prob1 - f64| = {e:.3e}')
    bounds.within(f'predict m {m}', e, PREDICT_BOUNDS[m])


# ---- one NUTS transition on the BNN target -----------------------------------------------------------------------------------------------------------
NUTS_CASE = dict(F=3, H=5, n=10, P=5, K=13, eps=.15, depth=6, data_seed=13)
# The Philox seed of the transition.  Whether a chain's f64 decision margin is below 1e-4 is a property of its random stream; this seed was chosen with the
# f64 emulation on the host (nothing of the device enters) so that the emulation leaves at most 2 % of the 65 chains out, which the first test below asserts.
NUTS_SEED = 3


@functools.lru_cache(maxsize=None)
def nuts_inputs():
    c = NUTS_CASE
    g = torch.Generator().manual_seed(c['data_seed'])
    x = torch.randn(c['P'], c['n'], c['F'], generator=g)
    y = (torch.rand(c['P'], c['n'], generator=g) > 0.5).float()
    theta0 = torch.randn(c['P'] * c['K'], ref.num_params(c['F'], c['H']), generator=g)      # f32: both sides start from the same numbers
    return x, y, theta0


@functools.lru_cache(maxsize=None)
def nuts_emulated(seed=None):
    c = NUTS_CASE
    x, y, theta0 = nuts_inputs()
    out = []
    for ch in range(theta0.shape[0]):
        fun = ref.potential_fun(x[ch // c['K']], y[ch // c['K']], c['n'], c['F'], c['H'], 'identity')
        th = theta0[ch].double().numpy()
        U, g = fun(th)
        out.append(emu.transition(fun, th, U, g, np.ones(len(th)), c['eps'], emu.Draws(NUTS_SEED if seed is None else seed, ch), 0, c['depth']))
    return out


def test_few_chains_are_left_out_of_the_exact_comparison():
    out = sum(w['margin'] < MARGIN for w in nuts_emulated())
    print(f'{out} of {len(nuts_emulated())} chains below the margin')
    assert out <= 0.02 * len(nuts_emulated())


def test_one_transition_on_the_bnn_target_against_the_emulation():
    c = NUTS_CASE
    x, y, theta0 = nuts_inputs()
    xd, yd = x.to(DEV), y.to(DEV)
    fun = lambda theta: hipops.bnn_logp_grad(xd, yd, theta, c['H'], K=c['K'])
    dev = mcmc.batched_nuts(fun, theta0.to(DEV), 1, 0, seed=NUTS_SEED, step_size=c['eps'], max_tree_depth=c['depth'], sync_every=8)
    samples, stats = dev['samples'].double().cpu().numpy(), dev['stats'].double().cpu().numpy()
    left_out, e_point, e_acc, leapfrogs = 0, 0., 0., 0
    for ch, want in enumerate(nuts_emulated()):
        if want['margin'] < MARGIN:
            left_out += 1
            continue
        got = (int(stats[ch, 0, 2]), int(stats[ch, 0, 3]), int(stats[ch, 0, 4]))
        assert got == (want['depth'], want['leapfrogs'], want['diverging']), (ch, got, want['depth'], want['leapfrogs'], want['diverging'], want['margin'])
        e_point = max(e_point, float(np.abs(samples[ch, 0] - want['theta']).max()))
        e_acc = max(e_acc, abs(stats[ch, 0, 1] - want['accept']))
        leapfrogs = max(leapfrogs, want['leapfrogs'])
    print(f'left out {left_out} of {len(samples)} (margin < {MARGIN}), kept point {e_point:.3e}, accept {e_acc:.3e}, most leapfrogs {leapfrogs}')
    assert left_out <= 0.02 * len(samples) and leapfrogs > 1
    bounds.within('kept point', e_point, NUTS_BOUNDS[0])
    bounds.within('accept', e_acc, NUTS_BOUNDS[1])


# ---- the sampler on the BNN ----------------------------------------------------------------------------------------------------------------------------
SMALL = dict(num_features=3, embed=5)


def test_with_no_data_the_chains_recover_the_prior():
    """n_of = 0, D = 32, 64 chains, 150 warmup + 100 draws.  The chains are independent, so the 64 chain means of a coordinate (and of its square) are iid and
    their t statistic against 0 (1) has 63 degrees of freedom: P(|t| > 4.5) = 3e-5 each, below 1 % for the 64 statistics together; the seed is fixed."""
    P, K = 4, 16
    x, y, _ = problem(5, 3, P, 1, 9)
    post = study.sample_bnn_posterior(x.to(DEV), y.to(DEV), SMALL, n_of=[0] * P, num_samples=100, warmup_steps=150, num_chains=K, seed=5)
    assert post.samples.shape == (P, K, 100, 32) and post.stats.shape == (P, K, 250, 8)
    s = post.samples.double().cpu().reshape(P * K, 100, 32)
    worst = 0.
    for name, per_chain, want in (('mean', s.mean(1), 0.), ('second moment', (s * s).mean(1), 1.)):
        t = (per_chain.mean(0) - want) / (per_chain.std(0) / math.sqrt(P * K))
        print(f'{name}: max |t| = {float(t.abs().max()):.2f}')
        worst = max(worst, float(t.abs().max()))
    assert worst < 4.5
    assert float(post.stats[:, :, 150:, 4].sum()) == 0      # no divergence on a Gaussian at an adapted step


def test_a_posterior_that_is_not_the_prior_against_importance_sampling():
    """F 1, H 2, n 3, one problem, 64 chains: the predictive class-1 probability at 5 test points against self-normalised importance sampling from the prior
    (4e5 f64 draws on the host, standard error by the delta method); the NUTS side's standard error is that of the 64 independent chain means."""
    F, H, n, K = 1, 2, 3, 64
    spec = dict(num_features=F, embed=H)
    x = torch.tensor([[[-1.5], [0.3], [1.1]]])
    y = torch.tensor([[1., 0., 1.]])
    xt = torch.tensor([[[-2.], [-0.7], [0.], [0.8], [2.2]]])
    rng = np.random.default_rng(3)
    th = rng.standard_normal((400000, ref.num_params(F, H)))
    W1, b1, W2, b2 = th[:, 0:2], th[:, 2:4], th[:, 4:8].reshape(-1, 2, 2), th[:, 8:10]

    def p1(xs):      # [draws, len(xs)]
        h = W1[:, None, :] * xs[None, :, None] + b1[:, None, :]
        o = np.einsum('dnh,dch->dnc', h, W2) + b2[:, None, :]
        return 1. / (1. + np.exp(o[..., 0] - o[..., 1]))
    p_train = p1(x[0, :, 0].double().numpy())
    w = np.prod(np.where(y[0].numpy()[None, :] > 0.5, p_train, 1. - p_train), axis=1)
    p_test = p1(xt[0, :, 0].double().numpy())
    want = (w[:, None] * p_test).sum(0) / w.sum()
    se_is = np.sqrt(((w[:, None] * (p_test - want)) ** 2).sum(0)) / w.sum()
    prior_mean = p_test.mean(0)
    assert np.abs(want - prior_mean).max() > 0.05      # the data moved the predictive
    post = study.sample_bnn_posterior(x.to(DEV), y.to(DEV), spec, num_samples=200, warmup_steps=200, num_chains=K, seed=2)
    prob = post.predictive(xt.to(DEV))
    assert prob.shape == (1, K * 200, 5)
    means = prob[0].double().cpu().reshape(K, 200, 5).mean(1).numpy()
    got, se = means.mean(0), means.std(0, ddof=1) / math.sqrt(K)
    z = (got - want) / np.sqrt(se ** 2 + se_is ** 2)
    print(f'importance sampling {want} +- {se_is}\nNUTS {got} +- {se}\nz {z}')
    assert np.abs(z).max() < 4.5
    # the predictive of the draws is the f64 predictive of those weights
    flat = post.samples.double().cpu().reshape(-1, ref.num_params(F, H))
    for i in (0, 199, 200, K * 200 - 1):
        assert float((ref.predict(flat[i], xt[0], F, H) - prob[0, i].double().cpu()).abs().max()) < 1e-5


def test_eval_mcmc_on_toy_data():
    spec = study.get_default_model_spec('small')
    model = study.BayesianModel(spec, device=DEV)
    X, y = study.generate_toy_data(model, 30, device=DEV)
    assert X.shape == (100, 30, 3) and y.shape == (100, 30)
    X, y = X[:4], y[:4]
    nll, acc = study.eval_mcmc(X, y, DEV, spec, 10, warmup_steps=20, num_pred_samples=20)
    assert isinstance(nll, np.ndarray) and isinstance(acc, np.ndarray) and nll.shape == (4,) and acc.shape == (4,)
    assert np.isfinite(nll).all() and np.isfinite(acc).all() and (acc >= 0).all() and (acc <= 1).all() and (nll > 0).all()
    nll2, acc2 = study.eval_mcmc(X, y, DEV, spec, 10, warmup_steps=20, num_pred_samples=20)
    assert np.array_equal(nll, nll2) and np.array_equal(acc, acc2)
    # the reference's estimator (sampled observations, mean hard prediction), and a model sampler in place of the spec
    nll3, acc3 = study.eval_mcmc(X, y, DEV, lambda: study.BayesianModel(spec, device=DEV), 10, warmup_steps=20, num_pred_samples=20, sample_obs=True)
    assert nll3.shape == (4,) and acc3.shape == (4,) and np.isfinite(nll3).all() and (acc3 >= 0).all() and (acc3 <= 1).all()
    with pytest.raises(ValueError, match='128'):
        study.eval_mcmc(torch.zeros(1, 12, 8, device=DEV), torch.zeros(1, 12, device=DEV), DEV, study.get_default_model_spec('big'), 10, 4, 4)
