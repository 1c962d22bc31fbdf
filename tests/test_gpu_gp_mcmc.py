"""The batched NUTS on the device (csrc/gp_mcmc.hip, mcmc.batched_nuts, priors.fast_gp_mix.sample_hyperparameter_posterior / evaluate_) against the f64
emulation of its state machine (tests/nuts_f64.py, itself verified on the host in tests/test_host_gp_mcmc.py) and against the f64 GP reference
(tests/gp_fit_f64.py).

The Gaussian target is value = sum theta^2 / (2 sigma^2), grad = theta / sigma^2, computed by torch on the device.  A transition's discrete outcome (depth,
leapfrogs, diverging) must EQUAL the emulation's, except for chains whose f64 decision margin is below 1e-4 (an f32 trajectory may legitimately take the
other branch there): those are left out, and at most 2 % of a case may be.

Bounds on continuous outputs: <= 2 x the value measured on the MI355X (profiles/r12_gp_mcmc_bounds_measured.json), and never above 1e-3."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds      # noqa: E402
import gp_fit_f64 as ref      # noqa: E402
import nuts_f64 as emu      # noqa: E402

from transformerscandobayesianinference_amd import hipops, mcmc      # noqa: E402
from transformerscandobayesianinference_amd.priors import fast_gp_mix      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SIGMA5 = (.3, .6, 1., 1.7, 3.)
MARGIN = 1e-4
CAP = 1e-3


def sigma_of(D):
    return torch.tensor(SIGMA5, dtype=torch.float64) if D == 5 else torch.linspace(.5, 2., D, dtype=torch.float64) if D > 1 else torch.tensor([.8], dtype=torch.float64)


def gaussian_on_device(sigma, D=None):
    inv = (1. / sigma ** 2).float().to(DEV)
    D = len(sigma) if D is None else D

    def fun(theta):
        t = theta[:, :D]
        grad = torch.full_like(theta, float('nan'))      # columns >= D are never read
        grad[:, :D] = t * inv
        return 0.5 * (t * t * inv).sum(1), grad
    return fun


def gaussian_f64(sigma, scale=1., shift=None):
    s2 = sigma.numpy() ** 2
    sh = np.zeros(len(s2)) if shift is None else np.asarray(shift, dtype=np.float64)
    return lambda th: (scale * 0.5 * float(np.sum(th * th / s2)) - float(np.sum(sh * th)), scale * th / s2 - sh)


def starts(C, sigma, seed):
    """Start points ~ N(0, sigma^2) whose f64 values are exact in f32, so the device and the emulation start from the same numbers."""
    return (torch.randn(C, len(sigma), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * sigma).float().double()


# measured on the MI355X (profiles/r12_gp_mcmc_bounds_measured.json): (kept point in units of sigma, mean accept probability), each <= 2 x measured
ONE_TRANSITION = {      # label: (D, C, eps, max_tree_depth, non-unit inverse mass, (bound point, bound accept))
    'D5': (5, 1029, .2, 6, False, (2.6e-06, 5.1e-06)),
    'D1': (1, 65, .2, 6, False, (9.4e-07, 1.2e-06)),
    'D64': (64, 65, .2, 6, False, (2.2e-06, 1.3e-05)),
    'D65': (65, 65, .2, 6, False, (3.9e-06, 9.3e-06)),
    'D128': (128, 65, .2, 6, False, (2.6e-06, 1.4e-05)),
    'depth1': (5, 65, .2, 1, False, (7.5e-07, 8.4e-07)),
    'depth10': (5, 9, .004, 10, False, (4.1e-06, 6.2e-06)),
    'mass': (5, 65, .3, 6, True, (1.6e-06, 2.0e-06)),
    'strided': (5, 65, .2, 6, False, (1.0e-06, 2.3e-06)),      # ld = D + 3, scale and shift set
}
assert all(b <= CAP for v in ONE_TRANSITION.values() for b in v[5])
SEED = 11
STRIDED_SHIFT = (.5, -.25, 0., 1., -.125)


def one_transition_inputs(label):
    D, C, eps, depth, mass, _ = ONE_TRANSITION[label]
    sigma = sigma_of(D)
    theta0 = starts(C, sigma, 100 + D + (50 if label == 'strided' else 0))
    inv_mass = None
    if mass:      # roughly sigma^2, different per chain
        inv_mass = (sigma ** 2 * (.5 + torch.rand(C, D, generator=torch.Generator().manual_seed(3), dtype=torch.float64))).float()
    scale = (1. + torch.arange(C, dtype=torch.float64) / C).float() if label == 'strided' else None
    # The depth-10 chains take their Philox streams from 28 on.  A chain of 1023 leaves compares 1023 uniforms with probabilities near 1 / (leaf + 1), which
    # hardly depend on the start point, so whether its f64 margin is below 1e-4 is a property of its stream; these nine streams were chosen with the f64
    # emulation on the host so that none is (the same kind of conditioning as `starts` making the f32 start points exact).
    ids = torch.arange(C) * 3 + (28 if label == 'depth10' else 1)
    return sigma, theta0, inv_mass, ids, scale


@functools.lru_cache(maxsize=None)
def emulated(label):
    """The f64 transition of every chain of a case (computed once, shared by the tests that need it)."""
    D, C, eps, depth, _, _ = ONE_TRANSITION[label]
    sigma, theta0, inv_mass, ids, scale = one_transition_inputs(label)
    out = []
    for c in range(C):
        fun = gaussian_f64(sigma) if scale is None else gaussian_f64(sigma, float(scale[c]), STRIDED_SHIFT)
        th = theta0[c].numpy()
        U, g = fun(th)
        m = np.ones(D) if inv_mass is None else inv_mass[c].double().numpy()
        out.append(emu.transition(fun, th, U, g, m, eps, emu.Draws(SEED, int(ids[c])), 0, depth))
    return out


def test_few_chains_are_left_out_of_the_exact_comparison():
    """In every case at most 2 % of the chains have an f64 decision margin below 1e-4 and are left out of the exact comparison."""
    for label, (_, C, *_rest) in ONE_TRANSITION.items():
        out = sum(w['margin'] < MARGIN for w in emulated(label))
        print(f'{label}: {out} of {C} chains below the margin')
        assert out <= 0.02 * C, (label, out)


def compare_one_transition(label, dev):
    """dev: dict(samples [C,1,D], stats [C,1,8]) of a W = 0, N = 1 run of the case."""
    D, C, eps, depth, _, (bound_point, bound_accept) = ONE_TRANSITION[label]
    sigma = sigma_of(D).numpy()
    samples, stats = dev['samples'].double().cpu().numpy(), dev['stats'].double().cpu().numpy()
    left_out, e_point, e_acc, deepest = 0, 0., 0., 0
    for c, want in enumerate(emulated(label)):
        if want['margin'] < MARGIN:
            left_out += 1
            continue
        got = (int(stats[c, 0, 2]), int(stats[c, 0, 3]), int(stats[c, 0, 4]))
        assert got == (want['depth'], want['leapfrogs'], want['diverging']), (label, c, got, want['depth'], want['leapfrogs'], want['diverging'], want['margin'])
        assert stats[c, 0, 0] == np.float32(eps) and stats[c, 0, 6] == 0 and stats[c, 0, 7] == 0
        e_point = max(e_point, float(np.abs((samples[c, 0] - want['theta']) / sigma).max()))
        e_acc = max(e_acc, abs(stats[c, 0, 1] - want['accept']))
        deepest = max(deepest, want['leapfrogs'])
    print(f'{label}: left out {left_out} of {C} (margin < {MARGIN}), kept point {e_point:.3e} sigma, accept {e_acc:.3e}, most leapfrogs {deepest}')
    assert left_out <= 0.02 * C, (label, left_out)
    bounds.within(f'{label} kept point / sigma', e_point, bound_point)
    bounds.within(f'{label} accept', e_acc, bound_accept)
    return deepest


@pytest.mark.parametrize('label', [k for k in ONE_TRANSITION if k != 'strided'])
def test_one_transition_against_the_emulation(label):
    D, C, eps, depth, mass, _ = ONE_TRANSITION[label]
    sigma, theta0, inv_mass, ids, _ = one_transition_inputs(label)
    dev = mcmc.batched_nuts(gaussian_on_device(sigma), theta0.float().to(DEV), 1, 0, seed=SEED, chain_ids=ids, step_size=eps, max_tree_depth=depth,
                            inv_mass=None if inv_mass is None else inv_mass.to(DEV), sync_every=8)
    deepest = compare_one_transition(label, dev)
    if mass:
        assert torch.equal(dev['inv_mass'].cpu(), inv_mass)      # nothing adapts without warmup
    if label == 'depth10':
        assert deepest == 1023      # a compared chain used the last checkpoint row and the last leaf slot
    if label == 'depth1':
        assert deepest == 1


def test_row_stride_scale_and_shift_leave_the_tail_columns_alone():
    """ld = D + 3 with `scale` and `shift` set, driven through the raw wrappers: the potential is scale value - shift . theta, and neither the poisoned tail of
    `trial` nor that of `grad` is ever read or written."""
    D, C, eps, depth, _, _ = ONE_TRANSITION['strided']
    ld = D + 3
    sigma, theta0, _, ids, scale = one_transition_inputs('strided')
    shift = torch.tensor(STRIDED_SHIFT)
    padded = torch.full((C, ld), 12345., dtype=torch.float32)
    padded[:, :D] = theta0.float()
    padded = padded.to(DEV)
    fun = gaussian_on_device(sigma, D)
    ws = hipops.nuts_workspace(C, D, depth, DEV)
    trial = torch.full((C, ld), -777., dtype=torch.float32, device=DEV)
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    samples = torch.zeros(C, 1, D, device=DEV)
    stats = torch.zeros(C, 1, 8, device=DEV)
    hipops.nuts_init(ws, padded, D, depth, 0, 1, SEED, trial, done, step_size=eps, chain_ids=ids.to(DEV))
    assert torch.equal(trial[:, :D], padded[:, :D]) and bool((trial[:, D:] == -777.).all())
    for _ in range(2 ** depth + 1):
        value, grad = fun(trial)
        hipops.nuts_advance(ws, D, depth, value, grad, trial, samples, stats, done, scale=scale.to(DEV), shift=shift.to(DEV))
    assert bool((trial[:, D:] == -777.).all()) and bool(torch.isnan(grad[:, D:]).all())
    assert int(done.item()) == C
    assert torch.equal(trial[:, :D], samples[:, 0])      # a finished chain rests at its last sample
    compare_one_transition('strided', dict(samples=samples, stats=stats))


def test_bad_arguments_are_refused_before_anything_is_launched():
    from transformerscandobayesianinference_amd import _hip
    theta0 = torch.zeros(4, 5, device=DEV)
    trial = torch.zeros(4, 5, device=DEV)
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(_hip.HipExtensionError):
        hipops.nuts_workspace(4, 129, 10, DEV)
    with pytest.raises(_hip.HipExtensionError):
        hipops.nuts_workspace(4, 5, 11, DEV)
    ws = hipops.nuts_workspace(4, 5, 10, DEV)
    for kw in (dict(D=6), dict(depth=11), dict(depth=0), dict(N=0), dict(W=-1), dict(step_size=0.), dict(window_ends=(5, 5), W=10), dict(window_ends=(11,), W=10),
               dict(window_ends=(10,), W=10)):      # (a window ending at W would restart dual averaging with nothing left to average)
        args = dict(D=5, depth=10, W=0, N=1, step_size=.1, window_ends=())
        args.update(kw)
        with pytest.raises(_hip.HipExtensionError):
            hipops.nuts_init(ws, theta0, args['D'], args['depth'], args['W'], args['N'], 0, trial, done, step_size=args['step_size'], window_ends=args['window_ends'])
    with pytest.raises(_hip.HipExtensionError):      # a workspace sized for fewer chains
        hipops.nuts_init(hipops.nuts_workspace(3, 5, 10, DEV), theta0, 5, 10, 0, 1, 0, trial, done)
    # buffers sized for another N than init was given: the kernel touches nothing (no output, no trial point, no counter)
    hipops.nuts_init(ws, theta0 + 1., 5, 10, 0, 2, 0, trial, done)
    before = trial.clone()
    samples, stats = torch.full((4, 3, 5), -1., device=DEV), torch.full((4, 3, 8), -1., device=DEV)
    hipops.nuts_advance(ws, 5, 10, torch.zeros(4, device=DEV), torch.zeros(4, 5, device=DEV), trial, samples, stats, done)
    assert torch.equal(trial, before) and int(done.item()) == 0 and bool((samples == -1.).all()) and bool((stats == -1.).all())
    samples, stats = torch.full((4, 2, 5), -1., device=DEV), torch.full((4, 2, 8), -1., device=DEV)      # the right ones: the first pass starts transition 0
    hipops.nuts_advance(ws, 5, 10, torch.zeros(4, device=DEV), torch.zeros(4, 5, device=DEV), trial, samples, stats, done)
    assert not torch.equal(trial, before)


def test_a_divergent_first_leaf_keeps_the_point():
    sigma = sigma_of(5)
    C = 64
    theta0 = sigma.float().repeat(C, 1)      # one sigma out in every coordinate: eps = 50 min sigma throws the stiffest one 1249 sigma away, dE ~ 8e5
    res = mcmc.batched_nuts(gaussian_on_device(sigma), theta0.to(DEV), 1, 0, seed=2, step_size=50 * .3)
    assert torch.equal(res['samples'][:, 0].cpu(), theta0)
    stats = res['stats'][:, 0].cpu()
    assert bool((stats[:, 4] == 1).all()) and bool((stats[:, 3] == 1).all()) and bool((stats[:, 2] == 1).all()) and bool((stats[:, 1] == 0).all())
    assert res['evaluations'] <= 17      # the start point, one leaf, and the passes until the host next looks


@pytest.mark.parametrize('how', ['value', 'info'])
def test_non_finite_values_and_info_act_as_a_wall(how):
    """value = inf (or info = 1 with a finite value) wherever theta_0 > 1: such a leaf is divergent, so no stored point is ever behind the wall."""
    sigma = torch.ones(3, dtype=torch.float64)
    base = gaussian_on_device(sigma)

    def fun(theta):
        value, grad = base(theta)
        behind = theta[:, 0] > 1.
        if how == 'value':
            return torch.where(behind, torch.full_like(value, float('inf')), value), grad
        return value, grad, behind.to(torch.int32)
    res = mcmc.batched_nuts(fun, torch.zeros(64, 3, device=DEV), 40, 30, seed=4, keep_warmup=True)
    pts = torch.cat([res['warm'], res['samples']], 1)
    assert bool(torch.isfinite(pts).all()) and float(pts[..., 0].max()) <= 1.
    assert float(res['samples'][..., 0].max()) > .5 and float(res['stats'][..., 4].sum()) > 0      # the wall was reached, and hitting it was recorded
    assert bool(torch.isfinite(res['stats']).all())


ADAPT_BOUNDS = dict(step=9.6e-06, mass=5.1e-07)      # relative


def test_adaptation_follows_the_f64_recurrences():
    """C = 64, W = 150 (one slow window, 75 .. 100), N = 50: from the device's OWN recorded warmup points and accept statistics the f64 recurrences (dual
    averaging, Welford window, regularised variance, restart) must give every step size the device recorded and its final inverse mass."""
    sigma = sigma_of(5)
    C, W, N = 64, 150, 50
    res = mcmc.batched_nuts(gaussian_on_device(sigma), torch.zeros(C, 5, device=DEV), N, W, seed=8, keep_warmup=True)
    stats, warm, inv_mass = res['stats'].double().cpu().numpy(), res['warm'].double().cpu().numpy(), res['inv_mass'].double().cpu().numpy()
    windows = mcmc.adaptation_windows(W)
    assert windows == [(75, 100)]
    e_step = e_mass = 0.
    for c in range(C):
        ad = emu.Adaptation(.1, .8, W, windows, np.ones(5))
        for t in range(W + N):
            e_step = max(e_step, abs(stats[c, t, 0] - ad.eps) / ad.eps)
            if t < W:
                ad.update(t, stats[c, t, 1], warm[c, t])
        e_mass = max(e_mass, float(np.abs(inv_mass[c] / ad.m - 1.).max()))
    print(f'adaptation: step size {e_step:.3e}, inverse mass {e_mass:.3e} (relative)')
    bounds.within('step size', e_step, ADAPT_BOUNDS['step'])
    bounds.within('inverse mass', e_mass, ADAPT_BOUNDS['mass'])
    assert np.all(stats[:, W:, 0] == stats[:, W:W + 1, 0]) and np.array_equal(res['step_size'].double().cpu().numpy(), stats[:, -1, 0])      # fixed after warmup
    assert np.abs(np.log(inv_mass / sigma.numpy() ** 2)).max() < 2.5      # 25 draws per variance: the right order of magnitude, per coordinate
    assert 0.6 < stats[:, W:, 1].mean() < 0.98


POTENTIAL_BOUND = 3.9e-07      # |U recorded - U64(sample)| / max(1, |U64|)


def test_moments_of_a_gaussian_and_the_recorded_potential():
    """C = 512 adapted chains: the chain means are independent, so the z of their average is standard normal whatever the autocorrelation; 4.5 is a 7e-6 tail."""
    sigma = sigma_of(5)
    C, W, N = 512, 150, 100
    res = mcmc.batched_nuts(gaussian_on_device(sigma), torch.zeros(C, 5, device=DEV), N, W, seed=21)
    s = res['samples'].double().cpu()
    for name, per_chain, want in (('mean', s.mean(1) / sigma, 0.), ('second moment', (s * s / sigma ** 2).mean(1), 1.)):
        z = (per_chain.mean(0) - want) / (per_chain.std(0) / math.sqrt(C))
        print(f'{name}: z = {z.tolist()}')
        assert float(z.abs().max()) <= 4.5, (name, z)
    U64 = 0.5 * (s * s / sigma ** 2).sum(-1)
    e = ((res['stats'][:, W:, 5].double().cpu() - U64).abs() / U64.clamp_min(1.)).max()
    print(f'recorded potential: {float(e):.3e}')
    bounds.within('recorded potential', e, POTENTIAL_BOUND)
    assert float(res['stats'][:, W:, 4].sum()) == 0      # no divergence on a Gaussian at an adapted step


def test_a_chain_depends_on_its_id_and_its_own_inputs_only():
    sigma = sigma_of(5)
    theta0 = starts(9, sigma, 1).float().to(DEV)
    fun = gaussian_on_device(sigma)
    full = mcmc.batched_nuts(fun, theta0, 10, 20, seed=6, keep_warmup=True)
    for c in (3, 7):
        one = mcmc.batched_nuts(fun, theta0[c:c + 1], 10, 20, seed=6, chain_ids=torch.tensor([c]), keep_warmup=True, sync_every=5)
        for key in ('samples', 'stats', 'warm', 'inv_mass', 'step_size'):
            assert torch.equal(one[key][0], full[key][c]), (c, key)
    other = mcmc.batched_nuts(fun, theta0[3:4], 10, 20, seed=6, chain_ids=torch.tensor([4]))
    assert not torch.equal(other['samples'][0], full['samples'][3])


@functools.lru_cache(maxsize=None)
def gp_batch():
    """One problem of 12 points (the host test's), and a batch with S = 68 and n_of = (12, 64, 65): the panel edge of pfn_gp_mll_grad."""
    prior = fast_gp_mix.hyperprior_vector(emu.GP_HP, dtype=torch.float64)
    x, y = ref.make_problems(3, 68, 2, 1, seed=31, prior=prior)
    return x, y, prior, [12, 64, 65]


def test_gp_chains_are_independent_of_the_batch_too():
    x, y, _, n_of = gp_batch()
    kw = dict(hyperparameters=emu.GP_HP, num_samples=6, warmup_steps=10, seed=3)
    full = fast_gp_mix.sample_hyperparameter_posterior(x.to(DEV), y.to(DEV), n_of=torch.tensor(n_of), num_chains=3, **kw)
    assert full.theta.shape == (3, 18, 5) and full.stats.shape == (3, 3, 16, 8) and full.divergences.shape == (3,)
    assert full.lengthscale.shape == (3, 18, 2) and full.outputscale.shape == (3, 18) and full.noise.shape == (3, 18) and bool((full.theta[..., 4] == 0).all())
    one = fast_gp_mix.sample_hyperparameter_posterior(x[1:2].to(DEV), y[1:2].to(DEV), n_of=torch.tensor(n_of[1:2]), num_chains=3, chain_id_base=3, **kw)
    assert torch.equal(one.theta[0], full.theta[1]) and torch.equal(one.stats[0], full.stats[1])
    # chains 3 and 7 of a nine-chain run of one problem against one-chain runs with those ids
    nine = fast_gp_mix.sample_hyperparameter_posterior(x[2:3].to(DEV), y[2:3].to(DEV), n_of=torch.tensor(n_of[2:3]), num_chains=9, **kw)
    for c in (3, 7):
        alone = fast_gp_mix.sample_hyperparameter_posterior(x[2:3].to(DEV), y[2:3].to(DEV), n_of=torch.tensor(n_of[2:3]), num_chains=1, chain_id_base=c, **kw)
        assert torch.equal(alone.theta[0], nine.theta[0, 6 * c:6 * c + 6]) and torch.equal(alone.stats[0, 0], nine.stats[0, c]), c


GP_POTENTIAL_BOUND = 5.0e-06


def test_gp_potential_at_the_panel_edge_and_masked_rows():
    x, y, prior, n_of = gp_batch()
    outs = []
    for fill in (0., 1e3, -1e3):
        xf, yf = x.clone(), y.clone()
        for p, n in enumerate(n_of):
            xf[p, n:] = fill
            yf[p, n:] = -fill
        model = fast_gp_mix.sample_hyperparameter_posterior(xf.to(DEV), yf.to(DEV), emu.GP_HP, n_of=torch.tensor(n_of), num_samples=10, warmup_steps=20, seed=9)
        outs.append((model.theta.cpu(), model.stats.cpu()))
    for other in outs[1:]:
        assert torch.equal(other[0], outs[0][0]) and torch.equal(other[1], outs[0][1])
    theta, stats = outs[0][0].double(), outs[0][1].double()
    e = 0.
    for p, n in enumerate(n_of):
        for s in range(10):
            U64 = n * float(ref.objective(theta[p, s], x[p], y[p], n, prior, 1)) - float(theta[p, s, :4].sum())
            e = max(e, abs(float(stats[p, 0, 20 + s, 5]) - U64) / max(1., abs(U64)))
    print(f'gp potential at the samples: {e:.3e}')
    bounds.within('gp potential', e, GP_POTENTIAL_BOUND)


def test_gp_chains_reproduce_the_quadrature():
    """The host test's problem (F = 1, n = 12, Matern 5/2), one problem x 64 chains x (150 + 100): |z| <= 4.5 per coordinate against the same f64 quadrature."""
    want, face_mass = emu.gp_quadrature()
    assert face_mass < 1e-4
    x, y, _, _ = emu.gp_problem()
    model = fast_gp_mix.sample_hyperparameter_posterior(x[None].to(DEV), y[None].to(DEV), emu.GP_HP, num_samples=100, warmup_steps=150, num_chains=64, seed=1)
    means = model.theta[0, :, :3].double().cpu().reshape(64, 100, 3).mean(1).numpy()
    z = (means.mean(0) - want) / (means.std(0, ddof=1) / 8.)
    print(f'gp: z = {z}, divergences {int(model.divergences[0])}, evaluations {model.evaluations}')
    assert np.abs(z).max() <= 4.5, z


DENSITY_BOUND = {      # (use_likelihood, full_range given, min_seq_len): |loss - f64 loss of the same samples|, nats
    (False, False, 0): 1.4e-06,
    (False, False, 3): 9.4e-07,
    (False, True, 0): 8.9e-07,
    (False, True, 3): 7.5e-07,
    (True, False, 0): 5.7e-07,
    (True, False, 3): 5.4e-07,
    (True, True, 0): 2.3e-07,
    (True, True, 3): 3.3e-07,
}
assert all(b <= CAP for b in DENSITY_BOUND.values()) and max(ADAPT_BOUNDS.values()) <= CAP and POTENTIAL_BOUND <= CAP and GP_POTENTIAL_BOUND <= CAP


@pytest.mark.parametrize('min_seq_len', [0, 3])
@pytest.mark.parametrize('full_range', [None, (-3., 3.)])
@pytest.mark.parametrize('use_likelihood', [False, True])
def test_evaluate_is_sample_then_mixture_density(use_likelihood, full_range, min_seq_len):
    T, B, F, NS, NW = 6, 2, 2, 8, 10
    prior = fast_gp_mix.hyperprior_vector(emu.GP_HP, dtype=torch.float64)
    xs, ys = ref.make_problems(B, T, F, 1, seed=21, prior=prior)
    ys = ys.clamp(-2.5, 2.5)
    x, y = xs.transpose(0, 1).contiguous(), ys.transpose(0, 1).contiguous()      # [T,B,F], [T,B]
    per_t, seconds, all_losses = fast_gp_mix.evaluate_(x, y, y, emu.GP_HP, device=DEV, num_samples=NS, warmup_steps=NW, full_range=full_range, min_seq_len=min_seq_len,
                                                       use_likelihood=use_likelihood)
    ts = list(range(max(min_seq_len, 1), T))
    assert isinstance(per_t, torch.Tensor) and per_t.shape == (len(ts) + (1 if min_seq_len == 0 else 0),) and seconds > 0
    assert isinstance(all_losses, list) and len(all_losses) == len(ts) and all(isinstance(l, list) and len(l) == B for l in all_losses)
    losses = torch.tensor(all_losses)
    if min_seq_len == 0:
        assert float(per_t[0]) == 0.
    torch.testing.assert_close(per_t[-len(ts):], losses.mean(1), rtol=1e-6, atol=1e-6)
    # the composition: every (t, b) problem in one batch of the public pieces, rows padded to the 64-row bucket and masked through n_of -- the batch `evaluate_` forms
    tt = torch.tensor([t for t in ts for _ in range(B)])
    bb = torch.arange(B).repeat(len(ts))
    xp = torch.cat([xs, xs.new_zeros(B, 64 - T, F)], 1)[bb].to(DEV)
    yp = torch.cat([ys, ys.new_zeros(B, 64 - T)], 1)[bb].to(DEV)
    model = fast_gp_mix.sample_hyperparameter_posterior(xp, yp, emu.GP_HP, n_of=tt, num_samples=NS, warmup_steps=NW)
    xt, yt = xs[bb, tt].unsqueeze(1), ys[bb, tt].unsqueeze(1)
    want = -model.log_density(xt.to(DEV), yt.to(DEV), full_range, use_likelihood)[:, 0].cpu().reshape(len(ts), B)
    # the same samples, means and variances on both sides (same batch, same kernels, same torch ops on the device): equal to the last bit but for the copy
    torch.testing.assert_close(losses, want, rtol=0, atol=0)
    # the mixture density itself against f64 at the device's samples
    theta = model.theta.double().cpu()
    e = 0.
    for j in range(len(tt)):
        logp = []
        for s in range(NS):
            mean, var = ref.posterior(theta[j, s], xs[bb[j]], ys[bb[j]], int(tt[j]), prior, 1, xt[j])
            if not use_likelihood:
                var = (var - (theta[j, s, F + 1].exp() + prior[6])).clamp_min(1e-6)
            sd = var.sqrt()
            lp = -0.5 * math.log(2 * math.pi) - sd.log() - 0.5 * ((yt[j].double() - mean) / sd) ** 2
            if full_range is not None:
                cdf = lambda v: 0.5 * (1 + torch.erf((v - mean) / (sd * math.sqrt(2.))))
                lp = lp - torch.log(cdf(full_range[1]) - cdf(full_range[0]))
            logp.append(lp[0])
        w64 = -(torch.logsumexp(torch.stack(logp), 0) - math.log(NS))
        e = max(e, abs(float(want.reshape(-1)[j]) - float(w64)))
    print(f'evaluate_ use_likelihood {use_likelihood} full_range {full_range} min_seq_len {min_seq_len}: |loss - f64 loss| = {e:.3e}')
    bounds.within('mixture density', e, DENSITY_BOUND[use_likelihood, full_range is not None, min_seq_len])


def test_get_mcmc_model_has_the_reference_call_shape():
    x, y, _, _ = emu.gp_problem()
    model, likelihood = fast_gp_mix.get_mcmc_model(x, y, emu.GP_HP, DEV, 6, 8)
    assert isinstance(model, fast_gp_mix.MCMCGP) and likelihood is model
    assert model.theta.shape == (1, 6, 4) and model.stats.shape == (1, 1, 14, 8)
    mean, var = model.posterior(torch.rand(1, 3, 1))
    assert mean.shape == (1, 6, 3) and var.shape == (1, 6, 3) and bool((var > model.noise.unsqueeze(-1) * (1 - 1e-5)).all())
    with pytest.raises(AssertionError):
        fast_gp_mix.get_mcmc_model(x, y, dict(emu.GP_HP, sigmoid=True), DEV, 6, 8)
    with pytest.raises(NotImplementedError):
        fast_gp_mix.get_model(x[None], y[None], emu.GP_HP, sample=False)
