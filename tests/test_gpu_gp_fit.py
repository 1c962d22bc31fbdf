"""The GP hyper-parameter fit on the device (csrc/gp_fit.hip, priors.fast_gp_mix.fit_hyperparameters / get_fitted_model / evaluate) against the f64
reference of tests/gp_fit_f64.py.

Shapes: S = 328 with n_of = 1, 5, 63, 64, 65, 255, 256, 257, 328 crosses every blocking edge of the factorisation and the inverse (64-wide panels, the
256-wide outer block, the 128-row trailing tiles) in one call of P = 9 problems; F in {1, 5, 18}; the four covariance functions.  y is drawn in f64 from the
model itself (gp_fit_f64.make_problems).  The hyper-prior is the default except outputscale_concentration = 2 (the default .5 has no minimum in the
outputscale, see the module docstring of priors.fast_gp_mix).

Bounds: <= 2 x the value measured on the MI355X (profiles/r11_gp_fit_bounds_measured.json), and never above 1e-3."""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds      # noqa: E402
import gp_fit_f64 as ref      # noqa: E402

from transformerscandobayesianinference_amd import hipops      # noqa: E402
from transformerscandobayesianinference_amd.priors import fast_gp_mix      # noqa: E402

pytestmark = pytest.mark.gpu

S, P = 328, 9
N_OF = [1, 5, 63, 64, 65, 255, 256, 257, 328]
HP = {'outputscale_concentration': 2.}
NU_OF_KERNEL = {1: 2.5, 2: 1.5, 3: 0.5}
DEV = 'cuda'


def prior64():
    return fast_gp_mix.hyperprior_vector(HP, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def problems(kernel, F):
    x, y = ref.make_problems(P, S, F, kernel, seed=1000 + 10 * kernel + F, prior=prior64())
    return x, y


def points(F):
    t0 = fast_gp_mix.default_theta(P, F, HP, dtype=torch.float64)
    g = torch.Generator().manual_seed(77 + F)
    return [('start', t0), ('perturbed', t0 + .5 * torch.randn(P, F + 3, generator=g, dtype=torch.float64))]


@functools.lru_cache(maxsize=None)
def reference_value_grad(kernel, F):
    x, y = problems(kernel, F)
    return {name: ref.batch_value_and_grad(theta, x, y, N_OF, prior64(), kernel) for name, theta in points(F)}


def device_value_grad(x, y, theta, kernel, n_of=N_OF, **kw):
    n = torch.tensor(n_of, dtype=torch.int32, device=DEV)
    v, g, info = hipops.gp_mll_grad(x.to(DEV).contiguous(), y.to(DEV).contiguous(), theta.float().to(DEV).contiguous(), prior64().float().to(DEV), kernel, n_of=n, **kw)
    return v.cpu(), g.cpu() if g is not None else None, info.cpu()


# measured on the MI355X (profiles/r11_gp_fit_bounds_measured.json): every asserted bound is <= 2 x the larger of the two points' measured values
VALUE_GRAD_BOUNDS = {      # (kernel, F): (value, gradient)
    (0, 1): (3.1e-07, 2.2e-06),
    (0, 5): (1.1e-06, 1.7e-06),
    (0, 18): (9.2e-07, 7.3e-07),
    (1, 1): (3.0e-07, 9.6e-06),
    (1, 5): (9.1e-07, 1.6e-06),
    (1, 18): (9.3e-07, 4.8e-07),
    (2, 1): (2.4e-07, 2.4e-06),
    (2, 5): (1.0e-06, 7.1e-07),
    (2, 18): (8.5e-07, 1.5e-06),
    (3, 1): (3.6e-07, 2.2e-06),
    (3, 5): (9.9e-07, 1.6e-06),
    (3, 18): (8.9e-07, 4.0e-06),
}
assert all(b <= 1e-3 for vb in VALUE_GRAD_BOUNDS.values() for b in vb)      # the north-star tolerance caps every bound


@pytest.mark.parametrize('F', [1, 5, 18])
@pytest.mark.parametrize('kernel', [0, 1, 2, 3])
def test_value_and_gradient_against_f64(kernel, F):
    """J and dJ/dtheta at the default start point and at a seeded perturbation of it, per problem, against f64 autograd.  The yardstick beside the
    measurement: the same formulas in f32 by torch on the CPU sit 3e-8 .. 4.5e-7 from f64 (gradient, relative to its largest component, n <= 130)."""
    x, y = problems(kernel, F)
    want = reference_value_grad(kernel, F)
    for name, theta in points(F):
        v, g, info = device_value_grad(x, y, theta, kernel)
        v64, g64 = want[name]
        assert int(info.abs().max()) == 0
        ev = ((v.double() - v64).abs() / v64.abs()).max()
        eg = ((g.double() - g64).abs().amax(1) / g64.abs().amax(1)).max()
        print(f'kernel {kernel} F {F} {name}: value {float(ev):.3e} grad {float(eg):.3e}')
        bounds.within(f'value {name}', ev, VALUE_GRAD_BOUNDS[kernel, F][0])
        bounds.within(f'grad {name}', eg, VALUE_GRAD_BOUNDS[kernel, F][1])
        v_only, none, _ = device_value_grad(x, y, theta, kernel, want_grad=False)
        assert none is None and torch.equal(v_only, v)


@pytest.mark.parametrize('kernel,F', [(1, 5), (0, 18), (3, 1)])
def test_masked_rows_reach_no_output_and_problems_do_not_see_each_other(kernel, F):
    x, y = problems(kernel, F)
    theta = points(F)[1][1]
    xt = torch.rand(P, 3, F, generator=torch.Generator().manual_seed(5))
    outs = []
    for fill in (0., 1e3, -1e3):
        xf, yf = x.clone(), y.clone()
        for p, n in enumerate(N_OF):
            xf[p, n:] = fill
            yf[p, n:] = -fill
        v, g, info = device_value_grad(xf, yf, theta, kernel)
        n = torch.tensor(N_OF, dtype=torch.int32, device=DEV)
        m, s2, _ = hipops.gp_fit_predict(xf.to(DEV), yf.to(DEV), theta.float().to(DEV).contiguous(), prior64().float().to(DEV), kernel, xt.to(DEV), n_of=n)
        outs.append((v, g, info, m.cpu(), s2.cpu()))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    v, g = outs[0][:2]
    assert torch.isfinite(v).all() and torch.isfinite(g).all()
    for p in range(P):
        v1, g1, _ = device_value_grad(x[p:p + 1], y[p:p + 1], theta[p:p + 1], kernel, n_of=N_OF[p:p + 1])
        assert torch.equal(v1[0], v[p]) and torch.equal(g1[0], g[p]), p


def test_a_failed_factorisation_stays_inside_its_problem():
    kernel, F, bad = 1, 5, 4
    x, y = problems(kernel, F)
    theta = points(F)[0][1].clone()
    v0, g0, info0 = device_value_grad(x, y, theta, kernel)
    xb, tb = x.clone(), theta.clone()
    xb[bad, :32] = xb[bad, 0]      # 32 coincident points, a huge outputscale and noise at its floor: a pivot drowns in the rounding of the others
    tb[bad, F] = 12.
    tb[bad, F + 1] = -40.
    v, g, info = device_value_grad(xb, y, tb, kernel)
    assert int(info[bad]) != 0 and 1 <= int(info[bad]) <= N_OF[bad]
    assert v[bad] == float('inf') and torch.equal(g[bad], torch.zeros(F + 3))
    keep = [p for p in range(P) if p != bad]
    assert torch.equal(v[keep], v0[keep]) and torch.equal(g[keep], g0[keep]) and int(info[keep].abs().max()) == 0 and int(info0.abs().max()) == 0


FIT_BOUND = {0: 4.8e-07, 1: 1.1e-06}      # per kernel, nats per point: <= 2 x measured (profiles/r11_gp_fit_bounds_measured.json), far below the cap of 1e-3


@functools.lru_cache(maxsize=None)
def device_fit(kernel, F):
    x, y = problems(kernel, F)
    hp = dict(HP, nu=NU_OF_KERNEL.get(kernel, 2.5))
    return fast_gp_mix.fit_hyperparameters(x.to(DEV), y.to(DEV), hp, n_of=torch.tensor(N_OF), kernel=kernel)


@pytest.mark.parametrize('kernel', [1, 0])
def test_fit_reaches_the_f64_optimum(kernel):
    F = 5
    x, y = problems(kernel, F)
    model = device_fit(kernel, F)
    theta0 = fast_gp_mix.default_theta(P, F, HP, dtype=torch.float64)
    theta_dev = model.theta.double().cpu()
    for p in range(P):
        _, J_scipy, nit = ref.scipy_fit(theta0[p], x[p], y[p], N_OF[p], prior64(), kernel)
        J_dev = float(ref.objective(theta_dev[p], x[p], y[p], N_OF[p], prior64(), kernel))
        print(f'kernel {kernel} problem {p} n {N_OF[p]}: J64(device) - J64(scipy) = {J_dev - J_scipy:.3e}; iterations {int(model.iterations[p])} vs scipy {nit}; '
              f'evaluations {model.evaluations}; converged {bool(model.converged[p])}')
        bounds.within('J64(theta_device) - J64(theta_scipy)', J_dev - J_scipy, FIT_BOUND[kernel])
        assert int(model.iterations[p]) <= 3 * nit, (p, int(model.iterations[p]), nit)
    assert bool(model.converged.all()) and int(model.info.abs().max()) == 0
    assert model.lengthscale.shape == (P, F) and model.outputscale.shape == (P,) and model.noise.shape == (P,) and model.mean.shape == (P,)
    assert model.objective.shape == (P,) and model.kernel == kernel


POST_MEAN_BOUND = {0: 2.1e-05, 1: 9.7e-06}      # per kernel: |mean - mean64| / (|mean64| + sd64), <= 2 x measured
POST_VAR_BOUND = {0: 2.2e-06, 1: 8.7e-06}       # |var - var64| / var64


@pytest.mark.parametrize('kernel', [1, 0])
def test_posterior_of_the_fitted_model_against_f64_at_the_same_theta(kernel):
    F = 5
    x, y = problems(kernel, F)
    model = device_fit(kernel, F)
    xt = torch.rand(P, 7, F, generator=torch.Generator().manual_seed(11))
    mean, var = model.posterior(xt.to(DEV))
    mean, var = mean.double().cpu(), var.double().cpu()
    theta = model.theta.double().cpu()
    em = ev = 0.
    for p in range(P):
        m64, v64 = ref.posterior(theta[p], x[p], y[p], N_OF[p], prior64(), kernel, xt[p])
        em = max(em, float(((mean[p] - m64).abs() / (m64.abs() + v64.sqrt())).max()))
        ev = max(ev, float(((var[p] - v64).abs() / v64).max()))
    print(f'kernel {kernel}: posterior mean {em:.3e} var {ev:.3e}')
    bounds.within('posterior mean', em, POST_MEAN_BOUND[kernel])
    bounds.within('posterior var', ev, POST_VAR_BOUND[kernel])


def test_evaluate_is_fit_then_predict_per_position_and_dataset():
    T, B, F = 12, 3, 2
    xs, ys = ref.make_problems(B, T, F, 1, seed=21, prior=prior64())
    x, y = xs.transpose(0, 1).contiguous(), ys.transpose(0, 1).contiguous()      # [T,B,F], [T,B]
    for use_mse, start_pos, step in ((False, 0, 1), (True, 3, 2)):
        losses, per_t, seconds = fast_gp_mix.evaluate(x, y, y, use_mse=use_mse, hyperparameters=HP, device=DEV, step_size=step, start_pos=start_pos)
        ts = list(range(max(start_pos, 1), T, step))
        assert losses.shape == (len(ts), B) and losses.device.type == 'cpu' and seconds > 0
        assert per_t.shape == (len(ts) + (1 if start_pos == 0 else 0),)
        if start_pos == 0:
            assert float(per_t[0]) == 0.
        torch.testing.assert_close(per_t[-len(ts):], losses.mean(1), rtol=1e-6, atol=1e-6)      # (the means are taken on the device, in another order)
        # the composition: problem (t, b) is "fit on rows [:t] of dataset b, predict row t" -- all of them as one batch of the public pieces, rows padded to
        # the 64-row bucket and masked through n_of (the same batch `evaluate` forms, so the two are the same arithmetic bit for bit)
        tt = torch.tensor([t for t in ts for _ in range(B)])
        bb = torch.arange(B).repeat(len(ts))
        xp = torch.cat([xs, xs.new_zeros(B, 64 - T, F)], 1)[bb].to(DEV)
        yp = torch.cat([ys, ys.new_zeros(B, 64 - T)], 1)[bb].to(DEV)
        model = fast_gp_mix.fit_hyperparameters(xp, yp, HP, n_of=tt)
        assert bool(model.converged.all())
        mean, var = model.posterior(xs[bb, tt].unsqueeze(1).to(DEV))
        mean, var, target = mean[:, 0].cpu(), var[:, 0].cpu(), ys[bb, tt]
        want = ((mean - target) ** 2 if use_mse else 0.5 * torch.log(2 * math.pi * var) + (target - mean) ** 2 / (2 * var)).reshape(len(ts), B)
        print(f'evaluate use_mse {use_mse}: max |losses - composition| = {float((losses - want).abs().max()):.3e}')
        # mean and var are the same bits on both sides (same batch, same kernels); `evaluate` forms the loss from them on the device, this test on the host,
        # whose log and division round differently: a handful of f32 operations, each within 2 ulp -- 16 eps relative, and as much absolute where the two
        # terms of the density (each of order 1) cancel
        torch.testing.assert_close(losses, want, rtol=16 * 2 ** -23, atol=16 * 2 ** -23)


def test_get_fitted_model_has_the_reference_call_shape():
    x, y = problems(1, 5)
    model, likelihood = fast_gp_mix.get_fitted_model(x[3, :64], y[3, :64], HP, DEV)
    assert isinstance(model, fast_gp_mix.FittedGP) and isinstance(likelihood, fast_gp_mix.FittedGP)
    assert model.lengthscale.shape == (1, 5) and bool(model.converged.all())
    with pytest.raises(AssertionError):
        fast_gp_mix.get_fitted_model(x[3, :64], y[3, :64], dict(HP, sigmoid=True), DEV)
    with pytest.raises(NotImplementedError):
        fast_gp_mix.get_model(x[3:4, :64], y[3:4, :64], HP, sample=False)
