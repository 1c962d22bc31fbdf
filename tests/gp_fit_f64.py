"""f64 reference of the GP hyper-parameter fit (pfn_gp_mll_grad / pfn_gp_fit_predict, priors.fast_gp_mix.fit_hyperparameters): plain torch on the
CPU with autograd, and scipy's L-BFGS-B on it.

Problem p uses the first n rows of x [S,F], y [S]; theta [F+3] = (log l_d, log os, log(noise - floor), c); prior [8] = (a_l, b_l, a_o, b_o, a_n, b_n,
floor, 0).  J = -(1/n) [log N(y; c 1, os k(x, x; l) + noise I) + sum_d lg(l_d) + lg(os) + lg(noise)], lg the Gamma log density."""
import math

import numpy as np
import torch

KERNELS = {0: 'rbf', 1: 'matern52', 2: 'matern32', 3: 'matern12'}


def cov(xa, xb, ls, kernel):
    """k(xa, xb; ls) in the dtype of the inputs; safe to differentiate at coincident points."""
    d = (xa[:, None, :] - xb[None, :, :]) / ls
    d2 = (d * d).sum(-1)
    if kernel == 0:
        return torch.exp(-0.5 * d2)
    r = torch.sqrt(d2.clamp_min(1e-300))
    r = torch.where(d2 > 0, r, torch.zeros_like(r))
    if kernel == 1:
        s = math.sqrt(5.) * r
        return (1 + s + s * s / 3) * torch.exp(-s)
    if kernel == 2:
        s = math.sqrt(3.) * r
        return (1 + s) * torch.exp(-s)
    return torch.exp(-r)


def unpack(theta, prior, F):
    return theta[:F].exp(), theta[F].exp(), theta[F + 1].exp() + prior[6], theta[F + 2]


def _lg(v, a, b):
    return a * torch.log(b) - torch.lgamma(a) + (a - 1) * torch.log(v) - b * v


def objective(theta, x, y, n, prior, kernel):
    """J(theta), differentiable in theta (f64)."""
    F = x.shape[1]
    x, y, prior = x[:n].double(), y[:n].double(), torch.as_tensor(prior).double()
    ls, os_, noise, c = unpack(theta, prior, F)
    K = os_ * cov(x, x, ls, kernel) + noise * torch.eye(n, dtype=torch.float64)
    L = torch.linalg.cholesky(K)
    w = torch.linalg.solve_triangular(L, (y - c)[:, None], upper=False)[:, 0]
    ll = -0.5 * (w * w).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * n * math.log(2 * math.pi)
    lp = _lg(ls, prior[0], prior[1]).sum() + _lg(os_, prior[2], prior[3]) + _lg(noise, prior[4], prior[5])
    return -(ll + lp) / n


def value_and_grad(theta, x, y, n, prior, kernel, fit_mean=True):
    t = torch.as_tensor(theta, dtype=torch.float64).clone().requires_grad_(True)
    J = objective(t, x, y, n, prior, kernel)
    g, = torch.autograd.grad(J, t)
    if not fit_mean:
        g[-1] = 0
    return J.detach(), g


def batch_value_and_grad(theta, x, y, n_of, prior, kernel, fit_mean=True):
    """The device call's shapes: theta [P,F+3], x [P,S,F], y [P,S], n_of [P] -> (value [P], grad [P,F+3]) in f64."""
    vs, gs = zip(*[value_and_grad(theta[p], x[p], y[p], int(n_of[p]), prior, kernel, fit_mean) for p in range(theta.shape[0])])
    return torch.stack(vs), torch.stack(gs)


def scipy_fit(theta0, x, y, n, prior, kernel, fit_mean=True):
    """L-BFGS-B (scipy defaults) from theta0.  Returns (theta, J, iterations)."""
    from scipy.optimize import minimize

    def fun(t):
        J, g = value_and_grad(t, x, y, n, prior, kernel, fit_mean)
        return float(J), g.numpy()

    res = minimize(fun, np.asarray(theta0, dtype=np.float64), jac=True, method='L-BFGS-B')
    return torch.from_numpy(res.x), float(res.fun), int(res.nit)


def posterior(theta, x, y, n, prior, kernel, x_test):
    """(mean [m], var [m] with observation noise) of the GP with parameters theta given the first n rows, at x_test [m,F] (f64)."""
    F = x.shape[1]
    theta, prior = torch.as_tensor(theta).double(), torch.as_tensor(prior).double()
    x, y, xt = x[:n].double(), y[:n].double(), x_test.double()
    ls, os_, noise, c = unpack(theta, prior, F)
    K = os_ * cov(x, x, ls, kernel) + noise * torch.eye(n, dtype=torch.float64)
    L = torch.linalg.cholesky(K)
    w = torch.linalg.solve_triangular(L, (y - c)[:, None], upper=False)[:, 0]
    v = torch.linalg.solve_triangular(L, os_ * cov(x, xt, ls, kernel), upper=False)      # [n, m]
    return c + v.T @ w, os_ + noise - (v * v).sum(0)


def sequential_evaluate(x, y, prior, kernel, theta_of, use_mse=False, step_size=1, start_pos=0):
    """The sequential evaluation built from the pieces above: x [T,B,F], y [T,B]; theta_of(t, b) gives the parameters fitted on rows [:t] of dataset b.
    Returns losses [n_t, B] (f64)."""
    T, B, _ = x.shape
    ts = list(range(max(start_pos, 1), T, step_size))
    out = torch.zeros(len(ts), B, dtype=torch.float64)
    for i, t in enumerate(ts):
        for b in range(B):
            mean, var = posterior(theta_of(t, b), x[:, b], y[:, b], t, prior, kernel, x[t:t + 1, b])
            r = y[t, b].double() - mean[0]
            out[i, b] = r * r if use_mse else 0.5 * torch.log(2 * math.pi * var[0]) + r * r / (2 * var[0])
    return out


def make_problems(P, S, F, kernel, seed, prior, n_of=None):
    """x ~ U[0,1), y drawn in f64 from the model itself: l ~ Gamma(3, 6), os in [.5, 20], noise in [1e-2, .3 os], zero mean.  Returns f32 (x [P,S,F], y [P,S])."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(P, S, F, generator=g, dtype=torch.float64).float()
    y = torch.zeros(P, S, dtype=torch.float64)
    for p in range(P):
        ls = (torch._standard_gamma(torch.full((F,), 3., dtype=torch.float64), generator=g) / 6.).clamp_min(.05)
        os_ = .5 + 19.5 * torch.rand((), generator=g, dtype=torch.float64)
        noise = 1e-2 + (.3 * os_ - 1e-2) * torch.rand((), generator=g, dtype=torch.float64)
        xp = x[p].double()
        K = os_ * cov(xp, xp, ls, kernel) + noise * torch.eye(S, dtype=torch.float64)
        y[p] = torch.linalg.cholesky(K) @ torch.randn(S, generator=g, dtype=torch.float64)
    return x, y.float()
