"""Mixture-of-GPs prior: every dataset draws its own kernel hyper-parameters from Gamma hyper-priors, then
y_b ~ N(0, outputscale_b * Matern_{5/2}(x_b, x_b; lengthscale_b[ARD]) + noise_b * I).

Replaces reference priors/fast_gp_mix.py `get_batch` (:58-134), whose model is botorch's SingleTaskGP with
gpytorch priors sampled through pyro (`get_model(...).pyro_sample_from_prior()`, :24-55): with a batched
train-x of shape [n, T, F] every one of the n datasets gets an independent draw of
    lengthscale_d ~ Gamma(lengthscale_concentration 3.0, rate 6.0)   per feature (ARD), :33
    outputscale   ~ Gamma(outputscale_concentration 0.5, rate 0.15)  :37
    noise         ~ Gamma(noise_concentration 1.1, rate 0.05), floored at botorch's MIN_INFERRED_NOISE_LEVEL 1e-4  :26-35
and the sample is `likelihood(model(x)).sample()` in prior mode (:96-99).  Here the hyper-parameters are drawn
with torch on the device and the whole batch goes through ONE call of the HIP sampler
(`pfn_gp_prior_sample`, Matern-5/2 ARD Gram -> blocked Cholesky -> L z) with per-dataset hyper-parameters;
the reference's Python loop over groups of `batch_size_per_gp_sample` datasets (:87) only exists to bound
gpytorch's memory and has no effect on the distribution, so the argument is accepted and ignored except for the
divisibility check.  `y_minmax_norm`, `sigmoid` (:100-103) and the `fix_to_range` rejection step (:104-122) are
kept.  Always exact Cholesky; nu in {0.5, 1.5, 2.5} (gpytorch MaternKernel's closed forms; the reference default is 2.5, :40).

The MAP-II baseline of the reference (`get_fitted_model`, :156-169: botorch `fit_gpytorch_model` on gpytorch's ExactMarginalLogLikelihood, and
`evaluate = partial(fast_gp.evaluate, get_model_on_device=get_fitted_model)`) is `fit_hyperparameters` / `get_fitted_model` / `evaluate` below: the
objective and its gradient come from the device (`pfn_gp_mll_grad`, csrc/gp_fit.hip: one read of K^-1 for all ARD lengthscales), a batched L-BFGS in
torch ops drives every problem of the batch at once, and `FittedGP.posterior` is `pfn_gp_fit_predict`.  The objective is gpytorch's (marginal log
likelihood plus Gamma hyper-priors on the natural values, divided by n) in LOG parameters with the noise floor built into the parameterisation
(noise = 1e-4 + exp(eta)) -- INTEGRATION.md lists both as deliberate deviations from softplus + an L-BFGS-B box.

A pathology of the DEFAULT hyper-prior: outputscale_concentration = 0.5 makes the outputscale log-prior (a - 1) log os unbounded as os -> 0, so J has
no minimum there (J -> -inf with the data explained by noise alone).  L-BFGS started at gpytorch's defaults (ln 2) finds the interior local optimum when
there is one, as botorch does; `FittedGP.converged` and `.outputscale` show when it did not (a run-away outputscale ends at max_iter with
converged False).  The tests fit with outputscale_concentration = 2.

The MCMC baseline of the reference (get_mcmc_model, get_mean_logdensity, evaluate_, :171-268: pyro NUTS over the kernel hyper-parameters, one (t, b) problem at a
time) is `sample_hyperparameter_posterior` / `MCMCGP` / `get_mcmc_model` / `get_mean_logdensity` / `evaluate_` below: the potential and its gradient are the
same device call as MAP-II (`pfn_gp_mll_grad`), the sampler is the batched NUTS of mcmc.py (`pfn_nuts_advance`, csrc/gp_mcmc.hip: every chain of every problem
advances by one leapfrog per pass), and the per-sample predictive distributions come from `pfn_gp_fit_predict`.  INTEGRATION.md lists the deviations from pyro.
"""
import math

import torch
from torch import nn

from transformerscandobayesianinference_amd import _hip, hipops, mcmc
from transformerscandobayesianinference_amd.bar_distribution import BarDistribution
from transformerscandobayesianinference_amd.priors import fast_gp
from transformerscandobayesianinference_amd.priors.utils import get_batch_to_dataloader
from transformerscandobayesianinference_amd.utils import default_device

MIN_INFERRED_NOISE_LEVEL = 1e-4   # botorch.models.gp_regression (reference :10,31)


def sample_hyperparameters(n, num_features, hyperparameters, device, generator=None):
    """Per-dataset draws of (lengthscale[n,F], outputscale[n], noise[n]) from the Gamma hyper-priors (reference :26,33,37)."""
    hp = hyperparameters or {}

    def gamma(concentration, rate, shape):
        c = torch.full(shape, float(concentration), device=device)
        if generator is None:
            return torch._standard_gamma(c) / float(rate)
        return torch._standard_gamma(c.cpu(), generator=generator).to(device) / float(rate)

    ls = gamma(hp.get('lengthscale_concentration', 3.0), hp.get('lengthscale_rate', 6.0), (n, num_features))
    osc = gamma(hp.get('outputscale_concentration', .5), hp.get('outputscale_rate', 0.15), (n,))
    nz = gamma(hp.get('noise_concentration', 1.1), hp.get('noise_rate', 0.05), (n,)).clamp_min(MIN_INFERRED_NOISE_LEVEL)
    # a Gamma(0.5, .) outputscale has mass at 0+: keep the Gram matrix positive definite in f32
    return ls.clamp_min(1e-6), osc.clamp_min(1e-12), nz


@torch.no_grad()
def get_batch(batch_size, seq_len, num_features, device=default_device, hyperparameters=None,
              batch_size_per_gp_sample=None, num_outputs=1, fix_to_range=None, equidistant_x=False):
    """Same signature and return layout as the reference: (x[T,B,F], y[T,B], target_y[T,B])."""
    assert num_outputs == 1
    hyperparameters = hyperparameters or {}
    nu = float(hyperparameters.get('nu', 2.5))
    if nu not in fast_gp.MATERN_KERNEL_OF_NU:
        raise ValueError(f'priors.fast_gp_mix: Matern nu must be 0.5, 1.5 or 2.5 (gpytorch MaternKernel, reference :40), got {nu}')
    matern = fast_gp.MATERN_KERNEL_OF_NU[nu]
    if batch_size_per_gp_sample is not None:   # grouping has no effect here (one batched sampler call); keep the reference's check (:77)
        assert batch_size % batch_size_per_gp_sample == 0
    factor = 2 if fix_to_range is not None else 1
    out_x, out_y = [], []
    need = batch_size
    attempts = 0
    while need > 0:
        n = need * factor                                  # the reference draws 2x candidates under fix_to_range (:81-82)
        x = None
        if equidistant_x:
            assert num_features == 1
            x = torch.linspace(0, 1., seq_len).unsqueeze(0).repeat(n, 1).unsqueeze(-1)
        ls, osc, nz = sample_hyperparameters(n, num_features, hyperparameters, device)
        # anything below that copies y (normalisation, rejection) must see a verified draw: check at once there; a plain
        # draw inside a prefetching loader is verified before its batch is handed out (priors/utils.py)
        copies = bool(hyperparameters.get('y_minmax_norm') or hyperparameters.get('sigmoid') or fix_to_range is not None)
        x, y, _, _ = fast_gp.gp_sample(n, seq_len, num_features, device, ls, osc, nz, matern, x=x,
                                       check='sync' if copies else True)
        if hyperparameters.get('y_minmax_norm'):
            lo, hi = y.min(1, keepdim=True)[0], y.max(1, keepdim=True)[0]
            y = (y - lo) / (hi - lo)
        if hyperparameters.get('sigmoid'):
            y = y.sigmoid()
        if fix_to_range is not None:
            ok = ~((y < fix_to_range[0]) | (y >= fix_to_range[1])).any(1)
            x, y = x[ok][:need], y[ok][:need]
            attempts += 1
            if attempts > 100:
                raise RuntimeError('priors.fast_gp_mix: fix_to_range rejects (almost) every draw; change the hyper-parameters '
                                   '(e.g. decrease the outputscale) -- the reference prints this advice and loops forever')
        out_x.append(x)
        out_y.append(y)
        need -= x.shape[0]
    x = torch.cat(out_x, 0) if len(out_x) > 1 else out_x[0]
    y = torch.cat(out_y, 0) if len(out_y) > 1 else out_y[0]
    sample = y.transpose(0, 1)
    return x.transpose(0, 1), sample, sample


class DataLoader(get_batch_to_dataloader(get_batch)):
    num_outputs = 1
    prefetch = True
    prefetch_group = 10
    prefetch_group_datasets = 640
    prefetch_memory_share = 0.125          # as priors.fast_gp: a group's factorisation workspace stays inside this share of free memory
    prefetch_bytes_per_dataset = staticmethod(fast_gp.workspace_bytes_per_dataset)     # from the library (pfn_gp_workspace_bytes), not a constant factor

    @torch.no_grad()
    def validate(self, model, step_size=1, start_pos=0):
        """Mean-squared error of the posterior-predictive mean at every evaluation position on one fresh batch
        (reference :139-153); forward-only passes through the HIP stack."""
        if isinstance(model.criterion, BarDistribution):
            (x, y), target_y = self.gbm(**self.get_batch_kwargs, fuse_x_y=self.fuse_x_y)
            model.eval()
            losses = []
            for eval_pos in range(start_pos, len(x), step_size):
                logits = model((x, y), single_eval_pos=eval_pos)
                means = model.criterion.mean(logits)  # num_evals x batch_size
                losses.append(nn.functional.mse_loss(means[0], target_y[eval_pos]))
            model.train()
            return torch.stack(losses)
        return 123.


class _PriorDraw:
    """What `likelihood(model(x))` is in the reference's sampling path (:96-99): the prior-predictive distribution of y at x under ONE draw of
    the hyper-parameters per dataset.  `.sample()` is the HIP sampler (Gram -> blocked Cholesky -> L z, csrc/gp_prior.hip)."""

    def __init__(self, model, x, with_noise):
        self.model, self.x, self.with_noise = model, x, with_noise

    @torch.no_grad()
    def sample(self):
        m = self.model
        x = self.x if self.x.dim() == 3 else self.x.unsqueeze(0)
        noise = m.noise if self.with_noise else torch.full_like(m.noise, 1e-9)      # the latent f: no observation noise (a jitter keeps f32 positive definite)
        _, y, _, _ = fast_gp.gp_sample(x.shape[0], x.shape[1], x.shape[2], x.device, m.lengthscale, m.outputscale, noise, m.kernel, x=x.float(), check='sync')
        return y


class _SampledLikelihood:
    """GaussianLikelihood of a sampled model: adds the sampled observation noise to the prior at x."""

    def __init__(self, model):
        self.model = model
        self.noise = model.noise

    def __call__(self, prior):
        return _PriorDraw(prior.model, prior.x, with_noise=True)


class SampledGP:
    """`get_model(x, y, hyperparameters, sample=True)[0]` (reference :24-55: `SingleTaskGP(...).pyro_sample_from_prior()`): a GP whose kernel
    hyper-parameters were DRAWN from the Gamma hyper-priors, one independent draw per dataset of the batch.  Exposes the sampled
    `lengthscale [n, F]` (ARD), `outputscale [n]`, `noise [n]` (floored at botorch's MIN_INFERRED_NOISE_LEVEL) and `nu`; `model(x)` is the
    prior at x, `likelihood(model(x)).sample()` the draw `get_batch` takes ([n, T], :96-99)."""

    def __init__(self, x, hyperparameters):
        hp = hyperparameters or {}
        x = x if x.dim() == 3 else x.unsqueeze(0)
        self.nu = float(hp.get('nu', 2.5))
        if self.nu not in fast_gp.MATERN_KERNEL_OF_NU:
            raise ValueError(f'priors.fast_gp_mix: Matern nu must be 0.5, 1.5 or 2.5 (gpytorch MaternKernel, reference :40), got {self.nu}')
        self.kernel = fast_gp.MATERN_KERNEL_OF_NU[self.nu]
        self.lengthscale, self.outputscale, self.noise = sample_hyperparameters(x.shape[0], x.shape[-1], hp, x.device)
        self.likelihood = _SampledLikelihood(self)

    def __call__(self, x):
        return _PriorDraw(self, x, with_noise=False)

    def to(self, device):
        self.lengthscale, self.outputscale, self.noise = self.lengthscale.to(device), self.outputscale.to(device), self.noise.to(device)
        return self


def get_model(x, y, hyperparameters: dict, sample=True):
    """Reference :24-55.  sample=True (the only form `get_batch` uses, :95): (sampled model, its likelihood), hyper-parameters drawn per dataset of the
    batched x [n, T, F]; `y` is ignored as in the reference's prior mode (it passes an empty tensor).  sample=False builds the botorch model for
    FITTING (get_fitted_model, :156-171), which needs gpytorch / botorch and is outside this path."""
    if not sample:
        raise NotImplementedError('priors.fast_gp_mix.get_model(sample=False) is the botorch SingleTaskGP for hyper-parameter FITTING (reference :156-171); '
                                  'fitting / MCMC baselines need gpytorch / botorch and are outside the MI355X hot path (SURVEY.md 2)')
    model = SampledGP(x, hyperparameters)
    return model, model.likelihood


# ---------------------------------------------------------------------------------------------------------------------
# MAP-II: hyper-parameters fitted to the observed points (reference :156-169)
# ---------------------------------------------------------------------------------------------------------------------
def hyperprior_vector(hyperparameters, device=None, dtype=torch.float32):
    """prior [8] of pfn_gp_mll_grad: (a_l, b_l, a_o, b_o, a_n, b_n, noise_floor, 0) with the keys and defaults of `sample_hyperparameters`."""
    hp = hyperparameters or {}
    return torch.tensor([hp.get('lengthscale_concentration', 3.0), hp.get('lengthscale_rate', 6.0), hp.get('outputscale_concentration', .5),
                         hp.get('outputscale_rate', 0.15), hp.get('noise_concentration', 1.1), hp.get('noise_rate', 0.05), MIN_INFERRED_NOISE_LEVEL, 0.],
                        dtype=dtype, device=device)


def default_theta(P, num_features, hyperparameters, device=None, dtype=torch.float32):
    """The start point, gpytorch's defaults: lengthscale_d = outputscale = softplus(0) = ln 2, noise = the prior mode (a_n - 1) / b_n (the prior mean when
    the mode is not above the floor), constant mean 0.  theta = (log l_d, log os, log(noise - floor), c)."""
    hp = hyperparameters or {}
    a_n, b_n = float(hp.get('noise_concentration', 1.1)), float(hp.get('noise_rate', 0.05))
    noise = (a_n - 1.) / b_n
    if not noise > 2 * MIN_INFERRED_NOISE_LEVEL:
        noise = max(a_n / b_n, 2 * MIN_INFERRED_NOISE_LEVEL)
    theta = torch.zeros(P, num_features + 3, dtype=dtype, device=device)
    theta[:, :num_features + 1] = math.log(math.log(2.))
    theta[:, num_features + 1] = math.log(noise - MIN_INFERRED_NOISE_LEVEL)
    return theta


def batched_lbfgs(fun, theta0, max_iter=200, gtol=1e-5, ftol=1e-7, history=10, c1=1e-4, max_backtracks=20, sync_every=10, callback=None):
    """L-BFGS (two-loop recursion over the last `history` pairs, Armijo backtracking) on P independent problems at once, in torch ops on [P, D] tensors of
    theta0's device and dtype.  fun(theta [P,D]) -> (value [P], grad [P,D]) evaluates all of them in one call.  Every pass of the loop is ONE call of `fun`
    at every problem's own trial point: a problem whose trial passes the Armijo test takes the step, updates its own history and direction and tries
    step 1 next; one whose trial fails (or is not finite: a rejected step) halves its own step.  A problem is frozen by masking once it is done -- its
    parameters are never written again -- and the batch is not resized.  Done means converged (|grad|_inf <= gtol; or an accepted step lowered the value
    by <= ftol max(|f|, 1); or the quasi-Newton step predicts a decrease -g.d <= ftol max(|f|, 1)), failed (non-finite value at the start, or
    `max_backtracks` halvings in a row twice with a reset to steepest descent in between), or out of iterations (max_iter accepted steps).  The host
    looks at the device once every `sync_every` passes, to test "all done".
    Returns dict(theta, objective, grad, iterations [accepted steps], converged, evaluations)."""
    theta = theta0.clone()
    P, D = theta.shape
    f, g = fun(theta)
    f, g = f.clone(), g.clone()
    fin = torch.isfinite(f) & torch.isfinite(g).all(1)
    g = torch.where(fin[:, None], g, torch.zeros_like(g))
    converged = fin & (g.abs().amax(1) <= gtol)
    done = converged | ~fin
    iters = torch.zeros(P, dtype=torch.int64, device=theta.device)
    backtracks = torch.zeros_like(iters)
    restarted = torch.zeros(P, dtype=torch.bool, device=theta.device)
    Sh = theta.new_zeros(history, P, D)
    Yh = theta.new_zeros(history, P, D)
    rho = theta.new_zeros(history, P)
    one = theta.new_ones(P)

    def first_step(g):
        return torch.minimum(one, 1. / g.abs().sum(1).clamp_min(1e-30))

    def direction(g, Sh, Yh, rho):
        q = g.clone()
        a = []
        for i in range(history - 1, -1, -1):
            ai = rho[i] * (Sh[i] * q).sum(1)
            q = q - ai[:, None] * Yh[i]
            a.append(ai)
        yy = (Yh[-1] * Yh[-1]).sum(1)
        gamma = torch.where(rho[-1] > 0, 1. / (rho[-1] * yy).clamp_min(1e-30), one)
        r = gamma[:, None] * q
        for i in range(history):
            b = rho[i] * (Yh[i] * r).sum(1)
            r = r + Sh[i] * (a[history - 1 - i] - b)[:, None]
        return -r

    d = -g
    gd = (g * d).sum(1)
    alpha = first_step(g)
    evaluations = 1
    for it in range(3 * max_iter + 2 * max_backtracks):
        if it % sync_every == 0 and bool(done.all()):
            break
        trial = torch.where(done[:, None], theta, theta + alpha[:, None] * d)
        ft, gt = fun(trial)
        evaluations += 1
        ok = ~done & torch.isfinite(ft) & torch.isfinite(gt).all(1)
        ok = ok & (torch.where(ok, ft, f) <= f + c1 * alpha * gd)
        okc = ok[:, None]
        gt = torch.where(okc, gt, g)
        # accepted steps: the pair (s, y) joins that problem's history when its curvature is positive
        s, yv = trial - theta, gt - g
        sy, yy = (s * yv).sum(1), (yv * yv).sum(1)
        push = ok & (sy > 1e-10 * yy) & (yy > 0)
        pc = push[None, :, None]
        Sh = torch.where(pc, torch.cat([Sh[1:], s[None]]), Sh)
        Yh = torch.where(pc, torch.cat([Yh[1:], yv[None]]), Yh)
        rho = torch.where(push[None], torch.cat([rho[1:], (1. / torch.where(push, sy, one))[None]]), rho)
        fscale = torch.maximum(torch.maximum(f.abs(), torch.where(ok, ft, f).abs()), one)
        conv_f = ok & (f - ft <= ftol * fscale)
        theta = torch.where(okc, trial, theta)
        f = torch.where(ok, ft, f)
        g = gt
        iters = iters + ok
        conv_g = ok & (g.abs().amax(1) <= gtol)
        # rejected steps: halve; too many in a row: once from steepest descent with an empty history, then give up
        rej = ~done & ~ok
        backtracks = torch.where(rej, backtracks + 1, torch.zeros_like(backtracks))
        stuck = rej & (backtracks > max_backtracks)
        give_up = stuck & (restarted | (rho.amax(0) <= 0))
        restart = stuck & ~give_up
        restarted = (restarted | restart) & ~ok
        rho = torch.where(restart[None], torch.zeros_like(rho), rho)
        backtracks = torch.where(restart, torch.zeros_like(backtracks), backtracks)
        d_new = direction(g, Sh, Yh, rho)
        gd_new = (g * d_new).sum(1)
        uphill = (ok | restart) & ~(gd_new < 0)
        rho = torch.where(uphill[None], torch.zeros_like(rho), rho)
        d_new = torch.where(uphill[:, None], -g, d_new)
        gd_new = torch.where(uphill, -(g * g).sum(1), gd_new)
        fresh = ok | restart
        conv_d = ok & (-gd_new <= ftol * torch.maximum(f.abs(), one))
        d = torch.where(fresh[:, None], d_new, d)
        gd = torch.where(fresh, gd_new, gd)
        alpha = torch.where(fresh, torch.where(rho.amax(0) > 0, one, first_step(g)), alpha * 0.5)
        newly = conv_f | conv_g | conv_d
        converged = converged | newly
        done = done | newly | give_up | (iters >= max_iter)
        if callback is not None:
            callback(it, theta, done)
    return dict(theta=theta, objective=f, grad=g, iterations=iters, converged=converged, evaluations=evaluations)


class FittedGP:
    """The GP with hyper-parameters fitted to (x, y) by MAP-II, one independent fit per problem of the batch: `lengthscale [P,F]`, `outputscale [P]`,
    `noise [P]`, `mean [P]` (the constant mean), `objective [P]` (J at the optimum, nats per point), `iterations [P]`, `converged [P]`, `info [P]`
    (0, or index + 1 of a non-positive pivot at the final point), `nu`, `kernel`.  Stands for both the model and the likelihood of the reference's
    `get_fitted_model`; `posterior(x_test)` is the predictive distribution of y at x_test (observation noise included)."""

    def __init__(self, x, y, n_of, theta, prior, kernel, nu, objective, iterations, converged, info, evaluations=None):
        F = x.shape[-1]
        self._x, self._y, self._n_of, self.theta, self._prior = x, y, n_of, theta, prior
        self.kernel, self.nu = kernel, nu
        self.lengthscale = theta[:, :F].exp()
        self.outputscale = theta[:, F].exp()
        self.noise = theta[:, F + 1].exp() + MIN_INFERRED_NOISE_LEVEL
        self.mean = theta[:, F + 2].clone()
        self.objective, self.iterations, self.converged, self.info, self.evaluations = objective, iterations, converged, info, evaluations
        self.likelihood = self

    @torch.no_grad()
    def posterior(self, x_test):
        """(mean [P,m], var [P,m]) at x_test [P,m,F] through pfn_gp_fit_predict."""
        x_test = x_test.to(self._x.device).float()
        if x_test.dim() == 2:
            x_test = x_test.unsqueeze(0)
        mean, var, _ = hipops.gp_fit_predict(self._x, self._y, self.theta, self._prior, self.kernel, x_test.contiguous(), n_of=self._n_of)
        return mean, var


def _kernel_of(hyperparameters, kernel):
    nu = float((hyperparameters or {}).get('nu', 2.5))
    if kernel is not None:
        return int(kernel), nu
    if nu not in fast_gp.MATERN_KERNEL_OF_NU:
        raise ValueError(f'priors.fast_gp_mix: Matern nu must be 0.5, 1.5 or 2.5 (gpytorch MaternKernel, reference :40), got {nu}')
    return fast_gp.MATERN_KERNEL_OF_NU[nu], nu


@torch.no_grad()
def fit_hyperparameters(x, y, hyperparameters=None, n_of=None, init=None, max_iter=200, gtol=1e-5, fit_mean=True, ftol=1e-7, kernel=None):
    """MAP-II fit of P independent GPs: x [P,S,F], y [P,S] on the GPU; problem p uses its first n_of[p] rows (all S when None).  `hyperparameters` holds
    the Gamma hyper-prior (keys and defaults of `sample_hyperparameters`) and `nu`; `kernel` overrides the covariance function (fast_gp.KERNEL_*).
    init: a theta [P,F+3] tensor replacing the start point (`default_theta`).  fit_mean=False keeps the constant mean at its start value.
    Returns a `FittedGP`."""
    if x.device.type != 'cuda':
        raise _hip.HipExtensionError(f'the GP hyper-parameter fit runs on the GPU only (got device {x.device}); no CPU fallback')
    kernel, nu = _kernel_of(hyperparameters, kernel)
    dev = x.device
    P, S, F = x.shape
    xp, yp = x.float(), y.float().reshape(P, S)
    n_of = torch.full((P,), S, dtype=torch.int32, device=dev) if n_of is None else torch.as_tensor(n_of, device=dev).to(torch.int32).clamp(1, S).contiguous()
    Sp = (S + 3) // 4 * 4
    if Sp != S:      # padded rows are masked through n_of: nothing in them is read
        xp = torch.cat([xp, xp.new_zeros(P, Sp - S, F)], 1)
        yp = torch.cat([yp, yp.new_zeros(P, Sp - S)], 1)
    xp, yp = xp.contiguous(), yp.contiguous()
    prior = hyperprior_vector(hyperparameters, dev)
    theta0 = default_theta(P, F, hyperparameters, dev) if init is None else torch.as_tensor(init, dtype=torch.float32, device=dev).reshape(P, F + 3).clone()
    ws = hipops.gp_fit_workspace(P, Sp, dev)
    flags = 0 if fit_mean else 1

    def fun(theta):
        value, grad, _ = hipops.gp_mll_grad(xp, yp, theta.contiguous(), prior, kernel, n_of=n_of, flags=flags, ws=ws)
        return value, grad

    res = batched_lbfgs(fun, theta0, max_iter=max_iter, gtol=gtol, ftol=ftol)
    theta = res['theta'].contiguous()
    _, _, info = hipops.gp_mll_grad(xp, yp, theta, prior, kernel, n_of=n_of, flags=flags, want_grad=False, ws=ws)
    return FittedGP(xp, yp, n_of, theta, prior, kernel, nu, res['objective'], res['iterations'], res['converged'], info, res['evaluations'])


def _reject_output_warping(hyperparameters):
    hp = hyperparameters or {}
    assert not (hp.get('sigmoid') or hp.get('y_minmax_norm')), 'Sigmoid and y_minmax_norm can only be used to sample models...'      # reference :54


def get_fitted_model(x, y, hyperparameters, device):
    """Reference :156-169: the model with hyper-parameters fitted to (x, y) and its likelihood -- here one object plays both parts.  x [n,F] or [P,n,F],
    y [n], [n,1] or [P,n].  Does not go through `get_model(sample=False)`, which keeps raising."""
    _reject_output_warping(hyperparameters)
    x = torch.as_tensor(x).to(device).float()
    x = x if x.dim() == 3 else x.unsqueeze(0)
    y = torch.as_tensor(y).to(device).float().reshape(x.shape[0], x.shape[1])
    model = fit_hyperparameters(x, y, hyperparameters)
    return model, model.likelihood


EVALUATE_MEMORY_SHARE = 0.125      # a group of problems keeps its workspace inside this share of the free device memory, as the prefetching loaders do
EVALUATE_MAX_GROUP = 4096


@torch.no_grad()
def evaluate(x, y, y_non_noisy, use_mse=False, hyperparameters={}, device=default_device, step_size=1, start_pos=0):
    """The MAP-II baseline (reference: `partial(fast_gp.evaluate, get_model_on_device=get_fitted_model)`): for every t in
    range(max(start_pos, 1), T, step_size) and every dataset b, hyper-parameters are fitted on rows [:t] of (x[:, b], y[:, b]) and the loss is taken at row
    t -- the negative log density of y[t] under the fitted predictive, or the squared error of its mean.  x [T,B,F], y [T,B]; returns what
    `fast_gp.evaluate` returns: (losses [n_t, B] on the CPU, their means per t with a leading 0. when start_pos == 0, seconds).  All (t, b) problems are
    batched: they are grouped by n = t rounded up to a multiple of 64 (so padding costs at most a bucket) and every group is cut to
    EVALUATE_MEMORY_SHARE of the free device memory."""
    import time
    start_time = time.time()
    _reject_output_warping(hyperparameters)
    dev = torch.device(device)
    T, B, F = x.shape
    xb = x.to(dev).float().transpose(0, 1).contiguous()
    yb = y.to(dev).float().reshape(T, B).transpose(0, 1).contiguous()
    ts = list(range(max(start_pos, 1), T, step_size))
    losses = torch.zeros(len(ts), B, dtype=torch.float32, device=dev)
    buckets = {}
    for i, t in enumerate(ts):
        buckets.setdefault((t + 63) // 64 * 64, []).append(i)
    for Sb, members in sorted(buckets.items()):
        xs, ys = xb[:, :Sb], yb[:, :Sb]
        if Sb > T:
            xs = torch.cat([xs, xs.new_zeros(B, Sb - T, F)], 1)
            ys = torch.cat([ys, ys.new_zeros(B, Sb - T)], 1)
        per_problem = max(1, int(_hip.lib().pfn_gp_fit_workspace_bytes(1, Sb)) + 8 * Sb * (F + 1))
        cap = max(1, min(EVALUATE_MAX_GROUP, int(EVALUATE_MEMORY_SHARE * torch.cuda.mem_get_info(dev)[0]) // per_problem))
        ii = torch.as_tensor([i for i in members for _ in range(B)], dtype=torch.long, device=dev)
        tt = torch.as_tensor([ts[i] for i in members for _ in range(B)], dtype=torch.long, device=dev)
        bb = torch.arange(B, device=dev).repeat(len(members))
        for lo in range(0, len(tt), cap):
            i_, t_, b_ = ii[lo:lo + cap], tt[lo:lo + cap], bb[lo:lo + cap]
            model = fit_hyperparameters(xs[b_], ys[b_], hyperparameters, n_of=t_)
            mean, var = model.posterior(xb[b_, t_].unsqueeze(1))
            mean, var, target = mean[:, 0], var[:, 0], yb[b_, t_]
            losses[i_, b_] = (mean - target) ** 2 if use_mse else 0.5 * torch.log(2 * math.pi * var) + (target - mean) ** 2 / (2 * var)
    per_t = losses.mean(1)
    if start_pos == 0:
        per_t = torch.cat([per_t.new_zeros(1), per_t])
    torch.cuda.synchronize(dev)
    return losses.to('cpu'), per_t.to('cpu'), time.time() - start_time


# ---------------------------------------------------------------------------------------------------------------------
# NUTS over the hyper-parameters (reference :171-268)
# ---------------------------------------------------------------------------------------------------------------------
def _memory_cap(dev, S, F):
    per_problem = max(1, int(_hip.lib().pfn_gp_fit_workspace_bytes(1, S)) + 8 * S * (F + 1))
    return max(1, min(EVALUATE_MAX_GROUP, int(EVALUATE_MEMORY_SHARE * torch.cuda.mem_get_info(dev)[0]) // per_problem))


class MCMCGP:
    """The GP under posterior samples of its hyper-parameters, P independent problems: `theta [P, N_tot, F+3]` (log lengthscale_d, log outputscale,
    log(noise - floor), mean 0; N_tot = chains x samples, chain-major), `lengthscale [P,N_tot,F]`, `outputscale [P,N_tot]`, `noise [P,N_tot]`, `stats
    [P, chains, W+N, 8]` (mcmc.batched_nuts), `divergences [P]` (diverging sampling transitions), `evaluations` (passes of the sampler).  Stands for both the
    model and the likelihood of the reference's `get_mcmc_model`."""

    def __init__(self, x, y, n_of, theta, prior, kernel, nu, stats, num_samples, evaluations):
        F = x.shape[-1]
        self._x, self._y, self._n_of, self.theta, self._prior = x, y, n_of, theta, prior
        self.kernel, self.nu = kernel, nu
        self.lengthscale = theta[..., :F].exp()
        self.outputscale = theta[..., F].exp()
        self.noise = theta[..., F + 1].exp() + MIN_INFERRED_NOISE_LEVEL
        self.stats, self.evaluations = stats, evaluations
        self.divergences = stats[:, :, stats.shape[2] - num_samples:, 4].sum((1, 2)).to(torch.int64)
        self.likelihood = self

    @torch.no_grad()
    def posterior(self, x_test, use_likelihood=True):
        """Per-sample predictive (mean, var) [P, N_tot, m] at x_test [P,m,F] through pfn_gp_fit_predict: the rows of (x, y) are gathered per sample and the
        batch is cut to EVALUATE_MEMORY_SHARE of the free device memory.  use_likelihood=False gives the latent function: the sample's noise is subtracted
        and the variance floored at 1e-6."""
        dev = self._x.device
        x_test = x_test.to(dev).float()
        if x_test.dim() == 2:
            x_test = x_test.unsqueeze(0)
        P, n_tot, _ = self.theta.shape
        m = x_test.shape[1]
        mean = torch.empty(P, n_tot, m, dtype=torch.float32, device=dev)
        var = torch.empty_like(mean)
        pp = torch.arange(P, device=dev).repeat_interleave(n_tot)
        ss = torch.arange(n_tot, device=dev).repeat(P)
        cap = _memory_cap(dev, self._x.shape[1], self._x.shape[2])
        for lo in range(0, P * n_tot, cap):
            p_, s_ = pp[lo:lo + cap], ss[lo:lo + cap]
            mu, v, _ = hipops.gp_fit_predict(self._x[p_].contiguous(), self._y[p_].contiguous(), self.theta[p_, s_].contiguous(), self._prior, self.kernel,
                                             x_test[p_].contiguous(), n_of=self._n_of[p_].contiguous())
            mean[p_, s_], var[p_, s_] = mu, v
        if not use_likelihood:
            var = (var - self.noise.unsqueeze(-1)).clamp_min(1e-6)
        return mean, var

    @torch.no_grad()
    def log_density(self, x_test, y_test, full_range=None, use_likelihood=True):
        """log of the posterior-predictive mixture density at y_test [P,m]: logsumexp over the samples of the normal log densities minus log N_tot, every
        component renormalised to `full_range` when given (reference get_mean_logdensity, :203-217).  Returns [P,m]."""
        mean, var = self.posterior(x_test, use_likelihood)
        y_test = y_test.to(mean.device).float().reshape(mean.shape[0], 1, -1)
        return _mixture_logdensity(mean, var, y_test, full_range, dim=1)


def _mixture_logdensity(mean, var, y, full_range, dim):
    sd = var.sqrt()
    logp = -0.5 * math.log(2 * math.pi) - sd.log() - 0.5 * ((y - mean) / sd) ** 2
    if full_range is not None:
        cdf = lambda v: 0.5 * (1. + torch.erf((float(v) - mean) / (sd * math.sqrt(2.))))
        logp = logp - torch.log(1. - (cdf(full_range[0]) + (1. - cdf(full_range[1]))))
    return torch.logsumexp(logp, dim) - math.log(mean.shape[dim])


@torch.no_grad()
def sample_hyperparameter_posterior(x, y, hyperparameters=None, n_of=None, num_samples=100, warmup_steps=300, num_chains=1, seed=0, kernel=None, init=None,
                                    chain_id_base=0, **nuts_kwargs):
    """NUTS over the log hyper-parameters of P independent GPs: x [P,S,F], y [P,S] on the GPU; problem p uses its first n_of[p] rows.  The potential is
    U(theta) = n J(theta) - sum_{k < F+2} theta_k: the negative unnormalised log posterior of the natural values (J is the MAP-II objective per point,
    `pfn_gp_mll_grad`) plus the Jacobian of the exp transform -- pyro samples in the same unconstrained space -- with the noise prior on
    noise = exp(eta) + floor; the constant mean stays at 0 as in the reference, whose NUTS samples only the parameters that have priors.  The chains of a
    problem are extra rows of the batch; chain j of problem p draws from Philox stream chain_id_base + p num_chains + j, so a sub-batch with the
    matching base reproduces its part of the full batch bit for bit.  init: theta [P,F+3] replacing `default_theta`.  nuts_kwargs go to
    mcmc.batched_nuts (step_size, target_accept, max_tree_depth, adapt_mass, sync_every).  Returns an `MCMCGP`."""
    if x.device.type != 'cuda':
        raise _hip.HipExtensionError(f'NUTS over the GP hyper-parameters runs on the GPU only (got device {x.device}); no CPU fallback')
    kernel, nu = _kernel_of(hyperparameters, kernel)
    dev = x.device
    P, S, F = x.shape
    K = int(num_chains)
    xp, yp = x.float(), y.float().reshape(P, S)
    n_of = torch.full((P,), S, dtype=torch.int32, device=dev) if n_of is None else torch.as_tensor(n_of, device=dev).to(torch.int32).clamp(1, S).contiguous()
    Sp = (S + 3) // 4 * 4
    if Sp != S:      # padded rows are masked through n_of: nothing in them is read
        xp = torch.cat([xp, xp.new_zeros(P, Sp - S, F)], 1)
        yp = torch.cat([yp, yp.new_zeros(P, Sp - S)], 1)
    xp, yp = xp.contiguous(), yp.contiguous()
    prior = hyperprior_vector(hyperparameters, dev)
    theta0 = default_theta(P, F, hyperparameters, dev) if init is None else torch.as_tensor(init, dtype=torch.float32, device=dev).reshape(P, F + 3).clone()
    theta0[:, F + 2] = 0.
    xc, yc, nc = xp.repeat_interleave(K, 0), yp.repeat_interleave(K, 0), n_of.repeat_interleave(K)
    ws = hipops.gp_fit_workspace(P * K, Sp, dev)

    def fun(theta):
        return hipops.gp_mll_grad(xc, yc, theta, prior, kernel, n_of=nc, flags=1, ws=ws)

    ids = int(chain_id_base) + torch.arange(P * K, dtype=torch.int64, device=dev)
    res = mcmc.batched_nuts(fun, theta0.repeat_interleave(K, 0), num_samples, warmup_steps, seed=seed, chain_ids=ids, scale=nc.float(),
                            shift=torch.ones(F + 2, device=dev), D=F + 2, **nuts_kwargs)
    theta = torch.zeros(P * K, num_samples, F + 3, dtype=torch.float32, device=dev)
    theta[..., :F + 2] = res['samples']
    return MCMCGP(xp, yp, n_of, theta.reshape(P, K * num_samples, F + 3), prior, kernel, nu, res['stats'].reshape(P, K, -1, 8), num_samples, res['evaluations'])


def get_mcmc_model(x, y, hyperparameters, device, num_samples, warmup_steps):
    """Reference :171-196: the model under `num_samples` NUTS draws of its hyper-parameters after `warmup_steps`, and its likelihood -- one object plays both
    parts, as in `get_fitted_model`.  x [n,F] or [P,n,F], y [n], [n,1] or [P,n]."""
    _reject_output_warping(hyperparameters)
    if torch.device(device).type != 'cuda':
        raise _hip.HipExtensionError(f'NUTS over the GP hyper-parameters runs on the GPU only (got device {device}); no CPU fallback')
    x = torch.as_tensor(x).to(device).float()
    x = x if x.dim() == 3 else x.unsqueeze(0)
    y = torch.as_tensor(y).to(device).float().reshape(x.shape[0], x.shape[1])
    model = sample_hyperparameter_posterior(x, y, hyperparameters, num_samples=num_samples, warmup_steps=warmup_steps)
    return model, model.likelihood


def get_mean_logdensity(dists, x, full_range=None):
    """Reference :203-217: the log of the equally weighted mixture of normals N(d.mean, d.variance) over every component of every object of `dists`, at the
    scalar x; with full_range = (lo, hi) every component is first renormalised to its mass inside the range."""
    means = torch.cat([d.mean.reshape(-1) for d in dists], 0)
    variances = torch.cat([d.variance.reshape(-1) for d in dists], 0)
    return _mixture_logdensity(means, variances, torch.as_tensor(x, dtype=means.dtype, device=means.device), full_range, dim=0)


@torch.no_grad()
def evaluate_(x, y, y_non_noisy, hyperparameters=None, device=default_device, num_samples=100, warmup_steps=300, full_range=None, min_seq_len=0,
              use_likelihood=False, seed=0):
    """The NUTS baseline (reference :220-268): for every t in range(max(min_seq_len, 1), T) and every dataset b, the hyper-parameters are sampled given rows
    [:t] of (x[:, b], y[:, b]) and the loss is minus the log of the mixture density of y[t, b] under the per-sample predictives (of the latent function
    unless use_likelihood).  x [T,B,F], y [T,B].  Returns the reference's triple: (mean loss per t as a tensor, with a leading 0. when min_seq_len == 0;
    seconds; the losses per t as a list of lists over b).  All (t, b) problems are batched in the 64-row buckets of `evaluate`; problem (t, b) draws from
    Philox stream index(t) B + b whatever the grouping."""
    import time
    start_time = time.time()
    _reject_output_warping(hyperparameters)
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _hip.HipExtensionError(f'NUTS over the GP hyper-parameters runs on the GPU only (got device {dev}); no CPU fallback')
    T, B, F = x.shape
    xb = x.to(dev).float().transpose(0, 1).contiguous()
    yb = y.to(dev).float().reshape(T, B).transpose(0, 1).contiguous()
    ts = list(range(max(min_seq_len, 1), T))
    losses = torch.zeros(len(ts), B, dtype=torch.float32, device=dev)
    buckets = {}
    for i, t in enumerate(ts):
        buckets.setdefault((t + 63) // 64 * 64, []).append(i)
    for Sb, members in sorted(buckets.items()):
        xs, ys = xb[:, :Sb], yb[:, :Sb]
        if Sb > T:
            xs = torch.cat([xs, xs.new_zeros(B, Sb - T, F)], 1)
            ys = torch.cat([ys, ys.new_zeros(B, Sb - T)], 1)
        cap = _memory_cap(dev, Sb, F)
        ii = torch.as_tensor([i for i in members for _ in range(B)], dtype=torch.long, device=dev)
        tt = torch.as_tensor([ts[i] for i in members for _ in range(B)], dtype=torch.long, device=dev)
        bb = torch.arange(B, device=dev).repeat(len(members))
        for lo in range(0, len(tt), cap):      # (a bucket's positions are consecutive, so its problems' stream indices are too)
            i_, t_, b_ = ii[lo:lo + cap], tt[lo:lo + cap], bb[lo:lo + cap]
            model = sample_hyperparameter_posterior(xs[b_], ys[b_], hyperparameters, n_of=t_, num_samples=num_samples, warmup_steps=warmup_steps, seed=seed,
                                                    chain_id_base=members[0] * B + lo)
            losses[i_, b_] = -model.log_density(xb[b_, t_].unsqueeze(1), yb[b_, t_].unsqueeze(1), full_range, use_likelihood)[:, 0]
    per_t = losses.mean(1)
    if min_seq_len == 0:
        per_t = torch.cat([per_t.new_zeros(1), per_t])
    torch.cuda.synchronize(dev)
    return per_t.to('cpu'), time.time() - start_time, losses.to('cpu').tolist()
