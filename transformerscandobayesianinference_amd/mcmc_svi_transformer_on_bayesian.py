"""The BNN study of the reference (mcmc_svi_transformer_on_bayesian.py): a PFN trained on a Bayesian-neural-network prior against NUTS and against stochastic
variational inference on the same BNN.

The reference builds the BNN as a PyroModule and runs pyro's NUTS on one dataset and one chain at a time (`eval_mcmc`, :249-267).  Here the model is a plain
class, its potential and gradient are ONE HIP launch for every chain of every dataset (`hipops.bnn_logp_grad`, csrc/bnn_mcmc.hip) and the sampler is
`mcmc.batched_nuts`, which advances all of them in the same pass; the posterior predictive is a second kernel (`hipops.bnn_predict`).

The reference's SVI arm (`eval_svi`, :211-246) fits pyro's AutoDiagonalNormal guide with Trace_ELBO and Adam, one dataset and one Python iteration per step.
Here the whole step loop of every dataset is one persistent launch (`hipops.bnn_svi_steps`, csrc/bnn_svi.hip, one block per dataset): `fit_bnn_svi` returns
a `BnnGuide`, `eval_svi` scores it through the same predictive kernel.  A guide has no limit on D, so SVI also runs the 'big' spec that NUTS refuses.

The reference's SVGD arm (`eval_svi(..., svgd=True)`: pyro's SVGD with RBFSteinKernel and 50 particles) is `eval_svgd` here: `fit_bnn_svgd` keeps N particles
per dataset and advances them by the Stein step (potential gradient, per-coordinate median bandwidth, kernel-weighted direction, Adam), again the whole step
loop of every dataset in one persistent launch (`hipops.bnn_svgd_steps`, csrc/bnn_svgd.hip); it returns `BnnParticles`, whose predictive is the particles
themselves.  `training_steps` / `training_samples` take the methods 'mcmc', 'svi' and 'svgd'.
Nothing depends on pyro.  DESIGN.md sections 16, 17 and 18 have the kernels; INTEGRATION.md lists what differs from the reference.

Not built: the plotting helpers."""
import math
import os
import time

import numpy as np
import torch
from torch import nn

from transformerscandobayesianinference_amd import encoders, hipops, mcmc, priors
from transformerscandobayesianinference_amd.train import Losses, train
from transformerscandobayesianinference_amd.utils import get_weighted_single_eval_pos_sampler

MAX_SAMPLED_DIM = 128      # mcmc.batched_nuts / pfn_nuts_advance: 1 <= D <= 128
SITES = ('fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias')      # pyro's site order of the reference's model = the layout of theta


def _activation_name(activation):
    name = {0: 'identity', 1: 'tanh'}.get(activation, activation)
    if name not in ('identity', 'tanh'):
        raise ValueError(f"activation {activation!r}: 'identity' (the reference's nn.Sequential(fc1, fc2)) or 'tanh'")
    return name


class BayesianModel:
    """fc1: num_features -> embed, fc2: embed -> 2, N(0, 1) on every weight and bias, y ~ Categorical(softmax(out)) (reference :28-67).  The reference's
    nn.Sequential(fc1, fc2) has no non-linearity: activation='identity' is that model, 'tanh' puts a tanh between the layers."""

    def __init__(self, model_spec, device='cuda', activation='identity'):
        self.model_spec = dict(model_spec)
        self.device = device
        self.activation = _activation_name(activation)
        self.num_features, self.embed = int(model_spec['num_features']), int(model_spec['embed'])
        self.params = None      # the weights of the last draw

    @property
    def shapes(self):
        F, H = self.num_features, self.embed
        return {'fc1.weight': (H, F), 'fc1.bias': (H,), 'fc2.weight': (2, H), 'fc2.bias': (2,)}

    @property
    def num_params(self):
        return hipops.bnn_num_params(self.num_features, self.embed)

    def pack(self, state):
        """{fc1.weight [.., H, F], fc1.bias [.., H], fc2.weight [.., 2, H], fc2.bias [.., 2]} -> theta [.., D]."""
        parts = []
        for name in SITES:
            t, shape = state[name], self.shapes[name]
            assert tuple(t.shape[t.dim() - len(shape):]) == shape, (name, tuple(t.shape), shape)
            parts.append(t.reshape(*t.shape[:t.dim() - len(shape)], -1))
        return torch.cat(parts, -1)

    def unpack(self, theta):
        """theta [.., D] -> the state-dict-like mapping of `pack`."""
        assert theta.shape[-1] == self.num_params, (tuple(theta.shape), self.num_params)
        out, at = {}, 0
        for name in SITES:
            shape = self.shapes[name]
            size = math.prod(shape)
            out[name] = theta[..., at:at + size].reshape(*theta.shape[:-1], *shape)
            at += size
        return out

    def logits(self, x, state):
        h = x @ state['fc1.weight'].transpose(-1, -2) + state['fc1.bias'].unsqueeze(-2)
        if self.activation == 'tanh':
            h = torch.tanh(h)
        return h @ state['fc2.weight'].transpose(-1, -2) + state['fc2.bias'].unsqueeze(-2)

    @torch.no_grad()
    def __call__(self, x=None, seq_len=1):
        """One draw from the prior: weights ~ N(0, 1), x [seq_len, F] ~ N(0, 1) unless given, obs ~ Categorical(softmax(out)).  Returns (x, obs [n] float)."""
        self.params = {name: torch.randn(*shape, device=self.device) for name, shape in self.shapes.items()}
        if x is None:
            x = torch.randn(seq_len, self.num_features, device=self.device)
        probs = torch.softmax(self.logits(x, self.params), -1)
        obs = torch.multinomial(probs, 1).squeeze(-1).float()
        return x, obs

    model = __call__      # `model(seq_len=n)`: what priors.pyro.get_batch and generate_toy_data call


def get_transformer_config(model_spec):
    return {'lr': 2.006434218345026e-05, 'epochs': 400, 'dropout': 0.0, 'emsize': 256, 'batch_size': 256, 'nlayers': 5, 'num_outputs': 1,
            'num_features': model_spec['num_features'], 'steps_per_epoch': 100, 'nhead': 4, 'seq_len': model_spec['seq_len'], 'nhid_factor': 2}


def get_model(model_generator, config, should_train=True, device='cuda'):
    """The PFN of the study: train() on priors.pyro.DataLoader with `model_generator` as the prior's model (reference :86-116)."""
    epochs = 0 if not should_train else config['epochs']
    return train(priors.pyro.DataLoader, Losses.bce, encoders.Linear, emsize=config['emsize'], nhead=config['nhead'], y_encoder_generator=encoders.Linear,
                 pos_encoder_generator=None, batch_size=config['batch_size'], nlayers=config['nlayers'], nhid=config['emsize'] * config['nhid_factor'], epochs=epochs,
                 warmup_epochs=config['epochs'] // 4, bptt=config['seq_len'], gpu_device=device, dropout=config['dropout'], steps_per_epoch=config['steps_per_epoch'],
                 single_eval_pos_gen=get_weighted_single_eval_pos_sampler(100),
                 extra_prior_kwargs_dict={'num_outputs': config['num_outputs'], 'num_features': config['num_features'], 'canonical_args': None, 'fuse_x_y': False,
                                          'model': model_generator},
                 lr=config['lr'], verbose=True)


def evaluate_preds(preds, y_test):
    """(accuracy, nll, mse) of sampled observations preds['obs'] [draws, m] (reference :130-139): the NLL is the BCE of the mean hard prediction."""
    preds_hard = preds['obs'] > 0.5
    acc = (preds_hard == y_test).float().mean()
    means = preds_hard.float().mean(axis=0)
    nll = nn.BCELoss()(means.float(), y_test.float())
    mse = Losses.mse(means, y_test).mean()
    return acc, nll, mse


def compute_mean_and_conf_interval(accuracies, confidence=.95):
    import scipy.stats as st
    accuracies = np.array(accuracies)
    n = len(accuracies)
    m, se = np.mean(accuracies), st.sem(accuracies)
    return m, se * st.t.ppf((1 + confidence) / 2., n - 1)


def generate_toy_data(model, bptt, device='cpu'):
    """100 datasets of `bptt` rows from the model's prior, seeded (reference :195-207).  Returns (X [100, bptt, F], y [100, bptt])."""
    torch.manual_seed(0)
    draws = [model(seq_len=bptt) for _ in range(100)]
    X, y = torch.stack([d[0] for d in draws], 0), torch.stack([d[1] for d in draws], 0)
    return X.to(device), y.to(device)


def get_default_model_spec(size):
    """'small' (F 3, H 5), 'big' (F 8, H 64) or '<features>_<embed>_<nlayers>'."""
    if size == 'big':
        num_features, embed, nlayers = 8, 64, 2
    elif size == 'small':
        num_features, embed, nlayers = 3, 5, 2
    else:
        num_features, embed, nlayers = (int(v) for v in size.split('_')[:3])
    return {'nlayers': nlayers, 'embed': embed, 'num_features': num_features, 'seq_len': 300}


def get_default_evaluation_points():
    return list(range(2, 100, 5))


def eval_transformer(X, y, device, model, training_samples_n):
    """The PFN on X [B, T, F], y [B, T] with the first `training_samples_n` rows as training set: (acc [B], nll [B], seconds) (reference :270-291).  x is
    standardised with the training rows' statistics before the model sees it, and all datasets go through the model in one call."""
    X_sample, y_sample = X.transpose(0, 1).to(device), y.transpose(0, 1).float().to(device)
    mean = X_sample[:training_samples_n].mean(0)
    std = X_sample[:training_samples_n].std(0) + .000001
    X_sample = (X_sample - mean) / std
    model = model.to(device)
    start = time.time()
    with torch.no_grad():
        output = model((X_sample, y_sample), single_eval_pos=training_samples_n).squeeze(-1)
    output = output.detach().float().cpu()
    elapsed = time.time() - start
    target = y_sample[training_samples_n:].cpu()
    acc = ((torch.sigmoid(output) > 0.5) == target.bool()).float().mean(axis=0)
    nll = nn.BCELoss(reduction='none')(torch.sigmoid(output), target).mean(axis=0)
    return acc, nll, elapsed


def _bnn_problem(x, y, model_spec, n_of, activation, max_dim=None):
    """The prologue of the three fits: x [P, S, F], y [P, S] as contiguous f32 on x's GPU, n_of as [P] int32 there (or None).  Returns
    (activation name, F, H, D, x, y, P, n_of).  A D above `max_dim` is refused first, with the limit named."""
    activation = _activation_name(activation)
    F, H = int(model_spec['num_features']), int(model_spec['embed'])
    D = hipops.bnn_num_params(F, H)
    if max_dim is not None and D > max_dim:
        raise ValueError(f'this BNN has D = H (F + 3) + 2 = {D} parameters; the batched sampler takes at most {max_dim} per chain '
                         f'(mcmc.batched_nuts), i.e. embed <= {(max_dim - 2) // (F + 3)} for num_features = {F}')
    hipops._hip.require_gpu_tensor(x, 'x')
    x, y = x.float().contiguous(), y.to(x.device).float().contiguous()
    P, S, _ = x.shape
    assert x.shape[2] == F and y.shape == (P, S)
    if n_of is not None:
        n_of = torch.as_tensor(n_of, dtype=torch.int32, device=x.device).contiguous()
    return activation, F, H, D, x, y, P, n_of


def _split(X, y, device, n):
    """X [P, T, F], y [P, T] on `device` as f32, split after the first n rows: (X_train, y_train, X_test, y_test), each contiguous."""
    X, y, n = X.to(device).float(), y.to(device).float(), int(n)
    return X[:, :n].contiguous(), y[:, :n].contiguous(), X[:, n:].contiguous(), y[:, n:].contiguous()


def _predictive(theta, x_test, spec, activation):
    """Class-1 probability of the parameter vectors theta [P, N, D] at x_test [P, m, F]: prob1 [P, N, m] (pfn_bnn_predict)."""
    P, N, D = theta.shape
    x_test = x_test.to(theta.device).float().contiguous()
    assert x_test.shape[0] == P and x_test.shape[2] == spec['num_features']
    return hipops.bnn_predict(x_test, theta.reshape(P * N, D).contiguous(), spec['embed'], K=N, activation=activation).view(P, N, x_test.shape[1])


class BnnPosterior:
    """NUTS draws of the BNN's weights for P problems: samples [P, K, N, D] in the layout of BayesianModel.pack, stats [P, K, W+N, 8] (mcmc.batched_nuts)."""

    def __init__(self, samples, stats, model_spec, activation, nuts):
        self.samples, self.stats, self.model_spec, self.activation, self.nuts = samples, stats, dict(model_spec), activation, nuts

    def predictive(self, x_test):
        """Class-1 probability of every draw at x_test [P, m, F]: prob1 [P, K N, m] (pfn_bnn_predict)."""
        P, K, N, D = self.samples.shape
        return _predictive(self.samples.reshape(P, K * N, D), x_test, self.model_spec, self.activation)


def sample_bnn_posterior(x, y, model_spec, n_of=None, num_samples=100, warmup_steps=100, num_chains=1, seed=0, activation='identity', **nuts_kwargs):
    """NUTS on the weights of the BNN given x [P, S, F], y [P, S] (class = y > 0.5; problem p uses its first n_of[p] rows, all when None): every one of the
    P num_chains chains advances in the same pass of mcmc.batched_nuts, one pfn_bnn_logp_grad launch per pass.  Start points ~ N(0, I) from `seed`.
    Returns a BnnPosterior."""
    activation, F, H, D, x, y, P, n_of = _bnn_problem(x, y, model_spec, n_of, activation, max_dim=MAX_SAMPLED_DIM)
    K = int(num_chains)
    theta0 = torch.randn(P * K, D, generator=torch.Generator(device=x.device).manual_seed(int(seed)), device=x.device)
    value = torch.empty(P * K, device=x.device)
    grad = torch.empty(P * K, D, device=x.device)

    def fun(theta):      # the sampler has consumed the previous pass's value / grad by the time it asks again: the two buffers are reused
        return hipops.bnn_logp_grad(x, y, theta, H, K=K, n_of=n_of, activation=activation, value=value, grad=grad)
    res = mcmc.batched_nuts(fun, theta0, num_samples, warmup_steps, seed=seed, **nuts_kwargs)
    N, T = res['samples'].shape[1], res['stats'].shape[1]
    return BnnPosterior(res['samples'].view(P, K, N, D), res['stats'].view(P, K, T, 8), model_spec, activation, res)


def _spec_of(model_spec):
    """A spec dict, or the reference's `model_sampler` (a callable returning a BayesianModel): -> (spec, activation)."""
    if callable(model_spec):
        model = model_spec()
        return model.model_spec, model.activation
    return model_spec, 'identity'


def _score(prob1, y_test, sample_obs, seed):
    """(nll [P], acc [P]) of the draws' class-1 probabilities prob1 [P, N, m] against y_test [P, m]: the mean probability, or the reference's estimator."""
    if sample_obs:
        obs = torch.bernoulli(prob1, generator=torch.Generator(device=prob1.device).manual_seed(int(seed)))
        acc, nll = zip(*[evaluate_preds({'obs': obs[p]}, y_test[p])[:2] for p in range(prob1.shape[0])])
        return torch.stack(nll).cpu().numpy(), torch.stack(acc).cpu().numpy()
    mean = prob1.mean(1)
    acc = ((mean > 0.5) == (y_test > 0.5)).float().mean(1)
    nll = nn.BCELoss(reduction='none')(mean, (y_test > 0.5).float()).mean(1)
    return nll.cpu().numpy(), acc.cpu().numpy()


def eval_mcmc(X, y, device, model_spec, training_samples_n, warmup_steps, num_pred_samples, sample_obs=False, seed=0):
    """NUTS on the BNN for every dataset of X [P, T, F], y [P, T] at once, trained on the first `training_samples_n` rows and scored on the rest: returns
    (nll [P], acc [P]) as numpy arrays (reference :249-267, one dataset at a time there).  By default the prediction is the mean class-1 probability over
    the draws (Rao-Blackwellised); sample_obs=True is the reference's estimator: Bernoulli observations per draw, the mean hard prediction, BCELoss."""
    spec, activation = _spec_of(model_spec)
    X_train, y_train, X_test, y_test = _split(X, y, device, training_samples_n)
    post = sample_bnn_posterior(X_train, y_train, spec, num_samples=num_pred_samples, warmup_steps=warmup_steps, num_chains=1, seed=seed, activation=activation)
    prob1 = post.predictive(X_test)      # [P, N, m]
    return _score(prob1, y_test, sample_obs, seed)


class BnnGuide:
    """Mean-field Gaussian guides of P problems (fit_bnn_svi): loc, scale [P, D] in the layout of BayesianModel.pack, losses [P, T] (the ELBO loss of every
    step, before its update), state [P, 6, D] (hipops.bnn_svi_state: what a further hipops.bnn_svi_steps call continues from)."""

    def __init__(self, state, losses, model_spec, activation):
        self.state, self.losses, self.model_spec, self.activation = state, losses, dict(model_spec), activation
        self.loc, self.scale = state[:, 0], torch.nn.functional.softplus(state[:, 1])

    def sample(self, num_samples, seed=0):
        """theta [P, N, D] ~ N(loc, diag(scale^2)), seeded."""
        P, D = self.loc.shape
        z = torch.randn(P, int(num_samples), D, generator=torch.Generator(device=self.loc.device).manual_seed(int(seed)), device=self.loc.device)
        return self.loc[:, None, :] + self.scale[:, None, :] * z

    def predictive(self, x_test, num_samples, seed=0):
        """Class-1 probability of `num_samples` draws from the guide at x_test [P, m, F]: prob1 [P, N, m] (pfn_bnn_predict)."""
        return _predictive(self.sample(int(num_samples), seed), x_test, self.model_spec, self.activation)


def fit_bnn_svi(x, y, model_spec, n_of=None, num_steps=1024, lr=1e-3, num_particles=1, seed=0, activation='identity', init_scale=0.1, steps_per_launch=256):
    """SVI on the weights of the BNN given x [P, S, F], y [P, S] (class = y > 0.5; problem p uses its first n_of[p] rows, all when None): a mean-field
    Gaussian guide per problem, `num_steps` Adam steps on the `num_particles`-particle ELBO, every problem in the same launches (hipops.bnn_svi_steps).
    The initial loc is the median of 15 N(0, 1) draws per coordinate from `seed` (pyro's init_to_median for this prior), the initial scale `init_scale`.
    `steps_per_launch` only bounds the length of one launch: the result does not depend on it, bit for bit.  Returns a BnnGuide."""
    activation, F, H, D, x, y, P, n_of = _bnn_problem(x, y, model_spec, n_of, activation)
    num_steps, per = int(num_steps), max(int(steps_per_launch), 1)
    loc0 = torch.randn(15, P, D, generator=torch.Generator(device=x.device).manual_seed(int(seed)), device=x.device).median(0).values
    state = hipops.bnn_svi_state(P, F, H, x.device, loc0=loc0, init_scale=init_scale)
    losses = torch.empty(P, num_steps, device=x.device)
    for step0 in range(0, num_steps, per):
        n = min(per, num_steps - step0)
        losses[:, step0:step0 + n] = hipops.bnn_svi_steps(x, y, state, H, n, step0=step0, num_particles=num_particles, lr=lr, seed=seed, n_of=n_of, activation=activation)
    return BnnGuide(state, losses, model_spec, activation)


def _require_gpu(device, what, kernel='the ELBO step kernel (pfn_bnn_svi_steps) runs on the GPU only and there is no CPU fallback'):
    if torch.device(device).type != 'cuda':
        raise NotImplementedError(f'{what}: {kernel}; got device {device!r}')


def eval_svi(X, y, device, model_sampler, training_samples_n, num_train_steps, num_pred_samples, lr=1e-3, num_particles=1, svgd=False, sample_obs=False, seed=0):
    """SVI on the BNN for every dataset of X [P, T, F], y [P, T] at once, trained on the first `training_samples_n` rows and scored on the rest with
    `num_pred_samples` draws from the guide: returns (nll [P], acc [P]) as numpy arrays (reference :211-246, one dataset and one step at a time there).
    `model_sampler`: a spec dict or the reference's callable.  The estimators are eval_mcmc's: the mean class-1 probability by default, sample_obs=True for
    the reference's sampled observations."""
    if svgd:
        raise NotImplementedError('svgd=True: eval_svi fits the ELBO guide only; the Stein-kernel particle step is eval_svgd(X, y, device, model_sampler, '
                                  'training_samples_n, num_train_steps)')
    _require_gpu(device, 'eval_svi')
    spec, activation = _spec_of(model_sampler)
    X_train, y_train, X_test, y_test = _split(X, y, device, training_samples_n)
    guide = fit_bnn_svi(X_train, y_train, spec, num_steps=num_train_steps, lr=lr, num_particles=num_particles, seed=seed, activation=activation)
    prob1 = guide.predictive(X_test, num_pred_samples, seed=seed)      # [P, N, m]
    return _score(prob1, y_test, sample_obs, seed)


class BnnParticles:
    """Stein particles of the BNN's weights for P problems (fit_bnn_svgd): particles [P, N, D] in the layout of BayesianModel.pack, potentials [P, T] (the mean
    over particles of U before every step's update), state [P, 3, N, D] (hipops.bnn_svgd_state: what a further hipops.bnn_svgd_steps call continues from)."""

    def __init__(self, state, potentials, model_spec, activation):
        self.state, self.potentials, self.model_spec, self.activation = state, potentials, dict(model_spec), activation
        self.particles = state[:, 0]

    def predictive(self, x_test):
        """Class-1 probability of every particle at x_test [P, m, F]: prob1 [P, N, m] (pfn_bnn_predict)."""
        return _predictive(self.particles, x_test, self.model_spec, self.activation)


def fit_bnn_svgd(x, y, model_spec, n_of=None, num_steps=1024, lr=1e-3, num_particles=50, seed=0, activation='identity', bandwidth_factor=1.0, steps_per_launch=256):
    """SVGD on the weights of the BNN given x [P, S, F], y [P, S] (class = y > 0.5; problem p uses its first n_of[p] rows, all when None): `num_particles`
    particles per problem, `num_steps` Stein steps with Adam, every problem in the same launches (hipops.bnn_svgd_steps).  Every coordinate of every initial
    particle is the median of 15 N(0, 1) draws from `seed` (pyro's init_to_median under the particle plate).  `steps_per_launch` only bounds the length of one
    launch: the result does not depend on it, bit for bit.  Returns BnnParticles."""
    activation, F, H, D, x, y, P, n_of = _bnn_problem(x, y, model_spec, n_of, activation)
    N, num_steps, per = int(num_particles), int(num_steps), max(int(steps_per_launch), 1)
    draws = torch.randn(15, P, N, D, generator=torch.Generator().manual_seed(int(seed)))      # on the host: the start does not depend on the device
    state = hipops.bnn_svgd_state(P, N, F, H, x.device, particles0=draws.median(0).values)
    potentials = torch.empty(P, num_steps, device=x.device)
    for step0 in range(0, num_steps, per):
        n = min(per, num_steps - step0)
        potentials[:, step0:step0 + n] = hipops.bnn_svgd_steps(x, y, state, H, n, step0=step0, lr=lr, bandwidth_factor=bandwidth_factor, n_of=n_of, activation=activation)[0]
    return BnnParticles(state, potentials, model_spec, activation)


def eval_svgd(X, y, device, model_sampler, training_samples_n, num_train_steps, num_pred_samples=None, lr=1e-3, num_particles=50, sample_obs=False, seed=0):
    """SVGD on the BNN for every dataset of X [P, T, F], y [P, T] at once, trained on the first `training_samples_n` rows and scored on the rest with the
    particles themselves: returns (nll [P], acc [P]) as numpy arrays (the reference's eval_svi(..., svgd=True), :211-246, which scores the untrained guide
    instead).  `num_pred_samples` is accepted for signature parity and ignored: the predictive is the `num_particles` particles.  The estimators are
    eval_mcmc's: the mean class-1 probability by default, sample_obs=True for the reference's sampled observations."""
    _require_gpu(device, 'eval_svgd', 'the Stein step kernel (pfn_bnn_svgd_steps) runs on the GPU only, like the ELBO step kernel; no CPU fallback')
    spec, activation = _spec_of(model_sampler)
    X_train, y_train, X_test, y_test = _split(X, y, device, training_samples_n)
    fit = fit_bnn_svgd(X_train, y_train, spec, num_steps=num_train_steps, lr=lr, num_particles=num_particles, seed=seed, activation=activation)
    return _score(fit.predictive(X_test), y_test, sample_obs, seed)


def _eval(method, X, y, device, model_spec, training_samples_n, steps):
    if method == 'mcmc':
        return eval_mcmc(X, y, device, model_spec, training_samples_n, warmup_steps=steps, num_pred_samples=steps)
    if method == 'svi':
        return eval_svi(X, y, device, model_spec, training_samples_n, num_train_steps=steps, num_pred_samples=steps)
    if method == 'svgd':
        raise NotImplementedError("method 'svgd': SVGD is not built here -- it needs a Stein-kernel particle step beside the ELBO kernel; 'mcmc' (NUTS through "
                                  "mcmc.batched_nuts) and 'svi' (pfn_bnn_svi_steps) are available")
    raise ValueError(f'unknown method {method!r}')


def training_steps(method, X, y, model_spec, device='cuda', path_interfix='', overwrite=False):
    """NLL / accuracy / seconds at 100 training rows for 2 .. 4096 warmup transitions and as many draws; one results_{method}_training_steps_{s}.npy each."""
    training_samples_n = 100
    for s in [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]:
        path = f'{path_interfix}/results_{method}_training_steps_{s}.npy'
        if os.path.isfile(path) and not overwrite:
            print(f'already done {s}')
            continue
        start = time.time()
        if method == 'svgd':
            nll, acc = eval_svgd(X, y, device, model_spec, training_samples_n, num_train_steps=s)
        else:
            nll, acc = _eval(method, X, y, device, model_spec, training_samples_n, s)
        elapsed = time.time() - start
        print(s)
        print('NLL ', compute_mean_and_conf_interval(nll))
        print('ACC ', compute_mean_and_conf_interval(acc))
        print('TIME ', elapsed)
        with open(path, 'wb') as f:
            np.save(f, np.array((np.array(nll), np.array(acc), elapsed), dtype=object))
        print(f'Saved results at {path}')


def training_samples(method, X, y, model_spec, evaluation_points, steps=None, device='cuda', path_interfix='', overwrite=False):
    """The same at a fixed number of transitions (512 for NUTS, 1024 steps for SVI and SVGD) for every training-set size of `evaluation_points`."""
    num_pred_samples = steps if steps else (1024 if method in ('svi', 'svgd') else 512)
    for training_samples_n in evaluation_points:
        path = f'{path_interfix}/results_{method}_{num_pred_samples}_training_samples_{training_samples_n}.npy'
        if os.path.isfile(path) and not overwrite:
            print(f'already done {training_samples_n}')
            continue
        start = time.time()
        if method == 'svgd':
            nll, acc = eval_svgd(X, y, device, model_spec, training_samples_n, num_train_steps=num_pred_samples)
        else:
            nll, acc = _eval(method, X, y, device, model_spec, training_samples_n, num_pred_samples)
        elapsed = time.time() - start
        print('NLL ', compute_mean_and_conf_interval(nll))
        print('ACC ', compute_mean_and_conf_interval(acc))
        print('TIME ', elapsed)
        with open(path, 'wb') as f:
            np.save(f, np.array((training_samples_n, np.array(nll), np.array(acc), elapsed), dtype=object))
