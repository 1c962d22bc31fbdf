"""Host-side checks of the BNN posterior target (csrc/bnn_mcmc.hip, mcmc_svi_transformer_on_bayesian.py, priors/pyro.py): the C ABI, the f64 restatement
(tests/bnn_f64.py) verified against central finite differences BEFORE the GPU tests use it as their oracle, the parameter layout, the error paths that
must answer without a GPU, the prior from a user-defined model, and the compat names.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnn_f64 as ref      # noqa: E402

from transformerscandobayesianinference_amd import _hip, hipops      # noqa: E402
from transformerscandobayesianinference_amd import mcmc_svi_transformer_on_bayesian as study      # noqa: E402
from transformerscandobayesianinference_amd.priors import pyro as pyro_prior      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pfn_bnn_logp_grad', 'pfn_bnn_predict')
PFN_ERR_UNSUPPORTED, PFN_ERR_ARGUMENT = -1, -4


def test_the_two_symbols_are_declared_exported_and_bound_at_abi_10():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    lib = _hip.lib()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert _hip.ABI_VERSION == 10 and lib.pfn_abi_version() == 10 and '#define PFN_ABI_VERSION 10' in header
    build = open(os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc', 'build.sh')).read()
    assert 'bnn_mcmc.hip' in build and '../_build/bnn_mcmc.o' in build      # compiled and linked


@pytest.mark.parametrize('activation', ['identity', 'tanh'])
def test_f64_value_and_gradient_agree_with_central_differences(activation):
    F, H, S, n = 3, 5, 12, 9
    g = torch.Generator().manual_seed(5)
    x = torch.randn(S, F, generator=g, dtype=torch.float64)
    y = (torch.rand(S, generator=g) > 0.5).double()
    D = ref.num_params(F, H)
    theta = torch.randn(D, generator=g, dtype=torch.float64)
    U, grad = ref.value_and_grad(theta, x, y, n, F, H, activation)
    # the value, term by term
    W1, b1, W2, b2 = ref.unpack(theta, F, H)
    want = 0.5 * float((theta ** 2).sum()) + 0.5 * D * np.log(2 * np.pi)
    for i in range(n):
        h = W1 @ x[i] + b1
        o = W2 @ (torch.tanh(h) if activation == 'tanh' else h) + b2
        want -= float(o[int(y[i])] - torch.logsumexp(o, 0))
    assert abs(U - want) < 1e-12 * abs(want)
    eps = 1e-6
    fd = torch.empty(D, dtype=torch.float64)
    for k in range(D):
        e = torch.zeros(D, dtype=torch.float64)
        e[k] = eps
        fd[k] = (float(ref.potential(theta + e, x, y, n, F, H, activation)) - float(ref.potential(theta - e, x, y, n, F, H, activation))) / (2 * eps)
    assert float((fd - grad).abs().max()) < 1e-7 * float(grad.abs().max())
    # rows >= n and entries >= D take no part; n = 0 is the prior
    x2, y2 = x.clone(), y.clone()
    x2[n:], y2[n:] = float('nan'), float('nan')
    assert ref.value_and_grad(torch.cat([theta, torch.full((3,), float('nan'), dtype=torch.float64)]), x2, y2, n, F, H, activation)[0] == U
    U0, g0 = ref.value_and_grad(theta, x, y, 0, F, H, activation)
    assert abs(U0 - (0.5 * float((theta ** 2).sum()) + 0.5 * D * np.log(2 * np.pi))) < 1e-12 and torch.equal(g0, theta)
    # the predictive is softmax(o)[1]
    p = ref.predict(theta, x, F, H, activation)
    o = ref.logits(theta, x, F, H, activation)
    assert torch.allclose(p, 1. / (1. + torch.exp(o[:, 0] - o[:, 1])), rtol=1e-13, atol=0)


def test_pack_and_unpack_follow_pyros_site_order():
    spec = dict(num_features=3, embed=5)
    model = study.BayesianModel(spec, device='cpu', activation='tanh')
    F, H = 3, 5
    assert model.num_params == ref.num_params(F, H) == hipops.bnn_num_params(F, H) == 32
    assert hipops.bnn_num_params(8, 64) == 706 and hipops.bnn_num_params(1, 1) == 6 and hipops.bnn_num_params(16, 64) == 1218
    theta = torch.arange(2 * 32, dtype=torch.float32).reshape(2, 32)
    state = model.unpack(theta)
    assert list(state) == ['fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias']
    assert state['fc1.weight'].shape == (2, 5, 3) and state['fc1.bias'].shape == (2, 5) and state['fc2.weight'].shape == (2, 2, 5) and state['fc2.bias'].shape == (2, 2)
    assert state['fc1.weight'][0, 1, 2] == 1 * 3 + 2 and state['fc1.bias'][0, 4] == 15 + 4 and state['fc2.weight'][0, 1, 0] == 20 + 5 and state['fc2.bias'][1, 1] == 32 + 31
    assert torch.equal(model.pack(state), theta)
    W1, b1, W2, b2 = ref.unpack(theta[0].double(), F, H)      # the oracle reads the same layout
    assert torch.equal(W1.float(), state['fc1.weight'][0]) and torch.equal(b1.float(), state['fc1.bias'][0])
    assert torch.equal(W2.float(), state['fc2.weight'][0]) and torch.equal(b2.float(), state['fc2.bias'][0])
    # a draw from the prior: shapes, classes, the recorded weights reproduce the logits' layout
    torch.manual_seed(1)
    x, obs = model.model(seq_len=7)
    assert x.shape == (7, 3) and obs.shape == (7,) and set(obs.tolist()) <= {0., 1.}
    t = model.pack(model.params)
    assert torch.allclose(model.logits(x, model.params).double(), ref.logits(t.double(), x.double(), F, H, 'tanh'), atol=1e-5)
    with pytest.raises(ValueError):
        study.BayesianModel(spec, device='cpu', activation='relu')


def test_out_of_range_shapes_are_refused_without_a_gpu():
    lib = _hip.lib()
    buf = torch.zeros(4096)      # host memory: a refused call never looks at it
    p = buf.data_ptr()
    grad = lambda P, K, S, F, H, act=0, ld=2048: lib.pfn_bnn_logp_grad(p, p, 0, p, ld, P, K, S, F, H, act, p, p, 0)
    pred = lambda P, K, m, F, H, act=0, ld=2048: lib.pfn_bnn_predict(p, p, ld, P, K, m, F, H, act, p, 0)
    for F, H in ((0, 5), (17, 5), (3, 0), (3, 65), (-1, 5)):
        assert grad(1, 1, 4, F, H) == PFN_ERR_UNSUPPORTED, (F, H)
        assert pred(1, 1, 4, F, H) == PFN_ERR_UNSUPPORTED, (F, H)
        assert lib.pfn_last_error_string()
    assert grad(1, 1, 4, 3, 5, act=2) == PFN_ERR_UNSUPPORTED and pred(1, 1, 4, 3, 5, act=-1) == PFN_ERR_UNSUPPORTED
    for P, K in ((0, 1), (1, 0), (-3, 2), (65536, 65536)):
        assert grad(P, K, 4, 3, 5) == PFN_ERR_ARGUMENT, (P, K)
        assert pred(P, K, 4, 3, 5) == PFN_ERR_ARGUMENT, (P, K)
    assert grad(1, 1, 0, 3, 5) == PFN_ERR_ARGUMENT and pred(1, 1, -1, 3, 5) == PFN_ERR_ARGUMENT      # S >= 1, m >= 0
    assert grad(1, 1, 4, 3, 5, ld=31) == PFN_ERR_ARGUMENT and pred(1, 1, 4, 3, 5, ld=31) == PFN_ERR_ARGUMENT      # ld >= D = 32
    assert lib.pfn_bnn_logp_grad(0, p, 0, p, 32, 1, 1, 4, 3, 5, 0, p, p, 0) == PFN_ERR_ARGUMENT      # NULL x
    assert lib.pfn_bnn_logp_grad(p, p, 0, p, 32, 1, 1, 4, 3, 5, 0, 0, p, 0) == PFN_ERR_ARGUMENT      # NULL value
    assert lib.pfn_bnn_predict(p, 0, 32, 1, 1, 4, 3, 5, 0, p, 0) == PFN_ERR_ARGUMENT      # NULL theta
    assert b'F 17' in [grad(1, 1, 4, 17, 5), lib.pfn_last_error_string()][1]      # the message names what was wrong


class StandIn:
    """A CPU stand-in for a generative model: dataset d of model k is x = k + d-th ramp, y = its row sums' sign."""
    made = 0

    def __init__(self):
        StandIn.made += 1
        self.k, self.calls = StandIn.made, 0

    def __call__(self, seq_len=1):
        self.calls += 1
        x = torch.arange(seq_len * 2, dtype=torch.float32).reshape(seq_len, 2) ** 1.5 * self.calls + self.k
        x[:, 1] = -x[:, 1] * (1 + torch.arange(seq_len) % 3)
        return x, (x.sum(1) > -20).float()


def test_pyro_prior_get_batch_with_a_stand_in_model():
    StandIn.made = 0
    T, B = 6, 8
    x, y, target = pyro_prior.get_batch(B, T, batch_size_per_gp_sample=4, model=StandIn, num_features=2, num_outputs=1, canonical_args=None)
    assert StandIn.made == 2      # B / batch_size_per_gp_sample models, 4 datasets from each
    assert x.shape == (T, B, 2) and y.shape == (T, B) and target is y
    StandIn.made = 0
    raw, ys = [], []
    for _ in range(2):
        m = StandIn()
        for _ in range(4):
            xi, yi = m(seq_len=T)
            raw.append(xi)
            ys.append(yi)
    raw = torch.stack(raw, 1)
    assert torch.equal(x, (raw - raw.mean(0)) / (raw.std(0) + .000001)) and torch.equal(y, torch.stack(ys, 1))
    assert float(x.mean(0).abs().max()) < 1e-5 and float((x.std(0) - 1).abs().max()) < 1e-4
    # default: 16 datasets per model ... and the divisibility the reference asserts
    StandIn.made = 0
    assert pyro_prior.get_batch(32, 3, model=StandIn)[0].shape == (3, 32, 2) and StandIn.made == 16
    with pytest.raises(AssertionError):
        pyro_prior.get_batch(10, 3, batch_size_per_gp_sample=4, model=StandIn)
    assert pyro_prior.DataLoader.num_outputs == 1
    dl = pyro_prior.DataLoader(num_steps=2, batch_size=4, seq_len=5, batch_size_per_gp_sample=2, model=StandIn, num_features=2)
    (bx, by), bt = next(iter(dl))
    assert bx.shape == (5, 4, 2) and by.shape == (5, 4) and len(dl) == 2 and dl.num_features == 2


def test_compat_exposes_the_new_modules():
    from transformerscandobayesianinference_amd import compat
    saved = dict(sys.modules)
    try:
        compat.install()
        import mcmc_svi_transformer_on_bayesian as top
        import priors
        import priors.pyro as pp
        assert top is study and pp is pyro_prior and priors.pyro is pyro_prior
        for name in ('BayesianModel', 'generate_toy_data', 'get_default_model_spec', 'get_default_evaluation_points', 'get_transformer_config', 'get_model', 'eval_transformer',
                     'eval_mcmc', 'evaluate_preds', 'compute_mean_and_conf_interval', 'sample_bnn_posterior', 'training_steps', 'training_samples'):
            assert callable(getattr(top, name)), name
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)


def test_the_study_helpers_keep_the_references_values():
    assert study.get_default_model_spec('small') == {'nlayers': 2, 'embed': 5, 'num_features': 3, 'seq_len': 300}
    assert study.get_default_model_spec('big') == {'nlayers': 2, 'embed': 64, 'num_features': 8, 'seq_len': 300}
    assert study.get_default_model_spec('4_7_3') == {'nlayers': 3, 'embed': 7, 'num_features': 4, 'seq_len': 300}
    assert study.get_default_evaluation_points() == list(range(2, 100, 5)) and len(study.get_default_evaluation_points()) == 20
    cfg = study.get_transformer_config(study.get_default_model_spec('small'))
    assert (cfg['emsize'], cfg['nlayers'], cfg['nhead'], cfg['batch_size'], cfg['seq_len'], cfg['num_features'], cfg['epochs']) == (256, 5, 4, 256, 300, 3, 400)
    model = study.BayesianModel(study.get_default_model_spec('small'), device='cpu')
    X, y = study.generate_toy_data(model, 12)
    assert X.shape == (100, 12, 3) and y.shape == (100, 12) and set(y.unique().tolist()) <= {0., 1.}
    X2, y2 = study.generate_toy_data(model, 12)
    assert torch.equal(X, X2) and torch.equal(y, y2)      # seeded
    # evaluate_preds: hard predictions, their mean, BCE of the mean
    obs = torch.tensor([[1., 0., 1.], [1., 0., 0.], [1., 1., 0.], [1., 0., 1.]])
    acc, nll, mse = study.evaluate_preds({'obs': obs}, torch.tensor([1., 0., 1.]))
    assert abs(float(acc) - 9 / 12) < 1e-6
    assert abs(float(nll) - float(-(np.log(1.) + np.log(1 - .25) + np.log(.5)) / 3)) < 1e-6 and abs(float(mse) - (0 + .0625 + .25) / 3) < 1e-6
    m, h = study.compute_mean_and_conf_interval([1., 2., 3., 4.])
    assert abs(m - 2.5) < 1e-12 and abs(h - 3.182446305284263 * np.std([1., 2., 3., 4.], ddof=1) / 2) < 1e-9
    for method in ('svi', 'svgd'):
        with pytest.raises(NotImplementedError, match='ELBO'):
            study.training_steps(method, X, y, study.get_default_model_spec('small'), device='cpu', path_interfix='/nonexistent')


def test_the_big_spec_is_refused_by_the_sampler_with_the_limit_named():
    spec = study.get_default_model_spec('big')
    with pytest.raises(ValueError) as e:
        study.sample_bnn_posterior(torch.zeros(1, 4, 8), torch.zeros(1, 4), spec)
    msg = str(e.value)
    assert '706' in msg and '128' in msg and 'embed <= 11' in msg      # H = 11 is the largest that fits for F = 8: 11 * 11 + 2 = 123
    assert hipops.bnn_num_params(8, 11) <= 128 < hipops.bnn_num_params(8, 12)
