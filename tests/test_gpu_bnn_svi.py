"""SVI on the BNN on the device (csrc/bnn_svi.hip: pfn_bnn_svi_steps) and what is built on it (mcmc_svi_transformer_on_bayesian.fit_bnn_svi / BnnGuide /
eval_svi) against the f64 restatement (tests/bnn_svi_f64.py, verified on the host in tests/test_host_bnn_svi.py against central differences and
torch.optim.Adam), which draws the kernel's own Philox noise.

Bounds on continuous outputs: <= 2 x the value measured on the MI355X (profiles/r14_bnn_svi_bounds_measured.json), and never above 1e-3.  Gradients, loc and
scale are compared relative to their norms, a one-step loss relative to |L|, the losses of a trajectory relative to max(1, |L|).  The invariants of the
contract (a problem alone and in a batch, a run split over launches, untouched tails, a non-finite neighbour) are compared bit for bit."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnn_f64 as ref      # noqa: E402
import bnn_svi_f64 as svi      # noqa: E402
import bounds      # noqa: E402

from transformerscandobayesianinference_amd import hipops      # noqa: E402
from transformerscandobayesianinference_amd import mcmc_svi_transformer_on_bayesian as study      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CAP = 1e-3
S = 100
BETA1 = float(np.float32(1) - np.float32(0.9))      # the kernel's 1 - beta1

# One step, P = 3: label -> (H, F, K, activation, n_of).  Every instantiation of the kernel: Hp 8 (H 1 / 5 / 8), Hp 16 (H 9 / 16), Hp 32 (H 17 / 32) and Hp 64
# (H 33 / 64), each with Fp 4 / 8 / 16 (F 1 / 3, 5 / 8, 16) and both activations; n of {0, 1, 63, 64, 65, 100} ragged over the problems; K of {1, 3} and one
# more than a block holds (33 at Hp 8, 17 at Hp 16, 9 at Hp 32, 5 at Hp 64: the round loop, with a single particle in the second round).
ONE_STEP = {
    'H1_F1_i': (1, 1, 1, 'identity', (100, 0, 1)),
    'H5_F3_t': (5, 3, 3, 'tanh', (0, 63, 100)),
    'H8_F8_i': (8, 8, 33, 'identity', (1, 64, 65)),
    'H5_F5_t': (5, 5, 33, 'tanh', (65, 100, 0)),
    'H8_F16_i': (8, 16, 3, 'identity', (63, 64, 1)),
    'H1_F16_t': (1, 16, 1, 'tanh', (100, 65, 63)),
    'H9_F3_i': (9, 3, 17, 'identity', (64, 0, 100)),
    'H16_F1_t': (16, 1, 1, 'tanh', (1, 65, 63)),
    'H16_F8_i': (16, 8, 3, 'identity', (100, 63, 0)),
    'H9_F5_t': (9, 5, 3, 'tanh', (65, 1, 64)),
    'H16_F16_i': (16, 16, 1, 'identity', (0, 100, 65)),
    'H9_F16_t': (9, 16, 17, 'tanh', (63, 64, 100)),
    'H17_F3_i': (17, 3, 3, 'identity', (1, 100, 64)),
    'H32_F1_t': (32, 1, 9, 'tanh', (65, 0, 63)),
    'H17_F8_i': (17, 8, 9, 'identity', (100, 1, 65)),
    'H32_F5_t': (32, 5, 1, 'tanh', (64, 63, 0)),
    'H32_F16_i': (32, 16, 1, 'identity', (63, 65, 100)),
    'H17_F16_t': (17, 16, 9, 'tanh', (0, 64, 1)),
    'H33_F3_i': (33, 3, 5, 'identity', (100, 64, 0)),
    'H64_F1_t': (64, 1, 3, 'tanh', (63, 1, 65)),
    'H64_F8_i': (64, 8, 1, 'identity', (65, 100, 63)),
    'H33_F8_t': (33, 8, 5, 'tanh', (1, 0, 64)),
    'H33_F16_i': (33, 16, 3, 'identity', (64, 65, 1)),
    'H64_F16_t': (64, 16, 5, 'tanh', (100, 63, 0)),
}
# measured on the MI355X (profiles/r14_bnn_svi_bounds_measured.json): (g_loc, g_u, loss), each <= 2 x measured
ONE_STEP_BOUNDS = {
    'H17_F3_i': (2.4e-7, 4.4e-7, 1.5e-7),
    'H32_F1_t': (2.4e-7, 3.5e-7, 8.9e-8),
    'H17_F8_i': (5.5e-7, 4.1e-7, 1.0e-7),
    'H32_F5_t': (4.4e-7, 4.3e-7, 2.2e-7),
    'H32_F16_i': (8.1e-7, 8.5e-7, 9.6e-8),
    'H17_F16_t': (2.3e-7, 3.5e-7, 1.5e-7),
    'H33_F3_i': (3.2e-7, 4.9e-7, 1.3e-7),
    'H33_F8_t': (3.1e-7, 4.3e-7, 6.0e-8),
    'H33_F16_i': (4.5e-7, 6.8e-7, 2.0e-7),
    'H1_F1_i': (2.7e-7, 3.4e-7, 2.8e-7),
    'H5_F3_t': (3.8e-7, 4.3e-7, 3.3e-7),
    'H8_F8_i': (1.4e-7, 3.7e-7, 1.0e-7),
    'H5_F5_t': (1.9e-7, 3.0e-7, 1.0e-7),
    'H8_F16_i': (5.6e-7, 7.2e-7, 1.7e-7),
    'H1_F16_t': (5.6e-7, 6.6e-7, 3.7e-7),
    'H9_F3_i': (3.0e-7, 4.3e-7, 1.3e-7),
    'H16_F1_t': (2.2e-7, 4.7e-7, 2.8e-7),
    'H16_F8_i': (2.8e-7, 5.5e-7, 2.5e-7),
    'H9_F5_t': (3.2e-7, 3.2e-7, 3.1e-7),
    'H16_F16_i': (3.3e-7, 5.0e-7, 2.5e-7),
    'H9_F16_t': (2.2e-7, 3.1e-7, 1.8e-7),
    'H64_F1_t': (2.4e-7, 4.2e-7, 1.9e-7),
    'H64_F8_i': (5.1e-7, 6.8e-7, 1.7e-7),
    'H64_F16_t': (3.2e-7, 4.4e-7, 1.9e-7),
}
TRAJECTORY_BOUNDS = {0.001: (3.5e-7, 2.6e-7, 6.2e-7), 0.05: (5.0e-7, 1.4e-7, 1.7e-6)}      # by lr: (loc, scale, loss)
CHUNKED_BOUNDS = (7.3e-8, 4.8e-8, 1.1e-6)      # (loc, scale, loss)
HP_OF = lambda H: 8 if H <= 8 else 16 if H <= 16 else 32 if H <= 32 else 64      # launch_bnn_svi_steps' dispatch
FP_OF = lambda F: 4 if F <= 4 else 8 if F <= 8 else 16
assert {(HP_OF(c[0]), FP_OF(c[1]), c[3]) for c in ONE_STEP.values()} == {(hp, fp, act) for hp in (8, 16, 32, 64) for fp in (4, 8, 16) for act in ('identity', 'tanh')}
assert all(any(HP_OF(c[0]) == hp and c[2] == 256 // hp + 1 for c in ONE_STEP.values()) for hp in (8, 16, 32, 64))      # one more particle than a block holds
assert all(b <= CAP for v in list(ONE_STEP_BOUNDS.values()) + list(TRAJECTORY_BOUNDS.values()) + [CHUNKED_BOUNDS] for b in v)


def problem(H, F, P, seed, rows=S):
    """x [P,rows,F], y [P,rows] in {0, 1}, state [P, 6, D] with loc ~ N(0, 1), u ~ N(-1, 0.5) and zero moments, all f32 (the f64 side reads the same numbers)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, rows, F, generator=g)
    y = (torch.rand(P, rows, generator=g) > 0.5).float()
    D = ref.num_params(F, H)
    state = torch.zeros(P, 6, D)
    state[:, 0] = torch.randn(P, D, generator=g)
    state[:, 1] = torch.randn(P, D, generator=g) * 0.5 - 1.
    return x, y, state


def steps(x, y, state, H, num_steps, n_of=None, problem_ids=None, **kw):
    """hipops.bnn_svi_steps on copies: (state after, loss), on the host."""
    n = None if n_of is None else torch.tensor(n_of, dtype=torch.int32, device=DEV)
    ids = None if problem_ids is None else torch.tensor(problem_ids, dtype=torch.int64, device=DEV)
    st = state.to(DEV).clone()
    loss = hipops.bnn_svi_steps(x.to(DEV), y.to(DEV), st, H, num_steps, n_of=n, problem_ids=ids, **kw)
    return st.cpu(), loss.cpu()


def rel(got, want):
    """max over problems of |got - want| / |want| (row norms)."""
    return float(((got.double() - want).norm(dim=-1) / want.norm(dim=-1)).max())


@functools.lru_cache(maxsize=None)
def one_step_case(label):
    """Inputs and the f64 (loss, g_loc, g_u) of every problem of a case (computed once)."""
    H, F, K, activation, n_of = ONE_STEP[label]
    x, y, state = problem(H, F, 3, 2000 + sum(map(ord, label)))
    D = ref.num_params(F, H)
    seed = 40 + len(label)
    want = [svi.loss_and_grads(state[p, 0].double(), state[p, 1].double(), svi.noise(seed, p, 0, K, D), x[p], y[p], n_of[p], F, H, activation) for p in range(3)]
    return x, y, state, seed, want


@pytest.mark.parametrize('label', list(ONE_STEP))
def test_one_step_against_f64(label):
    """From zero moments, m / (1 - beta1) after one step IS the ELBO gradient."""
    H, F, K, activation, n_of = ONE_STEP[label]
    x, y, state, seed, want = one_step_case(label)
    after, loss = steps(x, y, state, H, 1, n_of=n_of, num_particles=K, seed=seed, activation=activation)
    assert bool(torch.isfinite(after).all()) and bool(torch.isfinite(loss).all())
    e_loc = rel(after[:, 2] / BETA1, torch.stack([w[1] for w in want]))
    e_u = rel(after[:, 4] / BETA1, torch.stack([w[2] for w in want]))
    L64 = np.array([w[0] for w in want])
    e_loss = float(np.max(np.abs(loss[:, 0].double().numpy() - L64) / np.abs(L64)))
    print(f'{label}: H {H} F {F} K {K} {activation} n_of {n_of}: g_loc {e_loc:.3e}, g_u {e_u:.3e}, loss {e_loss:.3e}')
    bounds.within(f'{label} g_loc', e_loc, ONE_STEP_BOUNDS[label][0])
    bounds.within(f'{label} g_u', e_u, ONE_STEP_BOUNDS[label][1])
    bounds.within(f'{label} loss', e_loss, ONE_STEP_BOUNDS[label][2])


def test_a_null_n_of_means_all_rows():
    x, y, state = problem(5, 3, 3, 31)
    kw = dict(num_particles=3, lr=0.05, seed=8, activation='tanh')
    a1, l1 = steps(x, y, state, 5, 4, n_of=(S, S, S), **kw)
    a2, l2 = steps(x, y, state, 5, 4, **kw)
    assert torch.equal(a1, a2) and torch.equal(l1, l2)
    assert not torch.equal(steps(x, y, state, 5, 4, n_of=(S, S - 1, S), **kw)[0][1], a2[1])


@functools.lru_cache(maxsize=None)
def trajectory_f64(lr):
    H, F, K, T, n_of = 5, 3, 3, 50, (100, 63, 1)
    x, y, state = problem(H, F, 3, 91)
    out = [svi.run(state[p].double(), x[p], y[p], n_of[p], F, H, 'tanh', K=K, num_steps=T, lr=lr, seed=6, q=p) for p in range(3)]
    return x, y, state, n_of, torch.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def trajectory_errors(after, loss, want_state, want_loss):
    e_loc = rel(after[:, 0], want_state[:, 0])
    e_scale = rel(torch.nn.functional.softplus(after[:, 1].double()), svi.softplus(want_state[:, 1]))
    e_loss = float(np.max(np.abs(loss.double().numpy() - want_loss) / np.maximum(1., np.abs(want_loss))))
    return e_loc, e_scale, e_loss


@pytest.mark.parametrize('lr', [1e-3, 0.05])
def test_fifty_steps_against_f64(lr):
    x, y, state, n_of, want_state, want_loss = trajectory_f64(lr)
    after, loss = steps(x, y, state, 5, 50, n_of=n_of, num_particles=3, lr=lr, seed=6, activation='tanh')
    assert loss.shape == (3, 50) and bool(torch.isfinite(after).all()) and bool(torch.isfinite(loss).all())
    e_loc, e_scale, e_loss = trajectory_errors(after, loss, want_state, want_loss)
    print(f'50 steps at lr {lr}: loc {e_loc:.3e}, scale {e_scale:.3e}, loss {e_loss:.3e}')
    for name, e, b in zip(('loc', 'scale', 'loss'), (e_loc, e_scale, e_loss), TRAJECTORY_BOUNDS[lr]):
        bounds.within(f'lr {lr} {name}', e, b)


def test_the_chunked_path_against_f64():
    """S = n = 1100 rows of 16 features: 75 KB, above the kernel's 48 KB budget for resident rows, so every step stages 64-row chunks."""
    H, F, K, T, rows = 8, 16, 2, 3, 1100
    x, y, state = problem(H, F, 1, 17, rows=rows)
    want_state, want_loss = svi.run(state[0].double(), x[0], y[0], rows, F, H, 'tanh', K=K, num_steps=T, lr=0.01, seed=3, q=0)
    after, loss = steps(x, y, state, H, T, num_particles=K, lr=0.01, seed=3, activation='tanh')
    e_loc, e_scale, e_loss = trajectory_errors(after, loss, want_state[None], want_loss[None])
    print(f'chunked: loc {e_loc:.3e}, scale {e_scale:.3e}, loss {e_loss:.3e}')
    for name, e, b in zip(('loc', 'scale', 'loss'), (e_loc, e_scale, e_loss), CHUNKED_BOUNDS):
        bounds.within(f'chunked {name}', e, b)


@pytest.mark.parametrize('H,F,K,activation', [(5, 3, 33, 'tanh'), (9, 16, 3, 'identity'), (17, 8, 9, 'tanh'), (32, 3, 1, 'identity'), (33, 8, 1, 'tanh'), (64, 1, 5, 'identity')])
def test_a_problem_is_a_bitwise_function_of_its_own_inputs(H, F, K, activation):
    """(a) Problem q of a P = 3 call against the same problem alone with problem_ids = [q]; every Hp (8, 16, 32 twice, 64 twice)."""
    n_of = (65, 7, 100)
    x, y, state = problem(H, F, 3, 400 + H)
    after, loss = steps(x, y, state, H, 5, n_of=n_of, num_particles=K, lr=0.05, seed=9, activation=activation)
    for q in range(3):
        a1, l1 = steps(x[q:q + 1], y[q:q + 1], state[q:q + 1], H, 5, n_of=n_of[q:q + 1], problem_ids=[q], num_particles=K, lr=0.05, seed=9, activation=activation)
        assert torch.equal(a1[0], after[q]) and torch.equal(l1[0], loss[q]), q
    # ... wherever it sits: the batch reversed, with the ids saying who is who
    a2, l2 = steps(x.flip(0).contiguous(), y.flip(0).contiguous(), state.flip(0).contiguous(), H, 5, n_of=n_of[::-1], problem_ids=[2, 1, 0], num_particles=K, lr=0.05,
                   seed=9, activation=activation)
    assert torch.equal(a2.flip(0), after) and torch.equal(l2.flip(0), loss)
    # another id or another seed is another noise stream
    a3, _ = steps(x[:1], y[:1], state[:1], H, 5, n_of=n_of[:1], problem_ids=[7], num_particles=K, lr=0.05, seed=9, activation=activation)
    a4, _ = steps(x[:1], y[:1], state[:1], H, 5, n_of=n_of[:1], num_particles=K, lr=0.05, seed=10, activation=activation)
    assert not torch.equal(a3[0], after[0]) and not torch.equal(a4[0], after[0])


def test_a_run_split_over_launches_is_the_same_run():
    """(b) steps(0, 20) against steps(0, 7) then steps(7, 13), and fit_bnn_svi at three launch lengths."""
    H, F, K = 5, 3, 3
    x, y, state = problem(H, F, 3, 21)
    kw = dict(n_of=(100, 64, 3), num_particles=K, lr=0.05, seed=2, activation='tanh')
    whole, loss = steps(x, y, state, H, 20, **kw)
    first, l1 = steps(x, y, state, H, 7, **kw)
    second, l2 = steps(x, y, first, H, 13, step0=7, **kw)
    assert torch.equal(second, whole) and torch.equal(torch.cat([l1, l2], 1), loss)
    assert not torch.equal(steps(x, y, first, H, 13, step0=0, **kw)[0], whole)      # step0 counts: the noise and the bias corrections follow it
    spec = dict(num_features=F, embed=H)
    fits = [study.fit_bnn_svi(x.to(DEV), y.to(DEV), spec, n_of=[100, 64, 3], num_steps=20, lr=0.05, num_particles=K, seed=2, activation='tanh', steps_per_launch=per)
            for per in (1, 7, 256)]
    assert fits[0].losses.shape == (3, 20) and fits[0].loc.shape == (3, 32) and bool((fits[0].scale > 0).all())
    for f in fits[1:]:
        assert torch.equal(f.state, fits[0].state) and torch.equal(f.losses, fits[0].losses)


def test_rows_beyond_n_and_columns_beyond_d_are_never_touched():
    """(c) NaN in the rows >= n of x / y, a sentinel in the columns >= D of a state with ld = D + 5."""
    H, F, K = 5, 3, 3
    n_of = (0, 63, 99)
    D = ref.num_params(F, H)
    x, y, state = problem(H, F, 3, 77)
    clean, clean_loss = steps(x, y, state, H, 6, n_of=n_of, num_particles=K, lr=0.05, seed=1, activation='tanh')
    xp, yp = x.clone(), y.clone()
    for p, n in enumerate(n_of):
        xp[p, n:], yp[p, n:] = float('nan'), float('nan')
    wide = torch.full((3, 6, D + 5), -777.)
    wide[:, :, :D] = state
    after, loss = steps(xp, yp, wide, H, 6, n_of=n_of, num_particles=K, lr=0.05, seed=1, activation='tanh')
    assert bool((after[:, :, D:] == -777.).all()) and torch.equal(after[:, :, :D], clean) and torch.equal(loss, clean_loss)
    assert bool(torch.isfinite(clean).all()) and bool(torch.isfinite(clean_loss).all())


def test_a_non_finite_problem_stays_alone():
    """(d) One problem's loc0 is NaN: it stays non-finite, the others are the bits of a run without it."""
    H, F, K = 9, 5, 17
    x, y, state = problem(H, F, 3, 5)
    good, good_loss = steps(x, y, state, H, 6, num_particles=K, lr=0.05, seed=1)
    bad = state.clone()
    bad[1, 0, 3] = float('nan')
    after, loss = steps(x, y, bad, H, 6, num_particles=K, lr=0.05, seed=1)
    assert not bool(torch.isfinite(after[1, 0]).all()) and not bool(torch.isfinite(loss[1]).any())
    assert torch.equal(after[[0, 2]], good[[0, 2]]) and torch.equal(loss[[0, 2]], good_loss[[0, 2]])


def test_with_no_data_the_guides_find_the_prior():
    """n_of = 0: the ELBO's optimum is the prior N(0, I), where the loss is 0.  tests/test_host_bnn_svi.py shows the restatement alone meets the same three
    conditions with this seed and this noise (0.159, 0.070 and 0.079 there)."""
    c = svi.NO_DATA
    state = hipops.bnn_svi_state(c['P'], c['F'], c['H'], 'cpu', loc0=svi.no_data_loc0(), init_scale=c['init_scale'])
    x, y = torch.zeros(c['P'], 1, c['F']), torch.zeros(c['P'], 1)
    after, loss = steps(x, y, state, c['H'], c['T'], n_of=[0] * c['P'], num_particles=c['K'], lr=c['lr'], seed=c['seed'])
    loc, scale = after[:, 0], torch.nn.functional.softplus(after[:, 1])
    first, last = float(loss[:, 0].mean()), float(loss[:, -50:].mean())
    print(f'no data: max |loc| {float(loc.abs().max()):.3f}, max |scale - 1| {float((scale - 1).abs().max()):.3f}, loss {first:.1f} -> {last:.3f}')
    bounds.within('no data max |loc|', float(loc.abs().max()), 0.3)      # the issue's three conditions, with their values on record
    bounds.within('no data max |scale - 1|', float((scale - 1).abs().max()), 0.2)
    bounds.within('no data mean of the last 50 losses', last, 0.5)
    assert first > 30.


@pytest.mark.parametrize('activation', ['identity', 'tanh'])
def test_with_data_the_loss_falls_and_the_predictive_is_the_f64_predictive(activation):
    """Problems drawn from the model: n = 40, K = 4, T = 300, lr = 0.05."""
    F, H, P, n = 3, 5, 4, 40
    spec = dict(num_features=F, embed=H)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(P, n + 10, F, generator=g)
    w = torch.randn(P, ref.num_params(F, H), generator=g, dtype=torch.float64)
    p1 = torch.stack([ref.predict(w[p], x[p], F, H, activation) for p in range(P)])
    y = (torch.rand(P, n + 10, generator=g).double() < p1).float()
    guide = study.fit_bnn_svi(x[:, :n].contiguous().to(DEV), y[:, :n].contiguous().to(DEV), spec, num_steps=300, lr=0.05, num_particles=4, seed=3, activation=activation)
    losses = guide.losses.cpu()
    first, last = losses[:, :20].mean(1), losses[:, -20:].mean(1)
    print(f'{activation}: mean loss of the first 20 steps {first.tolist()}, of the last 20 {last.tolist()}')
    assert bool(torch.isfinite(losses).all()) and bool((first - last > 10.).all())
    xt = x[:, n:].contiguous()
    theta = guide.sample(6, seed=4)
    prob = guide.predictive(xt.to(DEV), 6, seed=4)
    assert theta.shape == (P, 6, 32) and prob.shape == (P, 6, 10) and bool(((prob >= 0) & (prob <= 1)).all())
    for p in range(P):
        for i in (0, 5):
            assert float((ref.predict(theta[p, i].double().cpu(), xt[p], F, H, activation) - prob[p, i].double().cpu()).abs().max()) < 1e-5


def test_eval_svi_on_toy_data(tmp_path):
    spec = study.get_default_model_spec('small')
    model = study.BayesianModel(spec, device=DEV)
    X, y = study.generate_toy_data(model, 30, device=DEV)
    X, y = X[:4], y[:4]
    nll, acc = study.eval_svi(X, y, DEV, spec, 10, num_train_steps=40, num_pred_samples=20)
    assert isinstance(nll, np.ndarray) and isinstance(acc, np.ndarray) and nll.shape == (4,) and acc.shape == (4,)
    assert np.isfinite(nll).all() and np.isfinite(acc).all() and (acc >= 0).all() and (acc <= 1).all() and (nll > 0).all()
    nll2, acc2 = study.eval_svi(X, y, DEV, spec, 10, num_train_steps=40, num_pred_samples=20)
    assert np.array_equal(nll, nll2) and np.array_equal(acc, acc2)
    # the reference's estimator (sampled observations, mean hard prediction), and a model sampler in place of the spec
    nll3, acc3 = study.eval_svi(X, y, DEV, lambda: study.BayesianModel(spec, device=DEV), 10, num_train_steps=40, num_pred_samples=20, num_particles=2, sample_obs=True)
    assert nll3.shape == (4,) and acc3.shape == (4,) and np.isfinite(nll3).all() and (acc3 >= 0).all() and (acc3 <= 1).all()
    # the 'big' spec (D = 706), which the NUTS arm refuses, runs
    big = study.get_default_model_spec('big')
    Xb = torch.randn(3, 20, 8, generator=torch.Generator().manual_seed(1)).to(DEV)
    yb = (torch.rand(3, 20, generator=torch.Generator().manual_seed(2)) > 0.5).float().to(DEV)
    nll4, acc4 = study.eval_svi(Xb, yb, DEV, big, 12, num_train_steps=30, num_pred_samples=8)
    assert nll4.shape == (3,) and np.isfinite(nll4).all() and np.isfinite(acc4).all() and (nll4 > 0).all()
    with pytest.raises(ValueError, match='128'):
        study.eval_mcmc(Xb, yb, DEV, big, 12, 4, 4)
    with pytest.raises(NotImplementedError, match='Stein'):
        study.eval_svi(X, y, DEV, spec, 10, 4, 4, svgd=True)


def test_training_steps_writes_the_references_files(tmp_path):
    """training_steps('svi', ...), the call of the reference's __main__: 2 .. 4096 steps and as many draws, one file each."""
    spec = study.get_default_model_spec('small')
    g = torch.Generator().manual_seed(3)
    X, y = torch.randn(3, 104, 3, generator=g), (torch.rand(3, 104, generator=g) > 0.5).float()
    study.training_steps('svi', X, y, spec, device=DEV, path_interfix=str(tmp_path))
    assert sorted(f.name for f in tmp_path.iterdir()) == sorted(f'results_svi_training_steps_{s}.npy' for s in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096))
    for s in (2, 4096):
        nll, acc, seconds = np.load(tmp_path / f'results_svi_training_steps_{s}.npy', allow_pickle=True)
        assert nll.shape == (3,) and acc.shape == (3,) and np.isfinite(nll).all() and (acc >= 0).all() and (acc <= 1).all() and seconds > 0
