"""pfn_bnn_cv on the MI355X against the restatement tests/bnn_cv_f64.py (written from the contract in include/pfn_hip.h): one step, fifty steps and the predictive
against f64 under the project's f32 rule -- a kernel result may differ from the f64 one by 4 max(e, floor), e the error of the float32 CPU run of the same
restatement on the same inputs --, the bitwise invariants of the contract, the recorded grid searches of tests/golden/tabular_bnn.pt, and the study's arm end to
end.  PFN_RECORD_BOUNDS=<path> writes every measured maximum with its e (profiles/r20_bnn_cv_bounds_measured.json is such a run)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnn_cv_f64 as cvf      # noqa: E402
import bnn_f64 as ref      # noqa: E402
import bounds      # noqa: E402
import tabular_cases      # noqa: E402

from transformerscandobayesianinference_amd import hipops, tabular      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
BETA1 = float(np.float32(1) - np.float32(0.9))      # the kernel's 1 - beta1
IDS = (5, 0, 9)
# label -> (n, F, T, n_splits, widths), P = 3 each.  Together: H of {1, 5, 10, 30, 63, 64}, F of {1, 3, 60, 127, 128}, n of {4, 5, 63, 64, 65, 128}, T of {1, 128},
# n_splits of {2, 5}, lists that mix widths, D from 7 to 8386 (the kernel has one placement of the state for every D: no switch to stand on both sides of).
CASES = {
    'n4_F1': (4, 1, 1, 2, (1, 5)),
    'n5_F3': (5, 3, 128, 2, (10, 1, 64)),
    'n63_F60': (63, 60, 1, 5, (30, 63)),
    'n64_F127': (64, 127, 1, 5, (5, 64)),
    'n65_F128': (65, 128, 128, 5, (63, 10)),
    'n128_F128': (128, 128, 128, 5, (64,)),
}
assert {h for c in CASES.values() for h in c[4]} == {1, 5, 10, 30, 63, 64} and {c[1] for c in CASES.values()} == {1, 3, 60, 127, 128}
assert {c[0] for c in CASES.values()} == {4, 5, 63, 64, 65, 128} and {c[2] for c in CASES.values()} == {1, 128} and {c[3] for c in CASES.values()} == {2, 5}


def problem(n, F, T, n_splits, widths, seed, P=3, loc_std=1.0):
    """train [P,n,F], labels [P,n], test [P,T,F], fold [P,n] int32 -- problem 0 has one row with a fold value above the range, problem 1 one below it -- and a
    state [P,NC,6,6,ld] with loc ~ N(0, loc_std^2), u ~ N(-1, 0.5), zero moments and ld three columns more than the largest D; all on the host."""
    g = torch.Generator().manual_seed(seed)
    train, test = torch.randn(P, n, F, generator=g), torch.randn(P, T, F, generator=g)
    labels = (torch.rand(P, n, generator=g) > 0.5).float()
    fold = torch.tensor([[(3 * i + p) % n_splits for i in range(n)] for p in range(P)], dtype=torch.int32)
    fold[0, 1] = 7
    if P > 1:
        fold[1, 2] = -1
    ld = max(ref.num_params(F, h) for h in widths) + 3
    state = torch.zeros(P, len(widths), 6, 6, ld)
    state[:, :, :, 0] = torch.randn(P, len(widths), 6, ld, generator=g) * loc_std
    state[:, :, :, 1] = torch.randn(P, len(widths), 6, ld, generator=g) * 0.5 - 1.
    return train, labels, test, fold, state


def launch(prob, n_splits, widths, lrs, num_steps, ids=IDS, sel=None, **kw):
    """hipops.bnn_cv on copies (of the problems `sel`): (state after, BnnCvOut), on the host."""
    train, labels, test, fold, state = (t if sel is None else t[list(sel)].contiguous() for t in prob)
    ids = None if ids is None else torch.tensor([ids[i] for i in (range(len(train)) if sel is None else sel)], dtype=torch.int64, device=DEV)
    st = state.to(DEV).clone()
    out = hipops.bnn_cv(train.to(DEV), labels.to(DEV), test.to(DEV), fold.to(DEV), n_splits, widths, lrs, st, num_steps, problem_ids=ids, **kw)
    return st.cpu(), hipops.BnnCvOut(*(None if t is None else t.cpu() for t in out))


def fits(P, widths, n_splits):
    return [(p, c, s) for p in range(P) for c in range(len(widths)) for s in range(n_splits + 1)]


def relerr(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


def floor_rule(e, floor=2. ** -23):
    return 4 * max(e, floor)


@functools.lru_cache(maxsize=None)
def one_step_case(label):
    """Inputs and, per fit, the f64 (L, g_loc, g_u) with the float32 restatement's errors against them (computed once)."""
    n, F, T, n_splits, widths = CASES[label]
    prob = problem(n, F, T, n_splits, widths, 3000 + sum(map(ord, label)))
    train, labels, test, fold, state = prob
    seed = 40 + len(label)
    want, e = {}, [0., 0., 0.]
    for p, c, s in fits(3, widths, n_splits):
        H = widths[c]
        D = ref.num_params(F, H)
        mask, q = cvf.row_mask(fold[p].numpy(), s, n_splits), cvf.stream(IDS[p], s)
        out = []
        for dtype in (torch.float64, torch.float32):
            loc, u = state[p, c, s, 0, :D].to(dtype), state[p, c, s, 1, :D].to(dtype)
            out.append(cvf.loss_and_grads(loc, u, cvf.step_noise(seed, q, 0, D, dtype), train[p], labels[p], mask, F, H))
        (L, g_loc, g_u), (L32, g32_loc, g32_u) = out
        want[p, c, s] = (float(L), g_loc, g_u)
        e = [max(e[0], relerr(g32_loc, g_loc)), max(e[1], relerr(g32_u, g_u)), max(e[2], abs(float(L32) - float(L)) / abs(float(L)))]
    return prob, seed, want, e


@pytest.mark.parametrize('label', list(CASES))
def test_one_step_against_f64(label):
    """From zero moments, m / (1 - beta1) after one step IS the ELBO gradient."""
    n, F, T, n_splits, widths = CASES[label]
    prob, seed, want, e = one_step_case(label)
    after, out = launch(prob, n_splits, widths, [1e-3] * len(widths), 1, seed=seed, want_loss=True)
    worst = [0., 0., 0.]
    for (p, c, s), (L, g_loc, g_u) in want.items():
        D = ref.num_params(F, widths[c])
        assert int(out.status[p, c, s]) == hipops.BNN_CV_DONE
        got = (relerr(after[p, c, s, 2, :D] / BETA1, g_loc), relerr(after[p, c, s, 4, :D] / BETA1, g_u), abs(float(out.loss[p, c, s, 0]) - L) / abs(L))
        worst = [max(a, b) for a, b in zip(worst, got)]
    print(f'{label}: g_loc {worst[0]:.3e} (e {e[0]:.3e}), g_u {worst[1]:.3e} (e {e[1]:.3e}), loss {worst[2]:.3e} (e {e[2]:.3e})')
    for name, v, ev in zip(('g_loc', 'g_u', 'loss'), worst, e):
        bounds.within(f'{label} {name} (e {ev:.3e})', v, floor_rule(ev))


TRAJ = dict(n=20, F=8, T=5, n_splits=5, widths=(5, 30), P=2, steps=50, seed=6)


@functools.lru_cache(maxsize=None)
def trajectory(lr):
    c = TRAJ
    prob = problem(c['n'], c['F'], c['T'], c['n_splits'], c['widths'], 91, P=c['P'])
    train, labels, test, fold, state = prob
    want, e = {}, [0., 0., 0.]
    for p, k, s in fits(c['P'], c['widths'], c['n_splits']):
        H = c['widths'][k]
        mask, q = cvf.row_mask(fold[p].numpy(), s, c['n_splits']), cvf.stream(IDS[p], s)
        (s64, l64), (s32, l32) = (cvf.run(state[p, k, s], train[p], labels[p], mask, c['F'], H, lr, q, c['seed'], 0, c['steps'], dtype=d) for d in (torch.float64, torch.float32))
        want[p, k, s] = (s64, l64)
        e = [max(e[0], relerr(s32[0], s64[0])), max(e[1], relerr(cvf.softplus(s32[1]), cvf.softplus(s64[1]))), max(e[2], float(np.max(np.abs(l32 - l64) / np.abs(l64))))]
    return prob, want, e


@pytest.mark.parametrize('lr', [1e-3, 0.05])
def test_fifty_steps_against_f64(lr):
    c = TRAJ
    prob, want, e = trajectory(lr)
    after, out = launch(prob, c['n_splits'], c['widths'], [lr] * 2, c['steps'], seed=c['seed'], want_loss=True)
    worst = [0., 0., 0.]
    for (p, k, s), (s64, l64) in want.items():
        D = s64.shape[1]
        got = (relerr(after[p, k, s, 0, :D], s64[0]), relerr(cvf.softplus(after[p, k, s, 1, :D].double()), cvf.softplus(s64[1])),
               float(np.max(np.abs(out.loss[p, k, s].double().numpy() - l64) / np.abs(l64))))
        worst = [max(a, b) for a, b in zip(worst, got)]
    print(f'50 steps at lr {lr}: loc {worst[0]:.3e} (e {e[0]:.3e}), scale {worst[1]:.3e} (e {e[1]:.3e}), loss {worst[2]:.3e} (e {e[2]:.3e})')
    for name, v, ev in zip(('loc', 'scale', 'loss'), worst, e):
        bounds.within(f'lr {lr} {name} (e {ev:.3e})', v, floor_rule(ev))


PRED = dict(n=65, F=60, T=128, n_splits=5, widths=(10, 64), P=2, S=40, seed=13)


@functools.lru_cache(maxsize=None)
def predictive_case():
    c = PRED
    prob = problem(c['n'], c['F'], c['T'], c['n_splits'], c['widths'], 77, P=c['P'], loc_std=0.15)
    train, labels, test, fold, state = prob
    want, e = {}, 0.
    for p, k, s in fits(c['P'], c['widths'], c['n_splits']):
        H = c['widths'][k]
        D = ref.num_params(c['F'], H)
        q = cvf.stream(IDS[p], s)
        rows = np.flatnonzero(fold[p].numpy() == s) if s < c['n_splits'] else np.arange(c['T'])
        x, ids = (train[p][rows], rows) if s < c['n_splits'] else (test[p], c['n'] + rows)
        p64, probs, hits = cvf.predictive(state[p, k, s, 0, :D].double(), state[p, k, s, 1, :D].double(), x, ids, c['F'], H, c['S'], q, c['seed'], want_draws=True)
        p32, _, _ = cvf.predictive(state[p, k, s, 0, :D], state[p, k, s, 1, :D], x, ids, c['F'], H, c['S'], q, c['seed'])
        uniforms = torch.stack([cvf.obs_uniforms(c['seed'], q, d, int(ids.max()) + 1)[ids] for d in range(c['S'])])
        want[p, k, s] = (rows, p64, probs, hits, uniforms)
        e = max(e, float((p32.double() - p64).abs().max()))
    return prob, want, e


def test_predictive_at_a_fixed_state_against_f64():
    c = PRED
    prob, want, e = predictive_case()
    window = floor_rule(e, 2. ** -24)
    after, out = launch(prob, c['n_splits'], c['widths'], [1e-3] * 2, 0, num_pred_samples=c['S'], seed=c['seed'], sample_obs=True)
    assert torch.equal(after, prob[4])      # no step: the state is only read
    worst, pairs, unsure, spread = 0., 0, 0, 0.
    for (p, k, s), (rows, p64, probs, hits, uniforms) in want.items():
        got, drawn = (out.cv_prob[p, k, rows], out.cv_draw[p, k, rows]) if s < c['n_splits'] else (out.test_prob[p, k], out.test_draw[p, k])
        worst = max(worst, float((got.double() - p64).abs().max()))
        close = (probs - uniforms).abs() <= window      # (row, draw) pairs the f32 probability may put on the other side of the uniform
        pairs, unsure = pairs + close.numel(), unsure + int(close.sum())
        counts = (drawn.double() * c['S']).round()      # the kernel writes count / S rounded to f32
        assert bool(((drawn.double() * c['S'] - counts).abs() <= 1e-4).all())
        assert bool(((counts - hits.sum(0).double()).abs() <= close.sum(0).double() + 1e-9).all()), (p, k, s)
        spread = max(spread, float((drawn.double() - p64).abs().max()))
    print(f'predictive: prob {worst:.3e} (e {e:.3e}), {unsure} of {pairs} pairs unsure, draws within {spread:.3f} of the probabilities')
    bounds.within(f'predictive prob (e {e:.3e})', worst, window)
    assert unsure <= 0.01 * pairs
    assert spread <= 5 * (0.25 / c['S']) ** 0.5
    assert bool(torch.isnan(out.cv_prob[0, :, 1]).all()) and bool(torch.isnan(out.cv_prob[1, :, 2]).all())      # a row in no fold is never written
    assert bool(torch.isfinite(out.cv_prob[:, :, 3:]).all()) and bool(torch.isfinite(out.test_prob).all())


SMALL = dict(n=10, F=3, T=4, n_splits=2, widths=(5, 10, 64, 5), lrs=(1e-3, 0.05, 1e-2, 1e-4))


@functools.lru_cache(maxsize=None)
def small_whole(steps=400, S=8):
    c = SMALL
    prob = problem(c['n'], c['F'], c['T'], c['n_splits'], c['widths'], 55)
    return prob, launch(prob, c['n_splits'], c['widths'], c['lrs'], steps, num_pred_samples=S, seed=21, want_loss=True, sample_obs=True)


def same(a, b):
    return all((x is None and y is None) or torch.equal(torch.nan_to_num(x, nan=-7.), torch.nan_to_num(y, nan=-7.)) for x, y in zip(a, b))


def test_a_fit_is_the_same_alone_in_a_batch_and_in_the_reversed_batch():
    c = SMALL
    prob, (after, out) = small_whole()
    kw = dict(num_pred_samples=8, seed=21, want_loss=True, sample_obs=True)
    for p in range(3):
        a1, o1 = launch(prob, c['n_splits'], c['widths'], c['lrs'], 400, sel=(p,), **kw)
        assert torch.equal(a1[0], after[p]) and same([t[0] for t in o1], [t[p] for t in out]), p
    a2, o2 = launch(prob, c['n_splits'], c['widths'], c['lrs'], 400, sel=(2, 1, 0), **kw)
    assert torch.equal(a2.flip(0), after) and same([t.flip(0) for t in o2], out)
    # the candidates reversed, and one candidate alone against the same inside the mixed list
    rev = tuple(t if i < 4 else t.flip(1) for i, t in enumerate(prob))
    a3, o3 = launch(rev, c['n_splits'], c['widths'][::-1], c['lrs'][::-1], 400, **kw)
    assert torch.equal(a3.flip(1), after) and same([t.flip(1) for t in o3], out)
    for k in (0, 2):
        D = ref.num_params(c['F'], c['widths'][k])
        one = tuple(t if i < 4 else t[:, k:k + 1, :, :, :D + 1].contiguous() for i, t in enumerate(prob))      # another ld as well
        a4, o4 = launch(one, c['n_splits'], c['widths'][k:k + 1], c['lrs'][k:k + 1], 400, **kw)
        assert torch.equal(a4[:, 0, :, :, :D], after[:, k, :, :, :D]) and same([t[:, 0] for t in o4], [t[:, k] for t in out]), k
    # another id or another seed is another noise stream; the two candidates of width 5 share theirs but not their learning rate
    assert not torch.equal(launch(prob, c['n_splits'], c['widths'], c['lrs'], 3, ids=(5, 0, 8), seed=21)[0][2], launch(prob, c['n_splits'], c['widths'], c['lrs'], 3, seed=21)[0][2])
    assert not torch.equal(after[:, 0], after[:, 3])


@pytest.mark.parametrize('per_launch', [1, 7])
def test_split_launches_and_the_predictive_in_a_call_of_its_own(per_launch):
    c = SMALL
    prob, (after, out) = small_whole()
    st = prob[4].to(DEV).clone()
    dev = [t.to(DEV) for t in prob[:4]]
    ids = torch.tensor(IDS, dtype=torch.int64, device=DEV)
    losses = []
    for t0 in range(0, 400, per_launch):
        k = min(per_launch, 400 - t0)
        losses.append(hipops.bnn_cv(*dev, c['n_splits'], c['widths'], c['lrs'], st, k, step0=t0, seed=21, problem_ids=ids, want_loss=True).loss)
    assert torch.equal(st.cpu(), after) and same([torch.cat(losses, -1).cpu()], [out.loss])
    alone = hipops.bnn_cv(*dev, c['n_splits'], c['widths'], c['lrs'], st, 0, num_pred_samples=8, seed=21, problem_ids=ids, sample_obs=True)
    assert torch.equal(st.cpu(), after) and same([t.cpu() for t in alone[1:5]], out[1:5]) and torch.equal(alone.status.cpu(), out.status)


def test_sentinels_stay_untouched():
    c = SMALL
    prob, (after, out) = small_whole()
    before = prob[4]
    assert bool((out.status[:, :, :3] == hipops.BNN_CV_DONE).all()) and bool((out.status[:, :, 3:] == hipops.BNN_CV_UNUSED).all())
    assert torch.equal(after[:, :, 3:], before[:, :, 3:])      # the unused slots
    for k, H in enumerate(c['widths']):
        D = ref.num_params(c['F'], H)
        assert torch.equal(after[:, k, :, :, D:], before[:, k, :, :, D:]) and not torch.equal(after[:, k, :3, :, :D], before[:, k, :3, :, :D])
    fold = prob[3]
    in_a_fold = (fold >= 0) & (fold < c['n_splits'])
    assert bool(torch.isnan(out.cv_prob[~in_a_fold[:, None, :].expand_as(out.cv_prob)]).all()) and bool(torch.isfinite(out.cv_prob[in_a_fold[:, None, :].expand_as(out.cv_prob)]).all())
    assert torch.equal(torch.isnan(out.cv_draw), torch.isnan(out.cv_prob)) and bool(torch.isfinite(out.test_prob).all())
    assert bool(torch.isfinite(out.loss[:, :, :3]).all()) and bool(torch.isnan(out.loss[:, :, 3:]).all())
    assert bool(((out.cv_prob >= 0) & (out.cv_prob <= 1))[in_a_fold[:, None, :].expand_as(out.cv_prob)].all())


def test_a_non_finite_fit_stays_alone():
    c = SMALL
    prob, (after, out) = small_whole()
    train = prob[0].clone()
    train[1][prob[3][1] == 0] = float('nan')      # the rows of fold 0 of problem 1
    a, o = launch((train,) + prob[1:], c['n_splits'], c['widths'], c['lrs'], 400, num_pred_samples=8, seed=21, want_loss=True, sample_obs=True)
    assert torch.equal(a[1, :, 0], after[1, :, 0]) and bool((o.status[1, :, 0] == hipops.BNN_CV_DONE).all())      # slot 0 never reads them
    assert torch.equal(o.loss[1, :, 0], out.loss[1, :, 0])
    assert bool((o.status[1, :, 1:3] == hipops.BNN_CV_NONFINITE).all()) and bool((o.status[1, :, 3:] == hipops.BNN_CV_UNUSED).all())
    for p in (0, 2):      # the neighbours
        assert torch.equal(a[p], after[p]) and same([t[p] for t in o], [t[p] for t in out])


@functools.lru_cache(maxsize=None)
def recorded():
    return torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_bnn.pt'), weights_only=False)


@pytest.mark.parametrize('k', range(len(cvf.SHAPES)))
def test_the_grid_search_against_the_recorded_f64_one(k):
    n, F, T = cvf.SHAPES[k]
    rec = recorded()
    r = rec['problems'][k]
    x, y, tx, ty = (torch.from_numpy(v).to(DEV) for v in tabular_cases.problem(n, F, T, r['seed']))
    details = {}
    metric, proba, params = tabular._bayes_batched(x[:, None], y[:, None], tx[:, None], ty[:, None], return_params=True, seed=rec['fit_seed'], details=details)
    window = floor_rule(r['e'])
    cv64, te64 = r['cv_prob'].numpy(), r['test_prob'].numpy()
    assert np.array_equal(details['folds'][0], r['folds'].numpy()) and bool((details['status'][0, :, :r['n_splits'] + 1] == hipops.BNN_CV_DONE).all())
    err = max(np.abs(details['cv_prob'][0] - cv64).max(), np.abs(details['test_prob'][0] - te64).max())
    print(f'(n {n}, F {F}, T {T}): probabilities within {err:.3e} of the recorded f64 ones (e {r["e"]:.3e})')
    bounds.within(f'fixture {k} prob (e {r["e"]:.3e})', err, window)
    sure = np.abs(cv64 - 0.5) > window
    assert np.array_equal((details['cv_prob'][0] > 0.5)[sure], (cv64 > 0.5)[sure])
    mean, best = details['scores'][0]
    if sure.all():
        assert best == r['best'] and mean.tobytes() == r['mean_test_score'].numpy().tobytes() and params[0] == tabular._bayes_grid()[0][best]
        assert np.abs(proba[:, 0] - te64[best]).max() <= window
    if k == 1:
        # the single-problem form is column 0 of the batched one, and the same seed gives the same bits twice
        m1, p1 = tabular.bayes_net_metric(x, y, tx, ty, [])
        assert np.array_equal([m1], metric[:1], equal_nan=True) and np.array_equal(p1, proba[:, 0])
        m2, p2 = tabular._bayes_batched(torch.stack([x, x.flip(0)], 1), torch.stack([y, y.flip(0)], 1), torch.stack([tx, tx], 1), torch.stack([ty, ty], 1))
        assert np.array_equal(m2[:1], metric[:1], equal_nan=True) and np.array_equal(p2[:, 0], proba[:, 0]) and not np.array_equal(p2[:, 1], p2[:, 0])
        m3, p3 = tabular._bayes_batched(x[:, None], y[:, None], tx[:, None], ty[:, None], sample_obs=True)
        assert np.abs(p3 - proba).max() <= 5 * (0.25 / 400) ** 0.5 and np.abs(p3 * 400 - np.round(p3 * 400)).max() <= 1e-3      # the reference's estimator: counts / 400


def test_it_learns():
    x, y, tx, ty = (torch.from_numpy(v).to(DEV) for v in tabular_cases.problem(80, 8, 20, 3))
    details = {}
    metric, proba = tabular._bayes_batched(x[:, None], y[:, None], tx[:, None], ty[:, None], details=details)
    loss = details['loss'][0, :, 5].astype(np.float64)      # the refits, [candidates, 400]
    drop = loss[:, :20].mean(1) - loss[:, -20:].mean(1)
    print('refit loss, first 20 minus last 20 steps, per candidate:', np.round(drop, 1).tolist(), 'AUC', metric[0])
    assert np.isfinite(loss).all() and (drop[0::2] > 10).all()      # every candidate at lr 1e-3 (the f64 restatement: 69 to 261 nats; at 1e-4 the narrowest drops 9.5)
    assert np.isfinite(metric[0]) and ((proba >= 0) & (proba <= 1)).all()


def test_evaluate_runs_the_bayes_arm_end_to_end():
    d = torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_diabetes.pt'))
    metric, outputs, ys = tabular.evaluate_position(d['X'].to(DEV), d['y'].to(DEV), [], tabular.bayes_net_metric, 30, 20, max_samples=3)
    assert metric.shape == (3,) and outputs.shape == (10, 3) and np.isfinite(metric).all() and ((outputs >= 0) & (outputs <= 1)).all()
    res = tabular.evaluate([['diabetes', d['X'], d['y'], []]], tabular.bayes_net_metric, 'bayes', 30, [10], DEV, max_samples=2)
    assert np.isfinite(res['mean_metric']) and res['diabetes_outputs_at_10'].shape == (20, 2)
