"""The logistic-regression baseline on the MI355X (csrc/logistic.hip; tabular.logistic_metric and what it calls) against the recorded f64 fits of
tests/golden/tabular_logistic.pt: the f64 optimality certificate of the kernel's own coefficients, coefficients and decision values, the integer counts, the
grid search end to end, independence of batch and grid position, the edge rules, and `evaluate`.  Fixtures only: no scikit-learn, no reference.
tests/logistic_f64.py holds the f64 restatement and the seeded problems.

PFN_LOGISTIC_MEASURE=<path> makes test_coefficients_and_decision_values write the distances it measured to <path>; the committed copy is
profiles/r17_logistic_bounds_measured.json, and the bounds asserted here are 4 x its entries."""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds      # noqa: E402
import logistic_f64 as lf      # noqa: E402

from transformerscandobayesianinference_amd import hipops, tabular      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -23
MEASURED = os.path.join(ROOT, 'profiles', 'r17_logistic_bounds_measured.json')
REQUIRED_C = (1e-5, 0.01, 1.0, 2.0)


def key(rec):
    return f"n{rec['n']}_F{rec['F']}_T{rec['T']}"


@pytest.fixture(scope='module')
def recorded():
    return torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_logistic.pt'), weights_only=False)


def run(x, y, test_x, folds, n_splits, cands):
    """One launch over problems stacked along the first axis (numpy in, numpy out)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    cvc, tz, st, coef = hipops.logistic_cv(t(x), t(y), t(test_x), t(folds), n_splits, [c for c, _ in cands], [k for _, k in cands], return_coef=True)
    return cvc.cpu().numpy(), tz.cpu().numpy(), st.cpu().numpy(), coef.cpu().numpy()


@pytest.fixture(scope='module')
def device(recorded):
    """The kernel's results for every recorded problem, computed once: key -> (cv_correct [NC,5], test_z [NC,T], status [NC,6,2], coef [NC,6,F+1])."""
    out = {}
    for rec in recorded['problems']:
        got = run(rec['x'].numpy()[None], rec['y'].numpy()[None], rec['test_x'].numpy()[None], rec['folds'].numpy()[None], rec['n_splits'], recorded['cands'])
        out[key(rec)] = tuple(a[0] for a in got)
    return out


def masks(rec):
    n, ns, folds = rec['n'], rec['n_splits'], rec['folds'].numpy()
    return [np.ones(n) if s == ns else (folds != s).astype(np.float64) for s in range(ns + 1)]


def decision_scale(x, w):
    F = x.shape[1]
    return np.abs(w[F]) + np.abs(x.astype(np.float64) * w[:F]).sum(1)


def has_optimum(rec, c, s, kind):
    """The f64 fit converged, and for 'none' the problem is one where the issue compares it: n >= 2 (F + 1) rows with noisy labels."""
    return int(rec['status'][c, s, 0]) == lf.CONVERGED and (kind & 3 != lf.NONE or rec['n'] >= 2 * (rec['F'] + 1))


def test_the_fixture_covers_the_cases(recorded):
    assert [(r['n'], r['F'], r['T']) for r in recorded['problems']] == [(4, 1, 1), (5, 3, 2), (10, 3, 20), (33, 8, 7), (80, 60, 20), (128, 128, 128)]
    have = set(recorded['cands'])
    for pen in (lf.L1, lf.L2):
        for icpt in (0, lf.FIT_INTERCEPT):
            assert all((C, pen | icpt) in have for C in REQUIRED_C)
    assert (1.0, lf.NONE) in have and (1.0, lf.NONE | lf.FIT_INTERCEPT) in have      # 'none' ignores C


def test_certificate_of_every_converged_fit(recorded, device):
    """(a) The f64 KKT residual of the kernel's own coefficients is within (64 + n) 2^-23 C max_j sum_i m_i |x_ij| wherever the kernel says 'converged': its
    threshold of 64 plus the worst-case round-off n 2^-23 of an n-term f32 gradient sum."""
    for rec in recorded['problems']:
        x, y, n = rec['x'].numpy(), rec['y'].numpy(), rec['n']
        _, _, status, coef = device[key(rec)]
        worst, converged = 0., 0
        for c, (C, kind) in enumerate(recorded['cands']):
            for s, mask in enumerate(masks(rec)):
                assert np.isfinite(coef[c, s]).all() and status[c, s, 0] in (lf.CONVERGED, lf.STALLED, lf.CAPPED, lf.ONE_CLASS)
                assert 0 <= status[c, s, 1] <= 48
                if status[c, s, 0] == lf.CONVERGED:
                    converged += 1
                    worst = max(worst, lf.kkt(x, y, mask, coef[c, s].astype(np.float64), C, kind) / (lf.effective_C(C, kind) * lf.scale(x, mask, kind)))
                if int(rec['status'][c, s, 0]) in (lf.ONE_CLASS, lf.CAPPED) or kind & 3 != lf.NONE:
                    # what f64 cannot solve, f32 cannot either; every penalised fit converges
                    assert status[c, s, 0] == (lf.CONVERGED if int(rec['status'][c, s, 0]) == lf.CONVERGED else int(rec['status'][c, s, 0])), (key(rec), C, kind, s)
            assert not status[c, rec['n_splits'] + 1:].any() and not coef[c, rec['n_splits'] + 1:].any()      # unused slots
        print(f'{key(rec)}: {converged} converged fits, worst certificate {worst / EPS:.2f} x 2^-23 of the scale (bound {64 + n})')
        assert converged >= 24 * (rec['n_splits'] + 1)
        bounds.within(f'certificate {key(rec)} / (2^-23 C max_j sum_i |x_ij|)', worst / EPS, 64 + n)


def measure(rec, cands, dev):
    """Worst distances of one problem to the recorded f64 fits: coefficients relative to max |w|, the refit's decision values relative to |b| + sum_j |w_j x_j|;
    where the f64 coefficients are all zero the kernel's must be, and its decision values too."""
    _, test_z, status, coef = dev
    tx, ns = rec['test_x'].numpy(), rec['n_splits']
    worst_w = worst_z = 0.
    for c, (C, kind) in enumerate(cands):
        for s in range(ns + 1):
            if not has_optimum(rec, c, s, kind):
                continue
            want = rec['coef'][c, s].numpy()
            if not want.any():
                assert not coef[c, s].any() and (s < ns or not test_z[c].any()), (key(rec), C, kind, s)
                continue
            worst_w = max(worst_w, float(np.abs(coef[c, s] - want).max() / np.abs(want).max()))
            if s == ns:
                worst_z = max(worst_z, float((np.abs(test_z[c] - rec['test_z'][c].numpy()) / decision_scale(tx, want)).max()))
    return worst_w, worst_z


def test_coefficients_and_decision_values(recorded, device):
    """(b) Against the recorded f64 fits, bounds 4 x the committed measurement (profiles/r17_logistic_bounds_measured.json, per problem: conditioning varies
    between them by orders of magnitude -- the intercept of an l2 fit at C = 1e-5 is determined by a sum that f32 holds to 2^-24 of 1/2)."""
    got = {key(rec): dict(zip(('coef', 'decision'), measure(rec, recorded['cands'], device[key(rec)]))) for rec in recorded['problems']}
    for k, v in got.items():
        print(f'{k}: coefficients {v["coef"]:.3e} of max |w|, decision values {v["decision"]:.3e} of |b| + sum |w_j x_j|')
    if os.environ.get('PFN_LOGISTIC_MEASURE'):
        with open(os.environ['PFN_LOGISTIC_MEASURE'], 'w') as f:
            json.dump(got, f, indent=1, sort_keys=True)
    committed = json.load(open(MEASURED))
    for k, v in got.items():
        for what, label in (('coef', 'coefficients'), ('decision', 'decision values')):
            if committed[k][what] == 0:
                assert v[what] == 0, (k, what)      # (measured as exact: it stays exact)
            else:
                bounds.within(f'{label} {k}', v[what], 4 * committed[k][what])


def windows(rec, cands, bound):
    """Per fit (c, s < n_splits) of a problem: (f64-correct rows outside the flip window, rows inside it, held-out rows) -- a held-out row may flip where its
    f64 decision value lies within `bound` of its scale."""
    x, cls, folds, ns = rec['x'].numpy(), rec['y'].numpy() > 0.5, rec['folds'].numpy(), rec['n_splits']
    out = {}
    for c in range(len(cands)):
        for s in range(ns):
            held = folds == s
            z, w = rec['cv_z'][c].numpy()[held], rec['coef'][c, s].numpy()
            inside = np.abs(z) <= bound * decision_scale(x[held], w)
            out[c, s] = (int((((z > 0) == cls[held]) & ~inside).sum()), int(inside.sum()), int(held.sum()))
    return out


def test_counts(recorded, device):
    """(c) cv_correct is the f64 count, except that a held-out row whose f64 decision value lies within the bound asserted in (b) of its scale may flip; such rows
    are at most 1 % of a problem's held-out (row, fit) pairs.  A fit with w = 0 exactly gives z == 0 exactly: class 0, the f64 count.  Fits without an optimum
    ('none' on separable rows, and 'none' wherever (b) does not compare it) end at iterates of their own in f32 and f64: their counts are only checked to be
    counts."""
    committed = json.load(open(MEASURED))
    cands = recorded['cands']
    zero_fits = 0
    for rec in recorded['problems']:
        cvc, _, status, coef = device[key(rec)]
        ns, cls, folds = rec['n_splits'], rec['y'].numpy() > 0.5, rec['folds'].numpy()
        bound = 4 * committed[key(rec)]['decision']
        inside_total = pairs = 0
        for (c, s), (sure, inside, size) in windows(rec, cands, bound).items():
            want, reason = int(rec['cv_correct'][c, s]), int(rec['status'][c, s, 0])
            if reason == lf.ONE_CLASS:
                assert status[c, s, 0] == lf.ONE_CLASS and cvc[c, s] == 0
            elif not rec['coef'][c, s].numpy().any():
                zero_fits += 1
                assert not coef[c, s].any() and cvc[c, s] == want == int((~cls[folds == s]).sum()), (key(rec), cands[c], s)
            elif has_optimum(rec, c, s, cands[c][1]):
                pairs, inside_total = pairs + size, inside_total + inside
                assert sure <= cvc[c, s] <= sure + inside, (key(rec), cands[c], s, cvc[c, s], want)
            else:
                assert 0 <= cvc[c, s] <= size
        assert not cvc[:, ns:].any()
        print(f'{key(rec)}: {inside_total} of {pairs} held-out (row, fit) pairs within {bound:.1e} of their scale')
        assert inside_total <= 0.01 * pairs
    assert zero_fits > 0


def test_pipeline_matches_the_recorded_grid_search(recorded, device):
    """(d) logistic_metric.batched on the recorded problems: the best parameters, predict_proba to the decision bound of (b) through the sigmoid (slope 1/4), and
    the ROC-AUC -- equal to the recorded ratio unless two test rows of opposite class have f64 decision values closer than the bound allows to tell apart."""
    committed = json.load(open(MEASURED))
    entries = lf.grid_entries()
    t = lambda a: torch.from_numpy(a).to(DEV)
    for rec in recorded['problems']:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')      # (a one-class test column: its AUC is NaN, on both sides)
            metric, proba, params = tabular.logistic_metric.batched(t(rec['x'].numpy())[:, None], t(rec['y'].numpy())[:, None], t(rec['test_x'].numpy())[:, None],
                                                                    t(rec['test_y'].numpy())[:, None], return_params=True)
        assert params[0] == entries[rec['best']], (key(rec), params[0], entries[rec['best']])
        best_fit = int(recorded['entry_fit'][rec['best']])
        w = rec['coef'][best_fit, rec['n_splits']].numpy()
        scale = decision_scale(rec['test_x'].numpy(), w)
        bound = 4 * committed[key(rec)]['decision']
        want = rec['proba'].numpy()
        assert proba.shape == (rec['T'], 1) and (np.abs(proba[:, 0] - want) <= 0.25 * bound * scale + 2e-16).all()
        if not w.any():
            assert (proba == 0.5).all()
        P, Nn, gt, eq = rec['auc_counts']
        if P == 0 or Nn == 0:
            assert np.isnan(metric[0]) and np.isnan(rec['auc'])
            continue
        z, pos = rec['test_z'][best_fit].numpy(), rec['test_y'].numpy() > 0.5
        # (f32 scores reach the pair count: a pair is also unclear where its probabilities are within 2^-23 of each other)
        unclear = (np.abs(z[pos][:, None] - z[~pos][None, :]) <= bound * (scale[pos][:, None] + scale[~pos][None, :]) + 8 * EPS) & (z[pos][:, None] != z[~pos][None, :])
        assert abs(metric[0] - rec['auc']) <= unclear.sum() / (P * Nn) + 1e-15, (key(rec), metric[0], rec['auc'])
        # the single-problem form is the batched form's column
        if rec['n'] == 33:
            one, one_proba = tabular.logistic_metric(t(rec['x'].numpy()), t(rec['y'].numpy()), t(rec['test_x'].numpy()), t(rec['test_y'].numpy()), [])
            assert one == metric[0] and np.array_equal(one_proba, proba[:, 0])


@pytest.mark.parametrize('n,F,T', [(10, 3, 20), (33, 8, 7), (80, 60, 20)])
def test_a_fit_is_a_function_of_its_own_problem_and_candidate(recorded, n, F, T):
    """(e) A problem alone is bit-equal to the same problem inside a batch; a candidate alone is bit-equal to the same candidate inside the grid."""
    cands, ns = recorded['cands'], min(5, n // 2)
    probs = [lf.problem(n, F, T, seed) for seed in (n + 1, n + 2, n + 3)]
    x, y, tx = (np.stack([p[i] for p in probs]) for i in range(3))
    folds = np.stack([tabular._stratified_folds(p[1] > 0.5, ns) for p in probs])
    batch = run(x, y, tx, folds, ns, cands)
    for w in (0, 2):
        alone = run(x[w:w + 1], y[w:w + 1], tx[w:w + 1], folds[w:w + 1], ns, cands)
        for a, b in zip(alone, batch):
            assert a[0].tobytes() == b[w].tobytes()
    for c in (0, 7, len(cands) - 1):
        alone = run(x, y, tx, folds, ns, cands[c:c + 1])
        for a, b in zip(alone, batch):
            assert a[:, 0].tobytes() == b[:, c].tobytes()


EVERY_KIND = [(C, pen | icpt) for pen in (lf.L1, lf.L2, lf.NONE) for icpt in (0, lf.FIT_INTERCEPT) for C in (0.01, 1.0)]


def test_a_column_that_is_zero_on_the_training_rows_gets_an_exact_zero(recorded, device):
    """(f) The recorded problems' column 1 is zero on every row; here column 2 is also zero on the training rows of fold slot 0 only."""
    for rec in recorded['problems']:
        if rec['F'] >= 3:
            assert not device[key(rec)][3][:, :, 1].any()
    n, F, T, ns = 24, 4, 5, 3
    x, y, tx, _ = lf.problem(n, F, T, 7)
    folds = tabular._stratified_folds(y > 0.5, ns)
    x = x.copy()
    x[folds != 0, 2] = 0      # alive only where slot 0 does not train
    _, tz, status, coef = (a[0] for a in run(x[None], y[None], tx[None], folds[None], ns, EVERY_KIND))
    assert (status[:, :ns + 1, 0] != lf.ONE_CLASS).all() and np.isfinite(coef).all() and np.isfinite(tz).all()
    assert not coef[:, :, 1].any() and not coef[:, 0, 2].any()
    big = [c for c, (C, kind) in enumerate(EVERY_KIND) if C == 1.0 and kind & 3 != lf.L1]
    assert (coef[big][:, 1:ns + 1, 2] != 0).all()      # (the other slots do use it)


def test_duplicated_rows_with_opposite_labels(recorded):
    """(f) Every row twice, once per class: no penalty is needed for an optimum (w = 0, b = 0 by symmetry), every fit converges and certifies."""
    n, F, T, ns = 20, 3, 4, 5
    half, _, tx, _ = lf.problem(n // 2, F, T, 11)
    x = np.concatenate([half, half])
    y = np.concatenate([np.zeros(n // 2, dtype=np.float32), np.ones(n // 2, dtype=np.float32)])
    folds = tabular._stratified_folds(y > 0.5, ns)
    cvc, tz, status, coef = (a[0] for a in run(x[None], y[None], tx[None], folds[None], ns, EVERY_KIND))
    assert (status[:, :ns + 1, 0] == lf.CONVERGED).all() and np.isfinite(coef).all() and np.isfinite(tz).all()
    for c, (C, kind) in enumerate(EVERY_KIND):
        assert np.abs(coef[c, ns]).max() <= 1e-5      # the refit sees every row twice
        for s in range(ns + 1):
            mask = np.ones(n) if s == ns else (folds != s).astype(np.float64)
            assert lf.kkt(x, y, mask, coef[c, s].astype(np.float64), C, kind) <= (64 + n) * EPS * lf.effective_C(C, kind) * lf.scale(x, mask, kind)


def test_none_on_a_separable_table_ends_capped_and_finite():
    n, F, T, ns = 16, 2, 6, 4
    rng = np.random.RandomState(3)
    x = rng.randn(n, F).astype(np.float32)
    x[:, 0] += np.where(np.arange(n) % 2, 2.5, -2.5).astype(np.float32)
    y = (x[:, 0] > 0).astype(np.float32)
    tx = rng.randn(T, F).astype(np.float32)
    folds = tabular._stratified_folds(y > 0.5, ns)
    cands = [(1.0, lf.NONE), (1.0, lf.NONE | lf.FIT_INTERCEPT), (1.0, lf.L2 | lf.FIT_INTERCEPT)]
    cvc, tz, status, coef = (a[0] for a in run(x[None], y[None], tx[None], folds[None], ns, cands))
    assert (status[:2, :ns + 1, 0] == lf.CAPPED).all() and (status[:2, :ns + 1, 1] == 48).all() and (status[2, :ns + 1, 0] == lf.CONVERGED).all()
    assert np.isfinite(coef).all() and np.isfinite(tz).all() and np.abs(coef[:2, :ns + 1]).max() > 5
    assert (cvc[:, :ns] >= 0).all() and (cvc[:, :ns] <= np.bincount(folds, minlength=ns)).all() and not cvc[:, ns:].any()


def test_a_single_class_training_fold_says_so_and_scores_nan():
    n, F, T = 8, 2, 3
    x, _, tx, _ = lf.problem(n, F, T, 5)
    y = np.array([1, 1, 0, 0, 0, 0, 0, 0], dtype=np.float32)
    folds = np.array([0, 0, 1, 1, 1, 0, 0, 1], dtype=np.int32)      # both positives in fold 0: slot 0 trains on one class
    cands = [(1.0, lf.L2 | lf.FIT_INTERCEPT), (0.1, lf.L1)]
    cvc, tz, status, coef = (a[0] for a in run(x[None], y[None], tx[None], folds[None], 2, cands))
    assert (status[:, 0, 0] == lf.ONE_CLASS).all() and (status[:, 0, 1] == 0).all() and not coef[:, 0].any() and (cvc[:, 0] == 0).all()
    assert (status[:, 1:3, 0] == lf.CONVERGED).all() and not status[:, 3:].any() and np.isfinite(tz).all()
    mean, best, proba = tabular._logistic_select(cvc, status, folds, 2, np.array([0, 1]), tz)
    assert np.isnan(mean).all() and best == 0 and np.isfinite(proba).all()      # fold 0 fails for every candidate: every mean is NaN, entry 0 is refit (as sklearn)
    status[1, 0, 0] = lf.CONVERGED      # (were one candidate's fold sound, its mean would be a number and it would win)
    mean, best, _ = tabular._logistic_select(cvc, status, folds, 2, np.array([0, 1]), tz)
    assert np.isnan(mean[0]) and not np.isnan(mean[1]) and best == 1


def test_a_single_class_window_raises():
    g = torch.Generator().manual_seed(0)
    x, tx = torch.randn(8, 3, generator=g).to(DEV), torch.randn(2, 3, generator=g).to(DEV)
    with pytest.raises(ValueError, match='one class'):
        tabular.logistic_metric(x, torch.ones(8, device=DEV), tx, torch.zeros(2, device=DEV), [])
    with pytest.raises(ValueError, match='window 1'):
        tabular.logistic_metric.batched(torch.stack([x, x], 1), torch.stack([torch.tensor([0., 1.] * 4), torch.zeros(8)], 1).to(DEV), torch.stack([tx, tx], 1),
                                        torch.zeros(2, 2, device=DEV))


def test_evaluate_runs_the_logistic_arm_end_to_end():
    """(g) evaluate with logistic_metric on the diabetes rows: the reference's result keys, finite AUCs, probabilities."""
    d = torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_diabetes.pt'))
    positions = [10, 20]
    res = tabular.evaluate([['diabetes', d['X'], d['y'], []]], tabular.logistic_metric, 'logistic', 30, positions, DEV, max_samples=6)
    keys = {'metric', 'mean_metric', 'diabetes_time'} | {f'mean_metric_at_{p}' for p in positions}
    keys |= {f'diabetes_{k}_at_{p}' for p in positions for k in ('mean_metric', 'per_ds_metric', 'outputs', 'ys')}
    assert set(res) == keys and res['metric'] == 'auc'
    for p in positions:
        per_window, outputs = res[f'diabetes_per_ds_metric_at_{p}'], res[f'diabetes_outputs_at_{p}']
        assert per_window.shape == (6,) and outputs.shape == (30 - p, 6) and outputs.dtype == np.float64
        assert np.isfinite(per_window).all() and ((outputs >= 0) & (outputs <= 1)).all()      # (sigmoid in f64: 'none' on separable rows can round to 0 or 1)
        assert np.isfinite(res[f'diabetes_mean_metric_at_{p}']) and 0 <= res[f'mean_metric_at_{p}'] <= 1
    assert np.isfinite(res['mean_metric'])
