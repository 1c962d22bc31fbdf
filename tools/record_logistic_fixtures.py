"""Record the fixture of the logistic-regression tests (CPU only; scikit-learn is used for the cross-check alone):

    python tools/record_logistic_fixtures.py

tests/golden/tabular_logistic.pt   per shape of tests/logistic_f64.SHAPES one seeded problem (float32 inputs), StratifiedKFold's fold assignment, and what the f64
                                   restatement (tests/logistic_f64.py) makes of the reference's whole grid: the coefficients, exit status and held-out decision
                                   values of all 26 distinct fits x (folds + refit), the integer counts, mean_test_score over the 108 grid entries, the best
                                   entry, predict_proba[:, 1] of its refit and the ROC-AUC as a ratio of pair counts.
Conditions on a problem (the next seed, + 100, is tried until they hold):
  * the GPU decides (z > 0) in f32: the recorder runs the same solver in f32 numpy, takes 8 x its worst decision-value error (relative to |b| + sum_j |w_j x_j|)
    as the window in which a held-out row may flip, and wants at most 1 % of the (held-out row, fit) pairs of the problem inside it (fits with w = 0 exactly
    apart: their rows are exactly 0 in any precision);
  * no flip can change the best entry: the best fit has no row inside the window, and every fit that has some stays below the best score even with all of
    them counted in its favour.
Cross-check against scikit-learn, where it solves the same objective reliably: lbfgs at tol 1e-13 for l2 / None (None only where the f64 fit has an optimum),
liblinear at tol 1e-12 for l1 without intercept, saga at tol 1e-12 for l1 with intercept at C >= 0.1 (on the shapes with F <= 8: saga needs 1e5 epochs and more
beyond).  A scikit-learn fit whose own f64 certificate exceeds 1e-9 of the scale is left out and counted.  Asserted: coefficients to 1e-6 of max |w|, each fold's score, hence mean_test_score, and the best parameters among the cross-checked candidates."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import logistic_f64 as lf      # noqa: E402
from transformerscandobayesianinference_amd import tabular      # noqa: E402


def decision_scale(x, w):
    """|b| + sum_j |w_j x_j| per row: what a decision value's error is relative to."""
    F = x.shape[1]
    return np.abs(w[F]) + np.abs(x.astype(np.float64) * w[:F]).sum(1)


def flip_share(x, folds, n_splits, coef, cv_z, window):
    """The share of (held-out row, fit) pairs whose f64 decision value lies within `window` of its scale; fits with w = 0 exactly are left out."""
    inside = total = 0
    for c in range(coef.shape[0]):
        for s in range(n_splits):
            w = coef[c, s]
            held = folds == s
            if not w.any() or np.isnan(cv_z[c, held]).any():
                continue
            total += int(held.sum())
            inside += int((np.abs(cv_z[c, held]) <= window * decision_scale(x[held], w)).sum())
    return inside / max(total, 1)


def sklearn_fit(x, y, C, kind, has_optimum):
    """scikit-learn's solution of the same objective, or None where no solver of it is an oracle."""
    from sklearn.linear_model import LogisticRegression
    pen, icpt, F = kind & 3, bool(kind & lf.FIT_INTERCEPT), x.shape[1]
    if pen == lf.L2:
        clf = LogisticRegression(penalty='l2', C=C, fit_intercept=icpt, solver='lbfgs', tol=1e-13, max_iter=100000)
    elif pen == lf.NONE:
        if not has_optimum:
            return None
        clf = LogisticRegression(penalty=None, fit_intercept=icpt, solver='lbfgs', tol=1e-13, max_iter=100000)
    elif not icpt:
        clf = LogisticRegression(penalty='l1', C=C, fit_intercept=False, solver='liblinear', tol=1e-12, max_iter=100000)
    elif C >= 0.1 and F <= 8:
        clf = LogisticRegression(penalty='l1', C=C, fit_intercept=True, solver='saga', tol=1e-12, max_iter=2000000, random_state=0)
    else:
        return None
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        clf.fit(x.astype(np.float64), y.astype(np.int64))
    return clf


def cross_check(x, y, folds, n_splits, cands, coef, status, cv_correct):
    """Asserts the f64 restatement against scikit-learn; returns (fits compared, worst coefficient distance relative to max |w|)."""
    F, worst, compared, sk_mean, ours_mean = x.shape[1], 0., 0, {}, {}
    sizes = np.bincount(folds, minlength=n_splits).astype(np.float64)
    for c, (C, kind) in enumerate(cands):
        scores, whole = [], True
        for s in range(n_splits + 1):
            train = np.ones(len(y), dtype=bool) if s == n_splits else folds != s
            if status[c, s, 0] == lf.ONE_CLASS:
                whole = False
                continue
            clf = sklearn_fit(x[train], y[train], C, kind, status[c, s, 0] == lf.CONVERGED)
            if clf is None:
                whole = False
                continue
            w = np.concatenate([clf.coef_[0], np.atleast_1d(clf.intercept_)[:1] if kind & lf.FIT_INTERCEPT else [0.]])
            ones = np.ones(int(train.sum()))
            if lf.kkt(x[train], y[train], ones, w, C, kind) > 1e-9 * lf.effective_C(C, kind) * lf.scale(x[train], ones, kind):
                # scikit-learn stopped short of the optimum by its own certificate (lbfgs ends on its function-value test where the intercept's curvature is
                # far below the weights', C <= 0.001): no oracle for this fit
                whole = False
                cross_check.short += 1
                continue
            dist = np.abs(w - coef[c, s]).max() / max(np.abs(coef[c, s]).max(), 1e-300) if coef[c, s].any() else np.abs(w).max()
            # saga is the loosest of the three (a stochastic solver at tol 1e-12)
            assert dist <= 1e-6, f'candidate {(C, kind)} slot {s}: scikit-learn is {dist:.2e} of max |w| away'
            worst, compared = max(worst, dist), compared + 1
            if s < n_splits:
                held = folds == s
                scores.append(clf.score(x[held].astype(np.float64), y[held].astype(np.int64)))
                assert scores[-1] == cv_correct[c, s] / sizes[s], f'candidate {(C, kind)} fold {s}: score {scores[-1]} vs {cv_correct[c, s]} / {sizes[s]}'
        if whole:
            sk_mean[c] = float(np.mean(scores))
            ours_mean[c] = float((cv_correct[c, :n_splits] / sizes).mean())
            assert sk_mean[c] == ours_mean[c]
    if sk_mean:      # the best parameters among the cross-checked candidates: the first maximum, on both sides
        order = sorted(sk_mean)
        assert int(np.argmax([sk_mean[c] for c in order])) == int(np.argmax([ours_mean[c] for c in order]))
    return compared, worst


cross_check.short = 0


def record(n, F, T, first_seed, entries, cands, entry_fit):
    for seed in range(first_seed, first_seed + 5000, 100):
        x, y, test_x, test_y = lf.problem(n, F, T, seed)
        try:      # the folds as the product makes them: one problem through its preparation of many
            n_splits, (folds,), _, _ = tabular._fold_problems(*(torch.from_numpy(v)[:, None] for v in (x, y, test_x)))
        except ValueError:
            continue
        coef, status, cv_z, cv_correct, test_z = lf.solve_problem(x, y, test_x, folds, n_splits, cands)
        coef32, status32, cv_z32, _, test_z32 = lf.solve_problem(x, y, test_x, folds, n_splits, cands, dtype=np.float32)
        # the f32 run's worst decision-value error on the fits that have an optimum
        est = 0.
        for c in range(len(cands)):
            for s in range(n_splits):
                held = folds == s
                if status[c, s, 0] != lf.CONVERGED or not coef[c, s].any():
                    continue
                est = max(est, float((np.abs(cv_z32[c, held] - cv_z[c, held]) / decision_scale(x[held], coef[c, s])).max()))
        window = 8 * est
        share = flip_share(x, folds, n_splits, coef, cv_z, window)
        one_class = status[:, :, 0] == lf.ONE_CLASS
        mean, best = lf.select(cv_correct, one_class, folds, n_splits, entry_fit)
        if share > 0.01 or np.isnan(mean).all():
            print(f'  seed {seed}: {share:.2%} of the held-out pairs within {window:.1e} of their scale: next seed')
            continue
        sizes = np.bincount(folds, minlength=n_splits).astype(np.float64)
        flippable = np.zeros(len(cands))
        for c in range(len(cands)):
            for s in range(n_splits):
                held = folds == s
                if coef[c, s].any() and not np.isnan(cv_z[c, held]).any():
                    flippable[c] += (np.abs(cv_z[c, held]) <= window * decision_scale(x[held], coef[c, s])).sum()
        cand_mean = np.nan_to_num((cv_correct[:, :n_splits] / sizes).mean(1) + np.where(one_class[:, :n_splits].any(1), np.nan, 0), nan=-np.inf)
        reach = cand_mean + flippable / sizes.min() / n_splits
        b = entry_fit[best]
        if flippable[b] > 0 or ((flippable > 0) & (reach >= cand_mean[b])).any():
            print(f'  seed {seed}: a flip inside the window could change the best entry: next seed')
            continue
        z = test_z[entry_fit[best]]
        proba = 1 / (1 + np.exp(-z))
        pos, neg = proba[test_y > 0.5], proba[test_y <= 0.5]
        gt, eq = int((pos[:, None] > neg[None, :]).sum()), int((pos[:, None] == neg[None, :]).sum())
        auc = (2 * gt + eq) / (2. * len(pos) * len(neg)) if len(pos) and len(neg) else float('nan')
        compared, worst = cross_check(x, y, folds, n_splits, cands, coef, status, cv_correct)
        print(f'{(n, F, T)} seed {seed}: f32 run {est:.1e} away, {share:.2%} of the pairs within {window:.1e}; scikit-learn agrees on {compared} fits to {worst:.1e}; '
              f'best entry {best} {entries[best]} score {mean[best]:.4f} auc {auc:.4f}')
        t = torch.from_numpy
        return dict(n=n, F=F, T=T, seed=seed, x=t(x), y=t(y), test_x=t(test_x), test_y=t(test_y), folds=t(folds), n_splits=n_splits, coef=t(coef), status=t(status),
                    cv_z=t(cv_z), cv_correct=t(cv_correct), test_z=t(test_z), mean_test_score=t(mean), best=best, proba=t(proba), auc_counts=(len(pos), len(neg), gt, eq),
                    auc=auc, flip_window=window, f32_run_distance=est)
    raise SystemExit(f'no seed meets the conditions for problem {(n, F, T)}')


def main():
    entries, (cands, entry_fit) = lf.grid_entries(), lf.distinct_fits(lf.grid_entries())
    assert len(entries) == 108 and len(cands) == 26
    problems = [record(n, F, T, n, entries, cands, entry_fit) for n, F, T in lf.SHAPES]
    path = os.path.join(ROOT, 'tests', 'golden', 'tabular_logistic.pt')
    torch.save({'problems': problems, 'cands': cands, 'entry_fit': torch.from_numpy(entry_fit)}, path)
    print('recorded', len(problems), 'problems,', os.path.getsize(path), 'bytes;', cross_check.short, 'scikit-learn fits fell short of their own optimum and were left out')


if __name__ == '__main__':
    main()
