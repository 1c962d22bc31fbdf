"""The logistic-regression baseline of the tabular study restated in f64 numpy (csrc/logistic.hip, tabular.logistic_metric): the proximal-Newton solver, the
optimality certificate of any coefficient vector, the grid of the reference and the grid search over it, and the seeded problems of the tests.  No GPU, no
scikit-learn.  `fit(..., dtype=np.float32)` runs the same algorithm with the kernel's caps and constants in f32, to see what that precision allows.

Objective (scikit-learn's):  C sum_i m_i softplus(-y_i z_i) + r(w),  z = x w + b,  y in {-1, +1},  r = 1/2 |w|^2 (l2), |w|_1 (l1), 0 (none, where C = 1);
the intercept is never penalised.  A coefficient vector has F + 1 entries: the weights, then the intercept (0 without one)."""
import numpy as np

from tabular_cases import problem  # noqa: F401  (the seeded problems of the fixtures, shared with the other arm)

NONE, L1, L2, FIT_INTERCEPT = 0, 1, 2, 4      # hipops.LOGIT_*
UNUSED, CONVERGED, STALLED, CAPPED, ONE_CLASS, NONFINITE = 0, 1, 2, 3, 4, 5
PENALTIES = {'none': NONE, None: NONE, 'l1': L1, 'l2': L2}
EPS32 = 2.0 ** -23

# the reference's param_grid['logistic'] (tabular.py:325), restated here so that the tests do not take the code under test's word for it
PARAM_GRID = {'solver': ['saga'], 'penalty': ['l1', 'l2', 'none'], 'tol': [1e-2, 1e-4, 1e-10], 'max_iter': [500], 'fit_intercept': [True, False],
              'C': [1e-5, 0.001, 0.01, 0.1, 1.0, 2.0]}
SHAPES = [(4, 1, 1), (5, 3, 2), (10, 3, 20), (33, 8, 7), (80, 60, 20), (128, 128, 128)]      # (n, F, T)


def effective_C(C, kind):
    return 1.0 if (kind & 3) == NONE else float(C)


def design(X, kind):
    """The columns a fit uses: the features and, with an intercept, a column of ones."""
    X = np.asarray(X, dtype=np.float64)
    return np.concatenate([X, np.ones((len(X), 1))], 1) if kind & FIT_INTERCEPT else X


def scale(X, mask, kind):
    """max_j sum_i m_i |x_ij| over the used columns: what the stopping rule and every bound of the tests are relative to."""
    return float((np.abs(design(X, kind)) * np.asarray(mask, dtype=np.float64)[:, None]).sum(0).max())


def signs(y):
    return np.where(np.asarray(y) > 0.5, 1.0, -1.0)


def _sigma_neg_margin(ys, z):
    """sigma(-y z), stable."""
    a = -ys * z
    e = np.exp(-np.abs(a))
    hi, lo = 1 / (1 + e), e / (1 + e)
    return np.where(a >= 0, hi, lo), hi * lo


def kkt(X, y, mask, w, C, kind):
    """The f64 optimality certificate of the coefficient vector w [F+1]: the infinity norm of the minimum-norm subgradient of the objective at w."""
    X, w, mask = np.asarray(X, dtype=np.float64), np.asarray(w, dtype=np.float64), np.asarray(mask, dtype=np.float64)
    F, pen, C = X.shape[1], kind & 3, effective_C(C, kind)
    A = design(X, kind)
    d = A.shape[1]
    ys = signs(y)
    p, _ = _sigma_neg_margin(ys, A @ w[:d])
    g = A.T @ (-C * mask * ys * p)
    r = np.abs(g)
    if pen == L2:
        r[:F] = np.abs(g[:F] + w[:F])
    elif pen == L1:
        r[:F] = np.where(w[:F] != 0, np.abs(g[:F] + np.sign(w[:F])), np.maximum(np.abs(g[:F]) - 1, 0))
    return float(r.max())


def fit(X, y, mask, C, kind, dtype=np.float64):
    """Proximal Newton from w = 0 as the kernel runs it; in f64 with a stopping threshold of 1e-13 of the scale and caps wide enough never to bind on a problem
    that has an optimum.  Returns (w [F+1] f64, exit reason, iterations)."""
    f32 = dtype == np.float32
    T_ = dtype
    X = np.asarray(X, dtype=np.float64)
    n, F = X.shape
    pen, C = kind & 3, T_(effective_C(C, kind))
    A = design(X, kind).astype(T_)
    d = A.shape[1]
    ys, m = signs(y).astype(T_), np.asarray(mask).astype(T_)
    out = np.zeros(F + 1)
    if not ((ys[m > 0] > 0).any() and (ys[m > 0] < 0).any()):
        return out, ONE_CLASS, 0
    mass = (np.abs(A) * m[:, None]).sum(0)
    act = mass > 0
    thr = T_(64 * EPS32 if f32 else 1e-13) * C * mass.max()
    max_outer, max_sweeps, max_bt = (48, 50, 30) if f32 else (200, 2000, 60)
    damp = T_(2.0 ** -16 if f32 else 2.0 ** -40)
    penalised = np.arange(d) < F
    w = np.zeros(d, dtype=T_)
    reason, it, polished = CAPPED, 0, False
    for it in range(max_outer + 1):
        p, pq = _sigma_neg_margin(ys, A @ w)
        p, pq = p.astype(T_), pq.astype(T_)
        g = A.T @ (-C * m * ys * p)
        Dw = C * m * pq
        hd = (A * A * Dw[:, None]).sum(0)
        if pen == L2:
            g = g + np.where(penalised, w, 0)
            hd = hd + penalised
        g = np.where(act, g, 0).astype(T_)
        hd = np.where(act, hd, 1).astype(T_)
        if pen == L1:
            r = np.where(penalised, np.where(w != 0, np.abs(g + np.sign(w)), np.maximum(np.abs(g) - 1, 0)), np.abs(g))
        else:
            r = np.abs(g)
        r = np.where(act, r, 0)
        k = r.max()
        # without a penalty, a w that separates the training rows proves that no optimum exists: its small residual certifies nothing, the fit goes on to the cap
        separates = pen == NONE and bool((ys * (A @ w) > 0)[m > 0].all())
        met = bool(k <= thr) and not separates
        if not k > thr and not k <= thr:
            reason = NONFINITE
            break
        # the first iterate that meets the threshold is followed by one more Newton step (the residual falls quadratically there: the step costs one iteration and
        # leaves the coefficients at the precision's floor, not at the threshold); the fit ends at the next iterate that meets it
        if met and polished:
            reason = CONVERGED
            break
        polished = met
        if it == max_outer:
            reason = CONVERGED if met else CAPPED
            break
        tau = T_(0) if pen == L2 else damp * hd.sum() / T_(d)      # l2: H is positive definite as it stands
        H = (A.T * Dw) @ A
        if pen == L2:
            H[np.arange(F), np.arange(F)] += 1
        H[np.arange(d), np.arange(d)] += tau
        H[~act, :] = 0
        H[:, ~act] = 0
        H[~act, ~act] = 1
        H = H.astype(T_)
        if pen != L1:
            try:
                L = np.linalg.cholesky(H.astype(np.float64))
                delta = -np.linalg.solve(L.T, np.linalg.solve(L, g.astype(np.float64)))
            except np.linalg.LinAlgError:
                delta = np.full(d, np.nan)
            delta = np.where(act, delta, 0).astype(T_)
        else:
            delta, q = np.zeros(d, dtype=T_), np.zeros(d, dtype=T_)
            live = np.flatnonzero(act)
            for _ in range(max_sweeps):
                moved = T_(0)
                for j in live:
                    hj, cur = H[j, j], w[j] + delta[j]
                    v, th = cur - (g[j] + q[j]) / hj, 1 / hj
                    u = v if j >= F else (v - th if v > th else (v + th if v < -th else T_(0)))
                    dz = u - cur
                    if dz != 0:
                        delta[j] = u - w[j]
                        q += dz * H[j]
                    moved = max(moved, abs(dz) * hj)
                if not moved > T_(0.25) * thr:
                    break
        model = (g * delta).sum()
        if pen == L1:
            model = model + (np.abs(w + delta) - np.abs(w))[:F].sum()
        xd = A @ delta
        t, moved_on = T_(1), False
        if model < 0:
            for _ in range(max_bt):
                with np.errstate(over='ignore', invalid='ignore'):
                    df = (C * m * np.log1p(p * np.expm1(-ys * t * xd)))[m > 0].sum()
                nw = w + t * delta
                if pen == L2:
                    df = df + (t * delta * (w + T_(0.5) * t * delta))[:F].sum()
                elif pen == L1:
                    same = (w != 0) & (nw != 0) & ((nw > 0) == (w > 0))
                    df = df + np.where(same, np.sign(w) * t * delta, np.abs(nw) - np.abs(w))[:F].sum()
                if df <= T_(1e-4) * t * model:
                    moved_on = True
                    break
                t = t * T_(0.5)
        if not moved_on:
            reason = CONVERGED if met else STALLED
            break
        w = nw.astype(T_)
    out[:d] = w
    return out, reason, it


# ---- the grid ------------------------------------------------------------------------------------------------------------------------------------------------
def grid_entries(param_grid=None):
    """The parameter dicts in sklearn.model_selection.ParameterGrid order: keys sorted, the last key varying fastest."""
    import itertools
    param_grid = PARAM_GRID if param_grid is None else param_grid
    keys = sorted(param_grid)
    return [dict(zip(keys, values)) for values in itertools.product(*(param_grid[k] for k in keys))]


def distinct_fits(entries):
    """tol, max_iter and solver do not change a fit that is solved to its optimum and 'none' ignores C: the distinct (C, kind) pairs in order of first
    appearance, and every entry's index into them."""
    cands, index, where = [], [], {}
    for e in entries:
        pen = PENALTIES[e['penalty']]
        kind = pen | (FIT_INTERCEPT if e['fit_intercept'] else 0)
        key = (1.0 if pen == NONE else float(e['C']), kind)
        if key not in where:
            where[key] = len(cands)
            cands.append(key)
        index.append(where[key])
    return cands, np.asarray(index)


def select(cv_correct, one_class, folds, n_splits, entry_fit):
    """GridSearchCV's arithmetic: cv_correct [NC, >= n_splits] counts, one_class [NC, >= n_splits] bool (the fold's fit was not run: its score is NaN).  A fold's
    score is correct / size, a candidate's the mean over folds, the best entry the FIRST maximum over the entries (NaN ranks last).
    Returns (mean_test_score [entries] f64, best entry index)."""
    sizes = np.bincount(np.asarray(folds), minlength=n_splits)[:n_splits].astype(np.float64)
    scores = np.asarray(cv_correct, dtype=np.float64)[:, :n_splits] / sizes
    scores[np.asarray(one_class)[:, :n_splits]] = np.nan
    mean = scores.mean(axis=1)[np.asarray(entry_fit)]
    ranked = np.where(np.isnan(mean), -np.inf, mean)
    return mean, int(np.argmax(ranked))


def solve_problem(x, y, test_x, folds, n_splits, cands, dtype=np.float64):
    """Every fit of one problem: coef [NC, 6, F+1], status [NC, 6, 2], cv_z [NC, n] (each row's decision value under the fit that holds it out; NaN where that
    fit was not run), cv_correct [NC, 5], test_z [NC, T]."""
    x, test_x, folds = np.asarray(x, dtype=np.float64), np.asarray(test_x, dtype=np.float64), np.asarray(folds)
    n, F = x.shape
    cls = np.asarray(y) > 0.5
    coef, status = np.zeros((len(cands), 6, F + 1)), np.zeros((len(cands), 6, 2), dtype=np.int64)
    cv_z, cv_correct, test_z = np.full((len(cands), n), np.nan), np.zeros((len(cands), 5), dtype=np.int64), np.zeros((len(cands), len(test_x)))
    for c, (C, kind) in enumerate(cands):
        for s in range(n_splits + 1):
            mask = np.ones(n) if s == n_splits else (folds != s).astype(np.float64)
            w, reason, it = fit(x, y, mask, C, kind, dtype=dtype)
            coef[c, s], status[c, s] = w, (reason, it)
            if s == n_splits:
                test_z[c] = test_x @ w[:F] + w[F] if reason != ONE_CLASS else np.nan
            elif reason != ONE_CLASS:
                held = folds == s
                z = x[held] @ w[:F] + w[F]
                cv_z[c, held] = z
                cv_correct[c, s] = int(((z > 0) == cls[held]).sum())
    return coef, status, cv_z, cv_correct, test_z
