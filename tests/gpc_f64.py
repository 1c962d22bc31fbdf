"""The GP-classifier baseline of the tabular study restated in f64 numpy (csrc/gpc.hip, tabular.gp_metric): scikit-learn's binary Laplace
GaussianProcessClassifier under c * RBF(l) -- the posterior mode (GPML algorithm 3.1), the log marginal likelihood Z and its gradient in theta = (log c, log l)
(algorithm 5.1), the decision values as pairs (m, e) with f* = m exp(-e), the predictive variance, the five-term erf mixture -- and the grid of the reference, the
selection of the grid search and the seeded problems of the tests.  No GPU, no scikit-learn (tools/record_gpc_fixtures.py checks this file against it).
`dtype=np.float32` runs the same formulas in f32 with the kernel's stopping rule, to see what that precision allows.

In f64 the mode search is scikit-learn's to the letter: it stops when Z rises by less than 1e-10 (or falls), returns the Z of the iteration BEFORE the one that
stopped it, and leaves pi, W and L of the last iteration, one step behind f."""
import itertools
import math

import numpy as np

from tabular_cases import problem  # noqa: F401  (the seeded problems of the fixtures, shared with the other arm)

UNUSED, CONVERGED, CAPPED, ONE_CLASS, NONPOSITIVE, NONFINITE = 0, 1, 2, 3, 4, 5      # hipops.GPC_*
MAX_NEWTON = 100
STOP32, EXTRA32 = 2.0 ** -20, 2      # the kernel's stopping level (of max(1, |Z|)) and the iterations it runs beyond it
BOX = (math.log(1e-5), math.log(1e5))

# the reference's param_grid['gp'] (tabular.py:480): kernel = c * RBF(l) over itertools.product(CS, LS), restated so that the tests do not take the code under
# test's word for it
CS = [0.05, 0.1, 0.5, 1, 5, 10]
LS = [0.1, 0.5, 1, 2]
SHAPES = [(4, 1, 1), (5, 3, 2), (10, 3, 20), (33, 8, 7), (80, 60, 20), (112, 128, 128)]      # (n, F, T): the last is the kernel's cap

# Williams & Barber's five-term erf approximation of the logistic sigmoid, as sklearn.gaussian_process._gpc has it
LAMBDAS = np.array([0.41, 0.4, 0.37, 0.44, 0.39])[:, None]
COEFS = np.array([-1854.8214151, 3516.89893646, 221.29346712, 128.12323805, -2010.49422654])[:, None]


def grid():
    """The 24 candidates (c, l) in the reference's order."""
    return [(float(c), float(l)) for c, l in itertools.product(CS, LS)]


def grid_theta():
    return np.log(np.asarray(grid(), dtype=np.float64))


def attach_rows(rec, wrap):
    """A recorded seeded problem holds its seed, not its rows: draw them again into rec['x'], rec['test_x'] (as wrap(numpy array)) and check the labels."""
    if 'x' not in rec:
        x, y, test_x, test_y = problem(rec['n'], rec['F'], rec['T'], rec['seed'])
        assert np.array_equal(y, np.asarray(rec['y'])) and np.array_equal(test_y, np.asarray(rec['test_y']))
        rec['x'], rec['test_x'] = wrap(x), wrap(test_x)
    return rec


def extra_thetas(seed):
    """Eight further theta per problem with log c <= 5: away from the grid, towards the box's edges in l."""
    rng = np.random.RandomState(1000 + seed)
    t = np.stack([rng.uniform(-6, 5, 8), rng.uniform(-2.3, 3, 8)], 1)
    t[0] = (5.0, 11.5)
    t[1] = (-11.5, 1.5)
    t[2] = (2.0, BOX[1])
    return t


def corners():
    return np.array([(a, b) for a in BOX for b in BOX])


def exponent_args(xa, xb, theta, dtype=np.float64):
    """d^2 / 2 l^2 of every row of xa against every row of xb."""
    xa, xb = np.asarray(xa).astype(dtype), np.asarray(xb).astype(dtype)
    length = np.exp(dtype(theta[1]))
    d2 = ((xa[:, None, :] - xb[None, :, :]) ** 2).sum(-1, dtype=dtype)
    return d2 * (dtype(0.5) / (length * length))


def _softplus(z):
    return np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))


def mode(K, y, dtype=np.float64):
    """GPML algorithm 3.1 from f = 0.  Returns dict(Z, pi, sw, L, a, f, reason, iters)."""
    f32 = dtype == np.float32
    n = len(y)
    y = np.asarray(y).astype(dtype)
    K = K.astype(dtype)
    f = np.zeros(n, dtype)
    Z, t_prev, left, reason, out = -np.inf, None, -1, CAPPED, None
    sgn = np.where(y > 0.5, -1, 1).astype(dtype)
    for it in range(1, MAX_NEWTON + 1):
        e = np.exp(-np.abs(f))
        hi = 1 / (1 + e)
        lo = e * hi
        pi, W = np.where(f >= 0, hi, lo), hi * lo
        sw = np.sqrt(W)
        B = np.eye(n, dtype=dtype) + sw[:, None] * K * sw[None, :]
        try:
            L = np.linalg.cholesky(B)
        except np.linalg.LinAlgError:
            return dict(Z=np.inf, reason=NONPOSITIVE, iters=it)
        b = W * f + (y - pi)
        z = np.linalg.solve(L, sw * (K @ b))
        a = b - sw * np.linalg.solve(L.T, z)
        f = K @ a
        t = dtype(-0.5) * a * f - _softplus(sgn * f) - np.log(np.diag(L))
        Z_new = t.sum(dtype=dtype)
        out = dict(pi=pi, sw=sw, L=L, a=a, f=f, iters=it)
        if f32:
            dZ = (t - t_prev).sum(dtype=dtype) if t_prev is not None else np.inf
            t_prev, Z = t, Z_new
            if left > 0:
                left -= 1
                if left == 0:
                    reason = CONVERGED
                    break
            elif it > 1 and not dZ >= dtype(STOP32) * max(dtype(1), abs(Z)):
                left = EXTRA32
        else:
            if Z_new - Z < 1e-10:      # scikit-learn's: the returned Z stays the previous iteration's
                reason = CONVERGED
                break
            Z = Z_new
    if not np.isfinite(Z):
        return dict(Z=np.inf, reason=NONFINITE, iters=out['iters'])
    out.update(Z=float(Z), reason=reason)
    return out


def one_class(y):
    y = np.asarray(y) > 0.5
    return bool(y.all() or not y.any())


def lml_grad(x, y, theta, dtype=np.float64):
    """(Z, dZ/dtheta [2], (reason, iterations)) of the fit on rows x [m,F], labels y [m] at theta = (log c, log l)."""
    if one_class(y):
        return np.nan, np.zeros(2), (ONE_CLASS, 0)
    c = np.exp(dtype(theta[0]))
    U = exponent_args(x, x, theta, dtype)
    K = c * np.exp(-U)
    md = mode(K, y, dtype)
    if md['reason'] not in (CONVERGED, CAPPED):
        return np.inf, np.zeros(2), (md['reason'], md['iters'])
    pi, sw, L, a = md['pi'], md['sw'], md['L'], md['a']
    n = len(pi)
    Linv = np.linalg.solve(L, np.eye(n, dtype=dtype))
    R = sw[:, None] * (Linv.T @ Linv) * sw[None, :]
    C = Linv @ (sw[:, None] * K)
    s2 = dtype(-0.5) * (np.diag(K) - (C * C).sum(0)) * (pi * (1 - pi) * (1 - 2 * pi))
    r = np.asarray(y).astype(dtype) - pi
    grad = np.zeros(2)
    for j, Kj in enumerate((K, K * (2 * U))):
        s1 = 0.5 * a @ Kj @ a - 0.5 * (R * Kj).sum()
        bj = Kj @ r
        s3 = bj - K @ (R @ bj)
        grad[j] = s1 + s2 @ s3
    if not np.isfinite(grad).all():
        return np.inf, np.zeros(2), (NONFINITE, md['iters'])
    return md['Z'], grad, (md['reason'], md['iters'])


def decision(x, y, xq, theta, dtype=np.float64):
    """The fit on (x, y) at theta, asked at the rows xq [Q,F]: dict(m, e, var, mass [Q], reason, iters).  f* = m exp(-e); e is the smallest exponent argument
    over the training rows; mass = sum_i |c exp(e - U_i) (y_i - pi_i)| is what an error of m is a share of; var = c - |L^-1 W^1/2 k*|^2 (not clamped)."""
    Q = len(xq)
    nan = np.full(Q, np.nan)
    if one_class(y):
        return dict(m=nan, e=nan, var=nan, mass=nan, reason=ONE_CLASS, iters=0)
    c = np.exp(dtype(theta[0]))
    K = c * np.exp(-exponent_args(x, x, theta, dtype))
    md = mode(K, y, dtype)
    if md['reason'] not in (CONVERGED, CAPPED):
        return dict(m=nan, e=nan, var=nan, mass=nan, reason=md['reason'], iters=md['iters'])
    U = exponent_args(xq, x, theta, dtype)
    e = U.min(1)
    r = np.asarray(y).astype(dtype) - md['pi']
    terms = c * np.exp(e[:, None] - U) * r[None, :]
    v = np.linalg.solve(md['L'], md['sw'][:, None] * (c * np.exp(-U)).T)
    var = c - (v * v).sum(0)
    return dict(m=terms.sum(1), e=e, var=var, mass=np.abs(terms).sum(1), reason=md['reason'], iters=md['iters'])


def f_star(m, e):
    """The decision value from its pair, in f64."""
    return np.asarray(m, dtype=np.float64) * np.exp(-np.asarray(e, dtype=np.float64))


def proba(fs, var):
    """scikit-learn's predict_proba[:, 1] from the latent mean and variance: the five-term erf mixture, written with 1 / sqrt(1 + 2 var lambda^2) so that
    var = 0 (the kernel clamps there) is an ordinary argument.  The same number as scikit-learn's expression wherever var > 0."""
    fs, var = np.asarray(fs, dtype=np.float64), np.maximum(np.asarray(var, dtype=np.float64), 0)
    erf = np.vectorize(math.erf, otypes=[np.float64])
    integrals = 0.5 * erf(LAMBDAS * fs / np.sqrt(1 + 2 * var * LAMBDAS ** 2))
    return (COEFS * integrals).sum(0) + 0.5 * COEFS.sum()


def slot_rows(folds, n_splits, s):
    folds = np.asarray(folds)
    return np.ones(len(folds), dtype=bool) if s == n_splits else folds != s


def grid_search(x, y, test_x, folds, n_splits, thetas, dtype=np.float64):
    """Every fit of a grid search at the given thetas [NC, n_splits + 1 (or 6), 2]: dict(cv_f [NC,n,2] (NaN where no fit holds the row out), cv_mass [NC,n],
    test_f [NC,T,2], test_var [NC,T], test_mass [NC,T], status [NC,6,2])."""
    NC, n, T = len(thetas), len(y), len(test_x)
    cv_f, cv_mass = np.full((NC, n, 2), np.nan), np.full((NC, n), np.nan)
    test_f, test_var, test_mass = np.full((NC, T, 2), np.nan), np.full((NC, T), np.nan), np.full((NC, T), np.nan)
    status = np.zeros((NC, 6, 2), dtype=np.int32)
    for c in range(NC):
        for s in range(n_splits + 1):
            rows = slot_rows(folds, n_splits, s)
            xq = test_x if s == n_splits else x[~rows]
            d = decision(x[rows], y[rows], xq, thetas[c, s], dtype)
            status[c, s] = (d['reason'], d['iters'])
            if s == n_splits:
                test_f[c, :, 0], test_f[c, :, 1], test_var[c], test_mass[c] = d['m'], d['e'], d['var'], d['mass']
            else:
                cv_f[c, ~rows, 0], cv_f[c, ~rows, 1], cv_mass[c, ~rows] = d['m'], d['e'], d['mass']
    return dict(cv_f=cv_f, cv_mass=cv_mass, test_f=test_f, test_var=test_var, test_mass=test_mass, status=status)


def select(cv_f, status, folds, y, n_splits):
    """GridSearchCV's selection from the decision values: a fold's score is the accuracy of (f* > 0) on its rows in f64, NaN where the fit did not run (a
    one-class training part, error_score = nan); a candidate's score the mean over folds; the best the FIRST maximum, NaN ranking last.
    Returns (mean_test_score [NC], best index, correct counts [NC, n_splits])."""
    folds, cls = np.asarray(folds), np.asarray(y) > 0.5
    NC = len(cv_f)
    scores, correct = np.full((NC, n_splits), np.nan), np.zeros((NC, n_splits), dtype=np.int64)
    for c in range(NC):
        for s in range(n_splits):
            held = folds == s
            if status[c, s, 0] not in (CONVERGED, CAPPED):
                continue
            correct[c, s] = int(((f_star(cv_f[c, held, 0], cv_f[c, held, 1]) > 0) == cls[held]).sum())
            scores[c, s] = correct[c, s] / held.sum()
    mean = scores.mean(1)
    return mean, int(np.argmax(np.where(np.isnan(mean), -np.inf, mean))), correct


def project(theta, grad_neg_Z):
    """The projected gradient of -Z on the box: components that point out of it at a bound are zero."""
    theta, g = np.asarray(theta, dtype=np.float64), np.array(grad_neg_Z, dtype=np.float64)
    g[(theta <= BOX[0]) & (g > 0)] = 0
    g[(theta >= BOX[1]) & (g < 0)] = 0
    return g
