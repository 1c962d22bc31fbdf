"""The GP-classifier baseline on the MI355X (csrc/gpc.hip; tabular.gp_metric and what it calls) against the recorded f64 results of
tests/golden/tabular_gpc.pt: value and gradient of the Laplace log marginal likelihood, decision values and variances, the fixed grid search against the
recorded scikit-learn run, a certificate of the optimising pipeline, independence of batch and grid position, the edge rules, and `evaluate`.  Fixtures only: no
scikit-learn, no reference.  tests/gpc_f64.py holds the f64 restatement and the seeded problems.

PFN_GPC_MEASURE=<path> makes the tests write what they measured to <path> (one JSON object, a key per test); the committed copy is
profiles/r18_gpc_bounds_measured.json, and the bounds asserted here are 4 x its entries."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds      # noqa: E402
import gpc_f64 as gf      # noqa: E402

from transformerscandobayesianinference_amd import _hip, hipops, tabular      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -23
MEASURED = os.path.join(ROOT, 'profiles', 'r18_gpc_bounds_measured.json')
NAMES = ['n4_F1_T1', 'n5_F3_T2', 'n10_F3_T20', 'n33_F8_T7', 'n80_F60_T20', 'n112_F128_T128', 'diabetes_n30']
OK = (gf.CONVERGED, gf.CAPPED)
# what the f32 numpy emulation of the formulas gives over the box with log c <= 5: Z to 1e-6 of |Z|, the gradient to 2e-4 of its scale.  A
# committed measurement beyond ten times that is no measurement to multiply by 4
CEILING = dict(Z=1e-5, grad=2e-3)


def committed(section, name):
    return json.load(open(MEASURED))[section][name]


def note(section, name, values):
    """Add one entry to the file PFN_GPC_MEASURE names (read-modify-write: the tests of a session run one after the other)."""
    path = os.environ.get('PFN_GPC_MEASURE')
    if not path:
        return
    have = json.load(open(path)) if os.path.exists(path) else {}
    have.setdefault(section, {})[name] = values
    with open(path, 'w') as f:
        json.dump(have, f, indent=1, sort_keys=True)


def check4(section, name, got):
    """Every entry of `got` within 4 x its committed measurement (an entry measured as exactly 0 stays exactly 0)."""
    note(section, name, got)
    have = committed(section, name)
    for what, value in got.items():
        print(f'{section} {name}: {what} {value:.3e} (committed {have[what]:.3e})')
        if have[what] == 0:
            assert value == 0, (section, name, what)
        else:
            bounds.within(f'{section} {what} {name}', value, 4 * have[what])


@pytest.fixture(scope='module')
def recorded():
    d = torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_gpc.pt'), weights_only=False)
    assert [r['name'] for r in d['problems']] == NAMES
    for rec in d['problems']:
        gf.attach_rows(rec, torch.from_numpy)
    return {r['name']: r for r in d['problems']}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def per_slot(thetas):
    """theta [NC, 2] -> the kernel's [1, NC, 6, 2] f32, the same theta in every slot."""
    return dev(np.repeat(np.asarray(thetas, dtype=np.float32)[None, :, None, :], 6, 2))


def inputs(rec):
    return dev(rec['x'].numpy()[None]), dev(rec['y'].numpy()[None]), dev(rec['test_x'].numpy()[None]), dev(rec['folds'].numpy().astype(np.int32)[None])


@pytest.fixture(scope='module')
def device(recorded):
    """Both kernels on every recorded problem, once: name -> dict(value, grad, status [36, 6(, 2)] at the 32 recorded theta and the four corners of the box; cv_f,
    test_f, test_var, pstatus at the 32 recorded theta)."""
    out = {}
    for name, rec in recorded.items():
        x, y, tx, folds = inputs(rec)
        thetas = rec['thetas'].numpy()
        value, grad, status = hipops.gpc_lml_grad(per_slot(np.concatenate([thetas, gf.corners()])), x, y, folds, rec['n_splits'])
        cv_f, test_f, test_var, pstatus = hipops.gpc_predict(per_slot(thetas), x, y, tx, folds, rec['n_splits'])
        out[name] = dict(value=value[0].cpu().numpy(), grad=grad[0].cpu().numpy(), status=status[0].cpu().numpy(), cv_f=cv_f[0].cpu().numpy(),
                         test_f=test_f[0].cpu().numpy(), test_var=test_var[0].cpu().numpy(), pstatus=pstatus[0].cpu().numpy())
    return out


@pytest.mark.parametrize('name', NAMES)
def test_value_and_gradient_against_f64(name, recorded, device):
    """(a) -Z and -dZ/dtheta at the 24 starts and the 8 further theta (all with log c <= 5), every slot: the error of Z as a share of |Z|, the gradient's as a
    share of max(|dZ|_inf, 1e-3 |Z|); bounds 4 x the committed measurement.  At the four corners of the box only: finite outputs and a valid status."""
    rec, got = recorded[name], device[name]
    ns, Z, dZ = rec['n_splits'], rec['Z'].numpy(), rec['dZ'].numpy()
    assert (rec['thetas'].numpy()[:, 0] <= 5).all()
    worst_z = worst_g = 0.
    iters = 0
    for k in range(32):
        for s in range(6):
            reason, it = got['status'][k, s]
            if s > ns:
                assert reason == gf.UNUSED and got['value'][k, s] == 0 and not got['grad'][k, s].any()
            elif np.isnan(Z[k, s]):
                assert reason == gf.ONE_CLASS and np.isnan(got['value'][k, s]) and not got['grad'][k, s].any()
            else:
                assert reason in OK and 1 <= it <= hipops.GPC_MAX_NEWTON, (k, s, reason, it)
                iters = max(iters, it)
                worst_z = max(worst_z, abs(-got['value'][k, s] - Z[k, s]) / abs(Z[k, s]))
                worst_g = max(worst_g, np.abs(-got['grad'][k, s].astype(np.float64) - dZ[k, s]).max() / max(np.abs(dZ[k, s]).max(), 1e-3 * abs(Z[k, s])))
    print(f'{name}: at most {iters} Newton iterations')
    have = committed('value_grad', name)
    assert have['Z'] <= CEILING['Z'] and have['grad'] <= CEILING['grad']
    check4('value_grad', name, dict(Z=float(worst_z), grad=float(worst_g)))
    for k in range(32, 36):
        for s in range(ns + 1):
            if not np.isnan(Z[0, s]):
                assert got['status'][k, s, 0] in OK and np.isfinite(got['value'][k, s]) and np.isfinite(got['grad'][k, s]).all(), (k, s, got['status'][k, s])


def decision_distances(rec, got):
    """Worst distances of the kernel's pairs and variances to the f64 ones over the 32 theta: m as a share of the mass sum_i |term_i|, e in f32 steps of e,
    var as a share of c."""
    gs = {k: v.numpy() for k, v in rec['gs'].items()}
    c = np.exp(rec['thetas'].numpy()[:, 0])
    worst = dict(m=0., e=0., var=0.)
    for have, want, mass in ((got['cv_f'], gs['cv_f'], gs['cv_mass']), (got['test_f'], gs['test_f'], gs['test_mass'])):
        fin = np.isfinite(want[..., 0])
        assert np.array_equal(np.isfinite(have[..., 0]), fin) and np.array_equal(np.isfinite(have[..., 1]), fin)
        if fin.any():
            worst['m'] = max(worst['m'], float((np.abs(have[..., 0] - want[..., 0])[fin] / mass[fin]).max()))
            worst['e'] = max(worst['e'], float((np.abs(have[..., 1] - want[..., 1])[fin] / (EPS * np.maximum(want[..., 1][fin], 1e-30))).max()))
    fin = np.isfinite(gs['test_var'])
    assert fin.all() and (got['test_var'] >= 0).all()
    worst['var'] = float((np.abs(got['test_var'] - np.maximum(gs['test_var'], 0)) / c[:, None]).max())
    return worst


@pytest.mark.parametrize('name', NAMES)
def test_decision_values_and_variance_against_f64(name, recorded, device):
    """(b) The pairs (m, e) of every held-out row and every test row, and the refits' variances, at the same 32 theta.  m is compared as a share of the mass
    sum_i |c exp(e - U_i) (y_i - pi_i)|; e in f32 steps: it is a sum of F squares and a product with 1 / 2 l^2, so within 8 + F / 2 steps whatever is measured;
    the variance as a share of c.  A slot's status is the same from both kernels."""
    rec, got = recorded[name], device[name]
    assert np.array_equal(got['pstatus'], got['status'][:32])
    assert np.array_equal(got['pstatus'][:, :, 0], rec['gs']['status'].numpy()[:, :, 0])      # f32 and f64 agree on which fits run
    worst = decision_distances(rec, got)
    assert worst['e'] <= 8 + rec['F'] / 2
    check4('decision', name, worst)


def test_a_row_in_no_fold_is_never_written(recorded):
    """(b) cv_f of a row that no slot holds out keeps the caller's bits; the row trains every fit."""
    rec = recorded['n10_F3_T20']
    x, y, tx, folds = inputs(rec)
    folds = folds.clone()
    folds[0, 3] = 9
    n, T, ns = rec['n'], rec['T'], rec['n_splits']
    theta = per_slot(gf.grid_theta()[:4])
    cv_f = torch.full((1, 4, n, 2), 123.25, device=DEV)
    test_f, test_var, status = torch.empty(1, 4, T, 2, device=DEV), torch.empty(1, 4, T, device=DEV), torch.empty(1, 4, 6, 2, dtype=torch.int32, device=DEV)
    _hip.check(_hip.lib().pfn_gpc_predict(theta.data_ptr(), x.data_ptr(), y.data_ptr(), tx.data_ptr(), folds.data_ptr(), 1, n, T, rec['F'], 4, ns, cv_f.data_ptr(),
                                          test_f.data_ptr(), test_var.data_ptr(), status.data_ptr(), _hip.stream_ptr(torch.device(DEV))), 'pfn_gpc_predict')
    cv_f = cv_f.cpu().numpy()
    assert (cv_f[0, :, 3] == 123.25).all()
    others = np.delete(np.arange(n), 3)
    assert np.isfinite(cv_f[0][:, others]).all() and not (cv_f[0][:, others, 1] == 123.25).any()


def scores_with_windows(rec, got, bound_m):
    """Per candidate of the fixed grid: (the kernel's counts equal the f64 ones on every row outside the flip window, rows left out, rows)."""
    gs = {k: v.numpy() for k, v in rec['gs'].items()}
    folds, cls, ns = rec['folds'].numpy(), rec['y'].numpy() > 0.5, rec['n_splits']
    left = total = 0
    touched = np.zeros(24, dtype=bool)
    for c in range(24):
        for s in range(ns):
            if gs['status'][c, s, 0] not in OK:
                continue
            held = np.flatnonzero(folds == s)
            m, e, mass = gs['cv_f'][c, held, 0], gs['cv_f'][c, held, 1], gs['cv_mass'][c, held]
            out = (np.abs(m) <= bound_m * mass) | ((e >= 700) & (e <= 760))
            want = gf.f_star(m, e) > 0
            have = gf.f_star(got['cv_f'][c, held, 0], got['cv_f'][c, held, 1]) > 0
            assert np.array_equal(have[~out], want[~out]), (c, s)
            left, total, touched[c] = left + int(out.sum()), total + len(held), touched[c] or bool(out.any())
    return left, total, touched


@pytest.mark.parametrize('name', NAMES)
def test_fixed_grid_search_against_the_recorded_scikit_learn_run(name, recorded, device):
    """(c) optimize=False: the class of every held-out row is the f64 one wherever its f64 |m| exceeds the bound asserted in (b) of its mass and e lies outside
    [700, 760] (where exp(-e) leaves f64's range); at most 1 % of a problem's (row, fit) pairs are left out.  The scores of every candidate without such a
    row, the best candidate and its probabilities are the recorded ones -- which tools/record_gpc_fixtures.py asserted equal to GridSearchCV(
    GaussianProcessClassifier(optimizer=None)).  A probability may differ by what the bounds of (b) allow: the mixture is a sigmoid of slope <= 1/4 in f*, and
    moves by at most 0.05 |f*| per unit of variance."""
    rec, got = recorded[name], device[name]
    b = {k: 4 * v for k, v in committed('decision', name).items()}
    left, total, touched = scores_with_windows(rec, got, b['m'])
    print(f'{name}: {left} of {total} held-out pairs left out')
    assert left <= 0.01 * total
    mean, best, proba = tabular._gp_select(got['cv_f'][:24], got['pstatus'][:24], rec['folds'].numpy(), rec['y'].numpy(), rec['n_splits'], got['test_f'][:24],
                                           got['test_var'][:24])
    want = rec['mean_test_score'].numpy()
    assert mean[~touched].tobytes() == want[~touched].tobytes()
    assert best == rec['best']
    gs = {k: v.numpy() for k, v in rec['gs'].items()}
    fs = gf.f_star(gs['test_f'][best, :, 0], gs['test_f'][best, :, 1])
    df = b['m'] * gs['test_mass'][best] * np.exp(-gs['test_f'][best, :, 1]) + np.abs(fs) * b['e'] * EPS * gs['test_f'][best, :, 1]
    allowed = 0.25 * df + 0.05 * np.abs(fs) * b['var'] * np.exp(rec['thetas'].numpy()[best, 0]) + 1e-12
    assert (np.abs(proba - rec['proba'].numpy()) <= allowed).all(), (np.abs(proba - rec['proba'].numpy()).max(), allowed.max())
    # and through the public path
    x, y, tx, ty = (rec[k].to(DEV)[:, None] for k in ('x', 'y', 'test_x', 'test_y'))
    metric, proba2, params = tabular._gp_batched(x, y, tx, ty, optimize=False, return_params=True)
    assert proba2[:, 0].tobytes() == proba.tobytes() and params[0]['index'] == best and params[0]['start'] == gf.grid()[best]
    assert np.allclose(params[0]['kernel'], gf.grid()[best], rtol=1e-6)


@pytest.mark.parametrize('name', NAMES)
def test_optimising_pipeline_carries_its_certificate(name, recorded):
    """(d) A certificate, not path equality: for every fit that batched_lbfgs reports converged, the f64 restatement at the device's final theta gives a Z not
    below the Z at the start (less twice the f32 error of Z asserted in (a): both ends were judged in f32), and a projected gradient, taken on max(1, |Z|),
    within 4 x its committed measurement.  Reported, not asserted: the share of fits whose Z is within 1e-3 of the recorded f64 pipeline's and of
    scikit-learn's own, and whether the best kernel is theirs."""
    rec = recorded[name]
    x, y, tx, ty = (rec[k].to(DEV)[:, None] for k in ('x', 'y', 'test_x', 'test_y'))
    counters = {}
    _, _, params = tabular._gp_batched(x, y, tx, ty, return_params=True, counters=counters)
    ns, folds = rec['n_splits'], rec['folds'].numpy()
    theta, conv = counters['theta'][0], counters['converged'][0]
    assert (theta >= gf.BOX[0]).all() and (theta <= gf.BOX[1]).all()      # the returned theta is inside the box
    xs, ys = rec['x'].numpy(), rec['y'].numpy()
    Z0, slack = rec['Z'].numpy()[:24], 2 * 4 * committed('value_grad', name)['Z']
    Zp, Zs = rec['pipeline']['Z'].numpy(), rec['sklearn']['Z'].numpy()
    worst = 0.
    n_conv = n_fits = near_pipe = near_sk = 0
    for c in range(24):
        for s in range(ns + 1):
            if np.isnan(Z0[c, s]):
                continue
            n_fits += 1
            if not conv[c, s]:
                continue
            n_conv += 1
            rows = gf.slot_rows(folds, ns, s)
            Z, dZ, (reason, _) = gf.lml_grad(xs[rows], ys[rows], theta[c, s])
            assert reason in OK and Z >= Z0[c, s] - slack * abs(Z0[c, s]), (c, s, Z, Z0[c, s])
            worst = max(worst, float(np.abs(gf.project(theta[c, s], -dZ)).max() / max(1., abs(Z))))
            near_pipe += abs(Z - Zp[c, s]) <= 1e-3 * max(1., abs(Zp[c, s]))
            near_sk += abs(Z - Zs[c, s]) <= 1e-3 * max(1., abs(Zs[c, s]))
    assert n_conv >= n_fits // 2      # (a certificate of a handful of fits would certify little)
    report = dict(fits=n_fits, converged=n_conv, passes=counters['passes'], share_within_1e3_of_f64_pipeline=near_pipe / n_conv,
                  share_within_1e3_of_sklearn=near_sk / n_conv, best=params[0]['index'], best_f64_pipeline=rec['pipeline']['best'], best_sklearn=rec['sklearn']['best'])
    print(f'{name}: {report}')
    note('pipeline_report', name, {k: (float(v) if isinstance(v, float) else int(v)) for k, v in report.items()})
    check4('pipeline', name, dict(projected_gradient=worst))


def test_results_do_not_depend_on_batch_or_grid_position():
    """(e) A problem alone against the same problem in a batch, a candidate alone against the same candidate in the grid, two calls at the same theta: bitwise,
    for both kernels."""
    n, F, T, ns = 10, 3, 20, 5
    probs = [gf.problem(n, F, T, seed) for seed in (10, 110, 210)]
    folds = np.stack([tabular._stratified_folds(p[1] > 0.5, ns) for p in probs]).astype(np.int32)
    x, y, tx = (dev(np.stack([p[k] for p in probs])) for k in range(3))
    fd = dev(folds)
    thetas = np.concatenate([gf.grid_theta(), gf.extra_thetas(3)])
    th = per_slot(thetas).expand(3, -1, -1, -1).contiguous()

    def both(theta, sl):
        a = hipops.gpc_lml_grad(theta, x[sl], y[sl], fd[sl], ns)
        b = hipops.gpc_predict(theta, x[sl], y[sl], tx[sl], fd[sl], ns)
        return [t.cpu().numpy() for t in a + b]
    full = both(th, slice(0, 3))
    again = both(th, slice(0, 3))
    for u, v in zip(full, again):
        assert u.tobytes() == v.tobytes()
    alone = both(th[1:2].contiguous(), slice(1, 2))
    for u, v in zip(full, alone):
        assert u[1].tobytes() == v[0].tobytes()
    one = both(th[:, 5:6].contiguous(), slice(0, 3))
    for u, v in zip(full, one):
        assert u[:, 5].tobytes() == v[:, 0].tobytes()


def test_edge_cases_stay_finite_and_follow_scikit_learn():
    """(f) A one-class training fold scores NaN and has its status; a one-class window raises; duplicated rows with opposite labels and all rows identical
    (K = c 1 1^T) stay finite."""
    rng = np.random.RandomState(0)
    x = rng.randn(6, 2).astype(np.float32)
    y = np.array([1, 0, 0, 0, 0, 0], dtype=np.float32)      # the fold that holds the one positive out trains on one class
    folds = tabular._stratified_folds(y > 0.5, 3).astype(np.int32)
    s1 = int(folds[0])
    theta = per_slot(gf.grid_theta()[:3])
    value, grad, status = (t[0].cpu().numpy() for t in hipops.gpc_lml_grad(theta, dev(x[None]), dev(y[None]), dev(folds[None]), 3))
    assert (status[:, s1, 0] == gf.ONE_CLASS).all() and np.isnan(value[:, s1]).all() and not grad[:, s1].any()
    others = [s for s in range(4) if s != s1]
    assert np.isin(status[:, others, 0], OK).all() and np.isfinite(value[:, others]).all()
    cv_f, test_f, test_var, pstatus = (t[0].cpu().numpy() for t in hipops.gpc_predict(theta, dev(x[None]), dev(y[None]), dev(x[None, :2]), dev(folds[None]), 3))
    assert np.isnan(cv_f[:, folds == s1]).all() and np.isfinite(cv_f[:, folds != s1]).all() and np.isfinite(test_f).all()
    mean, best, _ = tabular._gp_select(cv_f, pstatus, folds, y, 3, test_f, test_var)
    assert np.isnan(mean).all() and best == 0      # as GridSearchCV: every mean NaN, the first candidate is refitted
    with pytest.raises(ValueError, match='one class'):
        tabular.gp_metric(dev(x), torch.ones(6, device=DEV), dev(x[:2]), torch.zeros(2, device=DEV), [])
    # duplicated rows with opposite labels; then all rows identical
    for xs in (np.concatenate([x[:3], x[:3]]), np.repeat(x[:1], 6, 0)):
        ys = np.array([1, 0, 1, 0, 1, 0], dtype=np.float32)
        fo = tabular._stratified_folds(ys > 0.5, 3).astype(np.int32)
        th = per_slot(gf.grid_theta())
        value, grad, status = (t[0].cpu().numpy() for t in hipops.gpc_lml_grad(th, dev(xs[None]), dev(ys[None]), dev(fo[None]), 3))
        assert np.isin(status[:, :4, 0], OK).all() and np.isfinite(value[:, :4]).all() and np.isfinite(grad[:, :4]).all()
        cv_f, test_f, test_var, _ = (t[0].cpu().numpy() for t in hipops.gpc_predict(th, dev(xs[None]), dev(ys[None]), dev(x[None]), dev(fo[None]), 3))
        assert np.isfinite(cv_f).all() and np.isfinite(test_f).all() and np.isfinite(test_var).all() and (test_var >= 0).all()
        for k, theta_k in enumerate(gf.grid_theta()):
            Z, _, _ = gf.lml_grad(xs, ys, theta_k)
            assert abs(-value[k, 3] - Z) <= 1e-4 * abs(Z)


def test_short_lengthscale_keeps_the_sign_where_f32_underflows(recorded, device):
    """(f) The pitfall of l = 0.1: on the recorded n = 33, F = 8 problem d^2 / 2 l^2 = 50 d^2 lies between 87 and 700 for most held-out rows, so exp underflows
    in f32 -- a decision value formed there is exactly 0, class 0 -- and not in f64, which sees a tiny f* with a sign.  The pairs (m, e) keep it: the held-out
    classes of all six l = 0.1 candidates equal the f64 ones, on rows that a product in f32 gets wrong."""
    name = 'n33_F8_T7'
    rec, got = recorded[name], device[name]
    gs = {k: v.numpy() for k, v in rec['gs'].items()}
    cands = [c for c, (_, l) in enumerate(gf.grid()) if l == 0.1]
    assert len(cands) == 6
    lost = rows = 0
    for c in cands:
        m, e = got['cv_f'][c, :, 0], got['cv_f'][c, :, 1]
        assert np.isfinite(m).all() and (e > 87).any()
        want = gf.f_star(gs['cv_f'][c, :, 0], gs['cv_f'][c, :, 1])
        sure = (np.abs(gs['cv_f'][c, :, 0]) > 4 * committed('decision', name)['m'] * gs['cv_mass'][c]) & (gs['cv_f'][c, :, 1] < 700)
        assert np.array_equal((gf.f_star(m, e) > 0)[sure], (want > 0)[sure])
        naive = m.astype(np.float32) * np.exp(-e.astype(np.float32), dtype=np.float32)
        lost += int(((naive == 0) & (want > 0) & sure).sum())
        rows += int(sure.sum())
    print(f'{lost} of {rows} held-out rows have a positive f64 f* that an f32 product turns into class 0')
    assert rows >= 150 and lost >= rows // 4


def test_evaluate_with_gp_metric_end_to_end():
    """(g) evaluate with gp_metric on the diabetes rows: the reference's result keys, finite AUCs, probabilities; the chosen kernels with return_params."""
    d = torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_diabetes.pt'))
    positions = [10, 20]
    res = tabular.evaluate([['diabetes', d['X'], d['y'], []]], tabular.gp_metric, 'gp', 30, positions, DEV, max_samples=3)
    keys = {'metric', 'mean_metric', 'diabetes_time'} | {f'mean_metric_at_{p}' for p in positions}
    keys |= {f'diabetes_{k}_at_{p}' for p in positions for k in ('mean_metric', 'per_ds_metric', 'outputs', 'ys')}
    assert set(res) == keys and res['metric'] == 'auc'
    for p in positions:
        per_window, outputs = res[f'diabetes_per_ds_metric_at_{p}'], res[f'diabetes_outputs_at_{p}']
        assert per_window.shape == (3,) and outputs.shape == (30 - p, 3) and np.isfinite(outputs).all() and (outputs >= 0).all() and (outputs <= 1).all()
        assert np.isfinite(res[f'diabetes_mean_metric_at_{p}']) and 0 <= res[f'mean_metric_at_{p}'] <= 1
    X, y = d['X'].to(DEV), d['y'].to(DEV)
    starts = tabular.select_windows(X.shape[0], 30, 3)
    xw, _ = hipops.tabular_windows(X.float().contiguous(), y.float().contiguous(), starts, 30, 20, mode=hipops.TAB_NORM_TRAIN_ONLY)
    rows = (starts[:, None] + torch.arange(30)[None, :]).t().to(DEV)
    yw = y.float()[rows]
    metric, proba, params = tabular._gp_batched(xw[:20], yw[:20], xw[20:], yw[20:], return_params=True)
    assert np.array_equal(proba, res['diabetes_outputs_at_20']) and len(params) == 3
    for p in params:
        c, l = p['kernel']
        assert 1e-5 <= c * (1 - 1e-6) and c <= 1e5 * (1 + 1e-6) and 1e-5 <= l * (1 - 1e-6) and l <= 1e5 * (1 + 1e-6) and p['start'] == gf.grid()[p['index']]
