"""Host-side checks of the gradient-boosting baseline (csrc/xgb_cv.hip, hipops.xgb_cv, tabular.xgb_metric): the C ABI and the build, the entry point's argument
checks, the grid against scikit-learn's ParameterGrid, the folds against StratifiedKFold(5), the draw addressing against a fixed table of Philox words, the
restatement tests/xgb_f64.py against a brute-force enumeration in pure Python, the tie and legality rules on hand-built problems, the host half of the grid
search against GridSearchCV's ranking, the recorded fixture and its gap condition, the planted faults, and the kernel's compiled budgets.  No GPU."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tabular_cases      # noqa: E402
import xgb_cases as cases      # noqa: E402
import xgb_f64 as xf      # noqa: E402

from transformerscandobayesianinference_amd import _hip, hipops, tabular      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc')
PFN_ERR_UNSUPPORTED, PFN_ERR_ARGUMENT = -1, -4
FIX = 2 ** 23


def recorded():
    return torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_xgb.pt'), weights_only=False)


def test_the_symbol_is_declared_exported_and_bound_at_abi_10():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    source = open(os.path.join(CSRC, 'xgb_cv.hip')).read()
    lib = _hip.lib()
    assert re.search(r'\bpfn_xgb_cv\s*\(', header)
    assert 'pfn_xgb_cv' in _hip.SIGNATURES and hasattr(lib, 'pfn_xgb_cv') and len(_hip.SIGNATURES['pfn_xgb_cv'][1]) == 27
    assert re.search(r'^extern "C" int pfn_xgb_cv\s*\(', source, re.M) and re.search(r'\blaunch_xgb_cv\s*\(', source) and 'struct XgbCvArgs' in source
    assert _hip.ABI_VERSION == 10 and lib.pfn_abi_version() == 10 and '#define PFN_ABI_VERSION 10' in header
    for name, value in (('FOLDS', 5), ('SLOTS', 6), ('MAX_CANDIDATES', 64), ('MAX_DEPTH', 2), ('MAX_ROUNDS', 4096), ('UNUSED', 0), ('DONE', 1), ('NONFINITE', 2)):
        assert f'#define PFN_XGB_CV_{name} {value}\n' in header and getattr(hipops, 'XGB_CV_' + name) == value, name
    assert (hipops.XGB_CV_UNUSED, hipops.XGB_CV_DONE, hipops.XGB_CV_NONFINITE) == (hipops.BNN_CV_UNUSED, hipops.BNN_CV_DONE, hipops.BNN_CV_NONFINITE)
    assert (xf.SLOTS, xf.FOLDS, xf.MAX_DEPTH, xf.MAX_ROUNDS, xf.UNUSED, xf.DONE, xf.NONFINITE) == (6, 5, 2, 4096, 0, 1, 2)
    assert callable(hipops.xgb_cv) and callable(hipops.xgb_cv_check) and hipops.XGB_CV_LIMITS['n'] == (4, 128)
    assert callable(tabular.xgb_metric) and tabular.xgb_metric.batched is tabular._xgb_batched
    build = open(os.path.join(CSRC, 'build.sh')).read()
    assert 'xgb_cv.hip' in build and '../_build/xgb_cv.o' in build      # compiled and linked
    for shared in ('bnn_sigmoid', 'philox4x32_10', 'launch_lds', 'fold_shapes'):
        assert re.search(r'\b%s\s*\(' % shared, source), shared      # the shared pieces, not copies of them
    assert 'atomic' not in source.replace('No atomics', '').replace('no atomics', '')
    assert 'stay out: they need libraries' in tabular.__doc__ and 'xgb_metric' in tabular.__doc__ and 'CatBoost' in tabular.__doc__
    from transformerscandobayesianinference_amd import compat
    assert 'tabular' in compat._NAMES      # the reference's `from tabular import xgb_metric` resolves through the module alias, as for the other metric functions


def test_argument_errors_return_before_any_launch():
    lib = _hip.lib()
    buf = torch.zeros(4096)      # host memory standing in for device buffers: a refused call never looks at it
    p = buf.data_ptr()
    i32, f32, f64 = (lambda *v: np.array(v, dtype=np.int32)), (lambda *v: np.array(v, dtype=np.float32)), (lambda *v: np.array(v, dtype=np.float64))

    def call(P=1, n=8, T=2, F=3, NC=2, n_splits=4, depth=i32(1, 2), lr=f32(0.2, 0.02), mcw=f64(0.5, 1.), sub=f64(0.5, 1.), col=f64(0.8, 1.), ids=None, rounds=3, train=p,
             order=p, status=p, cv=p, te=p, trees=(0, 0, 0), depth_null=False):
        return lib.pfn_xgb_cv(train, p, p, p, 0 if depth_null else depth.ctypes.data, lr.ctypes.data, mcw.ctypes.data, sub.ctypes.data, col.ctypes.data,
                              0 if ids is None else ids.ctypes.data, P, n, T, F, NC, n_splits, rounds, 7, 0, order, cv, te, status, *trees, 0)
    nan, inf = float('nan'), float('inf')
    for kw in (dict(n=3), dict(n=129), dict(T=0), dict(T=129), dict(F=0), dict(F=129), dict(NC=0), dict(NC=65), dict(depth=i32(1, 0)), dict(depth=i32(3, 1)), dict(rounds=-1),
               dict(rounds=4097), dict(sub=f64(0., 1.)), dict(sub=f64(0.5, 1.5)), dict(col=f64(0.8, 0.)), dict(col=f64(1.01, 1.)), dict(mcw=f64(-0.5, 1.)), dict(lr=f32(0., 0.1)),
               dict(lr=f32(0.2, -1.))):
        assert call(**kw) == PFN_ERR_UNSUPPORTED, kw
    assert call(n=3) == PFN_ERR_UNSUPPORTED and b'4 .. 128' in lib.pfn_last_error_string()
    for kw in (dict(P=0), dict(n_splits=1), dict(n_splits=6), dict(train=0), dict(order=0), dict(status=0), dict(cv=0), dict(te=0), dict(depth_null=True),
               dict(lr=f32(nan, 0.1)), dict(lr=f32(inf, 0.1)), dict(mcw=f64(nan, 1.)), dict(mcw=f64(inf, 1.)), dict(sub=f64(nan, 1.)), dict(col=f64(0.8, nan)),
               dict(ids=i32(0, 64)), dict(ids=i32(-1, 0)), dict(trees=(p, 0, 0)), dict(trees=(p, p, 0))):
        assert call(**kw) == PFN_ERR_ARGUMENT, kw
    # the limits first, before the arguments and before any pointer is looked at
    assert call(n=3, train=0, P=0) == PFN_ERR_UNSUPPORTED and call(depth=i32(1, 3), P=0, status=0) == PFN_ERR_UNSUPPORTED


def test_python_checks_raise_before_the_device_is_asked_for():
    fold = torch.zeros(1, 8, dtype=torch.int32)
    x, y, tx = torch.zeros(1, 8, 3), torch.zeros(1, 8), torch.zeros(1, 2, 3)
    ok = ([1, 2], [0.2, 0.02], [0.5, 1.], [0.5, 0.8], [0.8, 0.8])
    with pytest.raises(ValueError, match='n = 3'):
        hipops.xgb_cv_check(3, 2, 3, [1])
    with pytest.raises(ValueError, match='max_depth = 3'):
        hipops.xgb_cv_check(8, 2, 3, [1, 3])
    with pytest.raises(ValueError, match='NC = 65'):
        hipops.xgb_cv_check(8, 2, 3, [1] * 65)
    with pytest.raises(ValueError, match='num_rounds = 4097'):
        hipops.xgb_cv_check(8, 2, 3, [1], 4097)
    with pytest.raises(ValueError, match='F = 129'):
        hipops.xgb_cv(torch.zeros(1, 8, 129), y, torch.zeros(1, 2, 129), fold, 4, *ok, 3)
    for bad in (([1, 2], [0.2, -1.], *ok[2:]), (*ok[:2], [0.5, float('nan')], *ok[3:]), (*ok[:3], [0.5, 0.], ok[4]), (*ok[:4], [0.8, 1.2]), (*ok[:4], [0.8])):
        with pytest.raises(ValueError):
            hipops.xgb_cv(x, y, tx, fold, 4, *bad, 3)
    with pytest.raises(ValueError):
        hipops.xgb_cv(x, y, tx, fold, 6, *ok, 3)
    with pytest.raises(ValueError, match='F = 129'):
        tabular.xgb_metric(torch.zeros(8, 129), torch.zeros(8), torch.zeros(2, 129), torch.zeros(2), [])
    # with sound arguments the product path asks for the GPU: there is no CPU fall-back
    with pytest.raises(_hip.HipExtensionError):
        hipops.xgb_cv(x, y, tx, fold, 4, *ok, 3)
    with pytest.raises(NotImplementedError):
        tabular.xgb_metric(torch.randn(12, 3), torch.tensor([0., 1.] * 6), torch.randn(2, 3), torch.zeros(2), [])


def test_grid_enumeration_is_parametergrids():
    reference = {'min_child_weight': [0.5, 1.0], 'learning_rate': [0.02, 0.2], 'subsample': [0.5, 0.8], 'max_depth': [1, 2], 'colsample_bytree': [0.8],
                 'eval_metric': ['logloss'], 'n_estimators': [100]}
    assert tabular.param_grid['xgb'] == reference == xf.PARAM_GRID
    entries, rounds = tabular._xgb_grid()
    assert rounds == 100 and len(entries) == 16 and entries == xf.grid_entries()
    # subsample fastest, then min_child_weight, max_depth, learning_rate
    assert [(e['learning_rate'], e['max_depth'], e['min_child_weight'], e['subsample']) for e in entries[:5]] == \
        [(0.02, 1, 0.5, 0.5), (0.02, 1, 0.5, 0.8), (0.02, 1, 1.0, 0.5), (0.02, 1, 1.0, 0.8), (0.02, 2, 0.5, 0.5)] and entries[8]['learning_rate'] == 0.2
    assert all(e['colsample_bytree'] == 0.8 and e['n_estimators'] == 100 and e['eval_metric'] == 'logloss' for e in entries)
    with pytest.raises(ValueError):
        tabular._xgb_grid(dict(reference, n_estimators=[100, 200]))
    model_selection = pytest.importorskip('sklearn.model_selection')
    assert entries == list(model_selection.ParameterGrid(reference))


def test_folds_are_stratified_kfold_5_whatever_n_is():
    model_selection = pytest.importorskip('sklearn.model_selection')
    rec = recorded()
    labels = [g['y'].numpy() for g in rec['grid']] + [tabular_cases.problem(n, F, T, seed)[1] for n, F, T, seed, _ in cases.STRUCTURAL]
    for y in labels:
        want = np.empty(len(y), dtype=np.int32)
        for k, (_, test) in enumerate(model_selection.StratifiedKFold(5).split(np.zeros((len(y), 1)), y > 0.5)):
            want[test] = k
        assert np.array_equal(tabular._stratified_folds(y > 0.5, 5), want)
    # the reference passes cv=5, not min(CV, n // 2): _fold_problems takes it, and without the argument does what it did
    x, y = torch.randn(12, 2, 3), torch.tensor([[0., 1.]] * 6 + [[1., 0.]] * 6)
    n5, f5, cls5, ops5 = tabular._fold_problems(x, y, torch.randn(2, 2, 3), n_splits=5)
    assert n5 == 5 and np.array_equal(f5[0], tabular._stratified_folds(cls5[:, 0], 5)) and ops5[3].dtype == torch.int32
    x8, y8 = x[:8], y[:8]
    n4, f4, _, ops4 = tabular._fold_problems(x8, y8, torch.randn(2, 2, 3))
    assert n4 == 4 and np.array_equal(f4[1], tabular._stratified_folds(y8[:, 1].numpy() > 0.5, 4)) and torch.equal(ops4[0], x8.transpose(0, 1).contiguous())
    with pytest.raises(ValueError):      # as scikit-learn: more splits than members in every class
        tabular._fold_problems(x8, torch.tensor([[0., 1.]] * 4 + [[1., 0.]] * 4), torch.randn(2, 2, 3), n_splits=5)


def test_draw_replay_against_a_fixed_table_of_philox_words():
    q = xf.stream(3, 2, 1)
    assert q == (3 * 64 + 2) * 8 + 1 == 1553
    assert [int(v) for v in xf.row_words(11, q, 5, 6)] == [0xf486bcd4, 0xade977cf, 0x1bad5b41, 0x5f8ef879, 0xcc6c4e6d, 0x3c88c6cd]
    assert [int(v) for v in xf.feature_words(11, q, 5, 6)] == [0x1da2626b, 0xa0f391a5, 0x77401b61, 0x0f6723ca, 0xd7ecc36e, 0x650fa6cb]
    import nuts_f64 as emu
    assert int(xf.row_words(11, q, 5, 6)[5]) == emu.philox4x32_10((5 << 6) | 1, q, 11)[1] and int(xf.feature_words(11, q, 5, 6)[2]) == emu.philox4x32_10((1 << 32) | (5 << 6), q, 11)[2]
    assert xf.sampled_rows(11, q, 5, 12, 0.5).astype(int).tolist() == [0, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 0]
    assert xf.sampled_features(11, q, 5, 10, 0.8).tolist() == [0, 1, 2, 3, 5, 6, 7, 9] and xf.sampled_features(11, q, 5, 10, 0.05).tolist() == [3]      # k = max(1, floor)
    assert (xf.subsample_threshold(0.5), xf.subsample_threshold(0.8), xf.subsample_threshold(1.0)) == (1 << 31, 3435973836, 1 << 32) and xf.sampled_rows(1, 2, 3, 9, 1.0).all()
    assert (xf.mcw_fixed(0.5), xf.mcw_fixed(1.0), xf.mcw_fixed(1e9)) == (1 << 22, 1 << 23, 1 << 30)
    # rounds and rows use disjoint counters: the last round's last block stays below the feature domain, which the row counters never reach
    assert ((4095 << 6) | 31) < 1 << 32 and not xf.sampled_rows(0, xf.stream(0, 0, 5), 2, 10, 0.1).any()      # (the zero-tree case of the GPU test)


def brute_force_node(x, rows, feats, gi, hi, mcwi):
    """Every candidate of a node enumerated in pure Python: for each feature and each pair of consecutive distinct values a cut between them, the sums by looping
    over the rows on either side.  Returns (feature, threshold) of the split, or None."""
    best = None
    for f in sorted(int(v) for v in feats):
        values = sorted({float(x[i, f]) for i in rows})
        for a, b in zip(values[:-1], values[1:]):
            left = [i for i in rows if float(x[i, f]) <= a]
            right = [i for i in rows if float(x[i, f]) >= b]
            GL, HL, GR, HR = sum(int(gi[i]) for i in left), sum(int(hi[i]) for i in left), sum(int(gi[i]) for i in right), sum(int(hi[i]) for i in right)
            if HL < mcwi or HR < mcwi:
                continue
            sc = lambda G, H: (G / FIX) ** 2 / (H / FIX + 1.)
            gain = (sc(GL, HL) + sc(GR, HR)) - sc(GL + GR, HL + HR)
            if best is None or gain > best[0]:      # (ascending feature, ascending value: the first of equal gains stays)
                best = (gain, f, xf.threshold(a, b))
    return None if best is None or not best[0] > 1e-6 else best[1:]


@pytest.mark.parametrize('n,F,seed', [(8, 2, 0), (12, 3, 1), (12, 5, 2), (10, 4, 3), (12, 1, 4)])
def test_the_restatement_against_brute_force(n, F, seed):
    rng = np.random.RandomState(seed)
    x = np.round(rng.randn(n, F) * 2).astype(np.float32) / 2      # repeated values in every column
    y = (rng.rand(n) < 0.5).astype(np.float32)
    mask = np.arange(n) % 4 != 1
    depth, eta, mcw, sub, col, rounds, q = 2, 0.3, 0.3, 0.8, 0.8, 4, xf.stream(seed, 1, 2)
    r = xf.fit(x, y, mask, x[:3], depth, eta, mcw, sub, col, rounds, 5, q)
    margin = np.zeros(n + 3)
    allx = np.concatenate([x, x[:3]])
    for t in range(rounds):
        gi, hi = xf.grad_stats(margin[:n], y > 0.5, np.float64)
        rows = [i for i in range(n) if mask[i] and xf.sampled_rows(5, q, t, n, sub)[i]]
        feats = xf.sampled_features(5, q, t, F, col)
        leaf = [0] * (n + 3)
        root = brute_force_node(x, rows, feats, gi, hi, xf.mcw_fixed(mcw))
        assert (r['feature'][t, 0], r['threshold'][t, 0]) == ((-1, 0) if root is None else root)
        if root is not None:
            leaf = [2 if not allx[i, root[0]] < root[1] else 0 for i in range(n + 3)]
            for node in (1, 2):
                child = brute_force_node(x, [i for i in rows if leaf[i] >> 1 == node - 1], feats, gi, hi, xf.mcw_fixed(mcw))
                assert (r['feature'][t, node], r['threshold'][t, node]) == ((-1, 0) if child is None else child), (t, node)
                if child is not None:
                    leaf = [L | 1 if L >> 1 == node - 1 and not allx[i, child[0]] < child[1] else L for i, L in enumerate(leaf)]
        for L in range(4):
            members = [i for i in rows if leaf[i] == L]
            G, H = sum(int(gi[i]) for i in members) / FIX, sum(int(hi[i]) for i in members) / FIX
            want = float(np.float32(eta)) * -(G / (H + 1.)) if members else 0.
            assert abs(r['leaf'][t, L] - want) <= 1e-15
        margin = margin + np.array([r['leaf'][t, L] for L in leaf])
    assert np.abs(np.concatenate([r['margin'], r['test_margin']]) - margin).max() <= 1e-14


def one_round(x, y, depth=1, mcw=0., **kw):
    return xf.fit(np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32), np.ones(len(x), dtype=bool), None, depth, 0.5, mcw, 1.0, 1.0, 1, 0, 0, **kw)


def test_tie_and_legality_rules_on_hand_built_problems():
    y = [0, 0, 0, 1, 1, 1]
    sep = [0., 1., 2., 3., 4., 5.]
    # a duplicated column: the lower index wins; a mirrored column cuts the same partition and ties bit for bit, in f32 as in f64
    for dtype in (np.float64, np.float32):
        r = one_round(np.stack([np.zeros(6), sep, sep], 1), y, dtype=dtype)
        assert r['feature'][0].tolist() == [1, -1, -1] and r['threshold'][0, 0] == 2.5
        r = one_round(np.stack([[-v for v in sep], sep], 1), y, dtype=dtype)
        assert r['feature'][0].tolist() == [0, -1, -1] and r['threshold'][0, 0] == -2.5
    # equal gains at two positions of one feature: the lower position.  Labels 0 1 | 0 1: the cuts after rows 0 and after row 2 mirror each other
    r = one_round(np.array([[0.], [1.], [2.], [3.]]), [1, 0, 0, 1])
    c = xf.candidates(np.array([[0.], [1.], [2.], [3.]], dtype=np.float32), np.arange(4), [0], *xf.grad_stats(np.zeros(4), np.array([1, 0, 0, 1]) > 0.5, np.float64), 0, np.float64)
    assert c['gain'][0] == c['gain'][2] > c['gain'][1] and r['threshold'][0, 0] == 0.5
    # a constant column is never split, and no cut falls between equal values: three distinct values give two candidates
    x3 = np.stack([np.ones(6), [0., 0., 1., 1., 2., 2.]], 1)
    c = xf.candidates(x3.astype(np.float32), np.arange(6), [0, 1], *xf.grad_stats(np.zeros(6), np.array(y) > 0.5, np.float64), 0, np.float64)
    assert c['f'].tolist() == [1, 1] and c['pos'].tolist() == [1, 3] and c['a'].tolist() == [0., 1.] and c['b'].tolist() == [1., 2.]
    assert one_round(np.ones((6, 2)), y)['feature'][0].tolist() == [-1, -1, -1]
    # legality: at round 0 every h is 1/4, so a side of k rows has H = k / 4, compared as integers: mcw 0.5 admits sides of 2 rows, 0.5 + 2^-23 does not
    assert one_round(np.array(sep)[:, None], [0, 0, 1, 1, 1, 1], mcw=0.5)['threshold'][0, 0] == 1.5
    r = one_round(np.array(sep)[:, None], [0, 0, 1, 1, 1, 1], mcw=0.5 + 2. ** -23)
    assert r['threshold'][0, 0] == 2.5      # the best legal cut now leaves three rows on either side
    assert one_round(np.array(sep)[:, None], y, mcw=0.75 + 2. ** -23)['feature'][0, 0] == -1 and one_round(np.array(sep)[:, None], y, mcw=1e9)['leaf'][0].tolist() == [0., 0., 0., 0.]
    # the threshold is the f32 midpoint, and the upper value where that rounds to the lower one
    a = np.float32(1.)
    b = np.nextafter(a, np.float32(2.))
    assert xf.threshold(a, b) == b and xf.threshold(np.float32(1.), np.float32(2.)) == np.float32(1.5) and xf.threshold(a, b).dtype == np.float32
    # a gain that is not above 1e-6 makes a leaf: one class only has G^2 / (H + 1) split into parts that add up to less
    assert one_round(np.array(sep)[:, None], [1] * 6)['feature'][0, 0] == -1
    # the leaf value: G = 3 (-1/2) + 0, H = 3/4: -eta G / (H + 1) on the side of the ones
    r = one_round(np.array(sep)[:, None], y)
    assert r['leaf'][0, 0] == pytest.approx(0.5 * -(1.5 / 1.75)) and r['leaf'][0, 2] == pytest.approx(0.5 * (1.5 / 1.75)) and r['margin'].tolist() == [r['leaf'][0, 0]] * 3 + [r['leaf'][0, 2]] * 3


def test_selection_against_gridsearchcvs_ranking_on_the_recorded_scores():
    rec = recorded()
    for g in rec['grid']:
        cv, folds, cls = g['cv_margin'].numpy(), g['folds'].numpy(), g['y'].numpy() > 0.5
        mean, best, proba = tabular._xgb_select(cv, folds, cls, 5, g['test_margin'].numpy())
        assert mean.dtype == np.float64 and mean.tobytes() == g['mean_test_score'].numpy().tobytes() and best == g['best']
        assert np.array_equal(proba, 1. / (1. + np.exp(-g['test_margin'].numpy()[best])))
        mean2, best2 = xf.select(cv, folds, cls, 5)
        assert mean2.tobytes() == mean.tobytes() and best2 == best
        # GridSearchCV: rank_test_score 1 goes to the first of the best means (scipy's rankdata, method 'min', on the negated means)
        stats = pytest.importorskip('scipy.stats')
        rank = stats.rankdata(-mean, method='min')
        assert int(np.flatnonzero(rank == 1)[0]) == best
    # hand-made: margin exactly 0 predicts class 0; a fit that left the finite numbers ranks last
    folds, cls = np.array([0, 0, 1, 1, 0, 1], dtype=np.int32), np.array([1, 0, 1, 0, 1, 0], dtype=bool)
    cv = np.array([[2., -2., 0., -1., -0.5, 1.], [1., -1., 1., -1., 1., 1.], [0.1, -0.1, 3., -3., 2., 2.]])
    mean, best, proba = tabular._xgb_select(cv, folds, cls, 2, np.array([[0., 1.], [-1., 2.], [5., 5.]]))
    assert mean.tolist() == [0.5, (1. + 2 / 3) / 2, (1. + 2 / 3) / 2] and best == 1 and proba.tolist() == [1 / (1 + np.e), 1 / (1 + np.exp(-2.))]
    cv[1, 0] = np.nan
    assert tabular._xgb_select(cv, folds, cls, 2, np.zeros((3, 2)))[1] == 2


def test_the_recorded_fixture_is_what_the_restatement_still_computes_and_meets_the_gap_condition():
    rec = recorded()
    assert rec['entries'] == tabular._xgb_grid()[0] and rec['fit_seed'] == cases.FIT_SEED and len(rec['grid']) == len(cases.GRID_WINDOWS)
    assert len(rec['structural']) >= rec['structural_fits'] // 2 and rec['certificate_e'] >= 0
    assert {f['problem'] for f in rec['structural']} == set(range(len(cases.STRUCTURAL))) and {f['cand'] for f in rec['structural']} == set(range(len(cases.STRUCTURAL_CANDS)))
    for f in rec['structural']:
        assert f['gap'] >= cases.MIN_GAP == 1e-4 and f['mcw_distance'] >= cases.MIN_MCW_DISTANCE == 2. ** -16
    for f in rec['structural'][::7]:      # a sample, recomputed
        n, F, T, seed, rounds = cases.STRUCTURAL[f['problem']]
        x, y, tx, ty = tabular_cases.problem(n, F, T, seed)
        folds = tabular._stratified_folds(y > 0.5, 5)
        depth, eta, mcw, sub, col = cases.STRUCTURAL_CANDS[f['cand']]
        r = xf.fit(x, y, xf.row_mask(folds, f['slot'], 5), tx if f['slot'] == 5 else None, depth, eta, mcw, sub, col, rounds, cases.FIT_SEED, xf.stream(f['problem'], f['cand'], f['slot']))
        assert np.array_equal(r['feature'], f['feature'].numpy()) and r['threshold'].tobytes() == f['threshold'].numpy().tobytes() and r['gap'] == f['gap']
        assert np.array_equal(r['test_margin'] if f['slot'] == 5 else r['margin'][folds == f['slot']], f['out'].numpy())
    d = torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_diabetes.pt'))
    for w, (g, window) in enumerate(zip(rec['grid'], cases.GRID_WINDOWS)):
        x, y, tx, ty = cases.diabetes_window(d['X'].numpy(), d['y'].numpy(), *window)
        assert tuple(g['window']) == window and np.array_equal(x, g['x'].numpy()) and np.array_equal(tx, g['test_x'].numpy()) and np.array_equal(y, g['y'].numpy())
        assert np.array_equal(tabular._stratified_folds(y > 0.5, 5), g['folds'].numpy())
        assert g['cv_margin'].shape == (16, window[1]) and g['test_margin'].shape == (16, window[2]) and bool(torch.isfinite(g['cv_margin']).all())
        assert 0 < g['e_margin'] < 1e-4 and 0 < g['e_proba'] < 1e-4 and g['near_zero'] == 0      # no held-out margin within the bound of the class boundary
        c, s = 9, 5      # one fit of the grid, recomputed: learning rate 0.2, depth 1, the refit
        en = rec['entries'][c]
        r = xf.fit(x, y, np.ones(len(x), dtype=bool), tx, en['max_depth'], en['learning_rate'], en['min_child_weight'], en['subsample'], en['colsample_bytree'], 100, g['seed'],
                   xf.stream(w, c, s))
        assert g['problem_id'] == w and np.array_equal(r['test_margin'], g['test_margin'].numpy()[c])


def test_each_planted_fault_moves_a_fixture_margin_past_the_bound():
    table = json.load(open(os.path.join(ROOT, 'profiles', 'xgb_cv_fault_sensitivity.json')))['faults']
    assert set(table) == set(cases.FAULTS) and all(v['ratio'] > 100 for v in table.values())
    # and here, recomputed on problem 0 with the rows in class order and column 4 repeated as column 5: the refit of candidate 1
    n, F, T, seed, rounds = cases.STRUCTURAL[0]
    x, y, tx, ty = tabular_cases.problem(n, F, T, seed)
    by_class = np.argsort(y, kind='stable')      # rows in class order: a cut between the equal values of the zero column (column 1) would separate the classes
    x, y = x[by_class], y[by_class]
    x = np.concatenate([x, x[:, 4:5]], 1)      # a duplicated column for the tie rule
    tx = np.concatenate([tx, tx[:, 4:5]], 1)
    depth, eta, mcw, sub, col = cases.STRUCTURAL_CANDS[1]
    args = (x, y, np.ones(n, dtype=bool), tx, depth, eta, mcw, sub, col, rounds, cases.FIT_SEED, xf.stream(0, 1, 5))
    r64 = xf.fit(*args)
    r32 = xf.follow((r64['feature'], r64['threshold']), *args, dtype=np.float32)
    scale = np.abs(r64['test_margin']).max()
    bound = 4 * max(np.abs(r32['test_margin'] - r64['test_margin']).max() / scale, 2. ** -23) * scale
    for fault in cases.FAULTS:
        rf = xf.fit(*args, faults=(fault,))
        shift = np.abs(rf['test_margin'] - r64['test_margin']).max()
        if fault == 'tie_to_higher':      # the same partition through the other column: the margins stay, the structure shows it
            both = np.array([4 in xf.sampled_features(cases.FIT_SEED, args[-1], t, F + 1, col) and F in xf.sampled_features(cases.FIT_SEED, args[-1], t, F + 1, col) for t in range(rounds)])
            assert both.any() and (rf['feature'][both] == F).any() and not (r64['feature'][both] == F).any() and not (rf['feature'][both] == 4).any()
        else:
            assert shift > 10 * bound, (fault, shift, bound)


def test_the_kernel_keeps_its_register_scratch_and_lds_budgets(tmp_path):
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    asm = str(tmp_path / 'xgb_cv.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-munsafe-fp-atomics', '-Wno-unused-result', '-S', '--cuda-device-only',
                    os.path.join(CSRC, 'xgb_cv.hip'), '-o', asm], check=True, capture_output=True)
    found = dict(re.findall(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', open(asm).read(), re.S))
    assert len(found) == 2      # the sort pre-pass and one kernel for every depth and shape
    for name, vgprs, lds in (('xgb_order_kernel', 32, 512), ('xgb_cv_kernel', 128, 512)):
        body = [b for k, b in found.items() if name in k][0]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0      # no scratch
        assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= vgprs      # four waves per SIMD
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1)) <= lds
    static_lds = 512

    def lds_bytes(n, F):      # xgb_cv_lds_bytes
        return 4 * (32 + n * (F | 1) + 3 * n + 2 * F) + ((F * n + 3) & ~3)
    assert lds_bytes(128, 128) == 85120 and lds_bytes(128, 128) + static_lds <= 160 * 1024
    assert lds_bytes(80, 60) == 25888 and 6 * (lds_bytes(80, 60) + static_lds) <= 160 * 1024      # the study's shape: six fits share a CU
    text = open(os.path.join(CSRC, 'xgb_cv.hip')).read()
    assert '(32 + (size_t)n * (F | 1) + 3 * (size_t)n + 2 * (size_t)F) * 4 + (((size_t)F * n + 3) & ~(size_t)3)' in text and 'static_assert' in text
