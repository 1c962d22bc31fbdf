"""Host-side checks of the CatBoost baseline (csrc/catboost_cv.hip, hipops.catboost_cv, tabular.catboost_metric): the C ABI and the build, the entry point's
argument errors (they come before any HIP call, so no GPU is needed), the grid map 81 -> 27, the seeded stratified hold-out, the selection rules, and the
restatement tests/catboost_f64.py itself -- the prefix property, follow against fit, a hand-computed stump, the draws -- with the planted faults that show the
bounds of tests/test_gpu_catboost.py are not vacuous (profiles/catboost_cv_fault_sensitivity.json)."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tabular_cases      # noqa: E402
import catboost_cases as cases      # noqa: E402
import catboost_f64 as cf      # noqa: E402

from transformerscandobayesianinference_amd import _hip, hipops, tabular      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc')
PFN_ERR_UNSUPPORTED, PFN_ERR_ARGUMENT = -1, -4
FLOOR = 2. ** -23


def recorded():
    return torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_catboost.pt'), weights_only=False)


def recorder():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import record_catboost_cv_fixtures
    return record_catboost_cv_fixtures


def test_the_symbol_is_declared_exported_and_bound_at_abi_10():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    source = open(os.path.join(CSRC, 'catboost_cv.hip')).read()
    lib = _hip.lib()
    assert re.search(r'\bpfn_catboost_cv\s*\(', header) and 'Oblivious boosted trees with their grid search' in header
    assert 'pfn_catboost_cv' in _hip.SIGNATURES and hasattr(lib, 'pfn_catboost_cv') and len(_hip.SIGNATURES['pfn_catboost_cv'][1]) == 26
    assert re.search(r'^extern "C" int pfn_catboost_cv\s*\(', source, re.M) and re.search(r'\blaunch_catboost_cv\s*\(', source) and 'struct CatCvArgs' in source
    assert _hip.ABI_VERSION == 10 and lib.pfn_abi_version() == 10 and '#define PFN_ABI_VERSION 10' in header
    for name, value in (('SLOTS', 2), ('MAX_CANDIDATES', 64), ('MAX_DEPTH', 7), ('MAX_LEAVES', 128), ('MAX_ROUNDS', 1024), ('MAX_CHECKPOINTS', 8), ('DONE', 1),
                        ('NONFINITE', 2), ('ONE_CLASS', 3)):
        assert f'#define PFN_CATBOOST_CV_{name} {value}\n' in header and getattr(hipops, 'CATBOOST_CV_' + name) == value, name
    assert (cf.SLOTS, cf.MAX_DEPTH, cf.MAX_LEAVES, cf.MAX_ROUNDS, cf.MAX_CHECKPOINTS, cf.DONE, cf.NONFINITE, cf.ONE_CLASS) == (2, 7, 128, 1024, 8, 1, 2, 3)
    assert (hipops.CATBOOST_CV_DONE, hipops.CATBOOST_CV_NONFINITE) == (hipops.XGB_CV_DONE, hipops.XGB_CV_NONFINITE)
    assert callable(hipops.catboost_cv) and callable(hipops.catboost_cv_check) and hipops.CATBOOST_CV_LIMITS['n'] == (4, 128)
    assert callable(tabular.catboost_metric) and tabular.catboost_metric.batched is tabular._catboost_batched
    build = open(os.path.join(CSRC, 'build.sh')).read()
    assert 'catboost_cv.hip' in build and '../_build/catboost_cv.o' in build      # compiled and linked
    for shared in ('philox4x32_10', 'launch_lds', 'fold_shapes'):
        assert re.search(r'\b%s\s*\(' % shared, source), shared      # the shared pieces, not copies of them
    assert 'atomic' not in source.replace('No atomics', '').replace('no atomics', '')
    assert 'static_assert' in source and '160 * 1024' in source      # the LDS limit, beside catboost_cv_lds_bytes
    assert 'catboost_metric' in tabular.__doc__ and 'stay out' in tabular.__doc__
    from transformerscandobayesianinference_amd import compat
    assert 'tabular' in compat._NAMES      # the reference's `from tabular import catboost_metric` resolves through the module alias


def test_argument_errors_return_before_any_launch():
    lib = _hip.lib()
    buf = torch.zeros(4096)      # host memory standing in for device buffers: a refused call never looks at it
    p = buf.data_ptr()
    i32, f32 = (lambda *v: np.array(v, dtype=np.int32)), (lambda *v: np.array(v, dtype=np.float32))

    def call(P=1, n=8, T=2, F=3, NC=2, NK=2, depth=i32(1, 7), lr=f32(0.5, 0.1), l2=f32(0., 1.), ids=None, ck=i32(1, 3), rounds=3, train=p, order=p, status=p, hold=p,
             te=p, trees=(0, 0, 0), depth_null=False, ck_null=False):
        return lib.pfn_catboost_cv(train, p, p, p, 0 if depth_null else depth.ctypes.data, lr.ctypes.data, l2.ctypes.data, 0 if ids is None else ids.ctypes.data,
                                   0 if ck_null else ck.ctypes.data, P, n, T, F, NC, NK, rounds, 7, 0, order, hold, te, status, *trees, 0)
    nan, inf = float('nan'), float('inf')
    for kw in (dict(n=3), dict(n=129), dict(T=0), dict(T=129), dict(F=0), dict(F=129), dict(NC=0), dict(NC=65), dict(depth=i32(1, 0)), dict(depth=i32(8, 1)), dict(rounds=0),
               dict(rounds=1025)):
        assert call(**kw) == PFN_ERR_UNSUPPORTED, kw
    assert call(n=3) == PFN_ERR_UNSUPPORTED and b'4 .. 128' in lib.pfn_last_error_string()
    for kw in (dict(P=0), dict(train=0), dict(order=0), dict(status=0), dict(hold=0), dict(te=0), dict(depth_null=True), dict(ck_null=True), dict(lr=f32(nan, 0.1)),
               dict(lr=f32(inf, 0.1)), dict(lr=f32(0., 0.1)), dict(lr=f32(0.5, -1.)), dict(l2=f32(-0.5, 1.)), dict(l2=f32(nan, 1.)), dict(l2=f32(0., inf)),
               dict(ids=i32(0, 64)), dict(ids=i32(-1, 0)), dict(trees=(p, 0, 0)), dict(trees=(p, p, 0)), dict(NK=0), dict(NK=9), dict(ck=i32(3, 3)), dict(ck=i32(2, 1)),
               dict(ck=i32(0, 3)), dict(ck=i32(1, 2)), dict(ck=i32(1, 4))):
        assert call(**kw) == PFN_ERR_ARGUMENT, kw
    # the limits first, before the arguments and before any pointer is looked at
    assert call(n=3, train=0, P=0) == PFN_ERR_UNSUPPORTED and call(depth=i32(1, 8), P=0, status=0) == PFN_ERR_UNSUPPORTED
    assert call(rounds=1025, ck=i32(1, 2), l2=f32(-1., 0.)) == PFN_ERR_UNSUPPORTED


def test_python_checks_raise_before_the_device_is_asked_for():
    fold = torch.ones(1, 8, dtype=torch.int32)
    x, y, tx = torch.zeros(1, 8, 3), torch.zeros(1, 8), torch.zeros(1, 2, 3)
    ok = ([2, 7], [0.5, 0.1], [0., 1.])
    with pytest.raises(ValueError, match='n = 3'):
        hipops.catboost_cv_check(3, 2, 3, [1])
    with pytest.raises(ValueError, match='depth = 8'):
        hipops.catboost_cv_check(8, 2, 3, [1, 8])
    with pytest.raises(ValueError, match='NC = 65'):
        hipops.catboost_cv_check(8, 2, 3, [1] * 65)
    with pytest.raises(ValueError, match='num_rounds = 1025'):
        hipops.catboost_cv_check(8, 2, 3, [1], 1025)
    with pytest.raises(ValueError, match='F = 129'):
        hipops.catboost_cv(torch.zeros(1, 8, 129), y, torch.zeros(1, 2, 129), fold, *ok, 3)
    for bad in (([2, 7], [0.5, -1.], ok[2]), (*ok[:2], [0., float('nan')]), (*ok[:2], [0., -1.]), (*ok[:2], [0.])):
        with pytest.raises(ValueError):
            hipops.catboost_cv(x, y, tx, fold, *bad, 3)
    for checkpoints in ((), (1, 2), (3, 3), (0, 3), tuple(range(1, 10))):
        with pytest.raises(ValueError, match='checkpoints'):
            hipops.catboost_cv(x, y, tx, fold, *ok, 3 if len(checkpoints) < 9 else 9, checkpoints=checkpoints)
    with pytest.raises(ValueError, match='F = 129'):
        tabular.catboost_metric(torch.zeros(8, 129), torch.zeros(8), torch.zeros(2, 129), torch.zeros(2), [])
    # with sound arguments the product path asks for the GPU: there is no CPU fall-back
    with pytest.raises(_hip.HipExtensionError):
        hipops.catboost_cv(x, y, tx, fold, *ok, 3)
    with pytest.raises(NotImplementedError):
        tabular.catboost_metric(torch.randn(12, 3), torch.tensor([0., 1.] * 6), torch.randn(2, 3), torch.zeros(2), [0])


def test_the_grid_is_81_entries_on_27_fits_read_at_three_checkpoints():
    reference = {'learning_rate': [0.1, 0.5, 1.0], 'depth': [2, 4, 7], 'l2_leaf_reg': [0.0, 0.5, 1], 'iterations': [10, 40, 70]}
    assert tabular.param_grid['catboost'] == reference == cf.PARAM_GRID and list(tabular.param_grid['catboost']) == list(reference)
    entries, fits, where, checkpoints = tabular._catboost_grid()
    assert (entries, fits, where, checkpoints) == cf.grid_entries()
    assert len(entries) == 81 and len(fits) == 27 and len(set(fits)) == 27 and checkpoints == [10, 40, 70]
    # the dict's key order, the last key varying fastest: iterations, then l2_leaf_reg, depth, learning_rate
    assert [(e['learning_rate'], e['depth'], e['l2_leaf_reg'], e['iterations']) for e in entries[:4]] == [(0.1, 2, 0.0, 10), (0.1, 2, 0.0, 40), (0.1, 2, 0.0, 70), (0.1, 2, 0.5, 10)]
    assert entries[9]['depth'] == 4 and entries[27]['learning_rate'] == 0.5 and entries[80] == {'learning_rate': 1.0, 'depth': 7, 'l2_leaf_reg': 1, 'iterations': 70}
    assert where[:4] == [(0, 0), (0, 1), (0, 2), (1, 0)] and where[80] == (26, 2) and fits[0] == (0.1, 2, 0.0) and fits[26] == (1.0, 7, 1.0)
    for e, (c, k) in zip(entries, where):
        assert fits[c] == (e['learning_rate'], e['depth'], e['l2_leaf_reg']) and checkpoints[k] == e['iterations']
    assert 'prefix' in tabular._catboost_grid.__doc__      # the sharing is stated where it is made


def test_the_hold_out_is_stratified_and_seeded():
    rng = np.random.RandomState(0)
    for n, share in ((40, 0.5), (80, 0.3), (13, 0.2), (10, 0.9)):
        cls = rng.rand(n) < share
        cls[:2] = (False, True)
        fold = tabular._catboost_holdout(cls, 3, 1)
        assert fold.dtype == np.int32 and set(fold.tolist()) <= {0, 1}
        for k in (False, True):
            count = int((cls == k).sum())
            want = int(np.floor(0.2 * count + 0.5))
            assert int(((fold == 0) & (cls == k)).sum()) == (max(want, 1) if count >= 2 else want), (n, k)
        assert np.array_equal(fold, tabular._catboost_holdout(cls, 3, 1))      # seeded
        assert not np.array_equal(fold, tabular._catboost_holdout(cls, 4, 1)) or not np.array_equal(fold, tabular._catboost_holdout(cls, 5, 1))
        assert not np.array_equal(fold, tabular._catboost_holdout(cls, 3, 2)) or not np.array_equal(fold, tabular._catboost_holdout(cls, 3, 3))
        assert np.array_equal(fold, tabular._catboost_holdout(cls.astype(np.float32), 3, 1))      # labels or classes
    # a class of one row is never held out; both classes stay to learn on
    fold = tabular._catboost_holdout(np.array([0, 0, 0, 0, 1]), 0, 0)
    assert fold[4] == 1 and (fold[:4] == 0).sum() == 1
    # the words are Philox's: the device's generator, on the host
    import nuts_f64 as emu
    assert tabular._philox4x32_10(5, 1553, 11) == emu.philox4x32_10(5, 1553, 11)
    assert [int(v) for v in cf.philox_words(np.array([5, (3 << 17) | 9]), 1553, 11)[0]] == [emu.philox4x32_10(5, 1553, 11)[0], emu.philox4x32_10((3 << 17) | 9, 1553, 11)[0]]


def test_the_selection_takes_the_first_minimum_and_ranks_nan_last():
    where = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]
    fold, cls = np.array([0, 1, 0, 1, 1]), np.array([True, False, False, True, False])
    hold = np.full((3, 2, 5), np.nan)
    hold[0, 0, [0, 2]] = (0.0, 0.0)          # log 2
    hold[0, 1, [0, 2]] = (2.0, -2.0)         # the minimum ...
    hold[1, 0, [0, 2]] = (2.0, -2.0)         # ... again: the first wins
    hold[1, 1, [0, 2]] = (np.nan, 5.0)       # NaN ranks last
    hold[2, 0, [0, 2]] = (1.0, -1.0)
    hold[2, 1, [0, 2]] = (-3.0, 3.0)
    test = np.arange(3 * 2 * 4, dtype=np.float64).reshape(3, 2, 4) / 10
    loss, best, proba = tabular._catboost_select(hold, fold, cls, where, test)
    assert best == 1 and np.isnan(loss[3]) and loss[1] == loss[2] == np.log1p(np.exp(-2.)) and abs(loss[0] - np.log(2.)) < 1e-15 and loss[5] > 3
    assert np.array_equal(proba, 1. / (1. + np.exp(-test[0, 1]))) and proba.dtype == np.float64
    assert np.array_equal(loss, cf.select(hold, fold, cls, where)[0], equal_nan=True) and cf.select(hold, fold, cls, where)[1] == 1
    hold[0, 1] = np.nan
    assert tabular._catboost_select(hold, fold, cls, where, test)[1] == 2
    assert tabular._catboost_select(np.full((3, 2, 5), np.nan), fold, cls, where, test)[1] == 0      # all NaN: entry 0


def small_problem():
    x, y, tx, ty = tabular_cases.problem(24, 5, 6, 1)
    return x, y, tx, cases.holdout_fold(y)


def test_a_fit_contains_the_shorter_fits_as_prefixes():
    x, y, tx, fold = small_problem()
    for slot, cand in ((0, (4, 0.5, 0.5)), (1, (7, 0.1, 0.0))):
        args = (x, y, cf.learn_mask(fold, slot), tx, *cand)
        long = cf.fit(*args, 8, 3, cf.stream(0, 1, slot))
        for count in (1, 3, 8):
            short = cf.fit(*args, count, 3, cf.stream(0, 1, slot))
            for k in ('feature', 'threshold', 'leaf', 'margin', 'test_margin'):
                assert np.array_equal(short[k], long[k][:count]), (slot, count, k)


def test_following_a_fits_own_trees_reproduces_it():
    x, y, tx, fold = small_problem()
    for dtype in (np.float64, np.float32):
        args = (x, y, cf.learn_mask(fold, 0), tx, 4, 0.5, 0.5, 5, 3, cf.stream(2, 0, 0))
        r = cf.fit(*args, dtype=dtype)
        f = cf.follow((r['feature'], r['threshold']), *args, dtype=dtype)
        assert all(np.array_equal(f[k], r[k]) for k in ('feature', 'threshold', 'leaf', 'margin', 'test_margin')) and f['gap'] == r['gap']
        assert len(f['levels']) == int((r['feature'] >= 0).sum()) and all(lv['legal'] and lv['value'] == lv['best'] for lv in f['levels'])
        assert cf.certificate(f['levels']) == 0
    # another legal border is followed and priced; a threshold that is no border, a used border and an early end are not legal
    trees = (r['feature'].copy(), r['threshold'].copy())
    trees[1][0, 0] += np.float32(1e-3)
    assert not cf.follow(trees, *args)['levels'][0]['legal'] and cf.certificate(cf.follow(trees, *args)['levels']) == np.inf
    trees = (r['feature'].copy(), r['threshold'].copy())
    trees[0][0, 1], trees[1][0, 1] = trees[0][0, 0], trees[1][0, 0]
    assert not cf.follow(trees, *args)['levels'][1]['legal']
    trees = (r['feature'].copy(), r['threshold'].copy())
    trees[0][0, 1:], trees[1][0, 1:] = -1, 0
    assert not cf.follow(trees, *args)['levels'][1]['legal']


def test_a_hand_computed_stump():
    x = np.array([[0.], [0.], [1.], [1.], [1.]], dtype=np.float32)
    y = np.array([0., 0., 1., 1., 0.], dtype=np.float32)
    tx = np.array([[-3.], [0.5], [0.75]], dtype=np.float32)
    lr, l2 = 0.5, 0.5
    r = cf.fit(x, y, np.ones(5, dtype=bool), tx, 1, lr, l2, 1, 0, 0, newton_iterations=1)
    assert r['feature'][0].tolist() == [0] + [-1] * 6 and r['threshold'][0, 0] == np.float32(0.5)      # the one border, between 0 and 1
    # one Newton iteration from v = 0: v = sum(y - 1/2) / (c / 4 + l2)
    v_lo, v_hi = (-0.5 - 0.5) / (2 / 4 + l2), (0.5 + 0.5 - 0.5) / (3 / 4 + l2)
    assert r['leaf'][0, 0] == lr * v_lo and r['leaf'][0, 1] == lr * v_hi and (r['leaf'][0, 2:] == 0).all()
    assert np.array_equal(r['margin'][0], lr * np.array([v_lo, v_lo, v_hi, v_hi, v_hi])) and np.array_equal(r['test_margin'][0], lr * np.array([v_lo, v_lo, v_hi]))
    # a second tree starts from those margins: g = y - sigmoid(margin), in 2^-23 fixed point
    r2 = cf.fit(x, y, np.ones(5, dtype=bool), tx, 1, lr, l2, 2, 0, 0, newton_iterations=1)
    assert np.array_equal(r2['leaf'][0], r['leaf'][0])
    z = r['margin'][0]
    q = 1 / (1 + np.exp(-z))
    steps = [float(np.rint((y[i] - q[i]) * 2. ** 40).sum()) / float(np.rint(q[i] * (1 - q[i]) * 2. ** 40).sum() + l2 * 2. ** 40) for i in ([0, 1], [2, 3, 4])]
    assert np.allclose(r2['leaf'][1, :2], lr * np.array(steps), rtol=1e-12, atol=0)
    # the threshold rule: the midpoint, and a where the midpoint rounds to b
    assert cf.threshold(0., 1.) == np.float32(0.5) and cf.threshold(1., np.nextafter(np.float32(1), np.float32(2))) == np.float32(1)
    # one class to learn on, a NaN: refused
    assert cf.fit(x, np.zeros(5), np.ones(5, dtype=bool), tx, 1, lr, l2, 1, 0, 0)['status'] == cf.ONE_CLASS
    assert cf.fit(np.where(x == 0, np.nan, x), y, np.ones(5, dtype=bool), tx, 1, lr, l2, 1, 0, 0)['status'] == cf.NONFINITE


def test_the_noise_is_a_standard_normal_from_exact_uniforms():
    f, j = np.repeat(np.arange(64), 64), np.tile(np.arange(64), 64)
    z = cf.normals(3, 2, f, j, cf.stream(1, 2, 1), 7, np.float64)
    assert abs(z.mean()) < 0.05 and abs(z.std() - 1) < 0.05 and np.isfinite(z).all() and len(np.unique(z)) == len(z)
    z32 = cf.normals(3, 2, f, j, cf.stream(1, 2, 1), 7, np.float32)
    assert z32.dtype == np.float32 and np.abs(z32 - z).max() < 8 * FLOOR * np.abs(z).max()
    assert not np.array_equal(z, cf.normals(3, 2, f, j, cf.stream(1, 2, 0), 7, np.float64)) and not np.array_equal(z, cf.normals(4, 2, f, j, cf.stream(1, 2, 1), 7, np.float64))
    # the counter's fields do not overlap: t < 1024, d < 8, f < 128, j < 128
    assert (1023 << 17 | 7 << 14 | 127 << 7 | 127) < 1 << 32 and (1 << 14) > (127 << 7 | 127) and (1 << 17) > (7 << 14 | 127 << 7 | 127)


def test_the_recorded_fixture_is_the_restatements():
    rec = recorded()
    assert rec['entries'] == tabular._catboost_grid()[0] and rec['fit_seed'] == cases.FIT_SEED
    assert 2 * len(rec['structural']) >= rec['structural_fits'] == len(cases.STRUCTURAL) * len(cases.STRUCTURAL_CANDS) * 2
    assert all(f['gap'] >= cases.MIN_GAP for f in rec['structural']) and np.isfinite(rec['certificate_e'])
    tool = recorder()
    for f in rec['structural'][::7]:
        k, c, s = f['problem'], f['cand'], f['slot']
        x, y, tx, ty, fold, rounds = tool.structural_problem(k)
        r = cf.fit(*tool.fit_args(x, y, tx, fold, cases.STRUCTURAL_CANDS[c], s, rounds, c, problem_id=k))
        assert np.array_equal(r['feature'], f['feature'].numpy()) and np.array_equal(r['threshold'], f['threshold'].numpy())
        assert np.array_equal(tool.outputs(r, fold, s), f['out'].numpy()) and r['gap'] == f['gap']
    d = torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_diabetes.pt'))
    for w, g in enumerate(rec['grid']):
        x, y, tx, ty = cases.diabetes_window(d['X'].numpy(), d['y'].numpy(), *cases.GRID_WINDOWS[w])
        assert np.array_equal(g['x'].numpy(), x) and np.array_equal(g['fold'].numpy(), tabular._catboost_holdout(y > 0.5, g['seed'], w))
        loss, best = cf.select(g['hold_margin'].numpy(), g['fold'].numpy(), y > 0.5, tabular._catboost_grid()[2])
        assert np.array_equal(loss, g['loss'].numpy()) and best == g['best'] and g['runner_up'] > g['loss_bound'] > 0
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'tabular_catboost.pt')) < 1 << 20


def test_planted_faults_move_what_the_gpu_test_bounds():
    """Each fault of catboost_cases.FAULTS, planted into the restatement, moves a margin or the certificate by at least 8 x the bound the GPU test asserts -- or
    is recorded and named as one that stays under (profiles/catboost_cv_fault_sensitivity.json: `under`)."""
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'catboost_cv_fault_sensitivity.json')))
    assert set(rec['faults']) == set(cases.FAULTS) and rec['required'] == 8
    ratios = recorder().fault_ratios(recorded()['certificate_e'])
    for f in cases.FAULTS:
        assert np.isclose(min(ratios[f]['ratio'], 1e300), rec['faults'][f]['ratio'], rtol=1e-6), f
        print(f'fault {f}: {ratios[f]["ratio"]:.3g} x the bound')
        if f in rec.get('under', []):
            assert ratios[f]['ratio'] < 8, f      # recorded and named, not asserted
        else:
            assert ratios[f]['ratio'] >= 8, f
