"""Host-side checks of the GP-classifier baseline (csrc/gpc.hip, tabular.gp_metric, hipops.gpc_*): the C ABI and the build, the kernels' descriptor budgets,
the f64 restatement against scikit-learn from the recorded problems, the grid against itertools.product, the host half of the grid search bit for bit from the
recorded pairs, and the argument checks that must answer without a GPU.  No GPU."""
import itertools
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpc_f64 as gf      # noqa: E402

from transformerscandobayesianinference_amd import _hip, hipops, tabular      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc')
PFN_ERR_UNSUPPORTED, PFN_ERR_ARGUMENT = -1, -4
OK = (gf.CONVERGED, gf.CAPPED)


@pytest.fixture(scope='module')
def recorded():
    d = torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_gpc.pt'), weights_only=False)
    for rec in d['problems']:
        gf.attach_rows(rec, torch.from_numpy)
    return d


def test_the_symbols_are_declared_exported_and_bound_at_abi_10():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    source = open(os.path.join(CSRC, 'gpc.hip')).read()      # the entry points stand beside their kernels
    lib = _hip.lib()
    for symbol, nargs in (('pfn_gpc_lml_grad', 13), ('pfn_gpc_predict', 16)):
        assert re.search(r'\b%s\s*\(' % symbol, header)
        assert symbol in _hip.SIGNATURES and hasattr(lib, symbol) and len(_hip.SIGNATURES[symbol][1]) == nargs
        assert re.search(r'^int %s\s*\(' % symbol, source, re.M), symbol      # defined there ...
    assert re.search(r'\blaunch_gpc_lml_grad\s*\(', source) and re.search(r'\blaunch_gpc_predict\s*\(', source)      # ... and wired to its launcher
    assert _hip.ABI_VERSION == 10 and lib.pfn_abi_version() == 10 and '#define PFN_ABI_VERSION 10' in header
    for name, value in (('FOLDS', 5), ('SLOTS', 6), ('MAX_CANDIDATES', 64), ('MAX_N', 112), ('MAX_NEWTON', 100), ('UNUSED', 0), ('CONVERGED', 1), ('CAPPED', 2),
                        ('ONE_CLASS', 3), ('NONPOSITIVE', 4), ('NONFINITE', 5)):
        assert f'#define PFN_GPC_{name} {value}\n' in header and getattr(hipops, 'GPC_' + name) == value, name
    assert (gf.UNUSED, gf.CONVERGED, gf.CAPPED, gf.ONE_CLASS, gf.NONPOSITIVE, gf.NONFINITE) == (0, 1, 2, 3, 4, 5) and gf.MAX_NEWTON == hipops.GPC_MAX_NEWTON
    assert hipops.GPC_MAX_N >= 80      # the study's largest eval position at bptt 100
    assert all(callable(f) for f in (hipops.gpc_lml_grad, hipops.gpc_predict, hipops.gpc_check, tabular.gp_metric, tabular.gp_metric.batched, tabular._gp_select))
    build = open(os.path.join(CSRC, 'build.sh')).read()
    assert 'gpc.hip' in build and '../_build/gpc.o' in build      # compiled and linked


def lds_bytes(n):
    """The launcher's dynamic LDS (gpc.hip gpc_lds_bytes): K, the exponent arguments and the factor (inverted in place for the gradient) at the odd stride n | 1, sixteen vectors over
    the rows, eight words of reduction space."""
    return 4 * (3 * n * (n | 1) + 16 * n + 8)


def test_the_kernels_keep_their_register_scratch_and_lds_budgets(tmp_path):
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    asm = str(tmp_path / 'gpc.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', os.path.join(CSRC, 'gpc.hip'), '-o', asm], check=True,
                   capture_output=True)
    found = re.findall(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', open(asm).read(), re.S)
    assert len(found) == 2 and sorted('lml_grad' in f[0] for f in found) == [False, True] and all('gpc_' in f[0] for f in found)
    for _, body in found:
        static_lds = int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1))
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0      # no scratch
        assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 128      # four waves per SIMD
        assert static_lds <= 512      # (the compaction's counts; everything else is dynamic)
        # the cap: three 112 x 113 matrices, 1792 + 8 words of vectors
        assert lds_bytes(112) == 4 * (3 * 112 * 113 + 1792 + 8) == 159072 and lds_bytes(112) + static_lds <= 160 * 1024
        assert lds_bytes(114) > 160 * 1024      # (and not much room is given away)
        # the study's largest shape: one block per CU there, two from n = 56 down
        assert lds_bytes(80) == 4 * (3 * 80 * 81 + 1280 + 8) == 82912
    text = open(os.path.join(CSRC, 'gpc.hip')).read()
    assert '((size_t)3 * n * (n | 1) + 16 * (size_t)n + 8) * 4' in text


def test_grid_is_the_references_product_in_its_order():
    reference = {'params_y_scale': [0.05, 0.1, 0.5, 1.0, 5.0, 10.0], 'params_length_scale': [0.1, 0.5, 1.0, 2.0]}
    assert tabular.param_grid['gp'] == reference
    want = list(itertools.product(reference['params_y_scale'], reference['params_length_scale']))
    assert tabular._gp_grid() == want == gf.grid() and len(want) == 24
    assert want[0] == (0.05, 0.1) and want[1] == (0.05, 0.5) and want[4] == (0.1, 0.1) and want[-1] == (10.0, 2.0)      # l varies fastest
    assert tabular.GP_BOX == gf.BOX == (np.log(1e-5), np.log(1e5))


def test_the_fixture_covers_the_cases(recorded):
    assert [(r['n'], r['F'], r['T']) for r in recorded['problems']] == gf.SHAPES + [(30, 8, 10)]
    assert gf.SHAPES[-1][0] == hipops.GPC_MAX_N and recorded['grid'] == gf.grid()
    assert sorted({r['n_splits'] for r in recorded['problems']}) == [2, 5]
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'tabular_gpc.pt')) <= os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'tabular_logistic.pt'))
    for rec in recorded['problems']:
        n, F, T = rec['n'], rec['F'], rec['T']
        assert rec['x'].shape == (n, F) and rec['test_x'].shape == (T, F) and rec['x'].dtype == torch.float32
        assert np.array_equal(rec['folds'].numpy(), tabular._stratified_folds(rec['y'].numpy() > 0.5, rec['n_splits'])) and rec['n_splits'] == min(5, n // 2)
        thetas = rec['thetas'].numpy()
        assert np.array_equal(thetas[:24], gf.grid_theta()) and thetas.shape == (32, 2) and (thetas[:, 0] <= 5).all()
        out, total = rec['left_out']
        assert out <= 0.01 * total      # the cap of the GPU test (c), met in the f32 restatement
    # the smallest folds: two rows (one of each class)
    assert min(np.bincount(r['folds'].numpy()).min() for r in recorded['problems']) == 2
    # both kinds of end point on the diabetes window: a proper optimum, and the plateau Z = -n log 2 of the fits that stay at c -> 0
    rec = recorded['problems'][-1]
    Zs = rec['sklearn']['Z'].numpy()[:, rec['n_splits']]
    plateau = np.abs(Zs + 30 * np.log(2)) < 1e-3
    assert plateau.any() and (~plateau).any() and (Zs[~plateau] > -30 * np.log(2) + 0.1).all()


def test_the_restatement_equals_scikit_learn(recorded):
    """Re-asserted from the file on a subset small enough for the suite: Z and dZ/dtheta against log_marginal_likelihood(theta, eval_gradient=True) to 1e-9
    of |Z|, predict and predict_proba with optimizer=None to 1e-10, and the optimize=False grid search against GridSearchCV."""
    gpmod = pytest.importorskip('sklearn.gaussian_process')
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel
    from sklearn.model_selection import GridSearchCV

    def kernel(th):
        return ConstantKernel(float(np.exp(th[0]))) * RBF(float(np.exp(th[1])))
    for rec in recorded['problems']:
        if rec['n'] > 33:
            continue
        x, y, tx, folds, ns = rec['x'].numpy(), rec['y'].numpy(), rec['test_x'].numpy(), rec['folds'].numpy(), rec['n_splits']
        thetas, Z, dZ = rec['thetas'].numpy(), rec['Z'].numpy(), rec['dZ'].numpy()
        gs = {k: v.numpy() for k, v in rec['gs'].items()}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for s in range(ns + 1):
                rows = gf.slot_rows(folds, ns, s)
                if gf.one_class(y[rows]):
                    assert np.isnan(Z[:, s]).all() and (gs['status'][:, s, 0] == gf.ONE_CLASS).all()
                    continue
                gp = gpmod.GaussianProcessClassifier(kernel=kernel(thetas[0]), optimizer=None).fit(x[rows].astype(np.float64), y[rows])
                for k in range(0, 32, 3):
                    Zs, gsk = gp.log_marginal_likelihood(thetas[k], eval_gradient=True)
                    assert abs(Z[k, s] - Zs) <= 1e-9 * abs(Zs) and np.abs(dZ[k, s] - gsk).max() <= 1e-9 * abs(Zs)
                    Zr, gr, _ = gf.lml_grad(x[rows], y[rows], thetas[k])      # the restatement still computes what was recorded
                    assert abs(Zr - Z[k, s]) <= 1e-12 * abs(Z[k, s]) and np.abs(gr - dZ[k, s]).max() <= 1e-10 * abs(Z[k, s])
            for c in (0, 7, 18, 23):
                gp = gpmod.GaussianProcessClassifier(kernel=kernel(thetas[c]), optimizer=None).fit(x.astype(np.float64), y)
                fs = gf.f_star(gs['test_f'][c, :, 0], gs['test_f'][c, :, 1])
                assert np.array_equal(gp.predict(tx.astype(np.float64)) > 0.5, fs > 0)
                assert np.abs(gp.predict_proba(tx.astype(np.float64))[:, 1] - gf.proba(fs, gs['test_var'][c])).max() <= 1e-10
            search = GridSearchCV(gpmod.GaussianProcessClassifier(optimizer=None), {'kernel': [kernel(th) for th in thetas[:24]]}, cv=ns)
            search.fit(x.astype(np.float64), y.astype(np.int64))
        assert search.cv_results_['mean_test_score'].tobytes() == rec['mean_test_score'].numpy().tobytes() and search.best_index_ == rec['best']
        assert np.abs(search.predict_proba(tx.astype(np.float64))[:, 1] - rec['proba'].numpy()).max() <= 1e-10


def test_selection_reproduces_the_recorded_scores_from_the_recorded_pairs(recorded):
    for rec in recorded['problems']:
        gs = {k: v.numpy() for k, v in rec['gs'].items()}
        folds, y, ns = rec['folds'].numpy(), rec['y'].numpy(), rec['n_splits']
        mean, best, proba = tabular._gp_select(gs['cv_f'][:24], gs['status'][:24], folds, y, ns, gs['test_f'][:24], gs['test_var'][:24])
        want = rec['mean_test_score'].numpy()
        assert mean.dtype == np.float64 and mean.tobytes() == want.tobytes()      # bit for bit, NaN included
        assert best == rec['best'] and np.abs(proba - rec['proba'].numpy()).max() <= 1e-12
        assert best == int(np.flatnonzero(want == np.nanmax(want))[0])      # the FIRST maximum
        mean2, best2, _ = gf.select(gs['cv_f'][:24], gs['status'][:24], folds, y, ns)      # the same from the oracle's own selection
        assert mean2.tobytes() == want.tobytes() and best2 == best
        # the erf mixture of the product path against the oracle's, at var = 0 too
        fs, var = gf.f_star(gs['test_f'][best, :, 0], gs['test_f'][best, :, 1]), gs['test_var'][best]
        assert np.abs(tabular._gp_proba(fs, var) - gf.proba(fs, var)).max() <= 1e-12
        assert np.abs(tabular._gp_proba(fs, 0 * var) - gf.proba(fs, 0 * var)).max() <= 1e-12 and np.isfinite(tabular._gp_proba(fs, -var)).all()


def test_selection_ranks_nan_last_and_raises_when_every_fit_failed():
    folds = np.array([0, 0, 1, 1, 0, 1], dtype=np.int32)
    y = np.array([1., 0., 1., 0., 1., 0.])
    status = np.zeros((3, 6, 2), dtype=np.int32)
    status[:, :3, 0] = hipops.GPC_CONVERGED
    status[0, 1, 0] = hipops.GPC_ONE_CLASS      # candidate 0: a one-class training part in fold 1 -> its mean is NaN
    cv_f = np.zeros((3, 6, 2))
    cv_f[0, :, 0] = 2 * y - 1      # all right, but for the failed fold
    cv_f[1, :, 0] = [1, 1, 1, 1, 1, 1]      # the positives right: 2/3 and 1/3
    cv_f[2, :, 0] = [-1, -1, 1, -1, 1, -1]      # 2/3 and 3/3
    cv_f[1:, :, 1] = 800.      # exp(-800) is 0 in f64: f* = 0 predicts class 0, as scikit-learn's f* > 0 does
    cv_f[2, :, 1] = [0, 0, 0, 0, 0, 800.]
    test_f, test_var = np.zeros((3, 2, 2)), np.zeros((3, 2))
    test_f[2, :, 0] = [0., 3.]
    mean, best, proba = tabular._gp_select(cv_f, status, folds, y, 2, test_f, test_var)
    assert np.isnan(mean[0]) and mean[1] == 0.5 and mean[2] == (2 / 3 + 3 / 3) / 2 and best == 2
    assert abs(proba[0] - 0.5) < 1e-8 and abs(proba[1] - gf.proba(np.array([3.]), np.array([0.]))[0]) < 1e-12 and 0.9 < proba[1] < 1      # (the mixture's own 0.5 is 0.499999995)
    cv_f[2] = cv_f[1]
    assert tabular._gp_select(cv_f, status, folds, y, 2, test_f, test_var)[1] == 1      # NaN last, then the first of the tied
    status[:, :2, 0] = hipops.GPC_ONE_CLASS
    with pytest.raises(ValueError, match='every fit'):
        tabular._gp_select(cv_f, status, folds, y, 2, test_f, test_var)


def test_argument_errors_return_before_any_launch():
    lib = _hip.lib()
    buf = torch.zeros(4096)      # host memory: a refused call never looks at it
    p = buf.data_ptr()

    def lml(P=1, n=8, F=3, NC=2, n_splits=4, theta=p, status=p):
        return lib.pfn_gpc_lml_grad(theta, p, p, p, P, n, F, NC, n_splits, p, p, status, 0)

    def predict(P=1, n=8, T=2, F=3, NC=2, n_splits=4, theta=p, status=p):
        return lib.pfn_gpc_predict(theta, p, p, p, p, P, n, T, F, NC, n_splits, p, p, p, status, 0)
    for kw in (dict(n=3), dict(n=113), dict(F=0), dict(F=129), dict(NC=0), dict(NC=65)):
        assert lml(**kw) == PFN_ERR_UNSUPPORTED and predict(**kw) == PFN_ERR_UNSUPPORTED, kw
    assert b'4 .. 112' in lib.pfn_last_error_string()
    for kw in (dict(T=0), dict(T=129)):
        assert predict(**kw) == PFN_ERR_UNSUPPORTED, kw
    for kw in (dict(P=0), dict(n_splits=1), dict(n_splits=6), dict(theta=0), dict(status=0)):
        assert lml(**kw) == PFN_ERR_ARGUMENT and predict(**kw) == PFN_ERR_ARGUMENT, kw
    assert lml(n=3, theta=0) == PFN_ERR_UNSUPPORTED      # the shapes first, before any pointer is looked at


def test_python_checks_raise_before_the_device_is_asked_for():
    fold = torch.zeros(1, 8, dtype=torch.int32)
    x, y, tx, th = torch.zeros(1, 8, 3), torch.zeros(1, 8), torch.zeros(1, 2, 3), torch.zeros(1, 2, 6, 2)
    with pytest.raises(ValueError, match='n = 3'):
        hipops.gpc_lml_grad(th, torch.zeros(1, 3, 2), torch.zeros(1, 3), torch.zeros(1, 3, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match='n = 113'):
        hipops.gpc_check(113, 1, 1)
    with pytest.raises(ValueError, match='NC = 65'):
        hipops.gpc_predict(torch.zeros(1, 65, 6, 2), x, y, tx, fold, 4)
    with pytest.raises(ValueError):
        hipops.gpc_lml_grad(torch.zeros(1, 2, 5, 2), x, y, fold, 4)      # theta per slot
    with pytest.raises(ValueError):
        hipops.gpc_lml_grad(th, x, y, fold, 6)
    with pytest.raises(ValueError, match='F = 129'):
        tabular.gp_metric(torch.zeros(8, 129), torch.zeros(8), torch.zeros(2, 129), torch.zeros(2), [])
    with pytest.raises(ValueError, match='one class'):      # as scikit-learn's fit raises
        tabular.gp_metric(torch.randn(8, 3), torch.ones(8), torch.randn(2, 3), torch.zeros(2), [])
    # with sound arguments the product path asks for the GPU: there is no CPU fall-back
    with pytest.raises(_hip.HipExtensionError):
        hipops.gpc_lml_grad(th, x, y, fold, 4)
    with pytest.raises(_hip.HipExtensionError):
        hipops.gpc_predict(th, x, y, tx, fold, 4)
    with pytest.raises(_hip.HipExtensionError):
        tabular.gp_metric(torch.randn(8, 3), torch.tensor([0., 1.] * 4), torch.randn(2, 3), torch.zeros(2), [])
