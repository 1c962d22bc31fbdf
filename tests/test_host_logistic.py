"""Host-side checks of the logistic-regression baseline (csrc/logistic.hip, tabular.logistic_metric, hipops.logistic_cv): the C ABI and the build, the kernel's
descriptor budgets, the f64 restatement's optimality certificates, the grid against scikit-learn's ParameterGrid, the host half of the grid search against the
recorded results, and the argument checks that must answer without a GPU.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logistic_f64 as lf      # noqa: E402

from transformerscandobayesianinference_amd import _hip, hipops, tabular      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc')
PFN_ERR_UNSUPPORTED, PFN_ERR_ARGUMENT = -1, -4


@pytest.fixture(scope='module')
def recorded():
    return torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_logistic.pt'), weights_only=False)


def test_the_symbol_is_declared_exported_and_bound_at_abi_10():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    source = open(os.path.join(CSRC, 'logistic.hip')).read()      # the entry point stands beside its kernel
    lib = _hip.lib()
    assert re.search(r'\bpfn_logistic_cv\s*\(', header)
    assert 'pfn_logistic_cv' in _hip.SIGNATURES and hasattr(lib, 'pfn_logistic_cv') and len(_hip.SIGNATURES['pfn_logistic_cv'][1]) == 17
    assert re.search(r'^extern "C" int pfn_logistic_cv\s*\(', source, re.M)      # defined there ...
    assert re.search(r'\blaunch_logit_cv\s*\(', source)      # ... and wired to its launcher
    assert _hip.ABI_VERSION == 10 and lib.pfn_abi_version() == 10 and '#define PFN_ABI_VERSION 10' in header
    for name, value in (('NONE', 0), ('L1', 1), ('L2', 2), ('FIT_INTERCEPT', 4), ('FOLDS', 5), ('SLOTS', 6), ('MAX_CANDIDATES', 64), ('UNUSED', 0), ('CONVERGED', 1),
                        ('STALLED', 2), ('CAPPED', 3), ('ONE_CLASS', 4), ('NONFINITE', 5)):
        assert f'#define PFN_LOGIT_{name} {value}\n' in header and getattr(hipops, 'LOGIT_' + name) == value, name
    assert (lf.NONE, lf.L1, lf.L2, lf.FIT_INTERCEPT) == (hipops.LOGIT_NONE, hipops.LOGIT_L1, hipops.LOGIT_L2, hipops.LOGIT_FIT_INTERCEPT)
    assert callable(hipops.logistic_cv) and callable(hipops.logistic_cv_check) and callable(tabular.logistic_metric) and callable(tabular.logistic_metric.batched)
    build = open(os.path.join(CSRC, 'build.sh')).read()
    assert 'logistic.hip' in build and '../_build/logistic.o' in build      # compiled and linked
    assert 'logit' not in open(os.path.join(CSRC, 'tabular.hip')).read()      # a file of its own


def lds_bytes(n, F):
    """The launcher's dynamic LDS (logistic.hip logit_cv_lds_bytes), in floats: the n rows and the F + 1 rows of H at the odd stride (F + 1) | 1, six vectors over
    the rows (sign, mask, sigma, gradient weight, curvature weight, x . delta), five over the F + 1 coordinates (w, gradient, direction, alive, trial point),
    eight words of reduction space."""
    stride = (F + 1) | 1
    return 4 * ((n + F + 1) * stride + 6 * n + 5 * (F + 1) + 8)


def test_the_kernel_keeps_its_register_scratch_and_lds_budgets(tmp_path):
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    asm = str(tmp_path / 'logistic.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', os.path.join(CSRC, 'logistic.hip'), '-o', asm], check=True,
                   capture_output=True)
    found = re.findall(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', open(asm).read(), re.S)
    assert len(found) == 1 and 'logit_cv_kernel' in found[0][0]
    body = found[0][1]
    static_lds = int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1))
    assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0      # no scratch
    assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 128      # four waves per SIMD
    assert static_lds <= 512      # (the block-wide counts' words; everything else is dynamic)
    # the largest supported fit: 257 rows of 129 floats, 768 + 645 + 8 words of vectors
    assert lds_bytes(128, 128) == 4 * (257 * 129 + 768 + 645 + 8) == 138296 and lds_bytes(128, 128) + static_lds <= 160 * 1024
    # the study's shape: 141 rows of 61 floats, 480 + 305 + 8 words: four blocks share a CU's 160 KB
    assert lds_bytes(80, 60) == 4 * (141 * 61 + 480 + 305 + 8) == 37576 and 4 * (lds_bytes(80, 60) + static_lds) <= 160 * 1024
    text = open(os.path.join(CSRC, 'logistic.hip')).read()
    assert '((size_t)(n + F + 1) * ((F + 1) | 1) + 6 * (size_t)n + 5 * (size_t)(F + 1) + 8) * 4' in text


def _certificate(x, y, mask, w, C, kind):
    return lf.kkt(x, y, mask, w, C, kind) / (lf.effective_C(C, kind) * lf.scale(x, mask, kind))


def test_f64_fits_carry_their_kkt_certificate(recorded):
    """Every recorded f64 fit that ended 'converged' is optimal to 1e-10 of the scale C max_j sum_i m_i |x_ij| (the solver stops at 1e-13); a fresh run of the
    restatement on the small problems gives the recorded coefficients; what does not converge is 'none' on separable rows, or a one-class fold."""
    cands = recorded['cands']
    assert cands == lf.distinct_fits(lf.grid_entries())[0]
    seen = {lf.CONVERGED: 0, lf.CAPPED: 0, lf.ONE_CLASS: 0}
    for rec, (n, F, T) in zip(recorded['problems'], lf.SHAPES):
        x, y, folds, ns = rec['x'].numpy(), rec['y'].numpy(), rec['folds'].numpy(), rec['n_splits']
        gx, gy, gtx, gty = lf.problem(n, F, T, rec['seed'])      # the generator still draws what was recorded
        assert x.shape == (n, F) and np.array_equal(gx, x) and np.array_equal(gy, y) and np.array_equal(gtx, rec['test_x'].numpy())
        assert np.array_equal(folds, tabular._stratified_folds(y > 0.5, ns)) and ns == min(5, n // 2)
        coef, status = rec['coef'].numpy(), rec['status'].numpy()
        for c, (C, kind) in enumerate(cands):
            for s in range(ns + 1):
                mask = np.ones(n) if s == ns else (folds != s).astype(np.float64)
                reason = int(status[c, s, 0])
                seen[reason] += 1
                if reason == lf.CONVERGED:
                    assert _certificate(x, y, mask, coef[c, s], C, kind) <= 1e-10, (n, F, C, kind, s)
                elif reason == lf.CAPPED:
                    assert kind & 3 == lf.NONE and ((lf.design(x, kind) @ coef[c, s][:F + (kind >> 2)]) * lf.signs(y) > 0)[mask > 0].all()
                if n <= 10:
                    w, again, _ = lf.fit(x, y, mask, C, kind)
                    assert again == reason
                    if reason == lf.CONVERGED:
                        assert np.abs(w - coef[c, s]).max() <= 1e-9 * max(np.abs(w).max(), 1e-300) or not (w.any() or coef[c, s].any())
            assert not status[c, ns + 1:].any() and not coef[c, ns + 1:].any()
        if F >= 3:
            assert not coef[:, :, 1].any()      # the all-zero column: exactly 0 under every penalty
    assert seen[lf.CONVERGED] > 500 and seen[lf.CAPPED] > 0


def test_grid_enumeration_is_parametergrids_and_maps_onto_26_fits():
    reference = {'solver': ['saga'], 'penalty': ['l1', 'l2', 'none'], 'tol': [1e-2, 1e-4, 1e-10], 'max_iter': [500], 'fit_intercept': [True, False],
                 'C': [1e-5, 0.001, 0.01, 0.1, 1.0, 2.0]}
    assert tabular.param_grid['logistic'] == reference == lf.PARAM_GRID
    entries, cands, entry_fit = tabular._logistic_grid()
    assert entries == lf.grid_entries() and len(entries) == 108
    want_cands, want_fit = lf.distinct_fits(entries)
    assert cands == want_cands and np.array_equal(entry_fit, want_fit) and len(cands) == 26
    assert sum(1 for _, k in cands if k & 3 == hipops.LOGIT_NONE) == 2 and all(C == 1.0 for C, k in cands if k & 3 == hipops.LOGIT_NONE)
    for e, f in zip(entries, entry_fit):      # an entry's fit has its penalty, intercept and (but for 'none') C
        C, kind = cands[f]
        assert kind & 3 == hipops.LOGIT_PENALTIES[e['penalty']] and bool(kind & 4) == e['fit_intercept'] and (e['penalty'] == 'none' or C == e['C'])
    model_selection = pytest.importorskip('sklearn.model_selection')
    assert entries == list(model_selection.ParameterGrid(reference))


def test_selection_reproduces_the_recorded_scores_from_the_recorded_counts(recorded):
    entry_fit = recorded['entry_fit'].numpy()
    entries = lf.grid_entries()
    nan_scores = 0
    for rec in recorded['problems']:
        status, folds, ns = rec['status'].numpy(), rec['folds'].numpy(), rec['n_splits']
        mean, best, proba = tabular._logistic_select(rec['cv_correct'].numpy(), status, folds, ns, entry_fit, rec['test_z'].numpy())
        want = rec['mean_test_score'].numpy()
        assert mean.dtype == np.float64 and mean.tobytes() == want.tobytes()      # bit for bit, NaN included
        assert best == rec['best'] and np.abs(proba - rec['proba'].numpy()).max() <= 2e-16
        top = np.nanmax(want)
        assert best == int(np.flatnonzero(want == top)[0])      # the FIRST maximum over the 108 entries
        assert entries[best]['tol'] == 1e-2      # (so of the three tol values that share a fit, the first)
        nan_scores += int(np.isnan(want).any())
        # the same from the oracle's own selection
        mean2, best2 = lf.select(rec['cv_correct'].numpy(), status[:, :, 0] == lf.ONE_CLASS, folds, ns, entry_fit)
        assert mean2.tobytes() == want.tobytes() and best2 == best


def test_selection_ranks_nan_last_and_raises_when_every_fit_failed():
    folds = np.array([0, 0, 1, 1, 0, 1], dtype=np.int32)
    entry_fit = np.array([0, 1, 1, 2])
    status = np.zeros((3, 6, 2), dtype=np.int32)
    status[:, :3, 0] = hipops.LOGIT_CONVERGED
    status[0, 1, 0] = hipops.LOGIT_ONE_CLASS      # candidate 0: a one-class training part in fold 1 -> its mean is NaN
    cv_correct = np.array([[3, 3, 0, 0, 0], [2, 1, 0, 0, 0], [1, 2, 0, 0, 0]])
    test_z = np.array([[9., 9.], [0., -2.], [1., 1.]])
    mean, best, proba = tabular._logistic_select(cv_correct, status, folds, 2, entry_fit, test_z)
    assert np.isnan(mean[0]) and mean[1] == mean[2] == mean[3] == 0.5 and best == 1      # NaN last, then the first of the tied
    assert proba[0] == 0.5 and abs(proba[1] - 1 / (1 + np.exp(2.))) < 1e-17
    status[:, :2, 0] = hipops.LOGIT_ONE_CLASS
    with pytest.raises(ValueError, match='every fit'):
        tabular._logistic_select(cv_correct, status, folds, 2, entry_fit, test_z)


def test_argument_errors_return_before_any_launch():
    lib = _hip.lib()
    buf = torch.zeros(4096)      # host memory: a refused call never looks at it
    p = buf.data_ptr()

    def call(P=1, n=8, T=2, F=3, NC=2, n_splits=4, train=p, cand=p, status=p, coef=p, stream=0):
        return lib.pfn_logistic_cv(train, p, p, p, cand, p, P, n, T, F, NC, n_splits, p, p, status, coef, stream)
    for kw in (dict(n=3), dict(n=129), dict(T=0), dict(T=129), dict(F=0), dict(F=129), dict(NC=0), dict(NC=65)):
        assert call(**kw) == PFN_ERR_UNSUPPORTED, kw
    assert b'4 .. 128' in lib.pfn_last_error_string()
    for kw in (dict(P=0), dict(n_splits=1), dict(n_splits=6), dict(train=0), dict(cand=0), dict(status=0)):
        assert call(**kw) == PFN_ERR_ARGUMENT, kw
    assert call(n=3, train=0) == PFN_ERR_UNSUPPORTED      # the shapes first, before any pointer is looked at


def test_python_checks_raise_before_the_device_is_asked_for():
    fold = torch.zeros(1, 8, dtype=torch.int32)
    x, y, tx = torch.zeros(1, 8, 3), torch.zeros(1, 8), torch.zeros(1, 2, 3)
    with pytest.raises(ValueError, match='n = 3'):
        hipops.logistic_cv(torch.zeros(1, 3, 2), torch.zeros(1, 3), torch.zeros(1, 4, 2), torch.zeros(1, 3, dtype=torch.int32), 2, [1.], [2])
    with pytest.raises(ValueError, match='NC = 65'):
        hipops.logistic_cv(x, y, tx, fold, 4, [1.] * 65, [2] * 65)
    with pytest.raises(ValueError):
        hipops.logistic_cv(x, y, tx, fold, 4, [1.], [3])      # no such penalty
    with pytest.raises(ValueError):
        hipops.logistic_cv(x, y, tx, fold, 4, [0.], [2])      # C > 0
    with pytest.raises(ValueError):
        hipops.logistic_cv(x, y, tx, fold, 6, [1.], [2])
    with pytest.raises(ValueError, match='F = 129'):
        tabular.logistic_metric(torch.zeros(8, 129), torch.zeros(8), torch.zeros(2, 129), torch.zeros(2), [])
    with pytest.raises(ValueError, match='one class'):      # as sklearn's fit raises
        tabular.logistic_metric(torch.randn(8, 3), torch.ones(8), torch.randn(2, 3), torch.zeros(2), [])
    # with sound arguments the product path asks for the GPU: there is no CPU fall-back
    with pytest.raises(_hip.HipExtensionError):
        hipops.logistic_cv(x, y, tx, fold, 4, [1.], [2])
    with pytest.raises(_hip.HipExtensionError):
        tabular.logistic_metric(torch.randn(8, 3), torch.tensor([0., 1.] * 4), torch.randn(2, 3), torch.zeros(2), [])
