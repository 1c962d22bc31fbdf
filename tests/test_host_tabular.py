"""Host-side checks of the tabular study's evaluation (csrc/tabular.hip, tabular.py, hipops.py): the C ABI and the build, the kernels' descriptor budgets, the
fold assignment against scikit-learn's own, the host half of the kNN grid search against the recorded GridSearchCV results (with a numpy stand-in for the
kernel's integer counts), the svmlight loader, and the shape checks that must answer without a GPU.  No GPU."""
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tabular_cases as cases      # noqa: E402

from transformerscandobayesianinference_amd import _hip, hipops, tabular      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pfn_tabular_windows', 'pfn_auc_counts', 'pfn_knn_cv')
PFN_ERR_UNSUPPORTED, PFN_ERR_ALIGNMENT, PFN_ERR_ARGUMENT = -1, -2, -4


@pytest.fixture(scope='module')
def recorded():
    return torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_knn_sklearn.pt'), weights_only=False)


def test_the_three_symbols_are_declared_exported_and_bound_at_abi_10():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    source = open(os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc', 'tabular.hip')).read()      # the entry points stand beside their kernels
    lib = _hip.lib()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in _hip.SIGNATURES and hasattr(lib, name)
        assert re.search(r'^int ' + name + r'\s*\(', source, re.M), name      # defined there ...
    for launcher in ('launch_tab_windows', 'launch_auc_counts', 'launch_knn_cv'):
        assert re.search(r'\b' + launcher + r'\s*\(', source), launcher      # ... and wired to its launcher
    assert _hip.ABI_VERSION == 10 and lib.pfn_abi_version() == 10 and '#define PFN_ABI_VERSION 10' in header
    assert '#define PFN_TAB_NORM_WITH_TEST 0' in header and '#define PFN_TAB_NORM_TRAIN_ONLY 1' in header
    assert (hipops.TAB_NORM_WITH_TEST, hipops.TAB_NORM_TRAIN_ONLY) == (0, 1)
    for name in ('tabular_windows', 'auc_counts', 'knn_cv'):
        assert callable(getattr(hipops, name)), name
    build = open(os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc', 'build.sh')).read()
    assert 'tabular.hip' in build and '../_build/tabular.o' in build      # compiled and linked


def test_new_kernels_keep_their_register_scratch_and_lds_budgets(tmp_path):
    """Read off the compiler's kernel descriptors (hipcc -S of tabular.hip with the flags of csrc/build.sh): no scratch anywhere; pfn_knn_cv within 128 VGPRs
    (four waves per SIMD) with all its rows in DYNAMIC LDS, which its launcher sizes -- at most 133,120 bytes at n = T = F = 128, inside the CU's 160 KB --;
    the windows kernel's static LDS is one statistics record per table column, the AUC kernel's one column of 4096 scores and flags."""
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    src = os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc', 'tabular.hip')
    asm = str(tmp_path / 'tabular.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', src, '-o', asm], check=True, capture_output=True)
    vgpr_cap = {'tab_windows_kernel': 256, 'auc_counts_kernel': 256, 'knn_cv_kernel': 128}
    lds_cap = {'tab_windows_kernel': 1024 * 24, 'auc_counts_kernel': 4096 * 5 + 128, 'knn_cv_kernel': 128}
    seen = set()
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', open(asm).read(), re.S):
        name, body = m.group(1), m.group(2)
        kernel = re.search(r'[a-z_]+_kernel', name).group(0)
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= vgpr_cap[kernel], name
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1)) <= lds_cap[kernel], name
        seen.add(kernel)
    assert seen == set(vgpr_cap)
    # the launcher's dynamic LDS at the largest supported problem: (128 + 128) rows of 129 floats, 128 labels and folds
    assert (128 + 128) * 129 * 4 + 128 * 8 == 133120 <= 160 * 1024


def _class_patterns(n):
    alt = np.arange(n) % 2
    yield 'alternating', alt
    yield 'sorted', np.sort(alt)
    one = np.zeros(n, dtype=np.int64)
    one[n // 2] = 1
    yield '1 positive', one
    two = np.zeros(n, dtype=np.int64)
    two[[0, n - 1]] = 1
    yield '2 positives', two
    for seed in range(5):
        yield f'random {seed}', np.random.RandomState(seed).randint(0, 2, n)


@pytest.mark.parametrize('n', [4, 5, 9, 10, 11, 30, 128])
def test_stratified_folds_equal_sklearns(n):
    pytest.importorskip('sklearn')
    from sklearn.model_selection import StratifiedKFold
    raised = 0
    for n_splits in sorted({2, min(5, n // 2), min(5, n)}):
        for what, y in _class_patterns(n):
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    want = np.empty(n, dtype=np.int32)
                    for f, (_, test) in enumerate(StratifiedKFold(n_splits).split(np.zeros(n), y)):
                        want[test] = f
            except ValueError:
                raised += 1
                with pytest.raises(ValueError):
                    tabular._stratified_folds(y, n_splits)
                continue
            with warnings.catch_warnings():
                warnings.simplefilter('error')      # where sklearn merely warns, the port goes on without a word
                got = tabular._stratified_folds(y, n_splits)
            assert got.dtype == np.int32 and np.array_equal(got, want), (n, n_splits, what)
            assert np.array_equal(tabular._stratified_folds(y.astype(np.float32) > 0.5, n_splits), want)      # the form knn_metric passes
    if n <= 5:
        assert raised > 0      # e.g. one positive and n - 1 < n_splits negatives
    with pytest.raises(ValueError):
        tabular._stratified_folds(np.arange(n) % 2, n + 1)
    with pytest.raises(ValueError):
        tabular._stratified_folds(np.arange(n) % 2, 1)


def test_knn_host_pipeline_reproduces_gridsearchcv_from_integer_counts(recorded):
    tied, split, nan_score = 0, 0, 0
    for rec, (n, T, F, _) in zip(recorded['problems'], cases.KNN_SKLEARN_PROBLEMS):
        x, y, tx = rec['x'], rec['y'], rec['test_x']
        assert x.shape == (n, F) and tx.shape == (T, F)
        gx, gy, gtx, gty = cases.knn_problem(n, T, F, rec['seed'])      # the generator still draws what was recorded
        assert torch.equal(gx, x) and torch.equal(gy, y) and torch.equal(gtx, tx) and torch.equal(gty, rec['test_y'])
        ks, n_splits = tabular._knn_grid(n)
        assert n_splits == rec['n_splits'] and len(ks) == len(rec['mean_test_score'])
        folds = tabular._stratified_folds(y.numpy() > 0.5, n_splits)
        assert np.array_equal(folds, rec['folds'].numpy())
        test_nbr, _, cv_nbr, _ = cases.knn_lists_f64(x, tx, folds)
        cv_correct, test_pos = cases.counts_from_lists(y, folds, n_splits, test_nbr, cv_nbr)
        mean, best, proba = tabular._knn_select(cv_correct, folds, n_splits, ks, test_pos)
        want = rec['mean_test_score'].numpy()
        assert mean.dtype == np.float64 and mean.tobytes() == want.tobytes(), (n, T, F, mean, want)      # bit for bit, NaN included
        assert best == rec['best_k'] and np.array_equal(proba, rec['proba'].numpy())
        top = np.nanmax(want)
        tied += int((want == top).sum() > 1 and best == 1 + int(np.flatnonzero(want == top)[0]))
        nan_score += int(np.isnan(want).any())
        cls = y.numpy() > 0.5
        split += int(any(cls[cv_nbr[q, 0]] != cls[cv_nbr[q, 1]] for q in range(n) if cv_nbr[q, 1] >= 0))
    assert tied > 0 and split > 0 and nan_score > 0      # two k tied in mean score (the first wins); a split vote at k = 2; a k beyond a fold's training rows


def test_knn_select_breaks_ties_as_documented():
    folds = np.array([0, 0, 1, 1, 0, 1], dtype=np.int32)
    cv_correct = np.zeros((5, 5), dtype=np.int64)
    cv_correct[:, 0], cv_correct[:, 1] = [1, 2, 2, 0, 0], [2, 1, 1, 0, 0]      # k = 1, 2, 3 all score (1/3 + 2/3) / 2 or its mirror
    test_pos = np.array([[1, 1, 2, 2, 3], [0, 1, 1, 2, 2]])
    mean, best, proba = tabular._knn_select(cv_correct, folds, 2, np.arange(1, 5), test_pos)
    assert np.isnan(mean[3]) and best == 1 and proba.tolist() == [1., 0.]      # k = 4 exceeds the 3 training rows; the first of the tied maxima wins
    cv_correct[1, 0] = 3
    mean, best, proba = tabular._knn_select(cv_correct, folds, 2, np.arange(1, 5), test_pos)
    assert best == 2 and proba.tolist() == [.5, .5]
    assert tabular._knn_grid(4)[0].tolist() == [1, 2] and tabular._knn_grid(4)[1] == 2 and tabular._knn_grid(7)[0].tolist() == [1, 2, 3, 4, 5]
    assert tabular._knn_grid(7)[1] == 3 and tabular._knn_grid(100)[1] == 5


def test_auc_from_counts_is_the_rational_and_nan_without_pairs(recorded):
    counts = torch.tensor([[2, 2, 3, 1], [3, 0, 0, 0], [0, 4, 0, 0], [1, 1, 0, 1]])
    auc = hipops.auc_from_counts(counts)
    assert auc.dtype == np.float64 and auc[0] == 7 / 8 and np.isnan(auc[1]) and np.isnan(auc[2]) and auc[3] == 0.5
    for T, C in [(2, 1), (63, 3), (65, 40)]:      # the numpy pair count and the recorded roc_auc_score are f64 evaluations of the same rational
        for kind in cases.AUC_KINDS:
            scores, labels = cases.auc_case(T, C, kind)
            rec = recorded['auc'][cases.auc_key(T, C, kind)]
            assert float(scores.double().sum() + 3 * labels.double().sum()) == rec['checksum']
            assert np.abs(hipops.auc_from_counts(torch.from_numpy(cases.pair_counts(scores, labels))) - rec['auc'].numpy()).max() <= 1e-12


def test_load_svmlight_table_balances_interleaves_and_flips(tmp_path):
    # rows 0 .. 11; positives (+1) are rows 1, 4, 7, 10 (the rarer class), feature 1 carries the row number, feature 3 is sparse
    lines = []
    for i in range(12):
        label = '+1' if i % 3 == 1 else '-1'
        lines.append(f'{label} 1:{i}.0' + (f' 3:{10 * i}.5' if i % 2 else '') + ('   # a comment' if i == 5 else ''))
    path = tmp_path / 'table.txt'
    path.write_text('\n'.join(lines) + '\n\n')
    X, y = tabular.load_svmlight_table(str(path))
    # by hand: stable sort by label -> negatives 0 2 3 5 6 8 9 11 then positives 1 4 7 10; the last 2 * 4 rows: 6 8 9 11 | 1 4 7 10;
    # interleaved 6 1 8 4 9 7 11 10; flipped
    order = [10, 11, 7, 9, 4, 8, 1, 6]
    assert X.dtype == torch.float32 and y.dtype == torch.float32 and X.shape == (8, 3)
    assert X[:, 0].tolist() == [float(i) for i in order]
    assert X[:, 1].tolist() == [0.] * 8
    assert X[:, 2].tolist() == [10 * i + .5 if i % 2 else 0. for i in order]
    assert y.tolist() == [1., 0., 1., 0., 1., 0., 1., 0.]
    # more positives than negatives: the negatives are kept whole and come second in each pair before the flip
    path.write_text('\n'.join(f'{"-1" if i in (2, 5) else "+1"} 1:{i}' for i in range(7)) + '\n')
    X, y = tabular.load_svmlight_table(str(path))
    # by hand: stable sort by -y -> positives 0 1 3 4 6 then negatives 2 5; the last 4 rows: 4 6 | 2 5; interleaved 4 2 6 5; flipped
    assert X[:, 0].tolist() == [5., 6., 2., 4.] and y.tolist() == [0., 1., 0., 1.]


def test_the_diabetes_fixture_is_balanced_and_alternating():
    d = torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_diabetes.pt'))
    assert d['X'].shape == (160, 8) and d['X'].dtype == torch.float32 and d['y'].shape == (160,)
    assert set(d['y'].tolist()) == {0., 1.} and bool((d['y'][::2] != d['y'][1::2]).all())


def test_out_of_range_shapes_are_refused_without_a_gpu():
    lib = _hip.lib()
    buf = torch.zeros(4096)      # host memory: a refused call never looks at it
    p = buf.data_ptr()
    assert p % 16 == 0
    win = lambda N=100, F=8, F_out=8, W=2, bptt=10, sep=5, rescale=1., mode=0, x_out=p: lib.pfn_tabular_windows(p, p, p, N, F, F_out, W, bptt, sep, rescale, mode, x_out, p, 0)
    assert win(F=0) == PFN_ERR_UNSUPPORTED and win(F=1025, F_out=1025) == PFN_ERR_UNSUPPORTED and win(F_out=7) == PFN_ERR_UNSUPPORTED
    assert b'1024' in lib.pfn_last_error_string()
    for kw in (dict(mode=2), dict(N=0), dict(W=0), dict(sep=0), dict(sep=10), dict(sep=11, mode=1), dict(rescale=0.), dict(rescale=float('nan')), dict(x_out=0)):
        assert win(**kw) == PFN_ERR_ARGUMENT, kw
    assert win(x_out=p + 4) == PFN_ERR_ALIGNMENT
    auc = lambda T, C, s=p: lib.pfn_auc_counts(s, p, T, C, p, 0)
    assert auc(0, 1) == PFN_ERR_UNSUPPORTED and auc(4097, 1) == PFN_ERR_UNSUPPORTED and auc(5, 0) == PFN_ERR_ARGUMENT and auc(5, 1, 0) == PFN_ERR_ARGUMENT
    knn = lambda P, n, T, F, tr=p: lib.pfn_knn_cv(tr, p, p, p, P, n, T, F, p, p, p, 0)
    for n, T, F in ((3, 1, 1), (129, 1, 1), (4, 0, 1), (4, 129, 1), (4, 1, 0), (4, 1, 129)):
        assert knn(1, n, T, F) == PFN_ERR_UNSUPPORTED, (n, T, F)
    assert b'4 .. 128' in lib.pfn_last_error_string()
    assert knn(0, 4, 1, 1) == PFN_ERR_ARGUMENT and knn(1, 4, 1, 1, 0) == PFN_ERR_ARGUMENT


def test_python_shape_checks_raise_before_the_device_is_asked_for():
    X, y = torch.zeros(30, 3), torch.zeros(30)      # CPU tensors: a shape error comes first, the missing GPU second
    with pytest.raises(ValueError, match='leaves the table'):
        hipops.tabular_windows(X, y, [0, 21], 10, 5)
    with pytest.raises(ValueError, match='leaves the table'):
        hipops.tabular_windows(X, y, [-1], 10, 5)
    with pytest.raises(ValueError):
        hipops.tabular_windows(X, y, [0], 10, 10)      # WITH_TEST needs a test row
    with pytest.raises(ValueError):
        hipops.tabular_windows(X, y, [0], 10, 5, F_out=2)
    with pytest.raises(ValueError):
        hipops.tabular_windows(X, y[:5], [0], 10, 5)
    with pytest.raises(ValueError):
        hipops.auc_counts(torch.zeros(4097, 1), torch.zeros(4097, 1))
    with pytest.raises(ValueError):
        hipops.auc_counts(torch.zeros(5, 2), torch.zeros(5, 1))
    fold = torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match='n = 3'):
        hipops.knn_cv(torch.zeros(1, 3, 2), torch.zeros(1, 3), torch.zeros(1, 4, 2), fold)
    with pytest.raises(ValueError, match='F = 129'):
        tabular.knn_metric(torch.zeros(8, 129), torch.zeros(8), torch.zeros(2, 129), torch.zeros(2), [])
    with pytest.raises(ValueError):
        tabular.evaluate_position(X, y, [], tabular.knn_metric, 10, 10)
    with pytest.raises(ValueError, match='no window'):
        tabular.evaluate_position(X, y, [], tabular.knn_metric, 30, 5)
    # with sound shapes the product path asks for the GPU: there is no CPU fall-back
    with pytest.raises(_hip.HipExtensionError):
        hipops.tabular_windows(X, y, [0, 20], 10, 5)
    with pytest.raises(_hip.HipExtensionError):
        hipops.auc_counts(torch.zeros(5, 2), torch.zeros(5, 2))
    with pytest.raises(_hip.HipExtensionError):
        tabular.evaluate_position(X, y, [], torch.nn.Linear(3, 1), 10, 5)


def test_window_selection_is_the_references_draw_and_leaves_the_generator_alone():
    torch.manual_seed(99)
    before = torch.random.get_rng_state()
    sel = tabular.select_windows(160, 50, 5)
    assert torch.equal(torch.random.get_rng_state(), before)
    with torch.random.fork_rng():
        torch.random.manual_seed(13)
        want = torch.randperm(110)[:5]
    assert torch.equal(sel, want) and len(tabular.select_windows(12, 10, 40)) == 2


def test_a_user_metric_function_is_looped_per_window_as_the_reference_loops():
    """batch_pred with a callable that has no batched form: torch's normalisation per window, one call per window, outputs [T, W] -- on the CPU."""
    g = torch.Generator().manual_seed(3)
    eval_xs, eval_ys = torch.randn(9, 4, 3, generator=g), (torch.rand(9, 4, generator=g) > 0.5).float()
    seen = []

    def metric(x, y, test_x, test_y, cat):
        seen.append((x, test_x, cat))
        return float(len(seen)), test_x[:, 0].numpy() * 2
    metrics, outputs = tabular.batch_pred(metric, eval_xs, eval_ys, ['c'], start=6)
    assert metrics.tolist() == [1., 2., 3., 4.] and outputs.shape == (3, 4) and len(seen) == 4
    for w, (x, test_x, cat) in enumerate(seen):
        raw = eval_xs[:, w]
        want = (raw - raw[:6].mean(0)) / (raw[:6].std(0) + .000001)
        assert torch.equal(x, want[:6]) and torch.equal(test_x, want[6:]) and cat == ['c']
        assert np.array_equal(outputs[:, w], want[6:, 0].numpy() * 2)
