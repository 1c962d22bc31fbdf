"""The tabular study's evaluation on the MI355X (csrc/tabular.hip; tabular.evaluate and what it calls): the window kernel against an f64 restatement, the
ROC-AUC pair counts against an O(T^2) numpy count and the recorded roc_auc_score, the kNN kernel against f64 brute-force neighbour lists, the kNN arm against
the recorded GridSearchCV results, the PFN arm against the reference's own loop over test rows (bounded by that loop's measured distance to the f64 oracle),
and `evaluate` end to end.  Fixtures only: no scikit-learn, no reference.  tests/tabular_cases.py holds the seeded inputs and the f64 restatements."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tabular_cases as cases      # noqa: E402

from oracle import pfn_oracle      # noqa: E402
from transformerscandobayesianinference_amd import _hip, encoders, hipops, tabular      # noqa: E402
from transformerscandobayesianinference_amd.transformer import TransformerModel      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -23
MEASURED = os.path.join(ROOT, 'profiles', 'r16_tabular_bounds_measured.json')


@pytest.fixture(scope='module')
def recorded():
    return torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_knn_sklearn.pt'), weights_only=False)


@pytest.fixture(scope='module')
def diabetes():
    d = torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_diabetes.pt'))
    return d['X'], d['y']


# ---- windows -------------------------------------------------------------------------------------------------------------------------------------------------
def table(N, F, seed):
    """Random columns of assorted scale and offset; from F = 3 on: column 0 constant, column 1 all zero, column 2 of mean 1000 and std 1."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, F, generator=g) * (0.5 + 3 * torch.rand(F, generator=g)) + 4 * torch.randn(F, generator=g)
    if F >= 3:
        X[:, 0] = 3.25
        X[:, 1] = 0.
        X[:, 2] = 1000. + torch.randn(N, generator=g)
    y = (torch.rand(N, generator=g) > 0.5).float()
    return X, y


@pytest.mark.parametrize('rescale', [1.0, 60 / 8])
@pytest.mark.parametrize('with_test', [True, False])
@pytest.mark.parametrize('N,F,F_out,bptt,sep,W', [(12, 1, 1, 3, 2, 2), (40, 3, 5, 10, 9, 4), (70, 8, 60, 50, 10, 20), (140, 61, 64, 100, 80, 7)])
def test_windows_against_the_f64_restatement(N, F, F_out, bptt, sep, W, with_test, rescale):
    X, y = table(N, F, seed=N)
    g = torch.Generator().manual_seed(N + 1)
    starts = [0, N - bptt] + torch.randint(0, N - bptt + 1, (W - 2,), generator=g).tolist()
    mode = hipops.TAB_NORM_WITH_TEST if with_test else hipops.TAB_NORM_TRAIN_ONLY
    Xd, yd = X.to(DEV), y.to(DEV)
    gx, gy = hipops.tabular_windows(Xd, yd, starts, bptt, sep, F_out=F_out, rescale=rescale, mode=mode)
    want, want_y, mean, std, raw = cases.windows_f64(X, y, starts, bptt, sep, F_out, rescale, with_test)
    T = bptt - sep
    assert gx.shape == want.shape == ((sep + 1, W * T, F_out) if with_test else (bptt, W, F_out)) and gy.shape == want_y.shape
    got = gx.double().cpu().numpy()
    assert np.isfinite(got).all()
    # the round-off of a centred f32 two-pass, element by element: 4 eps ((|x| + |mean|) / std + |result|)
    tol = 4 * EPS * ((np.abs(raw) + np.abs(mean)) / std + np.abs(want))
    assert np.array_equal(got[tol == 0], want[tol == 0])      # zeros normalised by zeros (the padding): nothing to round
    worst = float((np.abs(got - want)[tol > 0] / tol[tol > 0]).max())
    print(f'windows {(N, F, F_out, bptt, sep, W)} with_test={with_test} rescale={rescale:.3g}: max |error| / tolerance = {worst:.3f}')
    assert worst <= 1.0
    # the y rows and the column order w T + t, bit for bit; padding, constant and all-zero columns exactly 0
    assert np.array_equal(gy.cpu().numpy().astype(np.float64), want_y)
    assert not got[:, :, F:].any()
    if F >= 3:
        assert not got[:, :, :2].any() and np.abs(got[:, :, 2]).max() > 0.1
    # a window alone is the same bits as in the batch
    for w in sorted({0, 1, W - 1}):
        ax, ay = hipops.tabular_windows(Xd, yd, [starts[w]], bptt, sep, F_out=F_out, rescale=rescale, mode=mode)
        if with_test:
            assert torch.equal(ax, gx[:, w * T:(w + 1) * T]) and torch.equal(ay, gy[:, w * T:(w + 1) * T])
        else:
            assert torch.equal(ax, gx[:, w:w + 1]) and torch.equal(ay, gy[:, w:w + 1])


# ---- AUC -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,C', cases.AUC_SHAPES)
def test_auc_counts_are_integer_exact_and_match_roc_auc_score(T, C, recorded):
    for kind in cases.AUC_KINDS:
        scores, labels = cases.auc_case(T, C, kind)
        rec = recorded['auc'][cases.auc_key(T, C, kind)]
        assert float(scores.double().sum() + 3 * labels.double().sum()) == rec['checksum']
        counts = hipops.auc_counts(scores.to(DEV), labels.to(DEV))
        assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), cases.pair_counts(scores, labels)), (T, C, kind)
        auc = hipops.auc_from_counts(counts)
        assert not np.isnan(auc).any() and np.abs(auc - rec['auc'].numpy()).max() <= 1e-12
        got, undefined = tabular.roc_auc_columns(scores.to(DEV), labels.to(DEV))
        assert undefined == 0 and np.array_equal(got, auc)
    # all scores equal: every pair ties, AUC 1/2; an all-positive column: no pair, NaN, and counted
    scores, labels = cases.auc_case(T, C, 'ties')
    flat = torch.full_like(scores, 0.25)
    counts = hipops.auc_counts(flat.to(DEV), labels.to(DEV)).cpu().numpy()
    assert np.array_equal(counts, cases.pair_counts(flat, labels)) and not counts[:, 2].any() and np.array_equal(counts[:, 3], counts[:, 0] * counts[:, 1])
    assert (hipops.auc_from_counts(torch.from_numpy(counts)) == 0.5).all()
    labels[:, C - 1] = 1.
    auc, undefined = tabular.roc_auc_columns(scores.to(DEV), labels.to(DEV))
    assert undefined == 1 and np.isnan(auc[C - 1]) and not np.isnan(auc[:C - 1]).any()
    assert np.array_equal(hipops.auc_counts(scores.to(DEV), labels.to(DEV)).cpu().numpy(), cases.pair_counts(scores, labels))


# ---- kNN kernel ----------------------------------------------------------------------------------------------------------------------------------------------
def knn_launch(problems, folds):
    x = torch.stack([p[0] for p in problems]).to(DEV)
    y = torch.stack([p[1] for p in problems]).to(DEV)
    tx = torch.stack([p[2] for p in problems]).to(DEV)
    out = hipops.knn_cv(x, y, tx, torch.from_numpy(np.stack(folds)).to(DEV))
    return [o.cpu().numpy() for o in out]


def check_knn_problems(problems, exact_ties_ok=False):
    """The kernel against f64 brute force on a launch of problems of one shape.  Returns (queries left out, queries, the kernel's outputs, the folds)."""
    n = len(problems[0][1])
    n_splits = min(5, n // 2)
    folds = [tabular._stratified_folds(p[1].numpy() > 0.5, n_splits) for p in problems]
    cv_correct, test_pos, test_nbr = knn_launch(problems, folds)
    left_out = total = 0
    for i, (x, y, tx, _) in enumerate(problems):
        want_nbr, want_d, cv_nbr, cv_d = cases.knn_lists_f64(x, tx, folds[i])
        keep_t, keep_cv = cases.clear_of_near_ties(want_d, 1e-4, exact_ties_ok), cases.clear_of_near_ties(cv_d, 1e-4, exact_ties_ok)
        left_out += int((~keep_t).sum() + (~keep_cv).sum())
        total += len(keep_t) + len(keep_cv)
        assert np.array_equal(test_nbr[i][keep_t], want_nbr[keep_t, :5]), i
        want_correct, want_pos = cases.counts_from_lists(y, folds[i], n_splits, want_nbr, cv_nbr, keep_cv=keep_cv)
        assert np.array_equal(test_pos[i][keep_t], want_pos[keep_t]), i
        # cv_correct sums over a fold's rows: exact on the rows kept, and each row left out adds 0 or 1
        slack = np.zeros(5, dtype=np.int64)
        np.add.at(slack, folds[i][~keep_cv], 1)
        assert ((cv_correct[i] >= want_correct) & (cv_correct[i] <= want_correct + slack[None, :])).all(), (i, cv_correct[i], want_correct, slack)
        assert not cv_correct[i][:, n_splits:].any()
    return left_out, total, (cv_correct, test_pos, test_nbr), folds


@pytest.mark.parametrize('n,T,F', list(cases.KNN_KERNEL_SEEDS))
def test_knn_kernel_against_f64_brute_force(n, T, F):
    problems = [cases.knn_problem(n, T, F, s) for s in cases.KNN_KERNEL_SEEDS[(n, T, F)]]
    left_out, total, out, folds = check_knn_problems(problems)
    print(f'kNN {(n, T, F)}: {left_out} of {total} queries left out for near-tied neighbours')
    assert left_out <= 0.02 * total
    # a problem alone is the same bits as in the batch
    alone = knn_launch(problems[3:4], folds[3:4])
    for a, b in zip(alone, out):
        assert np.array_equal(a[0], b[3])


def test_knn_exact_ties_go_to_the_lower_index():
    """Train rows n / 2 .. n - 1 duplicate rows 0 .. n / 2 - 1 with the opposite label; half of the test rows sit exactly on a train row.  Equal distances are
    equal in f32 and in f64 (the same operations on the same numbers), and both sides order them by index."""
    problems = []
    for s in range(8):
        x, y, tx, ty = cases.knn_problem(24, 16, 6, 90 + s)
        x[12:], y[12:] = x[:12], 1 - y[:12]
        tx[:8] = x[2:10]
        problems.append((x, y, tx, ty))
    left_out, total, (cv_correct, test_pos, test_nbr), _ = check_knn_problems(problems, exact_ties_ok=True)
    assert left_out <= 0.02 * total
    for i in range(8):
        assert np.array_equal(test_nbr[i][:8, :2], np.stack([np.arange(2, 10), np.arange(14, 22)], 1))      # the original first, its duplicate second
        assert (test_pos[i][:8, 1] == 1).all()      # one of each label: a split vote at k = 2


def test_knn_unsupported_shapes_return_the_error_code():
    lib = _hip.lib()
    buf = torch.zeros(1 << 16, device=DEV)
    ints = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    p, q = buf.data_ptr(), ints.data_ptr()
    s = _hip.stream_ptr(buf.device)
    for n, T, F in ((3, 1, 1), (129, 1, 1), (4, 129, 1), (4, 1, 129), (4, 0, 1)):
        assert lib.pfn_knn_cv(p, p, p, q, 1, n, T, F, q, q, q, s) == -1, (n, T, F)
    assert lib.pfn_knn_cv(p, p, p, q, 1, 4, 1, 1, q, q, q, s) == 0
    torch.cuda.synchronize()


# ---- kNN arm end to end --------------------------------------------------------------------------------------------------------------------------------------
def test_knn_arm_reproduces_the_recorded_gridsearchcv(recorded):
    for rec in recorded['problems']:
        x, y, tx, ty = (rec[k].to(DEV) for k in ('x', 'y', 'test_x', 'test_y'))
        metric, proba, best = tabular.knn_metric.batched(x[:, None], y[:, None], tx[:, None], ty[:, None], return_k=True)
        what = (tuple(x.shape), tuple(tx.shape))
        assert best == [rec['best_k']], what
        assert proba.dtype == np.float64 and np.array_equal(proba[:, 0], rec['proba'].numpy()), what      # a ratio of small integers
        assert abs(metric[0] - rec['auc']) <= 1e-12, what
        one_metric, one_proba = tabular.knn_metric(x, y, tx, ty, [])
        assert one_metric == metric[0] and np.array_equal(one_proba, proba[:, 0])
    # problems of one shape in one launch: each as alone
    base = next(r for r in recorded['problems'] if tuple(r['test_x'].shape) == (90, 8))
    same = [base, dict(zip(('x', 'y', 'test_x', 'test_y'), cases.knn_problem(10, 90, 8, 321))), base]
    stack = lambda k: torch.stack([r[k] for r in same], 1).to(DEV)
    metric, proba = tabular.knn_metric.batched(stack('x'), stack('y'), stack('test_x'), stack('test_y'))
    for w, r in enumerate(same):
        m1, p1 = tabular.knn_metric(r['x'].to(DEV), r['y'].to(DEV), r['test_x'].to(DEV), r['test_y'].to(DEV), [])
        assert m1 == metric[w] and np.array_equal(p1, proba[:, w])


# ---- PFN arm -------------------------------------------------------------------------------------------------------------------------------------------------
def small_model(F, seed=0):
    """A BCE-shaped PFN (one output), 2 layers, 2 heads, exact-f32 kernels, seeded weights.  emsize 64: the narrowest two-head model the stack builds (its
    attention kernels start at head dim 32; emsize 32 with 2 heads is refused with PFN_ERR_UNSUPPORTED)."""
    torch.manual_seed(seed)
    m = TransformerModel(encoders.Linear(F, 64), 1, 64, 2, 128, 2, 0.0, y_encoder=encoders.Linear(1, 64), precision='f32')
    with torch.no_grad():
        for layer in m.transformer_encoder.layers:      # un-zero the residual branches
            for t in (layer.linear2.weight, layer.self_attn.out_proj.weight):
                t.normal_(0, 0.1)
    return m.to(DEV).eval()


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def record_measured(key, value):
    data = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}
    data[key] = value
    with open(MEASURED, 'w') as f:
        json.dump(data, f, indent=1, sort_keys=True)


@pytest.mark.parametrize('bptt,sep,max_samples', [(10, 9, 3), (50, 10, 5)])
def test_pfn_arm_against_the_references_loop(bptt, sep, max_samples, diabetes):
    """The new path -- every (window, test row) column from pfn_tabular_windows, one forward at batch W T -- against the reference's own form: a loop over test
    rows, torch's normalisation, model(...) at batch W.  Logits bound: 4 max(e, 2^-23) relative to the logits' norm, e the measured error of
    that looped, existing path against the f64 oracle on f64-normalised windows.  Measured on the MI355X (profiles/r16_tabular_bounds_measured.json)."""
    X, y = diabetes
    Xd, yd = X.to(DEV), y.to(DEV)
    model = small_model(8)
    T = bptt - sep
    metric, outputs, ys = tabular.evaluate_position(Xd, yd, [], model, bptt, sep, max_samples=max_samples)
    starts = tabular.select_windows(len(X), bptt, max_samples)
    W = len(starts)
    assert W == max_samples and metric.shape == (W,) and outputs.shape == (T, W) and outputs.dtype == np.float64 and ys.shape == (T, W)
    new = tabular.pfn_window_logits(Xd, yd, starts, model, bptt, sep)
    assert np.array_equal(torch.sigmoid(new).double().cpu().numpy(), outputs)
    # the reference's form, written out (tabular.py:238-299)
    with torch.random.fork_rng():
        torch.random.manual_seed(13)
        sel = torch.randperm(len(X) - bptt)[:max_samples]
    assert torch.equal(sel, starts)
    eval_xs = torch.stack([Xd[i:i + bptt] for i in sel.tolist()], 1)
    eval_ys = torch.stack([yd[i:i + bptt] for i in sel.tolist()], 1)
    assert torch.equal(ys, eval_ys[sep:])
    loop = torch.empty(T, W, device=DEV)
    with torch.no_grad():
        for i, pos in enumerate(range(sep, bptt)):
            eval_x = torch.cat([eval_xs[:sep], eval_xs[pos].unsqueeze(0)])
            eval_x = (eval_x - eval_x.mean(0)) / (eval_x.std(0) + .000001)
            loop[i] = model((eval_x / 1.0, eval_ys[:sep].float()), single_eval_pos=sep).squeeze(-1).squeeze(0)
    # the f64 oracle on f64-normalised windows
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if not k.startswith('criterion.')}
    x64, y64, _, _, _ = cases.windows_f64(X, y, sel.tolist(), bptt, sep, 8, 1.0, True)
    oracle = pfn_oracle.forward(sd, torch.from_numpy(x64), torch.from_numpy(y64), sep, 2).reshape(W, T).t()
    e, err_new = relerr(loop, oracle), relerr(new, oracle)
    bound = 4 * max(e, EPS)
    print(f'PFN arm {(bptt, sep, max_samples)}: looped path vs f64 oracle {e:.3e}, new path vs f64 oracle {err_new:.3e}, bound {bound:.3e}')
    record_measured(f'pfn_arm_bptt{bptt}_sep{sep}_W{W}', dict(looped_vs_oracle=e, new_vs_oracle=err_new, bound=bound, new_vs_looped=relerr(new, loop)))
    assert err_new <= bound
    # per-window AUC = the pair counts of the loop's outputs, wherever no two scores of the window are close enough for the bound to reorder them
    loop_auc, _ = tabular.roc_auc_columns(torch.sigmoid(loop), eval_ys[sep:])
    reach = 2 * bound * float(loop.double().norm())
    l64 = loop.double().cpu().numpy()
    clear = np.array([T < 2 or np.diff(np.sort(l64[:, w])).min() > reach for w in range(W)])
    skipped = float((~clear).mean())
    print(f'PFN arm {(bptt, sep, max_samples)}: {skipped:.0%} of the windows have two scores within {reach:.2e}')
    assert skipped < 0.05
    assert np.array_equal(metric[clear], loop_auc[clear], equal_nan=True)


def test_evaluate_returns_the_references_dict_and_loads_what_it_saved(diabetes, tmp_path, monkeypatch):
    X, y = diabetes
    datasets = [['first', X, y, []], ['second', X.flip(0).contiguous(), y.flip(0).contiguous(), []]]
    model = small_model(12, seed=1)
    positions = [5, 10]
    kw = dict(max_features=12, extend_features=True, rescale_features=True, max_samples=4, save_dir=tmp_path, path_interfix='t')
    res = tabular.evaluate(datasets, model, 'pfn', 20, positions, DEV, **kw)
    keys = {'metric', 'mean_metric'} | {f'mean_metric_at_{p}' for p in positions}
    for name in ('first', 'second'):
        keys |= {f'{name}_time'} | {f'{name}_{k}_at_{p}' for p in positions for k in ('mean_metric', 'per_ds_metric', 'outputs', 'ys')}
    assert set(res) == keys and res['metric'] == 'auc'
    for name, Xn, yn, _ in datasets:
        for p in positions:
            outputs, ys = res[f'{name}_outputs_at_{p}'], res[f'{name}_ys_at_{p}']
            assert outputs.shape == (20 - p, 4) and ys.shape == (20 - p, 4)
            pooled = hipops.auc_from_counts(hipops.auc_counts(torch.from_numpy(outputs).float().reshape(-1, 1).to(DEV), ys.reshape(-1, 1).to(DEV)))[0]
            assert res[f'{name}_mean_metric_at_{p}'] == pooled and 0. <= pooled <= 1.
            # the padded, rescaled windows are what a padded table and the factor 8 / 12 give
            m, o, _ = tabular.evaluate_position(torch.cat([Xn, torch.zeros(len(Xn), 4)], 1).to(DEV), yn.to(DEV), [], model, 20, p, rescale_features=8 / 12, max_samples=4)
            assert np.array_equal(o, outputs) and np.array_equal(m, res[f'{name}_per_ds_metric_at_{p}'], equal_nan=True)
    for p in positions:
        assert res[f'mean_metric_at_{p}'] == np.array([res[f'first_mean_metric_at_{p}'], res[f'second_mean_metric_at_{p}']]).mean()
    assert res['mean_metric'] == np.array([res[f'mean_metric_at_{p}'] for p in positions]).mean()
    assert sorted(os.listdir(tmp_path / 't')) == ['results_pfn_first.npy', 'results_pfn_second.npy']
    # a second call loads instead of recomputing
    def boom(*a, **k):
        raise AssertionError('recomputed')
    monkeypatch.setattr(tabular, 'evaluate_dataset', boom)
    again = tabular.evaluate(datasets, model, 'pfn', 20, positions, DEV, **kw)
    assert set(again) == keys
    for k in keys:
        a, b = res[k], again[k]
        assert (torch.equal(a, b) if torch.is_tensor(a) else np.array_equal(a, b, equal_nan=True) if isinstance(a, np.ndarray) else a == b), k
    with pytest.raises(AssertionError, match='recomputed'):
        tabular.evaluate(datasets, model, 'pfn', 20, positions, DEV, overwrite=True, **kw)
    monkeypatch.undo()
    # save_dir None: nothing read, nothing written; save=False keeps the per-window arrays out of the dict
    lean = tabular.evaluate(datasets[:1], model, 'pfn', 20, positions, DEV, max_features=12, extend_features=True, rescale_features=True, max_samples=4, save=False)
    assert set(lean) == {'metric', 'mean_metric', 'first_time'} | {f'{k}mean_metric_at_{p}' for p in positions for k in ('', 'first_')}
    assert all(lean[f'first_mean_metric_at_{p}'] == res[f'first_mean_metric_at_{p}'] for p in positions)


def test_knn_arm_through_evaluate_equals_the_per_window_loop(diabetes):
    """evaluate with knn_metric: the batched route (pfn_tabular_windows TRAIN_ONLY + one pfn_knn_cv launch) gives what the reference's loop gives -- torch's
    normalisation per window and one knn_metric call per window."""
    X, y = diabetes
    res = tabular.evaluate([['d', X, y, []]], tabular.knn_metric, 'knn', 30, [10, 20], DEV, max_samples=6)
    looped = lambda *a: tabular.knn_metric(*a)      # no `batched` attribute: batch_pred loops
    for p in (10, 20):
        metric, outputs, ys = tabular.evaluate_position(X.to(DEV), y.to(DEV), [], looped, 30, p, max_samples=6)
        assert outputs.shape == (30 - p, 6)
        assert np.array_equal(outputs, res[f'd_outputs_at_{p}']) and np.array_equal(metric, res[f'd_per_ds_metric_at_{p}'], equal_nan=True)
        assert torch.equal(ys.cpu(), res[f'd_ys_at_{p}'])
