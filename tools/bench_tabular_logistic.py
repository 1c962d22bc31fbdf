"""The tabular study's logistic-regression arm on the device, and scikit-learn's grid search on the same windows where scikit-learn is importable.

    python tools/bench_tabular_logistic.py [--out profiles/r17_tabular_logistic.json] [--sklearn-windows 2]

bptt 100, eval positions 10 / 20 / 40 / 80, 20 windows of a 60-feature table (the shapes of tools/bench_tabular.py):
logistic_batched   tabular.evaluate_position(logistic_metric): one TRAIN_ONLY window launch, the folds on the host, ONE pfn_logistic_cv launch for the
                   20 x 26 x 6 fits, the scores and the sigmoid on the host, one pfn_auc_counts launch; reported per call and per window
kernel             the pfn_logistic_cv launch alone on the same windows (hipops.logistic_cv, inputs resident), device-synchronised
logistic_sklearn   per window: GridSearchCV(LogisticRegression(), the reference's 108-entry grid, cv = 5) + predict_proba on the host, as the reference runs it
                   (saga, max_iter 500; 'none' spelled None for current scikit-learn).  It takes seconds per window, so it is timed ONCE on the first
                   --sklearn-windows windows of each position, not in the alternating rounds; without scikit-learn the device time stands alone and the
                   result says so.
There is no earlier implementation of this arm in this package: no ratio against a parent is claimed.  The sklearn figure is a different algorithm at a looser
tolerance on a different processor; it is context, not a like-for-like comparison.

Protocol: wall-clock time of whole calls, host work and transfers included, the device synchronised at both ends; both device variants are warmed up and
alternate for REPS rounds; the figure is the median round, the spread (max - min) / median.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformerscandobayesianinference_amd import hipops, tabular  # noqa: E402

REPS = 7
BPTT, WINDOWS, FEATURES = 100, 20, 60
POSITIONS = (10, 20, 40, 80)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--sklearn-windows', type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_tabular_logistic: no GPU -- nothing is measured without one')
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(1)
    N = BPTT + 3 * WINDOWS
    X = (torch.randn(N, FEATURES, generator=g) * (0.5 + torch.rand(FEATURES, generator=g)) + torch.randn(FEATURES, generator=g)).to(dev)
    w = torch.randn(FEATURES, generator=g).to(dev)
    y = ((X - X.mean(0)) @ w + torch.randn(N, generator=g).to(dev) > 0).float()
    starts = tabular.select_windows(N, BPTT, WINDOWS).tolist()
    try:
        from sklearn.linear_model import LogisticRegression
        from sklearn.model_selection import GridSearchCV
    except ImportError:
        LogisticRegression = None
    entries, cands, _ = tabular._logistic_grid()
    res = dict(bptt=BPTT, windows=WINDOWS, features=FEATURES, grid_entries=len(entries), distinct_fits=len(cands), reps=REPS, device=torch.cuda.get_device_name(0),
               sklearn='timed once on the first %d windows of each position' % a.sklearn_windows if LogisticRegression is not None
               else 'scikit-learn is not importable here: device time alone', positions={})
    for sep in POSITIONS:
        T = BPTT - sep
        keep = {}
        x_w, y_w = hipops.tabular_windows(X, y, starts, BPTT, sep, mode=hipops.TAB_NORM_TRAIN_ONLY)
        n_splits, _, _, operands = tabular._fold_problems(x_w[:sep], y_w[:sep], x_w[sep:])
        k_args = (*operands, n_splits, [c for c, _ in cands], [k for _, k in cands])

        def logistic_batched():
            keep['batched'] = tabular.evaluate_position(X, y, [], tabular.logistic_metric, BPTT, sep, max_samples=WINDOWS)

        def kernel():
            keep['kernel'] = hipops.logistic_cv(*k_args)

        variants = dict(logistic_batched=logistic_batched, kernel=kernel)
        times = {name: [] for name in variants}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for fn in variants.values():
                fn()
            for _ in range(REPS):
                for name, fn in variants.items():
                    times[name].append(wall(fn))
        pos = dict(train_rows=sep, test_rows_per_window=T, fits=WINDOWS * len(cands) * (n_splits + 1), variants={})
        for name, ts in times.items():
            med = statistics.median(ts)
            pos['variants'][name] = dict(median_ms=med * 1e3, min_ms=min(ts) * 1e3, max_ms=max(ts) * 1e3, spread=(max(ts) - min(ts)) / med)
        pos['logistic_ms_per_window'] = pos['variants']['logistic_batched']['median_ms'] / WINDOWS
        status = keep['kernel'][2].cpu().numpy()[:, :, :n_splits + 1]
        pos['exit_reasons'] = {name: int((status[..., 0] == code).sum()) for name, code in (('converged', hipops.LOGIT_CONVERGED), ('stalled', hipops.LOGIT_STALLED),
                                                                                            ('capped', hipops.LOGIT_CAPPED), ('one_class', hipops.LOGIT_ONE_CLASS))}
        pos['max_iterations'] = int(status[..., 1].max())
        pos['mean_auc'] = float(np.nanmean(keep['batched'][0]))
        if LogisticRegression is not None and a.sklearn_windows > 0:
            grid = dict(tabular.param_grid['logistic'], penalty=['l1', 'l2', None])
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                for wi in range(a.sklearn_windows):
                    clf = GridSearchCV(LogisticRegression(), grid, cv=n_splits)
                    clf.fit(x_w[:sep, wi].cpu().numpy(), y_w[:sep, wi].long().cpu().numpy())
                    clf.predict_proba(x_w[sep:, wi].cpu().numpy())
            pos['sklearn_ms_per_window_timed_once'] = (time.perf_counter() - t0) * 1e3 / a.sklearn_windows
        res['positions'][str(sep)] = pos
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
