"""The tabular study's GP-classifier arm on the device, and scikit-learn's grid search on the same windows where scikit-learn is importable.

    python tools/bench_tabular_gp.py [--out profiles/r18_tabular_gp.json] [--sklearn-windows 2]

bptt 100, eval positions 10 / 20 / 40 / 80, 20 windows of a 60-feature table (the shapes of tools/bench_tabular.py):
gp_batched    tabular.evaluate_position(gp_metric): one TRAIN_ONLY window launch, the folds on the host, batched_lbfgs over all 20 x 24 x (folds + 1) fits with
              ONE pfn_gpc_lml_grad launch per pass, ONE pfn_gpc_predict launch, the scores and the erf mixture on the host, one pfn_auc_counts launch; reported
              per call and per window, with the L-BFGS pass count, the fits it reports converged and the kernels' exit reasons
lml_launch    one pfn_gpc_lml_grad launch at the starting thetas on the same windows (hipops.gpc_lml_grad, inputs resident), device-synchronised; launch share =
              passes x this / the whole call (the rest is the optimiser's torch arithmetic, the prediction launch and the host half)
gp_sklearn    per window: GridSearchCV(GaussianProcessClassifier(), the reference's 24 kernels, cv = 5) + predict_proba on the host, as the reference runs it.  It
              takes seconds per window, so it is timed ONCE on the first --sklearn-windows windows of each position; without scikit-learn the device time stands
              alone and the result says so.
There is no earlier implementation of this arm in this package: no ratio against a parent is claimed.  The scikit-learn figure is another optimiser (L-BFGS-B in
f64) on another processor; it is context, not a like-for-like comparison.

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

REPS = 5
BPTT, WINDOWS, FEATURES = 100, 20, 60
POSITIONS = (10, 20, 40, 80)
REASONS = (('converged', hipops.GPC_CONVERGED), ('capped', hipops.GPC_CAPPED), ('one_class', hipops.GPC_ONE_CLASS), ('nonpositive', hipops.GPC_NONPOSITIVE),
           ('nonfinite', hipops.GPC_NONFINITE))


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
        sys.exit('bench_tabular_gp: no GPU -- nothing is measured without one')
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(1)
    N = BPTT + 3 * WINDOWS
    X = (torch.randn(N, FEATURES, generator=g) * (0.5 + torch.rand(FEATURES, generator=g)) + torch.randn(FEATURES, generator=g)).to(dev)
    w = torch.randn(FEATURES, generator=g).to(dev)
    y = ((X - X.mean(0)) @ w + torch.randn(N, generator=g).to(dev) > 0).float()
    starts = tabular.select_windows(N, BPTT, WINDOWS).tolist()
    try:
        from sklearn.gaussian_process import GaussianProcessClassifier
        from sklearn.gaussian_process.kernels import RBF
        from sklearn.model_selection import GridSearchCV
    except ImportError:
        GaussianProcessClassifier = None
    cands = tabular._gp_grid()
    res = dict(bptt=BPTT, windows=WINDOWS, features=FEATURES, candidates=len(cands), lbfgs=tabular.GP_LBFGS, reps=REPS, device=torch.cuda.get_device_name(0),
               sklearn='timed once on the first %d windows of each position' % a.sklearn_windows if GaussianProcessClassifier is not None
               else 'scikit-learn is not importable here: device time alone', positions={})
    for sep in POSITIONS:
        keep, counters = {}, {}
        x_w, y_w = hipops.tabular_windows(X, y, starts, BPTT, sep, mode=hipops.TAB_NORM_TRAIN_ONLY)
        n_splits, _, _, (train, labels, _, folds) = tabular._fold_problems(x_w[:sep], y_w[:sep], x_w[sep:])
        theta = torch.tensor(cands, dtype=torch.float64).log().float().to(dev)[None, :, None, :].expand(WINDOWS, len(cands), hipops.GPC_SLOTS, 2).contiguous()
        k_args = (theta, train, labels, folds, n_splits)

        def gp_batched():
            keep['batched'] = tabular.evaluate_position(X, y, [], tabular.gp_metric, BPTT, sep, max_samples=WINDOWS)

        def lml_launch():
            keep['kernel'] = hipops.gpc_lml_grad(*k_args)

        variants = dict(gp_batched=gp_batched, lml_launch=lml_launch)
        times = {name: [] for name in variants}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for fn in variants.values():
                fn()
            for _ in range(REPS):
                for name, fn in variants.items():
                    times[name].append(wall(fn))
            # the same call once more with its counters (not timed)
            tabular._gp_batched(x_w[:sep], y_w[:sep], x_w[sep:], y_w[sep:], counters=counters)
        pos = dict(train_rows=sep, test_rows_per_window=BPTT - sep, fits=WINDOWS * len(cands) * (n_splits + 1), variants={})
        for name, ts in times.items():
            med = statistics.median(ts)
            pos['variants'][name] = dict(median_ms=med * 1e3, min_ms=min(ts) * 1e3, max_ms=max(ts) * 1e3, spread=(max(ts) - min(ts)) / med)
        pos['gp_ms_per_window'] = pos['variants']['gp_batched']['median_ms'] / WINDOWS
        pos['lbfgs_passes'] = counters['passes']
        pos['lbfgs_converged'] = int(counters['converged'].sum())
        pos['launch_share'] = counters['passes'] * pos['variants']['lml_launch']['median_ms'] / pos['variants']['gp_batched']['median_ms']
        status = counters['status'][:, :, :n_splits + 1]
        pos['exit_reasons'] = {name: int((status[..., 0] == code).sum()) for name, code in REASONS}
        pos['max_newton_iterations'] = int(status[..., 1].max())
        pos['mean_auc'] = float(np.nanmean(keep['batched'][0]))
        if GaussianProcessClassifier is not None and a.sklearn_windows > 0:
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                for wi in range(a.sklearn_windows):
                    clf = GridSearchCV(GaussianProcessClassifier(), {'kernel': [c * RBF(l) for c, l in cands]}, cv=n_splits)
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
