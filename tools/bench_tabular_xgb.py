"""Times the gradient-boosting arm of the tabular study (tabular.xgb_metric, csrc/xgb_cv.hip) at the study's shape: bptt 100, 20 windows x 60 features, eval
positions 10 / 20 / 40 / 80, the reference's grid of 16 entries x (5 folds + refit) x 100 rounds.

xgb_batched   tabular.evaluate_position(xgb_metric): one TRAIN_ONLY window launch, the folds on the host, ONE pfn_xgb_cv call (the sort pre-pass and the launch
              of all 20 x 16 x 6 fits), scores and selection on the host
kernel        hipops.xgb_cv alone on the same operands: ms per launch, and over the 100 rounds the us per round of all fits
host_f64      the f64 restatement tests/xgb_f64.py: the same grid search of ONE window looped on one host core, timed ONCE (for scale: it is the test oracle, not
              a tuned implementation, and no boosting library is installed to race); "not measured" where it was skipped (--no-host)

Protocol: wall-clock time of whole calls, the device synchronised at both ends; every variant is warmed up, the variants alternate for REPS rounds; the figure is
the median round, the spread (max - min) / median.  No ratio is claimed: there is no parent implementation.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from transformerscandobayesianinference_amd import hipops, tabular  # noqa: E402

REPS = 5
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
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--host-position', type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_tabular_xgb: no GPU -- nothing is measured without one')
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(1)
    N = BPTT + 3 * WINDOWS
    X = (torch.randn(N, FEATURES, generator=g) * (0.5 + torch.rand(FEATURES, generator=g)) + torch.randn(FEATURES, generator=g)).to(dev)
    w = torch.randn(FEATURES, generator=g).to(dev)
    y = ((X - X.mean(0)) @ w + torch.randn(N, generator=g).to(dev) > 0).float()
    starts = tabular.select_windows(N, BPTT, WINDOWS).tolist()
    entries, rounds = tabular._xgb_grid()
    cand = [[e[k] for e in entries] for k in ('max_depth', 'learning_rate', 'min_child_weight', 'subsample', 'colsample_bytree')]
    res = dict(bptt=BPTT, windows=WINDOWS, features=FEATURES, entries=len(entries), rounds=rounds, reps=REPS, device=torch.cuda.get_device_name(0), positions={})
    for sep in POSITIONS:
        x_w, y_w = hipops.tabular_windows(X, y, starts, BPTT, sep, mode=hipops.TAB_NORM_TRAIN_ONLY)
        n_splits, folds, _, operands = tabular._fold_problems(x_w[:sep], y_w[:sep], x_w[sep:], n_splits=tabular.XGB_FOLDS)
        keep = {}

        def xgb_batched():
            keep['batched'] = tabular.evaluate_position(X, y, [], tabular.xgb_metric, BPTT, sep, max_samples=WINDOWS)

        def kernel():
            keep['kernel'] = hipops.xgb_cv(*operands, n_splits, *cand, rounds)

        variants = dict(xgb_batched=xgb_batched, kernel=kernel)
        times = {name: [] for name in variants}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for rep in range(REPS + 1):      # round 0 warms every variant up
                for name, fn in variants.items():
                    t = wall(fn)
                    if rep:
                        times[name].append(t)
        fits = WINDOWS * len(entries) * (n_splits + 1)
        pos = dict(train_rows=sep, test_rows_per_window=BPTT - sep, n_splits=n_splits, fits=fits, lds_bytes_per_fit=4 * (32 + sep * (FEATURES | 1) + 3 * sep + 2 * FEATURES)
                   + ((FEATURES * sep + 3) & ~3), variants={})
        for name, ts in times.items():
            med = statistics.median(ts)
            pos['variants'][name] = dict(median_ms=med * 1e3, min_ms=min(ts) * 1e3, max_ms=max(ts) * 1e3, spread=(max(ts) - min(ts)) / med)
        pos['ms_per_evaluate_position'] = pos['variants']['xgb_batched']['median_ms']
        pos['ms_per_launch'] = pos['variants']['kernel']['median_ms']
        pos['us_per_round_of_all_fits'] = pos['variants']['kernel']['median_ms'] * 1e3 / rounds
        pos['accuracy_mean'] = float(keep['batched'][0].mean())
        pos['status_done'] = int((keep['kernel'].status == hipops.XGB_CV_DONE).sum())
        pos['host_f64_one_window_s'] = 'not measured'
        if not a.no_host and sep == a.host_position:
            import xgb_f64 as xf
            x0, y0, t0 = (t[0].cpu().numpy() for t in operands[:3])
            start = time.perf_counter()
            xf.grid_search(x0, y0, t0, folds[0], n_splits, entries, 0)
            pos['host_f64_one_window_s'] = time.perf_counter() - start      # timed once
        res['positions'][str(sep)] = pos
        print(f'eval position {sep}: evaluate_position {pos["ms_per_evaluate_position"]:.2f} ms, launch {pos["ms_per_launch"]:.2f} ms, '
              f'{pos["us_per_round_of_all_fits"]:.1f} us per round of all {fits} fits, host f64 one window: {pos["host_f64_one_window_s"]}', flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
        print('wrote', a.out)


if __name__ == '__main__':
    main()
