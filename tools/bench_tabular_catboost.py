"""Times the CatBoost arm of the tabular study (tabular.catboost_metric, csrc/catboost_cv.hip) at the study's shape: bptt 100, 20 windows x 60 features, eval
positions 10 / 20 / 40 / 80, the reference's grid of 81 entries = 27 distinct fits x (search fit + refit) x 70 trees read at 10 / 40 / 70.

catboost_batched   tabular.evaluate_position(catboost_metric): one TRAIN_ONLY window launch, the hold-out on the host, ONE pfn_catboost_cv call (the sort pre-pass
                   and the launch of all 20 x 27 x 2 fits), the 81 log losses and the selection on the host
kernel             hipops.catboost_cv alone on the same operands: ms per launch, and over the 70 trees the us per tree of all fits
host_f64           the f64 restatement tests/catboost_f64.py: the same grid search of ONE window looped on one host core, timed ONCE (for scale: it is the test
                   oracle, not a tuned implementation, and no boosting library is installed to race); "not measured" where it was skipped (--no-host)

Protocol: wall-clock time of whole calls, the device synchronised at both ends; every variant is warmed up, the variants alternate for REPS rounds; the figure is
the median round, the spread (max - min) / median.  No ratio is claimed: there is no parent implementation.  Needs a GPU.
--bounds-out <path> then runs tests/test_gpu_catboost.py in a child process with PFN_RECORD_BOUNDS=<path>: every measured maximum of the GPU test with its e
(profiles/r24_catboost_cv_bounds_measured.json is such a run)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

import numpy as np
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
    ap.add_argument('--bounds-out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_tabular_catboost: no GPU -- nothing is measured without one')
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(1)
    N = BPTT + 3 * WINDOWS
    X = (torch.randn(N, FEATURES, generator=g) * (0.5 + torch.rand(FEATURES, generator=g)) + torch.randn(FEATURES, generator=g)).to(dev)
    w = torch.randn(FEATURES, generator=g).to(dev)
    y = ((X - X.mean(0)) @ w + torch.randn(N, generator=g).to(dev) > 0).float()
    starts = tabular.select_windows(N, BPTT, WINDOWS).tolist()
    entries, fits, where, checkpoints = tabular._catboost_grid()
    rounds = checkpoints[-1]
    cand = [[d for _, d, _ in fits], [lr for lr, _, _ in fits], [l2 for _, _, l2 in fits]]
    res = dict(bptt=BPTT, windows=WINDOWS, features=FEATURES, entries=len(entries), distinct_fits=len(fits), checkpoints=checkpoints, trees=rounds, reps=REPS,
               device=torch.cuda.get_device_name(0), positions={})
    for sep in POSITIONS:
        x_w, y_w = hipops.tabular_windows(X, y, starts, BPTT, sep, mode=hipops.TAB_NORM_TRAIN_ONLY)
        cls = y_w[:sep].cpu().numpy() > 0.5
        folds = np.stack([tabular._catboost_holdout(cls[:, k], 0, k) for k in range(WINDOWS)])
        operands = (x_w[:sep].float().transpose(0, 1).contiguous(), y_w[:sep].float().t().contiguous(), x_w[sep:].float().transpose(0, 1).contiguous(),
                    torch.from_numpy(folds).to(dev))
        keep = {}

        def catboost_batched():
            keep['batched'] = tabular.evaluate_position(X, y, [], tabular.catboost_metric, BPTT, sep, max_samples=WINDOWS)

        def kernel():
            keep['kernel'] = hipops.catboost_cv(*operands, *cand, rounds, checkpoints=checkpoints)

        variants = dict(catboost_batched=catboost_batched, kernel=kernel)
        times = {name: [] for name in variants}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for rep in range(REPS + 1):      # round 0 warms every variant up
                for name, fn in variants.items():
                    t = wall(fn)
                    if rep:
                        times[name].append(t)
        nfits = WINDOWS * len(fits) * hipops.CATBOOST_CV_SLOTS
        pos = dict(train_rows=sep, test_rows_per_window=BPTT - sep, held_out_rows=int((folds[0] == 0).sum()), fits=nfits,
                   lds_bytes_per_fit=4 * (32 + 4 * sep + sep * (FEATURES | 1) + 3 * sep + 10 * 128) + ((FEATURES * sep + 3) & ~3), variants={})
        for name, ts in times.items():
            med = statistics.median(ts)
            pos['variants'][name] = dict(median_ms=med * 1e3, min_ms=min(ts) * 1e3, max_ms=max(ts) * 1e3, spread=(max(ts) - min(ts)) / med)
        pos['ms_per_evaluate_position'] = pos['variants']['catboost_batched']['median_ms']
        pos['ms_per_launch'] = pos['variants']['kernel']['median_ms']
        pos['us_per_tree_of_all_fits'] = pos['variants']['kernel']['median_ms'] * 1e3 / rounds
        pos['auc_mean'] = float(np.nanmean(keep['batched'][0]))
        pos['status_done'] = int((keep['kernel'].status == hipops.CATBOOST_CV_DONE).sum())
        pos['host_f64_one_window_s'] = 'not measured'
        if not a.no_host and sep == a.host_position:
            import catboost_f64 as cf
            x0, y0, t0 = (t[0].cpu().numpy() for t in operands[:3])
            start = time.perf_counter()
            cf.grid_search(x0, y0, t0, folds[0], fits, checkpoints, 0)
            pos['host_f64_one_window_s'] = time.perf_counter() - start      # timed once
        res['positions'][str(sep)] = pos
        print(f'eval position {sep}: evaluate_position {pos["ms_per_evaluate_position"]:.2f} ms, launch {pos["ms_per_launch"]:.2f} ms, '
              f'{pos["us_per_tree_of_all_fits"]:.1f} us per tree of all {nfits} fits, host f64 one window: {pos["host_f64_one_window_s"]}', flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
        print('wrote', a.out)
    if a.bounds_out:      # a fresh child process: the GPU test with the PFN_RECORD_BOUNDS convention of tests/bounds.py
        env = dict(os.environ, PFN_RECORD_BOUNDS=os.path.abspath(a.bounds_out))
        rc = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', os.path.join(ROOT, 'tests', 'test_gpu_catboost.py')], env=env, cwd=ROOT).returncode
        print('wrote' if rc == 0 else 'the GPU test failed; what it measured is in', a.bounds_out)
        sys.exit(rc)


if __name__ == '__main__':
    main()
