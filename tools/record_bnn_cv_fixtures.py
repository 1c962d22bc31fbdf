"""Records tests/golden/tabular_bnn.pt: the BNN-classifier grid search of tabular.bayes_net_metric on four seeded problems, run by the restatement
tests/bnn_cv_f64.py on the CPU -- no GPU and no kernel takes part.  Per problem (tabular_cases.problem at bnn_cv_f64.SHAPES, the full 8-candidate grid, 400 steps,
400 draws, the starts of tabular._bayes_loc0 at seed 0, problem 0) it stores the seed, the folds, the f64 cv_prob [8, n] and test_prob [8, T], the f64 scores and
the best entry, and e: the largest difference between the float32 run of the same restatement and the f64 one over those probabilities.  States are not stored.

A seed is kept when, on the f64 results alone, at most 2 % of the held-out rows have a probability within 4 max(e, 2^-23) of 0.5 (a GPU run may put such a row
in the other class); the first seed from 0 that also leaves none is taken while fewer than three problems have none.

    python tools/record_bnn_cv_fixtures.py            (about two minutes on four cores)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import bnn_cv_f64 as cvf      # noqa: E402
import tabular_cases      # noqa: E402

from transformerscandobayesianinference_amd import tabular      # noqa: E402

FIT_SEED = 0


def record_problem(n, F, T, seed, cands, num_steps, num_draws):
    x, y, tx, ty = tabular_cases.problem(n, F, T, seed)
    n_splits = min(tabular.CV, n // 2)
    folds = tabular._stratified_folds(y > 0.5, n_splits)
    loc0_of = lambda c, D: tabular._bayes_loc0(FIT_SEED, 0, c, D)
    out = {}
    for dtype in (torch.float64, torch.float32):
        out[dtype] = cvf.pipeline(x, y, tx, folds, n_splits, cands, loc0_of, num_steps, num_draws, seed=FIT_SEED, problem_id=0, dtype=dtype)
    cv64, te64 = (v.numpy() for v in out[torch.float64])
    cv32, te32 = (v.double().numpy() for v in out[torch.float32])
    e = float(max(np.abs(cv32 - cv64).max(), np.abs(te32 - te64).max()))
    mean, best, _ = tabular._bayes_select(cv64, folds, y > 0.5, n_splits, te64)
    near = np.abs(cv64 - 0.5) <= 4 * max(e, 2. ** -23)
    return dict(seed=seed, n_splits=n_splits, folds=torch.from_numpy(folds), cv_prob=torch.from_numpy(cv64), test_prob=torch.from_numpy(te64),
                mean_test_score=torch.from_numpy(mean), best=best, e=e, near_half=int(near.sum()), near_share=float(near.mean()),
                checksum=float(np.float64(x).sum() + np.float64(tx).sum() + y.sum()))


def main():
    entries, cands, num_steps, num_draws = tabular._bayes_grid()
    problems, clean = [], 0
    for k, (n, F, T) in enumerate(cvf.SHAPES):
        for seed in range(0, 16):
            t0 = time.time()
            rec = record_problem(n, F, T, seed, cands, num_steps, num_draws)
            print(f'(n {n}, F {F}, T {T}) seed {seed}: e {rec["e"]:.3e}, {rec["near_half"]} rows near 0.5, best {rec["best"]} {entries[rec["best"]]}, scores '
                  f'{np.round(rec["mean_test_score"].numpy(), 3).tolist()}, {time.time() - t0:.0f} s', flush=True)
            must_be_clean = clean + (len(cvf.SHAPES) - 1 - k) < 3      # the remaining problems could not make it three
            if rec['near_share'] <= 0.02 and (rec['near_half'] == 0 or not must_be_clean):
                break
        else:
            raise SystemExit('no seed in 0 .. 15 meets the condition')
        clean += int(rec['near_half'] == 0)
        del rec['near_share']
        problems.append(rec)
    path = os.path.join(ROOT, 'tests', 'golden', 'tabular_bnn.pt')
    torch.save(dict(cands=cands, num_steps=num_steps, num_draws=num_draws, fit_seed=FIT_SEED, problems=problems), path)
    print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
