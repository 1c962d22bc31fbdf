"""Records tests/golden/tabular_xgb.pt and profiles/xgb_cv_fault_sensitivity.json: the gradient-boosting arm of the tabular study (tabular.xgb_metric) as the
restatement tests/xgb_f64.py runs it on the CPU.  No GPU and no boosting library is involved: include/pfn_hip.h is the specification, the f64 run of the
restatement the reference, its own float32 run the measure of what f32 may differ by.

    structural   the fits of tests/xgb_cases.py STRUCTURAL x STRUCTURAL_CANDS x 6 slots whose f64 run alone shows a relative gain gap >= 1e-4 at every node
                 and keeps every near-best candidate's HL / HR 2^-16 away from min_child_weight: their trees, margins and gaps.  An f32 run must grow these trees.
    certificate  over ALL those problems' fits, qualifying or not: the float32 run's trees followed in f64 -- the worst (best - chosen) / (|left| + |right| +
                 |root|) is what f32 rounding alone may cost a chosen split; the GPU test allows four times that.
    grid         the full grid search (16 entries x 6 slots x 100 rounds) on two windows of tests/golden/tabular_diabetes.pt, at the first fit seed for which the
                 float32 run grows the f64 run's trees in every fit: held-out margins, scores, best entry, the margins' and probabilities' e.
    faults       each planted fault of xgb_cases.FAULTS run on the structural problems: the largest margin shift over the bound the GPU test uses.

Usage: python tools/record_xgb_cv_fixtures.py [--max-seeds 12]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tabular_cases      # noqa: E402
import xgb_cases as cases      # noqa: E402
import xgb_f64 as xf      # noqa: E402

from transformerscandobayesianinference_amd import tabular      # noqa: E402

FLOOR = 2. ** -23


def fit_args(x, y, tx, folds, cand, slot, rounds, c, problem_id=0):
    depth, eta, mcw, sub, col = cand
    return (x, y, xf.row_mask(folds, slot, cases.N_SPLITS), tx if slot == cases.N_SPLITS else None, depth, eta, mcw, sub, col, rounds, cases.FIT_SEED,
            xf.stream(problem_id, c, slot))


def outputs(r, folds, slot):
    """What the kernel writes of a fit: the held-out rows' margins, or the test rows'."""
    return r['test_margin'] if slot == cases.N_SPLITS else r['margin'][np.asarray(folds) == slot]


def structural():
    kept, slack, every = [], 0., 0
    for k, (n, F, T, seed, rounds) in enumerate(cases.STRUCTURAL):
        x, y, tx, ty = tabular_cases.problem(n, F, T, seed)
        folds = tabular._stratified_folds(y > 0.5, cases.N_SPLITS)
        for c, cand in enumerate(cases.STRUCTURAL_CANDS):
            for s in range(cases.N_SPLITS + 1):
                args = fit_args(x, y, tx, folds, cand, s, rounds, c, problem_id=k)
                r64, r32 = xf.fit(*args), xf.fit(*args, dtype=np.float32)
                every += 1
                for node in xf.follow((r32['feature'], r32['threshold']), *args)['nodes']:
                    assert node['legal']
                    if node['given'] >= 0:
                        slack = max(slack, (node['best'] - node['gain']) / node['scale'])
                    elif node['best'] is not None and node['best'] > xf.MIN_GAIN:
                        slack = max(slack, (node['best'] - xf.MIN_GAIN) / node['scale'])
                if r64['gap'] >= cases.MIN_GAP and r64['mcw_distance'] >= cases.MIN_MCW_DISTANCE:
                    same = np.array_equal(r64['feature'], r32['feature']) and np.array_equal(r64['threshold'], r32['threshold'])
                    kept.append(dict(problem=k, cand=c, slot=s, feature=torch.from_numpy(r64['feature']), threshold=torch.from_numpy(r64['threshold']),
                                     leaf=torch.from_numpy(r64['leaf']), out=torch.from_numpy(outputs(r64, folds, s).copy()), gap=r64['gap'],
                                     mcw_distance=r64['mcw_distance'], f32_run_same=bool(same)))
    print(f'structural: {len(kept)} of {every} fits meet the gap condition; the float32 runs grow the same trees in {sum(f["f32_run_same"] for f in kept)} of them; '
          f'certificate: worst (best - chosen) / scale of the float32 runs {slack:.3e}')
    return kept, slack, every


def grid_window(X, y, window, problem_id, seeds):
    x, yy, tx, ty = cases.diabetes_window(X, y, *window)
    folds = tabular._stratified_folds(yy > 0.5, cases.N_SPLITS)
    entries = xf.grid_entries()
    for seed in seeds:
        t0 = time.time()
        cv64, te64, fits64 = xf.grid_search(x, yy, tx, folds, cases.N_SPLITS, entries, seed, problem_id=problem_id)
        cv32, te32, fits32 = xf.grid_search(x, yy, tx, folds, cases.N_SPLITS, entries, seed, problem_id=problem_id, dtype=np.float32)
        same = all(np.array_equal(fits64[k]['feature'], fits32[k]['feature']) and np.array_equal(fits64[k]['threshold'], fits32[k]['threshold']) for k in fits64)
        gap = min(f['gap'] for f in fits64.values())
        print(f'window {window} seed {seed}: float32 run grows the same trees: {same}; smallest gap {gap:.2e}; {time.time() - t0:.0f} s', flush=True)
        if not same:
            continue
        # (window w is problem w of the one launch the GPU test makes: its id in the noise addressing)
        held = ~np.isnan(cv64)
        scale = max(np.abs(cv64[held]).max(), np.abs(te64).max())
        e_margin = max(np.abs(cv32 - cv64)[held].max(), np.abs(te32 - te64).max()) / scale
        proba = lambda m: 1. / (1. + np.exp(-m))
        e_proba = np.abs(proba(te32) - proba(te64)).max()
        mean, best = xf.select(cv64, folds, yy > 0.5, cases.N_SPLITS)
        return dict(window=window, problem_id=problem_id, seed=seed, x=torch.from_numpy(x), y=torch.from_numpy(yy), test_x=torch.from_numpy(tx), test_y=torch.from_numpy(ty),
                    folds=torch.from_numpy(folds), cv_margin=torch.from_numpy(cv64), test_margin=torch.from_numpy(te64), mean_test_score=torch.from_numpy(mean),
                    best=best, margin_scale=float(scale), e_margin=float(e_margin), e_proba=float(e_proba), smallest_gap=float(gap),
                    near_zero=int((np.abs(cv64[held]) <= 4 * max(e_margin, FLOOR) * scale).sum()))
    return None


def fault_ratios():
    """Per fault: the largest shift of an output margin over the bound 4 max(e, 2^-23) x scale the GPU test allows, e from the float32 run of the unfaulted fit."""
    ratios = {f: dict(ratio=0., fit=None) for f in cases.FAULTS}
    for k, (n, F, T, seed, rounds) in enumerate(cases.STRUCTURAL[:2]):
        x, y, tx, ty = tabular_cases.problem(n, F, T, seed)
        folds = tabular._stratified_folds(y > 0.5, cases.N_SPLITS)
        for c, cand in enumerate(cases.STRUCTURAL_CANDS):
            for s in (0, cases.N_SPLITS):
                args = fit_args(x, y, tx, folds, cand, s, rounds, c, problem_id=k)
                r64 = xf.fit(*args)
                r32 = xf.follow((r64['feature'], r64['threshold']), *args, dtype=np.float32)
                want = outputs(r64, folds, s)
                scale = np.abs(want).max()
                bound = 4 * max(np.abs(outputs(r32, folds, s) - want).max() / scale, FLOOR) * scale
                for f in cases.FAULTS:
                    shift = np.abs(outputs(xf.fit(*args, faults=(f,)), folds, s) - want).max()
                    if shift / bound > ratios[f]['ratio']:
                        ratios[f] = dict(ratio=float(shift / bound), fit=[k, c, s], shift=float(shift), bound=float(bound))
    return ratios


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--max-seeds', type=int, default=12)
    args = ap.parse_args()
    kept, slack, every = structural()
    d = torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_diabetes.pt'))
    for seed in range(args.max_seeds):      # one launch has one seed: the first at which both windows' float32 runs follow their f64 runs
        grids = [grid_window(d['X'].numpy(), d['y'].numpy(), w, k, [seed]) for k, w in enumerate(cases.GRID_WINDOWS)]
        if all(g is not None for g in grids):
            break
    else:
        raise SystemExit(f'no seed below {args.max_seeds} at which the float32 runs follow the f64 ones on both windows')
    ratios = fault_ratios()
    for f, r in ratios.items():
        print(f'fault {f}: shift / bound = {r["ratio"]:.3g}')
    path = os.path.join(ROOT, 'tests', 'golden', 'tabular_xgb.pt')
    torch.save(dict(entries=xf.grid_entries(), fit_seed=cases.FIT_SEED, structural=kept, structural_fits=every, certificate_e=float(slack), grid=grids), path)
    print('wrote', path, os.path.getsize(path), 'bytes')
    out = os.path.join(ROOT, 'profiles', 'xgb_cv_fault_sensitivity.json')
    json.dump(dict(what='largest shift of an output margin under each planted fault over the bound 4 max(e, 2^-23) x scale of tests/test_gpu_xgb.py, on the CPU '
                        '(tests/xgb_f64.py, problems 0 and 1 of xgb_cases.STRUCTURAL, slots 0 and 5)', faults=ratios), open(out, 'w'), indent=1)
    print('wrote', out)


if __name__ == '__main__':
    main()
