"""Records tests/golden/tabular_catboost.pt and profiles/catboost_cv_fault_sensitivity.json: the CatBoost arm of the tabular study (tabular.catboost_metric) as
the restatement tests/catboost_f64.py runs it on the CPU.  No GPU and no boosting library is involved: include/pfn_hip.h is the specification, the f64 run of
the restatement the reference, its own float32 run the measure of what f32 may differ by.

    structural   the fits of tests/catboost_cases.py STRUCTURAL x STRUCTURAL_CANDS x 2 slots whose f64 run alone keeps the best noisy score of every level
                 MIN_GAP of the scale clear of the second: their trees, final margins and gaps.  An f32 run must grow these trees.  At least half must qualify.
    certificate  over ALL those problems' fits, qualifying or not: the float32 run's trees followed in f64 -- the worst (best - chosen) / scale is what f32
                 rounding alone may cost a chosen border; the GPU test allows four times that.
    grid         the full grid search (27 fits x 2 slots x 70 trees read at 10, 40, 70: 81 entries) on two windows of tests/golden/tabular_diabetes.pt, with the
                 hold-out tabular._catboost_holdout deals, at the first seed at which the float32 run selects the f64 run's entry and the f64 log losses of the
                 best entry and the runner-up stand further apart than the bound on a log loss: margins, log losses, best entry, and per fit whether the float32 run grew the same trees and its gap.
    faults       each planted fault of catboost_cases.FAULTS run on the structural problems: the largest shift of a margin over the bound the GPU test asserts,
                 or of the certificate (the faulted trees followed by the sound f64 restatement) over its slack.

Usage: python tools/record_catboost_cv_fixtures.py [--max-seeds 12]"""
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
import catboost_cases as cases      # noqa: E402
import catboost_f64 as cf      # noqa: E402

from transformerscandobayesianinference_amd import tabular      # noqa: E402

FLOOR = 2. ** -23
FAULT_CHECKPOINTS = (1, 3)


def fit_args(x, y, tx, fold, cand, slot, rounds, c, problem_id=0):
    depth, lr, l2 = cand
    return (x, y, cf.learn_mask(fold, slot), tx if slot == 1 else None, depth, lr, l2, rounds, cases.FIT_SEED, cf.stream(problem_id, c, slot))


def outputs(r, fold, slot, tree=-1):
    """What the kernel writes of a fit at a checkpoint: the held-out rows' margins, or the test rows'."""
    return r['test_margin'][tree] if slot == 1 else r['margin'][tree][np.asarray(fold) == 0]


fit_scale, certificate = cf.fit_scale, cf.certificate


def structural_problem(k):
    n, F, T, seed, rounds = cases.STRUCTURAL[k]
    x, y, tx, ty = tabular_cases.problem(n, F, T, seed)
    return x, y, tx, ty, cases.holdout_fold(y), rounds


def structural():
    kept, slack, every = [], 0., 0
    for k in range(len(cases.STRUCTURAL)):
        x, y, tx, ty, fold, rounds = structural_problem(k)
        for c, cand in enumerate(cases.STRUCTURAL_CANDS):
            for s in (0, 1):
                args = fit_args(x, y, tx, fold, cand, s, rounds, c, problem_id=k)
                r64, r32 = cf.fit(*args), cf.fit(*args, dtype=np.float32)
                every += 1
                slack = max(slack, certificate(cf.follow((r32['feature'], r32['threshold']), *args)['levels']))
                if r64['gap'] >= cases.MIN_GAP:
                    same = np.array_equal(r64['feature'], r32['feature']) and np.array_equal(r64['threshold'], r32['threshold'])
                    kept.append(dict(problem=k, cand=c, slot=s, feature=torch.from_numpy(r64['feature']), threshold=torch.from_numpy(r64['threshold']),
                                     out=torch.from_numpy(outputs(r64, fold, s).copy()), gap=r64['gap'], f32_run_same=bool(same)))
    print(f'structural: {len(kept)} of {every} fits meet the gap condition; the float32 runs grow the same trees in {sum(f["f32_run_same"] for f in kept)} of them; '
          f'certificate: worst (best - chosen) / scale of the float32 runs {slack:.3e}')
    assert 2 * len(kept) >= every, 'fewer than half of the recorded fits meet the gap condition: choose other seeds'
    assert np.isfinite(slack)
    return kept, slack, every


def grid_window(X, y, window, problem_id, seed):
    x, yy, tx, ty = cases.diabetes_window(X, y, *window)
    cls = yy > 0.5
    fold = tabular._catboost_holdout(cls, seed, problem_id)      # (window w is problem w of the one launch the GPU test makes)
    entries, fits, where, checkpoints = cf.grid_entries()
    t0 = time.time()
    h64, t64, f64 = cf.grid_search(x, yy, tx, fold, fits, checkpoints, seed, problem_id=problem_id)
    h32, t32, f32 = cf.grid_search(x, yy, tx, fold, fits, checkpoints, seed, problem_id=problem_id, dtype=np.float32)
    same = np.array([[np.array_equal(f64[c, s]['feature'], f32[c, s]['feature']) and np.array_equal(f64[c, s]['threshold'], f32[c, s]['threshold']) for s in (0, 1)]
                     for c in range(len(fits))])
    gaps = np.array([[f64[c, s]['gap'] for s in (0, 1)] for c in range(len(fits))])
    scales = np.array([[fit_scale(f64[c, s]) for s in (0, 1)] for c in range(len(fits))])
    loss64, best64 = cf.select(h64, fold, cls, where)
    loss32, best32 = cf.select(h32, fold, cls, where)
    held = fold == 0
    err = np.zeros((len(fits), 2))      # the float32 runs' margin error at the checkpoints, relative to the fit's scale, where they grew the same trees
    for c in range(len(fits)):
        err[c, 0] = np.abs(h32[c][:, held] - h64[c][:, held]).max() / scales[c, 0]
        err[c, 1] = np.abs(t32[c] - t64[c]).max() / scales[c, 1]
    clear = same & (gaps >= cases.MIN_GAP)
    e_margin = float(err[clear].max()) if clear.any() else 0.
    runner_up = float(np.sort(loss64)[1] - loss64[best64])
    c_best, k_best = where[best64]
    # what the selection stands on: the f32 rule on the margins of the best entry's search fit, on its scale -- the log loss is 1-Lipschitz in a margin
    loss_bound = 4 * max(e_margin, FLOOR) * scales[c_best, 0]
    print(f'window {window} seed {seed}: float32 run grows the same trees in {int(same.sum())} of {same.size} fits, {int(clear.sum())} with the gap; best entry {best64} '
          f'(float32 run: {best32}), runner-up {runner_up:.3e} away, bound {loss_bound:.3e}; e_margin {e_margin:.3e}; {time.time() - t0:.0f} s', flush=True)
    if best32 != best64 or runner_up <= loss_bound:      # (the GPU test then has the chosen entry to assert, not only its loss)
        return None
    return dict(window=window, problem_id=problem_id, seed=seed, x=torch.from_numpy(x), y=torch.from_numpy(yy), test_x=torch.from_numpy(tx), test_y=torch.from_numpy(ty),
                fold=torch.from_numpy(fold), hold_margin=torch.from_numpy(h64), test_margin=torch.from_numpy(t64), loss=torch.from_numpy(loss64), best=best64,
                runner_up=runner_up, loss_bound=float(loss_bound), e_margin=e_margin, same=torch.from_numpy(same), gap=torch.from_numpy(gaps),
                scale=torch.from_numpy(scales))


def fault_ratios(slack):
    """Per fault: the largest shift of an output margin over the bound 4 max(e, 2^-23) x scale the GPU test asserts (e from the float32 follow of the sound
    fit), and the certificate of the faulted trees under the sound f64 restatement over its slack 4 max(certificate e, 2^-23); the larger of the two counts."""
    ratios = {f: dict(ratio=0., fit=None) for f in cases.FAULTS}
    rounds = FAULT_CHECKPOINTS[-1]
    for k in range(2):
        x, y, tx, ty, fold, _ = structural_problem(k)
        for c, cand in enumerate(cases.STRUCTURAL_CANDS):
            for s in (0, 1):
                args = fit_args(x, y, tx, fold, cand, s, rounds, c, problem_id=k)
                r64 = cf.fit(*args)
                r32 = cf.follow((r64['feature'], r64['threshold']), *args, dtype=np.float32)
                scale = fit_scale(r64)
                want = np.stack([outputs(r64, fold, s, t - 1) for t in FAULT_CHECKPOINTS])
                approx = np.stack([outputs(r32, fold, s, t - 1) for t in FAULT_CHECKPOINTS])
                bound = 4 * max(np.abs(approx - want).max() / scale, FLOOR) * scale
                for f in cases.FAULTS:
                    if f == 'checkpoint_off_by_one':
                        got, cert = np.stack([outputs(r64, fold, s, min(t, rounds - 1)) for t in FAULT_CHECKPOINTS]), 0.
                    else:
                        bad = cf.fit(*args, faults=(f,))
                        got = np.stack([outputs(bad, fold, s, t - 1) for t in FAULT_CHECKPOINTS])
                        try:
                            cert = certificate(cf.follow((bad['feature'], bad['threshold']), *args)['levels'])
                        except ValueError:
                            cert = np.inf
                    by_margin, by_cert = float(np.abs(got - want).max() / bound), float(cert / (4 * max(slack, FLOOR)))
                    ratio = max(by_margin, by_cert)
                    if ratio > ratios[f]['ratio']:
                        ratios[f] = dict(ratio=min(ratio, 1e300), fit=[k, c, s], by_margin=by_margin, by_certificate=min(by_cert, 1e300))
    return ratios


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--max-seeds', type=int, default=12)
    ap.add_argument('--faults-only', action='store_true', help='rewrite the fault record alone, from the certificate e of the fixture on disk')
    args = ap.parse_args()
    path = os.path.join(ROOT, 'tests', 'golden', 'tabular_catboost.pt')
    if args.faults_only:
        return write_faults(torch.load(path, weights_only=False)['certificate_e'])
    kept, slack, every = structural()
    d = torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_diabetes.pt'))
    for seed in range(args.max_seeds):      # one launch has one seed: the first at which both windows qualify
        grids = [grid_window(d['X'].numpy(), d['y'].numpy(), w, k, seed) for k, w in enumerate(cases.GRID_WINDOWS)]
        if all(g is not None for g in grids):
            break
    else:
        raise SystemExit(f'no seed below {args.max_seeds} at which both windows qualify')
    torch.save(dict(entries=cf.grid_entries()[0], fit_seed=cases.FIT_SEED, structural=kept, structural_fits=every, certificate_e=float(slack), grid=grids), path)
    print('wrote', path, os.path.getsize(path), 'bytes')
    write_faults(slack)


def write_faults(slack):
    ratios = fault_ratios(slack)
    for f, r in ratios.items():
        print(f'fault {f}: shift / bound = {r["ratio"]:.3g}')
    out = os.path.join(ROOT, 'profiles', 'catboost_cv_fault_sensitivity.json')
    json.dump(dict(what='per planted fault the largest shift of an output margin over the bound 4 max(e, 2^-23) x scale of tests/test_gpu_catboost.py, or of the '
                        'certificate over its slack, on the CPU (tests/catboost_f64.py, problems 0 and 1 of catboost_cases.STRUCTURAL, both slots, 3 trees read '
                        'at checkpoints 1 and 3).  `under` names the faults that stay below `required`: they are recorded, not asserted',
                   required=8, under=[f for f, r in ratios.items() if r['ratio'] < 8], faults=ratios), open(out, 'w'), indent=1)
    print('wrote', out)


if __name__ == '__main__':
    main()
