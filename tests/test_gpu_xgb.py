"""pfn_xgb_cv on the MI355X against the restatement tests/xgb_f64.py (written from the contract in include/pfn_hip.h).  Everywhere, through `follow`: the device's
trees taken as given, every chosen split is legal and its f64 gain is within the certificate slack of the node's best, every leaf value and final margin within
the project's f32 rule 4 max(e, 2^-23) of its scale, e the error of the restatement's own float32 run of the same structure against the f64 one.  On the recorded
fits that meet the gap condition (tests/golden/tabular_xgb.pt) the trees equal the independent f64 fit's, thresholds bit for bit.  Then the planted columns, the
full grid against the recorded f64 grid searches, the bitwise invariants of the contract, and the study's arm end to end.
PFN_RECORD_BOUNDS=<path> writes every measured maximum with its e (profiles/r23_xgb_cv_bounds_measured.json is such a run)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds      # noqa: E402
import tabular_cases      # noqa: E402
import xgb_cases as cases      # noqa: E402
import xgb_f64 as xf      # noqa: E402

from transformerscandobayesianinference_amd import hipops, tabular      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
FLOOR = 2. ** -23


@functools.lru_cache(maxsize=None)
def recorded():
    return torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_xgb.pt'), weights_only=False)


def floor_rule(e):
    return 4 * max(e, FLOOR)


def certificate_slack():
    """Four times what f32 rounding alone cost the restatement's float32 runs (recorded: the worst (best - chosen) / (|left| + |right| + |root|) against f64), and no
    less than four f32 roundings of that scale: a gain is three quotients and two sums of f32."""
    return 4 * max(recorded()['certificate_e'], FLOOR)


def launch(problems, cands, rounds, seed=cases.FIT_SEED, ids=None, cand_ids=None, want_trees=True):
    """hipops.xgb_cv on problems [(x, y, tx, ty, folds)] with candidates [(depth, lr, mcw, subsample, colsample)]: XgbCvOut on the host."""
    dev = lambda k, dtype=None: torch.from_numpy(np.stack([p[k] for p in problems])).to(DEV)
    ids = None if ids is None else torch.tensor(list(ids), dtype=torch.int64, device=DEV)
    out = hipops.xgb_cv(dev(0), dev(1), dev(2), dev(4), cases.N_SPLITS, *([c[k] for c in cands] for k in range(5)), rounds, seed=seed, problem_ids=ids, want_trees=want_trees,
                        cand_ids=cand_ids)
    return hipops.XgbCvOut(*(None if t is None else t.cpu() for t in out))


def fit_args(prob, cand, slot, rounds, q, seed=cases.FIT_SEED):
    x, y, tx, ty, folds = prob
    return (x, y, xf.row_mask(folds, slot, cases.N_SPLITS), tx if slot == cases.N_SPLITS else None, *cand, rounds, seed, q)


def device_outputs(out, p, c, s, folds):
    return (out.test_margin[p, c] if s == cases.N_SPLITS else out.cv_margin[p, c][torch.from_numpy(np.asarray(folds) == s)]).double().numpy()


def host_outputs(r, s, folds):
    return r['test_margin'] if s == cases.N_SPLITS else r['margin'][np.asarray(folds) == s]


def fit_scale(r):
    """The scale of a fit's margins: the sum over the rounds of the round's largest leaf value.  A margin is a sum of leaf values of either sign and its error a sum
    of theirs, so a margin that cancels to almost nothing (one sampled row per round, a single test row) measures nothing by its own size."""
    return max(np.abs(r['leaf']).max(1).sum(), 1e-30)


def check_through_follow(label, out, p, c, s, prob, cand, rounds, q, worst):
    """The device's fit (p, c, s) followed in f64 and in f32; asserts legality and the certificate, adds the measured leaf and margin errors to `worst`."""
    trees = (out.tree_feature[p, c, s].numpy(), out.tree_threshold[p, c, s].numpy())
    args = fit_args(prob, cand, s, rounds, q)
    f64, f32 = xf.follow(trees, *args), xf.follow(trees, *args, dtype=np.float32)
    assert int(out.status[p, c, s]) == hipops.XGB_CV_DONE
    slack = certificate_slack()
    for node in f64['nodes']:
        # legal under THESE statistics, up to what f32 may move a side's H by: hi of a row is p (1 - p) 2^23 rounded, p an f32 sigmoid, so the two runs' sums differ
        # by a few units per row -- 4 x 2^-23 of the node's H, the f32 rule on the sum that is compared
        assert node['legal'] or node.get('short', np.inf) <= 4 * FLOOR * node['Ht'], (label, p, c, s, node)
        if node['given'] >= 0:
            assert node['gain'] > xf.MIN_GAIN - slack * node['scale'], (label, p, c, s, node)
            worst['certificate'] = max(worst['certificate'], (node['best'] - node['gain']) / node['scale'])
        elif node['best'] is not None and node['best'] > xf.MIN_GAIN:      # the device made a leaf of a node the f64 statistics would split
            worst['certificate'] = max(worst['certificate'], (node['best'] - xf.MIN_GAIN) / node['scale'])
    for name, got, want, approx in (('leaf', out.tree_leaf[p, c, s].double().numpy(), f64['leaf'], f32['leaf']),
                                    ('margin', device_outputs(out, p, c, s, prob[4]), host_outputs(f64, s, prob[4]), host_outputs(f32, s, prob[4]))):
        scale = np.abs(f64['leaf']).max() if name == 'leaf' else fit_scale(f64)
        worst[name] = max(worst[name], np.abs(got - want).max() / scale)
        worst['e_' + name] = max(worst['e_' + name], np.abs(approx.astype(np.float64) - want).max() / scale)
    return f64


def assert_worst(label, worst):
    print(f'{label}: certificate {worst["certificate"]:.3e} (slack {certificate_slack():.3e}), leaf {worst["leaf"]:.3e} (e {worst["e_leaf"]:.3e}), '
          f'margin {worst["margin"]:.3e} (e {worst["e_margin"]:.3e})')
    bounds.within(f'{label} certificate', worst['certificate'], certificate_slack())
    for name in ('leaf', 'margin'):
        bounds.within(f'{label} {name} (e {worst["e_" + name]:.3e})', worst[name], floor_rule(worst['e_' + name]))


def new_worst():
    return dict(certificate=0., leaf=0., margin=0., e_leaf=0., e_margin=0.)


@pytest.mark.parametrize('label', list(cases.CASES))
def test_shapes_through_follow(label):
    n, F, T, cands, rounds, slots = cases.CASES[label]
    probs = [cases.case_problem(label, p) for p in range(2)]
    ids = (5, 0)
    out = launch(probs, cands, rounds, ids=ids)
    assert bool((out.status == hipops.XGB_CV_DONE).all()) and bool(torch.isfinite(out.test_margin).all()) and bool(torch.isfinite(out.cv_margin).all())
    worst, structural, seen_duplicate = new_worst(), 0, 0
    for p, prob in enumerate(probs):
        for c, cand in enumerate(cands):
            for s in slots:
                q = xf.stream(ids[p], c, s)
                check_through_follow(label, out, p, c, s, prob, cand, rounds, q, worst)
                feature = out.tree_feature[p, c, s].numpy()
                if F >= 5:      # the planted columns: the constant column is never split, the duplicate wins only in a round whose column sample lacks its original
                    assert not (feature == cases.CONSTANT).any(), (label, p, c, s)
                    for t in np.flatnonzero((feature == cases.DUPLICATE[1]).any(1)):
                        assert cases.DUPLICATE[0] not in xf.sampled_features(cases.FIT_SEED, q, int(t), F, cand[4]), (label, p, c, s, t)
                    seen_duplicate += int((feature == cases.DUPLICATE[0]).sum())
                if p == 0 and s == slots[0]:      # where the f64 fit alone shows the gap, the independent fit grows the same trees, thresholds bit for bit
                    r = xf.fit(*fit_args(prob, cand, s, rounds, q))
                    if r['gap'] >= cases.MIN_GAP and r['mcw_distance'] >= cases.MIN_MCW_DISTANCE:
                        structural += 1
                        assert np.array_equal(feature, r['feature']) and out.tree_threshold[p, c, s].numpy().tobytes() == r['threshold'].tobytes(), (label, p, c, s)
    if F >= 5:      # a column of the three values -1, 0, 1: wherever it is chosen, the threshold is a midpoint of two of them
        thr = out.tree_threshold[out.tree_feature == cases.THREE_VALUED]
        assert bool(torch.isin(thr, torch.tensor([-0.5, 0., 0.5])).all())
        assert seen_duplicate > 0 or label != 'n10_F5_T128'      # and there its original is chosen: the tie was there to decide
    print(f'{label}: {structural} fits compared structurally')
    assert_worst(label, worst)


def test_recorded_fits_that_meet_the_gap_condition_grow_the_recorded_trees():
    rec = recorded()
    worst, count = new_worst(), 0
    for k, (n, F, T, seed, rounds) in enumerate(cases.STRUCTURAL):
        x, y, tx, ty = tabular_cases.problem(n, F, T, seed)
        prob = (x, y, tx, ty, tabular._stratified_folds(y > 0.5, cases.N_SPLITS))
        out = launch([prob], cases.STRUCTURAL_CANDS, rounds, ids=(k,))
        for f in (f for f in rec['structural'] if f['problem'] == k):
            c, s = f['cand'], f['slot']
            assert np.array_equal(out.tree_feature[0, c, s].numpy(), f['feature'].numpy()), (k, c, s)
            assert out.tree_threshold[0, c, s].numpy().tobytes() == f['threshold'].numpy().tobytes(), (k, c, s)
            f64 = check_through_follow('recorded', out, 0, c, s, prob, cases.STRUCTURAL_CANDS[c], rounds, xf.stream(k, c, s), worst)
            want = f['out'].numpy()
            assert np.array_equal(host_outputs(f64, s, prob[4]), want)      # the same trees: following them is the recorded fit
            assert np.abs(device_outputs(out, 0, c, s, prob[4]) - want).max() <= floor_rule(worst['e_margin']) * fit_scale(f64)
            count += 1
    assert count == len(rec['structural']) >= 36
    assert_worst('recorded', worst)


def test_a_min_child_weight_no_side_can_reach_makes_every_tree_a_single_leaf():
    prob = cases.case_problem('n10_F5_T128')
    out = launch([prob], [(2, 0.2, 40., 1.0, 1.0), (1, 0.2, 1e9, 0.8, 0.8)], 3)      # 10 rows hold H = 2.5 at the most
    assert bool((out.tree_feature == -1).all()) and bool((out.tree_threshold == 0).all()) and bool((out.tree_leaf[..., 1:] == 0).all())
    assert bool((out.tree_leaf[..., 0] != 0).any()) and bool((out.status == hipops.XGB_CV_DONE).all())
    worst = new_worst()
    for c, cand in enumerate([(2, 0.2, 40., 1.0, 1.0), (1, 0.2, 1e9, 0.8, 0.8)]):
        f64 = check_through_follow('single leaf', out, 0, c, 5, prob, cand, 3, xf.stream(0, c, 5), worst)
        assert (f64['feature'] == -1).all()
    assert_worst('single leaf', worst)


def test_a_round_with_no_sampled_row_grows_a_zero_tree():
    # the replay: seed 0, refit slot of problem 0 / candidate 0, subsample 0.1 on 10 rows -- round 2 samples nobody (tests/test_host_xgb.py holds the same line)
    assert not xf.sampled_rows(0, xf.stream(0, 0, 5), 2, 10, 0.1).any() and xf.sampled_rows(0, xf.stream(0, 0, 5), 1, 10, 0.1).any()
    prob = cases.case_problem('n10_F5_T128')
    cand = (2, 0.2, 0., 0.1, 1.0)
    out = launch([prob], [cand], 4, seed=0)
    assert bool((out.tree_feature[0, 0, 5, 2] == -1).all()) and bool((out.tree_leaf[0, 0, 5, 2] == 0).all())
    assert bool((out.tree_leaf[0, 0, 5, 1] != 0).any())
    r = xf.fit(*fit_args(prob, cand, 5, 4, xf.stream(0, 0, 5), seed=0))
    assert r['sampled'][2] == 0 and np.array_equal(out.tree_feature[0, 0, 5].numpy(), r['feature'])
    assert np.abs(out.test_margin[0, 0].double().numpy() - r['test_margin']).max() <= floor_rule(0.) * fit_scale(r)


@functools.lru_cache(maxsize=None)
def full_grid():
    """ONE launch: the 16 entries x 6 slots x 100 rounds of both recorded windows, through tabular._xgb_batched."""
    rec = recorded()
    g0, g1 = rec['grid']
    assert g0['seed'] == g1['seed']
    stack = lambda k: torch.stack([g0[k], g1[k]], 1).to(DEV)
    details = {}
    metric, proba, params = tabular._xgb_batched(stack('x'), stack('y'), stack('test_x'), stack('test_y'), return_params=True, seed=g0['seed'], details=details)
    return metric, proba, params, details


@pytest.mark.parametrize('w', [0, 1])
def test_the_full_grid_against_the_recorded_f64_grid_search(w):
    rec = recorded()
    g = rec['grid'][w]
    metric, proba, params, details = full_grid()
    cv64, te64, folds, cls = g['cv_margin'].numpy(), g['test_margin'].numpy(), g['folds'].numpy(), g['y'].numpy() > 0.5
    assert np.array_equal(details['folds'][w], folds) and details['n_splits'] == 5 and bool((details['status'][w] == hipops.XGB_CV_DONE).all())
    scale = g['margin_scale']
    err = max(np.abs(details['cv_margin'][w] - cv64).max(), np.abs(details['test_margin'][w] - te64).max()) / scale
    print(f'window {w}: margins within {err:.3e} of the recorded f64 ones, relative to {scale:.3f} (e {g["e_margin"]:.3e})')
    bounds.within(f'grid window {w} margin (e {g["e_margin"]:.3e})', err, floor_rule(g['e_margin']))
    assert np.array_equal(details['cv_margin'][w] > 0, cv64 > 0)      # the held-out classes
    mean, best = details['scores'][w]
    assert mean.tobytes() == g['mean_test_score'].numpy().tobytes() and best == g['best'] and params[w] == rec['entries'][best]
    p64 = 1. / (1. + np.exp(-te64[best]))
    perr = np.abs(proba[:, w] - p64).max()
    bounds.within(f'grid window {w} proba (e {g["e_proba"]:.3e})', perr, floor_rule(g['e_proba']))
    assert metric[w] == ((p64 > 0.5) == (g['test_y'].numpy() > 0.5)).mean()      # accuracy, as the reference's xgb_metric returns it


SMALL = dict(label='n10_F5_T128', cands=[(2, 0.2, 0.25, 0.8, 0.8), (1, 0.2, 0.5, 0.5, 0.5), (2, 0.02, 0.5, 0.8, 0.8)], rounds=20, ids=(5, 0, 9))


@functools.lru_cache(maxsize=None)
def small_whole():
    probs = [cases.case_problem(SMALL['label'], p) for p in range(3)]
    return probs, launch(probs, SMALL['cands'], SMALL['rounds'], ids=SMALL['ids'])


def same(a, b):
    return all(torch.equal(torch.nan_to_num(x.float(), nan=-7.), torch.nan_to_num(y.float(), nan=-7.)) for x, y in zip(a, b))


def test_a_fit_is_the_same_bits_in_any_batch_any_candidate_grouping_and_any_split_of_the_problems():
    probs, out = small_whole()
    c = SMALL
    # the batch reversed, and split over launches of one and two problems
    rev = launch(probs[::-1], c['cands'], c['rounds'], ids=c['ids'][::-1])
    assert same([t.flip(0) for t in rev], out)
    parts = [launch(probs[:1], c['cands'], c['rounds'], ids=c['ids'][:1]), launch(probs[1:], c['cands'], c['rounds'], ids=c['ids'][1:])]
    assert same([torch.cat([a, b]) for a, b in zip(*parts)], out)
    # the candidates reversed and one candidate alone, under their ids
    back = launch(probs, c['cands'][::-1], c['rounds'], ids=c['ids'], cand_ids=[2, 1, 0])
    assert same([t.flip(1) for t in back], out)
    for k in (0, 2):
        one = launch(probs, c['cands'][k:k + 1], c['rounds'], ids=c['ids'], cand_ids=[k])
        assert same([t[:, 0] for t in one], [t[:, k] for t in out]), k
    # without the trees the margins are the same; another problem id, candidate id or seed is another stream of draws
    bare = launch(probs, c['cands'], c['rounds'], ids=c['ids'], want_trees=False)
    assert bare.tree_feature is None and same(bare[:3], out[:3])
    for other in (dict(ids=(5, 0, 8)), dict(ids=c['ids'], cand_ids=[0, 1, 3]), dict(ids=c['ids'], seed=cases.FIT_SEED + 1)):
        assert not same(launch(probs, c['cands'], c['rounds'], **other)[:2], out[:2]), other


def test_sentinels_unused_slots_and_a_non_finite_problem_stays_alone():
    probs, out = small_whole()
    c = SMALL
    folds = torch.from_numpy(np.stack([p[4] for p in probs]))
    assert bool(torch.isfinite(out.cv_margin).all()) and bool((out.status == hipops.XGB_CV_DONE).all())
    # n_splits = 2 through the entry point: slots 3 .. 5 unused, rows in no fold never written
    dev = lambda k: torch.from_numpy(np.stack([p[k] for p in probs])).to(DEV)
    two = hipops.xgb_cv(dev(0), dev(1), dev(2), dev(4), 2, *([k[i] for k in c['cands']] for i in range(5)), 3, want_trees=True)
    assert bool((two.status[:, :, :3] == hipops.XGB_CV_DONE).all()) and bool((two.status[:, :, 3:] == hipops.XGB_CV_UNUSED).all())
    assert bool(torch.isnan(two.cv_margin.cpu()[(folds >= 2)[:, None, :].expand(-1, 3, -1)]).all()) and bool(torch.isfinite(two.cv_margin.cpu()[(folds < 2)[:, None, :].expand(-1, 3, -1)]).all())
    assert bool((two.tree_feature[:, :, 3:] == -1).all()) and bool(torch.isnan(two.tree_leaf[:, :, 3:]).all()) and bool(torch.isfinite(two.tree_leaf[:, :, :3]).all())
    # a NaN among problem 1's rows: its fits say so, the neighbours keep their bits
    bad = [probs[0], (np.where(np.arange(10)[:, None] == 3, np.nan, probs[1][0]).astype(np.float32),) + probs[1][1:], probs[2]]
    o = launch(bad, c['cands'], c['rounds'], ids=c['ids'])
    assert bool((o.status[1] == hipops.XGB_CV_NONFINITE).all()) and bool((o.status[[0, 2]] == hipops.XGB_CV_DONE).all())
    assert same([t[[0, 2]] for t in o], [t[[0, 2]] for t in out])


def test_evaluate_runs_the_xgb_arm_end_to_end():
    d = torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_diabetes.pt'))
    metric, outputs, ys = tabular.evaluate_position(d['X'].to(DEV), d['y'].to(DEV), [], tabular.xgb_metric, 40, 30, max_samples=3)
    assert metric.shape == (3,) and outputs.shape == (10, 3) and ((metric >= 0) & (metric <= 1)).all() and ((outputs > 0) & (outputs < 1)).all()
    assert np.array_equal(metric, ((outputs > 0.5) == (ys.cpu().numpy() > 0.5)).mean(0))
    res = tabular.evaluate([['diabetes', d['X'], d['y'], []]], tabular.xgb_metric, 'xgb', 40, [30], DEV, max_samples=2)
    assert np.isfinite(res['mean_metric']) and res['diabetes_outputs_at_30'].shape == (10, 2)
    # the single-problem form is column 0 of the batched one
    g = recorded()['grid'][0]
    m1, p1 = tabular.xgb_metric(g['x'].to(DEV), g['y'].to(DEV), g['test_x'].to(DEV), g['test_y'].to(DEV), [])
    m2, p2 = tabular._xgb_batched(*(g[k][:, None].to(DEV) for k in ('x', 'y', 'test_x', 'test_y')))
    assert m1 == m2[0] and np.array_equal(p1, p2[:, 0])
