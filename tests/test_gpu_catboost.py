"""pfn_catboost_cv on the MI355X against the restatement tests/catboost_f64.py (written from the contract in include/pfn_hip.h).  Everywhere, through `follow`:
the device's trees taken as given, every chosen border is a legal unused one and its noisy f64 score is within the certificate slack of the level's best, every
leaf value and every checkpoint's margins within the project's f32 rule 4 max(e, 2^-23) of their scale, e the error of the restatement's own float32 run of the
same structure against the f64 one (never taken from the kernel).  On the recorded fits that meet the gap condition (tests/golden/tabular_catboost.pt) the trees
equal the independent f64 fit's, thresholds bit for bit.  Then the planted columns, the tree that runs out of borders, ONE_CLASS, the bitwise invariants of the
contract, the full 81-entry grid against the recorded f64 grid searches, and the study's arm end to end.
PFN_RECORD_BOUNDS=<path> writes every measured maximum with its e (profiles/r24_catboost_cv_bounds_measured.json is such a run)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds      # noqa: E402
import tabular_cases      # noqa: E402
import catboost_cases as cases      # noqa: E402
import catboost_f64 as cf      # noqa: E402

from transformerscandobayesianinference_amd import hipops, tabular      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
FLOOR = 2. ** -23


@functools.lru_cache(maxsize=None)
def recorded():
    return torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_catboost.pt'), weights_only=False)


def floor_rule(e):
    return 4 * max(e, FLOOR)


def certificate_slack():
    """Four times what f32 rounding alone cost the restatement's float32 runs (recorded: the worst (best - chosen) / (|score| + |noise|) against f64), and no less
    than four f32 roundings of that scale."""
    return 4 * max(recorded()['certificate_e'], FLOOR)


def launch(problems, cands, rounds, checkpoints=None, seed=cases.FIT_SEED, ids=None, cand_ids=None, want_trees=True):
    """hipops.catboost_cv on problems [(x, y, tx, ty, fold)] with candidates [(depth, lr, l2)]: CatboostCvOut on the host."""
    dev = lambda k: torch.from_numpy(np.stack([p[k] for p in problems])).to(DEV)
    ids = None if ids is None else torch.tensor(list(ids), dtype=torch.int64, device=DEV)
    out = hipops.catboost_cv(dev(0), dev(1), dev(2), dev(4), *([c[k] for c in cands] for k in range(3)), rounds, checkpoints=checkpoints, seed=seed, problem_ids=ids,
                             want_trees=want_trees, cand_ids=cand_ids)
    return hipops.CatboostCvOut(*(None if t is None else t.cpu() for t in out))


def fit_args(prob, cand, slot, rounds, q, seed=cases.FIT_SEED):
    x, y, tx, ty, fold = prob
    return (x, y, cf.learn_mask(fold, slot), tx if slot == 1 else None, *cand, rounds, seed, q)


def device_outputs(out, p, c, s, fold):
    """[NK, rows]: the margins the fit wrote at every checkpoint."""
    return (out.test_margin[p, c] if s == 1 else out.hold_margin[p, c][:, torch.from_numpy(np.asarray(fold) == 0)]).double().numpy()


def host_outputs(r, s, fold, checkpoints):
    at = [k - 1 for k in checkpoints]
    return np.asarray(r['test_margin'][at] if s == 1 else r['margin'][at][:, np.asarray(fold) == 0], dtype=np.float64)


def check_through_follow(label, out, p, c, s, prob, cand, rounds, checkpoints, q, worst, seed=cases.FIT_SEED):
    """The device's fit (p, c, s) followed in f64 and in f32; asserts legality and the certificate, adds the measured leaf and margin errors to `worst`."""
    trees = (out.tree_feature[p, c, s].numpy(), out.tree_threshold[p, c, s].numpy())
    args = fit_args(prob, cand, s, rounds, q, seed)
    f64, f32 = cf.follow(trees, *args), cf.follow(trees, *args, dtype=np.float32)
    assert int(out.status[p, c, s]) == hipops.CATBOOST_CV_DONE
    slack = certificate_slack()
    for lv in f64['levels']:
        assert lv['legal'], (label, p, c, s, lv)      # a border of the learn rows, not used before in this tree; no tree ends where a border is left
        assert lv['value'] >= lv['best'] - slack * lv['scale'], (label, p, c, s, lv)
        worst['certificate'] = max(worst['certificate'], (lv['best'] - lv['value']) / max(lv['scale'], 1e-300))
    for name, got, want, approx in (('leaf', out.tree_leaf[p, c, s].double().numpy(), f64['leaf'], f32['leaf']),
                                    ('margin', device_outputs(out, p, c, s, prob[4]), host_outputs(f64, s, prob[4], checkpoints), host_outputs(f32, s, prob[4], checkpoints))):
        scale = max(np.abs(f64['leaf']).max(), 1e-30) if name == 'leaf' else cf.fit_scale(f64)
        assert np.isfinite(got).all(), (label, p, c, s, name)
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
    n, F, T, cands, rounds, checkpoints, slots = cases.CASES[label]
    probs = [cases.case_problem(label, p) for p in range(2)]
    ids = (5, 0)
    out = launch(probs, cands, rounds, checkpoints, ids=ids)
    held = torch.from_numpy(np.stack([p[4] for p in probs]) == 0)[:, None, None, :].expand(-1, len(cands), len(checkpoints), -1)
    assert bool((out.status == hipops.CATBOOST_CV_DONE).all()) and bool(torch.isfinite(out.test_margin).all())
    assert bool(torch.isfinite(out.hold_margin[held]).all()) and bool(torch.isnan(out.hold_margin[~held]).all())      # the learn rows are never written
    assert bool(torch.isfinite(out.tree_leaf).all()) and bool(torch.isfinite(out.tree_threshold).all())
    worst, structural = new_worst(), 0
    for p, prob in enumerate(probs):
        for c, cand in enumerate(cands):
            feature = out.tree_feature[p, c].numpy()
            levels = (feature >= 0).sum(-1)
            assert (levels <= cand[0]).all() and all(((f >= 0) == (np.arange(7) < k)).all() for f, k in zip(feature.reshape(-1, 7), levels.reshape(-1)))
            if F >= 5:      # the constant column has no border
                assert not (feature == cases.CONSTANT).any(), (label, p, c)
            for s in slots:
                q = cf.stream(ids[p], c, s)
                check_through_follow(label, out, p, c, s, prob, cand, rounds, checkpoints, q, worst)
                if p == 0:      # where the f64 fit alone shows the gap, the independent fit grows the same trees, thresholds bit for bit
                    r = cf.fit(*fit_args(prob, cand, s, rounds, q))
                    if r['gap'] >= cases.MIN_GAP:
                        structural += 1
                        assert np.array_equal(feature[s], r['feature']) and out.tree_threshold[p, c, s].numpy().tobytes() == r['threshold'].tobytes(), (label, p, c, s)
    if F >= 5:      # a column of the three values -1, 0, 1: wherever it is chosen, the threshold is a midpoint of two of them
        thr = out.tree_threshold[out.tree_feature == cases.THREE_VALUED]
        assert bool(torch.isin(thr, torch.tensor([-0.5, 0., 0.5])).all())
    print(f'{label}: {structural} fits compared structurally')
    assert_worst(label, worst)


def test_a_tree_ends_when_no_border_is_left():
    prob = cases.three_value_problem()
    cands = [(4, 0.5, 0.5), (1, 0.5, 0.0)]
    out = launch([prob], cands, 3, (1, 3))
    assert bool((out.status[0, :, 1] == hipops.CATBOOST_CV_DONE).all())
    feature = out.tree_feature[0, 0, 1].numpy()
    assert (feature[:, :2] == 0).all() and (feature[:, 2:] == -1).all()      # three values, two borders: depth 4 ends after two levels
    thr = np.sort(out.tree_threshold[0, 0, 1].numpy()[:, :2], axis=1)
    assert (thr == np.array([-0.5, 0.5], dtype=np.float32)).all()
    assert bool((out.tree_leaf[0, 0, 1][:, 4:] == 0).all())      # two bits: leaf codes 0 .. 3
    worst = new_worst()
    for c, cand in enumerate(cands):
        check_through_follow('three values', out, 0, c, 1, prob, cand, 3, (1, 3), cf.stream(0, c, 1), worst)
    assert_worst('three values', worst)


def test_a_hold_out_that_leaves_one_class_is_reported_and_writes_nothing():
    prob = cases.one_class_problem()
    out = launch([prob], [(2, 0.5, 0.5)], 3, (1, 3))
    assert int(out.status[0, 0, 0]) == hipops.CATBOOST_CV_ONE_CLASS and int(out.status[0, 0, 1]) == hipops.CATBOOST_CV_DONE
    assert bool(torch.isnan(out.hold_margin).all()) and bool(torch.isfinite(out.test_margin).all())
    assert bool((out.tree_feature[0, 0, 0] == -1).all()) and bool(torch.isnan(out.tree_leaf[0, 0, 0]).all()) and bool(torch.isfinite(out.tree_leaf[0, 0, 1]).all())
    assert cf.fit(*fit_args(prob, (2, 0.5, 0.5), 0, 3, cf.stream(0, 0, 0)))['status'] == cf.ONE_CLASS
    worst = new_worst()
    check_through_follow('one class', out, 0, 0, 1, prob, (2, 0.5, 0.5), 3, (1, 3), cf.stream(0, 0, 1), worst)
    assert_worst('one class', worst)


def test_recorded_fits_that_meet_the_gap_condition_grow_the_recorded_trees():
    rec = recorded()
    worst, count = new_worst(), 0
    for k, (n, F, T, seed, rounds) in enumerate(cases.STRUCTURAL):
        x, y, tx, ty = tabular_cases.problem(n, F, T, seed)
        prob = (x, y, tx, ty, cases.holdout_fold(y))
        out = launch([prob], cases.STRUCTURAL_CANDS, rounds, ids=(k,))
        for f in (f for f in rec['structural'] if f['problem'] == k):
            c, s = f['cand'], f['slot']
            assert np.array_equal(out.tree_feature[0, c, s].numpy(), f['feature'].numpy()), (k, c, s)
            assert out.tree_threshold[0, c, s].numpy().tobytes() == f['threshold'].numpy().tobytes(), (k, c, s)
            f64 = check_through_follow('recorded', out, 0, c, s, prob, cases.STRUCTURAL_CANDS[c], rounds, (rounds,), cf.stream(k, c, s), worst)
            want = f['out'].numpy()
            assert np.array_equal(host_outputs(f64, s, prob[4], (rounds,))[0], want)      # the same trees: following them is the recorded fit
            count += 1
    assert count == len(rec['structural']) and 2 * count >= rec['structural_fits']
    assert_worst('recorded', worst)


SMALL = dict(label='n10_F5_T128', cands=[(4, 0.5, 0.0), (7, 0.1, 0.5), (2, 1.0, 1.0)], rounds=6, checkpoints=(2, 5, 6), ids=(5, 0, 9))


@functools.lru_cache(maxsize=None)
def small_whole():
    probs = [cases.case_problem(SMALL['label'], p) for p in range(3)]
    return probs, launch(probs, SMALL['cands'], SMALL['rounds'], SMALL['checkpoints'], ids=SMALL['ids'])


def same(a, b):
    return all(torch.equal(torch.nan_to_num(x.float(), nan=-7.), torch.nan_to_num(y.float(), nan=-7.)) for x, y in zip(a, b))


def test_a_fit_is_the_same_bits_in_any_batch_any_candidate_grouping_and_a_second_run():
    probs, out = small_whole()
    c = SMALL
    again = launch(probs, c['cands'], c['rounds'], c['checkpoints'], ids=c['ids'])
    assert same(again, out)
    # the batch reversed, and split over launches of one and two problems
    rev = launch(probs[::-1], c['cands'], c['rounds'], c['checkpoints'], ids=c['ids'][::-1])
    assert same([t.flip(0) for t in rev], out)
    parts = [launch(probs[:1], c['cands'], c['rounds'], c['checkpoints'], ids=c['ids'][:1]), launch(probs[1:], c['cands'], c['rounds'], c['checkpoints'], ids=c['ids'][1:])]
    assert same([torch.cat([a, b]) for a, b in zip(*parts)], out)
    # the candidates reversed and one candidate alone, under their ids
    back = launch(probs, c['cands'][::-1], c['rounds'], c['checkpoints'], ids=c['ids'], cand_ids=[2, 1, 0])
    assert same([t.flip(1) for t in back], out)
    for k in (0, 2):
        one = launch(probs, c['cands'][k:k + 1], c['rounds'], c['checkpoints'], ids=c['ids'], cand_ids=[k])
        assert same([t[:, 0] for t in one], [t[:, k] for t in out]), k
    # without the trees the margins are the same; another problem id, candidate id or seed is another stream of draws
    bare = launch(probs, c['cands'], c['rounds'], c['checkpoints'], ids=c['ids'], want_trees=False)
    assert bare.tree_feature is None and same(bare[:3], out[:3])
    for other in (dict(ids=(5, 0, 8)), dict(ids=c['ids'], cand_ids=[0, 1, 3]), dict(ids=c['ids'], seed=cases.FIT_SEED + 1)):
        assert not same(launch(probs, c['cands'], c['rounds'], c['checkpoints'], **other)[:2], out[:2]), other


def test_a_checkpoint_holds_the_margins_of_a_launch_that_stops_there():
    probs, out = small_whole()
    c = SMALL
    for k, count in enumerate(c['checkpoints']):
        short = launch(probs, c['cands'], count, ids=c['ids'])
        assert same([short.hold_margin[:, :, 0], short.test_margin[:, :, 0]], [out.hold_margin[:, :, k], out.test_margin[:, :, k]]), count
        assert same([short.tree_feature, short.tree_threshold, short.tree_leaf], [t[:, :, :, :count] for t in out[3:]]), count


def test_a_non_finite_problem_stays_alone():
    probs, out = small_whole()
    c = SMALL
    bad = [probs[0], (np.where(np.arange(10)[:, None] == 3, np.nan, probs[1][0]).astype(np.float32),) + probs[1][1:], probs[2]]
    o = launch(bad, c['cands'], c['rounds'], c['checkpoints'], ids=c['ids'])
    assert bool((o.status[1] == hipops.CATBOOST_CV_NONFINITE).all()) and bool((o.status[[0, 2]] == hipops.CATBOOST_CV_DONE).all())
    assert bool(torch.isnan(o.hold_margin[1]).all()) and bool(torch.isnan(o.test_margin[1]).all())      # refused: nothing but the status is written
    assert same([t[[0, 2]] for t in o], [t[[0, 2]] for t in out])


@functools.lru_cache(maxsize=None)
def full_grid():
    """ONE launch: the 27 fits x 2 slots x 70 trees of both recorded windows, through tabular._catboost_batched."""
    rec = recorded()
    g0, g1 = rec['grid']
    assert g0['seed'] == g1['seed']
    stack = lambda k: torch.stack([g0[k], g1[k]], 1).to(DEV)
    details = {}
    metric, proba, params = tabular._catboost_batched(stack('x'), stack('y'), stack('test_x'), stack('test_y'), return_params=True, seed=g0['seed'], details=details)
    return metric, proba, params, details


@pytest.mark.parametrize('w', [0, 1])
def test_the_full_grid_against_the_recorded_f64_grid_search(w):
    rec = recorded()
    g = rec['grid'][w]
    metric, proba, params, details = full_grid()
    entries, fits, where, checkpoints = tabular._catboost_grid()
    fold, loss64 = g['fold'].numpy(), g['loss'].numpy()
    assert np.array_equal(details['folds'][w], fold) and bool((details['status'][w] == hipops.CATBOOST_CV_DONE).all())
    assert np.isfinite(details['test_margin'][w]).all() and np.isfinite(details['hold_margin'][w][:, :, fold == 0]).all()
    loss, best = details['scores'][w]
    bound = g['loss_bound']      # the f32 rule on the margins behind the recorded best entry's log loss (tools/record_catboost_cv_fixtures.py)
    print(f'window {w}: device entry {best} (f64 log loss {loss64[best]:.6f}), recorded entry {g["best"]} ({loss64[g["best"]]:.6f}), runner-up {g["runner_up"]:.3e} away, '
          f'bound {bound:.3e}')
    if g['runner_up'] > bound:
        assert best == g['best'] and params[w] == rec['entries'][best]
    assert loss64[best] - loss64[g['best']] <= bound
    # where the float32 restatement grew the f64 trees with the gap to spare, the device's margins are the recorded ones by the f32 rule on the fit's scale
    hold64, test64, clear = g['hold_margin'].numpy(), g['test_margin'].numpy(), (g['same'] & (g['gap'] >= cases.MIN_GAP)).numpy()
    worst = 0.
    for c in range(len(fits)):
        if clear[c, 0]:
            worst = max(worst, np.abs(details['hold_margin'][w][c][:, fold == 0] - hold64[c][:, fold == 0]).max() / float(g['scale'][c, 0]))
        if clear[c, 1]:
            worst = max(worst, np.abs(details['test_margin'][w][c] - test64[c]).max() / float(g['scale'][c, 1]))
    print(f'window {w}: margins of the {int(clear.sum())} clear fits within {worst:.3e} of the recorded f64 ones (e {g["e_margin"]:.3e})')
    bounds.within(f'grid window {w} margin (e {g["e_margin"]:.3e})', worst, floor_rule(g['e_margin']))
    c, k = where[best]
    assert np.array_equal(proba[:, w], 1. / (1. + np.exp(-details['test_margin'][w][c, k])))


def test_evaluate_runs_the_catboost_arm_end_to_end():
    d = torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_diabetes.pt'))
    metric, outputs, ys = tabular.evaluate_position(d['X'].to(DEV), d['y'].to(DEV), [], tabular.catboost_metric, 40, 30, max_samples=3)
    assert metric.shape == (3,) and outputs.shape == (10, 3) and ((metric >= 0) & (metric <= 1)).all() and ((outputs >= 0) & (outputs <= 1)).all()
    want, _ = tabular.roc_auc_columns(torch.from_numpy(outputs).float().to(DEV), ys)
    assert np.array_equal(metric, want)
    res = tabular.evaluate([['diabetes', d['X'], d['y'], []]], tabular.catboost_metric, 'catboost', 40, [30], DEV, max_samples=2)
    assert np.isfinite(res['mean_metric']) and res['diabetes_outputs_at_30'].shape == (10, 2)
    # the single-problem form is column 0 of the batched one
    g = recorded()['grid'][0]
    m1, p1 = tabular.catboost_metric(g['x'].to(DEV), g['y'].to(DEV), g['test_x'].to(DEV), g['test_y'].to(DEV), [])
    m2, p2 = tabular._catboost_batched(*(g[k][:, None].to(DEV) for k in ('x', 'y', 'test_x', 'test_y')))
    assert m1 == m2[0] and np.array_equal(p1, p2[:, 0])
    with pytest.raises(ValueError, match='one class'):
        tabular.catboost_metric(g['x'].to(DEV), torch.zeros_like(g['y']).to(DEV), g['test_x'].to(DEV), g['test_y'].to(DEV), [])
