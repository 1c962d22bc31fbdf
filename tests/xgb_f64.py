"""The gradient-boosting baseline of the tabular study restated in numpy (csrc/xgb_cv.hip, tabular.xgb_metric), written from the contract in include/pfn_hip.h
("Gradient-boosted trees with their grid search"): logistic loss, gradient statistics rounded to 2^-23 fixed point and summed as integers, exact greedy splits
with lambda = 1, the row and column samples replayed from Philox, the tie and legality rules, f32 thresholds.  The gains, the sigmoid, the leaf values and the
margins are f64 (dtype=np.float64) or, operation by operation, f32 (dtype=np.float32: the restatement's own float32 run, whose distance from the f64 one is the
`e` of the project's f32 rule).  Two modes:
    fit(...)            an independent fit;
    fit(..., trees=...) `follow`: the structure (feature, threshold per node) is taken as given -- the device's --, every node's statistics are recomputed, and
                        per node the f64 gain of the given split, the best gain, the legality and the scale |left| + |right| + |root| are reported.
Either mode also reports, per fit, the smallest relative gap between a chosen gain and the best gain of a DIFFERENT partition (or the 1e-6 threshold), and the
smallest distance of a near-best candidate's HL / HR from min_child_weight: where both are large, an f32 run must grow the same trees."""
import itertools

import numpy as np

import nuts_f64 as emu

FIX = float(2 ** 23)
SLOTS, FOLDS, MAX_DEPTH, MAX_ROUNDS = 6, 5, 2, 4096
UNUSED, DONE, NONFINITE = 0, 1, 2
FEATURE_DOMAIN = 1 << 32
MIN_GAIN = 1e-6
PARAM_GRID = {'min_child_weight': [0.5, 1.0], 'learning_rate': [0.02, 0.2], 'subsample': [0.5, 0.8], 'max_depth': [1, 2], 'colsample_bytree': [0.8],
              'eval_metric': ['logloss'], 'n_estimators': [100]}
NEAR = 1e-4      # a candidate is near-best within this share of the scale


def grid_entries(grid=None):
    grid = PARAM_GRID if grid is None else grid
    keys = sorted(grid)
    return [dict(zip(keys, values)) for values in itertools.product(*(grid[k] for k in keys))]


def stream(problem_id, cand_id, slot):
    return (int(problem_id) * 64 + int(cand_id)) * 8 + int(slot)


def row_words(seed, q, t, n):
    """The 32-bit word of every row of the window in round t: component i & 3 of the block at (t << 6) | (i >> 2)."""
    return np.array([emu.philox4x32_10((t << 6) | (i >> 2), q, seed)[i & 3] for i in range(n)], dtype=np.uint64)


def feature_words(seed, q, t, F):
    return np.array([emu.philox4x32_10(FEATURE_DOMAIN | (t << 6) | (f >> 2), q, seed)[f & 3] for f in range(F)], dtype=np.uint64)


def subsample_threshold(subsample):
    return int(np.floor(np.float64(subsample) * 4294967296.))


def sampled_rows(seed, q, t, n, subsample):
    return row_words(seed, q, t, n) < np.uint64(subsample_threshold(subsample)) if subsample_threshold(subsample) < 1 << 32 else np.ones(n, dtype=bool)


def num_columns(colsample, F, fault=None):
    k = max(1, int(np.floor(np.float64(colsample) * F)))
    return min(F, k + 1) if fault == 'k_off_by_one' else k


def sampled_features(seed, q, t, F, colsample, fault=None):
    """The k features of smallest (word, index), ascending by index."""
    w = feature_words(seed, q, t, F)
    return np.sort(np.lexsort((np.arange(F), w))[:num_columns(colsample, F, fault)])


def mcw_fixed(mcw):
    return int(min(np.rint(np.float64(mcw) * FIX), 2. ** 30))


def sigmoid(m, dtype):
    m = np.asarray(m, dtype=dtype)
    e = np.exp(-np.abs(m))
    return (np.where(m >= 0, dtype(1), e) / (dtype(1) + e)).astype(dtype)


def grad_stats(margin, cls, dtype):
    """(gi, hi) int64: g = p - y and h = p (1 - p) rounded to 2^-23."""
    p = sigmoid(margin, dtype)
    g, h = p - cls.astype(dtype), p * (dtype(1) - p)
    return np.rint(g.astype(np.float64) * FIX).astype(np.int64), np.rint(h.astype(np.float64) * FIX).astype(np.int64)


def score(Gi, Hi, dtype, lam=1.):
    G, H = np.asarray(Gi).astype(dtype) * dtype(1. / FIX), np.asarray(Hi).astype(dtype) * dtype(1. / FIX)
    return G * G / (H + dtype(lam))


def threshold(a, b):
    a, b = np.float32(a), np.float32(b)
    thr = np.float32(0.5) * (a + b)
    return b if thr == a else thr


def candidates(x, rows, feats, gi, hi, mcwi, dtype, faults=()):
    """Every candidate of the node with the sampled rows `rows` (ascending row indices): per sampled feature, between consecutive distinct values of the node's
    rows in the feature's (value, row) order.  Returns a dict of arrays over the candidates, ordered by (feature, position): f, pos, a, b (the two values), GLi, HLi,
    gain, scale, legal, and `left(i)`: candidate i's row set; plus the node totals."""
    rows = np.asarray(rows, dtype=np.int64)
    Gt, Ht = int(gi[rows].sum()), int(hi[rows].sum())
    lam = 0. if 'lambda_dropped' in faults else 1.
    out = dict(f=[], pos=[], a=[], b=[], GLi=[], HLi=[])
    order = {}
    for f in feats:
        col = x[rows, f]
        o = np.lexsort((rows, col))
        sr, sv = rows[o], col[o]
        order[int(f)] = sr
        GL, HL = np.cumsum(gi[sr]), np.cumsum(hi[sr])
        pos = np.arange(len(sr) - 1) if 'equal_values_split' in faults else np.flatnonzero(sv[:-1] != sv[1:])
        out['f'].append(np.full(len(pos), int(f), dtype=np.int64)), out['pos'].append(pos), out['a'].append(sv[pos]), out['b'].append(sv[pos + 1])
        out['GLi'].append(GL[pos]), out['HLi'].append(HL[pos])
    c = {k: (np.concatenate(v) if len(v) else np.zeros(0)) for k, v in out.items()}
    c['left'] = lambda i: frozenset(order[int(c['f'][i])][:int(c['pos'][i]) + 1].tolist())
    GLi, HLi = c['GLi'].astype(np.int64).reshape(-1), c['HLi'].astype(np.int64).reshape(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        left, right, root = score(GLi, HLi, dtype, lam), score(Gt - GLi, Ht - HLi, dtype, lam), score(Gt, Ht, dtype, lam)
        c['gain'] = (left + right) - root
    c['scale'] = np.abs(left.astype(np.float64)) + np.abs(right.astype(np.float64)) + abs(float(root))
    c['legal'] = np.ones(len(GLi), dtype=bool) if 'mcw_ignored' in faults else (HLi >= mcwi) & (Ht - HLi >= mcwi)
    c['GLi'], c['HLi'], c['Gt'], c['Ht'] = GLi, HLi, Gt, Ht
    return c


def choose(c, faults=()):
    """Index of the legal candidate of largest gain -- among equal gains the lowest feature, then the lowest position -- or None where there is none."""
    idx = np.flatnonzero(c['legal'])
    if len(idx) == 0:
        return None
    g = c['gain'][idx]
    top = idx[g == g.max()]      # (ordered by (feature, position) already)
    return int(top[-1] if 'tie_to_higher' in faults else top[0])


def node_report(c, chosen, all_rows, mcwi, count_mcw):
    """What the node's decision stands on: `gap`, the distance of the chosen gain (MIN_GAIN for a leaf) from the best legal gain of a different partition and from
    MIN_GAIN, relative to the scale; `mcw`, the smallest |H side - mcw| among the candidates, legal or not, within NEAR of deciding."""
    gain, scale = c['gain'].astype(np.float64), c['scale']
    gap, mcw = np.inf, np.inf
    if len(gain) == 0:
        return gap, mcw
    splits = chosen is not None and gain[chosen] > MIN_GAIN
    level = gain[chosen] if splits else MIN_GAIN
    if splits:
        part = c['left'](chosen)
        gap = (gain[chosen] - MIN_GAIN) / scale[chosen]
        for i in np.argsort(-gain, kind='stable'):
            if not c['legal'][i] or i == chosen:
                continue
            if c['left'](i) != part and c['left'](i) != all_rows - part:
                gap = min(gap, (gain[chosen] - gain[i]) / max(scale[chosen], scale[i]))
                break
    else:
        legal = np.flatnonzero(c['legal'])
        if len(legal):
            i = legal[np.argmax(gain[legal])]
            gap = (MIN_GAIN - gain[i]) / max(scale[i], MIN_GAIN)
    if count_mcw:
        near = gain >= level - NEAR * np.maximum(scale, MIN_GAIN)
        if near.any():
            d = np.minimum(np.abs(c['HLi'][near] - mcwi), np.abs(c['Ht'] - c['HLi'][near] - mcwi))
            mcw = float(d.min()) / FIX
    return float(gap), mcw


def fit(x, y, train_mask, test_x, depth, eta, mcw, subsample, colsample, rounds, seed, q, dtype=np.float64, trees=None, faults=()):
    """One fit.  x [n, F] f32 window rows, y [n] labels, train_mask [n] bool (the slot's training rows), test_x [T, F] f32 or None.  q = stream(problem id, candidate
    id, slot).  trees = (feature [rounds, 3] int, threshold [rounds, 3] f32): follow that structure instead of choosing.  faults: planted faults, for the
    sensitivity study ('lambda_dropped', 'mcw_ignored', 'equal_values_split', 'unsampled_counted', 'k_off_by_one', 'tie_to_higher').
    Returns dict(feature [rounds, 3], threshold [rounds, 3] f32, leaf [rounds, 4], margin [n], test_margin [T], gap, mcw_distance, sampled [rounds] (rows in each
    round's sample), and in follow mode nodes: a list of dict(round, node, given (feature or -1), legal, short, Ht, gain, best, scale) for every node that was open)."""
    x = np.asarray(x, dtype=np.float32)
    n, F = x.shape
    cls = np.asarray(y) > 0.5
    train_mask = np.asarray(train_mask, dtype=bool)
    tx = np.zeros((0, F), dtype=np.float32) if test_x is None else np.asarray(test_x, dtype=np.float32)
    allx = np.concatenate([x, tx])
    eta_t, lam = dtype(np.float32(eta)), (0. if 'lambda_dropped' in faults else 1.)
    mcwi = mcw_fixed(mcw)
    margin = np.zeros(n + len(tx), dtype=dtype)
    feature, thresh, leaves = np.full((rounds, 3), -1, dtype=np.int32), np.zeros((rounds, 3), dtype=np.float32), np.zeros((rounds, 4), dtype=dtype)
    gap, mcw_distance, sampled_count, nodes = np.inf, np.inf, [], []
    for t in range(rounds):
        gi, hi = grad_stats(margin[:n], cls, dtype)
        in_sample = train_mask & (sampled_rows(seed, q, t, n, subsample) | ('unsampled_counted' in faults))
        feats = sampled_features(seed, q, t, F, colsample, 'k_off_by_one' if 'k_off_by_one' in faults else None)
        sampled_count.append(int(in_sample.sum()))
        leaf = np.zeros(n + len(tx), dtype=np.int64)
        root_split = False
        for d in range(depth):
            if d == 1 and not root_split:
                break
            for node in ((0,) if d == 0 else (1, 2)):
                member = in_sample if d == 0 else in_sample & ((leaf[:n] >> 1) == node - 1)
                rows = np.flatnonzero(member)
                c = candidates(x, rows, feats, gi, hi, mcwi, dtype, faults)
                best = choose(c, faults)
                if trees is None:
                    chosen = best if best is not None and c['gain'][best] > MIN_GAIN else None
                    if chosen is not None:
                        feature[t, node], thresh[t, node] = c['f'][chosen], threshold(c['a'][chosen], c['b'][chosen])
                else:
                    gf, gt = int(trees[0][t, node]), np.float32(trees[1][t, node])
                    chosen, rec = None, dict(round=t, node=node, given=gf, legal=True, gain=None, best=None if best is None else float(c['gain'][best]), scale=None)
                    if gf >= 0:
                        feature[t, node], thresh[t, node] = gf, gt
                        match = [i for i in range(len(c['f'])) if c['f'][i] == gf and threshold(c['a'][i], c['b'][i]) == gt] if gf in feats else []
                        if match:
                            chosen = match[0]
                            rec.update(legal=bool(c['legal'][chosen]), gain=float(c['gain'][chosen]), scale=float(c['scale'][chosen]), Ht=int(c['Ht']),
                                       short=int(max(0, mcwi - min(c['HLi'][chosen], c['Ht'] - c['HLi'][chosen]))))      # fixed-point units the lighter side lacks
                        else:
                            rec.update(legal=False)      # no candidate of the node has this feature and threshold
                    elif best is not None:
                        rec.update(scale=float(c['scale'][best]))
                    nodes.append(rec)
                g1, m1 = node_report(c, chosen, frozenset(rows.tolist()), mcwi, t > 0)
                gap, mcw_distance = min(gap, g1), min(mcw_distance, m1)
                if feature[t, node] >= 0:
                    inside = np.ones(len(leaf), dtype=bool) if d == 0 else (leaf >> 1) == node - 1
                    right = inside & ~(allx[:, feature[t, node]] < thresh[t, node])
                    leaf[right] |= 2 if d == 0 else 1
                    root_split = root_split or d == 0
        for L in range(4):
            rows = np.flatnonzero(in_sample & (leaf[:n] == L))
            Gi, Hi = int(gi[rows].sum()), int(hi[rows].sum())
            G, H = dtype(Gi) * dtype(1. / FIX), dtype(Hi) * dtype(1. / FIX)
            leaves[t, L] = eta_t * -(G / (H + dtype(lam))) if len(rows) else dtype(0)
        margin = (margin + leaves[t][leaf]).astype(dtype)
    return dict(feature=feature, threshold=thresh, leaf=leaves, margin=margin[:n], test_margin=margin[n:], gap=float(gap), mcw_distance=float(mcw_distance),
                sampled=sampled_count, nodes=nodes)


def follow(trees, *args, **kw):
    return fit(*args, trees=trees, **kw)


def row_mask(fold, slot, n_splits):
    """The training rows of a slot: fold != slot, every row in the refit slot."""
    fold = np.asarray(fold)
    return np.ones(len(fold), dtype=bool) if slot == n_splits else fold != slot


def select(cv_margin, folds, cls, n_splits):
    """GridSearchCV's ranking from the held-out margins [NC, n]: (mean_test_score [NC], index of the first maximum)."""
    cv_margin, folds, cls = np.asarray(cv_margin, dtype=np.float64), np.asarray(folds), np.asarray(cls, dtype=bool)
    scores = np.stack([(((cv_margin > 0) == cls[None, :])[:, folds == s]).sum(1) / float((folds == s).sum()) for s in range(n_splits)], 1)
    mean = scores.mean(1)
    return mean, int(np.argmax(np.where(np.isnan(mean), -np.inf, mean)))


def grid_search(x, y, test_x, folds, n_splits, entries, seed, problem_id=0, dtype=np.float64, rounds=None, slots=None):
    """Every fit of the grid on one window: (cv_margin [NC, n], test_margin [NC, T], fits {(c, s): fit dict})."""
    n = len(x)
    cv, te, fits = np.full((len(entries), n), np.nan), np.full((len(entries), len(test_x)), np.nan), {}
    for c, e in enumerate(entries):
        for s in (range(n_splits + 1) if slots is None else slots):
            r = fit(x, y, row_mask(folds, s, n_splits), test_x if s == n_splits else None, int(e['max_depth']), e['learning_rate'], e['min_child_weight'],
                    e['subsample'], e['colsample_bytree'], int(e['n_estimators']) if rounds is None else rounds, seed, stream(problem_id, c, s), dtype=dtype)
            fits[c, s] = r
            if s == n_splits:
                te[c] = r['test_margin']
            else:
                held = np.asarray(folds) == s
                cv[c, held] = r['margin'][held]
    return cv, te, fits
