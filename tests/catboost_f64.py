"""The CatBoost baseline of the tabular study restated in numpy (csrc/catboost_cv.hip, tabular.catboost_metric), written from the contract in include/pfn_hip.h
("Oblivious boosted trees with their grid search"): logistic loss, symmetric trees, borders between consecutive distinct values of the learn rows, gradient
statistics rounded to 2^-23 fixed point and summed as integers, the Cosine score with its four running sums, the score noise replayed from Philox, ten Newton
iterations with AnyImprovement backtracking on 2^-40 fixed-point sums.  The scores, the sigmoid, the leaf values and the margins are f64 (dtype=np.float64) or,
operation by operation, f32 (dtype=np.float32: the restatement's own float32 run, whose distance from the f64 one is the `e` of the project's f32 rule).  Modes:
    fit(...)            an independent fit;
    fit(..., trees=...) `follow`: the structure (feature, threshold per level) is taken as given -- the device's --, every level's statistics are recomputed, and
                        per level the legality of the given border (a border of the learn rows, not used before in the tree), its noisy score, the level's
                        best noisy score and the scale |score| + |noise| are reported (the score's terms avg G are all >= 0: their sum of magnitudes is the score).
Either mode reports, per fit, `gap`: the smallest distance, relative to the scale, between a level's best and second noisy score."""
import itertools

import numpy as np

FIX, FIX40 = float(2 ** 23), float(2 ** 40)
SLOTS, MAX_DEPTH, MAX_LEAVES, MAX_ROUNDS, MAX_CHECKPOINTS = 2, 7, 128, 1024, 8
DONE, NONFINITE, ONE_CLASS = 1, 2, 3
NEWTON, HALVINGS = 10, 10
PARAM_GRID = {'learning_rate': [0.1, 0.5, 1.0], 'depth': [2, 4, 7], 'l2_leaf_reg': [0.0, 0.5, 1], 'iterations': [10, 40, 70]}
M32 = np.uint64(0xFFFFFFFF)


def grid_entries(grid=None):
    """The entries in the dict's key order, the last key varying fastest; the distinct fits (learning_rate, depth, l2) in order of first appearance, every
    entry's (fit, checkpoint) and the checkpoints."""
    grid = PARAM_GRID if grid is None else grid
    keys = list(grid)
    entries = [dict(zip(keys, values)) for values in itertools.product(*(grid[k] for k in keys))]
    fits, checkpoints, where = [], sorted({int(v) for v in grid['iterations']}), []
    for e in entries:
        key = (float(e['learning_rate']), int(e['depth']), float(e['l2_leaf_reg']))
        if key not in fits:
            fits.append(key)
        where.append((fits.index(key), checkpoints.index(int(e['iterations']))))
    return entries, fits, where, checkpoints


def stream(problem_id, cand_id, slot):
    return (int(problem_id) * 64 + int(cand_id)) * 8 + int(slot)


def philox_words(idx, q, seed):
    """The first two words of philox4x32_10(idx, stream q, key seed) for an array of counters."""
    idx = np.asarray(idx, dtype=np.uint64)
    c0, c1 = idx & M32, (idx >> np.uint64(32)) & M32
    c2, c3 = np.full_like(c0, int(q) & 0xFFFFFFFF), np.full_like(c0, (int(q) >> 32) & 0xFFFFFFFF)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1


def normals(t, d, f, j, q, seed, dtype):
    """z of the candidates (t, d, f[i], j[i]): Box-Muller on u1 = ((w0 >> 9) + 0.5) 2^-23, u2 = (w1 >> 8) 2^-24."""
    idx = (np.uint64(t) << np.uint64(17)) | (np.uint64(d) << np.uint64(14)) | (np.asarray(f, dtype=np.uint64) << np.uint64(7)) | np.asarray(j, dtype=np.uint64)
    w0, w1 = philox_words(idx, q, seed)
    u1 = ((w0 >> np.uint64(9)).astype(np.float64) + 0.5) * 2. ** -23
    u2 = (w1 >> np.uint64(8)).astype(np.float64) * 2. ** -24
    r = np.sqrt(dtype(-2) * np.log(u1.astype(dtype)))
    return (r * np.cos(np.pi * (2. * u2)).astype(dtype)).astype(dtype)      # (cos(pi x) of an exact x, rounded once)


def sig(z, dtype):
    z = np.asarray(z, dtype=dtype)
    e = np.exp(-np.abs(z))
    return (np.where(z >= 0, dtype(1), e) / (dtype(1) + e)).astype(dtype)


def threshold(a, b):
    a, b = np.float32(a), np.float32(b)
    thr = np.float32(0.5) * (a + b)
    return a if thr == b else thr


def seq_sum(terms, dtype):
    """The running sum from 0 along the last axis, every addition rounded in dtype."""
    terms = np.asarray(terms, dtype=dtype)
    return np.cumsum(terms, axis=-1, dtype=dtype)[..., -1] if terms.shape[-1] else np.zeros(terms.shape[:-1], dtype=dtype)


def borders(x, learn, faults=()):
    """Every border of the fit: arrays f, j (sorted position over all n rows of the last learn row that holds a), a, b, thr, ordered by (f, j)."""
    n, F = x.shape
    out = dict(f=[], j=[], a=[], b=[])
    for f in range(F):
        o = np.lexsort((np.arange(n), x[:, f]))
        pos = np.flatnonzero(learn[o])
        v = x[o[pos], f]
        at = np.arange(len(pos) - 1) if 'border_between_equal' in faults else np.flatnonzero(v[:-1] != v[1:])
        out['f'].append(np.full(len(at), f, dtype=np.int64)), out['j'].append(pos[at]), out['a'].append(v[at]), out['b'].append(v[at + 1])
    c = {k: np.concatenate(v) for k, v in out.items()}
    c['thr'] = np.array([threshold(a, b) for a, b in zip(c['a'], c['b'])], dtype=np.float32)
    return c


def child_terms(Gi, c, l2, dtype, weights=None):
    """(avg G, (avg avg) c) of children with integer sums Gi and counts c; zeros for an empty child.  weights: what stands in for c (a planted fault)."""
    G, cf = np.asarray(Gi).astype(dtype) * dtype(1. / FIX), (np.asarray(c) if weights is None else weights).astype(dtype)
    with np.errstate(divide='ignore', invalid='ignore'):
        avg = np.where(np.asarray(c) > 0, G / (cf + dtype(l2)), dtype(0)).astype(dtype)
    avg = np.where(np.isfinite(avg), avg, dtype(0)).astype(dtype)
    return (avg * G).astype(dtype), ((avg * avg).astype(dtype) * cf).astype(dtype)


def level_scores(x, learn_rows, leaf_index, NL, gi, cand, l2, dtype, faults=(), hess=None):
    """The Cosine score of every candidate of a level.  learn_rows: the learn rows' indices, leaf_index: their place in the leaf list (ascending code)."""
    scores = np.zeros(len(cand['f']), dtype=dtype)
    l2s = 0. if 'l2_dropped_from_score' in faults else l2
    onehot = (leaf_index[None, :] == np.arange(NL)[:, None]).astype(np.float64)      # [NL, learn rows]; the products below are exact integers in f64 (< 2^38)
    Gw, G_all, c_all = onehot * gi[learn_rows], (onehot * gi[learn_rows]).sum(1), onehot.sum(1)
    Hw = onehot * hess[learn_rows] if 'hessian_weights' in faults else None
    for f in np.unique(cand['f']):
        sel = np.flatnonzero(cand['f'] == f)
        bits = (x[learn_rows, f][None, :] > cand['thr'][sel][:, None]).astype(np.float64)      # [candidates, learn rows]
        G_hi, c_hi = np.rint(bits @ Gw.T).astype(np.int64), np.rint(bits @ onehot.T).astype(np.int64)      # [candidates, NL]
        G_lo, c_lo = G_all.astype(np.int64)[None] - G_hi, c_all.astype(np.int64)[None] - c_hi
        w_lo = w_hi = None
        if Hw is not None:
            w_hi = bits @ Hw.T
            w_lo = Hw.sum(1)[None] - w_hi
        n_lo, d_lo = child_terms(G_lo, c_lo, l2s, dtype, w_lo)
        n_hi, d_hi = child_terms(G_hi, c_hi, l2s, dtype, w_hi)
        num, den = seq_sum(n_lo, dtype) + seq_sum(n_hi, dtype), seq_sum(d_lo, dtype) + seq_sum(d_hi, dtype)
        with np.errstate(divide='ignore', invalid='ignore'):
            scores[sel] = np.where(den > 0, num / np.sqrt(den), dtype(0))
    return scores


def objective(margin, cls, v_rows, v_list, l2, dtype):
    z = (margin + v_rows).astype(dtype)
    loss = (np.maximum(np.where(cls, -z, z), dtype(0)) + np.log1p(np.exp(-np.abs(z)))).astype(dtype)
    total = int(np.rint(loss.astype(np.float64) * FIX40).astype(np.int64).sum())
    pen = seq_sum((v_list * v_list).astype(dtype), dtype)
    return dtype(dtype(total) * dtype(1. / FIX40) + dtype(dtype(0.5) * dtype(l2)) * pen)


def newton(margin, cls, leaf_index, NL, l2, dtype, iterations=NEWTON):
    """The leaf values of the list: margin, cls over the learn rows, leaf_index their leaves.  Returns v [NL]."""
    v = np.zeros(NL, dtype=dtype)
    obj = objective(margin, cls, v[leaf_index], v, l2, dtype)
    onehot = leaf_index[None, :] == np.arange(NL)[:, None]
    for _ in range(iterations):
        z = (margin + v[leaf_index]).astype(dtype)
        sp, sm = sig(z, dtype), sig(-z, dtype)
        ri = np.rint(np.where(cls, sm, -sp).astype(np.float64) * FIX40).astype(np.int64)
        hi = np.rint((sp * sm).astype(dtype).astype(np.float64) * FIX40).astype(np.int64)
        R, H = (onehot * ri).sum(1), (onehot * hi).sum(1)
        den = (H.astype(dtype) * dtype(1. / FIX40) + dtype(l2)).astype(dtype)
        with np.errstate(divide='ignore', invalid='ignore'):
            step = np.where(den > 0, (R.astype(dtype) * dtype(1. / FIX40)) / den, dtype(0)).astype(dtype)
        scale, taken = dtype(1), False
        for _ in range(HALVINGS + 1):
            tried_v = (v + (scale * step).astype(dtype)).astype(dtype)
            tried = objective(margin, cls, tried_v[leaf_index], tried_v, l2, dtype)
            if tried <= obj:
                v, obj, taken = tried_v, tried, True
                break
            scale = dtype(scale * dtype(0.5))
        if not taken:
            break
    return v


def fit(x, y, learn, test_x, depth, lr, l2, rounds, seed, q, dtype=np.float64, trees=None, faults=(), newton_iterations=NEWTON):
    """One fit.  x [n, F] f32 window rows, y [n] labels, learn [n] bool (the slot's learn rows), test_x [T, F] f32 or None.  q = stream(problem id, candidate id,
    slot).  trees = (feature [rounds, 7] int, threshold [rounds, 7] f32): follow that structure instead of choosing.  faults: planted faults, for the sensitivity
    study ('l2_dropped_from_score', 'noise_dropped', 'hessian_weights', 'border_between_equal', 'leaf_not_scaled', 'used_kept').
    Returns dict(status, feature [rounds, 7], threshold [rounds, 7] f32, leaf [rounds, 128] (lr v by leaf code), margin [rounds, n] and test_margin [rounds, T]
    (after every tree), gap, and in follow mode levels: a list of dict(tree, level, given, legal, value, best, scale) for every level the fit or the given
    structure has)."""
    x = np.asarray(x, dtype=np.float32)
    n, F = x.shape
    cls = np.asarray(y) > 0.5
    learn = np.asarray(learn, dtype=bool)
    tx = np.zeros((0, F), dtype=np.float32) if test_x is None else np.asarray(test_x, dtype=np.float32)
    if not (np.isfinite(x).all() and np.isfinite(tx).all()):
        return dict(status=NONFINITE)
    if cls[learn].all() or not cls[learn].any():
        return dict(status=ONE_CLASS)
    allx = np.concatenate([x, tx])
    lr_t, l2_t = dtype(np.float32(lr)), dtype(np.float32(l2))
    rows = np.flatnonzero(learn)
    m = len(rows)
    mf = dtype(m)
    all_borders = borders(x, learn, faults)
    margin = np.zeros(n + len(tx), dtype=dtype)
    feature, thresh = np.full((rounds, MAX_DEPTH), -1, dtype=np.int32), np.zeros((rounds, MAX_DEPTH), dtype=np.float32)
    leaves = np.zeros((rounds, MAX_LEAVES), dtype=dtype)
    margins = np.zeros((rounds, n + len(tx)), dtype=dtype)
    gap, levels = np.inf, []
    for t in range(rounds):
        p = sig(margin[:n], dtype)
        g = (cls.astype(dtype) - p).astype(dtype)
        gi = np.where(learn, np.rint(g.astype(np.float64) * FIX), 0).astype(np.int64)
        hess = (p * (dtype(1) - p)).astype(np.float64)
        S2 = int((gi * gi).sum())
        L = np.exp(np.log(mf) - dtype(t) * lr_t)
        sigma = dtype(np.sqrt(dtype(dtype(S2) * dtype(2. ** -46)) / mf) * dtype(L / (dtype(1) + L)))
        if 'noise_dropped' in faults:
            sigma = dtype(0)
        code = np.zeros(n + len(tx), dtype=np.int64)
        used = set()
        for d in range(depth):
            keep = np.array([('used_kept' in faults) or (int(f), int(j)) not in used for f, j in zip(all_borders['f'], all_borders['j'])], dtype=bool)
            cand = {k: v[keep] for k, v in all_borders.items()}
            given = None if trees is None else (int(trees[0][t, d]), np.float32(trees[1][t, d]))
            if len(cand['f']) == 0:
                if given is not None and given[0] >= 0:
                    levels.append(dict(tree=t, level=d, given=given[0], legal=False, value=None, best=None, scale=None))
                    raise ValueError(f'follow: tree {t} level {d} splits where no border is left')
                break
            list_codes = np.unique(code[rows])
            leaf_index = np.searchsorted(list_codes, code[rows])
            scores = level_scores(x, rows, leaf_index, len(list_codes), gi, cand, l2_t, dtype, faults, hess)
            noise = (sigma * normals(t, d, cand['f'], cand['j'], q, seed, dtype)).astype(dtype)
            noisy = (scores + noise).astype(dtype)
            scale = np.abs(scores.astype(np.float64)) + np.abs(noise.astype(np.float64))
            best = int(np.argmax(noisy))      # the first maximum: the candidates are ordered by (feature, position)
            if given is None:
                chosen = best
            else:
                rec = dict(tree=t, level=d, given=given[0], legal=True, value=None, best=float(noisy[best]), scale=float(scale[best]))
                levels.append(rec)
                if given[0] < 0:
                    rec.update(legal=False)      # the given tree ends where a border is left
                    break
                match = np.flatnonzero((cand['f'] == given[0]) & (cand['thr'] == given[1]))
                if len(match) == 0:
                    rec.update(legal=False)
                    chosen = None
                else:
                    chosen = int(match[0])
                    rec.update(value=float(noisy[chosen]), scale=float(max(scale[chosen], scale[best])))
            if chosen is not None:
                fs, th = int(cand['f'][chosen]), np.float32(cand['thr'][chosen])
                used.add((fs, int(cand['j'][chosen])))
                if len(noisy) > 1:
                    second = np.partition(noisy.astype(np.float64), -2)[-2] if chosen == best else float(noisy[best])
                    gap = min(gap, abs(float(noisy[chosen]) - second) / max(float(scale[chosen]), 1e-300))
            else:
                fs, th = given
            feature[t, d], thresh[t, d] = fs, th
            code |= (allx[:, fs] > th).astype(np.int64) << d
        list_codes = np.unique(code[rows])
        leaf_index = np.searchsorted(list_codes, code[rows])
        v = newton(margin[rows], cls[rows], leaf_index, len(list_codes), l2_t, dtype, newton_iterations)
        value = v if 'leaf_not_scaled' in faults else (lr_t * v).astype(dtype)
        leaves[t, list_codes] = value
        margin = (margin + leaves[t][code]).astype(dtype)
        margins[t] = margin
    return dict(status=DONE, feature=feature, threshold=thresh, leaf=leaves, margin=margins[:, :n], test_margin=margins[:, n:], gap=float(gap), levels=levels)


def follow(trees, *args, **kw):
    return fit(*args, trees=trees, **kw)


def certificate(levels):
    """The worst (best - given) / scale over the levels of a follow; inf where a given border is not a legal unused one.  (A level whose scores and noise are
    all 0 -- a saturated fit -- has scale 0 and best = given = 0: it adds nothing.)"""
    worst = 0.
    for lv in levels:
        if not lv['legal']:
            return np.inf
        worst = max(worst, (lv['best'] - lv['value']) / max(lv['scale'], 1e-300))
    return worst


def fit_scale(r):
    """The scale of a fit's margins: the sum over the trees of the tree's largest leaf value.  A margin is a sum of leaf values of either sign and its error a
    sum of theirs, so a margin that cancels to almost nothing measures nothing by its own size (as tests/test_gpu_xgb.py)."""
    return max(np.abs(np.asarray(r['leaf'], dtype=np.float64)).max(1).sum(), 1e-30)


def learn_mask(fold, slot):
    """The learn rows of a slot: fold != 0 in the search fit, every row in the refit."""
    fold = np.asarray(fold)
    return np.ones(len(fold), dtype=bool) if slot == 1 else fold != 0


def logloss(margin, cls):
    """Per row, f64: log(1 + exp(-margin)) for class 1, log(1 + exp(margin)) for class 0."""
    margin = np.asarray(margin, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.logaddexp(0., np.where(np.asarray(cls, dtype=bool), -margin, margin))


def select(hold_margin, fold, cls, where):
    """grid_search's ranking: hold_margin [fits, NK, n]; per entry the mean log loss of the held-out rows, NaN last, the FIRST minimum."""
    held = np.asarray(fold) == 0
    loss = np.array([logloss(hold_margin[c, k][held], np.asarray(cls)[held]).mean() for c, k in where])
    return loss, int(np.argmin(np.where(np.isnan(loss), np.inf, loss)))


def grid_search(x, y, test_x, fold, fits, checkpoints, seed, problem_id=0, dtype=np.float64, slots=(0, 1)):
    """Every fit of the grid on one window: (hold_margin [fits, NK, n] (NaN at the learn rows), test_margin [fits, NK, T], fits {(c, s): fit dict})."""
    n = len(x)
    hold, te, out = np.full((len(fits), len(checkpoints), n), np.nan), np.full((len(fits), len(checkpoints), len(test_x)), np.nan), {}
    held = np.asarray(fold) == 0
    for c, (lr, depth, l2) in enumerate(fits):
        for s in slots:
            r = fit(x, y, learn_mask(fold, s), test_x if s == 1 else None, depth, lr, l2, checkpoints[-1], seed, stream(problem_id, c, s), dtype=dtype)
            out[c, s] = r
            if r['status'] != DONE:
                continue
            for k, count in enumerate(checkpoints):
                if s == 1:
                    te[c, k] = r['test_margin'][count - 1]
                else:
                    hold[c, k, held] = r['margin'][count - 1][held]
    return hold, te, out
