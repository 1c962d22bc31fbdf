"""Restatement of csrc/bnn_cv.hip written from its contract (include/pfn_hip.h "BNN classifier with its grid search"), in torch / numpy on the CPU.  Every function
takes its precision from `dtype` (or from its operands): torch.float64 is the reference, torch.float32 -- the same formulas, operand by operand, in the
kernel's number format -- is the yardstick e of the project's f32 rule (README): a kernel result may differ from the f64 one by 4 max(e, 2^-23).

    theta = (W1 [H,F], b1 [H], W2 [2,H], b2 [2]),  o = W2 (W1 x + b1) + b2,  U = |theta|^2 / 2 + (D / 2) log 2 pi - sum_i m_i log softmax(o_i)[y_i]
    theta = loc + softplus(u) eps,  L = U(theta) - sum_i (log scale_i + eps_i^2 / 2) - (D / 2) log 2 pi
    g_loc = grad U,  g_scale = grad U * eps - 1 / scale,  g_u = g_scale sigmoid(u),  Adam as torch.optim.Adam (bnn_f64.adam)

The noise is the kernel's, from tests/nuts_f64.py's philox4x32_10 on numpy arrays: stream q = problem id * 8 + slot, key = seed, and
    step t, coordinate i:        component i & 3 of normal4(block ((t << 12) | (i >> 2)))
    predictive draw k:           the same at ((2^41 + k) << 12) | (i >> 2)
    observation uniform, row r:  (word r & 3 of block ((2^42 + k) << 12) | (r >> 2)) >> 8) * 2^-24,  r = i for train row i, n + j for test row j
The masked potential is bnn_f64.potentials on the compacted rows (f64); `dense_grads` is its closed-form gradient through the n x H hidden matrix, `rank_one_grads`
the form the kernel uses (v = W2[1] - W2[0], r = X^T g); the host tests check both against autograd and against each other."""
import math

import numpy as np
import torch

import bnn_f64 as ref
from bnn_f64 import adam, f32      # noqa: F401
import nuts_f64 as emu

SLOTS, FOLDS = 6, 5
UNUSED, DONE, NONFINITE = 0, 1, 2
PRED_DOMAIN, OBS_DOMAIN = 1 << 41, 1 << 42
PARAM_GRID = {'embed': [5, 10, 30, 64], 'lr': [1e-3, 1e-4], 'num_training_steps': [400], 'num_samples_for_prediction': [400]}      # reference tabular.py:372-376
# the problems of tests/golden/tabular_bnn.pt: (n, F, T) of tabular_cases.problem
SHAPES = [(10, 3, 5), (20, 8, 10), (40, 60, 8), (24, 128, 4)]


def stream(problem_id, slot):
    return int(problem_id) * 8 + int(slot)


def block_index(base, D):
    """The Philox counters of the blocks that hold coordinates 0 .. D - 1 in the domain `base` (a step index, 2^41 + draw, 2^42 + draw)."""
    return (np.uint64(int(base)) << np.uint64(12)) | np.arange((D + 3) // 4, dtype=np.uint64)


def _words(base, D, q, seed):
    return [np.asarray(c, dtype=np.uint64) for c in emu.philox4x32_10(block_index(base, D), int(q), int(seed))]


def normals(base, D, q, seed, dtype=torch.float64):
    """[D] standard normals of the domain `base`: Box-Muller on each block's four words, in `dtype`."""
    x, y, z, w = _words(base, D, q, seed)
    ft = np.float64 if dtype == torch.float64 else np.float32
    u_open = lambda r: ((r >> np.uint64(8)).astype(ft) + ft(1)) * ft(2. ** -24)
    u = lambda r: (r >> np.uint64(8)).astype(ft) * ft(2. ** -24)
    r0, r1 = np.sqrt(ft(-2) * np.log(u_open(x))), np.sqrt(ft(-2) * np.log(u_open(z)))
    a0, a1 = ft(2. * math.pi) * u(y), ft(2. * math.pi) * u(w)
    out = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], -1).reshape(-1)
    assert out.dtype == ft
    return torch.from_numpy(out[:D].copy())


def step_noise(seed, q, t, D, dtype=torch.float64):
    return normals(t, D, q, seed, dtype)


def pred_noise(seed, q, k, D, dtype=torch.float64):
    return normals(PRED_DOMAIN + k, D, q, seed, dtype)


def obs_uniforms(seed, q, k, R):
    """[R] uniforms of predictive draw k (multiples of 2^-24: the same number in f32 and f64)."""
    words = np.stack(_words(OBS_DOMAIN + k, R, q, seed), -1).reshape(-1)[:R]
    return torch.from_numpy((words >> np.uint64(8)).astype(np.float64) * 2. ** -24)


def row_mask(folds, slot, n_splits):
    """bool [n]: the rows slot `slot` trains on -- all for the refit, else those whose fold differs (a fold value outside 0 .. n_splits - 1 always trains)."""
    folds = np.asarray(folds)
    return np.ones(len(folds), dtype=bool) if slot == n_splits else folds != slot


def softplus(u):
    return torch.clamp(u, min=0.) + torch.log1p(torch.exp(-u.abs()))


def potential(theta, x, y, mask, F, H):
    """U(theta) (differentiable) on the rows with mask: bnn_f64.potentials on the compacted rows in f64; the same expression in theta's own precision otherwise."""
    keep = torch.as_tensor(np.asarray(mask, dtype=bool))
    xc, yc = x[keep], y[keep]
    if theta.dtype == torch.float64:
        return ref.potentials(theta[None, :], xc, yc, len(xc), F, H, 0)[0]
    W1, b1, W2, b2 = ref.unpack(theta, F, H)
    D = theta.shape[0]
    U = 0.5 * (theta * theta).sum() + 0.5 * D * math.log(2. * math.pi)
    if len(xc):
        o = (xc.to(theta.dtype) @ W1.T + b1) @ W2.T + b2
        U = U - torch.log_softmax(o, -1).gather(1, (yc > 0.5).long()[:, None]).sum()
    return U


def _rows(theta, x, y, mask):
    keep = torch.as_tensor(np.asarray(mask, dtype=bool))
    return x[keep].to(theta.dtype), (y[keep] > 0.5)


def _row_terms(d, y1):
    """(sum softplus(-+d), g = sigma(d) - y) from the logit differences of the kept rows."""
    z = torch.where(y1, -d, d)
    e = torch.exp(-z.abs())
    sp = torch.clamp(z, min=0.) + torch.log1p(e)
    sg = torch.where(z >= 0, torch.ones_like(e), e) / (1. + e)
    return sp.sum(), torch.where(y1, -sg, sg)


def dense_grads(theta, x, y, mask, F, H):
    """(U, grad U [D]) in closed form through the hidden matrix h [n, H]."""
    W1, b1, W2, b2 = ref.unpack(theta, F, H)
    xc, y1 = _rows(theta, x, y, mask)
    D = theta.shape[0]
    h = xc @ W1.T + b1
    o = h @ W2.T + b2
    sp, g = _row_terms(o[:, 1] - o[:, 0], y1)
    v = W2[1] - W2[0]
    A, G = g @ h, g.sum()
    dh = g[:, None] * v[None, :]
    grad = torch.cat([(dh.T @ xc).reshape(-1), dh.sum(0), -A, A, torch.stack([-G, G])]) + theta
    return 0.5 * (theta * theta).sum() + 0.5 * D * math.log(2. * math.pi) + sp, grad


def rank_one_grads(theta, x, y, mask, F, H):
    """The same two numbers as the kernel forms them: v = W2[1] - W2[0], o_1 - o_0 = x . (W1^T v) + v . b1 + b2[1] - b2[0], r = X^T g, A = W1 r + b1 G."""
    W1, b1, W2, b2 = ref.unpack(theta, F, H)
    xc, y1 = _rows(theta, x, y, mask)
    D = theta.shape[0]
    v = W2[1] - W2[0]
    sp, g = _row_terms(xc @ (W1.T @ v) + (v @ b1 + (b2[1] - b2[0])), y1)
    r, G = xc.T @ g, g.sum()
    A = W1 @ r + b1 * G
    grad = torch.cat([(v[:, None] * r[None, :]).reshape(-1), v * G, -A, A, torch.stack([-G, G])]) + theta
    return 0.5 * (theta * theta).sum() + 0.5 * D * math.log(2. * math.pi) + sp, grad


def loss(loc, u, eps, x, y, mask, F, H):
    """The per-step loss as a differentiable function of (loc, u) at fixed noise eps [D]."""
    scale = softplus(u)
    D = loc.shape[0]
    return potential(loc + scale * eps, x, y, mask, F, H) - (torch.log(scale) + 0.5 * eps * eps).sum() - 0.5 * D * math.log(2. * math.pi)


def loss_and_grads(loc, u, eps, x, y, mask, F, H, grads=dense_grads):
    """(L, g_loc [D], g_u [D]) by the closed form of the contract."""
    scale = softplus(u)
    D = loc.shape[0]
    U, gU = grads(loc + scale * eps, x, y, mask, F, H)
    L = U - (torch.log(scale) + 0.5 * eps * eps).sum() - 0.5 * D * math.log(2. * math.pi)
    return L, gU, (gU * eps - 1. / scale) * torch.sigmoid(u)


def run(state, x, y, mask, F, H, lr, q, seed=0, step0=0, num_steps=1, betas=(0.9, 0.999), eps=1e-8, dtype=torch.float64):
    """`num_steps` steps of one fit from state [6, >= D] (rows loc, u, m_loc, v_loc, m_u, v_u): returns (state [6, D] in dtype, losses [num_steps] f64)."""
    D = ref.num_params(F, H)
    loc, u, m_loc, v_loc, m_u, v_u = (torch.as_tensor(state)[r, :D].to(dtype).clone() for r in range(6))
    lr, b1, b2, eps = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps)
    losses = []
    for t in range(step0, step0 + num_steps):
        z = step_noise(seed, q, t, D, dtype)
        L, g_loc, g_u = loss_and_grads(loc, u, z, x, y, mask, F, H)
        losses.append(float(L))
        loc, m_loc, v_loc = adam(loc, m_loc, v_loc, g_loc, t + 1, lr, b1, b2, eps)
        u, m_u, v_u = adam(u, m_u, v_u, g_u, t + 1, lr, b1, b2, eps)
    return torch.stack([loc, u, m_loc, v_loc, m_u, v_u]), np.array(losses)


def predictive(loc, u, rows, row_ids, F, H, S, q, seed=0, want_draws=False):
    """The predictive of one fit at the rows `rows` [R, F] whose observation-uniform indices are row_ids [R]: (prob [R]: the mean over the S draws of
    sigmoid(o_1 - o_0), added in draw order; probs [S, R] and hit [S, R] bool = (uniform < prob) with want_draws, else None).  Precision: that of loc."""
    dtype = loc.dtype
    D = ref.num_params(F, H)
    scale = softplus(u)
    rows = rows.to(dtype)
    row_ids = np.asarray(row_ids)
    acc = torch.zeros(len(rows), dtype=dtype)
    probs, hits = [], []
    for k in range(S):
        theta = loc + scale * pred_noise(seed, q, k, D, dtype)
        W1, b1, W2, b2 = ref.unpack(theta, F, H)
        o = (rows @ W1.T + b1) @ W2.T + b2
        pr = torch.sigmoid(o[:, 1] - o[:, 0])
        acc = acc + pr
        if want_draws:
            un = obs_uniforms(seed, q, k, int(row_ids.max()) + 1)[row_ids]
            probs.append(pr)
            hits.append(un < pr.double())
    return acc / S, (torch.stack(probs) if want_draws else None), (torch.stack(hits) if want_draws else None)


def grid_entries(grid=None):
    """sklearn's ParameterGrid order: keys sorted, the last key varying fastest."""
    import itertools
    grid = PARAM_GRID if grid is None else grid
    keys = sorted(grid)
    return [dict(zip(keys, values)) for values in itertools.product(*(grid[k] for k in keys))]


def select(cv_prob, folds, cls, n_splits):
    """GridSearchCV's ranking from cv_prob [NC, n] (every row's probability from the fit that held it out): a fold's score is the share of its rows with
    (prob > 0.5) == class in f64, a candidate's score the mean over the folds, the best the FIRST maximum.  Returns (mean [NC], best)."""
    cv_prob, folds, cls = np.asarray(cv_prob, dtype=np.float64), np.asarray(folds), np.asarray(cls, dtype=bool)
    right = (cv_prob > 0.5) == cls[None, :]
    scores = np.stack([right[:, folds == s].sum(1) / float((folds == s).sum()) for s in range(n_splits)], 1)
    mean = scores.mean(1)
    return mean, int(np.argmax(mean))


def pipeline(x, y, test_x, folds, n_splits, cands, loc0_of, num_steps, S, seed=0, problem_id=0, dtype=torch.float64, init_scale=0.1):
    """Every fit of one problem's grid search: cands [(H, lr)], loc0_of(c, D) -> [6, D] f32 initial locs of candidate c's slots.  Returns (cv_prob [NC, n],
    test_prob [NC, T]) in dtype."""
    x, y, test_x = (torch.as_tensor(np.asarray(v)) for v in (x, y, test_x))
    n, F = x.shape
    folds = np.asarray(folds)
    cv_prob, test_prob = torch.zeros(len(cands), n, dtype=dtype), torch.zeros(len(cands), len(test_x), dtype=dtype)
    for c, (H, lr) in enumerate(cands):
        D = ref.num_params(F, H)
        loc0 = loc0_of(c, D)
        for s in range(n_splits + 1):
            state = torch.zeros(6, D, dtype=dtype)
            state[0] = loc0[s].to(dtype)
            state[1] = float(np.float32(math.log(math.expm1(init_scale))))
            q = stream(problem_id, s)
            state, _ = run(state, x, y, row_mask(folds, s, n_splits), F, H, lr, q, seed, 0, num_steps, dtype=dtype)
            if s < n_splits:
                held = np.flatnonzero(folds == s)
                cv_prob[c, held] = predictive(state[0], state[1], x[held], held, F, H, S, q, seed)[0]
            else:
                test_prob[c] = predictive(state[0], state[1], test_x, n + np.arange(len(test_x)), F, H, S, q, seed)[0]
    return cv_prob, test_prob
