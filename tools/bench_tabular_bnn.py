"""The tabular study's BNN-classifier arm on the device.

    python tools/bench_tabular_bnn.py [--out profiles/r20_tabular_bnn.json] [--torch-positions 80]

bptt 100, eval positions 10 / 20 / 40 / 80, 20 windows of a 60-feature table (the shapes of tools/bench_tabular_logistic.py): 20 x 8 x 6 = 960 fits of 400 steps and
400 predictive draws per position.
bayes_batched     tabular.evaluate_position(bayes_net_metric): one TRAIN_ONLY window launch, the folds and the starts (median of 15 draws) on the host, ONE
                  pfn_bnn_cv launch, the scores on the host, one pfn_auc_counts launch; reported per call and per window
kernel            the pfn_bnn_cv launch alone (400 steps + 400 draws) on the same windows from a fresh state, inputs resident, device-synchronised
kernel_steps      the same without the predictive: (kernel - kernel_steps) / kernel is the predictive's share
kernel_quarter    the same as kernel on the first 5 windows (240 fits): a launch whose time does not fall with the number of fits is bound by the serial chain
                  of one block's step (latency), one that falls in proportion by throughput
torch_adam        the same fits written with torch autograd + torch.optim.Adam on the GPU (all fits of one candidate batched, the eight candidates in turn,
                  the same Philox-free torch.randn noise): timed ONCE at --torch-positions, for scale only.
There is no earlier implementation of this arm in this package: no ratio against a parent is claimed.

The one shape that pfn_bnn_svi_steps and pfn_bnn_cv can both run -- F 8, H 64, one particle, 100 rows -- is timed for 400 steps, alternated in the same rounds:
svi_100 is pfn_bnn_svi_steps on 100 problems, cv_102 is pfn_bnn_cv on 17 problems x 6 slots = 102 fits (slots 0 .. 4 train on four fifths of the rows).

Counted from the shapes (per fit and step, `counts`): the bytes of state streamed, the multiply-adds of the four products, the transcendental calls.
Protocol: wall-clock time of whole calls, the device synchronised at both ends; every variant is warmed up, the variants alternate for REPS rounds; the figure is
the median round, the spread (max - min) / median.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def counts(n, F, H):
    """Per fit and step, from the shapes: bytes of state the block streams (loc and u read for theta, six rows read and written by the update), multiply-adds of
    W1^T v, X w, X^T g and W1 r, transcendental calls (normal4 per four coordinates: 2 log, 2 sqrt, 2 sincos; per coordinate: softplus twice, sigmoid, log scale,
    two Adam updates with a sqrt and two divisions each; per row: exp, log1p, a division)."""
    D = H * (F + 3) + 2
    return dict(D=D, state_bytes=14 * D * 4, mac=2 * H * F + 2 * n * F, transcendental=(D + 3) // 4 * 6 + D * 12 + n * 3)


def torch_fits(train, labels, fold, n_splits, H, lr, steps):
    """All W x (n_splits + 1) fits of one candidate as one batched autograd graph: loc, u [B, D]; for scale only (torch.randn noise)."""
    W, n, F = train.shape
    S = n_splits + 1
    mask = torch.stack([torch.ones_like(fold, dtype=torch.bool) if s == n_splits else fold != s for s in range(S)], 1).float().reshape(W * S, n)
    x = train[:, None].expand(W, S, n, F).reshape(W * S, n, F)
    y = (labels > 0.5).float()[:, None].expand(W, S, n).reshape(W * S, n)
    D = H * (F + 3) + 2
    loc = torch.zeros(W * S, D, device=train.device, requires_grad=True)
    u = torch.full((W * S, D), float(np.log(np.expm1(0.1))), device=train.device, requires_grad=True)
    opt = torch.optim.Adam([loc, u], lr=lr)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        eps = torch.randn_like(loc)
        scale = torch.nn.functional.softplus(u)
        th = loc + scale * eps
        W1, b1 = th[:, :H * F].reshape(-1, H, F), th[:, H * F:H * F + H]
        W2, b2 = th[:, H * F + H:H * F + 3 * H].reshape(-1, 2, H), th[:, H * F + 3 * H:]
        o = torch.einsum('bnh,bch->bnc', torch.einsum('bnf,bhf->bnh', x, W1) + b1[:, None], W2) + b2[:, None]
        d = o[..., 1] - o[..., 0]
        nll = (mask * torch.nn.functional.softplus(torch.where(y > 0.5, -d, d))).sum(1)
        loss = (0.5 * (th * th).sum(1) + nll - (torch.log(scale) + 0.5 * eps * eps).sum(1)).sum()
        loss.backward()
        opt.step()
    return loc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--torch-positions', default='80')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_tabular_bnn: no GPU -- nothing is measured without one')
    torch_positions = {int(v) for v in a.torch_positions.split(',') if v}
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(1)
    N = BPTT + 3 * WINDOWS
    X = (torch.randn(N, FEATURES, generator=g) * (0.5 + torch.rand(FEATURES, generator=g)) + torch.randn(FEATURES, generator=g)).to(dev)
    w = torch.randn(FEATURES, generator=g).to(dev)
    y = ((X - X.mean(0)) @ w + torch.randn(N, generator=g).to(dev) > 0).float()
    starts = tabular.select_windows(N, BPTT, WINDOWS).tolist()
    entries, cands, num_steps, num_draws = tabular._bayes_grid()
    cand_H, cand_lr = [h for h, _ in cands], [lr for _, lr in cands]
    res = dict(bptt=BPTT, windows=WINDOWS, features=FEATURES, candidates=cands, num_steps=num_steps, num_draws=num_draws, reps=REPS,
               device=torch.cuda.get_device_name(0), positions={})
    for sep in POSITIONS:
        T = BPTT - sep
        keep = {}
        x_w, y_w = hipops.tabular_windows(X, y, starts, BPTT, sep, mode=hipops.TAB_NORM_TRAIN_ONLY)
        n_splits, _, _, operands = tabular._fold_problems(x_w[:sep], y_w[:sep], x_w[sep:])
        quarter = tuple(t[:WINDOWS // 4].contiguous() for t in operands)
        state0 = hipops.bnn_cv_state(WINDOWS, cand_H, FEATURES, dev)
        state0[:, :, :, 0] = torch.randn(state0[:, :, :, 0].shape, generator=torch.Generator().manual_seed(2)).to(dev) * 0.3
        fresh = {}

        def bayes_batched():
            keep['batched'] = tabular.evaluate_position(X, y, [], tabular.bayes_net_metric, BPTT, sep, max_samples=WINDOWS)

        def kernel():
            keep['kernel'] = hipops.bnn_cv(*operands, n_splits, cand_H, cand_lr, fresh['s'], num_steps, num_pred_samples=num_draws)

        def kernel_steps():
            hipops.bnn_cv(*operands, n_splits, cand_H, cand_lr, fresh['s'], num_steps)

        def kernel_quarter():
            hipops.bnn_cv(*quarter, n_splits, cand_H, cand_lr, fresh['q'], num_steps, num_pred_samples=num_draws)

        variants = dict(bayes_batched=bayes_batched, kernel=kernel, kernel_steps=kernel_steps, kernel_quarter=kernel_quarter)
        times = {name: [] for name in variants}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for rep in range(REPS + 1):      # round 0 warms every variant up
                for name, fn in variants.items():
                    fresh['s'], fresh['q'] = state0.clone(), state0[:WINDOWS // 4].clone()      # outside the timed window
                    t = wall(fn)
                    if rep:
                        times[name].append(t)
        fits = WINDOWS * len(cands) * (n_splits + 1)
        pos = dict(train_rows=sep, test_rows_per_window=T, n_splits=n_splits, fits=fits, variants={})
        for name, ts in times.items():
            med = statistics.median(ts)
            pos['variants'][name] = dict(median_ms=med * 1e3, min_ms=min(ts) * 1e3, max_ms=max(ts) * 1e3, spread=(max(ts) - min(ts)) / med)
        v = pos['variants']
        pos['ms_per_evaluate_position'] = v['bayes_batched']['median_ms']
        pos['ms_per_window'] = v['bayes_batched']['median_ms'] / WINDOWS
        pos['us_per_step_of_all_fits'] = v['kernel_steps']['median_ms'] * 1e3 / num_steps
        pos['predictive_share_of_kernel'] = (v['kernel']['median_ms'] - v['kernel_steps']['median_ms']) / v['kernel']['median_ms']
        pos['quarter_over_full'] = v['kernel_quarter']['median_ms'] / v['kernel']['median_ms']
        per = [counts(sep, FEATURES, h) for h in cand_H]
        step_bytes = WINDOWS * (n_splits + 1) * sum(c['state_bytes'] for c in per)
        pos['counts_per_fit_step_by_candidate'] = per
        pos['state_bytes_per_step_all_fits'] = step_bytes
        pos['achieved_state_GB_per_s'] = step_bytes / (pos['us_per_step_of_all_fits'] * 1e-6) / 1e9
        pos['status_done'] = int((keep['kernel'].status == hipops.BNN_CV_DONE).sum())
        pos['mean_auc'] = float(np.nanmean(keep['batched'][0]))
        if sep in torch_positions:
            def torch_adam():
                for h, lr in cands:
                    torch_fits(operands[0], operands[1], operands[3], n_splits, h, lr, num_steps)
            torch_fits(operands[0], operands[1], operands[3], n_splits, 5, 1e-3, 3)      # warm-up
            pos['torch_adam_ms_timed_once'] = wall(torch_adam) * 1e3
        else:
            pos['torch_adam_ms_timed_once'] = 'not measured'
        res['positions'][str(sep)] = pos

    # the one shape both step kernels run: F 8, H 64, one particle, 100 rows
    F, H, rows, steps = 8, 64, 100, 400
    g = torch.Generator().manual_seed(3)
    xs, ys = torch.randn(100, rows, F, generator=g).to(dev), (torch.rand(100, rows, generator=g) > 0.5).float().to(dev)
    fold = (torch.arange(rows, dtype=torch.int32) % 5)[None].expand(17, rows).contiguous().to(dev)
    cv_ops = (xs[:17].contiguous(), ys[:17].contiguous(), xs[:17, :4].contiguous(), fold)
    both = {}

    def svi_100():
        hipops.bnn_svi_steps(xs, ys, both['svi'], H, steps, num_particles=1, lr=1e-3)

    def cv_102():
        hipops.bnn_cv(*cv_ops, 5, [H], [1e-3], both['cv'], steps)

    times = dict(svi_100=[], cv_102=[])
    for rep in range(REPS + 1):
        for name, fn in (('svi_100', svi_100), ('cv_102', cv_102)):
            both['svi'], both['cv'] = hipops.bnn_svi_state(100, F, H, dev), hipops.bnn_cv_state(17, [H], F, dev)
            t = wall(fn)
            if rep:
                times[name].append(t)
    shared = dict(F=F, H=H, rows=rows, steps=steps)
    for name, ts in times.items():
        med = statistics.median(ts)
        shared[name] = dict(median_ms=med * 1e3, min_ms=min(ts) * 1e3, max_ms=max(ts) * 1e3, spread=(max(ts) - min(ts)) / med, us_per_step=med * 1e6 / steps)
    res['shared_shape'] = shared
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
