"""The batched NUTS on the BNN posterior on the device: passes per second, where a pass spends its time, and the same target written with torch autograd.

    python tools/bench_bnn_mcmc.py [--out profiles/r13_bnn_mcmc.json]

A pass is one evaluation of the potential at every chain's trial point (hipops.bnn_logp_grad: pfn_bnn_logp_grad, ONE launch) followed by one call of the
sampler's state machine (hipops.nuts_advance: pfn_nuts_advance).  Timed per shape, in alternating windows of the same run:

pass            the live loop: init, then PASSES x (bnn_logp_grad, nuts_advance) -- what mcmc.batched_nuts does between two looks at the done counter
advance         pfn_nuts_advance alone, replaying the values and gradients recorded in a first run (the state machine is deterministic)
gradient        pfn_bnn_logp_grad alone at the recorded trial points
autograd        the same potential and gradient of all chains written with torch on the device (batched matmuls, log_softmax, autograd.grad) at the recorded
                trial points: what a user would write today, a dozen launch-bound kernels per evaluation
pass_autograd   the live loop with that function in place of the kernel

Shapes: 100 problems x {1, 8} chains, n = 100 rows, at (F 3, H 5) -- the reference's "small" model, D = 32 -- and (F 8, H 11), D = 123, the largest hidden
width the sampler's D <= 128 admits at 8 features.  Protocol: warm-up, then REPS rounds of the windows (device events around a window, synchronised); the
figure is the median window, the spread is (max - min) / median.  There is no parent implementation, so no ratio to one is formed; the autograd column is a
comparison inside one run.  Needs a GPU."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformerscandobayesianinference_amd import _hip, hipops, mcmc  # noqa: E402

REPS = 7
PASSES = 256
SHAPES = [(100, 1, 100, 3, 5), (100, 8, 100, 3, 5), (100, 1, 100, 8, 11), (100, 8, 100, 8, 11)]      # P, K, n, F, H
WARMUP, DEPTH = 150, 10


def autograd_fun(x, y, K, F, H):
    """(theta [P K, D]) -> (value [P K], grad [P K, D]) with torch ops on the device."""
    P, n, _ = x.shape
    D = hipops.bnn_num_params(F, H)
    cls = (y > 0.5).long()[:, None, :, None].expand(P, K, n, 1)
    const = 0.5 * D * math.log(2. * math.pi)

    def fun(theta):
        with torch.enable_grad():
            t = theta.detach().requires_grad_(True)
            v = t.view(P, K, D)
            W1, b1 = v[..., :H * F].reshape(P, K, H, F), v[..., H * F:H * F + H]
            W2, b2 = v[..., H * F + H:H * F + 3 * H].reshape(P, K, 2, H), v[..., H * F + 3 * H:]
            h = torch.einsum('pnf,pkhf->pknh', x, W1) + b1[:, :, None, :]
            o = torch.einsum('pknh,pkch->pknc', h, W2) + b2[:, :, None, :]
            value = 0.5 * (v * v).sum(-1) + const - torch.log_softmax(o, -1).gather(3, cls).sum((2, 3))
            grad, = torch.autograd.grad(value.sum(), t)
        return value.detach().reshape(P * K), grad
    return fun


def bench_shape(P, K, n, F, H, dev):
    g = torch.Generator().manual_seed(P + K + H)
    x = torch.randn(P, n, F, generator=g).to(dev)
    D = hipops.bnn_num_params(F, H)
    C = P * K
    # y from the model itself at weights drawn from the prior, so the posterior is a sensible one
    w = torch.randn(P, D, generator=g).to(dev)
    y = (torch.rand(P, n, generator=g).to(dev) < hipops.bnn_predict(x, w, H, K=1)).float().contiguous()
    theta0 = torch.randn(C, D, generator=g).to(dev)
    ws = hipops.nuts_workspace(C, D, DEPTH, dev)
    windows = mcmc.adaptation_windows(WARMUP)
    trial = theta0.clone()
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    samples = torch.zeros(C, PASSES, D, device=dev)
    stats = torch.zeros(C, WARMUP + PASSES, 8, device=dev)
    value, gradient_buf = torch.empty(C, device=dev), torch.empty(C, D, device=dev)
    slow = autograd_fun(x, y, K, F, H)

    def init():
        trial.copy_(theta0)
        hipops.nuts_init(ws, theta0, D, DEPTH, WARMUP, PASSES, 0, trial, done, flags=_hip.NUTS_ADAPT_MASS, window_start=windows[0][0], window_ends=[e for _, e in windows])

    def grad(t):
        return hipops.bnn_logp_grad(x, y, t, H, K=K, value=value, grad=gradient_buf)

    def advance(v, gr):
        hipops.nuts_advance(ws, D, DEPTH, v, gr, trial, samples, stats, done)

    record = []
    init()
    for _ in range(PASSES):
        t = trial.clone()
        v, gr = grad(t)
        v, gr = v.clone(), gr.clone()
        record.append((t, v, gr))
        advance(v, gr)
    torch.cuda.synchronize()
    transitions = int((stats[:, :, 3] > 0).sum())
    leapfrogs = float(stats[:, :, 3].sum())
    # the two implementations of the target agree (f32 round-off of sums over 100 rows)
    v2, g2 = slow(record[-1][0])
    agree = dict(value=float(((v2 - record[-1][1]).abs() / record[-1][1].abs()).max()), grad=float(((g2 - record[-1][2]).norm(dim=1) / record[-1][2].norm(dim=1)).max()))

    def live():
        for _ in range(PASSES):
            advance(*grad(trial))

    def live_autograd():
        for _ in range(PASSES):
            advance(*slow(trial))

    def replay():
        for _, v, gr in record:
            advance(v, gr)

    def gradient():
        for t, _, _ in record:
            grad(t)

    def autograd():
        for t, _, _ in record:
            slow(t)

    def window(fn):
        init()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) * 1e-3 / PASSES

    variants = {'pass': live, 'advance': replay, 'gradient': gradient, 'autograd': autograd, 'pass_autograd': live_autograd}
    for fn in variants.values():
        window(fn)
    times = {name: [] for name in variants}
    for _ in range(REPS):
        for name, fn in variants.items():
            times[name].append(window(fn))
    res = dict(shape=dict(P=P, K=K, n=n, F=F, H=H, D=D), chains=C, passes_per_window=PASSES, finished_transitions_in_the_recorded_window=transitions,
               mean_leapfrogs_per_finished_transition=leapfrogs / max(1, transitions), kernel_against_autograd_at_the_last_recorded_point=agree, variants={})
    for name, ts in times.items():
        med = statistics.median(ts)
        res['variants'][name] = dict(median_us=med * 1e6, min_us=min(ts) * 1e6, max_us=max(ts) * 1e6, spread=(max(ts) - min(ts)) / med)
    res['passes_per_second'] = 1. / statistics.median(times['pass'])
    res['chain_leapfrogs_per_second'] = C / statistics.median(times['pass'])
    res['passes_per_second_autograd'] = 1. / statistics.median(times['pass_autograd'])
    res['chain_leapfrogs_per_second_autograd'] = C / statistics.median(times['pass_autograd'])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'r13_bnn_mcmc.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_bnn_mcmc: no GPU -- nothing is measured without one')
    dev = 'cuda:0'
    res = dict(device=torch.cuda.get_device_name(0), reps=REPS, warmup=WARMUP, max_tree_depth=DEPTH, shapes=[bench_shape(*s, dev) for s in SHAPES])
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
    json.dump(res, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
