"""The batched NUTS over GP hyper-parameters on the device: passes per second, and where a pass spends its time.

    python tools/bench_gp_mcmc.py [--out profiles/r12_gp_mcmc.json]

A pass is one evaluation of the potential at every chain's trial point (hipops.gp_mll_grad: pfn_gp_mll_grad) followed by one call of the sampler's state
machine (hipops.nuts_advance: pfn_nuts_advance).  Three things are timed per shape, in alternating windows of the same run:

pass       the live loop: init, then PASSES x (gp_mll_grad, nuts_advance) -- what mcmc.batched_nuts does between two looks at the done counter
advance    pfn_nuts_advance alone: the state is re-initialised and the SAME passes are replayed from the values and gradients recorded in a first run (the
           state machine is deterministic, so the replay takes exactly the branches of the live run: leaves, subtree ends, transition ends, adaptation)
gradient   pfn_gp_mll_grad alone at the recorded trial points

Shapes: P = 512 chains x S = 64 points x F = 18 and P = 16 x S = 2000 x F = 18 (one chain per problem).  Protocol: warm-up, then REPS rounds of the three
windows (device events around a window, synchronised); the figure is the median window, the spread is (max - min) / median.  There is no parent
implementation of the sampler to compare with, so no ratio is formed.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformerscandobayesianinference_amd import _hip, hipops, mcmc  # noqa: E402
from transformerscandobayesianinference_amd.priors import fast_gp_mix  # noqa: E402

REPS = 7
HP = {'outputscale_concentration': 2.}
SHAPES = [(512, 64, 18, 256), (16, 2000, 18, 48)]      # P, S, F, passes per window
WARMUP, DEPTH = 150, 10


def bench_shape(P, S, F, passes, dev):
    g = torch.Generator().manual_seed(P + S)
    x = torch.rand(P, S, F, generator=g).to(dev)
    prior = fast_gp_mix.hyperprior_vector(HP, dev)
    # y from the model itself at the default hyper-parameters, so the posterior is a sensible one
    ls, osc, nz = torch.full((P, F), 0.5, device=dev), torch.ones(P, device=dev), torch.full((P,), 0.1, device=dev)
    y = fast_gp_mix.fast_gp.gp_sample(P, S, F, dev, ls, osc, nz, 1, x=x, check='sync')[1].contiguous()
    theta0 = fast_gp_mix.default_theta(P, F, HP, dev)
    theta0[:, F + 2] = 0.
    D, ld = F + 2, F + 3
    n_of = torch.full((P,), S, dtype=torch.int32, device=dev)
    scale, shift = n_of.float(), torch.ones(D, device=dev)
    gws = hipops.gp_fit_workspace(P, S, dev)
    ws = hipops.nuts_workspace(P, D, DEPTH, dev)
    windows = mcmc.adaptation_windows(WARMUP)
    trial = theta0.clone()
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    samples = torch.zeros(P, passes, D, device=dev)
    stats = torch.zeros(P, WARMUP + passes, 8, device=dev)

    def init():
        trial.copy_(theta0)
        hipops.nuts_init(ws, theta0, D, DEPTH, WARMUP, passes, 0, trial, done, flags=_hip.NUTS_ADAPT_MASS, window_start=windows[0][0], window_ends=[e for _, e in windows])

    def grad(t):
        return hipops.gp_mll_grad(x, y, t, prior, 1, n_of=n_of, flags=1, ws=gws)

    def advance(v, gr, info):
        hipops.nuts_advance(ws, D, DEPTH, v, gr, trial, samples, stats, done, info=info, scale=scale, shift=shift)

    record = []
    init()
    for _ in range(passes):
        t = trial.clone()
        v, gr, info = grad(t)
        record.append((t, v, gr, info))
        advance(v, gr, info)
    torch.cuda.synchronize()
    transitions = int((stats[:, :, 3] > 0).sum())
    leapfrogs = float(stats[:, :, 3].sum())

    def live():
        for _ in range(passes):
            advance(*grad(trial))

    def replay():
        for _, v, gr, info in record:
            advance(v, gr, info)

    def gradient():
        for t, _, _, _ in record:
            grad(t)

    def window(fn):
        init()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) * 1e-3 / passes

    variants = {'pass': live, 'advance': replay, 'gradient': gradient}
    for fn in variants.values():
        window(fn)
    times = {name: [] for name in variants}
    for _ in range(REPS):
        for name, fn in variants.items():
            times[name].append(window(fn))
    res = dict(shape=dict(P=P, S=S, F=F), chains=P, passes_per_window=passes, finished_transitions_in_the_recorded_window=transitions,
               mean_leapfrogs_per_finished_transition=leapfrogs / max(1, transitions), variants={})
    for name, ts in times.items():
        med = statistics.median(ts)
        res['variants'][name] = dict(median_us=med * 1e6, min_us=min(ts) * 1e6, max_us=max(ts) * 1e6, spread=(max(ts) - min(ts)) / med)
    res['passes_per_second'] = 1. / statistics.median(times['pass'])
    res['chain_leapfrogs_per_second'] = P / statistics.median(times['pass'])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'r12_gp_mcmc.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_gp_mcmc: no GPU -- nothing is measured without one')
    dev = 'cuda:0'
    res = dict(device=torch.cuda.get_device_name(0), reps=REPS, warmup=WARMUP, max_tree_depth=DEPTH, shapes=[bench_shape(P, S, F, n, dev) for P, S, F, n in SHAPES])
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
    json.dump(res, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
