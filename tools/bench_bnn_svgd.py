"""SVGD on the BNN on the device: seconds per step of the persistent launch, what persistence buys, and the same step written with torch autograd.

    python tools/bench_bnn_svgd.py [--out profiles/r15_bnn_svgd.json]

A step is (potential gradient of N particles -> per-coordinate median bandwidth -> Stein direction -> Adam on every particle) for every one of the P problems.
Timed per shape, in alternating windows of the same run:

persistent      hipops.bnn_svgd_steps with num_steps = STEPS: ONE launch of pfn_bnn_svgd_steps runs the whole loop, one block per problem
per_step        the same kernel at one step per launch, STEPS launches (step0 = 0 .. STEPS - 1): the same arithmetic, bit for bit, with the state going through
                global memory and a launch boundary between steps
autograd        the same step written with torch on the device: the batched potential by einsum / log_softmax, its gradient by autograd, the pairwise squared
                differences [P, N (N - 1) / 2, D] and torch.median for the bandwidth, the kernel matrix [P, N, N, D] for the direction, and torch.optim.Adam
                with .grad set to it -- what a user would write today; AUTOGRAD_STEPS steps per window

Shapes: 100 problems x 100 rows, N = 50 particles, at (F 3, H 5) -- the reference's 'small' spec, D = 32, the state resident in LDS -- and the 'big' spec
(F 8, H 64), D = 706, the state tiled through LDS.  Protocol: warm-up, then REPS rounds of the windows (device events around a window, synchronised); the figure
is the median window divided by its steps (a window repeats its variant RUNS times, the state copied back to the start each time), the spread is
(max - min) / median.  There is no parent implementation, so no ratio to one is formed; the per_step and autograd columns are comparisons inside one run.
Needs a GPU."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformerscandobayesianinference_amd import hipops  # noqa: E402

REPS = 5
STEPS = 256
AUTOGRAD_STEPS = 16
RUNS = dict(persistent=4, per_step=2, autograd=2)      # repetitions inside a window: a window lasts a tenth of a second or more at every shape
P, N_ROWS, N_PARTICLES = 100, 100, 50
SPECS = [(3, 5), (8, 64)]      # F, H
LR = 1e-3


def autograd_step(x, y, F, H, particles):
    """One SVGD step on particles [P, N, D] (a leaf tensor with an Adam over it) with torch ops on the device: returns the step function."""
    n, N = x.shape[1], particles.shape[1]
    cls = (y > 0.5).long()[:, None, :, None].expand(P, N, n, 1)
    opt = torch.optim.Adam([particles], lr=LR)
    iu, ju = torch.triu_indices(N, N, 1, device=x.device)
    log_n1 = math.log(N + 1)

    def step():
        v = particles.detach().requires_grad_(True)
        W1, b1 = v[..., :H * F].reshape(P, N, H, F), v[..., H * F:H * F + H]
        W2, b2 = v[..., H * F + H:H * F + 3 * H].reshape(P, N, 2, H), v[..., H * F + 3 * H:]
        h = torch.einsum('pnf,pkhf->pknh', x, W1) + b1[:, :, None, :]
        o = torch.einsum('pknh,pkch->pknc', h, W2) + b2[:, :, None, :]
        U = 0.5 * (v * v).sum(-1) - torch.log_softmax(o, -1).gather(3, cls).sum((2, 3))      # [P, N]
        g, = torch.autograd.grad(U.sum(), v)
        with torch.no_grad():
            xd = v.detach()
            bw = torch.median((xd[:, iu] - xd[:, ju]) ** 2, 1).values / log_n1      # [P, D]
            diff = xd[:, :, None, :] - xd[:, None, :, :]      # [P, n, m, D] = x_n - x_m
            bw = bw[:, None, None, :]
            k = torch.exp(-diff * diff / bw)
            s = (k * (g[:, None, :, :] - 2. * diff / bw)).mean(2)
        opt.zero_grad(set_to_none=True)
        particles.grad = s
        opt.step()
        return U.detach().mean(1)
    return step


def bench_shape(F, H, dev):
    g = torch.Generator().manual_seed(F + H)
    D = hipops.bnn_num_params(F, H)
    x = torch.randn(P, N_ROWS, F, generator=g).to(dev)
    # y from the model itself at weights drawn from the prior, so the posterior is a sensible one
    w = torch.randn(P, D, generator=g).to(dev)
    y = (torch.rand(P, N_ROWS, generator=g).to(dev) < hipops.bnn_predict(x, w, H, K=1)).float().contiguous()
    start = torch.randn(15, P, N_PARTICLES, D, generator=g).median(0).values      # fit_bnn_svgd's start
    state0 = hipops.bnn_svgd_state(P, N_PARTICLES, F, H, dev, particles0=start)
    state = state0.clone()
    pot = torch.empty(P, STEPS, device=dev)
    pot1 = torch.empty(P, 1, device=dev)
    bw = torch.zeros(P, D, device=dev)
    particles = state0[:, 0].clone().requires_grad_(True)
    slow = autograd_step(x, y, F, H, particles)

    def persistent():
        state.copy_(state0)
        hipops.bnn_svgd_steps(x, y, state, H, STEPS, lr=LR, potential=pot, bandwidth=bw)

    def per_step():
        state.copy_(state0)
        for t in range(STEPS):
            hipops.bnn_svgd_steps(x, y, state, H, 1, step0=t, lr=LR, potential=pot1, bandwidth=bw)

    def autograd():
        for _ in range(AUTOGRAD_STEPS):
            slow()

    def window(fn, steps, runs):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        begin.record()
        for _ in range(runs):
            fn()
        end.record()
        torch.cuda.synchronize()
        return begin.elapsed_time(end) * 1e-3 / (steps * runs)

    variants = {'persistent': (persistent, STEPS, RUNS['persistent']), 'per_step': (per_step, STEPS, RUNS['per_step']), 'autograd': (autograd, AUTOGRAD_STEPS, RUNS['autograd'])}
    persistent()
    whole = state.clone()
    per_step()
    torch.cuda.synchronize()
    same_bits = bool(torch.equal(whole, state))      # a run split into single steps is the same run
    first, last = float(pot[:, :20].mean()), float(pot[:, -20:].mean())
    # the torch step is the kernel's step: one step of each from the same start
    one = state0.clone()
    hipops.bnn_svgd_steps(x, y, one, H, 1, lr=LR, potential=pot1, bandwidth=bw)
    ref = state0[:, 0].clone().requires_grad_(True)
    autograd_step(x, y, F, H, ref)()
    torch_step_rel = float(((one[:, 0] - ref.detach()).norm() / (ref.detach() - state0[:, 0]).norm()))      # relative to the length of the step
    for fn, steps, _ in variants.values():
        window(fn, steps, 1)
    times = {name: [] for name in variants}
    for _ in range(REPS):
        for name, (fn, steps, runs) in variants.items():
            times[name].append(window(fn, steps, runs))
    res = dict(shape=dict(P=P, n=N_ROWS, F=F, H=H, D=D, N=N_PARTICLES),
               steps_per_window=dict(persistent=STEPS * RUNS['persistent'], per_step=STEPS * RUNS['per_step'], autograd=AUTOGRAD_STEPS * RUNS['autograd']),
               per_step_launches_give_the_bits_of_the_persistent_launch=same_bits, first_step_of_the_torch_version_vs_the_kernel_relative_to_the_step=torch_step_rel,
               mean_potential_first_20_steps=first, mean_potential_last_20_steps=last, variants={})
    for name, ts in times.items():
        med = statistics.median(ts)
        res['variants'][name] = dict(median_us_per_step=med * 1e6, min_us_per_step=min(ts) * 1e6, max_us_per_step=max(ts) * 1e6, spread=(max(ts) - min(ts)) / med)
    res['steps_per_second'] = 1. / statistics.median(times['persistent'])
    res['problem_steps_per_second'] = P / statistics.median(times['persistent'])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'r15_bnn_svgd.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_bnn_svgd: no GPU -- nothing is measured without one')
    dev = 'cuda:0'
    res = dict(device=torch.cuda.get_device_name(0), reps=REPS, lr=LR, shapes=[bench_shape(F, H, dev) for F, H in SPECS])
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
    json.dump(res, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
