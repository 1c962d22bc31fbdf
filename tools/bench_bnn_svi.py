"""SVI on the BNN on the device: seconds per step of the persistent launch, what persistence buys, and the same step written with torch autograd.

    python tools/bench_bnn_svi.py [--out profiles/r14_bnn_svi.json]

A step is (draw noise -> ELBO gradient over K particles -> Adam on loc and u) for every one of the P guides.  Timed per shape, in alternating windows of the
same run:

persistent      hipops.bnn_svi_steps with num_steps = STEPS: ONE launch of pfn_bnn_svi_steps runs the whole loop, one block per problem
per_step        the same kernel at one step per launch, STEPS launches (step0 = 0 .. STEPS - 1): the same arithmetic, bit for bit, with the state going through
                global memory and a launch boundary between steps
autograd        the same step written with torch on the device: batched reparameterised particles, the potential by einsum / log_softmax, autograd, and
                torch.optim.Adam on (loc, u) -- what a user would write today, a few dozen launch-bound kernels per step; AUTOGRAD_STEPS steps per window

Shapes: 100 problems x 100 rows, K of {1, 8, 32} particles, at (F 3, H 5) -- the reference's 'small' spec, D = 32 --, (F 8, H 11), D = 123, and the 'big'
spec (F 8, H 64), D = 706.  Protocol: warm-up, then REPS rounds of the windows (device events around a window, synchronised); the figure is the median
window divided by its steps (a window repeats its variant RUNS times, the state copied back to the start each time), the spread is (max - min) / median.  There is no parent implementation, so no ratio to one is formed; the per_step and
autograd columns are comparisons inside one run.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformerscandobayesianinference_amd import hipops  # noqa: E402

REPS = 5
STEPS = 1024
AUTOGRAD_STEPS = 64
RUNS = dict(persistent=8, per_step=4, autograd=2)      # repetitions inside a window: a window lasts a tenth of a second or more at every shape
P, N_ROWS = 100, 100
SPECS = [(3, 5), (8, 11), (8, 64)]      # F, H
PARTICLES = [1, 8, 32]
LR = 1e-3


def autograd_step(x, y, K, F, H, loc, u):
    """One SVI step on (loc, u) [P, D] (leaf tensors with an Adam over them) with torch ops on the device: returns the step function."""
    n = x.shape[1]
    D = hipops.bnn_num_params(F, H)
    cls = (y > 0.5).long()[:, None, :, None].expand(P, K, n, 1)
    opt = torch.optim.Adam([loc, u], lr=LR)

    def step():
        opt.zero_grad(set_to_none=True)
        scale = torch.nn.functional.softplus(u)
        eps = torch.randn(P, K, D, device=x.device)
        v = loc[:, None, :] + scale[:, None, :] * eps
        W1, b1 = v[..., :H * F].reshape(P, K, H, F), v[..., H * F:H * F + H]
        W2, b2 = v[..., H * F + H:H * F + 3 * H].reshape(P, K, 2, H), v[..., H * F + 3 * H:]
        h = torch.einsum('pnf,pkhf->pknh', x, W1) + b1[:, :, None, :]
        o = torch.einsum('pknh,pkch->pknc', h, W2) + b2[:, :, None, :]
        U = 0.5 * (v * v).sum(-1) - torch.log_softmax(o, -1).gather(3, cls).sum((2, 3))
        loss = (U - 0.5 * (eps * eps).sum(-1)).mean(1) - torch.log(scale).sum(-1)      # [P]; (D / 2) log 2 pi of U and of the entropy cancel
        loss.sum().backward()
        opt.step()
        return loss.detach()
    return step


def bench_shape(F, H, K, dev):
    g = torch.Generator().manual_seed(F + H + K)
    D = hipops.bnn_num_params(F, H)
    x = torch.randn(P, N_ROWS, F, generator=g).to(dev)
    # y from the model itself at weights drawn from the prior, so the posterior is a sensible one
    w = torch.randn(P, D, generator=g).to(dev)
    y = (torch.rand(P, N_ROWS, generator=g).to(dev) < hipops.bnn_predict(x, w, H, K=1)).float().contiguous()
    loc0 = torch.randn(P, D, generator=g).to(dev)
    state0 = hipops.bnn_svi_state(P, F, H, dev, loc0=loc0)
    state = state0.clone()
    loss = torch.empty(P, STEPS, device=dev)
    loss1 = torch.empty(P, 1, device=dev)
    loc, u = state0[:, 0].clone().requires_grad_(True), state0[:, 1].clone().requires_grad_(True)
    slow = autograd_step(x, y, K, F, H, loc, u)

    def persistent():
        state.copy_(state0)
        hipops.bnn_svi_steps(x, y, state, H, STEPS, num_particles=K, lr=LR, seed=1, loss=loss)

    def per_step():
        state.copy_(state0)
        for t in range(STEPS):
            hipops.bnn_svi_steps(x, y, state, H, 1, step0=t, num_particles=K, lr=LR, seed=1, loss=loss1)

    def autograd():
        for _ in range(AUTOGRAD_STEPS):
            slow()

    def window(fn, steps, runs):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(runs):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) * 1e-3 / (steps * runs)

    variants = {'persistent': (persistent, STEPS, RUNS['persistent']), 'per_step': (per_step, STEPS, RUNS['per_step']), 'autograd': (autograd, AUTOGRAD_STEPS, RUNS['autograd'])}
    persistent()
    whole = state.clone()
    per_step()
    torch.cuda.synchronize()
    same_bits = bool(torch.equal(whole, state))      # a run split into single steps is the same run
    first, last = float(loss[:, :20].mean()), float(loss[:, -20:].mean())
    for fn, steps, _ in variants.values():
        window(fn, steps, 1)
    times = {name: [] for name in variants}
    for _ in range(REPS):
        for name, (fn, steps, runs) in variants.items():
            times[name].append(window(fn, steps, runs))
    res = dict(shape=dict(P=P, n=N_ROWS, F=F, H=H, D=D, K=K), steps_per_window=dict(persistent=STEPS * RUNS['persistent'], per_step=STEPS * RUNS['per_step'], autograd=AUTOGRAD_STEPS * RUNS['autograd']),
               per_step_launches_give_the_bits_of_the_persistent_launch=same_bits, mean_loss_first_20_steps=first, mean_loss_last_20_steps=last, variants={})
    for name, ts in times.items():
        med = statistics.median(ts)
        res['variants'][name] = dict(median_us_per_step=med * 1e6, min_us_per_step=min(ts) * 1e6, max_us_per_step=max(ts) * 1e6, spread=(max(ts) - min(ts)) / med)
    res['steps_per_second'] = 1. / statistics.median(times['persistent'])
    res['problem_steps_per_second'] = P / statistics.median(times['persistent'])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'r14_bnn_svi.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_bnn_svi: no GPU -- nothing is measured without one')
    dev = 'cuda:0'
    res = dict(device=torch.cuda.get_device_name(0), reps=REPS, lr=LR, shapes=[bench_shape(F, H, K, dev) for F, H in SPECS for K in PARTICLES])
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
    json.dump(res, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
