"""The MAP-II objective and gradient on the device against the composition it replaces, on the same data and the same GPU.

    python tools/bench_gp_fit.py [--out profiles/r11_gp_fit.json] [--kernel-stats kernel_stats.csv]

fused      hipops.gp_mll_grad (pfn_gp_mll_grad: masked Gram, blocked Cholesky, L^-1, K^-1, the fused gradient reduction)
composed   torch f32 on the device: Gram (Matern-5/2 ARD from |a|^2 + |b|^2 - 2 a.b, as gpytorch forms it), torch.linalg.cholesky, the same objective,
           autograd for the gradient
fit        priors.fast_gp_mix.batched_lbfgs for a fixed number of passes, driven by either of the two

Shapes: P = 512, S = 64, F = 18 and P = 16, S = 2000, F = 18.  Protocol: every variant is warmed up, then timed in windows (device events around the
window, synchronised); the windows of the variants alternate, REPS rounds; the figure is the median window, the spread is (max - min) / median.  If the
composed path runs out of memory at a shape, that is what is recorded.  --kernel-stats: the CSV of a `rocprofv3 --kernel-trace --stats` run of
tools/bench_gp_fit.py --trace (one shape, a few calls, nothing timed), from which the gradient kernel's own time and its achieved bytes/s against the
one-read-of-K^-1 floor (4 S^2 P bytes) are taken.  Needs a GPU."""
import argparse
import csv
import json
import math
import os
import re
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformerscandobayesianinference_amd import hipops  # noqa: E402
from transformerscandobayesianinference_amd.priors import fast_gp_mix  # noqa: E402

REPS = 7
WINDOW_S = 0.3
HP = {'outputscale_concentration': 2.}
SHAPES = [(512, 64, 18), (16, 2000, 18)]
FIT_PASSES = 20


def window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e-3 / iters


def composed_objective(theta, x, y, prior):
    F = x.shape[-1]
    n = x.shape[1]
    ls, os_, noise, c = theta[:, :F].exp(), theta[:, F].exp(), theta[:, F + 1].exp() + prior[6], theta[:, F + 2]
    xs = x / ls[:, None, :]
    sq = (xs * xs).sum(-1)
    d2 = (sq[:, :, None] + sq[:, None, :] - 2 * xs @ xs.transpose(1, 2)).clamp_min(1e-30)
    s = (5 * d2).sqrt()
    K = os_[:, None, None] * ((1 + s + s * s / 3) * torch.exp(-s)) + noise[:, None, None] * torch.eye(n, device=x.device)
    L = torch.linalg.cholesky(K)
    w = torch.linalg.solve_triangular(L, (y - c[:, None])[:, :, None], upper=False)[:, :, 0]
    ll = -0.5 * (w * w).sum(1) - torch.diagonal(L, dim1=1, dim2=2).log().sum(1) - 0.5 * n * math.log(2 * math.pi)

    def lg(v, a, b):
        return a * torch.log(b) - torch.lgamma(a) + (a - 1) * torch.log(v) - b * v
    lp = lg(ls, prior[0], prior[1]).sum(1) + lg(os_, prior[2], prior[3]) + lg(noise, prior[4], prior[5])
    return -(ll + lp) / n


def make(P, S, F, dev):
    g = torch.Generator().manual_seed(P + S)
    x = torch.rand(P, S, F, generator=g).to(dev)
    y = torch.randn(P, S, generator=g).to(dev)
    return x, y, fast_gp_mix.default_theta(P, F, HP, dev), fast_gp_mix.hyperprior_vector(HP, dev)


def bench_shape(P, S, F, dev):
    x, y, theta, prior = make(P, S, F, dev)
    ws = hipops.gp_fit_workspace(P, S, dev)

    def fused(t=theta):
        v, g, _ = hipops.gp_mll_grad(x, y, t.contiguous(), prior, 1, ws=ws)
        return v, g

    def fused_value():
        hipops.gp_mll_grad(x, y, theta, prior, 1, ws=ws, want_grad=False)

    def composed(t=theta):
        t = t.detach().requires_grad_(True)
        with torch.enable_grad():
            J = composed_objective(t, x, y, prior)
            g, = torch.autograd.grad(J.sum(), t)
        return J.detach(), g

    def fit_with(fun):
        return lambda: fast_gp_mix.batched_lbfgs(fun, theta, max_iter=FIT_PASSES, gtol=0., ftol=0., sync_every=10 ** 9)

    res = dict(shape=dict(P=P, S=S, F=F), kernel='matern52', variants={})
    variants = dict(fused_value_and_grad=fused, fused_value_only=fused_value, fused_fit=fit_with(fused))
    try:
        vc, gc = composed()
        vf, gf = fused()
        res['agreement'] = dict(value_max_rel=float(((vc - vf).abs() / vc.abs()).max()), grad_max_rel_inf=float(((gc - gf).abs().amax(1) / gc.abs().amax(1)).max()))
        variants.update(composed_value_and_grad=composed, composed_fit=fit_with(composed))
        res['composed_peak_bytes'] = int(torch.cuda.max_memory_allocated())
    except torch.OutOfMemoryError as e:
        res['composed'] = 'out of memory: ' + str(e)[:200]
    iters = {}
    for name, fn in variants.items():
        for _ in range(2):
            fn()
        iters[name] = max(2, int(WINDOW_S / max(window(fn, 2), 1e-7)))
    times = {name: [] for name in variants}
    for _ in range(REPS):
        for name, fn in variants.items():
            times[name].append(window(fn, iters[name]))
    for name, ts in times.items():
        med = statistics.median(ts)
        res['variants'][name] = dict(median_ms=med * 1e3, min_ms=min(ts) * 1e3, max_ms=max(ts) * 1e3, spread=(max(ts) - min(ts)) / med, iters_per_window=iters[name])
    V = res['variants']
    if 'composed_value_and_grad' in V:
        res['composed_over_fused_call'] = V['composed_value_and_grad']['median_ms'] / V['fused_value_and_grad']['median_ms']
        res['composed_over_fused_fit'] = V['composed_fit']['median_ms'] / V['fused_fit']['median_ms']
    res['fit_passes'] = FIT_PASSES
    res['kinv_floor_bytes'] = 4 * S * S * P
    return res


def trace(dev):
    """A few calls at the large shape and nothing else: the workload of a `rocprofv3 --kernel-trace --stats` run."""
    P, S, F = SHAPES[1]
    x, y, theta, prior = make(P, S, F, dev)
    ws = hipops.gp_fit_workspace(P, S, dev)
    for _ in range(5):
        hipops.gp_mll_grad(x, y, theta, prior, 1, ws=ws)
    torch.cuda.synchronize()


def kernel_stats(path, floor_bytes):
    rows = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r'\b(gpfit_[a-z]+_kernel|gp_[a-z_]+_kernel)\b', r.get('Name') or r.get('KernelName') or '')
        if m:
            name = m.group(1)
            rows[name] = dict(calls=int(r['Calls']), average_us=float(r['AverageNs']) * 1e-3, total_ms=float(r['TotalDurationNs']) * 1e-6)
    out = dict(kernels=rows)
    for name, v in rows.items():
        if 'gpfit_grad_kernel' in name:
            out['grad_kernel_achieved_GBps_against_one_read_of_Kinv'] = floor_bytes / (v['average_us'] * 1e-6) * 1e-9
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--kernel-stats', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_gp_fit: no GPU -- nothing is measured without one')
    dev = 'cuda:0'
    if a.trace:
        return trace(dev)
    res = dict(device=torch.cuda.get_device_name(0), reps=REPS, shapes=[bench_shape(P, S, F, dev) for P, S, F in SHAPES])
    if a.kernel_stats:
        P, S, F = SHAPES[1]
        res['kernel_trace_P16_S2000'] = kernel_stats(a.kernel_stats, 4 * S * S * P)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
