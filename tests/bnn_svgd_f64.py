"""f64 restatement of the SVGD step of csrc/bnn_svgd.hip, written from its contract (include/pfn_hip.h "SVGD on the BNN"), in torch on the CPU:

    g_n = grad U(x_n)                                                                   (U: tests/bnn_f64.py, batched over the particles)
    h_d = bandwidth_factor * median_{i<j} (x_id - x_jd)^2 / log(N + 1)                   (torch.median: the lower middle value, one of the pairwise values)
    k_d(n,m) = exp(-(x_nd - x_md)^2 / h_d),  s_nd = (1/N) sum_m [ k_d(n,m) g_md + k_d(n,m) 2 (x_md - x_nd) / h_d ]      (h a constant of the step)
    Adam: m <- b1 m + (1 - b1) s, v <- b2 v + (1 - b2) s^2, x <- x - lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps), t = step index + 1

There is no randomness inside a step.  The host tests (tests/test_host_bnn_svgd.py) check `bandwidth` against torch.median over explicit pairs, `stein_direction`
against a construction whose repulsive term is torch.autograd's, and `run` against torch.optim.Adam, before the GPU tests use this file as their oracle."""
import math

import numpy as np
import torch

import bnn_f64 as ref
from bnn_f64 import adam, f32, potentials      # noqa: F401  (shared with the other restatement; the tests reach them through this module)

ROWS = ('particles', 'm', 'v')
# The no-data case of the host and the GPU test: n = 0, so the target is the prior N(0, I) in every coordinate.  The start is fit_bnn_svgd's: every coordinate
# of every particle the median of 15 N(0, 1) draws (standard deviation about 0.32).
NO_DATA = dict(F=3, H=5, P=2, N=50, T=300, lr=0.05, seed=5)


def potentials_and_grads(theta, x, y, n, F, H, activation=0):
    """(U [N], grad U [N, D]) in f64, the gradient from autograd."""
    t = theta.detach().clone().requires_grad_(True)
    U = potentials(t, x, y, n, F, H, activation)
    g, = torch.autograd.grad(U.sum(), t)
    return U.detach(), g


def bandwidth(x, bandwidth_factor=1.0):
    """h [D] of particles x [N, D]."""
    N = x.shape[0]
    i, j = torch.triu_indices(N, N, 1)
    d2 = (x[i] - x[j]) ** 2      # [N (N - 1) / 2, D]
    return bandwidth_factor * torch.median(d2, 0).values / math.log(N + 1)


def stein_direction(x, g, h):
    """s [N, D] from particles x [N, D], their potential gradients g [N, D] and the bandwidth h [D]."""
    N = x.shape[0]
    diff = x[:, None, :] - x[None, :, :]      # [n, m, d] = x_nd - x_md
    k = torch.exp(-diff * diff / h)
    return (k * g[None, :, :] + k * 2. * (-diff) / h).sum(1) / N


def step_terms(particles, x, y, n, F, H, activation=0, bandwidth_factor=1.0):
    """(mean U, h [D], s [N, D]) of one step from particles [N, D] f64."""
    U, g = potentials_and_grads(particles, x, y, n, F, H, activation)
    h = bandwidth(particles, f32(bandwidth_factor))
    return float(U.mean()), h, stein_direction(particles, g, h)


def run(state, x, y, n, F, H, activation=0, step0=0, num_steps=1, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, bandwidth_factor=1.0):
    """`num_steps` steps from state [3, N, >= D] (row blocks ROWS; only the first D columns count) of one problem: returns (state [3, N, D] f64,
    potentials [num_steps], h [D] of the last step)."""
    D = ref.num_params(F, H)
    p, m, v = (torch.as_tensor(state, dtype=torch.float64)[r, :, :D].clone() for r in range(3))
    lr, b1, b2, eps = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps)
    pots, h = [], torch.full((D,), float('nan'), dtype=torch.float64)
    for t in range(step0, step0 + num_steps):
        U, h, s = step_terms(p, x, y, n, F, H, activation, bandwidth_factor)
        pots.append(U)
        p, m, v = adam(p, m, v, s, t + 1, lr, b1, b2, eps)
    return torch.stack([p, m, v]), np.array(pots), h


def initial_particles(P, N, D, seed):
    """fit_bnn_svgd's start: every coordinate of every particle the median of 15 N(0, 1) draws from `seed`, f32 [P, N, D]."""
    return torch.randn(15, P, N, D, generator=torch.Generator().manual_seed(int(seed))).median(0).values


def no_data_start():
    c = NO_DATA
    return initial_particles(c['P'], c['N'], ref.num_params(c['F'], c['H']), c['seed'])


def no_data_conditions(particles, pots):
    """The three figures of the no-data case from particles [P, N, D] and potentials [P, T]: (max |mean|, max |std - 1|, min over problems of
    (min of the last 50 potentials - the first))."""
    particles, pots = torch.as_tensor(particles).double(), np.asarray(pots, dtype=np.float64)
    return (float(particles.mean(1).abs().max()), float((particles.std(1) - 1.).abs().max()), float((pots[:, -50:].min(1) - pots[:, 0]).min()))
