"""f64 restatement of the SVI step of csrc/bnn_svi.hip, written from its contract (include/pfn_hip.h "SVI on the BNN"), in torch / numpy on the CPU:

    q(theta) = N(loc, diag(scale^2)), scale = softplus(u);  theta_k = loc + scale eps_k, k < K
    L = mean_k [ U(theta_k) - sum_i (log scale_i + eps_ki^2 / 2) - (D / 2) log 2 pi ]            (U: tests/bnn_f64.py)
    g_loc = mean_k grad U(theta_k),  g_scale = mean_k grad U(theta_k) * eps_k - 1 / scale,  g_u = g_scale sigmoid(u)
    Adam: m <- b1 m + (1 - b1) g, v <- b2 v + (1 - b2) g^2, p <- p - lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps), t = step index + 1

The noise is the kernel's: eps of (problem id q, step t, particle k, coordinate i) is component i & 3 of normal4(philox4x32_10(((t K + k) << 10) | (i >> 2), q,
seed)), with tests/nuts_f64.py's philox4x32_10 (called on numpy arrays) and its Box-Muller formulas applied to whole arrays.  `loss` is the same objective as a
differentiable torch expression: the host tests check the closed-form gradient against it and against central differences, and the Adam recurrence against
torch.optim.Adam."""
import math

import numpy as np
import torch

import bnn_f64 as ref
from bnn_f64 import adam, f32, potentials      # noqa: F401  (shared with the other restatement; the tests reach them through this module)
import nuts_f64 as emu

ROWS = ('loc', 'u', 'm_loc', 'v_loc', 'm_u', 'v_u')
# The no-data case of the host and the GPU test: n = 0, so the ELBO's optimum is the prior N(0, I), where the loss is 0.  loc0 ~ N(0, 1) from `loc_seed`.
NO_DATA = dict(F=3, H=5, P=4, K=16, T=1500, lr=0.02, seed=11, loc_seed=3, init_scale=0.1)


def noise(seed, q, t, K, D):
    """eps [K, D] f64 of problem id q at absolute step t."""
    nb = (D + 3) // 4
    idx = ((np.uint64(t) * np.uint64(K) + np.arange(K, dtype=np.uint64))[:, None] << np.uint64(10)) | np.arange(nb, dtype=np.uint64)[None, :]
    x, y, z, w = (np.asarray(c, dtype=np.uint64) for c in emu.philox4x32_10(idx, int(q), int(seed)))
    u_open = lambda r: ((r >> np.uint64(8)).astype(np.float64) + 1.) * 2. ** -24
    u = lambda r: (r >> np.uint64(8)).astype(np.float64) * 2. ** -24
    r0, r1 = np.sqrt(-2. * np.log(u_open(x))), np.sqrt(-2. * np.log(u_open(z)))
    a0, a1 = 2. * math.pi * u(y), 2. * math.pi * u(w)
    out = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], -1).reshape(K, 4 * nb)
    return torch.from_numpy(out[:, :D].copy())


def softplus(u):
    return torch.clamp(u, min=0.) + torch.log1p(torch.exp(-u.abs()))


def loss(loc, u, eps, x, y, n, F, H, activation=0):
    """The per-step loss as a differentiable function of (loc, u) at fixed noise eps [K, D]."""
    scale = softplus(u)
    theta = loc[None, :] + scale[None, :] * eps
    D = loc.shape[0]
    return (potentials(theta, x, y, n, F, H, activation) - (torch.log(scale)[None, :] + 0.5 * eps * eps).sum(1) - 0.5 * D * math.log(2. * math.pi)).mean()


def loss_and_grads(loc, u, eps, x, y, n, F, H, activation=0):
    """(L, g_loc [D], g_u [D]) by the closed form of the contract; grad U of every particle from autograd of the potential alone."""
    scale = softplus(u)
    theta = (loc[None, :] + scale[None, :] * eps).detach().requires_grad_(True)
    U = potentials(theta, x, y, n, F, H, activation)
    gU, = torch.autograd.grad(U.sum(), theta)
    D = loc.shape[0]
    L = (U.detach() - (torch.log(scale)[None, :] + 0.5 * eps * eps).sum(1) - 0.5 * D * math.log(2. * math.pi)).mean()
    g_loc = gU.mean(0)
    g_scale = (gU * eps).mean(0) - 1. / scale
    return float(L), g_loc, g_scale * torch.sigmoid(u)


def run(state, x, y, n, F, H, activation=0, K=1, step0=0, num_steps=1, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=0, q=0):
    """`num_steps` steps from state [6, >= D] (rows ROWS; only the first D columns count) of one problem: returns (state [6, D] f64, losses [num_steps])."""
    D = ref.num_params(F, H)
    loc, u, m_loc, v_loc, m_u, v_u = (torch.as_tensor(state, dtype=torch.float64)[r, :D].clone() for r in range(6))
    lr, b1, b2, eps = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps)
    losses = []
    for t in range(step0, step0 + num_steps):
        z = noise(seed, q, t, K, D)
        L, g_loc, g_u = loss_and_grads(loc, u, z, x, y, n, F, H, activation)
        losses.append(L)
        loc, m_loc, v_loc = adam(loc, m_loc, v_loc, g_loc, t + 1, lr, b1, b2, eps)
        u, m_u, v_u = adam(u, m_u, v_u, g_u, t + 1, lr, b1, b2, eps)
    return torch.stack([loc, u, m_loc, v_loc, m_u, v_u]), np.array(losses)


def no_data_loc0():
    c = NO_DATA
    return torch.randn(c['P'], ref.num_params(c['F'], c['H']), generator=torch.Generator().manual_seed(c['loc_seed']))
