"""f64 restatement of the BNN posterior target of csrc/bnn_mcmc.hip, written from its formula (include/pfn_hip.h "BNN posterior target"), in torch on the CPU:

    theta = (W1 [H,F] row-major, b1 [H], W2 [2,H], b2 [2]),  D = H (F + 3) + 2
    o_i = W2 act(W1 x_i + b1) + b2,   act = identity | tanh
    U(theta) = |theta|^2 / 2 + (D / 2) log 2 pi - sum_{i<n} log softmax(o_i)[y_i],   y_i = (y > 0.5)

The gradient comes from autograd in f64; `potential_fun` has the (theta) -> (U, grad) signature of tests/nuts_f64.py; `predict` is the class-1 probability.
`potentials` (U of a batch of parameter vectors), `adam` and `f32` are what the SVI and SVGD restatements (bnn_svi_f64.py, bnn_svgd_f64.py) share."""
import math

import numpy as np
import torch

ACT = {'identity': 0, 'tanh': 1, 0: 0, 1: 1}


def num_params(F, H):
    return H * (F + 3) + 2


def unpack(theta, F, H):
    W1 = theta[:H * F].reshape(H, F)
    b1 = theta[H * F:H * F + H]
    W2 = theta[H * F + H:H * F + 3 * H].reshape(2, H)
    b2 = theta[H * F + 3 * H:H * F + 3 * H + 2]
    return W1, b1, W2, b2


def logits(theta, x, F, H, activation):
    W1, b1, W2, b2 = unpack(theta, F, H)
    h = x @ W1.T + b1
    if ACT[activation]:
        h = torch.tanh(h)
    return h @ W2.T + b2


def potential(theta, x, y, n, F, H, activation=0):
    """U(theta) as an f64 tensor (differentiable in theta).  theta [>= D] (only the first D entries are used), x [S,F], y [S]; the first n rows count."""
    D = num_params(F, H)
    theta = theta[:D]
    U = 0.5 * (theta * theta).sum() + 0.5 * D * math.log(2. * math.pi)
    if n > 0:
        o = logits(theta, x[:n].double(), F, H, activation)
        cls = (y[:n] > 0.5).long()
        U = U - torch.log_softmax(o, -1).gather(1, cls[:, None]).sum()
    return U


def potentials(theta, x, y, n, F, H, activation=0):
    """U(theta_k) [K] for a batch of parameter vectors theta [K, D] (differentiable): `potential`, batched."""
    K, D = theta.shape
    U = 0.5 * (theta * theta).sum(1) + 0.5 * D * math.log(2. * math.pi)
    if n > 0:
        W1 = theta[:, :H * F].reshape(K, H, F)
        b1 = theta[:, H * F:H * F + H]
        W2 = theta[:, H * F + H:H * F + 3 * H].reshape(K, 2, H)
        b2 = theta[:, H * F + 3 * H:]
        h = torch.einsum('nf,khf->knh', x[:n].double(), W1) + b1[:, None, :]
        if ACT[activation]:
            h = torch.tanh(h)
        o = torch.einsum('knh,kch->knc', h, W2) + b2[:, None, :]
        cls = (y[:n] > 0.5).long()[None, :, None].expand(K, n, 1)
        U = U - torch.log_softmax(o, -1).gather(2, cls).sum((1, 2))
    return U


def adam(p, m, v, g, t, lr, beta1, beta2, eps):
    """One Adam update of (p, m, v) with gradient g at t = step index + 1 (the SVI and SVGD step loops)."""
    m = beta1 * m + (1. - beta1) * g
    v = beta2 * v + (1. - beta2) * g * g
    p = p - lr * (m / (1. - beta1 ** t)) / (torch.sqrt(v / (1. - beta2 ** t)) + eps)
    return p, m, v


def f32(v):
    """The f64 value of v rounded to f32: what a kernel receives for lr, beta1, beta2, eps and bandwidth_factor."""
    return float(np.float32(v))


def value_and_grad(theta, x, y, n, F, H, activation=0):
    """(U, dU/dtheta [D]) in f64."""
    D = num_params(F, H)
    t = torch.as_tensor(theta, dtype=torch.float64)[:D].clone().requires_grad_(True)
    U = potential(t, x, y, n, F, H, activation)
    g, = torch.autograd.grad(U, t)
    return float(U.detach()), g


def potential_fun(x, y, n, F, H, activation=0):
    """fun(theta numpy [D]) -> (U, grad numpy [D]): the target in the form tests/nuts_f64.py drives."""
    def fun(theta):
        U, g = value_and_grad(np.asarray(theta, dtype=np.float64), x, y, n, F, H, activation)
        return U, g.numpy()
    return fun


def predict(theta, x_test, F, H, activation=0):
    """Class-1 probability [m] in f64."""
    t = torch.as_tensor(theta, dtype=torch.float64)[:num_params(F, H)]
    return torch.softmax(logits(t, x_test.double(), F, H, activation), -1)[:, 1]
