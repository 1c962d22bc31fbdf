"""Host-side checks of SVI on the BNN (csrc/bnn_svi.hip, hipops.bnn_svi_steps, mcmc_svi_transformer_on_bayesian.fit_bnn_svi / eval_svi): the C ABI and its
error paths without a GPU, the f64 restatement (tests/bnn_svi_f64.py) verified against central differences and against torch.optim.Adam BEFORE the GPU tests
use it as their oracle, the kernels' register and scratch budgets read off the compiler's kernel descriptors, the no-data condition of the GPU test on the
restatement alone, and the Python surface.  No GPU."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnn_f64 as ref      # noqa: E402
import bnn_svi_f64 as svi      # noqa: E402
import nuts_f64 as emu      # noqa: E402

from transformerscandobayesianinference_amd import _hip, hipops      # noqa: E402
from transformerscandobayesianinference_amd import mcmc_svi_transformer_on_bayesian as study      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc')
PFN_ERR_UNSUPPORTED, PFN_ERR_ARGUMENT = -1, -4

def test_the_symbol_is_declared_exported_and_bound_at_abi_10():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    lib = _hip.lib()
    assert re.search(r'\bpfn_bnn_svi_steps\s*\(', header)
    assert 'pfn_bnn_svi_steps' in _hip.SIGNATURES and hasattr(lib, 'pfn_bnn_svi_steps')
    assert _hip.ABI_VERSION == 10 and lib.pfn_abi_version() == 10 and '#define PFN_ABI_VERSION 10' in header
    build = open(os.path.join(CSRC, 'build.sh')).read()
    assert 'bnn_svi.hip' in build and '../_build/bnn_svi.o' in build      # compiled and linked
    # the shared device functions live in one place
    shared = open(os.path.join(CSRC, 'bnn_device.h')).read()
    for name in ('struct BnnLane', 'bnn_hidden', 'bnn_sigmoid', 'bnn_stage', 'bnn_row_step'):
        assert name in shared, name
    for src in ('bnn_mcmc.hip', 'bnn_svi.hip'):
        text = open(os.path.join(CSRC, src)).read()
        assert '#include "bnn_device.h"' in text and 'struct BnnLane' not in text, src


def test_out_of_range_arguments_are_refused_without_a_gpu():
    lib = _hip.lib()
    buf = torch.zeros(4096)      # host memory: a refused call never looks at it
    p = buf.data_ptr()

    def call(F=3, H=5, K=1, ld=32, state=p, step0=0, num_steps=4, P=1, S=4, act=0, x=p, y=p, lr=1e-3, beta1=.9, beta2=.999, eps=1e-8):
        return lib.pfn_bnn_svi_steps(x, y, 0, state, ld, P, S, F, H, act, K, step0, num_steps, lr, beta1, beta2, eps, 0, 0, 0, 0)
    for F, H in ((17, 5), (3, 65), (0, 5), (3, 0)):
        assert call(F=F, H=H) == PFN_ERR_UNSUPPORTED, (F, H)
        assert lib.pfn_last_error_string()
    assert call(act=2) == PFN_ERR_UNSUPPORTED
    assert b'F 17' in [call(F=17), lib.pfn_last_error_string()][1]      # the message names what was wrong
    assert call(F=17, K=0, state=0) == PFN_ERR_UNSUPPORTED      # the limits come first
    for kw in (dict(K=0), dict(K=-2), dict(ld=31), dict(state=0), dict(step0=-1), dict(num_steps=-1), dict(P=0), dict(S=0), dict(x=0), dict(y=0),
               dict(beta1=1.), dict(beta2=-.1), dict(lr=float('nan')), dict(eps=-1.)):
        assert call(**kw) == PFN_ERR_ARGUMENT, kw
    assert call(num_steps=-1, state=0) == PFN_ERR_ARGUMENT
    assert call(num_steps=0) == 0      # nothing to do: returns at once, no HIP call (there is no GPU here)
    assert call(F=16, H=64, ld=1217) == PFN_ERR_ARGUMENT and hipops.bnn_num_params(16, 64) == 1218


def problem(F, H, S, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, F, generator=g)
    y = (torch.rand(S, generator=g) > 0.5).float()
    D = ref.num_params(F, H)
    return x, y, torch.randn(D, generator=g, dtype=torch.float64), torch.randn(D, generator=g, dtype=torch.float64) * 0.5 - 1.


def test_the_noise_is_nuts_f64s_philox_and_box_muller_with_the_contracts_addressing():
    K, D, t, q, seed = 3, 10, 7, 5, 123
    z = svi.noise(seed, q, t, K, D)
    assert z.shape == (K, D) and z.dtype == torch.float64
    for k in range(K):
        for i in range(D):
            want = emu.normal4(emu.philox4x32_10(((t * K + k) << 10) | (i >> 2), q, seed))[i & 3]
            assert abs(float(z[k, i]) - want) < 1e-15, (k, i)
    assert torch.equal(svi.noise(seed, q, t, K, 7), z[:, :7])      # a function of (seed, q, t, k, i) alone
    many = torch.cat([svi.noise(1, 0, s, 8, 64).reshape(-1) for s in range(40)])
    assert abs(float(many.mean())) < 0.03 and abs(float(many.std()) - 1.) < 0.03


@pytest.mark.parametrize('activation', ['identity', 'tanh'])
def test_the_elbo_gradient_agrees_with_central_differences(activation):
    F, H, S, n, K = 3, 5, 12, 9, 3
    x, y, loc, u = problem(F, H, S, 4)
    D = ref.num_params(F, H)
    eps = svi.noise(2, 0, 0, K, D)
    L, g_loc, g_u = svi.loss_and_grads(loc, u, eps, x, y, n, F, H, activation)
    fun = lambda a, b: float(svi.loss(a, b, eps, x, y, n, F, H, activation))
    assert abs(L - fun(loc, u)) < 1e-12 * abs(L)
    # the batched potential is tests/bnn_f64's
    theta = loc[None, :] + svi.softplus(u)[None, :] * eps
    for k in range(K):
        assert abs(float(svi.potentials(theta, x, y, n, F, H, activation)[k]) - float(ref.potential(theta[k], x, y, n, F, H, activation))) < 1e-12 * abs(L)
    h = 1e-6
    fd_loc, fd_u = torch.empty(D, dtype=torch.float64), torch.empty(D, dtype=torch.float64)
    for i in range(D):
        e = torch.zeros(D, dtype=torch.float64)
        e[i] = h
        fd_loc[i] = (fun(loc + e, u) - fun(loc - e, u)) / (2 * h)
        fd_u[i] = (fun(loc, u + e) - fun(loc, u - e)) / (2 * h)
    assert float((fd_loc - g_loc).abs().max()) < 1e-7 * float(g_loc.abs().max())
    assert float((fd_u - g_u).abs().max()) < 1e-7 * float(g_u.abs().max())


def test_ten_steps_match_torch_adam_on_the_autograd_loss():
    F, H, S, n, K, T = 3, 5, 12, 12, 2, 10
    x, y, loc0, u0 = problem(F, H, S, 8)
    D = ref.num_params(F, H)
    lr, betas, eps, seed, q = 0.05, (0.9, 0.999), 1e-8, 4, 2
    state = torch.zeros(6, D, dtype=torch.float64)
    state[0], state[1] = loc0, u0
    got, losses = svi.run(state, x, y, n, F, H, 'tanh', K=K, num_steps=T, lr=lr, betas=betas, eps=eps, seed=seed, q=q)
    loc, u = loc0.clone().requires_grad_(True), u0.clone().requires_grad_(True)
    opt = torch.optim.Adam([loc, u], lr=svi.f32(lr), betas=(svi.f32(betas[0]), svi.f32(betas[1])), eps=svi.f32(eps))
    want_losses = []
    for t in range(T):
        opt.zero_grad()
        L = svi.loss(loc, u, svi.noise(seed, q, t, K, D), x, y, n, F, H, 'tanh')
        L.backward()
        opt.step()
        want_losses.append(float(L.detach()))
    assert float((got[0] - loc.detach()).abs().max()) < 1e-12 and float((got[1] - u.detach()).abs().max()) < 1e-12
    assert float(np.abs(losses - np.array(want_losses)).max()) < 1e-12 * float(np.abs(want_losses).max())
    assert float((got[2] - opt.state[loc]['exp_avg']).abs().max()) < 1e-12 and float((got[5] - opt.state[u]['exp_avg_sq']).abs().max()) < 1e-12
    # split runs continue each other
    a, la = svi.run(state, x, y, n, F, H, 'tanh', K=K, num_steps=4, lr=lr, seed=seed, q=q)
    b, lb = svi.run(a, x, y, n, F, H, 'tanh', K=K, step0=4, num_steps=6, lr=lr, seed=seed, q=q)
    assert torch.equal(b, got) and np.array_equal(np.concatenate([la, lb]), losses)


def test_svi_kernels_keep_their_register_budget_and_use_no_scratch(tmp_path):
    """Every instantiation (Hp 8 / 16 / 32 / 64 x Fp 4 / 8 / 16 x 2 activations): no scratch, at most 256 VGPRs; read off the compiler's own kernel descriptors
    (hipcc -S of bnn_svi.hip with the flags of csrc/build.sh)."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    asm = str(tmp_path / 'bnn_svi.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-munsafe-fp-atomics', '-S', '--cuda-device-only', os.path.join(CSRC, 'bnn_svi.hip'), '-o', asm],
                   check=True, capture_output=True)
    seen = set()
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', open(asm).read(), re.S):
        name, body = m.group(1), m.group(2)
        inst = re.search(r'bnn_svi_kernelILi(\d+)ELi(\d+)ELi(\d+)E', name)
        if not inst:
            continue
        vgpr = int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1))
        scratch = int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1))
        assert scratch == 0, (name, scratch)
        assert vgpr <= 256, (name, vgpr)
        seen.add(tuple(int(v) for v in inst.groups()))
    assert seen == {(hp, fp, act) for hp in (8, 16, 32, 64) for fp in (4, 8, 16) for act in (0, 1)}


def no_data_f64():
    """The no-data case on the restatement, from the f32 numbers the kernel starts from: (loc [P, D], scale [P, D], losses [P, T])."""
    c = svi.NO_DATA
    start = hipops.bnn_svi_state(c['P'], c['F'], c['H'], 'cpu', loc0=svi.no_data_loc0(), init_scale=c['init_scale']).double()
    x, y = torch.zeros(1, c['F']), torch.zeros(1)
    out = [svi.run(start[p], x, y, 0, c['F'], c['H'], K=c['K'], num_steps=c['T'], lr=c['lr'], seed=c['seed'], q=p) for p in range(c['P'])]
    return torch.stack([o[0][0] for o in out]), svi.softplus(torch.stack([o[0][1] for o in out])), np.stack([o[1] for o in out])


def test_with_no_data_the_restatement_alone_finds_the_prior():
    """n = 0: the ELBO's optimum is the prior N(0, I) and its loss there is 0.  The GPU test asserts the same three conditions on the kernel's result with the
    same seed and the same Philox noise; here the restatement is shown to satisfy them by itself."""
    loc, scale, losses = no_data_f64()
    first, last = float(losses[:, 0].mean()), float(losses[:, -50:].mean())
    print(f'no data (f64): max |loc| {float(loc.abs().max()):.3f}, max |scale - 1| {float((scale - 1).abs().max()):.3f}, loss {first:.1f} -> {last:.3f}')
    assert float(loc.abs().max()) < 0.3 and float((scale - 1).abs().max()) < 0.2 and last < 0.5 and first > 30.


def test_state_and_the_surface():
    state = hipops.bnn_svi_state(3, 3, 5, 'cpu')
    assert state.shape == (3, 6, 32) and state.dtype == torch.float32 and hipops.SVI_ROWS == svi.ROWS
    assert float((torch.nn.functional.softplus(state[:, 1]) - 0.1).abs().max()) < 1e-7 and float(state[:, [0, 2, 3, 4, 5]].abs().max()) == 0
    loc0 = torch.arange(96.).reshape(3, 32)
    assert torch.equal(hipops.bnn_svi_state(3, 3, 5, 'cpu', loc0=loc0, init_scale=0.5)[:, 0], loc0)
    with pytest.raises(_hip.HipExtensionError):      # no CPU fallback
        hipops.bnn_svi_steps(torch.zeros(3, 4, 3), torch.zeros(3, 4), state, 5, 2)
    spec = study.get_default_model_spec('small')
    X, y = torch.zeros(2, 12, 3), torch.zeros(2, 12)
    with pytest.raises(NotImplementedError, match='ELBO'):
        study.eval_svi(X, y, 'cpu', spec, 10, 4, 4)
    with pytest.raises(NotImplementedError, match='ELBO'):
        study.eval_svi(X, y, 'cpu', spec, 10, 4, 4, svgd=True)
    with pytest.raises(NotImplementedError, match='Stein'):
        study.eval_svi(X, y, 'cuda', spec, 10, 4, 4, svgd=True)      # refused before anything touches the device
    with pytest.raises(NotImplementedError, match='Stein'):
        study._eval('svgd', X, y, 'cuda', spec, 10, 4)
    with pytest.raises(NotImplementedError, match='GPU only'):
        study._eval('svi', X, y, 'cpu', spec, 10, 4)
    state[:, 0] = 2.
    guide = study.BnnGuide(state, torch.zeros(3, 0), spec, 'identity')
    assert guide.loc.shape == (3, 32) and guide.scale.shape == (3, 32) and float((guide.scale - 0.1).abs().max()) < 1e-7
    th = guide.sample(500, seed=1)
    assert th.shape == (3, 500, 32) and torch.equal(th, guide.sample(500, seed=1)) and not torch.equal(th, guide.sample(500, seed=2))
    assert abs(float(th.mean()) - 2.) < 0.01 and abs(float(th.std()) - 0.1) < 0.01
    from transformerscandobayesianinference_amd import compat
    saved = dict(sys.modules)
    try:
        compat.install()
        import mcmc_svi_transformer_on_bayesian as top
        for name in ('eval_svi', 'fit_bnn_svi', 'BnnGuide'):
            assert getattr(top, name) is getattr(study, name), name
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)
