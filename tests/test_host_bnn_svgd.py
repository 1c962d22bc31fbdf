"""Host-side checks of SVGD on the BNN (csrc/bnn_svgd.hip, hipops.bnn_svgd_steps, mcmc_svi_transformer_on_bayesian.fit_bnn_svgd / eval_svgd): the C ABI and its
error paths without a GPU, the f64 restatement (tests/bnn_svgd_f64.py) verified against torch.median over explicit pairs, against torch.autograd and against
torch.optim.Adam BEFORE the GPU tests use it as their oracle, the no-data conditions of the GPU test on the restatement alone, the kernels' register and
scratch budgets read off the compiler's kernel descriptors, and the Python surface.  No GPU."""
import math
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
import bnn_svgd_f64 as svgd      # noqa: E402

from transformerscandobayesianinference_amd import _hip, hipops      # noqa: E402
from transformerscandobayesianinference_amd import mcmc_svi_transformer_on_bayesian as study      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc')
PFN_ERR_UNSUPPORTED, PFN_ERR_ARGUMENT = -1, -4


def test_the_symbols_are_declared_exported_and_bound_at_abi_10():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    lib = _hip.lib()
    for name in ('pfn_bnn_svgd_steps', 'pfn_bnn_svgd_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in _hip.SIGNATURES and hasattr(lib, name), name
    assert '#define PFN_BNN_SVGD_MAX_PARTICLES 64' in header and hipops.SVGD_MAX_PARTICLES == 64
    assert _hip.ABI_VERSION == 10 and lib.pfn_abi_version() == 10 and '#define PFN_ABI_VERSION 10' in header
    build = open(os.path.join(CSRC, 'build.sh')).read()
    assert 'bnn_svgd.hip' in build and '../_build/bnn_svgd.o' in build      # compiled and linked
    text = open(os.path.join(CSRC, 'bnn_svgd.hip')).read()
    assert '#include "bnn_device.h"' in text
    for name in ('struct BnnLane', 'struct BnnSums', 'float bnn_hidden', 'float bnn_sigmoid', 'void bnn_stage', 'void bnn_row_step', 'void bnn_rows', 'float bnn_group_sum'):
        assert name not in text, name      # the shared device functions live in one place


def test_out_of_range_arguments_are_refused_without_a_gpu():
    lib = _hip.lib()
    buf = torch.zeros(4096)      # host memory: a refused call never looks at it
    p = buf.data_ptr()

    def call(F=3, H=5, N=4, ld=32, state=p, step0=0, num_steps=4, P=1, S=4, act=0, x=p, y=p, lr=1e-3, beta1=.9, beta2=.999, eps=1e-8, bw=1., ws=p, ws_bytes=1 << 30):
        return lib.pfn_bnn_svgd_steps(x, y, 0, state, ld, P, S, F, H, act, N, step0, num_steps, lr, beta1, beta2, eps, bw, ws, ws_bytes, 0, 0, 0)
    for F, H in ((17, 5), (3, 65), (0, 5), (3, 0)):
        assert call(F=F, H=H) == PFN_ERR_UNSUPPORTED, (F, H)
        assert lib.pfn_last_error_string()
    assert call(act=2) == PFN_ERR_UNSUPPORTED
    for N in (1, 65, 0, -3):
        assert call(N=N) == PFN_ERR_UNSUPPORTED, N
    assert b'num_particles 65' in [call(N=65), lib.pfn_last_error_string()][1]      # the message names what was wrong
    assert b'F 17' in [call(F=17), lib.pfn_last_error_string()][1]
    assert call(F=17, state=0) == PFN_ERR_UNSUPPORTED and call(N=1, state=0, ld=0) == PFN_ERR_UNSUPPORTED      # the limits come first
    for kw in (dict(ld=31), dict(state=0), dict(step0=-1), dict(num_steps=-1), dict(P=0), dict(S=0), dict(x=0), dict(y=0), dict(beta1=1.), dict(beta2=-.1),
               dict(lr=float('nan')), dict(lr=float('inf')), dict(lr=-1.), dict(eps=-1.), dict(bw=0.), dict(bw=-1.), dict(bw=float('nan'))):
        assert call(**kw) == PFN_ERR_ARGUMENT, kw
    assert b'ld 31' in [call(ld=31), lib.pfn_last_error_string()][1]
    assert call(num_steps=-1, state=0) == PFN_ERR_ARGUMENT
    assert call(num_steps=0) == 0      # nothing to do: returns at once, no HIP call (there is no GPU here)
    assert call(F=16, H=64, ld=1217) == PFN_ERR_ARGUMENT and hipops.bnn_num_params(16, 64) == 1218
    # the workspace: none while the state stays in LDS (small D), the particles' gradients otherwise
    wb = lib.pfn_bnn_svgd_workspace_bytes
    assert wb(100, 50, 3, 5) == 0 and call(N=50, ws=0, ws_bytes=0, num_steps=0) == 0
    assert wb(100, 50, 8, 64) == 100 * 50 * 706 * 4 and wb(1, 64, 16, 64) == 64 * 1218 * 4
    for bad in ((0, 50, 3, 5), (1, 1, 3, 5), (1, 65, 3, 5), (1, 50, 17, 5), (1, 50, 3, 65)):
        assert wb(*bad) < 0, bad
    need = wb(2, 50, 8, 64)
    assert call(F=8, H=64, N=50, P=2, ld=706, ws_bytes=need - 1) == PFN_ERR_ARGUMENT      # a short workspace
    assert call(F=8, H=64, N=50, P=2, ld=706, ws=0, ws_bytes=need) == PFN_ERR_ARGUMENT
    assert call(F=8, H=64, N=50, P=2, ld=706, ws_bytes=need, num_steps=0) == 0


def problem(F, H, S, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, F, generator=g)
    y = (torch.rand(S, generator=g) > 0.5).float()
    return x, y, torch.randn(N, ref.num_params(F, H), generator=g, dtype=torch.float64)


def test_the_batched_potential_is_bnn_f64s():
    for activation in ('identity', 'tanh'):
        x, y, theta = problem(3, 5, 12, 4, 1)
        for n in (0, 9):
            U, g = svgd.potentials_and_grads(theta, x, y, n, 3, 5, activation)
            for k in range(4):
                want_U, want_g = ref.value_and_grad(theta[k], x, y, n, 3, 5, activation)
                assert abs(float(U[k]) - want_U) < 1e-12 * abs(want_U) and float((g[k] - want_g).abs().max()) < 1e-12 * float(want_g.abs().max())


@pytest.mark.parametrize('N', [2, 3, 4, 5, 50])
def test_the_bandwidth_is_torch_medians_lower_median_over_the_pairs(N):
    x = torch.randn(N, 7, generator=torch.Generator().manual_seed(N), dtype=torch.float64)
    pairs = torch.stack([(x[i] - x[j]) ** 2 for i in range(N) for j in range(i + 1, N)])
    assert pairs.shape[0] == N * (N - 1) // 2
    want = torch.median(pairs, 0).values / math.log(N + 1)
    assert torch.equal(svgd.bandwidth(x), want) and torch.equal(svgd.bandwidth(x, 2.), 2. * want)
    srt = pairs.sort(0).values
    k = (pairs.shape[0] - 1) // 2      # the lower of the two middle values when the count is even (N = 4: 6 pairs, N = 5: 10 pairs)
    assert torch.equal(want, srt[k] / math.log(N + 1))
    if pairs.shape[0] % 2 == 0:
        assert bool((srt[k] < srt[k + 1]).all())      # ... and not their mean: the bandwidth is one of the pairwise values


def test_the_stein_direction_is_the_kernel_weighted_gradient_plus_autograds_repulsion():
    x, y, p = problem(3, 5, 12, 6, 3)
    _, g = svgd.potentials_and_grads(p, x, y, 9, 3, 5, 'tanh')
    h = svgd.bandwidth(p)
    got = svgd.stein_direction(p, g, h)
    N, D = p.shape
    want = torch.empty(N, D, dtype=torch.float64)
    for n in range(N):
        xm = p.clone().requires_grad_(True)
        k = torch.exp(-(p[n][None, :].detach() - xm) ** 2 / h.detach())      # k_d(x_n, x_m) [m, d], h a constant
        rep, = torch.autograd.grad(k.sum(), xm)      # d / d x_m of sum_m k_d(x_n, x_m): [m, d]
        # s is a DESCENT gradient (Adam subtracts it): minus the ascent direction (1/N) sum_m [ k grad log p(x_m) + grad_{x_m} k ], with grad log p = -g
        want[n] = ((k.detach() * g).sum(0) - rep.sum(0)) / N
    assert float((got - want).abs().max()) < 1e-12 * float(want.abs().max())


def test_ten_steps_match_torch_adam_with_the_direction_as_the_gradient():
    F, H, S, n, N, T = 3, 5, 12, 12, 7, 10
    x, y, p0 = problem(F, H, S, N, 8)
    D = ref.num_params(F, H)
    lr, betas, eps = 0.05, (0.9, 0.999), 1e-8
    state = torch.zeros(3, N, D, dtype=torch.float64)
    state[0] = p0
    got, pots, h = svgd.run(state, x, y, n, F, H, 'tanh', num_steps=T, lr=lr, betas=betas, eps=eps)
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=svgd.f32(lr), betas=(svgd.f32(betas[0]), svgd.f32(betas[1])), eps=svgd.f32(eps))
    want_pots = []
    for t in range(T):
        U, hh, s = svgd.step_terms(p.detach(), x, y, n, F, H, 'tanh')
        want_pots.append(U)
        opt.zero_grad()
        p.grad = s
        opt.step()
    assert float((got[0] - p.detach()).abs().max()) < 1e-12 and float(np.abs(pots - np.array(want_pots)).max()) < 1e-12 * float(np.abs(want_pots).max())
    assert float((got[1] - opt.state[p]['exp_avg']).abs().max()) < 1e-12 and float((got[2] - opt.state[p]['exp_avg_sq']).abs().max()) < 1e-12
    assert float((h - hh).abs().max()) < 1e-12      # the bandwidth of the last step
    # split runs continue each other
    a, pa, _ = svgd.run(state, x, y, n, F, H, 'tanh', num_steps=4, lr=lr)
    b, pb, hb = svgd.run(a, x, y, n, F, H, 'tanh', step0=4, num_steps=6, lr=lr)
    assert torch.equal(b, got) and np.array_equal(np.concatenate([pa, pb]), pots) and torch.equal(hb, h)


def no_data_f64():
    """The no-data case on the restatement, from the f32 numbers the kernel starts from: (particles [P, N, D], potentials [P, T])."""
    c = svgd.NO_DATA
    start = hipops.bnn_svgd_state(c['P'], c['N'], c['F'], c['H'], 'cpu', particles0=svgd.no_data_start()).double()
    x, y = torch.zeros(1, c['F']), torch.zeros(1)
    out = [svgd.run(start[p], x, y, 0, c['F'], c['H'], num_steps=c['T'], lr=c['lr']) for p in range(c['P'])]
    return torch.stack([o[0][0] for o in out]), np.stack([o[1] for o in out])


def test_with_no_data_the_restatement_alone_spreads_the_particles_over_the_prior():
    """n = 0: the target is N(0, I).  From the median-of-15 start (std about 0.32) the particles' mean stays at 0 and their standard deviation reaches 1 in every
    coordinate, and their mean potential rises above its first value.  The GPU test asserts the same three conditions on the kernel's result."""
    start = svgd.no_data_start()
    assert 0.25 < float(start.std()) < 0.4
    particles, pots = no_data_f64()
    mean, std, rise = svgd.no_data_conditions(particles, pots)
    print(f'no data (f64): max |mean| {mean:.2e}, max |std - 1| {std:.3f}, potential {pots[:, 0].mean():.2f} -> {pots[:, -50:].mean():.2f} (min rise {rise:.2f})')
    assert mean < 0.05 and std < 0.1 and rise > 0.


def test_svgd_kernels_keep_their_register_budget_and_use_no_scratch(tmp_path):
    """Every instantiation (Hp 8 / 16 / 32 / 64 x Fp 4 / 8 / 16 x 2 activations): no scratch, at most 256 VGPRs (the launch bounds' two waves per SIMD); read
    off the compiler's own kernel descriptors (hipcc -S of bnn_svgd.hip with the flags of csrc/build.sh)."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    asm = str(tmp_path / 'bnn_svgd.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-munsafe-fp-atomics', '-S', '--cuda-device-only', os.path.join(CSRC, 'bnn_svgd.hip'), '-o', asm],
                   check=True, capture_output=True)
    seen = set()
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', open(asm).read(), re.S):
        name, body = m.group(1), m.group(2)
        inst = re.search(r'bnn_svgd_kernelILi(\d+)ELi(\d+)ELi(\d+)E', name)
        if not inst:
            continue
        vgpr = int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1))
        scratch = int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1))
        assert scratch == 0, (name, scratch)
        assert vgpr <= 256, (name, vgpr)
        seen.add(tuple(int(v) for v in inst.groups()))
    assert seen == {(hp, fp, act) for hp in (8, 16, 32, 64) for fp in (4, 8, 16) for act in (0, 1)}


def test_state_and_the_surface():
    state = hipops.bnn_svgd_state(3, 7, 3, 5, 'cpu')
    assert state.shape == (3, 3, 7, 32) and state.dtype == torch.float32 and float(state.abs().max()) == 0 and hipops.SVGD_ROWS == svgd.ROWS
    p0 = torch.arange(3 * 7 * 32.).reshape(3, 7, 32)
    filled = hipops.bnn_svgd_state(3, 7, 3, 5, 'cpu', particles0=p0)
    assert torch.equal(filled[:, 0], p0) and float(filled[:, 1:].abs().max()) == 0
    with pytest.raises(_hip.HipExtensionError):      # no CPU fallback
        hipops.bnn_svgd_steps(torch.zeros(3, 4, 3), torch.zeros(3, 4), filled, 5, 2)
    spec = study.get_default_model_spec('small')
    X, y = torch.zeros(2, 12, 3), torch.zeros(2, 12)
    with pytest.raises(NotImplementedError) as e:
        study.eval_svgd(X, y, 'cpu', spec, 10, 4)
    assert 'GPU only' in str(e.value) and 'ELBO' in str(e.value) and 'pfn_bnn_svgd_steps' in str(e.value)
    with pytest.raises(NotImplementedError, match='eval_svgd'):      # eval_svi keeps refusing svgd=True, and now says where SVGD is
        study.eval_svi(X, y, 'cuda', spec, 10, 4, 4, svgd=True)
    for fun in (study.training_steps, lambda *a, **k: study.training_samples(*a, evaluation_points=[5], **k)):
        with pytest.raises(NotImplementedError, match='GPU only'):
            fun('svgd', X, y, spec, device='cpu', path_interfix='/nonexistent')
    fit = study.BnnParticles(filled, torch.zeros(3, 0), spec, 'identity')
    assert fit.particles.shape == (3, 7, 32) and torch.equal(fit.particles, p0) and fit.potentials.shape == (3, 0) and fit.model_spec == spec
    # the start of fit_bnn_svgd: the median of 15 draws per coordinate
    start = svgd.initial_particles(2, 50, 32, 0)
    assert start.shape == (2, 50, 32) and torch.equal(start, svgd.initial_particles(2, 50, 32, 0)) and not torch.equal(start, svgd.initial_particles(2, 50, 32, 1))
    from transformerscandobayesianinference_amd import compat
    saved = dict(sys.modules)
    try:
        compat.install()
        import mcmc_svi_transformer_on_bayesian as top
        for name in ('eval_svgd', 'fit_bnn_svgd', 'BnnParticles'):
            assert getattr(top, name) is getattr(study, name), name
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)
