"""Host-side checks of the batched NUTS (csrc/gp_mcmc.hip, mcmc.py, priors.fast_gp_mix): the C ABI, the workspace size, the warmup schedule, the f64
emulation of the state machine (tests/nuts_f64.py) verified against the recursive formulation and against grid quadrature of a GP hyper-posterior BEFORE
the GPU tests use it as their oracle, the ported `get_mean_logdensity`, the error paths, and the resource budgets of the new kernels.  No GPU."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nuts_f64 as emu      # noqa: E402

from transformerscandobayesianinference_amd import _hip, mcmc      # noqa: E402
from transformerscandobayesianinference_amd.priors import fast_gp_mix      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pfn_nuts_workspace_bytes', 'pfn_nuts_init', 'pfn_nuts_advance')


def test_the_three_symbols_are_declared_exported_and_bound_at_abi_10():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    lib = _hip.lib()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert _hip.ABI_VERSION == 10 and lib.pfn_abi_version() == 10 and '#define PFN_ABI_VERSION 10' in header
    for macro, value in (('PFN_NUTS_ADAPT_MASS', _hip.NUTS_ADAPT_MASS), ('PFN_NUTS_KEEP_WARMUP', _hip.NUTS_KEEP_WARMUP), ('PFN_NUTS_MAX_WINDOWS', _hip.NUTS_MAX_WINDOWS),
                         ('PFN_NUTS_INV_MASS_OFFSET', _hip.NUTS_INV_MASS_OFFSET)):
        assert f'#define {macro} {value}\n' in header, macro


def test_workspace_grows_with_every_size_and_refuses_bad_ones():
    size = _hip.lib().pfn_nuts_workspace_bytes
    for D in (1, 5, 64, 65, 128):
        for depth in (1, 6, 10):
            got = [size(C, D, depth) for C in (1, 2, 3, 9, 1029)]
            assert all(b > a > 0 for a, b in zip(got, got[1:])), got
    for C in (1, 9):
        for depth in (1, 10):
            got = [size(C, D, depth) for D in (1, 2, 64, 65, 128)]
            assert all(b > a for a, b in zip(got, got[1:])), got
        got = [size(C, 20, depth) for depth in range(1, 11)]
        assert all(b > a for a, b in zip(got, got[1:])), got
    # the state the kernel keeps: the inverse mass behind the header, and at least the 14 + 2 depth vectors of a chain
    assert size(7, 20, 10) >= _hip.NUTS_INV_MASS_OFFSET + 4 * 7 * 20 * (1 + 14 + 20)
    for bad in ((0, 5, 10), (4, 0, 10), (4, 129, 10), (4, 5, 0), (4, 5, 11), (-1, 5, 10)):
        assert size(*bad) < 0, bad


def test_adaptation_windows_are_stans_schedule():
    ends = lambda w: tuple(e for _, e in mcmc.adaptation_windows(w))
    assert ends(300) == (100, 150, 250) and ends(1000) == (100, 150, 250, 450, 950) and ends(150) == (100,)
    assert mcmc.adaptation_windows(19) == [] and mcmc.adaptation_windows(0) == []
    assert mcmc.adaptation_windows(300)[0] == (75, 100)
    for w in (20, 57, 100, 149, 150, 151, 299, 2000):
        win = mcmc.adaptation_windows(w)
        assert win and win[0][0] >= 0 and win[-1][1] <= w and len(win) <= _hip.NUTS_MAX_WINDOWS
        assert all(a < b for a, b in win) and all(p[1] == q[0] for p, q in zip(win, win[1:]))      # contiguous, non-empty
    assert mcmc.adaptation_windows(100) == [(15, 90)]      # 15 % / 75 % / 10 %


SIGMA = np.array([.3, .6, 1., 1.7, 3.])


def gaussian(theta):
    return 0.5 * float(np.sum(theta * theta / SIGMA ** 2)), theta / SIGMA ** 2


def test_philox_matches_the_published_test_vector():
    """Random123's known-answer test for philox4x32-10 (kat_vectors): counter and key of all ones."""
    assert emu.philox4x32_10(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert emu.philox4x32_10(0, 0, 0) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)


def test_iterative_transition_equals_the_recursive_formulation():
    """300 chains of a 5-D Gaussian at three step sizes: the iterative tree with its popcount-indexed checkpoints stops exactly where recursive doubling
    does -- the same depth, number of leapfrogs and divergence flag -- from shallow trees (eps .45) to depth 8 (eps .05)."""
    rng = np.random.default_rng(0)
    depths = set()
    for eps in (.05, .2, .45):
        for c in range(300):
            theta = rng.standard_normal(5) * SIGMA
            U, g = gaussian(theta)
            draws = emu.Draws(7, c)
            a = emu.transition(gaussian, theta, U, g, np.ones(5), eps, draws, 3, 10)
            b = emu.transition_recursive(gaussian, theta, U, g, np.ones(5), eps, draws, 3, 10)
            assert (a['depth'], a['leapfrogs'], a['diverging']) == (b['depth'], b['leapfrogs'], b['diverging']), (eps, c)
            depths.add(a['depth'])
    assert min(depths) <= 2 and max(depths) >= 8, depths
    # a divergent first leaf: the recursion and the iteration both stop after one leapfrog and keep the start point
    theta = np.ones(5)
    U, g = gaussian(theta)
    a = emu.transition(gaussian, theta, U, g, np.ones(5), 50 * .3, emu.Draws(7, 0), 0, 10)
    b = emu.transition_recursive(gaussian, theta, U, g, np.ones(5), 50 * .3, emu.Draws(7, 0), 0, 10)
    assert (a['depth'], a['leapfrogs'], a['diverging']) == (1, 1, 1) == (b['depth'], b['leapfrogs'], b['diverging']) and np.array_equal(a['theta'], theta)


def test_closed_form_gp_potential_equals_autograd():
    x, y, prior, kernel = emu.gp_problem()
    fast, slow = emu.gp_potential(x, y, prior, kernel), emu.gp_potential_autograd(x, y, prior, kernel)
    rng = np.random.default_rng(1)
    for _ in range(5):
        theta = rng.standard_normal(3) * 1.5
        (U, g), (U64, g64) = fast(theta), slow(theta)
        assert abs(U - U64) < 1e-10 * max(1., abs(U64)) and np.abs(g - g64).max() < 1e-9 * max(1., np.abs(g64).max())


def test_emulated_chains_reproduce_the_quadrature_of_a_gp_hyperposterior():
    """24 chains x (150 warmup + 150 samples) of the f64 emulation on the GP target (F = 1, n = 12, Matern 5/2) against f64 grid quadrature of the same
    density.  The chain means are independent, so z = (mean over chains - quadrature mean) / (sd of the chain means / sqrt(chains)) is standard normal (t with 23
    degrees of freedom) whatever the autocorrelation inside a chain; 4.5 is a 7e-6 tail.  The box holds the posterior: its faces carry < 1e-4 of the mass."""
    want, face_mass = emu.gp_quadrature()
    print(f'quadrature mean {want}, mass on the box faces {face_mass:.2e}')
    assert face_mass < 1e-4
    x, y, prior, kernel = emu.gp_problem()
    fun = emu.gp_potential(x, y, prior, kernel)
    theta0 = fast_gp_mix.default_theta(1, 1, emu.GP_HP)[0, :3].double().numpy()
    chains, evaluations = 24, 0
    means = []
    for c in range(chains):
        res = emu.run_chain(fun, theta0, 150, 150, 0, c, windows=mcmc.adaptation_windows(150))
        means.append(res['samples'].mean(0))
        evaluations += res['stats'][:, 3].sum()
    means = np.array(means)
    z = (means.mean(0) - want) / (means.std(0, ddof=1) / math.sqrt(chains))
    print(f'z = {z}, {evaluations / chains / 300:.2f} evaluations per transition')
    assert np.abs(z).max() <= 4.5, z


class _Dist:
    def __init__(self, mean, variance):
        self.mean, self.variance = mean, variance


def test_get_mean_logdensity_against_scipy():
    from scipy.special import logsumexp
    from scipy.stats import norm
    g = torch.Generator().manual_seed(3)
    dists = [_Dist(torch.randn(1, 7, generator=g, dtype=torch.float64), torch.rand(1, 7, generator=g, dtype=torch.float64) + .05),
             _Dist(torch.randn(5, generator=g, dtype=torch.float64), torch.rand(5, generator=g, dtype=torch.float64) + .05)]
    mu = np.concatenate([d.mean.reshape(-1).numpy() for d in dists])
    sd = np.sqrt(np.concatenate([d.variance.reshape(-1).numpy() for d in dists]))
    for y in (-.7, .2, 1.9):
        want = logsumexp(norm.logpdf(y, mu, sd)) - math.log(12)
        assert abs(float(fast_gp_mix.get_mean_logdensity(dists, torch.tensor(y, dtype=torch.float64))) - want) < 1e-12
        lo, hi = -1., 2.5
        want = logsumexp(norm.logpdf(y, mu, sd) - np.log(norm.cdf(hi, mu, sd) - norm.cdf(lo, mu, sd))) - math.log(12)
        assert abs(float(fast_gp_mix.get_mean_logdensity(dists, torch.tensor(y, dtype=torch.float64), full_range=(lo, hi))) - want) < 1e-12
    assert fast_gp_mix.get_mean_logdensity(dists, torch.tensor(.2, dtype=torch.float64)).shape == ()


def test_the_sampler_needs_a_gpu_and_rejects_output_warping():
    x, y = torch.rand(1, 8, 2), torch.zeros(1, 8)
    with pytest.raises(_hip.HipExtensionError):
        fast_gp_mix.sample_hyperparameter_posterior(x, y)
    with pytest.raises(_hip.HipExtensionError):
        fast_gp_mix.get_mcmc_model(x[0], y[0], {}, 'cpu', 4, 4)
    with pytest.raises(_hip.HipExtensionError):
        fast_gp_mix.evaluate_(x.transpose(0, 1), y.transpose(0, 1), y.transpose(0, 1), {}, device='cpu', num_samples=4, warmup_steps=4)
    with pytest.raises(_hip.HipExtensionError):
        mcmc.batched_nuts(lambda t: (t.sum(1), t), torch.zeros(2, 3), 4, 4)
    for hp in ({'y_minmax_norm': True}, {'sigmoid': True}):
        with pytest.raises(AssertionError):
            fast_gp_mix.get_mcmc_model(x[0], y[0], hp, 'cpu', 4, 4)
        with pytest.raises(AssertionError):
            fast_gp_mix.evaluate_(x.transpose(0, 1), y.transpose(0, 1), y.transpose(0, 1), hp, device='cpu', num_samples=4, warmup_steps=4)
    with pytest.raises(NotImplementedError):      # unchanged: the botorch model for fitting is still not built
        fast_gp_mix.get_model(x, y, {}, sample=False)


def test_new_kernels_keep_their_register_and_scratch_budgets(tmp_path):
    """Read off the compiler's kernel descriptors (hipcc -S of gp_mcmc.hip with the flags of csrc/build.sh): no scratch, no LDS (the checkpoint rows live in
    the workspace, nothing is a per-thread array), at most 256 VGPRs."""
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    src = os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc', 'gp_mcmc.hip')
    asm = str(tmp_path / 'gp_mcmc.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-munsafe-fp-atomics', '-S', '--cuda-device-only', src, '-o', asm], check=True, capture_output=True)
    seen = set()
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', open(asm).read(), re.S):
        name, body = m.group(1), m.group(2)
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 256, name
        seen.add(re.search(r'nuts_[a-z]+_kernel', name).group(0))
    assert seen == {'nuts_init_kernel', 'nuts_advance_kernel'}
