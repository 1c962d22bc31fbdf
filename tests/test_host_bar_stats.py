"""Posterior summaries and draws of the bar distribution (pfn_bar_stats / pfn_bar_stats_backward / pfn_bar_sample), host side: the ABI addition,
its argument checks (nothing is launched), and the f64 reference of the GPU tests (tests/bar_f64.py) anchored to the reference's own quantile / ei
(tests/golden/bar_distribution.pt) and to the density of oracle.pfn_oracle.bar_nll."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bar_f64  # noqa: E402
from oracle import pfn_oracle  # noqa: E402
from transformerscandobayesianinference_amd import _hip  # noqa: E402

NEW = ('pfn_bar_stats', 'pfn_bar_stats_backward', 'pfn_bar_sample')
FAKE = 0x1000      # a non-null "device pointer": every call below returns before anything could read it


def test_symbols_are_declared_bound_and_exported_at_abi_10():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    declared = set(re.findall(r'\b(pfn_[a-z0-9_]+)\s*\(', header))
    lib = _hip.lib()
    for name in NEW:
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name), name
    assert re.search(r'#define\s+PFN_ABI_VERSION\s+10\b', header) and lib.pfn_abi_version() == 10 == _hip.ABI_VERSION
    from transformerscandobayesianinference_amd import bar_distribution as bd
    for i, name in enumerate(['MEAN', 'VARIANCE', 'MODE', 'CDF', 'ICDF', 'EI_MAX', 'EI_MIN']):
        assert re.search(rf'#define\s+PFN_BAR_STAT_{name}\s+{i}\b', header) and getattr(bd, 'STAT_' + name) == i
    assert re.search(r'#define\s+PFN_BAR_STATS_MAX\s+16\b', header) and bd.MAX_STATS == 16


def _kinds(*k):
    return (ctypes.c_int32 * max(1, len(k)))(*k)


def _stats(logits=FAKE, ld=8, borders=FAKE, R=4, nbars=8, full=1, kinds=(0, 4), K=None, args=FAKE, arg_ld=0, out=FAKE):
    ck = _kinds(*kinds) if kinds is not None else None
    return _hip.lib().pfn_bar_stats(logits, ld, borders, R, nbars, full, ctypes.addressof(ck) if ck is not None else 0, len(kinds) if K is None else K,
                                    args, arg_ld, out, 0)


def _stats_bwd(logits=FAKE, ld=8, borders=FAKE, R=4, nbars=8, full=1, kinds=(0, 4), K=None, args=FAKE, arg_ld=0, out=FAKE, gout=FAKE, dlogits=FAKE):
    ck = _kinds(*kinds) if kinds is not None else None
    return _hip.lib().pfn_bar_stats_backward(logits, ld, borders, R, nbars, full, ctypes.addressof(ck) if ck is not None else 0,
                                             len(kinds) if K is None else K, args, arg_ld, out, gout, dlogits, 0)


def _sample(logits=FAKE, ld=8, borders=FAKE, R=4, nbars=8, full=1, n=3, seed=1, out=FAKE):
    return _hip.lib().pfn_bar_sample(logits, ld, borders, R, nbars, full, n, seed, out, 0)


BAD = -4      # PFN_ERR_ARGUMENT


@pytest.mark.parametrize('call', [_stats, _stats_bwd], ids=['stats', 'backward'])
def test_stats_argument_checks_return_before_any_launch(call):
    for ptr in ['logits', 'borders', 'args', 'out'] + (['gout', 'dlogits'] if call is _stats_bwd else []):
        assert call(**{ptr: 0}) == BAD, ptr
    assert call(kinds=None, K=2) == BAD
    assert call(kinds=(), K=0) == BAD and call(kinds=(0,) * 17) == BAD and call(kinds=(0,), K=-1) == BAD
    assert call(kinds=(0, 7)) == BAD and call(kinds=(-1,)) == BAD      # unknown kind
    assert call(nbars=0, ld=8) == BAD and call(nbars=1, full=1) == BAD
    assert call(ld=7) == BAD
    assert call(R=-1) == BAD
    assert call(kinds=(0, 1, 3), arg_ld=2) == BAD
    assert b'pfn_bar_stats' in _hip.lib().pfn_last_error_string()
    # nothing to do: PFN_OK without a launch
    assert call(R=0) == 0 and call(R=0, nbars=1, ld=1, full=0) == 0 and call(R=0, kinds=tuple(range(7)) * 2, arg_ld=14) == 0


def test_sample_argument_checks_return_before_any_launch():
    for ptr in ['logits', 'borders', 'out']:
        assert _sample(**{ptr: 0}) == BAD, ptr
    assert _sample(nbars=0) == BAD and _sample(nbars=1, ld=1, full=1) == BAD and _sample(ld=7) == BAD and _sample(n=-1) == BAD and _sample(R=-1) == BAD
    assert _sample(R=0) == 0 and _sample(n=0) == 0 and _sample(R=0, nbars=1, ld=1, full=0, seed=2 ** 64 - 1) == 0


def test_python_layer_refuses_what_it_cannot_run():
    from transformerscandobayesianinference_amd import bar_distribution as bd
    crit = bd.FullSupportBarDistribution(torch.linspace(-1, 1, 9))
    with pytest.raises(_hip.HipExtensionError):      # GPU only, like mean
        crit.stats(torch.zeros(3, 8), [('mean',)])
    with pytest.raises(_hip.HipExtensionError):
        crit.sample(torch.zeros(3, 8), 2, seed=0)


def _golden():
    rec = torch.load(os.path.join(ROOT, 'tests', 'golden', 'bar_distribution.pt'))
    return {k: v for k, v in rec.items() if isinstance(k, tuple)}


def test_f64_helper_matches_the_reference_quantile_and_ei():
    """bounded class: icdf(side) / icdf(1 - side) are the reference's quantile; ei is the reference's for both classes; mode too."""
    seen = 0
    for (nb, full), c in _golden().items():
        lg, b = c['logits'], c['borders']
        for name, maximize in (('ei_max', True), ('ei_min', False)):
            got = bar_f64.ei(lg, b, c['best_f'], maximize)
            assert (got - c[name].double()).abs().max().item() < 1e-5 * max(1., c[name].abs().max().item()), (nb, full, name)
        assert torch.equal(bar_f64.mode(lg, b).float(), c['mode'])
        assert (bar_f64.mean(lg, b, full) - c['mean'].double()).abs().max().item() < 1e-5 * (b[-1] - b[0]).item()
        if full:
            continue
        for key, center in (('quantile', .682), ('quantile90', .9)):
            side = (1 - center) / 2
            q = torch.stack([bar_f64.icdf(lg, b, False, side), bar_f64.icdf(lg, b, False, 1 - side)], -1)
            q = torch.where(reference_wraps(lg, side), wrapped_value(lg, b, side), q)
            assert (q - c[key].double()).abs().max().item() < 2e-5 * (b[-1] - b[0]).item(), (nb, key)
            seen += 1
    assert seen >= 2


def reference_wraps(logits, side):
    """[R, 2] bool: rows whose lower (upper) quantile lies in the first (last) bucket.  There the reference reads cum[idx - 1] with idx = 0, i.e. the LAST
    cumulative sum (bar_distribution.py:52-56; kept in BarDistribution.quantile), so its value is not the quantile; every other row is."""
    p = torch.softmax(logits.double(), -1)
    return torch.stack([p[:, 0] >= side, p[:, -1] >= side], -1)


def wrapped_value(logits, borders, side):
    """what the reference returns on those rows: the edge bucket extrapolated with (side - 1) / p in place of side / p"""
    p = torch.softmax(logits.double(), -1)
    b = borders.double()
    return torch.stack([b[0] + (b[1] - b[0]) * (side - 1) / p[:, 0], b[-1] + (b[-2] - b[-1]) * (side - 1) / p[:, -1]], -1)


def _integrate(f, a, b, cuts, m=4000):
    """midpoint rule on [a, b] split at `cuts` (the borders: the density jumps there), m points per piece"""
    pts = sorted({a, b, *[c for c in cuts if a < c < b]})
    total = 0.0
    for lo, hi in zip(pts[:-1], pts[1:]):
        x = lo + (hi - lo) * (torch.arange(m, dtype=torch.float64) + 0.5) / m
        total += (f(x).sum() * (hi - lo) / m).item()
    return total


def test_f64_helper_integrates_the_density_of_bar_nll():
    """full support: total mass, mean, variance and CDF of bar_f64 against a numerical integral of exp(-bar_nll) (oracle.pfn_oracle)."""
    gen = torch.Generator().manual_seed(5)
    for nb in (2, 5):
        borders = torch.cumsum(torch.rand(nb + 1, generator=gen, dtype=torch.float64) + 0.2, 0) - 1.5
        logits = torch.randn(1, nb, generator=gen, dtype=torch.float64) * 1.5
        w0, w1 = (borders[1] - borders[0]).item(), (borders[-1] - borders[-2]).item()
        lo, hi = borders[1].item() - 14 * w0 / bar_f64.C_HALF, borders[-2].item() + 14 * w1 / bar_f64.C_HALF      # 14 sigma of each tail
        cuts = borders.tolist()
        dens = lambda x: torch.exp(-pfn_oracle.bar_nll(logits.expand(len(x), nb), x, borders, True))      # noqa: E731
        mass = _integrate(dens, lo, hi, cuts)
        m1 = _integrate(lambda x: x * dens(x), lo, hi, cuts)
        m2 = _integrate(lambda x: x * x * dens(x), lo, hi, cuts)
        assert abs(mass - 1) < 1e-6
        assert abs(m1 - bar_f64.mean(logits, borders, True).item()) < 1e-6
        assert abs(m1 - pfn_oracle.bar_mean(logits, borders, True).item()) < 1e-6
        assert abs((m2 - m1 * m1) - bar_f64.variance(logits, borders, True).item()) < 1e-5
        ys = [lo / 2, borders[0].item(), borders[1].item() - 0.3 * w0, borders[1].item(), (borders[1] + 0.25 * (borders[2] - borders[1])).item(),
              borders[-2].item(), borders[-2].item() + 0.4 * w1, borders[-1].item(), borders[-1].item() + 2 * w1]
        for y in ys:
            want = _integrate(dens, lo, y, cuts)
            got = bar_f64.cdf(logits, borders, True, y).item()
            assert abs(got - want) < 1e-6, (nb, y, got, want)
            # and the inverse CDF inverts it
            if 1e-9 < got < 1 - 1e-9:
                assert abs(bar_f64.icdf(logits, borders, True, got).item() - y) < 1e-6 * max(1., abs(y)), (nb, y)


def test_f64_helper_bounded_cdf_and_edges():
    borders = torch.tensor([-1., 0., 0.5, 2.])
    logits = torch.tensor([[0.3, -1e4, 1.0]])
    p = torch.softmax(logits.double(), -1)[0]
    assert bar_f64.cdf(logits, borders, False, -2.).item() == 0 and bar_f64.cdf(logits, borders, False, 2.5).item() == 1
    assert abs(bar_f64.cdf(logits, borders, False, -0.5).item() - 0.5 * p[0].item()) < 1e-15
    assert bar_f64.icdf(logits, borders, False, 0.).item() == -1 and bar_f64.icdf(logits, borders, False, 1.).item() == 2
    assert math.isinf(bar_f64.icdf(logits, borders, True, 0.).item()) and math.isinf(bar_f64.icdf(logits, borders, True, 1.).item())
    # the empty middle bucket is skipped: just above C_0 the quantile is in bucket 2
    q = bar_f64.icdf(logits, borders, False, p[0].item() + 1e-9).item()
    assert 0.5 <= q < 0.5 + 1e-6
