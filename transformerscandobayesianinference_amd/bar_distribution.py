"""Bar ("Riemann") output distribution of the PFN (reference bar_distribution.py).

`forward` (the training loss, reference :25-33 / :89-108) and `mean` (posterior-predictive mean,
:35-38 / :110-117) run in fused HIP kernels (csrc/bar.hip) through the C ABI; the evaluation-only
helpers (`quantile`, `mode`, `ei`) and the one-off border construction `get_bucket_limits` are
PyTorch plumbing exactly as in the reference.  The loss kernels have no CPU fallback.

`stats` computes any set of posterior summaries (mean, variance, mode, CDF, inverse CDF, expected
improvement) in one fused pass per logits row, differentiable in the logits; `variance`, `cdf`,
`icdf`, `median`, `pi`, `ucb` are thin wrappers, and `sample` draws from the predictive distribution
through the same inverse CDF (pfn_bar_stats / pfn_bar_stats_backward / pfn_bar_sample).  GPU only.
"""
import torch
from torch import nn

from transformerscandobayesianinference_amd import _hip


class _BarNLL(torch.autograd.Function):
    """nll[r] = -log p(y[r] | logits[r,:]) with d nll / d logits = softmax(logits) - onehot(bucket)."""

    @staticmethod
    def forward(ctx, logits, y, borders, full_support):
        _hip.require_gpu_tensor(logits, 'logits')
        lib = _hip.lib()
        logits = logits.contiguous().float()
        y = y.contiguous().float().to(logits.device)
        borders = borders.contiguous().float().to(logits.device)   # a criterion left on the CPU must not hand a host pointer to the kernel
        R, nbars = logits.shape
        nll = torch.empty(R, device=logits.device, dtype=torch.float32)
        lse = torch.empty_like(nll)
        bucket = torch.empty(R, device=logits.device, dtype=torch.int32)
        _hip.check(lib.pfn_bar_nll_forward(logits.data_ptr(), nbars, y.data_ptr(), borders.data_ptr(), R, nbars,
                                           int(full_support), nll.data_ptr(), lse.data_ptr(), bucket.data_ptr(),
                                           _hip.stream_ptr(logits.device)), 'pfn_bar_nll_forward')
        ctx.save_for_backward(logits, lse, bucket)
        return nll

    @staticmethod
    def backward(ctx, gout):
        logits, lse, bucket = ctx.saved_tensors
        R, nbars = logits.shape
        gout = gout.contiguous().float()
        dlogits = torch.empty_like(logits)
        _hip.check(_hip.lib().pfn_bar_nll_backward(logits.data_ptr(), nbars, lse.data_ptr(), bucket.data_ptr(),
                                                   gout.data_ptr(), R, nbars, dlogits.data_ptr(),
                                                   _hip.stream_ptr(logits.device)), 'pfn_bar_nll_backward')
        return dlogits, None, None, None


class _BarMeanFunction(torch.autograd.Function):
    """mean = softmax(logits) . bucket means (pfn_bar_mean); backward pfn_bar_mean_backward: d mean / d logit_j = p_j (c_j - mean)."""

    @staticmethod
    def forward(ctx, flat, borders, full_support):
        out = torch.empty(flat.shape[0], device=flat.device, dtype=torch.float32)
        _hip.check(_hip.lib().pfn_bar_mean(flat.data_ptr(), flat.shape[1], borders.data_ptr(),
                                           flat.shape[0], flat.shape[1], int(full_support), out.data_ptr(),
                                           _hip.stream_ptr(flat.device)), 'pfn_bar_mean')
        ctx.save_for_backward(flat, borders, out)
        ctx.full_support = full_support
        return out

    @staticmethod
    def backward(ctx, gout):
        flat, borders, mean = ctx.saved_tensors
        gout = gout.contiguous().float()
        dlogits = torch.empty_like(flat)
        _hip.check(_hip.lib().pfn_bar_mean_backward(flat.data_ptr(), flat.shape[1], borders.data_ptr(), flat.shape[0], flat.shape[1],
                                                    int(ctx.full_support), mean.data_ptr(), gout.data_ptr(), dlogits.data_ptr(),
                                                    _hip.stream_ptr(flat.device)), 'pfn_bar_mean_backward')
        return dlogits, None, None


def _bar_mean(logits, borders, full_support):
    _hip.require_gpu_tensor(logits, 'logits')
    shape = logits.shape[:-1]
    flat = logits.reshape(-1, logits.shape[-1]).contiguous().float()
    borders = borders.detach().contiguous().float().to(flat.device)
    return _BarMeanFunction.apply(flat, borders, full_support).view(shape)


STAT_MEAN, STAT_VARIANCE, STAT_MODE, STAT_CDF, STAT_ICDF, STAT_EI_MAX, STAT_EI_MIN = range(7)      # PFN_BAR_STAT_* (include/pfn_hip.h)
MAX_STATS = 16                                                                                    # PFN_BAR_STATS_MAX
_STAT_KINDS = {'mean': STAT_MEAN, 'variance': STAT_VARIANCE, 'mode': STAT_MODE, 'cdf': STAT_CDF, 'icdf': STAT_ICDF,
               'ei': STAT_EI_MAX, 'ei_max': STAT_EI_MAX, 'ei_min': STAT_EI_MIN}
_STAT_NO_ARG = (STAT_MEAN, STAT_VARIANCE, STAT_MODE)
_SHARED_ARGS = {}


class _BarStatsFunction(torch.autograd.Function):
    """out[r, k] = statistic kinds[k] of row r (pfn_bar_stats); backward pfn_bar_stats_backward.  Differentiable in the logits only."""

    @staticmethod
    def forward(ctx, flat, borders, full_support, kinds, args, arg_ld):
        import ctypes
        R, nbars = flat.shape
        K = len(kinds)
        ckinds = (ctypes.c_int32 * K)(*kinds)
        out = torch.empty(R, K, device=flat.device, dtype=torch.float32)
        _hip.check(_hip.lib().pfn_bar_stats(flat.data_ptr(), nbars, borders.data_ptr(), R, nbars, int(full_support), ctypes.addressof(ckinds), K,
                                            args.data_ptr(), arg_ld, out.data_ptr(), _hip.stream_ptr(flat.device)), 'pfn_bar_stats')
        ctx.save_for_backward(flat, borders, args, out)
        ctx.spec = (full_support, tuple(kinds), arg_ld)
        return out

    @staticmethod
    def backward(ctx, gout):
        import ctypes
        flat, borders, args, out = ctx.saved_tensors
        full_support, kinds, arg_ld = ctx.spec
        R, nbars = flat.shape
        K = len(kinds)
        ckinds = (ctypes.c_int32 * K)(*kinds)
        gout = gout.contiguous().float()
        dlogits = torch.empty_like(flat)
        _hip.check(_hip.lib().pfn_bar_stats_backward(flat.data_ptr(), nbars, borders.data_ptr(), R, nbars, int(full_support), ctypes.addressof(ckinds), K,
                                                     args.data_ptr(), arg_ld, out.data_ptr(), gout.data_ptr(), dlogits.data_ptr(),
                                                     _hip.stream_ptr(flat.device)), 'pfn_bar_stats_backward')
        return dlogits, None, None, None, None, None


def _bar_stats(logits, borders, full_support, spec):
    _hip.require_gpu_tensor(logits, 'logits')
    spec = [(s,) if isinstance(s, str) else tuple(s) for s in spec]
    if not 1 <= len(spec) <= MAX_STATS:
        raise ValueError(f'stats: {len(spec)} statistics requested, 1 .. {MAX_STATS} per call')
    shape = logits.shape[:-1]
    flat = logits.reshape(-1, logits.shape[-1]).contiguous().float()
    R = flat.shape[0]
    kinds, vals = [], []
    for s in spec:
        name = s[0]
        if name not in _STAT_KINDS:
            raise ValueError(f'stats: unknown statistic {name!r} (one of {sorted(_STAT_KINDS)})')
        kind = _STAT_KINDS[name]
        rest = s[1:]
        if name == 'ei' and len(rest) == 2:      # ('ei', best_f, maximize)
            kind = STAT_EI_MAX if rest[1] else STAT_EI_MIN
            rest = rest[:1]
        if len(rest) != (0 if kind in _STAT_NO_ARG else 1):
            raise ValueError(f'stats: {s!r} takes {"no" if kind in _STAT_NO_ARG else "one"} argument')
        v = rest[0] if rest else 0.
        if torch.is_tensor(v) and v.requires_grad:
            raise ValueError(f'stats: the argument of {name!r} requires grad; the statistics are differentiable in the logits only')
        kinds.append(kind)
        vals.append(v)
    if any(torch.is_tensor(v) and v.numel() > 1 for v in vals):      # per-row arguments: [R, K]
        cols = [torch.broadcast_to(torch.as_tensor(v, dtype=torch.float32, device=flat.device), shape).reshape(-1) for v in vals]
        args, arg_ld = torch.stack(cols, -1).contiguous(), len(vals)
    else:      # K values shared by all rows: the device copy is kept, an evaluation loop passes the same ones again and again
        key = (tuple(float(v) for v in vals), flat.device)
        args, arg_ld = _SHARED_ARGS.get(key), 0
        if args is None:
            if len(_SHARED_ARGS) >= 256:
                _SHARED_ARGS.clear()
            args = _SHARED_ARGS[key] = torch.tensor(key[0], dtype=torch.float32).to(flat.device)
    if R == 0:
        return flat.new_empty(*shape, len(kinds))
    borders = borders.detach().contiguous().float().to(flat.device)
    return _BarStatsFunction.apply(flat, borders, full_support, kinds, args, arg_ld).view(*shape, len(kinds))


def _bar_sample(logits, borders, full_support, n, seed):
    _hip.require_gpu_tensor(logits, 'logits')
    if n < 0:
        raise ValueError(f'sample: n = {n}')
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())      # from torch's (CPU) generator: torch.manual_seed makes the draws repeatable
    shape = logits.shape[:-1]
    flat = logits.detach().reshape(-1, logits.shape[-1]).contiguous().float()
    R = flat.shape[0]
    out = torch.empty(n, R, device=flat.device, dtype=torch.float32)
    if n > 0 and R > 0:
        borders = borders.detach().contiguous().float().to(flat.device)
        _hip.check(_hip.lib().pfn_bar_sample(flat.data_ptr(), flat.shape[1], borders.data_ptr(), R, flat.shape[1], int(full_support), n,
                                             int(seed) & (2 ** 64 - 1), out.data_ptr(), _hip.stream_ptr(flat.device)), 'pfn_bar_sample')
    return out.view(n, *shape)


class BarDistribution(nn.Module):
    """Piecewise-constant density over sorted `borders` (min, ..., max); bucket k is (b_k, b_{k+1}].

    Buffers `borders` / `bucket_widths` become part of the model state-dict through
    `model.criterion` (reference train.py:45)."""
    _full_support = False

    def __init__(self, borders: torch.Tensor):
        super().__init__()
        assert len(borders.shape) == 1
        self.register_buffer('borders', borders)
        self.register_buffer('bucket_widths', self.borders[1:] - self.borders[:-1])
        span = self.borders[-1] - self.borders[0]
        assert (self.bucket_widths.sum() - span).abs() < 1e-4, f'diff: {self.bucket_widths.sum() - span}'
        assert (torch.argsort(borders) == torch.arange(len(borders), device=borders.device)).all(), "Please provide sorted borders!"
        self.num_bars = len(borders) - 1

    def map_to_bucket_idx(self, y):
        """searchsorted(borders, y) - 1 with both end points mapped inside (reference :19-23)."""
        idx = torch.searchsorted(self.borders, y) - 1
        idx[y == self.borders[0]] = 0
        idx[y == self.borders[-1]] = self.num_bars - 1
        return idx

    def forward(self, logits, y):
        """Negative log density; logits [..., num_bars], y [...] -> [...]. Out-of-support targets give
        NaN (the reference asserts, :27; a device kernel cannot)."""
        assert logits.shape[-1] == self.num_bars, f'{logits.shape[-1]} vs {self.num_bars}'
        nll = _BarNLL.apply(logits.reshape(-1, self.num_bars), y.reshape(-1), self.borders, self._full_support)
        return nll.view(y.shape)

    def bucket_means(self):
        return self.borders[:-1] + self.bucket_widths / 2

    def mean(self, logits):
        return _bar_mean(logits, self.borders, self._full_support)

    def stats(self, logits, spec):
        """Several posterior summaries in one fused pass over each logits row (pfn_bar_stats; GPU only, like `mean`): [..., K].
        `spec` lists up to 16 statistics: ('mean',), ('variance',), ('mode',), ('cdf', y), ('icdf', u), ('ei', best_f[, maximize]),
        ('ei_max', best_f), ('ei_min', best_f).  An argument is a Python float or a tensor broadcastable to logits.shape[:-1] (a best_f
        per dataset, a target per row).  Differentiable in the logits only (pfn_bar_stats_backward); an argument that requires grad raises.
        The definitions -- half-normal tails of the full-support class included -- are in the header of csrc/bar.hip."""
        assert logits.shape[-1] == self.num_bars, f'{logits.shape[-1]} vs {self.num_bars}'
        return _bar_stats(logits, self.borders, self._full_support, spec)

    def variance(self, logits):
        return self.stats(logits, [('variance',)])[..., 0]

    def cdf(self, logits, y):
        """P(Y <= y)."""
        return self.stats(logits, [('cdf', y)])[..., 0]

    def icdf(self, logits, p):
        """The level-`p` quantile: linear inside a bucket, the half-normal tails inverted for full support."""
        return self.stats(logits, [('icdf', p)])[..., 0]

    def median(self, logits):
        return self.icdf(logits, .5)

    def pi(self, logits, best_f, maximize=True):
        """Probability of improvement over `best_f`."""
        c = self.cdf(logits, best_f)
        return 1 - c if maximize else c

    def ucb(self, logits, rest_prob=.05, maximize=True):
        """Upper (lower when minimising) confidence bound: the quantile that leaves `rest_prob` beyond it."""
        return self.icdf(logits, 1 - rest_prob if maximize else rest_prob)

    def sample(self, logits, n, seed=None):
        """`n` draws per row from the predictive distribution (pfn_bar_sample): [n, ...].  Counter-based: a function of (seed, row, draw index);
        seed=None takes one from torch's generator."""
        assert logits.shape[-1] == self.num_bars, f'{logits.shape[-1]} vs {self.num_bars}'
        return _bar_sample(logits, self.borders, self._full_support, n, seed)

    def quantile(self, logits, center_prob=.682):
        """Central interval [lower, upper] with mass `center_prob`, linear inside a bucket
        (reference :40-62; vectorised over rows instead of the reference's Python loop).  Host-side PyTorch ending in .cpu();
        `stats(logits, [('icdf', side), ('icdf', 1 - side)])` is the fused, differentiable form on the device."""
        shape = logits.shape
        probs = logits.reshape(-1, shape[-1]).softmax(-1)
        side = (1 - center_prob) / 2

        def lower(p, borders):
            cum = torch.cumsum(p, -1)
            idx = torch.searchsorted(cum, torch.full_like(cum[:, :1], side)).clamp(0, cum.shape[1] - 1)
            prev = torch.where(idx > 0, cum.gather(1, (idx - 1).clamp(min=0)), cum[:, -1:])  # cum[idx-1], idx=0 wraps as in the reference
            left, right = borders[idx], borders[idx + 1]
            return (left + (right - left) * (side - prev) / p.gather(1, idx)).squeeze(1)

        lo = lower(probs, self.borders)
        hi = lower(probs.flip(-1), self.borders.flip(0))
        return torch.stack([lo, hi], -1).reshape(*shape[:-1], 2).cpu()

    def mode(self, logits):
        """Centre of the most likely bucket (reference :64-67).  The plain centre also for the two half-normal tail
        buckets of the full-support variant -- the reference does not override `mode` there."""
        return BarDistribution.bucket_means(self)[logits.argmax(-1)]

    def ei(self, logits, best_f, maximize=True):
        """Expected improvement over `best_f` under the bar density (reference :69-80)."""
        lo, hi = self.borders[:-1], self.borders[1:]
        best = torch.as_tensor(best_f, dtype=lo.dtype, device=lo.device)
        if maximize:
            contrib = ((hi + torch.maximum(lo, best)) / 2 - best).clamp(min=0)
        else:
            contrib = -((torch.minimum(hi, best) + lo) / 2 - best).clamp(max=0)
        return torch.softmax(logits, -1) @ contrib.to(logits.dtype)


class FullSupportBarDistribution(BarDistribution):
    """Bar distribution whose two outer buckets are half-normal tails (reference :83-117)."""
    _full_support = True

    @staticmethod
    def halfnormal_with_p_weight_before(range_max, p=.5):
        scale = range_max / torch.distributions.HalfNormal(torch.tensor(1.)).icdf(torch.tensor(p))
        return torch.distributions.HalfNormal(scale)

    def forward(self, logits, y):
        assert self.num_bars > 1
        return super().forward(logits, y)

    def bucket_means(self):
        means = super().bucket_means().clone()
        tails = (self.halfnormal_with_p_weight_before(self.bucket_widths[0]),
                 self.halfnormal_with_p_weight_before(self.bucket_widths[-1]))
        means[0] = -tails[0].mean + self.borders[1]
        means[-1] = tails[1].mean + self.borders[-2]
        return means


def get_bucket_limits(num_outputs: int, full_range: tuple = None, ys: torch.Tensor = None):
    """Bucket borders: equal-count quantiles of `ys` (clipped to `full_range` if given) or a uniform
    grid over `full_range` (reference :121-143). One-off host-side setup, not on the hot path."""
    assert (ys is not None) or (full_range is not None)
    if ys is None:
        width = (full_range[1] - full_range[0]) / num_outputs
        limits = torch.cat([full_range[0] + torch.arange(num_outputs).float() * width, torch.tensor(full_range[1]).unsqueeze(0)], 0)
    else:
        ys = ys.flatten()
        extra = len(ys) % num_outputs
        if extra:
            ys = ys[:-extra]
        print(f'Using {len(ys)} y evals to estimate {num_outputs} buckets. Cut off the last {extra} ys.')
        per_bucket = len(ys) // num_outputs
        if full_range is None:
            full_range = (ys.min(), ys.max())
        else:
            assert full_range[0] <= ys.min() and full_range[1] >= ys.max()
            full_range = torch.tensor(full_range)
        ordered = ys.sort(0)[0]
        inner = (ordered[per_bucket - 1::per_bucket][:-1] + ordered[per_bucket::per_bucket]) / 2
        print(full_range)
        limits = torch.cat([full_range[0].unsqueeze(0), inner, full_range[1].unsqueeze(0)], 0)
    assert len(limits) - 1 == num_outputs and full_range[0] == limits[0] and full_range[-1] == limits[-1]
    return limits
