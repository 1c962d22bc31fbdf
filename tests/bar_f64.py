"""f64 reference of the bar-distribution summaries (pfn_bar_stats): plain torch on the CPU, differentiable in the logits.

Definitions (the header of that section of csrc/bar.hip): p = softmax(logits); borders b_0 < ... < b_n, w_i = b_{i+1} - b_i, C_k = sum_{i <= k} p_i;
c = HalfNormal(1).icdf(.5), s_lo = w_0 / c, s_hi = w_{n-1} / c.  g_i(y), the conditional CDF of bucket i, is clamp((y - b_i) / w_i, 0, 1) for the inner
buckets and every bucket of the bounded class; with full support g_0(y) = erfc((b_1 - y) / (s_lo sqrt 2)) below b_1 and g_{n-1}(y) = erf((y - b_{n-1}) /
(s_hi sqrt 2)) above b_{n-1}: the integral of the density whose negative log is oracle.pfn_oracle.bar_nll (tests/test_host_bar_stats.py integrates it)."""
import math

import torch

C_HALF = 0.6744897501960817
SQRT2 = math.sqrt(2.0)
SQRT_2_OVER_PI = math.sqrt(2.0 / math.pi)


def _as_rows(v, R):
    v = torch.as_tensor(v, dtype=torch.float64)
    return v.expand(R) if v.dim() == 0 else v.reshape(R)


def geometry(borders, full):
    b = borders.double()
    w = b[1:] - b[:-1]
    return b, w, w[0] / C_HALF, w[-1] / C_HALF


def bucket_cdf(borders, full, y):
    """g[r, i] = g_i(y[r])."""
    b, w, s_lo, s_hi = geometry(borders, full)
    g = ((y[:, None] - b[:-1]) / w).clamp(0, 1)
    if full:
        g0 = torch.where(y < b[1], torch.special.erfc((b[1] - y) / (s_lo * SQRT2)), torch.ones_like(y))
        gn = torch.where(y > b[-2], torch.erf((y - b[-2]) / (s_hi * SQRT2)), torch.zeros_like(y))
        g = torch.cat([g0[:, None], g[:, 1:-1], gn[:, None]], 1)
    return g


def moments(borders, full):
    """(m_i, s2_i): first and second moment of each bucket."""
    b, w, s_lo, s_hi = geometry(borders, full)
    m = b[:-1] + w / 2
    s2 = m * m + w * w / 12
    if full:
        m, s2 = m.clone(), s2.clone()
        m[0] = b[1] - s_lo * SQRT_2_OVER_PI
        s2[0] = b[1] ** 2 - 2 * b[1] * s_lo * SQRT_2_OVER_PI + s_lo ** 2
        m[-1] = b[-2] + s_hi * SQRT_2_OVER_PI
        s2[-1] = b[-2] ** 2 + 2 * b[-2] * s_hi * SQRT_2_OVER_PI + s_hi ** 2
    return m, s2


def mean(logits, borders, full):
    return torch.softmax(logits.double(), -1) @ moments(borders, full)[0]


def variance(logits, borders, full):
    p = torch.softmax(logits.double(), -1)
    m, s2 = moments(borders, full)
    return p @ s2 - (p @ m) ** 2


def cdf(logits, borders, full, y):
    p = torch.softmax(logits.double(), -1)
    return (p * bucket_cdf(borders, full, _as_rows(y, p.shape[0]))).sum(-1)


def mode(logits, borders):
    b = borders.double()
    k = logits.argmax(-1)      # the first maximum
    return (b[k] + (b[k + 1] - b[k]) / 2)


def ei(logits, borders, best_f, maximize=True):
    b = borders.double()
    lo, hi = b[:-1], b[1:]
    p = torch.softmax(logits.double(), -1)
    best = _as_rows(best_f, p.shape[0])[:, None]
    if maximize:
        contrib = ((hi + torch.maximum(lo, best)) / 2 - best).clamp(min=0)
    else:
        contrib = -((torch.minimum(hi, best) + lo) / 2 - best).clamp(max=0)
    return (p * contrib).sum(-1)


def icdf(logits, borders, full, u):
    b, w, s_lo, s_hi = geometry(borders, full)
    p = torch.softmax(logits.double(), -1)
    R, n = p.shape
    u = _as_rows(u, R)
    cum = torch.cumsum(p, -1)
    hit = (cum >= u[:, None]) & (p > 0)
    k = torch.where(hit.any(-1), hit.to(torch.int8).argmax(-1), (n - 1) - (p > 0).flip(-1).to(torch.int8).argmax(-1))
    pk = p.gather(1, k[:, None])[:, 0]
    prev = torch.where(k > 0, cum.gather(1, (k - 1).clamp(min=0)[:, None])[:, 0], torch.zeros_like(pk))
    frac = ((u - prev) / pk).clamp(0, 1)
    q = b[k] + w[k] * frac
    if full:
        q = torch.where(k == 0, b[1] - s_lo * SQRT2 * torch.special.erfinv((1 - frac).clamp(max=1 - 1e-16)), q)
        q = torch.where(k == n - 1, b[-2] + s_hi * SQRT2 * torch.special.erfinv(frac.clamp(max=1 - 1e-16)), q)
    lo_edge = -math.inf if full else b[0].item()
    hi_edge = math.inf if full else b[-1].item()
    q = torch.where(u <= 0, torch.full_like(q, lo_edge), q)
    q = torch.where(u >= 1, torch.full_like(q, hi_edge), q)
    return q


def stats(logits, borders, full, spec):
    """[R, K] f64; spec as BarDistribution.stats (arguments: floats or [R] tensors)."""
    cols = []
    for s in spec:
        name, rest = s[0], s[1:]
        if name == 'mean':
            cols.append(mean(logits, borders, full))
        elif name == 'variance':
            cols.append(variance(logits, borders, full))
        elif name == 'mode':
            cols.append(mode(logits, borders) + 0 * logits.double().sum(-1))
        elif name == 'cdf':
            cols.append(cdf(logits, borders, full, rest[0]))
        elif name == 'icdf':
            cols.append(icdf(logits, borders, full, rest[0]))
        elif name in ('ei', 'ei_max', 'ei_min'):
            maximize = name == 'ei_max' or (name == 'ei' and (len(rest) < 2 or rest[1]))
            cols.append(ei(logits, borders, rest[0], maximize))
        else:
            raise ValueError(name)
    return torch.stack(cols, -1)
