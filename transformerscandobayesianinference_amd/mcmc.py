"""Batched NUTS on the device: `batched_nuts` drives C independent chains of the No-U-Turn sampler, every pass of its loop being ONE evaluation of the
caller's potential at every chain's own trial point followed by one call of the HIP state machine (`pfn_nuts_advance`, csrc/gp_mcmc.hip), which finishes the
leapfrog, does the tree's bookkeeping, adapts step size and mass during warmup and hands out the next trial points.  The pattern is `batched_lbfgs` of
priors.fast_gp_mix with the per-pass logic fused into one launch; the sampler knows nothing about the target.  DESIGN.md section 15 has the state machine.

Replaces what the reference gets from pyro (`NUTS(pyro_model, adapt_step_size=True)`, `MCMC(...).run`, priors/fast_gp_mix.py:185-188), one chain and one
problem at a time in Python there."""
import torch

from transformerscandobayesianinference_amd import _hip, hipops


def adaptation_windows(warmup):
    """Stan's warmup schedule as [(start, end), ...] of the slow (mass) windows, in transitions: a start buffer of 75, an end buffer of 50, a first window of
    25 that doubles; a window is stretched to the end of the slow region when the next one would not fit.  Below 150 warmup transitions the three parts
    scale to 15 % / 75 % / 10 %; below 20 there is no mass adaptation (an empty list)."""
    warmup = int(warmup)
    if warmup < 20:
        return []
    start_buffer, end_buffer, window = 75, 50, 25
    if start_buffer + window + end_buffer > warmup:
        start_buffer, end_buffer = int(0.15 * warmup), int(0.1 * warmup)
        window = warmup - start_buffer - end_buffer
    out, start, stop = [], start_buffer, warmup - end_buffer
    while start < stop:
        end = start + window
        if end + 2 * window > stop:
            end = stop
        out.append((start, end))
        start, window = end, 2 * window
    return out


@torch.no_grad()
def batched_nuts(fun, theta0, num_samples, warmup_steps, seed=0, chain_ids=None, scale=None, shift=None, D=None, step_size=0.1, target_accept=.8, max_tree_depth=10,
                 adapt_mass=True, inv_mass=None, keep_warmup=False, sync_every=16):
    """NUTS on C independent chains at once.  theta0 [C, ld] f32 on the GPU; the first D columns (all when None) are sampled, the rest is passed through to
    `fun` untouched.  fun(theta [C, ld]) -> (value [C], grad [C, ld][, info [C] int32]) evaluates all chains in one call; the potential of chain c is
    scale[c] value[c] - sum_k shift[k] theta[c, k] (scale [C], shift [D] optional), and a non-finite value or a non-zero info makes that leaf divergent.
    Chain c's history depends on (seed, chain_ids[c], its own inputs) alone (chain_ids: int64 [C], default 0 .. C-1).  Warmup: dual averaging of the
    step size from `step_size` towards `target_accept`, and with adapt_mass a diagonal mass from Stan's windows (`adaptation_windows`).  The host looks
    at the device counter of finished chains once every `sync_every` passes; the passes are bounded by (warmup + samples) 2^max_tree_depth + 1.
    Returns dict(samples [C, N, D], stats [C, W+N, 8] = (step size, mean accept probability, depth, leapfrogs, diverging, potential, 0, 0) per transition,
    inv_mass [C, D], step_size [C] (the one the sampling transitions used), evaluations, and warm [C, W, D] with keep_warmup)."""
    _hip.require_gpu_tensor(theta0, 'theta0')
    theta0 = theta0.float().contiguous()
    C, ld = theta0.shape
    D = ld if D is None else int(D)
    dev = theta0.device
    N, W = int(num_samples), int(warmup_steps)
    windows = adaptation_windows(W) if adapt_mass else []
    flags = (_hip.NUTS_ADAPT_MASS if windows else 0) | (_hip.NUTS_KEEP_WARMUP if keep_warmup else 0)
    ws = hipops.nuts_workspace(C, D, max_tree_depth, dev)
    trial = theta0.clone()      # (columns >= D travel to `fun` as they came: the kernels never touch them)
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    samples = torch.zeros(C, N, D, dtype=torch.float32, device=dev)
    stats = torch.zeros(C, W + N, 8, dtype=torch.float32, device=dev)
    warm = torch.zeros(C, W, D, dtype=torch.float32, device=dev) if keep_warmup else None
    f32 = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float32, device=dev).contiguous()
    scale, shift, inv_mass = f32(scale), f32(shift), f32(inv_mass)
    if chain_ids is not None:
        chain_ids = torch.as_tensor(chain_ids, dtype=torch.int64, device=dev).contiguous()
    hipops.nuts_init(ws, theta0, D, max_tree_depth, W, N, seed, trial, done, flags=flags, window_start=windows[0][0] if windows else 0,
                     window_ends=[e for _, e in windows], step_size=step_size, target_accept=target_accept, chain_ids=chain_ids, inv_mass=inv_mass)
    evaluations = 0
    for it in range((W + N) * 2 ** max_tree_depth + 1):
        if it % sync_every == 0 and it and int(done.item()) == C:
            break
        out = fun(trial)
        value, grad, info = out if len(out) == 3 else (out[0], out[1], None)
        evaluations += 1
        hipops.nuts_advance(ws, D, max_tree_depth, value.contiguous(), grad.contiguous(), trial, samples, stats, done, info=info, scale=scale, shift=shift, warm=warm)
    res = dict(samples=samples, stats=stats, inv_mass=hipops.nuts_inv_mass(ws, C, D).clone(), step_size=stats[:, -1, 0].clone(), evaluations=evaluations)
    if keep_warmup:
        res['warm'] = warm
    return res
