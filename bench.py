"""Benchmark of the PFN training hot path on MI355X (contract: see the task statement / DESIGN.md).

    python bench.py [--config 2|4|5] --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

`--gpus N` with N > 1 and no torchrun environment spawns the N ranks itself (same torch.distributed.run command line).

One "step" = one full training step of the selected BASELINE.json configuration on every rank: draw `batch` synthetic
datasets from the prior (HIP sampler), forward through the PFN (HIP), loss (HIP bar NLL / BCE), backward (HIP), [RCCL
all-reduce of the flat gradient], clip + Adam (HIP).  The metric is synthetic datasets / second over all ranks (weak
scaling: per-GPU batch fixed).  The default is configs[1] (the configuration the metric is quoted on).

A plain run sets up, runs W untimed and K timed steps, writes the outputs of the last timed step when --dump-outputs is given
(DIR/<name>.npy: `loss`, `parameters`, `grad_norm`, see timed_outputs) and prints the line: the contract keys, `config` and
`step_roofline` (FLOP arithmetic on the timed window, no run of its own).  Every side measurement below runs only with --full
(the --no-* flags then drop single ones of them).

With --full the JSON line also carries
  roofline     : the step's dominant kernel (picked by launches x isolated duration): `frac` / `achieved` = algorithmic FLOPs (mask-aware,
                 SURVEY.md 8(d)) / its average launch duration INSIDE the running step -- HIP event pairs around the launches on their
                 launch stream (pfn_profile_*), two micro-batch streams + the sampler sharing the chip -- vs the dense bf16 MFMA peak;
                 `isolated_*` = the same launch timed on an idle chip; `kernels` carries both for every kernel class of the step;
  other_configs: short runs (10 steps) of BASELINE configs[3] and configs[4] in the same process: datasets/s, ms per step, whole-step
                 roofline fraction, parity of inference outputs and of the timed path;
  batch_sweep  : configs[1] at per-GPU batch 4 x aggregate_k_gradients 25 (the notebook's recipe), 8, 16, 32;
  step_roofline: the same accounting for the whole step (train(S,sep) = 3 * fwd(S,sep) per dataset);
  parity_inference / parity_timed_path : the benchmarked model (its weights after the timed steps) against the f64 CPU oracle on the SAME
                 fixed-seed draw, weights and eval position, one block per PATH: inference outputs (eval mode under no_grad: exact-f32 kernels
                 by default -- what the north star's 1e-3 is asserted on; with the latency and memory that pass costs) and the forward of the
                 TIMED bf16 training path (rank 0, N = 1).  `parity` keeps the combined layout of rounds 2-3;
  val_bar_nll  : the loss of the benchmarked model on a fixed-seed validation draw (second half of BASELINE.json's metric);
  cpu_baseline : the reference's CPU path timed on the host cores on a bounded sample of the same workload from the same
                 weights and inputs (rank 0, N = 1 only): the torch nn.TransformerEncoder stack the reference instantiates
                 (kind "torch-modules", the reported value) and the explicit-math port that is the parity checker;
  allreduce_ms : (N > 1) the two collectives of the gradient buffer timed alone, back to back, after the timed steps.
"""
import argparse
import contextlib
import io
import json
import math
import os
import random
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_BF16_PEAK = 2.5e15     # dense bf16 MFMA, /opt/skills/guides/MI355X_MICROARCH.md
# committed rocprofv3 passes of THIS command per BASELINE configuration (tools/profile_bench.sh with BENCH_ARGS="--config N --precision P"): kernel trace (in-step kernel
# durations) and PMC FETCH_SIZE / WRITE_SIZE per launch.  Each file records what it profiled (config, batch, streams, precision, ABI); a file of another command is not used.
IN_STEP_TRACE = os.path.join(ROOT, 'profiles', 'r06_in_step_kernels_config{config}.json')
PMC_TRAFFIC = os.path.join(ROOT, 'profiles', 'r06_pmc_traffic_config{config}.json')
TRAINED = os.path.join(ROOT, 'profiles', 'r03_trained_config2.json')

# BASELINE.json configs (index = position in the list; 3 is configs[1] on 8 GPUs).  batch / streams: datasets per GPU per optimizer step and the micro-batch streams they
# run on -- BASELINE.json fixes neither.  Three streams of 64 (128; 8) datasets measure 3.2 % (9 %; 1.5 %) faster than two of 32 (32; 4) on one box
# (profiles/r06_step_experiments.txt, GPU calls 19 / 20: `--batch 192 --streams 3` etc.), but the GP lines stay at 64 x 2 and 8 x 2: their timed-path parity figure
# divides by the norm of the posterior means of a model that sits at the prior (rms 1e-3 .. 6e-3 against targets of rms 1: the task at 18 features is not learnable in
# a bench run), a number that moves with every change of the datasets seen -- 4.4e-4 at 64 x 2, 9.1e-4 at 192 x 3 on the same absolute error (8e-6).  The BNN line's
# means are real (rms 0.48) and it takes the larger batch.
CONFIGS = {
    2: dict(prior='fast_gp', bptt=2000, num_features=18, emsize=512, nhead=4, nhid=1024, nlayers=6, criterion='bar', num_bars=1000,
            hyperparameters=dict(noise=1e-4, outputscale=1.0, lengthscale=0.6), batch=64, streams=2, eval_pos='weighted', parity_batch=2, parity_sep=1755,
            metric='synthetic datasets/sec (GP prior, bptt=2000)',
            workload='priors.fast_gp, bptt=2000, num_features=18, emsize=512, nhead=4, nhid=1024, nlayers=6, 1000 bars (BASELINE.json configs[1])'),
    4: dict(prior='mlp', bptt=1000, num_features=60, emsize=512, nhead=4, nhid=1024, nlayers=6, criterion='bce', num_bars=1,
            hyperparameters=None, batch=384, streams=3, eval_pos='uniform', parity_batch=2, parity_sep=500,
            metric='synthetic datasets/sec (BNN prior, bptt=1000)',
            workload='priors.mlp (tabular_model_bnn BNN prior, batch_size_per_gp_sample=8), bptt=1000, num_features=60, emsize=512, nhead=4, nhid=1024, '
                     'nlayers=6, BCE head (BASELINE.json configs[3])'),
    5: dict(prior='fast_gp_mix', bptt=4000, num_features=18, emsize=1024, nhead=4, nhid=2048, nlayers=12, criterion='bar', num_bars=1000,
            hyperparameters={}, batch=8, streams=2, eval_pos='weighted', parity_batch=1, parity_sep=3549,
            metric='synthetic datasets/sec (GP-mixture prior, bptt=4000)',
            workload='priors.fast_gp_mix default hyper-prior, bptt=4000, num_features=18, emsize=1024, nhead=4 (head dim 256), nhid=2048, nlayers=12, '
                     '1000 bars (BASELINE.json configs[4])'),
}
CONFIGS[3] = CONFIGS[2]
WORKLOAD = CONFIGS[2]   # tools/ import this name


def bnn_hyperparameters():
    """The 17-tuple of the tabular_model_bnn configuration (reference tabular.py:47-70)."""
    from transformerscandobayesianinference_amd.priors.utils import gamma_sampler_f, scaled_beta_sampler_f
    return (lambda: 3, scaled_beta_sampler_f(2., 4., 150, 2), torch.nn.Tanh, gamma_sampler_f(3.6187797729244253, 0.06773738681062867),
            gamma_sampler_f(1.8663049257557085, 0.05275478076173361), lambda: 0.0, True, scaled_beta_sampler_f(1., 1.6, 60, 2),
            None, False, None, None, None, True, False, lambda n: ([], []), 0.0)


def pairs(S, sep):
    return S * sep + (S - sep)


def fwd_flops(S, sep, nf, E, F, L, n_out, top_rows_only=False):
    """Algorithmic forward FLOPs of one dataset: embeddings, L layers with mask-aware
    attention, decoder on the test rows only.  top_rows_only: the top layer's train rows feed nothing (the reference returns
    output[single_eval_pos:]) and the stack does not compute them -- that layer then counts its K / V projection on every row and
    everything else (Q projection, attention, out_proj, FFN) on the S - sep test rows."""
    layer = 6 * S * E * E + 4 * E * pairs(S, sep) + 2 * S * E * E + 4 * S * E * F
    T = S - sep
    top = (4 * S * E * E + 2 * T * E * E + 4 * E * (T * sep + T) + 2 * T * E * E + 4 * T * E * F) if (top_rows_only and L > 0) else layer
    return (2 * S * nf * E + 2 * sep * E + max(L - 1, 0) * layer + (top if L > 0 else 0)
            + (S - sep) * (2 * E * F + 2 * F * n_out))


def train_flops(S, sep, nf, E, F, L, n_out, top_rows_only=False):
    return 3 * fwd_flops(S, sep, nf, E, F, L, n_out, top_rows_only)


def quiet():
    """The reference's loaders / get_bucket_limits print; stdout carries the JSON line only."""
    return contextlib.redirect_stdout(io.StringIO())


def prior_module(w):
    from transformerscandobayesianinference_amd.priors import fast_gp, fast_gp_mix, mlp
    return {'fast_gp': fast_gp, 'fast_gp_mix': fast_gp_mix, 'mlp': mlp}[w['prior']]


def prior_kwargs(w):
    kw = dict(num_features=w['num_features'])
    if w['prior'] == 'mlp':
        kw.update(hyperparameters=bnn_hyperparameters(), batch_size_per_gp_sample=8)
    else:
        kw.update(hyperparameters=w['hyperparameters'])
    return kw


def make_criterion(w, device):
    from transformerscandobayesianinference_amd import bar_distribution
    if w['criterion'] == 'bce':
        return torch.nn.BCEWithLogitsLoss(reduction='none')
    ys = prior_module(w).get_batch(5000 if w['prior'] == 'fast_gp' else 1000, 20, w['num_features'], device=device, hyperparameters=w['hyperparameters'])[1]
    with quiet():
        borders = bar_distribution.get_bucket_limits(w['num_bars'], ys=ys.cpu())
    return bar_distribution.FullSupportBarDistribution(borders)


def loss_of(w, criterion):
    """per-(position, dataset) losses of the test rows, as train.py's compute_losses does"""
    O = w['num_bars']
    if w['criterion'] == 'bce':
        return lambda out, tg: criterion(out.squeeze(-1), tg)
    return lambda out, tg: criterion(out.reshape(-1, O), tg.reshape(-1)).view(out.shape[0], -1)


def build_model(device, precision, w=WORKLOAD, criterion=None):
    from transformerscandobayesianinference_amd import encoders
    from transformerscandobayesianinference_amd.transformer import TransformerModel
    torch.manual_seed(0)
    criterion = criterion if criterion is not None else make_criterion(w, device)
    model = TransformerModel(encoders.Linear(w['num_features'], w['emsize']), w['num_bars'], w['emsize'], w['nhead'], w['nhid'],
                             w['nlayers'], 0.0, y_encoder=encoders.Linear(1, w['emsize']), precision=precision,
                             deterministic=os.environ.get('PFN_BENCH_DETERMINISTIC') == '1')      # (experiment hook: the bit-reproducible schedule's cost)
    model.criterion = criterion
    with torch.no_grad():  # random-init weights of the named architecture; un-zero the residual branches so all kernels see real data
        for layer in model.transformer_encoder.layers:
            layer.linear2.weight.normal_(0, 0.02)
            layer.self_attn.out_proj.weight.normal_(0, 0.02)
    return model.to(device)


_spin = {}


def run_ahead(ms=1.5):
    """Keeps the GPU busy for ~`ms` (a spin kernel, calibrated once) so that the host enqueues the launches and events that follow while it runs:
    they then execute back to back, and an event-to-event interval holds the kernel between the two events and no host gap.  (Without it a slow
    host shows up inside the intervals of short sequences: the key-block pass behind the 30-us delta kernel read 526 us on one box and 646 on
    another whose whole step was FASTER; the three launches enqueued as one call took 793 us on both.)"""
    if 'cycles_per_ms' not in _spin:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(10000)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(1000000)
        b.record()
        b.synchronize()
        _spin['cycles_per_ms'] = 1000000 / max(a.elapsed_time(b), 1e-3)
    torch.cuda._sleep(int(ms * _spin['cycles_per_ms']))


def time_kernel(fn, iters=10, warm=3):
    """Average duration (s) of fn() with HIP events recorded on the stream the kernels run on."""
    for _ in range(warm):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    run_ahead()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / 1e3 / iters


def time_sequence(fns, iters=10, warm=3):
    """Average duration (s) of each fn() of a launch SEQUENCE run back to back, `iters` times, with a HIP event between consecutive launches
    on the launch stream: every kernel is timed in the context it runs in (the attention backward's key-block pass is always followed
    by the query-block pass that reads what it wrote; the same launch repeated on its own queues ten 0.9 GB write bursts behind each
    other and reads 530-660 us by box where the sequence gives 525-570)."""
    for _ in range(warm):
        for fn in fns:
            fn()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(iters)]
    for it in range(iters):
        run_ahead()
        ev[it][0].record()
        for j, fn in enumerate(fns):
            fn()
            ev[it][j + 1].record()
    torch.cuda.synchronize()
    return [sum(ev[it][j].elapsed_time(ev[it][j + 1]) for it in range(iters)) / iters / 1e3 for j in range(len(fns))]


def kernel_breakdown(batch, sep, w=WORKLOAD, fused_ln_wide=False, top_rows=None, precision='bf16'):
    """Isolated timings of the step's kernels at the workload shape (through the single-op C ABI): one entry per kernel
    symbol, with the number of launches per step, so the dominant one can be picked by in-step time.  top_rows (pfn_top_layer_rows): the rows
    the top layer runs on behind its K / V projection -- when that is the (S - sep) * batch test rows, L - 1 launches of every row-wise kernel
    run on all rows and one on those (separate entries)."""
    from transformerscandobayesianinference_amd import _hip
    from transformerscandobayesianinference_amd import hipops
    dev = torch.device('cuda')
    S, E, F, H, L = w['bptt'], w['emsize'], w['nhid'], w['nhead'], w['nlayers']
    M = batch * S
    Mt = M if top_rows is None else int(top_rows)
    top = Mt != M                      # the top layer on the test rows only
    Lf = L - 1 if top else L           # launches of a per-layer kernel on all rows
    PREC = _hip.PRECISIONS[precision]      # the 16-bit operand format of the timed path (bf16 / fp16: the same kernels, instantiated per format)
    bf = hipops.TDT[PREC]
    tmangle = hipops.MANGLED_OPERAND[PREC]
    r = lambda *s: (torch.randn(*s, device=dev) * 0.5).to(bf)
    f32 = lambda *s: torch.randn(*s, device=dev)
    Hh = _hip
    out = []

    def add(kernel, rocprof, seconds, flops, count, executed=None, nbytes=None, prof=None):
        # nbytes: ALGORITHMIC HBM bytes of one launch (every operand read once, every output written once); its floor at the 6.3 TB/s
        # a stream achieves on this part (MI355X_MICROARCH.md) next to the MFMA floor says which of the two bounds the launch
        # prof: the library's in-step timing class of this launch (PROF_SLOTS; main() adds `in_step_us` from the profiled steps)
        out.append(dict(kernel=kernel, rocprof_name=rocprof, prof_class=prof, launches_per_step=count, seconds=seconds, flops=flops,
                        executed_flops=executed if executed is not None else flops, bytes=nbytes,
                        hbm_floor_us=None if nbytes is None else nbytes / 6.3e12 * 1e6, mfma_floor_us=flops / MFMA_BF16_PEAK * 1e6))

    def gemm(name, n, k, flags, count, M=M, prof=None):
        """One encoder GEMM with its REAL epilogue (bias / GELU / residual / output streams), M = batch * bptt rows."""
        if count <= 0 or M <= 0:
            return
        A, B_ = r(M, k), r(n, k)
        kw = {}
        if flags & Hh.EPI_BIAS: kw['bias'] = f32(n)
        if flags & Hh.EPI_RESID: kw['resid'] = f32(M, n)
        if flags & (Hh.EPI_GELU_BWD | Hh.EPI_RESID_T): kw['aux'] = r(M, n)
        if flags & Hh.EPI_OUT_F32: kw['out_f32'] = torch.empty(M, n, device=dev)
        if flags & Hh.EPI_OUT_T: kw['out_t'] = torch.empty(M, n, dtype=bf, device=dev)
        if flags & Hh.EPI_OUT2_T: kw['out2_t'] = torch.empty(M, n, dtype=bf, device=dev)
        t = time_kernel(lambda: hipops.gemm_nt(A, B_, flags, PREC, **kw))
        nbytes = sum(v.numel() * v.element_size() for v in [A, B_] + list(kw.values()))
        add(f'gemm_nt[{name} {M}x{n}x{k}]', f'_ZN3pfn18gemm_nt_big_kernelI{tmangle}Li{flags}E', t, 2.0 * M * n * k, count, nbytes=nbytes, prof=prof)

    def gemm_ln(name, k, count, M=M, prof=None):
        """out_proj / linear2 with bias + residual + LayerNorm in the epilogue (the kernel the step runs when emsize allows)."""
        if E > 512 and not fused_ln_wide:      # emsize 1024: the stack runs GEMM + LayerNorm kernels unless PFN_TUNE_FUSE_LN_WIDE is set (measured faster)
            return False
        if count <= 0 or M <= 0:
            return True
        A, B_ = r(M, k), r(E, k)
        bias, gamma, beta, resid = f32(E), f32(E), f32(E), f32(M, E)
        sums16 = precision == 'fp16'      # (fp16 models keep the pre-LayerNorm sums in operand precision: PFN_OP_SUMS_16BIT, what the step launches)
        bufs = (torch.empty(M + 2, E, dtype=bf if sums16 else torch.float32, device=dev), torch.empty(M, E, dtype=bf, device=dev), torch.empty(M, device=dev), torch.empty(M, device=dev))
        try:
            t = time_kernel(lambda: hipops.gemm_ln(A, B_, bias, gamma, beta, 1e-5, resid=resid, out=bufs, sums16=sums16))
        except _hip.HipExtensionError:   # shape outside the fused kernel (emsize 1024): the step runs GEMM + LayerNorm kernels there
            return False
        nbytes = sum(v.numel() * v.element_size() for v in (A, B_, resid) + bufs)     # operands, f32 residual in, f32 sum + bf16 LN output + statistics out
        add(f'gemm_nt_ln[{name} + residual + LayerNorm {M}x{E}x{k}]', 'gemm_nt_ln_kernel', t, 2.0 * M * E * k, count, nbytes=nbytes, prof=prof)
        return True

    def gemm_lnbwd(name, k, count, M=M, prof=None):
        """a data-gradient GEMM with the backward of the LayerNorm it feeds in the epilogue (what the step runs when emsize allows)"""
        if E > 512 and not fused_ln_wide:
            return False
        if count <= 0 or M <= 0:
            return True
        A, B_, aux = r(M, k), r(E, k), r(M, E)
        y, gamma = f32(M, E), f32(E)
        mean, rstd = y.mean(1), 1 / torch.sqrt(y.var(1, unbiased=False) + 1e-5)
        if precision == 'fp16':
            y = y.to(bf)
        bufs = (torch.empty(M, E, dtype=bf, device=dev), torch.zeros(E, device=dev), torch.zeros(E, device=dev))
        try:
            t = time_kernel(lambda: hipops.gemm_lnbwd(A, B_, aux, y, mean, rstd, gamma, out=bufs))
        except _hip.HipExtensionError:
            return False
        nbytes = sum(v.numel() * v.element_size() for v in (A, B_, aux, y, mean, rstd, bufs[0]))
        add(f'gemm_nt_lnbwd[{name} {M}x{E}x{k}]', 'gemm_nt_lnbwd_kernel', t, 2.0 * M * E * k, count, nbytes=nbytes, prof=prof)
        return True

    def layernorm_bwd(count, M=M):
        if count <= 0 or M <= 0:
            return
        gA, y, gamma = r(M, E), f32(M, E), f32(E)
        mean, rstd = y.mean(1), 1 / torch.sqrt(y.var(1, unbiased=False) + 1e-5)
        t = time_kernel(lambda: hipops.layernorm_bwd(gA, y, gamma, mean, rstd, PREC, want_f32=False))
        add(f'layernorm_bwd[{M}x{E}, operand-precision gradient in and out]', 'layernorm_bwd_kernel', t, 0.0, count)

    def layernorm_fwd(count, M=M):
        if count <= 0 or M <= 0:
            return
        x, gamma, beta = f32(M, E), f32(E), f32(E)
        t = time_kernel(lambda: hipops.layernorm_fwd(x, gamma, beta, 1e-5, PREC))
        add(f'layernorm_fwd[{M}x{E}: f32 in, f32 + operand-precision out]', 'layernorm_fwd_kernel', t, 0.0, count, nbytes=M * E * (4 + 4 + 2))

    def wgrad_group():
        # every weight gradient of the stack in ONE grouped launch (pfn_stack_backward defers them); a top layer on the test rows contributes its
        # K / V / Q projection's gradient there and its other three as a second, short launch over the test rows
        probs = []
        for l in range(L):
            if not (top and l == L - 1):
                probs += [(r(M, E), r(M, F), torch.zeros(E, F, device=dev), None), (r(M, F), r(M, E), torch.zeros(F, E, device=dev), torch.zeros(F, device=dev)),
                          (r(M, E), r(M, E), torch.zeros(E, E, device=dev), None)]
            probs += [(r(M, 3 * E), r(M, E), torch.zeros(3 * E, E, device=dev), torch.zeros(3 * E, device=dev))]
        nmax = 26
        launches = [probs[i:i + nmax] for i in range(0, len(probs), nmax)]
        t = time_kernel(lambda: [hipops.gemm_tn_group(g, 0) for g in launches], iters=5, warm=2)
        add(f'gemm_tn_group[{len(probs)} weight gradients, {M} tokens, {len(launches)} launch(es)]', 'gemm_tn_big_kernel', t / len(launches),
            2.0 * M * (Lf * (2 * E * F + E * E) + L * 3 * E * E) / len(launches), len(launches), prof='gemm_tn_group')
        if top:
            tp = [(r(Mt, E), r(Mt, F), torch.zeros(E, F, device=dev), None), (r(Mt, F), r(Mt, E), torch.zeros(F, E, device=dev), torch.zeros(F, device=dev)),
                  (r(Mt, E), r(Mt, E), torch.zeros(E, E, device=dev), None)]
            t = time_kernel(lambda: hipops.gemm_tn_group(tp, 0), iters=5, warm=2)
            add(f'gemm_tn_group[top layer: 3 weight gradients, {Mt} test rows]', 'gemm_tn_big_kernel', t, 2.0 * Mt * (2 * E * F + E * E), 1, prof='gemm_tn_group [top layer: test rows]')

    # (`rows`: every per-layer kernel runs Lf times on all rows and, with the top layer on the test rows, once more on those)
    for rows, cnt, tag in ([(M, Lf, '')] + ([(Mt, 1, 'top layer, test rows: ')] if top else [])):
        sfx = ' [top layer: test rows]' if tag else ''       # the library's in-step timing class of the compact-row launches (PROF_SLOTS + 1)
        if rows == M:
            gemm('qkv', 3 * E, E, Hh.EPI_BIAS | Hh.EPI_OUT_T, L, prof='gemm_qkv')
        if not gemm_ln(tag + 'out_proj', E, cnt, rows, prof='gemm_out_proj_ln' + sfx):
            gemm(tag + 'out_proj + residual', E, E, Hh.EPI_BIAS | Hh.EPI_RESID | Hh.EPI_OUT_F32, cnt, rows)
            layernorm_fwd(2 * cnt, rows)
        gemm(tag + 'linear1 + GELU', F, E, Hh.EPI_BIAS | Hh.EPI_GELU | Hh.EPI_OUT_T | Hh.EPI_OUT2_T, cnt, rows, prof='gemm_linear1_gelu' + sfx)
        if not gemm_ln(tag + 'linear2', F, cnt, rows, prof='gemm_linear2_ln' + sfx):
            gemm(tag + 'linear2 + residual', E, F, Hh.EPI_BIAS | Hh.EPI_RESID | Hh.EPI_OUT_F32, cnt, rows)
        gemm(tag + 'd(hpre) = dy2.W2 * gelu\'', F, E, Hh.EPI_GELU_BWD | Hh.EPI_OUT_T, cnt, rows, prof='gemm_dhpre' + sfx)
        if gemm_lnbwd(tag + 'dy1 = LN1 backward of dh.W1 + dy2', F, cnt, rows, prof='gemm_dy1_lnbwd' + sfx):
            if rows == M:
                if L > 1:
                    gemm_lnbwd('dy2 = LN2 backward (layer below) of dqkv.Win + dy1', 3 * E, L - 1, prof='gemm_dx_lnbwd')
                gemm('dx = dqkv.Win + dy1 (first layer: gradient of the embedding output)', E, 3 * E, Hh.EPI_RESID_T | Hh.EPI_OUT_T, 1)
            if rows == Mt:
                layernorm_bwd(1, rows)          # the top LayerNorm's backward (its gradient comes from the decoder)
        else:
            gemm(tag + 'dx1 = dh.W1 + dy2', E, F, Hh.EPI_RESID_T | Hh.EPI_OUT_T, cnt, rows)
            if rows == M:
                gemm('dx = dqkv.Win + dy1', E, 3 * E, Hh.EPI_RESID_T | Hh.EPI_OUT_T, L)
            layernorm_bwd(2 * cnt, rows)
        gemm(tag + 'd(ctx) = dy1.Wo', E, E, Hh.EPI_OUT_T, cnt, rows, prof='gemm_dctx' + sfx)
    wgrad_group()
    qkv = r(batch, S, 3 * E)
    D = E // H
    unit = 2.0 * E * pairs(S, sep) * batch          # one S x keys x head-dim product over all heads
    ctx, lse = hipops.attention_fwd(qkv, H, sep, PREC)
    dctx = r(batch, S, E)
    if Lf > 0:
        t = time_kernel(lambda: hipops.attention_fwd(qkv, H, sep, PREC))
        add('attn_fwd', hipops.ATTENTION_FWD_ROCPROF.format(D=D, T=tmangle), t, 2 * unit, Lf, prof='attn_fwd')
        # the backward's three launches, each timed inside their sequence (delta, key-block pass, query-block pass back to back)
        seq = time_sequence([(lambda part=part: hipops.attention_bwd(qkv, ctx, lse, dctx, H, sep, PREC, parts=part))
                             for _, _, part, _, _ in hipops.ATTENTION_BWD_PARTS])
        for (name, rocprof, part, alg_units, exec_units), t in zip(hipops.ATTENTION_BWD_PARTS, seq):
            rocprof = rocprof.format(D=D, T=tmangle)
            if part == 2:
                exec_units = hipops.ATTENTION_BWD_KV_EXECUTED_UNITS.get(D, exec_units)
            add(name, rocprof, t, alg_units * unit, Lf, exec_units * unit, prof={1: 'attn_bwd_delta', 2: 'attn_bwd_kv', 4: 'attn_bwd_dq'}[part])
    if top:
        # the top layer's attention: the queries >= sep only (q_begin; the kernels start at the query block that holds sep)
        unit_t = 2.0 * E * ((S - sep) * sep + (S - sep)) * batch
        q0 = sep // 256 * 256
        unit_x = 2.0 * E * ((S - q0) * sep + (S - sep)) * batch          # executed: whole query blocks
        dctx_t = dctx.clone()
        dctx_t[:, :sep] = 0
        bufs_t = (torch.empty_like(ctx), torch.empty_like(lse))
        t = time_kernel(lambda: hipops.attention_fwd(qkv, H, sep, PREC, q_begin=sep, out=bufs_t))
        add('top layer: attn_fwd for the queries >= sep', hipops.ATTENTION_FWD_ROCPROF.format(D=D, T=tmangle), t, 2 * unit_t, 1, 2 * unit_x, prof='attn_fwd [top layer: test rows]')
        seq = time_sequence([(lambda part=part: hipops.attention_bwd(qkv, ctx, lse, dctx_t, H, sep, PREC, parts=part, q_begin=sep))
                             for _, _, part, _, _ in hipops.ATTENTION_BWD_PARTS])
        for (name, rocprof, part, alg_units, exec_units), t in zip(hipops.ATTENTION_BWD_PARTS, seq):
            if part == 2:
                exec_units = hipops.ATTENTION_BWD_KV_EXECUTED_UNITS.get(D, exec_units)
            add('top layer, queries >= sep: ' + name, rocprof.format(D=D, T=tmangle), t, alg_units * unit_t, 1, exec_units * unit_x,
                prof={1: 'attn_bwd_delta', 2: 'attn_bwd_kv', 4: 'attn_bwd_dq'}[part] + ' [top layer: test rows]')
        # ... and its row moves: attention output / layer input gathered, d(attention output) / LayerNorm-input gradient scattered back
        c_t, y32 = r(batch, S, E), f32(batch, S, E)
        g_t = r(Mt, E)
        o1, o2, o3 = torch.empty(Mt, E, dtype=bf, device=dev), torch.empty(Mt, E, device=dev), torch.empty(batch, S, E, dtype=bf, device=dev)
        t = time_kernel(lambda: (hipops.gather_rows(c_t, sep, out=o1), hipops.gather_rows(y32, sep, out=o2), hipops.scatter_rows(g_t, batch, S, sep, q0, out=o3),
                                 hipops.scatter_rows(g_t, batch, S, sep, 0, out=o3)))
        add('top layer: test rows gathered (attention output, layer input) and scattered back (2 gradients)', 'gather_rows_kernel / scatter_rows_kernel', t, 0.0, 1,
            nbytes=(S - sep) * batch * E * (2 * 2 + 4 * 2 + 2 + 2) + M * E * 2)
    t = time_kernel(lambda: hipops.attention_bwd(qkv, ctx, lse, dctx, H, sep, PREC, parts=7))
    out.append(dict(kernel='attn_bwd (whole launch set, for reference)', rocprof_name='attn_bwd_* + attn_delta_kernel', launches_per_step=0,
                    seconds=t, flops=4 * unit, executed_flops=(hipops.ATTENTION_BWD_KV_EXECUTED_UNITS.get(D, 4.0) + 1.0) * unit))
    for k in out:
        k['tflops'] = k['flops'] / k['seconds'] / 1e12
        k['executed_tflops'] = k['executed_flops'] / k['seconds'] / 1e12
        k['step_seconds'] = k['seconds'] * k['launches_per_step']
    return out


def usable_cores(cap=32):
    """Host cores this process may really use: affinity mask, cgroup CPU quota, capped (torch's intra-op
    pool degrades badly when it is given more threads than the cgroup grants)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()
        if quota != 'max':
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, cap))


# ---- parity + CPU baseline (rank 0, N = 1): both paths on the same fixed-seed inputs and the same weights -------------------
def parity_inputs(w, device, seed=1234):
    """(x[T,B,F], y[T,B]) on the CPU in f64: a fixed-seed draw of the configuration's prior.  GP priors: the oracle's own
    sampler (f64 Cholesky on the host).  BNN prior: no host port of the sampler exists, the fixed-seed draw comes from the HIP
    sampler and both paths then read the same tensors."""
    from oracle import pfn_oracle
    B, S, nf = w['parity_batch'], w['bptt'], w['num_features']
    gen = torch.Generator().manual_seed(seed)
    if w['prior'] == 'fast_gp':
        x, y, _ = pfn_oracle.get_batch_fast_gp(B, S, nf, w['hyperparameters'], gen, dtype=torch.float64)
        return x.double(), y.double()
    if w['prior'] == 'fast_gp_mix':
        from transformerscandobayesianinference_amd.priors import fast_gp_mix
        ls, osc, nz = fast_gp_mix.sample_hyperparameters(B, nf, w['hyperparameters'], 'cpu', generator=gen)
        x = torch.rand(B, S, nf, generator=gen)
        z = torch.randn(B, S, generator=gen)
        y = pfn_oracle.gp_sample(x, z, ls.double(), osc.double(), nz.double(), 'matern', torch.float64)
        return x.transpose(0, 1).double(), y.transpose(0, 1).double()
    import numpy as np
    from transformerscandobayesianinference_amd.priors import mlp
    state = (torch.random.get_rng_state(), random.getstate(), np.random.get_state())
    torch.manual_seed(seed); random.seed(seed); np.random.seed(seed)
    x, y, _ = mlp.get_batch(8, S, nf, device=device, **{k: v for k, v in prior_kwargs(w).items() if k != 'num_features'})
    torch.random.set_rng_state(state[0]); random.setstate(state[1]); np.random.set_state(state[2])
    return x[:, :B].double().cpu(), y[:, :B].double().cpu()


def oracle_loss_and_means(w, sd, logits, y_test):
    from oracle import pfn_oracle
    if w['criterion'] == 'bce':
        z = logits.squeeze(-1)
        return torch.nn.functional.binary_cross_entropy_with_logits(z, y_test.to(z.dtype), reduction='none'), torch.sigmoid(z)
    borders = sd['criterion.borders'].to(logits.dtype)
    return (pfn_oracle.bar_nll(logits.reshape(-1, w['num_bars']), y_test.reshape(-1), borders).view(logits.shape[:2]),
            pfn_oracle.bar_mean(logits, borders))


def hip_loss_and_means(w, model, logits, y_test):
    if w['criterion'] == 'bce':
        z = logits.squeeze(-1)
        return model.criterion(z, y_test), torch.sigmoid(z)
    return model.criterion(logits.reshape(-1, w['num_bars']), y_test.reshape(-1)).view(logits.shape[:2]), model.criterion.mean(logits)


def parity_check(model, w, device, precision):
    """HIP path (benchmarked weights) vs the f64 oracle on the same inputs, twice:
      * the model's INFERENCE outputs -- model.eval() under no_grad, what validate / run_test / criterion.mean serve; these run in
        `model.eval_precision` (exact-f32 kernels by default) and carry the north star's 1e-3 bound on NLL and posterior means;
      * `training_forward`: the forward of the TIMED path (train mode, benchmarked precision), same inputs, reported beside it."""
    from oracle import pfn_oracle
    x, y = parity_inputs(w, device)
    sep = w['parity_sep']
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    was_training = model.training
    xd, yd = x.float().to(device), y.float().to(device)

    def hip(train_mode):
        model.train(train_mode)
        with torch.no_grad():
            lg = model((xd, yd), single_eval_pos=sep)
            loss_h, mean_h = hip_loss_and_means(w, model, lg, yd[sep:])
        return lg.double().cpu(), loss_h.double().cpu(), mean_h.double().cpu()

    out_eval, out_train = hip(False), hip(True)
    model.train(was_training)
    t0 = time.time()
    with torch.no_grad():
        lo = pfn_oracle.forward({k: v for k, v in sd.items() if not k.startswith('criterion.')}, x, y, sep, w['nhead'], dtype=torch.float64)
        loss_o, mean_o = oracle_loss_and_means(w, sd, lo, y[sep:])
    oracle_s = time.time() - t0
    y_test = y[sep:]
    nll_o = loss_o.mean().item()

    def metrics(lg, loss_h, mean_h):
        d = mean_h - mean_o
        nll_h = loss_h.mean().item()
        return dict(
            nll_hip=nll_h, nll_oracle=nll_o, nll_rel=abs(nll_h - nll_o) / abs(nll_o),
            nll_per_row_max_abs=(loss_h - loss_o).abs().max().item(),
            logits_rel_l2=((lg - lo).norm() / lo.norm()).item(),
            mean_rel_l2=(d.norm() / mean_o.norm()).item(),                                   # relative to the means' own norm
            mean_max_over_range=(d.abs().max() / (mean_o.max() - mean_o.min())).item(),       # ... to the spread of the reference means
            mean_rel_l2_vs_targets=(d.norm() / y_test.norm()).item(),                        # ... to the scale of the predicted quantity
            mean_max_over_y_range=(d.abs().max() / (y.max() - y.min())).item(),
            mean_abs_max=d.abs().max().item())

    eval_prec = getattr(model, 'eval_precision', None) or precision
    if getattr(model, '_eval_desc', None) is None:
        eval_prec = precision                     # no separate inference precision configured / supported at this shape
    res = dict(
        against='oracle/pfn_oracle.py forward + loss in f64 on the host (pinned to the reference modules by tests/golden)',
        inputs=f"fixed-seed draw of the configuration's prior (seed 1234), {w['parity_batch']} dataset(s), bptt {w['bptt']}, eval position {sep}; "
               f"weights = the benchmarked model's after the timed steps",
        precision=eval_prec, outputs='model.eval() under no_grad (inference passes run in model.eval_precision)',
        **metrics(*out_eval),
        mean_ref_rms=mean_o.pow(2).mean().sqrt().item(), y_test_rms=y_test.pow(2).mean().sqrt().item(), oracle_forward_s=oracle_s,
        training_forward=dict(precision=precision, note='forward of the timed path (train mode) on the same inputs and weights', **metrics(*out_train)))
    return res, (x, y, sd)


def cpu_baseline(w, inputs, steps=3, warm=1):
    """The reference's CPU path on the host cores, two legs, each a few full training steps ([prior draw +] forward + loss +
    backward + clip + Adam) at the workload shape from the benchmarked weights and the parity inputs:
      torch-modules : the model as the reference BUILDS it -- torch's nn.TransformerEncoder(nn.TransformerEncoderLayer(...,
                      activation='gelu')) with the dense host-built mask, embeddings and decoder on all rows
                      (oracle/torch_modules.py; reference transformer.py:14-25, 55-91).  torch's modules take fused CPU kernels,
                      so this is what a user of the reference gets on these cores: THE reported baseline.
      port          : the explicit-math restatement that serves as the parity checker (oracle/pfn_oracle.py), for comparison."""
    from oracle import pfn_oracle, torch_modules
    x0, y0, sd = inputs
    threads = usable_cores()
    torch.set_num_threads(threads)
    S, nf, B = w['bptt'], w['num_features'], x0.shape[1]
    if w['prior'] == 'fast_gp_mix':
        steps, warm = 1, 0
    sep = w['parity_sep']

    def draw(it):
        if it == 0 or w['prior'] == 'mlp':
            return x0.float(), y0.float()            # the parity inputs (BNN prior: no host port of the sampler -- draw time not included)
        if w['prior'] == 'fast_gp':
            x, y, _ = pfn_oracle.get_batch_fast_gp(B, S, nf, w['hyperparameters'], dtype=torch.float32)
            return x, y
        from transformerscandobayesianinference_amd.priors import fast_gp_mix
        ls, osc, nz = fast_gp_mix.sample_hyperparameters(B, nf, w['hyperparameters'], 'cpu', generator=torch.Generator().manual_seed(it))
        y = pfn_oracle.gp_sample(torch.rand(B, S, nf), torch.randn(B, S), ls, osc, nz, 'matern', torch.float32).float().transpose(0, 1)
        return x0.float(), y

    def leg(kind):
        torch.manual_seed(0)
        if kind == 'port':
            params = {k: v.detach().float().clone().requires_grad_(True) for k, v in sd.items() if not k.startswith('criterion.')}
            plist = list(params.values())
            fwd = lambda x, y: pfn_oracle.forward(params, x, y, sep, w['nhead'], dtype=torch.float32)
        else:
            module = torch_modules.from_state_dict(sd, w['nhead']).train()
            plist = list(module.parameters())
            fwd = lambda x, y: module((x, y), sep)
        opt = torch.optim.Adam(plist, lr=1e-4)
        times, loss0 = [], None
        for it in range(warm + steps):
            t0 = time.time()
            x, y = draw(it)
            logits = fwd(x, y)
            loss = oracle_loss_and_means(w, sd, logits, y[sep:])[0].mean()
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(plist, 1.0)
            opt.step()
            if it == 0:
                loss0 = loss.item()
            if it >= warm:
                times.append(time.time() - t0)
        per_step = sum(times) / len(times)
        return dict(kind=kind, value=B / per_step, unit='datasets/s', seconds_per_step=per_step, first_step_loss=loss0)

    legs = [leg('torch-modules'), leg('port')]
    note = ' (BNN prior draw not included: the reference sampler is per-dataset Python, 57 datasets/s in BASELINE.md)' if w['prior'] == 'mlp' else ''
    best = max(legs, key=lambda l: l['value'])     # the faster leg is the honest baseline (torch-modules on every box seen so far)
    return dict(value=best['value'], unit='datasets/s', cores=threads, kind='port', port=best['kind'],
                sample_short=f'{steps} full training steps (draw+fwd+loss+bwd+clip+Adam), batch {B}, bptt {S}, sep {sep}, torch f32, leg {best["kind"]}',
                sample=f'{steps} full training step(s) (prior draw + fwd + loss + bwd + clip + Adam), batch {B}, bptt {S}, eval position {sep}, torch f32 on the '
                       f'host cores from the benchmarked weights; step 0 reads the parity inputs.  kind "torch-modules" = the nn.TransformerEncoder stack the '
                       f'reference instantiates (transformer.py:17-18) with its dense mask and all-row decoder; the explicit-math port (the parity checker) is '
                       f'timed beside it in `legs`' + note,
                seconds_per_step=best['seconds_per_step'], legs=legs,
                legs_agree=abs(legs[0]['first_step_loss'] - legs[1]['first_step_loss']) / abs(legs[1]['first_step_loss']))


def validation_loss(model, w, device, n=8, seed=4321):
    """Loss of the benchmarked model on a fixed-seed validation draw at the configuration's typical eval position."""
    w2 = dict(w, parity_batch=n if w['prior'] != 'fast_gp_mix' else 4)
    x, y = parity_inputs(w2, device, seed=seed)
    sep = w['parity_sep']
    was_training = model.training
    model.eval()
    with torch.no_grad():
        xd, yd = x.float().to(device), y.float().to(device)
        loss = hip_loss_and_means(w, model, model((xd, yd), single_eval_pos=sep), yd[sep:])[0].mean().item()
    model.train(was_training)
    out = dict(value=loss, datasets=x.shape[1], eval_position=sep, seed=seed, checkpoint='none: random initialisation + the optimizer steps of this run',
               note='bar NLL (BCE for the BNN configuration) of the benchmarked model -- random initialisation plus the few optimizer steps of this '
                    'run -- on a fixed-seed draw; it is a regression value for the step, not a trained model\'s score (see `trained`)')
    if w is CONFIGS[2] and os.path.exists(TRAINED):
        # what this stack reaches when it TRAINS (tools/train_pfn.py, one MI355X, 512 k datasets each): the notebook's own recipe
        # (5 features) and BASELINE.json's 18-feature variant of it, PFN bar NLL next to the exact GP posterior on the same draws
        tr = json.load(open(TRAINED))
        pick = lambda k: {kk: tr[k]['paired_eval_trained']['summary'][kk] for kk in ('pfn_bar_nll', 'exact_gp_nll', 'prior_nll')}
        out['trained'] = dict(source='profiles/' + os.path.basename(TRAINED),
                              notebook_recipe_5_features=dict(pick('notebook_recipe_5_features'), val_bar_nll_at_1755=tr['notebook_recipe_5_features']['val_bar_nll']['value'],
                                                              training_seconds=tr['notebook_recipe_5_features']['training_seconds']),
                              config2_18_features=dict(pick('config2_18_features_lr3e-4_batch64'), note='still at the prior after 512 k datasets under two recipes and after 2.05 M under a third'))
        if 'notebook_recipe_5_features_1M_datasets' in tr:
            k = 'notebook_recipe_5_features_1M_datasets'
            out['trained'][k] = dict(pick(k), val_bar_nll_at_1755=tr[k]['val_bar_nll']['value'], training_seconds=tr[k]['training_seconds'])
    return out


def self_launch(args):
    """`python bench.py --gpus N` without a torchrun environment: spawn the N ranks (one per GPU, RCCL) and relay rank 0's line."""
    visible = torch.cuda.device_count()
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    if visible < args.gpus and env.get('PFN_DP_SINGLE_DEVICE') != '1':
        raise SystemExit(f'bench.py --gpus {args.gpus}: only {visible} GPU(s) visible.  (Test hook for a one-GPU box: PFN_DP_SINGLE_DEVICE=1 '
                         f'PFN_DP_BACKEND=gloo runs every rank on device 0; the line then says so.)')
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    res = subprocess.run(cmd, env=env)
    raise SystemExit(res.returncode)


# kernel classes the library can time INSIDE the step (include/pfn_hip.h PFN_PROF_*; slot + 1 = the top layer's launch on the test rows)
PROF_SLOTS = {'attn_fwd': 0, 'attn_bwd_delta': 2, 'attn_bwd_kv': 4, 'attn_bwd_dq': 6, 'gemm_qkv': 8, 'gemm_out_proj_ln': 10, 'gemm_linear1_gelu': 12,
              'gemm_linear2_ln': 14, 'gemm_dhpre': 16, 'gemm_dy1_lnbwd': 18, 'gemm_dctx': 20, 'gemm_dx_lnbwd': 22, 'gemm_tn_group': 24}


def read_profile():
    """{class: {avg_us, launches}} of the event pairs the library recorded since the last read (pfn_profile_read)."""
    import ctypes
    from transformerscandobayesianinference_amd import _hip
    out = {}
    for name, slot in PROF_SLOTS.items():
        for top in (0, 1):
            ms, n = ctypes.c_double(0), ctypes.c_int64(0)
            _hip.check(_hip.lib().pfn_profile_read(slot + top, ctypes.byref(ms), ctypes.byref(n)), 'pfn_profile_read')
            if n.value:
                out[name + (' [top layer: test rows]' if top else '')] = dict(avg_us=ms.value * 1e3 / n.value, launches=n.value)
    return out


def run_config(config, device, rank, world, precision, batch=None, streams=None, steps=20, warmup=5, aggregate_k=1, fixed_sep=None, prefetch_group=None,
               profile_steps=0, aggregate_streams=0, aggregate_stacked=False, capture_outputs=False, time_allreduce=False):
    """One benchmark run of a BASELINE.json configuration: builds criterion, model, optimizer and the prior's loader, runs `warmup` untimed and
    `steps` timed OPTIMIZER steps (each = `aggregate_k` batches of `batch` datasets per rank: forward + loss + backward per batch, gradients
    summed, then [all-reduce +] clip + Adam -- reference train.py:66-97) between barrier + synchronize on both sides, max over ranks.
    profile_steps > 0: that many further steps with the library's in-step kernel timing on (not part of the timed window).
    capture_outputs: `outputs` = timed_outputs() of the last timed step, taken right after the timed window.
    time_allreduce (N > 1): `allreduce_ms` = the two collectives timed alone after the timed window."""
    from transformerscandobayesianinference_amd import _hip, dp
    from transformerscandobayesianinference_amd.optim import FusedClipAdam
    from transformerscandobayesianinference_amd.streams import MicroBatchStreams
    from transformerscandobayesianinference_amd.utils import get_uniform_single_eval_pos_sampler, get_weighted_single_eval_pos_sampler
    import numpy as np
    w = CONFIGS[config]
    batch = batch or w['batch']
    streams = streams or w['streams']
    S = w['bptt']
    torch.manual_seed(0); np.random.seed(0)
    criterion = make_criterion(w, device)
    model = build_model(device, precision, w, criterion)
    if world > 1:
        torch.distributed.broadcast(model.flat_parameters()[0], 0)
        if criterion is not None and hasattr(criterion, 'borders'):
            criterion.to(device)
            torch.distributed.broadcast(criterion.borders, 0)
    model.train()
    opt = FusedClipAdam(model, lr=1e-4, max_grad_norm=1.0)
    opt.grad_multiplier = 1.0 / world
    random.seed(1234)                      # rank-shared eval-position stream
    torch.manual_seed(1234 + rank)         # rank-distinct prior draws
    np.random.seed(1234 + rank)
    sampler = (get_weighted_single_eval_pos_sampler if w['eval_pos'] == 'weighted' else get_uniform_single_eval_pos_sampler)(S)
    seps = []
    loss_fn = loss_of(w, criterion)
    micro = MicroBatchStreams(streams)
    # aggregate_streams > 1: the batches of one optimizer step run whole, round-robin on that many streams (streams.py forward_backward_on; train()'s
    # automatic choice for small batches) instead of each being split into column groups
    alt = MicroBatchStreams(aggregate_streams) if (aggregate_streams > 1 and aggregate_k > 1) else None
    if alt is not None and not alt.can_alternate(model):
        alt = None
    reducer = None
    if world > 1:
        backend = torch.distributed.get_backend()
        if backend != 'nccl' and os.environ.get('PFN_DP_SINGLE_DEVICE') != '1':
            raise SystemExit(f'bench.py --gpus {world}: the collective backend is {backend!r}, not nccl (= RCCL on ROCm) although {torch.cuda.device_count()} '
                             f'GPU(s) are visible -- a multi-GPU number over a host-side backend would not be a measurement of this design')
        reducer = dp.OverlappedGradientReducer(model)

    stacked = aggregate_stacked and aggregate_k > 1 and micro.can_stack(model)
    last = {}      # the per-(position, dataset) losses of the latest batch (a reference to the step's own tensor: no work added)

    def step(batches):
        if stacked:      # the batches of the optimizer step as one launch set per micro-batch stream, every dataset with its own eval position (streams.py)
            stack = []
            for k in range(aggregate_k):
                sep = fixed_sep if fixed_sep is not None else sampler()
                seps.append(sep)
                (x, y), target = next(batches)
                stack.append(((x, y), target, sep))
            outs = micro.forward_backward_batches(model, stack, lambda out, tg, sep: loss_fn(out, tg[sep:]),
                                                  before=(lambda n: reducer.arm(n)) if reducer is not None else None)
            if reducer is not None:
                reducer.finish()
            opt.step(zero_grad=True)
            last['losses'] = outs[-1]
            return outs[-1].mean()
        for k in range(aggregate_k):       # reference train.py:92-97: micro-batch gradients are summed, one optimizer step per aggregate_k batches
            sep = fixed_sep if fixed_sep is not None else sampler()
            seps.append(sep)
            (x, y), target = next(batches)
            if alt is not None:
                if reducer is not None and k == aggregate_k - 1:
                    reducer.arm(1, wait_for=alt.fence_others(k))      # as train(): the last batch of the step is armed, the collective waits for the others
                losses = alt.forward_backward_on(k, model, (x, y), target, sep, lambda out, tg, sep=sep: loss_fn(out, tg[sep:]))
                continue
            if reducer is not None and k == aggregate_k - 1:
                reducer.arm(micro.groups(model, x.shape[1]))
            # forward + loss + backward of the batch, as `streams` concurrent column groups (streams.py)
            losses = micro.forward_backward(model, (x, y), target, sep, lambda out, tg: loss_fn(out, tg[sep:]))
        if alt is not None:
            alt.join()
        if reducer is not None:
            reducer.finish()       # two collectives: the upper layers' half was enqueued behind their weight gradients, under the backward
        opt.step(zero_grad=True)
        last['losses'] = losses
        return losses.mean()

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    # ONE loader across warm-up and timed steps: a continuous training run.  The sampler works one look-ahead group of G batches
    # ahead on a side stream (priors/utils.py): the draw for group g + 1 is enqueued when the first batch of group g is handed
    # out.  With G dividing the timed batches the groups enqueued inside the timed window are exactly that many / G full groups wherever the
    # window starts -- as much sampler work as the window's steps consume -- and the synchronisations on both sides of the window make the
    # executed work equal the enqueued work.  The loader is a whole number of groups long and extends one group past the window.
    loader_cls = prior_module(w).DataLoader
    nb = steps * aggregate_k
    # (group: the loader's own rule -- its step count, or for small batches its dataset count, priors/utils.py -- rounded down to a divisor of the timed batches)
    target = int(prefetch_group or max(getattr(loader_cls, 'prefetch_group', 1), -(-int(getattr(loader_cls, 'prefetch_group_datasets', 0) or 0) // batch)))
    group = max(d for d in range(1, nb + 1) if nb % d == 0 and d <= max(1, target)) if getattr(loader_cls, 'prefetch', False) else 1
    solo_steps = 3 if profile_steps > 0 else 0      # further steps that time ONE kernel class only (the usually dominant one: less perturbation)
    num_batches = ((warmup + steps + profile_steps + solo_steps) * aggregate_k + group + group - 1) // group * group
    with quiet():   # DataLoader.__init__ prints its kwargs (reference behaviour)
        dl = loader_cls(num_steps=num_batches, batch_size=batch, seq_len=S, device=device, **prior_kwargs(w))
    dl.prefetch_group = group
    dl._prefetch_group_fixed = True      # (the group is exactly what the accounting above assumes)
    batches = iter(dl)
    for _ in range(warmup):
        step(batches)
    barrier()
    seps.clear()
    t0 = time.time()
    for _ in range(steps):
        loss = step(batches)
    barrier()
    local_elapsed = elapsed = time.time() - t0
    timed_seps = list(seps)
    out = dict(config=config, w=w, model=model, batch=batch, streams=streams, steps=steps, warmup=warmup, aggregate_k=aggregate_k, group=group, seps=timed_seps,
               micro_groups=micro.groups(model, batch))
    if capture_outputs:
        out['outputs'] = timed_outputs(model, opt, last['losses'])
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        every = [torch.zeros_like(t) for _ in range(world)]
        torch.distributed.all_gather(every, t)
        out['per_rank_elapsed'] = [e.item() for e in every]
        elapsed = max(out['per_rank_elapsed'])
        ranks_seen = torch.ones(1, device=device, dtype=torch.float64)
        torch.distributed.all_reduce(ranks_seen)
        out['ranks_seen'] = int(ranks_seen.item())
        grad = model.flat_parameters()[1]
        out['overlapped_in_steps'] = bool(reducer.overlapped_last_step)
        out['fallback_steps'] = reducer.fallbacks
        if time_allreduce:
            barrier()
            t1 = time.time()
            for _ in range(5):
                reducer.finish()           # not armed: both collectives back to back, nothing to hide behind = the exposed cost
            torch.cuda.synchronize()
            out['allreduce_ms'] = (time.time() - t1) / 5 * 1e3
            grad.zero_()
        out['reducer_layout'] = reducer.layout()
    out['elapsed'], out['local_elapsed'], out['final_loss'] = elapsed, local_elapsed, loss.item()
    if profile_steps > 0 and world == 1:
        # the same steps once more with an event pair around every launch of the step's kernel classes, ON their launch streams: how long each
        # kernel runs INSIDE the step, where two micro-batch streams and the prior sampler share the chip
        lib = _hip.lib()
        # ... first for the key-block pass of the attention backward ALONE (the dominant kernel at every shape seen): an event pair is a marker in the
        # hardware queue, and with every class bracketed the step itself stretches (round 4: the all-class figure was 11 % above rocprofv3's)
        _hip.check(lib.pfn_profile_enable(2 + PROF_SLOTS['attn_bwd_kv']), 'pfn_profile_enable')
        read_profile()
        for _ in range(solo_steps):
            step(batches)
        torch.cuda.synchronize()
        out['in_step_solo'] = read_profile()
        _hip.check(lib.pfn_profile_enable(1), 'pfn_profile_enable')
        for _ in range(profile_steps):
            step(batches)
        torch.cuda.synchronize()
        _hip.check(lib.pfn_profile_enable(0), 'pfn_profile_enable')
        out['in_step'] = read_profile()
        out['profile_seps'] = seps[len(timed_seps):]
    if reducer is not None:
        reducer.detach()
    return out


def throughput_fields(r, world):
    """datasets/s, ms per optimizer step and the whole-step roofline fraction of a run_config() result."""
    import ctypes
    from transformerscandobayesianinference_amd import _hip
    w = r['w']
    S, nf, E, F, L, O = w['bptt'], w['num_features'], w['emsize'], w['nhid'], w['nlayers'], w['num_bars']
    lib, desc = _hip.lib(), r['model']._make_desc()
    top_rows_of = lambda rows, s: int(lib.pfn_top_layer_rows(ctypes.byref(desc), rows, S, s, 0))     # rows the top layer runs on (all, or the test rows only)
    step_flops = sum(train_flops(S, s, nf, E, F, L, O) for s in r['seps']) * r['batch'] * world               # the reference's graph
    needed_flops = sum(train_flops(S, s, nf, E, F, L, O, top_rows_of(1, s) != S) for s in r['seps']) * r['batch'] * world
    total = r['batch'] * world * r['steps'] * r['aggregate_k']
    return dict(value=total / r['elapsed'], ms_per_step=r['elapsed'] / r['steps'] * 1e3, frac=needed_flops / r['elapsed'] / world / MFMA_BF16_PEAK,
                reference_graph_frac=step_flops / r['elapsed'] / world / MFMA_BF16_PEAK, needed_flops=needed_flops, top_rows_of=top_rows_of)


def inference_cost(model, w, device, sep):
    """Latency of one inference pass (eval mode, no_grad -> model.eval_precision kernels) and of the same forward in the training precision,
    at the parity batch, plus the extra device memory the separate inference precision holds (its operand copy of the weights)."""
    B, S, nf = w['parity_batch'], w['bptt'], w['num_features']
    x, y = torch.rand(S, B, nf, device=device), torch.randn(S, B, device=device)
    was = model.training
    out = {}
    with torch.no_grad():
        for name, mode in (('inference_ms', False), ('training_precision_forward_ms', True)):
            model.train(mode)
            out[name] = time_kernel(lambda: model((x, y), single_eval_pos=sep), iters=3, warm=1) * 1e3
    model.train(was)
    out['batch'] = B
    out['inference_extra_weight_bytes'] = int(model._eval_shadow.numel()) if getattr(model, '_eval_shadow', None) is not None else 0
    return out


DUMP_LIMIT_BYTES = 64 << 20
DUMP_CAP = {'loss': 1 << 22, 'parameters': 1 << 23}      # elements per array: 16 + 32 MiB of float32 at most


def dump_sample(t, cap, seed=0):
    """`t` whole when it has at most `cap` elements; otherwise a fixed seeded sample of `cap` of its elements (flat indices drawn with
    replacement by a CPU generator seeded with `seed`, sorted), the same positions on every run of the same shape."""
    if t.numel() <= cap:
        return t
    idx = torch.randint(0, t.numel(), (cap,), generator=torch.Generator().manual_seed(seed)).sort()[0]
    return t.reshape(-1)[idx.to(t.device)]


def timed_outputs(model, opt, losses):
    """What a caller of the timed step receives from its last step, as host arrays:
      loss       [T - sep, batch] float32: the per-(position, dataset) losses of the step's (last) batch on this rank;
      parameters float32: the flat parameter buffer after the step's clip + Adam update (a fixed seeded sample when larger than DUMP_CAP);
      grad_norm  [1] float64: the global gradient norm the update saw, before clipping."""
    import numpy as np
    flat = model.flat_parameters()[0]
    return {'loss': dump_sample(losses.detach().float(), DUMP_CAP['loss']).cpu().numpy(),
            'parameters': dump_sample(flat.detach().float(), DUMP_CAP['parameters']).cpu().numpy(),
            'grad_norm': np.array([opt.last_grad_norm()], dtype=np.float64)}


def write_outputs(directory, outputs):
    """outputs {name: float32 / float64 array} -> directory/<name>.npy"""
    import numpy as np
    total = sum(a.nbytes for a in outputs.values())
    assert total <= DUMP_LIMIT_BYTES, f'outputs of {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte dump limit'
    os.makedirs(directory, exist_ok=True)
    for name, a in outputs.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(directory, f'{name}.npy'), a)


def release(r):
    r.pop('model', None)
    import gc
    gc.collect()
    torch.cuda.empty_cache()


DETAIL_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'bench_detail.json')
LINE_LIMIT = 6000     # the driver keeps an 8 KB tail of stdout: the line it parses must fit in it whole (round 4's 26 KB line lost its head)


def _num(v, digits=6):
    if isinstance(v, bool) or v is None or isinstance(v, (int, str)):
        return v
    if isinstance(v, float):
        return float(f'{v:.{digits}g}')
    if isinstance(v, (list, tuple)):
        return [_num(x, digits) for x in v]
    if isinstance(v, dict):
        return {k: _num(x, digits) for k, x in v.items()}
    return v


def _pick(d, keys):
    return {k: d[k] for k in keys if d is not None and k in d}


def compact_line(result):
    """The ONE line the driver parses: the contract keys + one number per side measurement.  Everything else (kernel table, notes, legs of the
    CPU baseline, parity details) lives in `bench_detail.json` next to this script, whose path the line names."""
    line = _pick(result, ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data'))
    cfg = result['config']
    line['config'] = _pick(cfg, ('workload', 'baseline_config', 'per_gpu_batch', 'global_batch', 'aggregate_k_gradients', 'aggregate_streams', 'aggregate_stacked', 'seq_len', 'parallelism',
                                 'micro_batch_streams', 'eval_pos', 'mean_sep', 'final_loss', 'tuning', 'library_variant', 'deterministic_schedule'))
    line['step_roofline'] = _pick(result['step_roofline'], ('bound', 'achieved', 'peak', 'unit', 'frac', 'reference_graph_frac'))
    if 'roofline' in result:
        line['roofline'] = _pick(result['roofline'], ('bound', 'kernel', 'rocprof_kernel', 'achieved', 'peak', 'unit', 'frac', 'frac_is', 'avg_launch_us', 'isolated_frac',
                                                      'isolated_avg_launch_us', 'algorithmic_flops_per_launch', 'executed_frac', 'launches_per_step', 'traffic', 'traffic_source'))
        line['roofline']['frac_is'] = 'in-step' if str(line['roofline'].get('frac_is', '')).startswith('IN-STEP') else 'isolated'
    if 'cpu_baseline' in result:
        c = result['cpu_baseline']
        line['cpu_baseline'] = dict(_pick(c, ('value', 'unit', 'cores', 'kind', 'port')), sample=c.get('sample_short', c.get('sample', ''))[:200])
    if 'parity_inference' in result:
        line['parity_inference'] = _pick(result['parity_inference'], ('precision', 'nll_rel', 'mean_rel_l2', 'logits_rel_l2', 'passed'))
        line['parity_timed_path'] = _pick(result['parity_timed_path'], ('precision', 'nll_rel', 'mean_rel_l2', 'logits_rel_l2', 'mean_ref_rms', 'nll_within_1e3', 'mean_within_1e3_of_own_norm'))
    if 'val_bar_nll' in result:
        v = result['val_bar_nll']
        line['val_bar_nll'] = v if not isinstance(v, dict) else _pick(v, ('bar_nll', 'value', 'n', 'sep'))
    for name, e in result.get('other_configs', {}).items():
        line.setdefault('other_configs', {})[name] = dict(value=e['value'], ms_per_step=e['ms_per_step'], per_gpu_batch=e['per_gpu_batch'], frac=e['step_roofline']['frac'])
    if 'also_bf16' in result:
        e = result['also_bf16']
        line['also_bf16'] = dict(value=e['value'], ms_per_step=e['ms_per_step'], **{k: e['parity_timed_path'][k] for k in ('nll_rel', 'mean_rel_l2') if 'parity_timed_path' in e})
    if 'batch_sweep' in result:
        line['batch_sweep'] = [dict(b=e['per_gpu_batch'], k=e['aggregate_k_gradients'], schedule=e['schedule'].split(' (')[0], value=e['value']) for e in result['batch_sweep']]
    for k in ('ranks_seen', 'per_rank_ms_per_step', 'allreduce_ms', 'allreduce_bytes', 'collective_backend', 'devices_visible', 'ranks_share_device'):
        if k in result:
            line[k] = result[k]
    if 'allreduce_overlapped' in result:
        line['allreduce_overlapped'] = _pick(result['allreduce_overlapped'], ('overlapped_bytes', 'exposed_bytes', 'in_timed_steps', 'fallback_steps'))
    line['seconds_total'] = result['seconds_total']
    line['detail'] = os.path.basename(DETAIL_FILE)
    line = _num(line)
    text = json.dumps(line, separators=(',', ':'))
    for drop in ('batch_sweep', 'other_configs', 'val_bar_nll', 'allreduce_overlapped', 'per_rank_ms_per_step'):    # never reached at the sizes above; the limit is a hard one
        if len(text) <= LINE_LIMIT:
            break
        line.pop(drop, None)
        text = json.dumps(line, separators=(',', ':'))
    assert len(text) <= LINE_LIMIT, len(text)
    return text


def emit(result):
    """Full record -> bench_detail.json (and stderr when PFN_BENCH_VERBOSE=1); compact line -> the LAST line of stdout."""
    try:
        with open(DETAIL_FILE, 'w') as f:
            json.dump(result, f, indent=1)
    except OSError as e:
        print(f'bench.py: could not write {DETAIL_FILE}: {e}', file=sys.stderr)
    if os.environ.get('PFN_BENCH_VERBOSE') == '1':
        print(json.dumps(result), file=sys.stderr)
    sys.stdout.flush()
    print(compact_line(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--config', type=int, default=2, choices=sorted(CONFIGS), help='BASELINE.json configuration (2 = configs[1], the metric\'s; 4 = BNN prior; 5 = GP mixture, bptt 4000)')
    ap.add_argument('--batch', type=int, default=None, help='datasets per GPU per batch (default: per configuration)')
    ap.add_argument('--aggregate-k', type=int, default=1, help='batches per optimizer step (train()\'s aggregate_k_gradients)')
    ap.add_argument('--aggregate-streams', type=int, default=0, help='> 1: the aggregate_k batches of a step run whole, round-robin on that many streams (small batches)')
    ap.add_argument('--aggregate-stacked', action='store_true', help='the aggregate_k batches of a step stacked into one launch set per micro-batch stream, every dataset with its own eval position (what train() picks for small batches since round 5)')
    ap.add_argument('--streams', type=int, default=None, help='concurrent micro-batches per step (column groups of the batch on separate HIP streams)')
    ap.add_argument('--precision', default='fp16', choices=['bf16', 'fp16', 'f32'],
                    help='operand format of the TIMED (training) path, recorded as `dtype`.  fp16 (round 6): the 16-bit format whose training forward holds the north star\'s 1e-3 on NLL and '
                         'posterior means (same MFMA rate and bytes as bf16; gradients under a device-side loss scale); the bf16 figures ride along as `also_bf16`')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step computed to DIR/<name>.npy (float32 / float64, at most 64 MB in all): loss, parameters, grad_norm')
    ap.add_argument('--full', action='store_true',
                    help='also run every side measurement: in-step and isolated kernel timings (roofline, kernels), parity against the f64 oracle, '
                         'val_bar_nll, cpu_baseline, also_bf16, other_configs, batch_sweep, allreduce_ms (N > 1).  Off: the headline figure only')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip `cpu_baseline`')
    ap.add_argument('--no-parity', action='store_true', help='with --full: skip the parity blocks, `val_bar_nll` and `cpu_baseline`')
    ap.add_argument('--no-kernel-breakdown', action='store_true', help='with --full: skip the in-step profile steps and the kernel table (`roofline`, `kernels`)')
    ap.add_argument('--no-extras', action='store_true', help='with --full: skip `also_bf16`, `other_configs` (short runs of configs 4 and 5) and `batch_sweep` (configs[1] at per-GPU batch 4 x 25, 8, 16, 32)')
    ap.add_argument('--fixed-sep', type=int, default=None, help='use one eval position instead of the sampler')
    ap.add_argument('--prefetch-group', type=int, default=None, help='steps of datasets per sampler call (default: the loader class\'s; the bench uses its gcd with --steps)')
    ap.add_argument('--tune', default='', help='experiments: comma-separated key=value pairs for pfn_set_tuning (include/pfn_hip.h); recorded in config')
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be at least 1 and --warmup at least 0')
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        self_launch(args)

    from transformerscandobayesianinference_amd import dp
    rank, world, local = dp.init_from_env()
    assert world == args.gpus, f'--gpus {args.gpus} but WORLD_SIZE={world}'
    device = torch.device('cuda', local)
    torch.cuda.set_device(device)
    w = CONFIGS[args.config]
    tuning = {int(k): int(v) for k, v in (kv.split('=') for kv in args.tune.split(',') if kv)}
    from transformerscandobayesianinference_amd import _hip
    if os.environ.get('PFN_LIB'):      # experiment builds of the library (tools/build_variants.sh): same-box A/B of a kernel change inside the step; recorded in config
        _hip.LIB_PATH = os.path.abspath(os.environ['PFN_LIB'])
    for k, v in tuning.items():
        _hip.check(_hip.lib().pfn_set_tuning(k, v), 'pfn_set_tuning')
    t_start = time.time()
    r = run_config(args.config, device, rank, world, args.precision, batch=args.batch, streams=args.streams, steps=args.steps, warmup=args.warmup,
                   aggregate_k=args.aggregate_k, fixed_sep=args.fixed_sep, prefetch_group=args.prefetch_group, aggregate_streams=args.aggregate_streams, aggregate_stacked=args.aggregate_stacked,
                   profile_steps=5 if (args.full and world == 1 and not args.no_kernel_breakdown) else 0,
                   capture_outputs=args.dump_outputs is not None and rank == 0, time_allreduce=args.full)
    if rank != 0:
        return
    if args.dump_outputs is not None:
        write_outputs(args.dump_outputs, r.pop('outputs'))
    model, batch, streams, seps = r['model'], r['batch'], r['streams'], r['seps']
    S, nf, E, F, L, O = w['bptt'], w['num_features'], w['emsize'], w['nhid'], w['nlayers'], w['num_bars']
    tp = throughput_fields(r, world)
    top_rows_of = tp['top_rows_of']
    result = {
        'metric': w['metric'], 'value': tp['value'], 'unit': 'datasets/s',
        'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': tp['ms_per_step'],
        'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': {'bf16': 'bf16', 'fp16': 'fp16', 'f32': 'f32'}[args.precision], 'data': 'synthetic',
        'config': {'workload': w['workload'], 'baseline_config': args.config,
                   'per_gpu_batch': batch, 'global_batch': batch * world, 'aggregate_k_gradients': args.aggregate_k, 'aggregate_streams': args.aggregate_streams, 'aggregate_stacked': bool(args.aggregate_stacked), 'seq_len': S, 'parallelism': f'dp{world}',
                   'micro_batch_streams': streams,
                   'eval_pos': f"{w['eval_pos']} sampler({S})" if args.fixed_sep is None else args.fixed_sep, 'mean_sep': sum(seps) / len(seps),
                   'sampler_group_steps': r['group'], 'final_loss': r['final_loss']},
        'step_roofline': {'bound': 'mfma', 'achieved': tp['needed_flops'] / r['elapsed'] / 1e12 / world, 'peak': MFMA_BF16_PEAK / 1e12, 'unit': 'TFLOP/s',
                          'frac': tp['frac'], 'reference_graph_frac': tp['reference_graph_frac'],
                          'note': 'whole step per GPU, algorithmic mask-aware FLOPs 3*fwd(S,sep).  `frac` counts what the result needs: the top encoder layer\'s train '
                                  'rows feed nothing (the reference returns output[single_eval_pos:]) and are not computed (pfn_top_layer_rows); '
                                  '`reference_graph_frac` counts the reference\'s graph, which computes and discards them (the figure of rounds 1-2)'},
    }
    if tuning:
        result['config']['tuning'] = tuning
    if os.environ.get('PFN_LIB'):
        result['config']['library_variant'] = os.path.basename(os.environ['PFN_LIB'])
    if os.environ.get('PFN_BENCH_DETERMINISTIC') == '1':
        result['config']['deterministic_schedule'] = True
    if world > 1:
        result['ranks_seen'] = r['ranks_seen']
        result['per_rank_ms_per_step'] = [e / args.steps * 1e3 for e in r['per_rank_elapsed']]      # spread = load imbalance / stragglers at the all-reduce
        if 'allreduce_ms' in r:
            result['allreduce_ms'] = r['allreduce_ms']
        result['allreduce_bytes'] = model.flat_parameters()[1].numel() * 4
        result['allreduce_overlapped'] = dict(r['reducer_layout'], in_timed_steps=r['overlapped_in_steps'], fallback_steps=r['fallback_steps'],
                                              note='the gradient buffer is reduced as two collectives; `overlapped_bytes` (upper half of the layers + '
                                                   'decoder) start behind those layers\' weight gradients and run under the rest of the backward, '
                                                   '`exposed_bytes` after it; allreduce_ms (--full) = both collectives timed alone, back to back (an upper bound on what a step '
                                                   'can lose to communication); fallback_steps = armed steps whose early collective could not be overlapped')
        result['collective_backend'] = torch.distributed.get_backend()
        result['devices_visible'] = torch.cuda.device_count()
        if os.environ.get('PFN_DP_SINGLE_DEVICE') == '1':
            result['ranks_share_device'] = True    # one-GPU test hook: NOT a scaling measurement
    if args.full and world == 1 and not args.no_kernel_breakdown:
        # kernels are launched per micro-batch (column group of the batch, streams.py): time them at THAT shape
        groups = r['micro_groups']
        mean_sep = int(round(sum(seps) / len(seps)))
        mb = -(-batch // groups)      # (the larger group when the batch does not divide)
        ks = kernel_breakdown(mb, mean_sep, w, fused_ln_wide=bool(tuning.get(5)), top_rows=top_rows_of(mb, mean_sep), precision=args.precision)
        in_step = r.get('in_step', {})
        in_solo = r.get('in_step_solo', {})
        for k in ks:
            k['launches_per_step'] *= groups * args.aggregate_k
            k['step_seconds'] *= groups * args.aggregate_k
            cls = k.get('prof_class')
            if cls and cls in in_step:
                k['in_step_us'] = in_step[cls]['avg_us']
                k['in_step_launches_timed'] = in_step[cls]['launches']
            if cls and cls in in_solo:      # timed with no other class bracketed: the figure `roofline` quotes
                k['in_step_all_classes_us'] = k.get('in_step_us')
                k['in_step_us'] = in_solo[cls]['avg_us']
                k['in_step_launches_timed'] = in_solo[cls]['launches']
        dom = max(ks, key=lambda k: k['step_seconds'])   # the kernel the step spends most time in
        traffic, traffic_src = None, None
        pmc_file, trace_file = PMC_TRAFFIC.format(config=args.config), IN_STEP_TRACE.format(config=args.config)
        pmc = json.load(open(pmc_file)) if os.path.exists(pmc_file) else {}

        def same_command(rec):      # a committed pass counts only for the command it profiled: configuration, batch, streams, operand format, library ABI
            return bool(rec) and rec.get('config') == args.config and rec.get('batch') == batch and rec.get('streams', 1) == streams and \
                rec.get('precision', 'bf16') == args.precision and rec.get('abi', _hip.ABI_VERSION) == _hip.ABI_VERSION
        if same_command(pmc):
            hit = [v for name, v in pmc.get('kernels', {}).items() if dom['rocprof_name'] in name and 'top layer' not in name]   # (the attention's top-layer launches are listed apart)
            if hit:
                traffic = hit[0].get('read_bytes', 0) + hit[0].get('write_bytes', 0)
                traffic_src = f"profiles/{os.path.basename(pmc_file)} ({pmc.get('note', '')})"
        else:
            traffic_src = f"none: no committed PMC pass of this command (profiles/{os.path.basename(pmc_file)}: " + \
                          (f"config {pmc.get('config')} / batch {pmc.get('batch')} / streams {pmc.get('streams')} / {pmc.get('precision')} / ABI {pmc.get('abi')}" if pmc else 'absent') + ')'
        in_us = dom.get('in_step_us')
        iso_frac = dom['tflops'] * 1e12 / MFMA_BF16_PEAK
        # the COMMITTED kernel trace of this command, for the same kernel's full-layer launches: begin / end of the kernel itself, where the event pair of the live
        # figure also counts the wait of a launch for free CUs behind the other streams.  Not measured in this run: it goes to bench_detail.json under `committed_trace_*`
        # with its source, never into the line the driver parses (VERDICT r5 weak 8 / ADVICE r5).
        trace_us = None
        trace = json.load(open(trace_file)) if os.path.exists(trace_file) else {}
        if same_command(trace):
            trace_us = next((v.get('avg_us') for name, v in trace.get('kernels', {}).items() if dom['rocprof_name'] in name and 'top layer' not in name), None)
        in_frac = None if in_us is None else dom['flops'] / (in_us * 1e-6) / MFMA_BF16_PEAK
        # (the in-step launches run at the eval positions of the profiled steps; the isolated ones at the mean position -- FLOPs per launch taken at the mean)
        result['roofline'] = {'bound': 'mfma', 'kernel': dom['kernel'], 'rocprof_kernel': dom['rocprof_name'],
                              'achieved': dom['tflops'] if in_us is None else dom['flops'] / (in_us * 1e-6) / 1e12,
                              'peak': MFMA_BF16_PEAK / 1e12, 'unit': 'TFLOP/s', 'frac': iso_frac if in_frac is None else in_frac,
                              'frac_is': 'isolated (no in-step timing for this kernel class)' if in_frac is None else
                                         'IN-STEP: average launch duration inside the running step (HIP event pairs on the launch stream, pfn_profile_*; two micro-batch '
                                         'streams + the sampler share the chip)',
                              'in_step_avg_launch_us': in_us, 'in_step_launches_timed': dom.get('in_step_launches_timed'),
                              'committed_trace_avg_launch_us': trace_us, 'committed_trace_frac': None if not trace_us else dom['flops'] / (trace_us * 1e-6) / MFMA_BF16_PEAK,
                              'committed_trace_source': f'profiles/{os.path.basename(trace_file)} (a rocprofv3 kernel trace of this command, committed; NOT measured in this run)' if trace_us else None,
                              'isolated_frac': iso_frac, 'isolated_avg_launch_us': dom['seconds'] * 1e6, 'isolated_achieved': dom['tflops'],
                              'traffic': traffic, 'traffic_source': traffic_src, 'algorithmic_flops_per_launch': dom['flops'],
                              'executed_flops_per_launch': dom['executed_flops'], 'executed_frac': dom['executed_tflops'] * 1e12 / MFMA_BF16_PEAK,
                              'avg_launch_us': dom['seconds'] * 1e6 if in_us is None else in_us, 'launches_per_step': dom['launches_per_step'],
                              'in_step_ms': dom['step_seconds'] * 1e3,
                              'note': 'dominant kernel by launches x isolated duration.  isolated_* = every launch timed with HIP events on its stream without co-runners '
                                      '(GEMMs and the attention forward repeated on their own, the attention backward\'s three launches inside their sequence); `frac` / '
                                      '`achieved` / `avg_launch_us` = the same kernel class timed inside the step'}
        result['kernels'] = [{k: (round(v, 6) if isinstance(v, float) else v) for k, v in kk.items()} for kk in ks]
        result['in_step_kernel_us'] = {k: dict(avg_us=round(v['avg_us'], 2), launches=v['launches']) for k, v in in_step.items()}
    if args.full and world == 1 and not args.no_parity:
        parity, inputs = parity_check(model, w, device, args.precision)
        timed = parity.pop('training_forward')
        timed['mean_ref_rms'] = parity['mean_ref_rms']      # the scale `mean_rel_l2` divides by (targets: y_test_rms)
        cost = inference_cost(model, w, device, w['parity_sep'])
        # two blocks, each saying which path it covers: the north star's 1e-3 is a statement about OUTPUTS (inference passes: eval mode ->
        # model.eval_precision kernels); the throughput above is the bf16 training path, whose forward is measured beside it on the same inputs
        result['parity_inference'] = dict(parity, covers='inference outputs: model.eval() under no_grad (validate / run_test / criterion.mean); NOT the timed path',
                                          gate='north_star 1e-3 on nll_rel and mean_rel_l2', passed=bool(parity['nll_rel'] < 1e-3 and parity['mean_rel_l2'] < 1e-3), cost=cost)
        result['parity_timed_path'] = dict(timed, covers=f'forward of the TIMED path (train mode, {args.precision} operands) on the same inputs and weights',
                                           gate='reported; nll_rel < 1e-3 holds on these (untrained) weights, trained weights: DESIGN.md section 4',
                                           nll_within_1e3=bool(timed['nll_rel'] < 1e-3), mean_within_1e3_of_own_norm=bool(timed['mean_rel_l2'] < 1e-3))
        result['parity'] = dict(parity, training_forward=timed)      # (the layout of rounds 2-3, kept for tools/)
        result['val_bar_nll'] = validation_loss(model, w, device)
        if not args.no_cpu_baseline:
            result['cpu_baseline'] = cpu_baseline(w, inputs)
    result['seconds_main_line'] = time.time() - t_start
    if args.full and world == 1 and not args.no_extras and args.config == 2 and args.batch is None and args.aggregate_k == 1:
        release(r)
        del model
        result['other_configs'] = {}
        # the same configuration with bf16 operands (rounds 1-5's timed path; BASELINE configs[1] says "bf16"): throughput and timed-path parity beside the fp16 line
        if args.precision != 'bf16':
            t0 = time.time()
            rb16 = run_config(2, device, 0, 1, 'bf16', steps=args.steps, warmup=args.warmup)      # (straight after the main line, same step counts: the chip in the same state)
            tb16 = throughput_fields(rb16, 1)
            entry = dict(dtype='bf16', value=tb16['value'], unit='datasets/s', ms_per_step=tb16['ms_per_step'], steps=args.steps, warmup=args.warmup, per_gpu_batch=rb16['batch'],
                         step_roofline_frac=tb16['frac'])
            if not args.no_parity:
                par16, _ = parity_check(rb16['model'], CONFIGS[2], device, 'bf16')
                tf16 = par16['training_forward']
                entry['parity_timed_path'] = dict(precision='bf16', nll_rel=tf16['nll_rel'], mean_rel_l2=tf16['mean_rel_l2'], logits_rel_l2=tf16['logits_rel_l2'])
            entry['seconds'] = time.time() - t0
            result['also_bf16'] = entry
            release(rb16)
            del rb16
        for cfg in (4, 5):
            t0 = time.time()
            rc = run_config(cfg, device, 0, 1, args.precision, steps=10, warmup=3)
            tc = throughput_fields(rc, 1)
            entry = dict(workload=CONFIGS[cfg]['workload'], value=tc['value'], unit='datasets/s', ms_per_step=tc['ms_per_step'], steps=10, warmup=3,
                         per_gpu_batch=rc['batch'], micro_batch_streams=rc['streams'], mean_sep=sum(rc['seps']) / len(rc['seps']),
                         step_roofline=dict(frac=tc['frac'], reference_graph_frac=tc['reference_graph_frac']))
            if not args.no_parity:
                par, _ = parity_check(rc['model'], CONFIGS[cfg], device, args.precision)
                tf = par['training_forward']
                entry['parity'] = dict(precision=par['precision'], nll_rel=par['nll_rel'], mean_rel_l2=par['mean_rel_l2'], mean_max_over_y_range=par['mean_max_over_y_range'],
                                       logits_rel_l2=par['logits_rel_l2'], oracle_forward_s=par['oracle_forward_s'],
                                       timed_path=dict(precision=tf['precision'], nll_rel=tf['nll_rel'], mean_rel_l2=tf['mean_rel_l2'], logits_rel_l2=tf['logits_rel_l2']))
            entry['seconds'] = time.time() - t0
            result['other_configs'][f'configs[{cfg - 1}]'] = entry
            release(rc)
            del rc
        # the small-batch regime of the reference's notebooks (SetupForGPFittingExperiments.ipynb:143-149 trains configs[1] at batch_size 4 with
        # aggregate_k_gradients 25): per-GPU batch 4 x 25 batches per optimizer step, then 8 / 16 / 32 with one batch per step
        result['batch_sweep'] = []
        # (schedule: `alternating` = the batches of one optimizer step whole, round-robin on that many streams -- what train() picks for small batches;
        # `column groups` = every batch split over the two micro-batch streams, what the large batches use)
        for b, k, st, alt_streams in ((4, 25, 3, -1), (4, 25, 3, 8), (4, 25, 3, 0), (8, 1, 10, 0), (16, 1, 10, 0), (32, 1, 10, 0)):      # (-1: the stacked schedule)
            t0 = time.time()
            rb = run_config(2, device, 0, 1, args.precision, batch=b, aggregate_k=k, steps=st, warmup=2, aggregate_streams=max(alt_streams, 0), aggregate_stacked=alt_streams < 0)
            tb = throughput_fields(rb, 1)
            result['batch_sweep'].append(dict(per_gpu_batch=b, aggregate_k_gradients=k, datasets_per_optimizer_step=b * k,
                                              schedule='stacked (one launch set per stream, per-dataset eval positions)' if alt_streams < 0 else f'alternating x {alt_streams}' if alt_streams else f"column groups x {rb['micro_groups']}",
                                              value=tb['value'], unit='datasets/s', ms_per_optimizer_step=tb['ms_per_step'], steps=st,
                                              step_roofline_frac=tb['frac'], seconds=time.time() - t0))
            release(rb)
            del rb
    result['seconds_total'] = time.time() - t_start
    emit(result)


if __name__ == '__main__':
    main()
