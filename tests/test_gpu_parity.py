"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and against the golden
vectors recorded from the reference itself (tests/golden, oracle/make_golden.py).

Tolerances (north_star: NLL and posterior-predictive means within 1e-3 relative):
  * exact-f32 MFMA mode ('f32'): 1e-4 relative on logits / losses / means / gradients -- any layout
    or algorithmic mistake fails here;
  * bf16 mode (the benchmarked product mode): 1e-3 relative on the bar NLL (mean over the batch) and 1e-3 on the
    posterior-predictive means relative to the scale of the quantity they predict (the targets' range / rms; an
    untrained PFN predicts the prior mean ~ 0 everywhere, so an error relative to the means' own norm only restates
    the logit error).  Measured at the benchmarked shape (tools/parity_probe.py, profiles/r02_parity_probe.txt):
    logits 4.3e-3 (the bf16 operand rounding of every GEMM stage, ~1.6e-3 each), NLL 1.5e-5, means 1e-5 of the target
    range.  Per-element logits are asserted at 1e-2, the global gradient at 1.2e-2: twice the values measured on the MI355X and recorded
    in profiles/r03_parity_measured.json (`within`, tests/bounds.py); the gradient at the BENCHMARKED shapes against the f64 oracle is
    in profiles/r03_grad_parity.json (tools/grad_parity.py: 6.1e-3 at configs[1], 5.0e-3 at the configs[4] slice).
"""
import ctypes
import math
import os
import random
import re

import pytest
import torch

from oracle import pfn_oracle
from bounds import within
from transformerscandobayesianinference_amd import _hip, bar_distribution, encoders, positional_encodings
from transformerscandobayesianinference_amd.optim import FusedClipAdam
from transformerscandobayesianinference_amd.transformer import TransformerModel

pytestmark = pytest.mark.gpu


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return str(sk.getsockname()[1])
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda:0'


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def tol3(precision, f32, bf16, fp16=None):
    """Bound by operand format of the training path.  fp16 (11 significand bits against bf16's 8: a factor 8 expected) defaults to a QUARTER of the bf16
    bound, never below the exact-f32 bound; where a measured value is on record (profiles/r06_parity_measured.json) the explicit bound is 2 x that."""
    if precision == 'f32':
        return f32
    if precision == 'bf16':
        return bf16
    return fp16 if fp16 is not None else max(f32, bf16 / 4)


def mean_err(got, want, y):
    """max |posterior mean error| relative to the range of the targets (north_star's 1e-3 bound is asserted on this)."""
    return ((got.detach().double().cpu() - want.detach().double().cpu()).abs().max() / (y.max() - y.min()).double().cpu()).item()


def build_model(cfg, sd, precision):
    crit = bar_distribution.FullSupportBarDistribution(sd['criterion.borders'].clone())
    m = TransformerModel(encoders.Linear(cfg['F'], cfg['E']), cfg['nbars'], cfg['E'], cfg['H'], cfg['nhid'], cfg['L'], 0.0,
                         y_encoder=encoders.Linear(1, cfg['E']),
                         pos_encoder=positional_encodings.NoPositionalEncoding(cfg['E'], cfg['T'] * 2), precision=precision, eval_precision=precision)
    m.criterion = crit
    missing = m.load_state_dict(sd, strict=True)
    return m.to(DEV)


@pytest.mark.parametrize('case', ['model_small_h32', 'model_small_h64'])
@pytest.mark.parametrize('precision', ['f32', 'bf16', 'fp16'])
def test_forward_loss_grads_vs_reference_golden(case, precision):
    rec = torch.load(os.path.join(GOLD, case + '.pt'))
    cfg = rec['config']
    model = build_model(cfg, rec['state_dict'], precision)
    model.train()
    x, y = rec['x'].to(DEV), rec['y'].to(DEV)
    tight = precision == 'f32'
    for sep, want in rec['per_sep'].items():
        model.zero_grad()
        logits = model((x, y), single_eval_pos=sep)
        assert logits.shape == want['logits'].shape
        within(f'{precision} logits rel l2', relerr(logits, want['logits']), tol3(precision, 1e-4, 1e-2, 1.2e-3))
        losses = model.criterion(logits.reshape(-1, cfg['nbars']), y[sep:].flatten()).view(*logits.shape[:2])
        loss = losses.mean()
        within(f'{precision} loss rel', abs(loss.item() - want['loss'].item()) / abs(want['loss'].item()), tol3(precision, 1e-4, 1e-3, 1.0e-4))
        means = model.criterion.mean(logits)
        within(f'{precision} means max / target range', mean_err(means, want['mean'], y), tol3(precision, 1e-5, 1e-3, 2.0e-5))
        within(f'{precision} means rel l2 (own norm)', relerr(means, want['mean']), tol3(precision, 1e-4, 4e-3, 7.1e-4))      # relative to the means' own norm: the logit error
        if 'grads' in want:
            loss.backward()
            got = {k: p.grad for k, p in model.named_parameters()}
            tot_err = math.sqrt(sum(((got[k].double().cpu() - g.double()) ** 2).sum().item() for k, g in want['grads'].items()))
            tot = math.sqrt(sum((g.double() ** 2).sum().item() for g in want['grads'].values()))
            within(f'{precision} global gradient rel l2', tot_err / tot, tol3(precision, 2e-4, 1.2e-2, 1.2e-3))
            if tight:
                for k, g in want['grads'].items():
                    if g.norm() > 1e-6:
                        assert relerr(got[k], g) < 2e-3, (sep, k, relerr(got[k], g))


@pytest.mark.parametrize('precision', ['f32', 'bf16', 'fp16'])
def test_two_training_steps_vs_reference_golden(precision):
    """clip-to-1 + Adam on the flat buffer reproduces the reference's two torch steps (train.py:92-97)."""
    rec = torch.load(os.path.join(GOLD, 'model_small_h32.pt'))
    cfg, tr = rec['config'], rec['train']
    model = build_model(cfg, rec['state_dict'], precision)
    model.train()
    opt = FusedClipAdam(model, lr=1e-3, max_grad_norm=1.0)
    x, y = rec['x'].to(DEV), rec['y'].to(DEV)
    sep = tr['sep']
    for step in range(2):
        logits = model((x, y), single_eval_pos=sep)
        loss = model.criterion(logits.reshape(-1, cfg['nbars']), y[sep:].flatten()).mean()
        loss.backward()
        opt.step(zero_grad=True)
        want = tr['steps'][step]
        tol = tol3(precision, 2e-4, 2e-3)
        assert abs(loss.item() - want['loss'].item()) < tol * abs(want['loss'].item()), (step, loss.item(), want['loss'].item())
        within(f'{precision} grad norm rel', abs(opt.last_grad_norm() - want['grad_norm'].item()) / want['grad_norm'].item(), tol3(precision, 1e-3, 2e-3))
    # Adam normalises each element by its own gradient history, so elements whose gradient is at the
    # rounding-noise level legitimately differ by O(lr); compare the update as a whole instead.
    final = model.state_dict()
    num = den = 0.0
    for k, v in tr['final_state_dict'].items():
        if k.startswith('criterion.'):
            continue
        d_ref = v.double() - rec['state_dict'][k].double()
        d_got = final[k].cpu().double() - rec['state_dict'][k].double()
        num += ((d_got - d_ref) ** 2).sum().item()
        den += (d_ref ** 2).sum().item()
    within(f'{precision} two-step Adam update rel l2', math.sqrt(num / den), tol3(precision, 2e-2, 0.12, 7e-2))      # (fp16 measured 3.3e-2: Adam turns rounding-level gradients into O(lr) steps in every format)


def random_model(cfg, precision, seed=0):
    torch.manual_seed(seed)
    borders = torch.sort(torch.randn(cfg['nbars'] + 1) * 1.5)[0]
    crit = bar_distribution.FullSupportBarDistribution(borders)
    m = TransformerModel(encoders.Linear(cfg['F'], cfg['E']), cfg['nbars'], cfg['E'], cfg['H'], cfg['nhid'], cfg['L'], 0.0,
                         y_encoder=encoders.Linear(1, cfg['E']), pos_encoder=None, precision=precision, eval_precision=precision)
    m.criterion = crit
    with torch.no_grad():
        for layer in m.transformer_encoder.layers:  # un-zero the residual branches
            for t in (layer.linear2.weight, layer.self_attn.out_proj.weight):
                t.normal_(0, 0.03)
    return m


@pytest.mark.parametrize('precision', ['f32', 'bf16', 'fp16'])
def test_config1_vs_oracle(precision):
    """BASELINE config 1 shape (bptt=100, nf=5, emsize=128, nlayers=2, batch=8) against the f64 oracle."""
    cfg = dict(T=100, B=8, F=5, E=128, H=4, nhid=256, L=2, nbars=100)
    model = random_model(cfg, precision, seed=3)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    gen = torch.Generator().manual_seed(5)
    x, y, _ = pfn_oracle.get_batch_fast_gp(cfg['B'], cfg['T'], cfg['F'], {'noise': 1e-4, 'outputscale': 1., 'lengthscale': .6}, gen)
    for sep in (81, 99, 1):
        loss_o, logits_o, grads_o = pfn_oracle.loss_and_grads(sd, x, y, y, sep, cfg['H'], sd['criterion.borders'])
        model.zero_grad()
        logits = model((x.to(DEV), y.to(DEV)), single_eval_pos=sep)
        loss = model.criterion(logits.reshape(-1, cfg['nbars']), y[sep:].to(DEV).flatten()).mean()
        loss.backward()
        tight = precision == 'f32'
        within(f'{precision} loss rel', abs(loss.item() - loss_o.item()) / abs(loss_o.item()), tol3(precision, 1e-4, 1e-3, 1.0e-4))
        within(f'{precision} logits rel l2', relerr(logits, logits_o), tol3(precision, 1e-4, 1e-2, 1.3e-3))
        m_o = pfn_oracle.bar_mean(logits_o, sd['criterion.borders'])
        m_h = model.criterion.mean(logits)
        within(f'{precision} means max / target range', mean_err(m_h, m_o, y), tol3(precision, 1e-5, 1e-3, 1.9e-5))
        within(f'{precision} means rel l2 (own norm)', relerr(m_h, m_o), tol3(precision, 1e-4, 4e-3, 2.1e-4))
        tot_err = math.sqrt(sum(((p.grad.double().cpu() - grads_o[k]) ** 2).sum().item() for k, p in model.named_parameters()))
        tot = math.sqrt(sum((g ** 2).sum().item() for g in grads_o.values()))
        within(f'{precision} global gradient rel l2', tot_err / tot, tol3(precision, 2e-4, 1.2e-2, 1.3e-3))
        if tight:
            # every tensor by itself, at the bound rule of tests/test_gpu_stack_grads.py for the exact-f32 mode: 4 x max(e, 2^-23), e = the oracle in f32 against f64
            _, _, grads_32 = pfn_oracle.loss_and_grads(sd, x, y, y, sep, cfg['H'], sd['criterion.borders'], dtype=torch.float32)
            for k, p in model.named_parameters():
                within('f32 ' + re.sub(r'layers\.\d+\.', 'layers.*.', k) + ' grad rel l2 / bound', relerr(p.grad, grads_o[k]) / (4 * max(relerr(grads_32[k], grads_o[k]), 2.0 ** -23)), 1.0)


@pytest.mark.parametrize('E,H', [(128, 4), (512, 4), (1024, 4)])      # LayerNorm-fused GEMMs (128, 512) / the LayerNorm as its own kernel (1024 = configs[4])
def test_fp16_pre_layernorm_sums_in_operand_precision_vs_f32(E, H):
    """fp16 operands store the pre-LayerNorm sums -- the residual the next block adds, the LayerNorm backward's input -- in fp16 by default (GemmLN::y16: half the
    bytes of the LayerNorm-fused GEMMs' two f32 streams); PFN_SCHED_F32_RESIDUAL keeps them in f32 as in bf16.  Both against the f64 oracle, and against each other:
    the 16-bit sums add less than the operand rounding that is there anyway.  At emsize 1024, where the LayerNorm is its own kernel, the GEMM ahead of it adds the
    residual from the operand-precision copy of the layer input and stores an fp16 sum (launch_layernorm_fwd x_is_t)."""
    cfg = dict(T=160, B=4, F=5, E=E, H=H, nhid=2 * E, L=3, nbars=100)
    ref = random_model(cfg, 'fp16', seed=11)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    gen = torch.Generator().manual_seed(6)
    x, y, _ = pfn_oracle.get_batch_fast_gp(cfg['B'], cfg['T'], cfg['F'], {'noise': 1e-4, 'outputscale': 1., 'lengthscale': .6}, gen)
    for sep in (120, 30):       # (the top layer on the test rows only / on every row)
        loss_o, logits_o, grads_o = pfn_oracle.loss_and_grads(sd, x, y, y, sep, cfg['H'], sd['criterion.borders'])
        tot = math.sqrt(sum((g ** 2).sum().item() for g in grads_o.values()))
        out = {}
        for name, bits in (('fp16 sums', 0), ('f32 sums', _hip.SCHED_F32_RESIDUAL)):
            model = random_model(cfg, 'fp16', seed=11)
            model.schedule = bits
            model = model.to(DEV).train()
            logits = model((x.to(DEV), y.to(DEV)), single_eval_pos=sep)
            loss = model.criterion(logits.reshape(-1, cfg['nbars']), y[sep:].to(DEV).flatten()).mean()
            loss.backward()
            g = {k: p.grad.double().cpu() for k, p in model.named_parameters()}
            err = math.sqrt(sum(((g[k] - grads_o[k]) ** 2).sum().item() for k in g)) / tot
            within(f'{name}, sep {sep}: logits rel l2 vs oracle', relerr(logits, logits_o), 1.7e-3)       # (measured: 5.8-6.0e-4 with f32 sums; fp16 sums 7.3e-4 inside the fused GEMMs, 8.5e-4 ahead of layernorm_fwd at emsize 1024)
            within(f'{name}, sep {sep}: loss rel vs oracle', abs(loss.item() - loss_o.item()) / abs(loss_o.item()), 2.5e-5)
            within(f'{name}, sep {sep}: global gradient rel l2 vs oracle', err, 1.4e-3)
            out[name] = (logits.detach(), g)
        within(f'sep {sep}: logits, fp16 sums vs f32 sums, rel l2', relerr(out['fp16 sums'][0], out['f32 sums'][0]), 1.6e-3)
        assert not torch.equal(out['fp16 sums'][0], out['f32 sums'][0])      # (the bit does select another arithmetic)


@pytest.mark.parametrize('target', [9, 12])
def test_fp16_backward_saturates_where_the_loss_scale_leaves_no_headroom(target):
    """fp16 backward with the loss-scale target pushed up (PFN_TUNE_LOSS_SCALE_TARGET): max|dlogits| lands at 2^9 or 2^12 -- seven or four binades below 65504 --
    so gradients along the chain leave the format.  Every kernel that stores fp16 runs with MODE.FP16_OVFL set (pfn_device.h operand_store_mode): the
    overflowing elements saturate at +-65504 and every parameter gradient stays finite -- without it they are inf, and NaN one product later (round 6: the
    GP-fitting recipe's weights were all NaN at epoch 68).  At the default target the same batch matches the oracle (test_config1_vs_oracle)."""
    cfg = dict(T=100, B=8, F=5, E=128, H=4, nhid=256, L=2, nbars=100)
    model = random_model(cfg, 'fp16', seed=3).to(DEV).train()
    with torch.no_grad():
        model.decoder[2].weight.mul_(40.)      # a confident head: d(hidden) = W^T dlogits is 40 x larger against max|dlogits|
    model.mark_params_updated()
    gen = torch.Generator().manual_seed(5)
    x, y, _ = pfn_oracle.get_batch_fast_gp(cfg['B'], cfg['T'], cfg['F'], {'noise': 1e-4, 'outputscale': 1., 'lengthscale': .6}, gen)
    lib = _hip.lib()
    assert lib.pfn_set_tuning(15, 13) != 0 and lib.pfn_set_tuning(15, -9) != 0      # outside -8 .. 12: refused
    grads = {}
    try:
        for tg in (2, target):
            _hip.check(lib.pfn_set_tuning(15, tg), 'pfn_set_tuning')
            for sep in (81, 1):
                model.zero_grad()
                logits = model((x.to(DEV), y.to(DEV)), single_eval_pos=sep)
                loss = model.criterion(logits.reshape(-1, cfg['nbars']), y[sep:].to(DEV).flatten()).mean()
                loss.backward()
                g = torch.cat([p.grad.flatten() for p in model.parameters()])
                assert torch.isfinite(g).all(), (tg, sep)
                grads[tg, sep] = g.clone()
    finally:
        _hip.check(lib.pfn_set_tuning(15, 2), 'pfn_set_tuning')
    for sep in (81, 1):       # the saturated gradient still points the way of the exact one
        a, b = grads[2, sep].double(), grads[target, sep].double()
        within(f'1 - cosine of the target-{target} gradient and the default one, sep {sep}', 1. - (a @ b / (a.norm() * b.norm())).item(), 8e-3)      # (measured 3.7e-3 at target 12, sep 1; 1e-11 where nothing saturates)


@pytest.mark.parametrize('H', [4, 16])
@pytest.mark.parametrize('precision', ['f32', 'bf16', 'fp16'])
def test_config5_width_vs_oracle(precision, H):
    """BASELINE config 5 width (emsize 1024, nhid 2048; nhead 4 -> head dim 256 as in the notebook, nhead 16 -> 64) at
    a length and depth the f64 oracle finishes in seconds: the kernels this width selects (head dim 256 attention,
    N = 1024 / 2048 GEMM epilogues, the unfused LayerNorm path) against explicit math."""
    cfg = dict(T=160, B=2, F=18, E=1024, H=H, nhid=2048, L=2, nbars=100)
    model = random_model(cfg, precision, seed=4)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    gen = torch.Generator().manual_seed(6)
    x, y, _ = pfn_oracle.get_batch_fast_gp(cfg['B'], cfg['T'], cfg['F'], {'noise': 1e-4, 'outputscale': 1., 'lengthscale': .6}, gen)
    sep = 131
    loss_o, logits_o, grads_o = pfn_oracle.loss_and_grads(sd, x, y, y, sep, cfg['H'], sd['criterion.borders'])
    model.zero_grad()
    logits = model((x.to(DEV), y.to(DEV)), single_eval_pos=sep)
    loss = model.criterion(logits.reshape(-1, cfg['nbars']), y[sep:].to(DEV).flatten()).mean()
    tight = precision == 'f32'
    within(f'{precision} H{H} loss rel', abs(loss.item() - loss_o.item()) / abs(loss_o.item()), tol3(precision, 1e-4, 1e-3, 1.0e-4))
    within(f'{precision} H{H} logits rel l2', relerr(logits, logits_o), tol3(precision, 1e-4, 1e-2, 1.8e-3))
    within(f'{precision} H{H} means max / target range', mean_err(model.criterion.mean(logits), pfn_oracle.bar_mean(logits_o, sd['criterion.borders']), y), tol3(precision, 1e-5, 1e-3, 2.4e-5))
    # (exact-f32 at head dim 256, round 5: the backward runs the plain vector-ALU attention kernels -- csrc/attention.hip attn_bwd_plain_* -- and is held to the
    # same 2e-4 "any layout mistake fails" bound as every other f32 shape)
    loss.backward()
    tot_err = math.sqrt(sum(((p.grad.double().cpu() - grads_o[k]) ** 2).sum().item() for k, p in model.named_parameters()))
    tot = math.sqrt(sum((g ** 2).sum().item() for g in grads_o.values()))
    within(f'{precision} H{H} global gradient rel l2', tot_err / tot, tol3(precision, 2e-4, 1.2e-2, 1.6e-3))


def test_full_size_properties_bf16():
    """North-star shape (bptt=2000, nf=18, emsize=512, nlayers=6, 1000 bars): size-independent properties of
    the mask: test outputs are invariant to permuting the train rows and to changing
    OTHER test rows; and the f32 and bf16 paths agree on the NLL within 1e-3."""
    cfg = dict(T=2000, B=2, F=18, E=512, H=4, nhid=1024, L=6, nbars=1000)
    sep = 1755
    model = random_model(cfg, 'bf16', seed=9).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(cfg['T'], cfg['B'], cfg['F'], generator=g).to(DEV)
    y = torch.randn(cfg['T'], cfg['B'], generator=g).to(DEV)
    with torch.no_grad():
        base = model((x, y), single_eval_pos=sep)
        perm = torch.randperm(sep, generator=g).to(DEV)
        xp, yp = x.clone(), y.clone()
        xp[:sep], yp[:sep] = x[perm], y[perm]
        permuted = model((xp, yp), single_eval_pos=sep)
        x2 = x.clone()
        x2[sep + 5] = torch.rand(cfg['B'], cfg['F'], generator=g).to(DEV)
        changed = model((x2, y), single_eval_pos=sep)
    assert torch.isfinite(base).all()
    assert relerr(permuted, base) < 2e-2          # same math, different bf16 summation order over keys
    keep = torch.ones(cfg['T'] - sep, dtype=torch.bool)
    keep[5] = False
    assert torch.equal(changed[keep], base[keep])  # other test rows are bit-identical
    assert not torch.equal(changed[5], base[5])
    # f32-mode cross check of the bar NLL at full size
    model32 = random_model(cfg, 'f32', seed=9).to(DEV).eval()
    with torch.no_grad():
        ref = model32((x, y), single_eval_pos=sep)
        nll16 = model.criterion(base.reshape(-1, 1000), y[sep:].flatten()).mean().item()
        nll32 = model32.criterion(ref.reshape(-1, 1000), y[sep:].flatten()).mean().item()
    assert abs(nll16 - nll32) < 1e-3 * abs(nll32), (nll16, nll32)
    # ... and of the backward: the global gradient of the product precision against the exact-f32 kernels at full size
    grads = {}
    for name, mdl in (('bf16', model), ('f32', model32)):
        mdl.train()
        mdl.flat_parameters()[1].zero_()
        out = mdl((x, y), single_eval_pos=sep)
        mdl.criterion(out.reshape(-1, 1000), y[sep:].flatten()).mean().backward()
        grads[name] = mdl.flat_parameters()[1].double().clone()
    assert torch.isfinite(grads['bf16']).all()
    within('bf16 vs f32-mode global gradient rel l2', ((grads['bf16'] - grads['f32']).norm() / grads['f32'].norm()).item(), 1.2e-2)


def test_negative_and_edge_eval_positions():
    cfg = dict(T=64, B=2, F=3, E=64, H=2, nhid=64, L=1, nbars=10)
    model = random_model(cfg, 'f32', seed=1).to(DEV).eval()
    x, y = torch.rand(64, 2, 3, device=DEV), torch.randn(64, 2, device=DEV)
    with torch.no_grad():
        a = model((x, y), single_eval_pos=-1)
        b = model((x, y), single_eval_pos=63)
        assert a.shape == (1, 2, 10) and torch.equal(a, b)
        assert model((x, y), single_eval_pos=64).shape == (0, 2, 10)
        assert model((x, y), single_eval_pos=0).shape == (64, 2, 10)
    xt = x.transpose(0, 1).contiguous().transpose(0, 1)  # the [B,T,F]-backed view priors return (fast_gp.py:58)
    with torch.no_grad():
        assert torch.equal(model((xt, y), single_eval_pos=10), model((x, y), single_eval_pos=10))


def test_cpu_tensors_fail_loudly():
    cfg = dict(T=16, B=1, F=2, E=64, H=2, nhid=64, L=1, nbars=4)
    model = random_model(cfg, 'bf16', seed=1)
    with pytest.raises(_hip.HipExtensionError):
        model((torch.rand(16, 1, 2), torch.rand(16, 1)), single_eval_pos=3)
    with pytest.raises(_hip.HipExtensionError):
        model.criterion(torch.randn(4, 4), torch.randn(4))


def test_gp_prior_sampler_vs_oracle():
    from transformerscandobayesianinference_amd.priors import fast_gp
    g = torch.Generator().manual_seed(3)
    for (B, T, F, hp, kernel) in [(3, 100, 5, (1e-4, 1.0, 0.6), 'rbf'), (2, 332, 18, (0.1, 0.1, 0.1), 'rbf'),
                                  (2, 2000, 18, (1e-4, 1.0, 0.6), 'rbf'), (2, 260, 4, (1e-2, 0.7, 0.5), 'matern'),
                                  (2, 196, 6, (1e-2, 1.3, 0.4), 'matern32'), (2, 132, 3, (1e-2, 0.9, 0.7), 'matern12')]:   # hyperparameters['nu'] of fast_gp_mix.py:40
        x = torch.rand(B, T, F, generator=g)
        z = torch.randn(B, T, generator=g)
        noise, os_, ls = hp
        want = pfn_oracle.gp_sample(x, z, ls, os_, noise, kernel)
        kid = {'rbf': fast_gp.KERNEL_RBF, 'matern': fast_gp.KERNEL_MATERN52, 'matern32': fast_gp.KERNEL_MATERN32, 'matern12': fast_gp.KERNEL_MATERN12}[kernel]
        _, got, _, info = fast_gp.gp_sample(B, T, F, DEV, ls, os_, noise, kid, x=x, z=z)
        assert int(info.abs().sum()) == 0
        err = relerr(got, want)
        assert err < 2e-3, (B, T, F, hp, err)   # f32 Cholesky of a cond ~1e6 matrix (6e-4 at nf=5)


def test_gp_sampler_block_structure_and_batch_placement():
    """The sampler's blocked factorisation at the sizes where its structure changes (256-wide outer blocks handled in PAIRS by the delayed trailing update:
    a strip after the even block, a rank-512 pass after the odd one; partial last blocks; exact multiples) and at batch sizes that take the dataset -> XCD
    placement of the wide kernels (B % 8 == 0) as well as the plain one -- every draw against the f64 oracle on the same (x, z), prior and posterior mode."""
    from transformerscandobayesianinference_amd.priors import fast_gp
    g = torch.Generator().manual_seed(21)
    for (B, T, F) in [(8, 516, 4), (16, 772, 3), (8, 1024, 5), (5, 1284, 4), (8, 600, 6), (24, 260, 3), (3, 1540, 4)]:
        x = torch.rand(B, T, F, generator=g)
        z = torch.randn(B, T, generator=g)
        osc = 0.5 + torch.rand(B, generator=g)              # per-dataset scales: the fp16 planes' power-of-two scale differs between datasets
        noise = 1e-2 * (0.5 + torch.rand(B, generator=g))
        ls = 0.3 + 0.5 * torch.rand(B, F, generator=g)
        want = pfn_oracle.gp_sample(x, z, ls, osc, noise, 'rbf')
        _, got, _, info = fast_gp.gp_sample(B, T, F, DEV, ls, osc, noise, fast_gp.KERNEL_RBF, x=x, z=z)
        assert int(info.abs().sum()) == 0
        per_dataset = ((got.double().cpu() - want).norm(dim=1) / want.norm(dim=1)).max().item()
        assert per_dataset < 1e-4, (B, T, F, per_dataset)    # measured 2e-6 .. 2e-5; a misplaced block or dataset gives O(1)
    # the same without the plane scratch (PFN_TUNE_GP_PLANES = 0; also what a caller whose K_ws holds the matrix alone gets): the wide solve stores its rows and
    # the update splits them per tile -- the round-2/3 form, one pass per outer block
    from transformerscandobayesianinference_amd import _hip
    _hip.check(_hip.lib().pfn_set_tuning(8, 0), 'pfn_set_tuning')
    try:
        for (B, T, F) in [(8, 772, 4), (3, 1284, 3)]:
            x = torch.rand(B, T, F, generator=g)
            z = torch.randn(B, T, generator=g)
            want = pfn_oracle.gp_sample(x, z, 0.5, 1.0, 1e-2, 'rbf')
            _, got, _, info = fast_gp.gp_sample(B, T, F, DEV, 0.5, 1.0, 1e-2, fast_gp.KERNEL_RBF, x=x, z=z)
            assert int(info.abs().sum()) == 0 and relerr(got, want) < 1e-4, (B, T, F, relerr(got, want))
    finally:
        _hip.check(_hip.lib().pfn_set_tuning(8, 1), 'pfn_set_tuning')
    for (B, T, F, hps) in [(8, 600, 4, (0.05, 1.0, 0.6)), (16, 516, 3, (0.1, 0.5, 0.4))]:
        x, y, _ = pfn_oracle.get_batch_fast_gp(B, T, F, hps, g)
        mean, var, nll, info = fast_gp.gp_posterior(x.transpose(0, 1).contiguous().to(DEV), y.transpose(0, 1).contiguous().to(DEV), hps[2], hps[1], hps[0])
        assert int(info.abs().sum()) == 0
        t64 = lambda v: torch.tensor(v, dtype=torch.float64).reshape(1, 1, 1)
        C = pfn_oracle.gp_gram(x.transpose(0, 1).double(), t64(hps[2]), t64(hps[1]), t64(hps[0]))
        joint = -torch.distributions.MultivariateNormal(torch.zeros(B, T, dtype=torch.float64), covariance_matrix=C).log_prob(y.transpose(0, 1).double())
        assert ((nll.double().sum(1).cpu() - joint).abs() / joint.abs()).max().item() < 1e-4, (B, T)      # chain rule, per dataset


def test_gp_prior_sampler_statistics():
    """Generated draws: x ~ U[0,1), and the empirical covariance of y matches os*RBF + noise*I."""
    from transformerscandobayesianinference_amd.priors import fast_gp
    torch.manual_seed(0)
    xs, ys, ts = fast_gp.get_batch(64, 24, 3, device=DEV, hyperparameters=(0.05, 1.0, 0.8))
    assert xs.shape == (24, 64, 3) and ys.shape == (24, 64) and ts is ys
    assert 0 <= xs.min().item() and xs.max().item() < 1 and abs(xs.mean().item() - 0.5) < 0.03
    # fix x across the batch to estimate the covariance
    x = torch.rand(1, 24, 3).expand(4096, 24, 3).contiguous()
    _, y, z, _ = fast_gp.gp_sample(4096, 24, 3, DEV, 0.8, 1.0, 0.05, fast_gp.KERNEL_RBF, x=x)
    assert abs(z.mean().item()) < 0.02 and abs(z.std().item() - 1) < 0.02
    emp = (y.double().t() @ y.double() / 4096).cpu()
    K = pfn_oracle.gp_gram(x[:1].double(), torch.tensor(0.8).reshape(1, 1, 1), torch.tensor(1.0).reshape(1, 1, 1), torch.tensor(0.05).reshape(1, 1, 1))[0]
    assert (emp - K).abs().max().item() < 0.12
    ys2 = fast_gp.get_batch(64, 24, 3, device=DEV, hyperparameters=(0.05, 1.0, 0.8))[1]
    assert not torch.equal(ys, ys2)


def test_gp_posterior_vs_oracle():
    """priors.fast_gp.evaluate: every sequential exact-GP prediction from ONE batched factorisation on the GPU against
    the oracle's one-Cholesky-per-position restatement of the reference loop (fast_gp.py:88-120).  f32 factorisation
    vs f64: 1e-3 relative on the losses the paper's baseline curve is drawn from (their mean per position)."""
    from transformerscandobayesianinference_amd.priors import fast_gp
    g = torch.Generator().manual_seed(11)
    for (B, T, F, hps) in [(4, 64, 3, (0.1, 0.1, 0.1)), (3, 201, 5, (0.05, 1.0, 0.6)), (2, 330, 18, (0.1, 0.1, 0.1))]:
        x, y, _ = pfn_oracle.get_batch_fast_gp(B, T, F, hps, g)
        want_nll, want_mean, want_var = pfn_oracle.gp_evaluate(x, y, hyperparameters=hps)
        losses, per_t, secs = fast_gp.evaluate(x, y, y, hyperparameters=hps, device=DEV)
        assert losses.shape == (T - 1, B) and per_t.shape == (T,) and per_t[0].item() == 0.0 and secs > 0
        assert (losses.double() - want_nll).abs().max().item() < 2e-3 * want_nll.abs().max().item(), (B, T, F)
        assert relerr(per_t[1:], want_nll.mean(1)) < 1e-3
        mean, var, nll, info = fast_gp.gp_posterior(x.transpose(0, 1).contiguous().to(DEV), y.transpose(0, 1).contiguous().to(DEV),
                                                    hps[2], hps[1], hps[0])
        assert int(info.abs().sum()) == 0
        # means relative to the range of y (far from every earlier point the true mean is ~0: no relative error there)
        assert (mean[:, 1:].t().double().cpu() - want_mean).abs().max().item() < 1e-3 * y.abs().max().item()
        assert relerr(var[:, 1:].t(), want_var) < 1e-3
        # position 0 is the prior: mean 0, variance outputscale + noise
        assert mean[:, 0].abs().max().item() < 1e-6 and torch.allclose(var[:, 0].cpu(), torch.full((B,), hps[1] + hps[0]), rtol=1e-5)
        mse, per_t2, _ = fast_gp.evaluate(x, y, y, use_mse=True, hyperparameters=hps, device=DEV, step_size=5, start_pos=2)
        want_mse, _, _ = pfn_oracle.gp_evaluate(x, y, use_mse=True, hyperparameters=hps, step_size=5, start_pos=2)
        assert mse.shape == want_mse.shape and per_t2.shape == (want_mse.shape[0],)
        assert (mse.double() - want_mse).abs().max().item() < 1e-3 * want_mse.abs().max().item()


def test_gp_posterior_full_size_chain_rule():
    """bptt = 2000 (north-star size), where the per-position oracle loop is too slow: the per-position negative log
    densities plus the prior term of position 0 must add up to the joint -log N(y; 0, C), computed in f64 on the CPU."""
    from transformerscandobayesianinference_amd.priors import fast_gp
    g = torch.Generator().manual_seed(12)
    B, T, F, hps = 2, 2000, 18, (0.1, 0.1, 0.1)
    x, y, _ = pfn_oracle.get_batch_fast_gp(B, T, F, hps, g)
    mean, var, nll, info = fast_gp.gp_posterior(x.transpose(0, 1).contiguous().to(DEV), y.transpose(0, 1).contiguous().to(DEV), hps[2], hps[1], hps[0])
    assert int(info.abs().sum()) == 0
    t64 = lambda v: torch.tensor(v, dtype=torch.float64).reshape(1, 1, 1)
    C = pfn_oracle.gp_gram(x.transpose(0, 1).double(), t64(hps[2]), t64(hps[1]), t64(hps[0]))
    joint = -torch.distributions.MultivariateNormal(torch.zeros(B, T, dtype=torch.float64), covariance_matrix=C).log_prob(y.transpose(0, 1).double())
    assert relerr(nll.double().sum(1), joint) < 1e-4
    assert (var > 0).all() and (var.cpu() <= hps[1] + hps[0] + 1e-5).all()   # conditioning never adds variance


def test_gp_mix_sampler_per_dataset_hyperparameters_vs_oracle():
    """priors.fast_gp_mix path of the sampler: Matern-5/2, ARD lengthscales and per-dataset outputscale / noise,
    against the f64 restatement on injected (x, z) (reference priors/fast_gp_mix.py:28-47, 96-99)."""
    from transformerscandobayesianinference_amd.priors import fast_gp, fast_gp_mix
    g = torch.Generator().manual_seed(5)
    for (B, T, F) in [(4, 130, 3), (3, 516, 18)]:
        x = torch.rand(B, T, F, generator=g)
        z = torch.randn(B, T, generator=g)
        ls, osc, nz = fast_gp_mix.sample_hyperparameters(B, F, None, 'cpu', generator=g)
        ls = ls.clamp_min(0.05)   # keep cond(K) where an f32 Cholesky is meaningful for the comparison
        want = pfn_oracle.gp_sample(x, z, ls, osc, nz, 'matern')
        _, got, _, info = fast_gp.gp_sample(B, T, F, DEV, ls, osc, nz, fast_gp.KERNEL_MATERN52, x=x, z=z)
        assert int(info.abs().sum()) == 0
        assert relerr(got, want) < 2e-3, (B, T, F, relerr(got, want))


def test_gp_mix_get_batch_and_validate():
    from transformerscandobayesianinference_amd.priors import fast_gp_mix
    torch.manual_seed(11)
    x, y, t = fast_gp_mix.get_batch(20, 64, 4, device=DEV)
    assert x.shape == (64, 20, 4) and y.shape == (64, 20) and t is y
    assert torch.isfinite(y).all() and 0 <= x.min() and x.max() < 1
    # the default hyper-prior has E[noise] = 22 and E[outputscale] = 3.3: marginal std of y is sqrt(os + noise)
    _, ybig, _ = fast_gp_mix.get_batch(400, 32, 2, device=DEV)
    assert 3.0 < ybig.std().item() < 8.0
    xn, yn, _ = fast_gp_mix.get_batch(10, 50, 2, device=DEV, hyperparameters={'y_minmax_norm': True})
    assert yn.min().item() == 0.0 and yn.max().item() == 1.0
    hp = {'outputscale_concentration': 2.0, 'outputscale_rate': 40.0, 'noise_concentration': 1.1, 'noise_rate': 400.0}
    xr, yr, _ = fast_gp_mix.get_batch(16, 40, 2, device=DEV, hyperparameters=hp, fix_to_range=(-1.0, 1.0))
    assert yr.shape == (40, 16) and yr.min() >= -1.0 and yr.max() < 1.0
    # DataLoader.validate: forward-only sweeps over the evaluation positions through the HIP stack
    dl = fast_gp_mix.DataLoader(num_steps=1, batch_size=4, seq_len=24, num_features=3, device=DEV, hyperparameters=hp)
    borders = bar_distribution.get_bucket_limits(20, ys=yr.flatten().cpu())
    model = TransformerModel(encoders.Linear(3, 64), 20, 64, 2, 128, 1, 0.0, y_encoder=encoders.Linear(1, 64), precision='bf16', eval_precision='bf16')
    model.criterion = bar_distribution.FullSupportBarDistribution(borders)
    model.to(DEV)
    scores = dl.validate(model, step_size=6, start_pos=3)
    assert scores.shape == (4,) and torch.isfinite(scores).all()


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_mlp_prior_kernel_vs_reference_golden():
    """The BNN-prior kernel on the very tensors the reference drew (tests/golden/mlp_prior.pt): injected parameters,
    causes and layer noise must reproduce the reference's priors.mlp.get_batch output."""
    from transformerscandobayesianinference_amd.priors import mlp
    rec = torch.load(os.path.join(GOLD, 'mlp_prior.pt'))
    cfg = rec['config']
    T, B, NF, PER = cfg['T'], cfg['B'], cfg['NF'], cfg['PER']
    M = B // PER
    weights = [[rec['params'][6 * m + 2 * l] for l in range(3)] for m in range(M)]
    biases = [[rec['params'][6 * m + 2 * l + 1] for l in range(3)] for m in range(M)]
    W, b, dims, HP = mlp.pack_networks(weights, biases, DEV)
    causes = torch.zeros(B, T, HP)
    noise = torch.zeros(B, 2, T, HP)
    for i in range(B):
        c, n1, n2 = [t[:, 0, :] for t in rec['normals'][3 * i: 3 * i + 3]]
        causes[i, :, :c.shape[1]] = c
        noise[i, 0, :, :n1.shape[1]] = n1
        noise[i, 1, :, :n2.shape[1]] = n2
    model_of = (torch.arange(B, dtype=torch.int32) // PER).to(DEV)
    ones = torch.ones(M, device=DEV)   # the recorded noise tensors already carry their std
    got_c, y_raw = mlp.forward_networks(W, b, dims, ones, model_of, T, 2, causes=causes.to(DEV), noise=noise.to(DEV))
    nfu = dims[:, 0][model_of.long()]
    for i in range(B):
        m = i // PER
        want = pfn_oracle.mlp_prior_forward([w_.double() for w_ in weights[m]], [b_.double() for b_ in biases[m]], causes[i, :, :weights[m][0].shape[1]].double(),
                                            [noise[i, 0, :, :weights[m][1].shape[0]].double(), noise[i, 1, :, :1].double()], 'tanh')
        assert relerr(y_raw[i], want) < 1e-5, (i, relerr(y_raw[i], want))
    sign = torch.tensor([1.0 if c else -1.0 for c in rec['coins']], device=DEV)
    x, y = mlp.postprocess(got_c, y_raw, nfu, NF, True, sign)
    assert torch.equal(y.cpu().t(), rec['y'])            # class pattern after order_by_y
    xr = rec['x'].transpose(0, 1)                        # [B,T,NF]; ties inside a class may be ordered differently:
    for i in range(B):                                   # compare each class's rows as sorted sets
        for cls in (0.0, 1.0):
            a_ = x[i][y[i] == cls].cpu()
            b_ = xr[i][rec['y'][:, i] == cls]
            assert torch.allclose(a_[a_[:, 0].argsort()], b_[b_[:, 0].argsort()], atol=2e-5, rtol=2e-5), (i, cls)


def test_mlp_prior_causal_branches_vs_reference_golden():
    """The causal-graph / categorical / pre-sampled-noise-scale branches (reference priors/mlp.py:94-104, 119-121, 139-140, 158-179) on the
    tensors the reference drew (tests/golden/mlp_prior_causal.pt): the kernel's per-layer node outputs, the node selection, the
    categorical discretisation and the tail of the forward must reproduce the reference's get_batch output."""
    from transformerscandobayesianinference_amd.priors import mlp
    rec = torch.load(os.path.join(GOLD, 'mlp_prior_causal.pt'))
    cfg = rec['config']
    T, B, NF, PER, NFU, HID = cfg['T'], cfg['B'], cfg['NF'], cfg['PER'], cfg['NFU'], cfg['hidden']
    M = B // PER
    weights = [[rec['params'][6 * m + 2 * l] for l in range(3)] for m in range(M)]
    biases = [[rec['params'][6 * m + 2 * l + 1] for l in range(3)] for m in range(M)]
    W, b, dims, HP = mlp.pack_networks(weights, biases, DEV)
    causes = torch.zeros(B, T, HP)
    noise = torch.zeros(B, 2, T, HP)
    for i in range(B):
        c, n1, n2 = [t[:, 0, :].float() for t in rec['normals'][2 * M + 3 * i: 2 * M + 3 * i + 3]]
        causes[i, :, :c.shape[1]] = c
        noise[i, 0, :, :n1.shape[1]] = n1
        noise[i, 1, :, :n2.shape[1]] = n2
    model_of = (torch.arange(B, dtype=torch.int32) // PER).to(DEV)
    ones = torch.ones(M, device=DEV)   # the recorded noise tensors already carry their per-unit scales
    _, _, hidden = mlp.forward_networks(W, b, dims, ones, model_of, T, 2, causes=causes.to(DEV), noise=noise.to(DEV), want_hidden=True)
    x_raw = torch.zeros(B, T, 4, device=DEV)
    y_raw = torch.zeros(B, T, device=DEV)
    for i in range(B):
        xs, ys = mlp.causal_select(hidden[i:i + 1], 3, HID, NFU, False, perm=rec['perms'][2 * i][None].to(DEV))
        x_raw[i:i + 1] = mlp.categorical_columns(xs.clone(), cfg['cats'], cfg['ordinal'], perm=rec['perms'][2 * i + 1][None].to(DEV))
        y_raw[i:i + 1] = ys
        m = i // PER
        outs = pfn_oracle.mlp_prior_layers([w_.double() for w_ in weights[m]], [b_.double() for b_ in biases[m]], causes[i, :, :5].double(),
                                           [noise[i, 0, :, :HID].double(), noise[i, 1, :, :1].double()], 'tanh')
        want_x, want_y = pfn_oracle.mlp_prior_causal_select(outs, rec['perms'][2 * i], NFU)
        assert relerr(ys[0], want_y) < 1e-5 and relerr(xs[0], want_x) < 1e-5
    sign = torch.tensor([1.0 if c else -1.0 for c in rec['coins']], device=DEV)
    nfu = torch.full((B,), NFU, device=DEV)
    x, y = mlp.postprocess(x_raw, y_raw, nfu, NF, True, sign)
    assert torch.equal(y.cpu().t(), rec['y'])
    xr = rec['x'].transpose(0, 1)
    for i in range(B):
        for cls in (0.0, 1.0):
            a_ = x[i][y[i] == cls].cpu()
            b_ = xr[i][rec['y'][:, i] == cls]
            wv = torch.tensor([1.0, 0.7310585786, 0.4142135624, 0.2360679775, 0.1415926536, 0.0577215665])
            key = lambda t_: (t_.double() * wv.double()).sum(1)     # columns can be categorical (ties): order rows by a generic projection
            assert torch.allclose(a_[key(a_).argsort()], b_[key(b_).argsort()], atol=2e-4, rtol=2e-4), (i, cls)
    # and the public entry point runs every branch end to end
    import numpy as np
    hps = (lambda: 3, lambda: 7, torch.nn.Tanh, lambda: 0.8, lambda: 0.05, lambda: 0.1, True, lambda: 4,
           lambda: (np.random.normal(0, 1, 5), np.abs(np.random.normal(0, 1, 5))), True, True, True, False, True, True,
           lambda n: ([np.random.rand(3), np.random.rand(2)], [True, False]), 0.0)
    xg, yg, _ = mlp.get_batch(8, 64, 6, device=DEV, hyperparameters=hps, batch_size_per_gp_sample=4)
    assert xg.shape == (64, 8, 6) and yg.shape == (64, 8) and set(yg.unique().tolist()) <= {0.0, 1.0}
    assert torch.isfinite(xg).all() and (xg[:, :, 4:] == 0).all() and (xg[:, :, :4].abs().sum(0) > 0).float().mean() > 0.5   # (a categorical column may be constant)
    xe, ye, _ = mlp.get_batch(8, 64, 6, device=DEV, hyperparameters=hps[:12] + (True,) + hps[13:], batch_size_per_gp_sample=4)   # y_is_effect
    assert torch.isfinite(xe).all() and set(ye.unique().tolist()) <= {0.0, 1.0}


def test_mlp_prior_get_batch():
    from transformerscandobayesianinference_amd.priors import mlp
    from transformerscandobayesianinference_amd.priors.utils import gamma_sampler_f, scaled_beta_sampler_f
    import numpy as np
    torch.manual_seed(3); random.seed(3); np.random.seed(3)
    hps = (lambda: 3, scaled_beta_sampler_f(2., 4., 150, 2), torch.nn.Tanh, gamma_sampler_f(3.6187797729244253, 0.06773738681062867),
           gamma_sampler_f(1.8663049257557085, 0.05275478076173361), lambda: 0.0, True, scaled_beta_sampler_f(1., 1.6, 60, 2),
           None, False, None, None, None, True, False, lambda n: ([], []), 0.0)
    x, y, t = mlp.get_batch(64, 1000, 60, device=DEV, hyperparameters=hps, batch_size_per_gp_sample=8)
    assert x.shape == (1000, 64, 60) and y.shape == (1000, 64) and t is y
    assert set(y.unique().tolist()) <= {0.0, 1.0}
    assert (y.mean(0) - 0.5).abs().max() <= 0.002             # median split of 1000 rows
    assert torch.equal(y[0::2].sum(0) + y[1::2].sum(0), y.sum(0))
    used = (x.abs().sum(0) > 0)                                 # [B, F]
    assert (used.sum(1) >= 2).all() and (used.sum(1) <= 60).all()
    xm, xs = x.mean(0)[used], x.std(0)[used]
    assert xm.abs().max() < 1e-3 and (xs - 1).abs().max() < 1e-3
    # order_by_y interleaves the sorted halves: row 2k comes from the first half, row 2k+1 from the second
    d = (y[1::2] - y[0::2])
    assert (d.abs().sum(0) > 0).all() and ((d >= 0).all(0) | (d <= 0).all(0)).all()
    # the DataLoader protocol (prefetching iterator) and a second, different draw
    dl = mlp.DataLoader(num_steps=2, batch_size=16, seq_len=100, num_features=60, device=DEV, hyperparameters=hps, batch_size_per_gp_sample=8)
    batches = list(dl)
    assert len(batches) == 2 and batches[0][0][0].shape == (100, 16, 60)
    assert not torch.equal(batches[0][0][0], batches[1][0][0])


def test_train_entry_point_with_every_prior():
    """train() (reference train.py:22-135 call surface) drives all three priors through the HIP stack: GP + adaptive
    full-support bar NLL (configs 1-3), BNN prior + BCE (config 4, tabular.py:129), GP mixture + bar NLL with its
    validate() sweep (config 5)."""
    import numpy as np
    from transformerscandobayesianinference_amd import train as train_mod, utils as u
    from transformerscandobayesianinference_amd.priors import fast_gp, fast_gp_mix, mlp
    from transformerscandobayesianinference_amd.priors.utils import gamma_sampler_f, scaled_beta_sampler_f
    torch.manual_seed(1); random.seed(1); np.random.seed(1)
    common = dict(emsize=64, nhid=128, nlayers=2, nhead=2, dropout=0.0, epochs=2, steps_per_epoch=2, batch_size=8, lr=1e-3, warmup_epochs=1,
                  y_encoder_generator=encoders.Linear, gpu_device=DEV, verbose=False)
    ys = fast_gp.get_batch(64, 20, 3, device=DEV, hyperparameters=(1e-4, 1., .6))[1].cpu()
    crit = bar_distribution.FullSupportBarDistribution(bar_distribution.get_bucket_limits(20, ys=ys))
    loss, pos, model = train_mod.train(fast_gp.DataLoader, crit, encoders.Linear, bptt=40, single_eval_pos_gen=u.get_weighted_single_eval_pos_sampler(40),
                                       extra_prior_kwargs_dict={'num_features': 3, 'hyperparameters': (1e-4, 1., .6), 'device': DEV}, **common)
    assert math.isfinite(loss) and next(model.parameters()).device.type == 'cpu'
    hps = (lambda: 3, scaled_beta_sampler_f(2., 4., 30, 2), torch.nn.Tanh, gamma_sampler_f(3.6, 0.07), gamma_sampler_f(1.9, 0.05), lambda: 0.0, True,
           scaled_beta_sampler_f(1., 1.6, 12, 2), None, False, None, None, None, True, False, lambda n: ([], []), 0.0)
    loss, pos, model = train_mod.train(mlp.DataLoader, train_mod.Losses.bce, encoders.Linear, bptt=40, single_eval_pos_gen=u.get_uniform_single_eval_pos_sampler(40),
                                       extra_prior_kwargs_dict={'num_features': 12, 'hyperparameters': hps, 'batch_size_per_gp_sample': 4, 'device': DEV}, **common)
    assert math.isfinite(loss) and 0.3 < loss < 1.5          # BCE of a barely trained classifier on balanced labels
    mix_hp = {'outputscale_concentration': 2.0, 'outputscale_rate': 40.0, 'noise_concentration': 1.1, 'noise_rate': 400.0}
    ys = fast_gp_mix.get_batch(64, 20, 3, device=DEV, hyperparameters=mix_hp)[1].cpu()
    crit = bar_distribution.FullSupportBarDistribution(bar_distribution.get_bucket_limits(20, ys=ys))
    loss, pos, model = train_mod.train(fast_gp_mix.DataLoader, crit, encoders.Linear, bptt=40, single_eval_pos_gen=u.get_weighted_single_eval_pos_sampler(40),
                                       validation_period=1, extra_prior_kwargs_dict={'num_features': 3, 'hyperparameters': mix_hp, 'device': DEV}, **common)
    assert math.isfinite(loss)


def test_micro_batch_streams_match_single_stream():
    """Concurrent column groups of a batch on two / three / four HIP streams (streams.py) give the full-batch loss and gradients; three groups of a batch of 8
    are 3 + 3 + 2 datasets, each weighted by its share."""
    from transformerscandobayesianinference_amd.priors import fast_gp
    from transformerscandobayesianinference_amd.streams import MicroBatchStreams
    torch.manual_seed(2)
    T, B, F, E, nb, sep = 120, 8, 4, 128, 30, 77
    x, y, target = fast_gp.get_batch(B, T, F, device=DEV, hyperparameters=(1e-4, 1., .6))
    borders = bar_distribution.get_bucket_limits(nb, ys=y.flatten().cpu())
    model = TransformerModel(encoders.Linear(F, E), nb, E, 2, 256, 2, 0.0, y_encoder=encoders.Linear(1, E), precision='bf16', eval_precision='bf16')
    model.criterion = bar_distribution.FullSupportBarDistribution(borders)
    with torch.no_grad():
        for layer in model.transformer_encoder.layers:
            layer.linear2.weight.normal_(0, 0.05)
            layer.self_attn.out_proj.weight.normal_(0, 0.05)
    model.to(DEV).train()
    loss_fn = lambda out, tg: model.criterion(out.reshape(-1, nb), tg[sep:].reshape(-1)).view(out.shape[0], -1)
    grads = []
    for n in (1, 2, 3, 4):
        flat, g = model.flat_parameters()
        g.zero_()
        losses = MicroBatchStreams(n).forward_backward(model, (x, y), target, sep, loss_fn)
        torch.cuda.synchronize()
        grads.append((losses.mean().item(), model.flat_parameters()[1].clone()))
    for loss_n, g_n in grads[1:]:
        assert abs(loss_n - grads[0][0]) < 1e-5 * abs(grads[0][0])
        assert relerr(g_n, grads[0][1]) < 1e-4, relerr(g_n, grads[0][1])


def test_tabular_get_model_and_checkpoint_roundtrip(tmp_path):
    """tabular.get_model (reference tabular.py:109-155) trains a tiny BNN-prior classifier through the HIP path; the
    notebooks' `(state_dict, None)` checkpoint tuple (BayesianModels...ipynb cells 14/16, TabularEvalSimple cell 12)
    written from it loads into a freshly built (`should_train=False`) model with identical predictions, and its keys
    are the reference's state-dict keys."""
    import numpy as np
    from test_host import _tabular_config
    from transformerscandobayesianinference_amd import tabular
    from transformerscandobayesianinference_amd.priors import mlp
    torch.manual_seed(4); random.seed(4); np.random.seed(4)
    cfg = _tabular_config('mlp')
    loss, pos, model = tabular.get_model(cfg, DEV, eval_positions=[10, 20, 30], should_train=True, steps_per_epoch=3)
    assert math.isfinite(loss) and len(pos) == cfg['bptt']
    path = str(tmp_path / 'pfn.cpkt')
    tabular.save_checkpoint(model, path)
    state, opt = torch.load(path)
    assert opt is None
    keys = set(state)
    for k in ['encoder.weight', 'y_encoder.bias', 'transformer_encoder.layers.0.self_attn.in_proj_weight',
              'transformer_encoder.layers.1.self_attn.out_proj.bias', 'transformer_encoder.layers.0.linear1.weight',
              'transformer_encoder.layers.1.linear2.bias', 'transformer_encoder.layers.0.norm1.weight',
              'transformer_encoder.layers.1.norm2.bias', 'decoder.0.weight', 'decoder.2.bias']:
        assert k in keys, k
    assert state['transformer_encoder.layers.0.self_attn.in_proj_weight'].shape == (3 * cfg['emsize'], cfg['emsize'])
    assert state['decoder.2.weight'].shape == (1, cfg['emsize'] * cfg['nhid_factor'])
    _, _, fresh = tabular.get_model(cfg, DEV, eval_positions=[10, 20, 30], should_train=False)
    assert tabular.load_checkpoint(fresh, path) is None
    x, y, _ = mlp.get_batch(4, cfg['bptt'], cfg['num_features'], device=DEV, hyperparameters=tabular.get_mlp_prior_hyperparameters(cfg),
                            batch_size_per_gp_sample=4)
    model.to(DEV).eval(); fresh.to(DEV).eval()
    with torch.no_grad():
        a = model((x, y), single_eval_pos=25)
        b = fresh((x, y), single_eval_pos=25)
    assert a.shape == (cfg['bptt'] - 25, 4, 1) and torch.equal(a, b)


def test_binarized_regression_priors():
    """priors.binarized_regression (reference :4-21): labels ~ Bernoulli(sigmoid(y)) of a HIP GP draw."""
    from transformerscandobayesianinference_amd.priors import binarized_regression as br
    torch.manual_seed(0)
    for cls, kw in [(br.Binarized_fast_gp_dataloader, {'hyperparameters': (1e-4, 1., .6)}), (br.Binarized_fast_gp_mix_dataloader, {})]:
        dl = cls(num_steps=1, batch_size=64, seq_len=32, num_features=3, device=DEV, **kw)
        (x, y), target = next(iter(dl))
        assert x.shape == (32, 64, 3) and y.shape == (32, 64) and target is y and x.is_cuda
        assert set(y.unique().tolist()) <= {0., 1.} and 0.25 < y.mean().item() < 0.75
    assert cls.num_outputs == 1


def test_evaluation_sweeps():
    """evaluation.run_test (notebook SetupForGPFittingExperiments.ipynb cell 6) and the exact-GP curve it is compared
    with: shapes / finiteness of the 5-tuple on a barely trained PFN, and the baseline's sanity -- more training points
    never hurt an exact GP on its own prior, and no PFN beats it on average."""
    import numpy as np
    from transformerscandobayesianinference_amd import evaluation, train as train_mod, utils as u
    from transformerscandobayesianinference_amd.priors import fast_gp
    torch.manual_seed(5); random.seed(5); np.random.seed(5)
    hps = (1e-2, 1., .6)
    ys = fast_gp.get_batch(256, 20, 2, device=DEV, hyperparameters=hps)[1].cpu()
    crit = bar_distribution.FullSupportBarDistribution(bar_distribution.get_bucket_limits(50, ys=ys))
    _, _, model = train_mod.train(fast_gp.DataLoader, crit, encoders.Linear, emsize=64, nhid=128, nlayers=2, nhead=2, dropout=0.0, epochs=2,
                                  steps_per_epoch=4, batch_size=16, lr=1e-3, warmup_epochs=1, y_encoder_generator=encoders.Linear, gpu_device=DEV,
                                  verbose=False, bptt=40, single_eval_pos_gen=u.get_weighted_single_eval_pos_sampler(40),
                                  extra_prior_kwargs_dict={'num_features': 2, 'hyperparameters': hps, 'device': DEV})
    pos, mse, mode_mse, nll, conf = evaluation.run_test(model, DEV, step_size=12, start_pos=1, batch_size=64, sub_batch_size=32, seq_len=40,
                                                        num_features=2, hyperparameters=hps)
    assert pos == [1, 13, 25, 37]
    for t in (mse, mode_mse, nll, conf):
        assert t.shape == (4,) and torch.isfinite(t).all()
    assert (mse > 0).all() and (conf > 0).all()
    gpos, gmse, gnll, gconf = evaluation.gp_baseline(DEV, step_size=12, start_pos=1, batch_size=256, sub_batch_size=128, seq_len=40,
                                                     num_features=2, hyperparameters=hps)
    assert gpos == pos and gmse.shape == gnll.shape == gconf.shape == (4,)
    assert gnll[-1] < gnll[0] - 0.3 and gmse[-1] < 0.5 * gmse[0]          # 37 training points vs 1
    assert (gnll < nll + 3 * (conf + gconf)).all()                        # the Bayes-optimal predictor is not beaten
    m, h = evaluation.compute_mean_and_conf_interval([1., 2., 3., 4.])
    assert m == 2.5 and abs(h - 2.0541) < 1e-3


def test_train_option_matrix():
    """The less travelled arguments of train() (reference train.py:22-27): gradient aggregation over k batches, Gaussian
    NLL head (two outputs per point), sinusoidal / learned positional encodings, input normalisation (SeqBN), MSE loss.
    Each runs a few optimizer steps through the HIP stack and must produce a finite loss."""
    import numpy as np
    from torch import nn
    from transformerscandobayesianinference_amd import positional_encodings as pe, train as train_mod, utils as u
    from transformerscandobayesianinference_amd.priors import fast_gp
    torch.manual_seed(6); random.seed(6); np.random.seed(6)
    base = dict(emsize=64, nhid=128, nlayers=2, nhead=2, dropout=0.0, epochs=1, steps_per_epoch=4, batch_size=8, lr=1e-3, warmup_epochs=0,
                y_encoder_generator=encoders.Linear, gpu_device=DEV, verbose=False, bptt=32,
                extra_prior_kwargs_dict={'num_features': 3, 'hyperparameters': (1e-2, 1., .6), 'device': DEV})
    ys = fast_gp.get_batch(64, 20, 3, device=DEV, hyperparameters=(1e-2, 1., .6))[1].cpu()
    bars = lambda: bar_distribution.FullSupportBarDistribution(bar_distribution.get_bucket_limits(20, ys=ys))
    cases = [
        dict(criterion=bars(), aggregate_k_gradients=2, single_eval_pos_gen=u.get_weighted_single_eval_pos_sampler(32)),
        dict(criterion=nn.GaussianNLLLoss(reduction='none', full=True), single_eval_pos_gen=u.get_uniform_single_eval_pos_sampler(32)),
        dict(criterion=nn.MSELoss(reduction='none'), single_eval_pos_gen=20, pos_encoder_generator=pe.PositionalEncoding),
        dict(criterion=bars(), single_eval_pos_gen=u.get_weighted_single_eval_pos_sampler(32), pos_encoder_generator=pe.LearnedPositionalEncoding),
        dict(criterion=bars(), single_eval_pos_gen=u.get_weighted_single_eval_pos_sampler(32), input_normalization=True),
        dict(criterion=bars(), single_eval_pos_gen=u.get_weighted_single_eval_pos_sampler(32), micro_streams=1),
        dict(criterion=bars(), single_eval_pos_gen=u.get_weighted_single_eval_pos_sampler(32), dropout=0.2),          # the reference's default (train.py:22)
        dict(criterion=bars(), single_eval_pos_gen=20, dropout=0.5, pos_encoder_generator=pe.PositionalEncoding),      # (the tabular notebook's value; PyTorch-side embedding)
    ]
    for extra in cases:
        kw = dict(base); kw.update(extra)
        crit = kw.pop('criterion')
        loss, pos, model = train_mod.train(fast_gp.DataLoader, crit, encoders.Linear, **kw)
        assert math.isfinite(loss), extra
        assert len(pos) == 32


_DP_GPU_SCRIPT = r"""
import os, sys, random, math, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))
from transformerscandobayesianinference_amd import dp, bar_distribution, encoders
from transformerscandobayesianinference_amd.optim import FusedClipAdam
from transformerscandobayesianinference_amd.transformer import TransformerModel
rank, world, local = dp.init_from_env()                 # PFN_DP_BACKEND=gloo, PFN_DP_SINGLE_DEVICE=1: both ranks on cuda:0
dev = torch.device('cuda', local)
torch.cuda.set_device(dev)
T, B, F, E, nb, sep = 96, 8, 4, 128, 24, 61
def build():
    torch.manual_seed(0)
    m = TransformerModel(encoders.Linear(F, E), nb, E, 2, 256, 2, 0.0, y_encoder=encoders.Linear(1, E), precision='f32', eval_precision='f32')
    m.criterion = bar_distribution.FullSupportBarDistribution(torch.linspace(-4, 4, nb + 1))
    with torch.no_grad():
        for layer in m.transformer_encoder.layers:
            layer.linear2.weight.normal_(0, 0.05); layer.self_attn.out_proj.weight.normal_(0, 0.05)
    return m.to(dev).train()
g = torch.Generator().manual_seed(1)
x, y = torch.rand(T, B, F, generator=g).to(dev), (torch.randn(T, B, generator=g) * 0.8).to(dev)
def run(model, cols):
    model.flat_parameters()[1].zero_()
    out = model((x[:, cols], y[:, cols]), single_eval_pos=sep)
    loss = model.criterion(out.reshape(-1, nb), y[sep:, cols].reshape(-1)).mean()
    loss.backward()
    return loss.detach(), model.flat_parameters()[1]
model = build()
h = B // world
# the production path: two collectives, the top layer's half of the buffer enqueued behind its (early) weight-gradient launch
reducer = dp.OverlappedGradientReducer(model)
assert reducer.first_group_layers == 1 and reducer.split == model.layer_offset(1)
reducer.arm(1)
loss, grad = run(model, slice(rank * h, (rank + 1) * h))        # this rank's shard of the global batch
assert len(reducer.events) == 1                                  # pfn_stack_backward_split called back behind the first group
reducer.finish()
assert reducer.overlapped_last_step
grad = grad / world
ref_loss, ref_grad = run(build(), slice(0, B))                   # the global batch in one process
err = ((grad - ref_grad).norm() / ref_grad.norm()).item()
assert err < 1e-5, err
# one fused clip + Adam step with the 1/world factor folded in leaves every rank with the single-process weights
m1, m2 = build(), build()
o1 = FusedClipAdam(m1, lr=1e-3, max_grad_norm=1.0); o1.grad_multiplier = 1.0 / world
run(m1, slice(rank * h, (rank + 1) * h)); dp.all_reduce_gradients(m1.flat_parameters()[1]); o1.step(zero_grad=True)   # (the one-collective helper)
o2 = FusedClipAdam(m2, lr=1e-3, max_grad_norm=1.0)
g2 = run(m2, slice(0, B))[1].clone(); o2.step(zero_grad=True)
dw = (m1.flat_parameters()[0] - m2.flat_parameters()[0]).abs()
# Adam's first step moves every element by lr * g / (|g| + eps): where the gradient is rounding noise around zero (the key bias:
# softmax is invariant to it) the two summation orders may disagree about the whole step, so the tight bound is asserted where
# the gradient is a gradient and the step size everywhere
real = g2.abs() > 1e-3 * g2.abs().max()      # (1e-6 until round 5: one full-suite run in six failed here -- the f32 atomics' summation-order noise reaches that level; 1e-4 until the end
                                             # of round 6: one run in ten)
werr = dw[real].max().item()
assert werr < 2e-5, werr          # 2 % of one Adam step (lr 1e-3)
assert dw.max().item() <= 2.1e-3, dw.max().item()
print('rank', rank, 'ok', err, werr)
"""


def test_data_parallel_gradient_equals_global_batch(tmp_path):
    """SURVEY.md 8(e) end to end on the GPU: two ranks, each running the HIP forward / backward on its half of a batch,
    all-reduce the flat gradient buffer -- as the two collectives of dp.OverlappedGradientReducer, the upper layer's half behind the
    early weight-gradient launch of pfn_stack_backward_split; the average equals the single-process gradient of the whole batch and
    one fused optimizer step leaves identical weights.  RCCL refuses two ranks on one device, so the one-GPU box runs the ranks over
    gloo on cuda:0 (dp.py test hooks); the collective call, the buffers and the optimizer path are the production ones."""
    import subprocess, sys
    script = tmp_path / 'dp_gpu_check.py'
    script.write_text(_DP_GPU_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _PORT = _free_port()      # (a fixed port collided once in a full-suite run: a listener of an earlier test was still closing)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=_PORT, PFN_DP_BACKEND='gloo', PFN_DP_SINGLE_DEVICE='1')
    res = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
                          '--master-port', _PORT, str(script), root], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert res.stdout.count(' ok ') == 2


# ---- round 2: the benchmarked shapes against the oracle -------------------------------------------------------------------
def _bench():
    import importlib, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module('bench')


@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'f32'])
def test_config2_full_shape_vs_oracle(precision):
    """BASELINE configs[1] at its real size (bptt 2000, 18 features, emsize 512, 6 layers, 1000 bars): the HIP forward + bar NLL +
    posterior means against the f64 oracle on the same fixed-seed GP draw and the same weights -- what bench.py reports as
    `parity` (north_star: 1e-3 on the NLL and the means)."""
    bench = _bench()
    w = bench.CONFIGS[2]
    model = bench.build_model(DEV, precision, w)
    par, _ = bench.parity_check(model, w, torch.device(DEV), precision)
    # inference outputs (model.eval() under no_grad): exact-f32 kernels whatever the training precision -- the north star's 1e-3 with room
    assert par['precision'] == 'f32'
    within(f'{precision} model, inference outputs: nll rel', par['nll_rel'], 1e-5)
    within(f'{precision} model, inference outputs: means rel l2 (own norm)', par['mean_rel_l2'], 1e-3)
    within(f'{precision} model, inference outputs: means max / target range', par['mean_max_over_y_range'], 1e-6)
    within(f'{precision} model, inference outputs: logits rel l2', par['logits_rel_l2'], 1e-4)
    # the forward of the training path in the model's training precision
    tight = precision == 'f32'
    tf = par['training_forward']
    assert tf['precision'] == precision
    within(f'{precision} training forward: nll rel', tf['nll_rel'], tol3(precision, 1e-5, 1e-3, 1.1e-5))
    within(f'{precision} training forward: means max / target range', tf['mean_max_over_y_range'], tol3(precision, 1e-6, 1e-3, 6.4e-6))
    within(f'{precision} training forward: means rel l2 vs targets', tf['mean_rel_l2_vs_targets'], tol3(precision, 1e-6, 1e-3, 1.7e-5))
    within(f'{precision} training forward: logits rel l2', tf['logits_rel_l2'], tol3(precision, 1e-4, 1e-2, 1.7e-3))


@pytest.mark.parametrize('sep', [437, 500])
@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'f32'])
def test_config4_model_shape_vs_oracle(precision, sep):
    """BASELINE configs[3] model shape (reference tabular.py:109-155): one output (decoder N padded to 8 inside the library), BCE
    head (train.py:18,82-83), 60 features, bptt 1000, emsize 512, 6 layers -- logits, loss and EVERY parameter gradient against
    the f64 oracle on a draw of the BNN prior."""
    bench = _bench()
    w = bench.CONFIGS[4]
    model = bench.build_model(DEV, precision, w).train()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    x, y = bench.parity_inputs(w, torch.device(DEV))      # sep 500 = the bench record's parity_sep for this configuration
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    lo = pfn_oracle.forward(leaves, x, y, sep, w['nhead'], dtype=torch.float64)
    loss_o = torch.nn.functional.binary_cross_entropy_with_logits(lo.squeeze(-1), y[sep:])
    loss_o.backward()
    model.zero_grad()
    xd, yd = x.float().to(DEV), y.float().to(DEV)
    lg = model((xd, yd), single_eval_pos=sep)
    assert lg.shape == (w['bptt'] - sep, x.shape[1], 1)
    loss = model.criterion(lg.squeeze(-1), yd[sep:]).mean()
    loss.backward()
    tight = precision == 'f32'
    within(f'{precision} sep {sep} loss rel', abs(loss.item() - loss_o.item()) / abs(loss_o.item()), tol3(precision, 1e-5, 1e-3, 1.2e-5))
    within(f'{precision} sep {sep} logits rel l2', relerr(lg, lo), tol3(precision, 1e-4, 1.1e-2, 2.3e-3))
    p_err = (torch.sigmoid(lg).double().cpu() - torch.sigmoid(lo)).abs().max().item()      # posterior-predictive mean of the label
    within(f'{precision} sep {sep} probability max abs', p_err, tol3(precision, 1e-5, 1e-3))
    got = {k: p.grad for k, p in model.named_parameters()}
    tot_err = math.sqrt(sum(((got[k].double().cpu() - v.grad) ** 2).sum().item() for k, v in leaves.items()))
    tot = math.sqrt(sum((v.grad ** 2).sum().item() for v in leaves.values()))
    within(f'{precision} sep {sep} global gradient rel l2', tot_err / tot, tol3(precision, 2e-4, 1.2e-2, 1.6e-3))
    if tight:
        for k, v in leaves.items():
            if v.grad.norm() > 1e-7:
                assert relerr(got[k], v.grad) < 2e-3, (k, relerr(got[k], v.grad))


def test_config5_sampler_and_slice_at_bptt_4000():
    """BASELINE configs[4] at its real length: (a) the Matern-5/2 ARD sampler with per-dataset hyper-parameters at S = 4000 against
    the f64 restatement (reference priors/fast_gp_mix.py:28-47, 96-99); (b) a 2-layer slice of the emsize-1024 / head-dim-256 model
    at S = 4000 (forward, bar NLL, means) against the f64 oracle."""
    from transformerscandobayesianinference_amd.priors import fast_gp, fast_gp_mix
    g = torch.Generator().manual_seed(7)
    B, T, F = 2, 4000, 18
    x = torch.rand(B, T, F, generator=g)
    z = torch.randn(B, T, generator=g)
    ls, osc, nz = fast_gp_mix.sample_hyperparameters(B, F, None, 'cpu', generator=g)
    want = pfn_oracle.gp_sample(x, z, ls, osc, nz, 'matern')
    _, got, _, info = fast_gp.gp_sample(B, T, F, DEV, ls, osc, nz, fast_gp.KERNEL_MATERN52, x=x, z=z, check=False)
    assert int(info.abs().sum()) == 0
    assert relerr(got, want) < 2e-3, relerr(got, want)       # f32 factorisation of a 4000 x 4000 Gram matrix (unpinned: gpytorch absent)
    bench = _bench()
    w = dict(bench.CONFIGS[5], nlayers=2)
    model = bench.build_model(DEV, 'bf16', w)
    par, _ = bench.parity_check(model, w, torch.device(DEV), 'bf16')
    assert par['precision'] == 'f32'         # inference at head dim 256 runs the exact-f32 kernels too (round 4: the forward's V / O columns in two slices)
    assert par['nll_rel'] < 1e-5 and par['mean_max_over_y_range'] < 1e-6 and par['logits_rel_l2'] < 1e-4, par
    part = par['training_forward']
    assert part['nll_rel'] < 1e-3 and part['mean_max_over_y_range'] < 1e-3 and part['logits_rel_l2'] < 1e-2, part


def test_shadow_weights_follow_in_place_parameter_updates():
    """The operand-precision shadow of the weights must be rebuilt after ANY parameter update: load_state_dict into a model that
    has already run, a torch optimizer stepping model.parameters(), a manual p.copy_() (the flat buffer's version
    counter sees none of them)."""
    cfg = dict(T=48, B=2, F=3, E=64, H=2, nhid=128, L=2, nbars=16)
    a = random_model(cfg, 'bf16', seed=21).to(DEV).eval()
    b = random_model(cfg, 'bf16', seed=22)
    sd_b = {k: v.clone() for k, v in b.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand(cfg['T'], cfg['B'], cfg['F'], generator=g), torch.randn(cfg['T'], cfg['B'], generator=g)
    sep = 30
    with torch.no_grad():
        first = a((x.to(DEV), y.to(DEV)), single_eval_pos=sep)          # builds flat views + shadow of model a's weights
        a.load_state_dict({k: v.to(DEV) for k, v in sd_b.items()})
        after = a((x.to(DEV), y.to(DEV)), single_eval_pos=sep)
    want = pfn_oracle.forward(sd_b, x, y, sep, cfg['H'])
    assert relerr(after, want) < 1e-2 and relerr(first, want) > 0.1
    with torch.no_grad():
        for p in a.parameters():
            p.mul_(0.5)                                                  # what torch.optim / manual updates do
        halved = a((x.to(DEV), y.to(DEV)), single_eval_pos=sep)
    sd_h = {k: (v * 0.5 if not k.startswith('criterion.') else v) for k, v in sd_b.items()}
    assert relerr(halved, pfn_oracle.forward(sd_h, x, y, sep, cfg['H'])) < 1e-2


def test_failed_cholesky_is_repaired_with_jitter():
    """A Gram matrix that is not positive definite in f32 (duplicated points, noise at its 1e-9 floor) must not hand garbage to
    training: the failure flag is read and the failed datasets are redrawn from the same (x, z) with gpytorch's jitter ladder --
    directly (a host sync) and, inside a prefetching loader, before the batch is handed out."""
    import warnings
    from transformerscandobayesianinference_amd.priors import fast_gp
    g = torch.Generator().manual_seed(2)
    B, T, F = 3, 128, 5
    x = torch.rand(B, T, F, generator=g)
    x[1, 64:] = x[1, :64]                                   # dataset 1: every point twice -> singular Gram matrix
    z = torch.randn(B, T, generator=g)
    noise = torch.tensor([1e-2, 1e-9, 1e-2])                # ... and no noise to speak of on its diagonal
    _, y_raw, _, info = fast_gp.gp_sample(B, T, F, DEV, 0.6, 1.0, noise, x=x, z=z, check=False)
    assert info[1].item() != 0 and info[0].item() == 0 and info[2].item() == 0
    fast_gp.repair_log.clear()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        _, y, _, _ = fast_gp.gp_sample(B, T, F, DEV, 0.6, 1.0, noise, x=x, z=z)
    assert fast_gp.repair_log and fast_gp.repair_log[0][0] == 1 and any('Cholesky failed' in str(c.message) for c in caught)
    assert torch.isfinite(y).all() and torch.equal(y[0], y_raw[0]) and torch.equal(y[2], y_raw[2])
    jitter = fast_gp.repair_log[0][1]
    want = pfn_oracle.gp_sample(x[1:2], z[1:2], 0.6, 1.0, 1e-9 + jitter)
    assert (y[1].double().cpu() - want[0]).abs().max().item() < 0.05 * want.abs().max().item()   # cond ~ 1/jitter: loose on purpose
    # the loader path: the repair happens before the batch reaches the consumer
    calls = []
    orig = fast_gp.gp_sample

    def singular_gp_sample(batch_size, seq_len, num_features, device, *a, **kw):
        xs = torch.rand(batch_size, seq_len, num_features, device=device)
        xs[0, seq_len // 2:] = xs[0, :seq_len // 2]
        calls.append(1)
        return orig(batch_size, seq_len, num_features, device, *a, **{**kw, 'x': xs})

    fast_gp.repair_log.clear()
    fast_gp.gp_sample = singular_gp_sample
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            dl = fast_gp.DataLoader(num_steps=4, batch_size=2, seq_len=64, num_features=3, hyperparameters=(1e-9, 1., .6), device=DEV)
            batches = list(dl)
    finally:
        fast_gp.gp_sample = orig
    assert len(batches) == 4 and fast_gp.repair_log and all(torch.isfinite(b[0][1]).all() for b in batches)
    with pytest.raises(fast_gp.NotPSDError):
        xs = torch.rand(1, 64, 2)
        fast_gp.gp_sample(1, 64, 2, DEV, 0.6, -1.0, 1e-9, x=xs)          # negative outputscale: no jitter of the ladder helps


@pytest.mark.parametrize('ranks', [2, 8])
def test_bench_self_launches_the_ranks_on_one_device(ranks):
    """`python bench.py --gpus N` without a torchrun environment spawns the ranks itself; on a one-GPU box the PFN_DP_* hooks put
    every rank on device 0 over gloo (RCCL refuses two ranks per device) -- the line must say so, count every rank, carry the per-rank step times, the
    all-reduce figures (`allreduce_ms`: --full) and the fallback count, and stay inside the 6 KB contract (N = 8: what the driver's scaling run launches)."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(PFN_DP_BACKEND='gloo', PFN_DP_SINGLE_DEVICE='1')
    res = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', str(ranks), '--steps', '2', '--warmup', '1', '--batch', '4', '--full'],
                         capture_output=True, text=True, env=env, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    text = [l for l in res.stdout.splitlines() if l.startswith('{')][-1]
    assert len(text) <= 6 * 1024
    line = json.loads(text)
    assert line['n_gpus'] == ranks and line['ranks_seen'] == ranks and line['ranks_share_device'] is True and line['scaling'] == 'weak'
    assert line['config']['global_batch'] == 4 * ranks and line['config']['parallelism'] == f'dp{ranks}' and line['allreduce_ms'] > 0 and line['value'] > 0
    assert len(line['per_rank_ms_per_step']) == ranks and all(v > 0 for v in line['per_rank_ms_per_step'])
    assert line['allreduce_overlapped']['fallback_steps'] == 0 and line['allreduce_overlapped']['in_timed_steps'] is True      # every armed step overlapped its early collective
    assert line['allreduce_overlapped']['overlapped_bytes'] + line['allreduce_overlapped']['exposed_bytes'] == line['allreduce_bytes']


def test_train_cli_smoke(capsys):
    """`train.main` (reference train.py:154-287): the `gp` prior with the adaptive full-support bar loss through the HIP stack; the
    reference's default positional encoding (`sinus`, :168) puts `pos_encoder.pe` into the state dict."""
    from transformerscandobayesianinference_amd import train as train_mod
    torch.manual_seed(0); random.seed(0)
    loss, pos, model = train_mod.main(['gp', '--loss_function', 'adaptivefullsupportbarnll', '--num_buckets', '20', '--bptt', '24', '--epochs', '2',
                                       '--warmup_epochs', '1', '--emsize', '64', '--nlayers', '1', '--nhead', '2', '--steps_per_epoch', '2',
                                       '--batch_size', '8', '--permutation_invariant_max_eval_pos', '20',
                                       '--extra_prior_kwargs_dict', 'num_features=3', 'fuse_x_y=False'])
    assert math.isfinite(loss) and len(pos) == 24
    assert 'pos_encoder.pe' in model.state_dict()
    assert 'ARGS for `train`' in capsys.readouterr().out


def test_validate_and_run_test_vs_oracle():
    """The evaluation sweeps that define `val bar-NLL` (reference priors/fast_gp_mix.py:139-153 `validate`; notebook `run_test`,
    SetupForGPFittingExperiments.ipynb:176-224) against the oracle on IDENTICAL draws: per-position MSE of the posterior mean,
    per-position bar NLL, mean and mode errors (f32 mode 1e-4; bf16 1e-3 on the NLL, means 1e-3 of the target range)."""
    from transformerscandobayesianinference_amd import evaluation
    from transformerscandobayesianinference_amd.priors import fast_gp_mix
    cfg = dict(T=40, B=6, F=3, E=64, H=2, nhid=128, L=2, nbars=30)
    for precision in ('f32', 'bf16', 'fp16'):
        tight = precision == 'f32'
        model = random_model(cfg, precision, seed=31)
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        borders = sd['criterion.borders']
        model.to(DEV)
        # validate(): record the batch the loader draws, then restate the sweep with the oracle
        dl = fast_gp_mix.DataLoader(num_steps=1, batch_size=cfg['B'], seq_len=cfg['T'], num_features=cfg['F'], device=DEV,
                                    hyperparameters={'outputscale_concentration': 2.0, 'outputscale_rate': 40.0, 'noise_concentration': 1.1, 'noise_rate': 400.0})
        drawn = []
        orig = dl.gbm
        dl.gbm = lambda *a, **kw: drawn.append(orig(*a, **kw)) or drawn[-1]
        scores = dl.validate(model, step_size=7, start_pos=2)
        (x, y), target = drawn[0]
        x, y = x.cpu(), y.cpu()
        want = []
        for pos in range(2, cfg['T'], 7):
            lo = pfn_oracle.forward(sd, x, y, pos, cfg['H'])
            want.append(((pfn_oracle.bar_mean(lo, borders)[0] - y[pos].double()) ** 2).mean())
        want = torch.stack(want)
        assert scores.shape == want.shape
        within(f'{precision} validate scores rel l2', relerr(scores, want), tol3(precision, 1e-4, 5e-3, 1.6e-4))
        # run_test(): same idea through its `get_batch` argument
        drawn = []

        def recording_get_batch(**kw):
            g = torch.Generator().manual_seed(100 + len(drawn))
            xb, yb, _ = pfn_oracle.get_batch_fast_gp(kw['batch_size'], kw['seq_len'], kw['num_features'], kw['hyperparameters'], g)
            drawn.append((xb, yb))
            return xb.to(DEV), yb.to(DEV), yb.to(DEV)

        pos, mse, mode_mse, nll, conf = evaluation.run_test(model, DEV, step_size=9, start_pos=3, batch_size=8, sub_batch_size=4, seq_len=cfg['T'],
                                                            num_features=cfg['F'], hyperparameters={'noise': 1e-2, 'outputscale': 1., 'lengthscale': .6},
                                                            get_batch=recording_get_batch)
        it = iter(drawn)
        for j, p in enumerate(pos):
            nl, se, me = [], [], []
            for _ in range(2):
                xb, yb = next(it)
                lo = pfn_oracle.forward(sd, xb, yb, p, cfg['H'])
                nl.append(pfn_oracle.bar_nll(lo[0], yb[p].double(), borders.double()))
                se.append(((pfn_oracle.bar_mean(lo, borders)[0] - yb[p].double()) ** 2).mean())
                top = lo[0].argmax(-1)
                me.append((((borders[top] + borders[top + 1]).double() / 2 - yb[p].double()) ** 2).mean())
            within(f'{precision} run_test nll rel', abs(nll[j].item() - torch.cat(nl).mean().item()) / abs(torch.cat(nl).mean().item()), tol3(precision, 1e-4, 1e-3, 1.0e-4))
            within(f'{precision} run_test mse rel', abs(mse[j].item() - torch.stack(se).mean().item()) / torch.stack(se).mean().item(), tol3(precision, 1e-4, 5e-3, 1.0e-4))
            if tight:
                assert abs(mode_mse[j].item() - torch.stack(me).mean().item()) < 1e-4 * torch.stack(me).mean().item()


@pytest.mark.parametrize('precision', ['f32', 'bf16', 'fp16'])
def test_custom_decoder_module_vs_oracle(precision):
    """`decoder=` generators (reference transformer.py:23, decoders.py): the HIP stack hands the encoder's test rows to the PyTorch
    module and takes their gradient back; forward and every parameter gradient against the f64 oracle."""
    from transformerscandobayesianinference_amd import decoders
    cfg = dict(T=56, B=3, F=4, E=64, H=2, nhid=128, L=2, nbars=12)
    torch.manual_seed(41)
    borders = torch.sort(torch.randn(cfg['nbars'] + 1) * 1.5)[0]
    model = TransformerModel(encoders.Linear(cfg['F'], cfg['E']), cfg['nbars'], cfg['E'], cfg['H'], cfg['nhid'], cfg['L'], 0.0,
                             y_encoder=encoders.Linear(1, cfg['E']), decoder=decoders.FixedScaledDecoder, precision=precision, eval_precision=precision)
    assert isinstance(model.decoder, decoders.FixedScaledDecoder)
    model.criterion = bar_distribution.FullSupportBarDistribution(borders)
    with torch.no_grad():
        for layer in model.transformer_encoder.layers:
            for t in (layer.linear2.weight, layer.self_attn.out_proj.weight):
                t.normal_(0, 0.03)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(4)
    x, y = torch.rand(cfg['T'], cfg['B'], cfg['F'], generator=g), torch.randn(cfg['T'], cfg['B'], generator=g)
    sep = 37
    # oracle: encoder in f64, then the same decoder arithmetic (mapper(x) / T.sum())
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in sd.items() if not k.startswith('criterion.')}
    hidden = pfn_oracle.forward({k: v for k, v in leaves.items() if not k.startswith('decoder.')}, x, y, sep, cfg['H'], return_hidden=True)[sep:]
    h1 = torch.nn.functional.gelu(hidden @ leaves['decoder.mapper.0.weight'].t() + leaves['decoder.mapper.0.bias'])
    lo = (h1 @ leaves['decoder.mapper.2.weight'].t() + leaves['decoder.mapper.2.bias']) / leaves['decoder.T'].sum()
    loss_o = pfn_oracle.bar_nll(lo.reshape(-1, cfg['nbars']), y[sep:].reshape(-1).double(), borders.double()).mean()
    loss_o.backward()
    model.to(DEV).train()
    logits = model((x.to(DEV), y.to(DEV)), single_eval_pos=sep)
    assert logits.shape == (cfg['T'] - sep, cfg['B'], cfg['nbars'])
    loss = model.criterion(logits.reshape(-1, cfg['nbars']), y[sep:].to(DEV).flatten()).mean()
    loss.backward()
    tight = precision == 'f32'
    within(f'{precision} logits rel l2', relerr(logits, lo), tol3(precision, 1e-4, 1e-2, 3.2e-4))
    within(f'{precision} loss rel', abs(loss.item() - loss_o.item()) / abs(loss_o.item()), tol3(precision, 1e-4, 1e-3, 1.0e-4))
    got = {k: p.grad for k, p in model.named_parameters()}
    tot_err = math.sqrt(sum(((got[k].double().cpu() - v.grad) ** 2).sum().item() for k, v in leaves.items()))
    tot = math.sqrt(sum((v.grad ** 2).sum().item() for v in leaves.values()))
    within(f'{precision} global gradient rel l2', tot_err / tot, tol3(precision, 2e-4, 1.2e-2, 5.9e-4))
    # a custom decoder runs in PyTorch (AccumulateGrad's += on views of the shared flat buffer): such a model is NOT split over micro-batch
    # streams, a plain one is -- and the unsplit pass through MicroBatchStreams reproduces the gradients above
    from transformerscandobayesianinference_amd.streams import MicroBatchStreams
    micro = MicroBatchStreams(2)
    assert micro.groups(model, cfg['B'] * 2) == 1
    plain = random_model(dict(cfg, nbars=12), precision, seed=41).to(DEV)
    assert micro.groups(plain, cfg['B'] * 2) == 2
    ref_grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    model.zero_grad()
    micro.forward_backward(model, (x.to(DEV), y.to(DEV)), y.to(DEV), sep,
                           lambda out, tg: model.criterion(out.reshape(-1, cfg['nbars']), tg[sep:].reshape(-1)).view(out.shape[0], -1))
    for k, p in model.named_parameters():
        assert relerr(p.grad, ref_grads[k]) < 1e-6 or ref_grads[k].norm() < 1e-12, k
    # the optimizer's flat buffer covers the decoder module's parameters too
    opt = FusedClipAdam(model, lr=1e-3)
    before = model.decoder.mapper[0].weight.detach().clone()
    opt.step(zero_grad=True)
    assert not torch.equal(before, model.decoder.mapper[0].weight.detach())


@pytest.mark.parametrize('decoder', ['built-in', 'module'])
@pytest.mark.parametrize('L', [1, 3])
@pytest.mark.parametrize('precision', ['f32', 'bf16', 'fp16'])
def test_top_layer_on_the_test_rows_equals_every_layer_on_every_row(precision, L, decoder):
    """The reference returns output[single_eval_pos:] (transformer.py:91): the top encoder layer's train rows feed nothing, and the stack runs that
    layer on the test rows only (PFN_TUNE_TOP_LAYER_TEST_ROWS, include/pfn_hip.h).  Same logits and the same gradient of every parameter as the
    schedule that runs every layer on every row (the oracle comparisons of this file all run with the default, i.e. the shortened schedule)."""
    from transformerscandobayesianinference_amd import decoders
    cfg = dict(T=600, B=3, F=5, E=128, H=2, nhid=256, L=L, nbars=20)
    sep = 437                                                      # first query block the attention kernels touch: 256
    desc = None
    results = {}
    if True:
        for mode in (1, 0):
            if decoder == 'module':
                torch.manual_seed(7)
                borders = torch.sort(torch.randn(cfg['nbars'] + 1) * 1.5)[0]
                model = TransformerModel(encoders.Linear(cfg['F'], cfg['E']), cfg['nbars'], cfg['E'], cfg['H'], cfg['nhid'], cfg['L'], 0.0,
                                         y_encoder=encoders.Linear(1, cfg['E']), decoder=decoders.FixedScaledDecoder, precision=precision, eval_precision=precision)
                model.criterion = bar_distribution.FullSupportBarDistribution(borders)
                with torch.no_grad():
                    for layer in model.transformer_encoder.layers:
                        for t in (layer.linear2.weight, layer.self_attn.out_proj.weight):
                            t.normal_(0, 0.03)
            else:
                model = random_model(cfg, precision, seed=7)
            model.schedule = 0 if mode else _hip.SCHED_TOP_LAYER_ALL_ROWS      # pfn_model_desc.schedule: per model, the same bits in its forward and backward
            model = model.to(DEV).train()
            desc = model._make_desc()
            rows = _hip.lib().pfn_top_layer_rows(ctypes.byref(desc), cfg['B'], cfg['T'], sep, 0)
            assert rows == ((cfg['T'] - sep) * cfg['B'] if mode else cfg['T'] * cfg['B'])
            g = torch.Generator().manual_seed(9)
            x, y = torch.rand(cfg['T'], cfg['B'], cfg['F'], generator=g).to(DEV), torch.randn(cfg['T'], cfg['B'], generator=g).to(DEV)
            logits = model((x, y), single_eval_pos=sep)
            model.criterion(logits.reshape(-1, cfg['nbars']), y[sep:].flatten()).mean().backward()
            with torch.no_grad():
                model.eval()
                infer = model((x, y), single_eval_pos=sep)
            results[mode] = (logits.detach().clone(), infer.clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()})
    desc = _hip.ModelDesc(*desc.key()[:-1], 0)
    tight = precision == 'f32'
    # (bf16: the row-wise products are the same instructions on the same rows; what differs is the f32 decoder gradient entering the top LayerNorm's
    # backward unrounded, and the summation order of the weight gradients over fewer rows)
    within(f'{precision} top-layer schedules: logits rel l2', relerr(results[1][0], results[0][0]), tol3(precision, 1e-6, 1e-5, 1.0e-6))
    within(f'{precision} top-layer schedules: inference logits rel l2', relerr(results[1][1], results[0][1]), tol3(precision, 1e-6, 1e-5, 1.0e-6))
    for k, g0 in results[0][2].items():
        if g0.norm() < 1e-12:
            assert results[1][2][k].norm() < 1e-9, k
            continue
        within(f'{precision} top-layer schedules: gradient rel l2', relerr(results[1][2][k], g0), tol3(precision, 1e-5, 3.5e-3, 4.7e-4))
    # short train parts keep every row (nothing to gain) and dropout does too (its masks are indexed by the full-layout row)
    assert _hip.lib().pfn_top_layer_rows(ctypes.byref(desc), cfg['B'], cfg['T'], cfg['T'] // 4 - 1, 0) == cfg['T'] * cfg['B']
    assert _hip.lib().pfn_top_layer_rows(ctypes.byref(desc), cfg['B'], cfg['T'], cfg['T'], 0) == cfg['T'] * cfg['B']


def test_trained_checkpoint_parity():
    """Parity on a TRAINED model: tests/golden/trained_config1.pt is a configs[0]-shaped PFN (bptt 100,
    5 features, emsize 128, 2 layers, 100 bars) trained by this stack on the GP prior (tools/train_pfn.py --stage config1; its loss
    curve and its distance to the exact GP posterior are in profiles/r03_trained.json).  A trained PFN's posterior means track the
    targets, so errors relative to the means' OWN norm mean something here.  Inference outputs (eval mode, exact-f32 kernels) carry the
    north star's 1e-3 on the NLL and the means; the bf16 forward of the training path is bounded at what was measured."""
    path = os.path.join(GOLD, 'trained_config1.pt')
    sd, _ = torch.load(path)
    cfg = dict(T=100, B=8, F=5, E=128, H=4, nhid=256, L=2, nbars=100)
    borders = sd['criterion.borders']

    def build(precision, schedule):
        m = TransformerModel(encoders.Linear(cfg['F'], cfg['E']), cfg['nbars'], cfg['E'], cfg['H'], cfg['nhid'], cfg['L'], 0.0,
                             y_encoder=encoders.Linear(1, cfg['E']), precision=precision)           # product defaults: inference in f32
        m.criterion = bar_distribution.FullSupportBarDistribution(borders.clone())
        m.load_state_dict(sd)
        m.schedule = schedule
        return m.to(DEV)
    # (path, operand format of the training forward, train mode, schedule bits, bounds on NLL / means (own norm) / logits)
    # This checkpoint saw 9.6 M datasets: its attention is sharp (|q| up to 80, the keys of a dataset share a common component nine times their spread), and the
    # forward amplifies operand rounding -- f32 kernels land at 2e-5 (untrained models: 1e-6).  Rounds 1-5's bf16 training forward: 3-6e-2.  Round 6: the keys are
    # centred per dataset before they are rounded (same outputs in exact arithmetic: csrc/pfn_kernels.h launch_key_shift), and fp16 operands carry 3 more bits:
    # profiles/r06_operand_format_simulation.json predicted 2.6 - 6.2e-2 (bf16, centred) and 3.5 - 7.0e-3 (fp16, centred) on the means by eval position; the device
    # lands on them (bounds = 2 x measured).  Inference carries the north star's 1e-3.
    variants = [('inference outputs (f32 kernels)', 'bf16', False, 0, (1e-3, 1e-3, 2e-4)),
                ('bf16 training forward (keys not centred: the arithmetic of rounds 1-5, the default of bf16)', 'bf16', True, 0, (6e-2, 0.12, 0.13)),
                ('bf16 training forward, keys centred', 'bf16', True, _hip.SCHED_KEY_CENTERING, (6e-2, 0.13, 0.13)),           # measured 2.4e-2 / 6.2e-2 / 6.1e-2 (the maximum sits at sep 20: 80 % test rows, whose
                                                                                        # self keys are not what the train-row mean centres; at sep 81: 2.3e-2 / 2.6e-2 / 3.4e-2 emulated)
                ('fp16 training forward, keys not centred', 'fp16', True, _hip.SCHED_NO_KEY_CENTERING, (1.5e-2, 3e-2, 3e-2)),
                ('fp16 training forward (keys centred: the default of fp16)', 'fp16', True, 0, (5e-3, 1.4e-2, 1.5e-2))]      # measured 2.5e-3 / 7.0e-3 / 7.6e-3: 8 - 12 x below rounds 1-5's bf16 forward

    models = {}
    gen = torch.Generator().manual_seed(2024)
    x, y, _ = pfn_oracle.get_batch_fast_gp(cfg['B'], cfg['T'], cfg['F'], {'noise': 1e-4, 'outputscale': 1., 'lengthscale': .6}, gen)
    params = {k: v for k, v in sd.items() if not k.startswith('criterion.')}
    for sep in (81, 50, 20):
        lo = pfn_oracle.forward(params, x, y, sep, cfg['H'])
        nll_o = pfn_oracle.bar_nll(lo.reshape(-1, cfg['nbars']), y[sep:].reshape(-1), borders).mean().item()
        mean_o = pfn_oracle.bar_mean(lo, borders)
        assert mean_o.pow(2).mean().sqrt().item() > 0.3          # a trained model: its means are not the prior mean 0
        assert relerr(mean_o, y[sep:]) < 0.7                      # ... they track the targets
        for mode, precision, train_mode, schedule, (b_nll, b_mean, b_logits) in variants:
            model = models.setdefault((precision, schedule), build(precision, schedule))
            model.train(train_mode)
            with torch.no_grad():
                lg = model((x.to(DEV), y.to(DEV)), single_eval_pos=sep)
                nll = model.criterion(lg.reshape(-1, cfg['nbars']), y[sep:].to(DEV).flatten()).mean().item()
                mean = model.criterion.mean(lg)
            # (a trained model's NLL crosses zero as the train set grows, so the relative error is taken against max(|nll|, 0.5).)
            within(f'{mode}: nll rel', abs(nll - nll_o) / max(abs(nll_o), 0.5), b_nll)
            within(f'{mode}: means rel l2 (own norm)', relerr(mean, mean_o), b_mean)
            within(f'{mode}: logits rel l2', relerr(lg, lo), b_logits)


@pytest.mark.parametrize('emsize', [64, 256, 512])       # head dims 32, 128 (the benchmarked kernels) and 256
@pytest.mark.parametrize('precision', ['f32', 'bf16', 'fp16'])
def test_dropout_vs_oracle_with_the_same_masks(precision, emsize):
    """Training with dropout > 0 (reference train.py:22 default 0.2; torch TransformerEncoderLayer drops the attention probabilities,
    the out_proj output, the FFN activation and the linear2 output): the HIP stack's masks are counter-based functions of a per-pass
    seed (csrc/pfn_kernels.h dropout_keep), the oracle evaluates the SAME masks in f64, and logits, loss and every parameter
    gradient must agree -- forward masks in the flash kernel's register layout, backward masks regenerated in the key-block pass's
    (transposed) layout and in the query-block pass's self-key terms."""
    cfg = dict(T=200, B=2, F=4, E=emsize, H=2, nhid=128, L=2, nbars=20)
    pdrop, sep = 0.3, 150
    torch.manual_seed(51)
    borders = torch.sort(torch.randn(cfg['nbars'] + 1) * 1.5)[0]
    model = TransformerModel(encoders.Linear(cfg['F'], cfg['E']), cfg['nbars'], cfg['E'], cfg['H'], cfg['nhid'], cfg['L'], pdrop,
                             y_encoder=encoders.Linear(1, cfg['E']), precision=precision, eval_precision=precision)
    model.criterion = bar_distribution.FullSupportBarDistribution(borders)
    with torch.no_grad():
        for layer in model.transformer_encoder.layers:
            for t in (layer.linear2.weight, layer.self_attn.out_proj.weight):
                t.normal_(0, 0.05)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    g = torch.Generator().manual_seed(8)
    x = torch.rand(cfg['T'], cfg['B'], cfg['F'], generator=g)
    y = torch.randn(cfg['T'], cfg['B'], generator=g)
    model.zero_grad()
    logits = model((x.to(DEV), y.to(DEV)), single_eval_pos=sep)
    seed = model._last_dropout_seed
    loss = model.criterion(logits.reshape(-1, cfg['nbars']), y[sep:].to(DEV).flatten()).mean()
    loss.backward()
    loss_o, logits_o, grads_o = pfn_oracle.loss_and_grads(sd, x, y, y, sep, cfg['H'], borders, dropout=(pdrop, seed))
    _, logits_plain, _ = pfn_oracle.loss_and_grads(sd, x, y, y, sep, cfg['H'], borders)
    assert relerr(logits_o, logits_plain) > 0.05                       # the masks do something
    tight = precision == 'f32'
    within(f'{precision} logits rel l2', relerr(logits, logits_o), tol3(precision, 1e-4, 2e-2, 1.3e-3))
    within(f'{precision} loss rel', abs(loss.item() - loss_o.item()) / abs(loss_o.item()), tol3(precision, 1e-4, 5e-3, 1.0e-4))
    got = {k: p.grad for k, p in model.named_parameters()}
    tot_err = math.sqrt(sum(((got[k].double().cpu() - v) ** 2).sum().item() for k, v in grads_o.items()))
    tot = math.sqrt(sum((v ** 2).sum().item() for v in grads_o.values()))
    within(f'{precision} global gradient rel l2', tot_err / tot, tol3(precision, 2e-4, 2e-2, 1.2e-3))
    if tight:
        for k, v in grads_o.items():
            if v.norm() > 1e-7:
                assert relerr(got[k], v) < 2e-3, (k, relerr(got[k], v))
    # a second pass draws new masks; eval mode applies none
    logits2 = model((x.to(DEV), y.to(DEV)), single_eval_pos=sep)
    assert model._last_dropout_seed != seed and relerr(logits2, logits) > 0.05
    model.eval()
    with torch.no_grad():
        lg_eval = model((x.to(DEV), y.to(DEV)), single_eval_pos=sep)
    within(f'{precision} eval-mode logits rel l2 (no dropout)', relerr(lg_eval, logits_plain), tol3(precision, 1e-4, 2e-2, 1.3e-3))
    # the keep rate of a mask is 1 - p
    keep = pfn_oracle.dropout_keep_mask(pfn_oracle.dropout_site_seed(seed, 0, 1), range(400), range(64), pdrop)
    assert abs(keep.float().mean().item() - (1 - pdrop)) < 0.01


def test_emsize_1024_fused_layernorm_gemms_in_the_stack():
    """emsize 1024 with the LayerNorm-fused GEMMs on 64-row x 1024-column tiles switched ON (PFN_TUNE_FUSE_LN_WIDE; off by default because
    GEMM + LayerNorm kernels measure faster at that width): forward, loss and every gradient against the f64 oracle, and against the
    default path."""
    cfg = dict(T=160, B=2, F=18, E=1024, H=16, nhid=2048, L=2, nbars=100)
    lib = _hip.lib()
    outs = {}
    if True:
        for wide in (1, 0):
            model = random_model(cfg, 'bf16', seed=4)
            model.schedule = _hip.SCHED_FUSE_LN_WIDE if wide else 0
            sd = {k: v.clone() for k, v in model.state_dict().items()}
            model = model.to(DEV).train()
            gen = torch.Generator().manual_seed(6)
            x, y, _ = pfn_oracle.get_batch_fast_gp(cfg['B'], cfg['T'], cfg['F'], {'noise': 1e-4, 'outputscale': 1., 'lengthscale': .6}, gen)
            sep = 131
            model.zero_grad()
            logits = model((x.to(DEV), y.to(DEV)), single_eval_pos=sep)
            loss = model.criterion(logits.reshape(-1, cfg['nbars']), y[sep:].to(DEV).flatten()).mean()
            loss.backward()
            outs[wide] = (logits.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()})
    loss_o, logits_o, grads_o = pfn_oracle.loss_and_grads(sd, x, y, y, sep, cfg['H'], sd['criterion.borders'])
    for wide in (1, 0):
        logits, grads = outs[wide]
        within(f'fused-wide={wide} logits rel l2', relerr(logits, logits_o), 1e-2)
        tot_err = math.sqrt(sum(((grads[k].double().cpu() - g) ** 2).sum().item() for k, g in grads_o.items()))
        tot = math.sqrt(sum((g ** 2).sum().item() for g in grads_o.values()))
        within(f'fused-wide={wide} global gradient rel l2', tot_err / tot, 1.2e-2)
    assert relerr(outs[1][0], outs[0][0]) < 5e-3          # the two paths round differently, not more


def test_eval_mode_forward_then_backward_uses_the_training_kernels():
    """with the DEFAULT eval_precision='f32' on a bf16 model, an eval()-mode forward that is differentiated afterwards
    (fine-tuning under eval(), input gradients) must run the training-precision kernels -- its backward reads that workspace layout.
    eval() + backward == train() + backward at dropout 0 (the same kernels); under no_grad eval() still takes the exact-f32 inference kernels."""
    cfg = dict(T=96, B=3, F=4, E=64, H=2, nhid=128, L=2, nbars=20)
    model = random_model(cfg, 'bf16', seed=31)
    model.eval_precision = 'f32'                                # the constructor default (random_model pins it to the training precision)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV)
    g = torch.Generator().manual_seed(2)
    x, y = torch.rand(cfg['T'], cfg['B'], cfg['F'], generator=g).to(DEV), torch.randn(cfg['T'], cfg['B'], generator=g).to(DEV)
    sep = 70
    grads, outs = {}, {}
    for mode in ('train', 'eval'):
        getattr(model, mode)()
        model.flat_parameters()[1].zero_()
        out = model((x, y), single_eval_pos=sep)
        model.criterion(out.reshape(-1, cfg['nbars']), y[sep:].flatten()).mean().backward()
        grads[mode], outs[mode] = model.flat_parameters()[1].clone(), out.detach().clone()
    assert model._eval_desc is not None                          # a separate inference precision IS configured
    assert torch.isfinite(grads['eval']).all()
    assert torch.equal(outs['eval'], outs['train'])                # the same kernels on the same data
    assert relerr(grads['eval'], grads['train']) < 1e-5             # (the weight gradients are split-K sums of f32 atomics: equal up to summation order)
    _, _, grads_o = pfn_oracle.loss_and_grads(sd, x.cpu(), y.cpu(), y.cpu(), sep, cfg['H'], sd['criterion.borders'])
    tot_err = math.sqrt(sum(((p.grad.double().cpu() - grads_o[k]) ** 2).sum().item() for k, p in model.named_parameters()))
    within('eval-mode backward, global gradient rel l2', tot_err / math.sqrt(sum((v ** 2).sum().item() for v in grads_o.values())), 1.2e-2)
    with torch.no_grad():
        inf = model((x, y), single_eval_pos=sep)                 # inference pass: exact-f32 kernels
    want = pfn_oracle.forward(sd, x.cpu(), y.cpu(), sep, cfg['H'])
    assert relerr(inf, want) < 1e-4 < relerr(outs['eval'], want)


def test_trained_head_dim_256_inference_parity():
    """inference at head dim 256 (BASELINE configs[4]: emsize 1024, nhead 4) honours eval_precision='f32' -- the exact-f32
    attention forward exists at that head dim since round 4 (V / O columns in two slices, attention.hip) -- and the north star's 1e-3 on the bar NLL and
    on the posterior means (relative to their OWN norm) holds on TRAINED weights.  A 2-layer emsize-1024 / nhead-4 PFN is trained here by the bf16 stack
    on GP draws (a 67 MB checkpoint is not a fixture), then compared with the f64 oracle on a fixed-seed draw: inference outputs at 1e-3, the bf16
    training forward on the same weights recorded beside them (reference transformer.py:55-91, priors/fast_gp_mix.py:139-153 `validate`)."""
    from transformerscandobayesianinference_amd.priors import fast_gp
    cfg = dict(T=160, B=16, F=3, E=1024, H=4, nhid=2048, L=2, nbars=100)
    hyper = (1e-4, 1.0, 1.0)                                     # (noise, outputscale, lengthscale)
    torch.manual_seed(77)
    fast_gp._call_counter[0] = 0                                 # the sampler's Philox offset counts calls in this process: the draws below do not depend on the tests before
    borders = bar_distribution.get_bucket_limits(cfg['nbars'], ys=fast_gp.get_batch(400, 20, cfg['F'], device=DEV, hyperparameters=hyper)[1].cpu())
    # round 5: trained under the DETERMINISTIC schedule (PFN_SCHED_DETERMINISTIC) -- the trajectory, hence the weights and every number below, is reproducible
    model = TransformerModel(encoders.Linear(cfg['F'], cfg['E']), cfg['nbars'], cfg['E'], cfg['H'], cfg['nhid'], cfg['L'], 0.0,
                             y_encoder=encoders.Linear(1, cfg['E']), precision='bf16', deterministic=True)      # product defaults otherwise: bf16 training, f32 inference
    model.criterion = bar_distribution.FullSupportBarDistribution(borders)
    model = model.to(DEV).train()
    opt = FusedClipAdam(model, lr=1e-4)
    steps, warm = 2500, 200
    g = torch.Generator().manual_seed(5)
    first = last = None
    for it in range(steps):
        for grp in opt.param_groups:
            grp['lr'] = 2e-4 * min(1.0, (it + 1) / warm)
        sep = int(torch.randint(20, cfg['T'] - 10, (1,), generator=g))
        x, y, target = fast_gp.get_batch(cfg['B'], cfg['T'], cfg['F'], device=DEV, hyperparameters=hyper)
        out = model((x, y), single_eval_pos=sep)
        loss = model.criterion(out.reshape(-1, cfg['nbars']), target[sep:].reshape(-1)).mean()
        loss.backward()
        opt.step(zero_grad=True)
        if it < 20:
            first = loss.item() if first is None else 0.9 * first + 0.1 * loss.item()
        if it >= steps - 100:
            last = loss.item() if last is None else 0.9 * last + 0.1 * loss.item()
    assert model._eval_desc is not None and model._eval_desc.precision == _hip.PREC_F32      # eval_precision='f32' is honoured at head dim 256
    within('training moved the loss (last / first, smoothed; < 1 - margin)', last - first + 1.0, 0.9)        # at least 0.1 nats below the start
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    params = {k: v for k, v in sd.items() if not k.startswith('criterion.')}
    gen = torch.Generator().manual_seed(2025)
    x, y, _ = pfn_oracle.get_batch_fast_gp(4, cfg['T'], cfg['F'], {'noise': hyper[0], 'outputscale': hyper[1], 'lengthscale': hyper[2]}, gen)
    for sep in (130, 60):
        lo = pfn_oracle.forward(params, x, y, sep, cfg['H'])
        nll_o = pfn_oracle.bar_nll(lo.reshape(-1, cfg['nbars']), y[sep:].reshape(-1), sd['criterion.borders']).mean().item()
        mean_o = pfn_oracle.bar_mean(lo, sd['criterion.borders'])
        for mode, train_mode in (('inference outputs (f32 kernels, head dim 256)', False), ('bf16 training forward (head dim 256)', True)):
            model.train(train_mode)
            with torch.no_grad():
                lg = model((x.to(DEV), y.to(DEV)), single_eval_pos=sep)
                nll = model.criterion(lg.reshape(-1, cfg['nbars']), y[sep:].to(DEV).flatten()).mean().item()
                mean = model.criterion.mean(lg)
            tight = not train_mode
            # (round 5: the model is trained under the deterministic schedule, so these values repeat to the last digit -- two runs, gpurun call 3 of round 5:
            # inference 7.18e-7 / 1.10e-6 / 9.37e-7; the bf16 training forward on these weights -- 2500 optimizer steps, the loss 2.8 nats below its start --
            # 4.20e-4 / 1.13e-3 / 1.28e-3 in both.  Later in round 5 the GP sampler's arithmetic changed (fp16 two-term products: the draws differ in the last
            # bits), i.e. ANOTHER trajectory and other weights: inference 7.5e-7 / 6.7e-7 / 1.0e-6 -- the asserted tier does not care -- and the bf16 forward
            # 1.71e-3 / 6.96e-4 / 1.35e-3, again identical in two runs.  The bf16 error of a trained emsize-1024 model depends on WHICH weights training
            # arrived at (nll x 4, means x 0.6 between the two); bf16 bounds = 2 x the larger of the two trajectories' values)
            within(f'{mode}: nll rel', abs(nll - nll_o) / max(abs(nll_o), 0.5), 1e-3 if tight else 3.4e-3)
            within(f'{mode}: means rel l2 (own norm)', relerr(mean, mean_o), 1e-3 if tight else 2.3e-3)
            within(f'{mode}: logits rel l2', relerr(lg, lo), 2e-4 if tight else 2.7e-3)
        # round 6: the fp16 training forward on the SAME trained weights (the benchmarked operand format; head dim 256 kernels, keys centred): the north star's 1e-3
        # holds on the TIMED path's forward too, on a trained emsize-1024 model
        if sep == 130:
            m16 = TransformerModel(encoders.Linear(cfg['F'], cfg['E']), cfg['nbars'], cfg['E'], cfg['H'], cfg['nhid'], cfg['L'], 0.0,
                                   y_encoder=encoders.Linear(1, cfg['E']), precision='fp16')
            m16.criterion = bar_distribution.FullSupportBarDistribution(borders.clone())
            m16.load_state_dict(sd)
            m16 = m16.to(DEV).train()
        with torch.no_grad():
            lg = m16((x.to(DEV), y.to(DEV)), single_eval_pos=sep)
            nll = m16.criterion(lg.reshape(-1, cfg['nbars']), y[sep:].to(DEV).flatten()).mean().item()
            mean = m16.criterion.mean(lg)
        within('fp16 training forward (head dim 256): nll rel', abs(nll - nll_o) / max(abs(nll_o), 0.5), 4e-4)      # (2 x measured: 1.9e-4 / 8.0e-5 / 1.7e-4; bf16: 1.7e-3 / 7.0e-4 / 1.4e-3)
        within('fp16 training forward (head dim 256): means rel l2 (own norm)', relerr(mean, mean_o), 1.6e-4)
        within('fp16 training forward (head dim 256): logits rel l2', relerr(lg, lo), 3.4e-4)


@pytest.mark.parametrize('precision,aggregate_streams,aggregate_stacked', [('f32', 0, False), ('bf16', 0, False), ('fp16', 0, False), ('f32', 2, False), ('f32', 0, True), ('bf16', 0, True), ('fp16', 0, True)])
def test_training_loop_vs_reference_train_golden(precision, aggregate_streams, aggregate_stacked):
    """The training loop pinned to the reference's OWN `train.train` (train.py:58-110,134; utils.py:10-22):
    tests/golden/train_loop_small.pt = recorded batches + recorded eval positions + what the reference's loop made of them (4 epochs x 8
    batches, aggregate_k_gradients 2, per-epoch cosine schedule whose first epoch runs at lr 0; oracle/make_golden.py::train_loop_case).
    `train()` of this repo replays the stream through the HIP stack: exact-f32 mode reproduces every batch loss to 1e-4 and the whole
    parameter update to 1e-3; the bf16 product path follows the same curve (bounds = 2 x measured, tests/bounds.py)."""
    import replay
    from transformerscandobayesianinference_amd import train as train_mod, utils
    rec = torch.load(os.path.join(GOLD, 'train_loop_small.pt'))
    losses, lrs, total, final = replay.replay(train_mod.train, rec, bar_distribution.FullSupportBarDistribution, encoders, utils.get_cosine_schedule_with_warmup,
                                              gpu_device=DEV, precision=precision, micro_streams=1, aggregate_streams=aggregate_streams, aggregate_stacked=aggregate_stacked)
    # (aggregate_streams = 2: the two batches of every optimizer step run whole on alternating HIP streams -- streams.py forward_backward_on; aggregate_stacked:
    # the two batches stacked into ONE launch set, every dataset with its own eval position -- forward_backward_batches, train()'s choice for small batches
    # since round 5.  Both must reproduce the reference's sequential accumulation just the same)
    cfg = rec['config']
    assert lrs == pytest.approx(rec['batch_lr'], rel=1e-12, abs=0) and lrs[0] == 0.0
    tight = precision == 'f32'
    # (measured: f32 5.4e-7 / 2.4e-7 / 2.6e-4, bf16 7.5e-4 / 1.3e-4 / 4.2e-2 -- profiles/r04_parity_measured.json)
    within(f'{precision} batch losses, max rel', max(abs(a - b) / abs(b) for a, b in zip(losses, rec['batch_losses'])), tol3(precision, 1e-4, 2e-3, 2.6e-4))
    epoch = [sum(losses[e * cfg['steps_per_epoch']:(e + 1) * cfg['steps_per_epoch']]) / cfg['steps_per_epoch'] for e in range(cfg['epochs'])]
    within(f'{precision} epoch losses, max rel', max(abs(a - b) / abs(b) for a, b in zip(epoch, rec['epoch_losses'])), tol3(precision, 1e-4, 2e-3, 1.0e-4))
    within(f'{precision} returned total loss rel', abs(total - rec['returned_total_loss']) / abs(rec['returned_total_loss']), tol3(precision, 1e-4, 2e-3, 1.0e-4))
    within(f'{precision} parameter update over the run, rel l2', replay.update_error(final, rec), tol3(precision, 1e-3, 0.1, 6e-2))      # (fp16 measured 1.7-2.8e-2)


def _two_gpus():
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs (RCCL refuses two ranks on one device); the one-GPU box runs test_data_parallel_gradient_equals_global_batch over gloo')


def test_rccl_data_parallel_on_two_gpus(tmp_path):
    """SURVEY.md 8(e) over RCCL: the same two-rank check as test_data_parallel_gradient_equals_global_batch, on two DEVICES
    over the `nccl` backend -- the production collective path (dp.OverlappedGradientReducer: the upper layers' half of the flat gradient buffer
    all-reduced on a side stream behind the early weight-gradient launch, the rest behind the backward).  Skipped on a one-GPU box."""
    _two_gpus()
    import subprocess, sys
    script = tmp_path / 'dp_rccl_check.py'
    script.write_text(_DP_GPU_SCRIPT + "\nassert torch.distributed.get_backend() == 'nccl' and local == rank and torch.cuda.current_device() == rank\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith('PFN_DP_')}
    _PORT = _free_port()      # (a fixed port collided once in a full-suite run: a listener of an earlier test was still closing)
    env.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=_PORT, HSA_ENABLE_IPC_MODE_LEGACY='0')
    res = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
                          '--master-port', _PORT, str(script), root], capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert res.stdout.count(' ok ') == 2


def test_bench_on_two_gpus_over_rccl():
    """`python bench.py --gpus 2 --full` end to end (the driver's scaling run launches it without --full): rank 0's JSON line says the collectives ran on RCCL,
    both ranks were seen, the timed steps took the overlapped two-collective path, and carries the numbers that make an 8-GPU line diagnosable
    (allreduce_ms, exposed bytes, per-rank step times).  Skipped on a one-GPU box."""
    _two_gpus()
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith('PFN_DP_')}
    res = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '2', '--full'], capture_output=True, text=True,
                         env=env, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    line = json.loads([l for l in res.stdout.splitlines() if l.startswith('{')][-1])
    assert line['n_gpus'] == 2 and line['collective_backend'] == 'nccl' and line['ranks_seen'] == 2 and line['devices_visible'] >= 2
    assert line['allreduce_overlapped']['in_timed_steps'] and line['allreduce_overlapped']['fallback_steps'] == 0
    assert line['allreduce_ms'] > 0 and line['allreduce_overlapped']['exposed_bytes'] > 0
    assert len(line['per_rank_ms_per_step']) == 2 and max(line['per_rank_ms_per_step']) <= line['ms_per_step'] * 1.001
    assert line['config']['global_batch'] == 2 * line['config']['per_gpu_batch'] and line['scaling'] == 'weak'


def test_fast_gp_mix_get_model_samples_like_the_reference_call_sequence():
    """priors.fast_gp_mix.get_model(x, y, hyperparameters, sample=True) (reference :24-55) and the call sequence `get_batch` runs on it (:95-99):
    `model, likelihood = get_model(x, torch.Tensor(), hp); sample = likelihood(model(x)).sample()` -- one independent hyper-parameter draw per
    dataset of the batched x, the draw through the HIP sampler, checked against the f64 restatement with the SAME hyper-parameters and normals."""
    from transformerscandobayesianinference_amd.priors import fast_gp, fast_gp_mix
    torch.manual_seed(3)
    n, T, F = 6, 96, 4
    x = torch.rand(n, T, F, device=DEV)
    model, likelihood = fast_gp_mix.get_model(x, torch.Tensor(), {'nu': 1.5})
    assert model.lengthscale.shape == (n, F) and model.outputscale.shape == (n,) and model.noise.shape == (n,) and model.nu == 1.5
    assert (model.noise >= fast_gp_mix.MIN_INFERRED_NOISE_LEVEL).all() and likelihood.noise is model.noise
    y = likelihood(model(x)).sample()
    assert y.shape == (n, T) and torch.isfinite(y).all()
    # the same hyper-parameters and the same base normals through the oracle
    _, got, z, info = fast_gp.gp_sample(n, T, F, DEV, model.lengthscale, model.outputscale, model.noise, model.kernel, x=x, check=False)
    want = pfn_oracle.gp_sample(x.cpu(), z.cpu(), model.lengthscale.cpu(), model.outputscale.cpu(), model.noise.cpu(), 'matern32')
    assert int(info.abs().sum()) == 0 and relerr(got, want) < 1e-3
    with pytest.raises(NotImplementedError):
        fast_gp_mix.get_model(x, torch.Tensor(), {}, sample=False)


def test_bench_line_contract():
    """The driver parses the LAST stdout line of `python bench.py --gpus 1 --steps 20 --warmup 5`, here with every side measurement on (--full; round 4's 26 KB
    line lost its head in the driver's 8 KB tail): the line is one compact JSON object of at most 6 KB carrying every key of the contract with the right type, the metric / workload
    are BASELINE.json's, `roofline` and `cpu_baseline` carry their fields, one number each for configs[3], configs[4] and the batch sweep, and the timed
    window fits inside the command's own clock.  The full record goes to bench_detail.json."""
    import json, subprocess, sys, time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT') and not k.startswith('PFN_DP_')}
    t0 = time.time()
    res = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5', '--full'], capture_output=True, text=True, env=env, timeout=1200)
    wall = time.time() - t0
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1                                                   # stdout carries the JSON line only
    assert len(lines[0]) <= 6000 and len(res.stdout[-8192:].splitlines()[-1]) == len(lines[0])     # whole inside the driver's 8 KB tail
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(root, 'BASELINE.json')))
    assert d['metric'].split(' (')[0] in base['metric'] and d['unit'] == 'datasets/s' and d['value'] > 0
    assert d['n_gpus'] == 1 and d['steps'] == 20 and d['warmup'] == 5 and d['higher_is_better'] is True and d['scaling'] == 'weak' and d['vs_baseline'] is None
    assert abs(d['value'] - d['config']['global_batch'] * 1e3 / d['ms_per_step']) < 1e-4 * d['value']
    assert d['ms_per_step'] * d['steps'] * 1e-3 < d['seconds_total'] <= wall
    assert d['dtype'] == 'fp16' and d['data'] == 'synthetic' and 'bptt=2000' in d['config']['workload'] and 'num_features=18' in d['config']['workload'] and 'model' not in d['config']
    r = d['roofline']
    assert r['bound'] in ('hbm', 'mfma') and r['unit'] in ('GB/s', 'TFLOP/s') and r['peak'] == 2500.0 and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-4
    assert r['frac_is'] == 'in-step' and r['avg_launch_us'] > r['isolated_avg_launch_us'] * 0.9 and r['frac'] <= r['isolated_frac'] * 1.1
    assert r['traffic'] is None or r['traffic'] > 0
    assert 0 < d['step_roofline']['frac'] < 1
    c = d['cpu_baseline']
    assert c['value'] > 0 and c['unit'] == 'datasets/s' and c['cores'] >= 1 and c['kind'] in ('port', 'reference') and c['sample']
    assert d['parity_inference']['precision'] == 'f32' and d['parity_inference']['passed']
    # round 6: the TIMED path (fp16 operands, train mode) holds the north star's 1e-3 on the NLL AND on the posterior means relative to their own norm;
    # the bf16 figures of the same configuration ride along
    tp = d['parity_timed_path']
    assert tp['precision'] == 'fp16' and tp['nll_rel'] < 1e-3 and tp['mean_rel_l2'] < 1e-3 and tp['mean_within_1e3_of_own_norm'] is True
    assert d['also_bf16']['value'] > 0 and d['also_bf16']['nll_rel'] < 1e-3 and abs(d['also_bf16']['value'] / d['value'] - 1) < 0.05
    assert d['value'] / c['value'] > 100                                      # (a reported baseline, not the target: just a sanity bound on the two legs)
    assert set(d['other_configs']) == {'configs[3]', 'configs[4]'} and all(e['value'] > 0 for e in d['other_configs'].values())
    assert len(d['batch_sweep']) >= 4 and all(e['value'] > 0 for e in d['batch_sweep'])
    detail = json.load(open(os.path.join(root, d['detail'])))
    assert detail['value'] == pytest.approx(d['value'], rel=1e-4) and 'kernels' in detail and 'legs' in detail['cpu_baseline']


def test_bench_plain_run_and_dumped_outputs(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` measures the headline only: one line with the contract keys, `steps` = K, `ms_per_step` = the
    timed window / K, and none of the side measurements of --full.  --dump-outputs writes what the last timed step computed (the losses of its batch,
    the updated parameters, the gradient norm) as float32 / float64 .npy within 64 MB, and two runs of the same arguments draw the same inputs: under
    the bit-reproducible schedule (PFN_BENCH_DETERMINISTIC=1) they write the same arrays."""
    import json, subprocess, sys, time
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT') and not k.startswith('PFN_DP_')}
    env['PFN_BENCH_DETERMINISTIC'] = '1'
    runs = []
    for i in range(2):
        out = tmp_path / f'run{i}'
        t0 = time.time()
        res = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', str(out)],
                             capture_output=True, text=True, env=env, timeout=600)
        wall = time.time() - t0
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        lines = [l for l in res.stdout.splitlines() if l.strip()]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 1 and d['unit'] == 'datasets/s' and d['higher_is_better'] is True and d['dtype'] == 'fp16'
        assert abs(d['value'] - d['config']['global_batch'] * 1e3 / d['ms_per_step']) < 1e-4 * d['value']
        assert d['ms_per_step'] * d['steps'] * 1e-3 < d['seconds_total'] <= wall
        assert not set(d) & {'roofline', 'cpu_baseline', 'parity_inference', 'parity_timed_path', 'val_bar_nll', 'also_bf16', 'other_configs', 'batch_sweep'}
        files = {p.stem: np.load(p) for p in out.glob('*.npy')}
        assert set(files) == {'loss', 'parameters', 'grad_norm'}
        assert sum(p.stat().st_size for p in out.glob('*.npy')) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) and a.size and np.isfinite(a).all() for a in files.values())
        assert files['loss'].shape[1] == d['config']['per_gpu_batch'] and files['grad_norm'][0] > 0
        assert abs(float(files['loss'].mean()) - d['config']['final_loss']) < 1e-4 * abs(d['config']['final_loss'])
        runs.append((d, files))
    (d0, a), (d1, b) = runs
    assert d0['config']['mean_sep'] == d1['config']['mean_sep']
    for k in a:
        np.testing.assert_allclose(b[k], a[k], rtol=1e-5, atol=1e-6, err_msg=k)


_DP_TRAIN_SCRIPT = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))
import replay
from transformerscandobayesianinference_amd import dp, bar_distribution, encoders, utils, train as train_mod
rank, world, local = dp.init_from_env()                 # PFN_DP_BACKEND=gloo, PFN_DP_SINGLE_DEVICE=1: both ranks on cuda:0 (or nccl on two devices)
torch.cuda.set_device(local)
rec = torch.load(os.path.join(sys.argv[1], 'tests', 'golden', 'train_loop_small.pt'))
cfg = dict(rec['config'], B=rec['config']['B'] * world)        # train() takes the GLOBAL batch size and hands every rank batch_size / world
nb = len(rec['batches'])
shard = lambda i, r: rec['batches'][(i + 7 * r) % nb]           # rank r's datasets of global batch i (recorded batches, shifted per rank)
mine = dict(rec, config=cfg, batches=[shard(i, rank) for i in range(nb)])
whole = dict(rec, config=cfg, batches=[tuple(torch.cat([shard(i, r)[k] for r in range(world)], 1) for k in (0, 1)) for i in range(nb)])
seen = dict(armed=0, overlapped=0, fallbacks=0)
_finish = dp.OverlappedGradientReducer.finish
def finish(self):
    armed = self._armed
    out = _finish(self)
    seen['armed'] += int(armed); seen['overlapped'] += int(self.overlapped_last_step); seen['fallbacks'] = self.fallbacks
    return out
dp.OverlappedGradientReducer.finish = finish
run = lambda r, **kw: replay.replay(train_mod.train, r, bar_distribution.FullSupportBarDistribution, encoders, utils.get_cosine_schedule_with_warmup,
                                    gpu_device=f'cuda:{local}', precision='f32', micro_streams=1, **kw)
# data-parallel: batch_size is the GLOBAL batch (train() hands every rank batch_size / world); the two batches of an optimizer step run whole on
# alternating streams, the last one armed -- the schedule train() picks by itself for small batches
_, _, total_dp, final_dp = run(mine, aggregate_streams=2)
steps = cfg['epochs'] * cfg['steps_per_epoch'] // cfg['aggregate_k_gradients']
assert seen['armed'] == steps and seen['overlapped'] == steps and seen['fallbacks'] == 0, seen
# ... and with the two batches of a step STACKED into one launch set (per-dataset eval positions; the reducer is armed for the launch sets of the step)
seen.update(armed=0, overlapped=0)
_, _, total_st, final_st = run(mine, aggregate_stacked=True)
assert seen['armed'] == steps and seen['overlapped'] == steps and seen['fallbacks'] == 0, seen
# ... against this process alone on the whole batches (no process group: world 1)
torch.distributed.barrier()
torch.distributed.destroy_process_group()
_, _, total_1, final_1 = run(whole, aggregate_streams=2)
err = replay.update_error(final_dp, dict(rec, final_state_dict=final_1))
err_st = replay.update_error(final_st, dict(rec, final_state_dict=final_1))
assert err < 1e-3 and err_st < 1e-3, (err, err_st)                # the whole parameter update over 16 optimizer steps (f32 kernels; summation order + Adam's normalisation of near-zero gradients)
assert abs(total_dp - total_1) < 1e-5 * abs(total_1) and abs(total_st - total_1) < 1e-5 * abs(total_1), (total_dp, total_st, total_1)     # the returned loss is the mean over ranks
print('rank', rank, 'ok', err, err_st)
"""


def test_data_parallel_train_with_alternating_streams_equals_single_process(tmp_path):
    """VERDICT round 4 (missing 2 / next 8): `train(aggregate_k_gradients=2, aggregate_streams=2)` under data parallelism -- the batches of an optimizer
    step whole on alternating streams, the LAST one armed so the upper layers' half of the all-reduce starts behind its early weight-gradient
    launch and additionally waits for the batch still running on the other stream (dp.OverlappedGradientReducer.arm(wait_for=...)).  Two ranks
    replay their halves of the reference-recorded batches (tests/golden/train_loop_small.pt) through train(); the final weights equal the
    single-process run on the whole batches to 1e-3 of the update, every optimizer step took the overlapped path.  One-GPU box: gloo on cuda:0."""
    import subprocess, sys
    script = tmp_path / 'dp_train_check.py'
    script.write_text(_DP_TRAIN_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    two = torch.cuda.device_count() >= 2
    env = {k: v for k, v in os.environ.items() if not k.startswith('PFN_DP_')}
    _PORT = _free_port()      # (a fixed port collided once in a full-suite run: a listener of an earlier test was still closing)
    env.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=_PORT, HSA_ENABLE_IPC_MODE_LEGACY='0')
    if not two:
        env.update(PFN_DP_BACKEND='gloo', PFN_DP_SINGLE_DEVICE='1')
    res = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
                          '--master-port', _PORT, str(script), root], capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert res.stdout.count(' ok ') == 2


def test_explicit_src_mask_of_the_eval_position_is_accepted():
    """reference transformer.py:60-65: an explicit `src_mask` replaces the mask the model would build.  The kernels implement exactly
    generate_D_q_matrix(T, T - single_eval_pos) from the integer, so that mask -- float 0/-inf (what the reference builds) or torch's boolean form -- is accepted
    and gives the same logits bit for bit; any other mask raises instead of being silently ignored (missing 6)."""
    rec = torch.load(os.path.join(GOLD, 'model_small_h32.pt'))
    cfg = rec['config']
    model = build_model(cfg, rec['state_dict'], 'f32').eval()
    x, y = rec['x'].to(DEV), rec['y'].to(DEV)
    T = x.shape[0]
    sep = sorted(rec['per_sep'])[len(rec['per_sep']) // 2]
    with torch.no_grad():
        base = model((x, y), single_eval_pos=sep)
        mask = TransformerModel.generate_D_q_matrix(T, T - sep)
        assert torch.equal(model((x, y), src_mask=mask.to(DEV), single_eval_pos=sep), base)
        assert torch.equal(model((x, y), src_mask=(mask != 0), single_eval_pos=sep), base)         # boolean form: True = masked
        within('f32 logits with the explicit mask vs the reference golden', relerr(base, rec['per_sep'][sep]['logits']), 1e-4)
        with pytest.raises(NotImplementedError):
            model((x, y), src_mask=TransformerModel.generate_D_q_matrix(T, T - sep - 1).to(DEV), single_eval_pos=sep)
        with pytest.raises(NotImplementedError):
            model((x, y), src_mask=TransformerModel.generate_square_subsequent_mask(T).to(DEV), single_eval_pos=sep)
        with pytest.raises(ValueError):
            model((x, y), src_mask=mask[:-1].to(DEV), single_eval_pos=sep)


@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'f32'])
def test_deterministic_schedule_is_bit_reproducible(precision):
    """VERDICT round 4 (missing 4 / next 6a): the reference's CPU loop is deterministic (train.py:58-110); the default HIP schedule sums weight-gradient token splits,
    LayerNorm / bias column sums and two micro-batch streams with f32 atomics, so two runs of one seed differ in the last bits.  `deterministic=True`
    (PFN_SCHED_DETERMINISTIC) gives every gradient element one writer per launch and a fixed summation order: the reference-recorded training loop
    (tests/golden/train_loop_small.pt: 32 batches, 16 optimizer steps) replayed twice ends in BIT-IDENTICAL weights and batch losses, and still
    follows the reference's own loop within the bounds of the default schedule."""
    import replay
    from transformerscandobayesianinference_amd import train as train_mod, utils
    rec = torch.load(os.path.join(GOLD, 'train_loop_small.pt'))
    run = lambda: replay.replay(train_mod.train, rec, bar_distribution.FullSupportBarDistribution, encoders, utils.get_cosine_schedule_with_warmup,
                                gpu_device=DEV, precision=precision, deterministic=True)
    losses_a, _, total_a, final_a = run()
    losses_b, _, total_b, final_b = run()
    assert losses_a == losses_b and total_a == total_b
    for k in final_a:
        assert torch.equal(final_a[k], final_b[k]), k
    tight = precision == 'f32'
    within(f'{precision} deterministic schedule: batch losses, max rel', max(abs(a - b) / abs(b) for a, b in zip(losses_a, rec['batch_losses'])), tol3(precision, 1e-4, 2e-3, 1.4e-4))
    within(f'{precision} deterministic schedule: parameter update over the run, rel l2', replay.update_error(final_a, rec), tol3(precision, 1e-3, 0.1, 4e-2))      # (fp16 measured 1.8e-2)


@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'f32'])
def test_deterministic_schedule_gradients_at_a_benchmark_like_shape(precision):
    """The deterministic schedule at a shape that takes the product kernels (emsize 512, 256-wide tiles, grouped weight gradients, the top layer on the test
    rows, the GEMM form of the embedding gradient): two backward passes of the same inputs give bit-identical gradient buffers, equal to the default
    schedule's gradient within its own rounding."""
    cfg = dict(T=520, B=4, F=18, E=512, H=4, nhid=1024, L=2, nbars=100)
    sep = 401
    torch.manual_seed(77)
    borders = torch.sort(torch.randn(cfg['nbars'] + 1) * 1.5)[0]
    def build(det):
        torch.manual_seed(5)
        m = TransformerModel(encoders.Linear(cfg['F'], cfg['E']), cfg['nbars'], cfg['E'], cfg['H'], cfg['nhid'], cfg['L'], 0.0,
                             y_encoder=encoders.Linear(1, cfg['E']), precision=precision, deterministic=det)
        m.criterion = bar_distribution.FullSupportBarDistribution(borders.clone())
        with torch.no_grad():
            for layer in m.transformer_encoder.layers:
                layer.linear2.weight.normal_(0, 0.05); layer.self_attn.out_proj.weight.normal_(0, 0.05)
        return m.to(DEV).train()
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand(cfg['T'], cfg['B'], cfg['F'], generator=g).to(DEV), torch.randn(cfg['T'], cfg['B'], generator=g).to(DEV)
    def grad(m):
        m.flat_parameters()[1].zero_()
        out = m((x, y), single_eval_pos=sep)
        m.criterion(out.reshape(-1, cfg['nbars']), y[sep:].reshape(-1)).mean().backward()
        return m.flat_parameters()[1].clone()
    md = build(True)
    assert md.deterministic and md._make_desc().schedule & _hip.SCHED_DETERMINISTIC
    g1, g2 = grad(md), grad(md)
    assert torch.equal(g1, g2)
    g0 = grad(build(False))
    within(f'{precision} deterministic vs default schedule: gradient rel l2', relerr(g1, g0), tol3(precision, 1e-5, 5e-3, 2.5e-4))


@pytest.mark.parametrize('E,H', [(256, 4), (512, 4), (1024, 4)], ids=['head-dim-64', 'head-dim-128', 'head-dim-256'])
def test_delta_from_the_dctx_gemm_equals_the_delta_kernel(E, H):
    """Round 5: on the full-sequence layers of the bf16 stack the attention backward's delta = rowsum(dO . O) is taken in the epilogue of the GEMM that produces
    dO (EPI_ROWDOT: f32 atomics of one / two / four 64-column waves per head at head dim 64 / 128 / 256) instead of by attn_delta_kernel (PFN_TUNE_FUSE_DELTA).
    The two forms must give the same gradient: the 256 x 256 LDS-DMA kernel is forced (tuning key 0 = 2) so that the fused form runs at a test-sized shape, the
    delta kernel form of the same launch set is the yardstick (itself held to the oracle by the stack-backward parity tests)."""
    cfg = dict(T=520, B=3, F=7, nhid=512, L=3, nbars=50)
    sep = 380
    torch.manual_seed(9)
    borders = torch.sort(torch.randn(cfg['nbars'] + 1) * 1.5)[0]
    m = TransformerModel(encoders.Linear(cfg['F'], E), cfg['nbars'], E, H, cfg['nhid'], cfg['L'], 0.0, y_encoder=encoders.Linear(1, E), precision='bf16')
    m.criterion = bar_distribution.FullSupportBarDistribution(borders)
    with torch.no_grad():
        for layer in m.transformer_encoder.layers:
            layer.linear2.weight.normal_(0, 0.05); layer.self_attn.out_proj.weight.normal_(0, 0.05)
    m = m.to(DEV).train()
    g = torch.Generator().manual_seed(4)
    x, y = torch.rand(cfg['T'], cfg['B'], cfg['F'], generator=g).to(DEV), torch.randn(cfg['T'], cfg['B'], generator=g).to(DEV)
    def grad():
        m.flat_parameters()[1].zero_()
        out = m((x, y), single_eval_pos=sep)
        m.criterion(out.reshape(-1, cfg['nbars']), y[sep:].reshape(-1)).mean().backward()
        return m.flat_parameters()[1].clone()
    lib = _hip.lib()
    _hip.check(lib.pfn_set_tuning(0, 2), 'pfn_set_tuning')
    try:
        _hip.check(lib.pfn_set_tuning(9, 0), 'pfn_set_tuning')
        kernel_a, kernel_b = grad(), grad()
        _hip.check(lib.pfn_set_tuning(9, 1), 'pfn_set_tuning')
        fused = grad()
    finally:
        lib.pfn_set_tuning(9, 1); lib.pfn_set_tuning(0, 0)
    assert fused.abs().max().item() > 0 and torch.isfinite(fused).all()
    noise = relerr(kernel_a, kernel_b)             # two runs of ONE form differ by the order of the weight gradients' f32 atomics
    within(f'fused delta vs delta kernel, head dim {E // H}: gradient rel l2', relerr(fused, kernel_a), max(10 * noise, 1e-4))


@pytest.mark.parametrize('seps', [[257, 0, 300, 131, 299], [257, 290, 80, 131, 299]], ids=['every-row-top-layer', 'test-row-top-layer'])
@pytest.mark.parametrize('precision', ['f32', 'bf16', 'fp16'])
def test_forward_batches_equals_separate_forwards(precision, seps):
    """Round 5: `model.forward_batches` runs several micro-batches -- each with its OWN single_eval_pos, as the reference's accumulation loop
    draws them (train.py:66-69, 92-97) -- as ONE launch set (pfn_stack_forward_ragged: per-dataset eval positions in the embedding, the three attention kernels
    and the test-row gather / scatter).  It must return exactly the logits of the separate `model((x, y), single_eval_pos=sep)` calls, and the backward of the
    summed per-batch mean losses must leave the gradient the sequential accumulation leaves."""
    cfg = dict(T=300, F=5, E=128, H=2, nhid=256, L=3, nbars=40)
    torch.manual_seed(21)
    borders = torch.sort(torch.randn(cfg['nbars'] + 1) * 1.5)[0]
    model = TransformerModel(encoders.Linear(cfg['F'], cfg['E']), cfg['nbars'], cfg['E'], cfg['H'], cfg['nhid'], cfg['L'], 0.0,
                             y_encoder=encoders.Linear(1, cfg['E']), precision=precision, eval_precision=precision)
    model.criterion = bar_distribution.FullSupportBarDistribution(borders)
    with torch.no_grad():
        for layer in model.transformer_encoder.layers:
            layer.linear2.weight.normal_(0, 0.05); layer.self_attn.out_proj.weight.normal_(0, 0.05)
    model = model.to(DEV).train()
    g = torch.Generator().manual_seed(4)
    widths = [4, 1, 3, 4, 2]          # first id: incl. no train rows at all, no test rows at all, one test row (the top layer then runs on every row);
                                      # second id: every position >= T / 4, so the top layer runs on the (ragged) test rows only
    batches = [(torch.rand(cfg['T'], w, cfg['F'], generator=g).to(DEV), torch.randn(cfg['T'], w, generator=g).to(DEV)) for w in widths]
    loss_of = lambda out, y, sep: model.criterion(out.reshape(-1, cfg['nbars']), y[sep:].reshape(-1)).mean() if sep < cfg['T'] else out.sum() * 0
    # sequential accumulation, as the reference does it
    _, grad = model.flat_parameters()
    grad.zero_()
    want = []
    for (x, y), sep in zip(batches, seps):
        out = model((x, y), single_eval_pos=sep)
        want.append(out.detach().clone())
        if sep < cfg['T']:
            loss_of(out, y, sep).backward()
    g_seq = grad.clone()
    # one launch set
    grad.zero_()
    outs = model.forward_batches(batches, seps)
    for got, ref, w, sep in zip(outs, want, widths, seps):
        assert got.shape == ref.shape == (cfg['T'] - sep, w, cfg['nbars'])
        assert torch.equal(got, ref), (sep, relerr(got, ref) if ref.numel() else 0)
    sum(loss_of(o, y, sep) for o, (_, y), sep in zip(outs, batches, seps) if sep < cfg['T']).backward()
    within(f'{precision} stacked vs sequential accumulation: gradient rel l2', relerr(grad, g_seq), tol3(precision, 1e-5, 5e-3, 5.3e-4))
    # and the inference pass (eval mode, no_grad) takes the same route
    model.eval()
    with torch.no_grad():
        outs_e = model.forward_batches(batches, seps)
        for got, (x, y), sep in zip(outs_e, batches, seps):
            assert torch.equal(got, model((x, y), single_eval_pos=sep))



@pytest.mark.parametrize('E,H', [(128, 4), (256, 4), (512, 4)], ids=['head-dim-32', 'head-dim-64', 'head-dim-128'])
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_q_projection_inside_the_attention_kernel_equals_the_gemm_projection(precision, E, H):
    """PFN_SCHED_FUSE_Q_PROJECTION (north_star: "QKV projection + scaled-dot-product attention + softmax ... as one fused kernel"; the half that can exist -- K and V are
    shared by every query block of a head and stay a GEMM): the attention forward forms its queries' head slice x W_q[h]^T + b_q[h] on the matrix cores in its prologue.
    Same operands in the same contraction order as the GEMM: the forward must agree to the last bit -- uniform and ragged batches, the top layer on the test rows or on
    every row -- and so must the gradients up to the atomics' summation order."""
    cfg = dict(T=600, B=3, F=4, E=E, H=H, nhid=2 * E, L=2, nbars=20)
    g = torch.Generator().manual_seed(17)
    x, y = torch.rand(cfg['T'], cfg['B'], cfg['F'], generator=g).to(DEV), torch.randn(cfg['T'], cfg['B'], generator=g).to(DEV)
    out = {}
    for fused in (False, True):
        model = random_model(cfg, precision, seed=11)
        model.schedule = _hip.SCHED_FUSE_Q_PROJECTION if fused else 0
        model = model.to(DEV).train()
        res = []
        for sep in (520, 100):                                   # the top layer on the test rows / on every row (sep < T / 4)
            model.zero_grad()
            lg = model((x, y), single_eval_pos=sep)
            model.criterion(lg.reshape(-1, cfg['nbars']), y[sep:].flatten()).mean().backward()
            res.append((lg.detach().clone(), model.flat_parameters()[1].clone()))
        with torch.no_grad():
            rag = model.forward_batches([(x[:, :2], y[:, :2]), (x[:, 2:], y[:, 2:])], [517, 300])
        out[fused] = (res, [r.clone() for r in rag])
    for (lg0, g0), (lg1, g1) in zip(out[False][0], out[True][0]):
        assert torch.equal(lg1, lg0), relerr(lg1, lg0)
        within(f'{precision} fused vs GEMM Q projection: gradient rel l2', relerr(g1, g0), 1e-5)
    for r0, r1 in zip(out[False][1], out[True][1]):
        assert torch.equal(r1, r0)
