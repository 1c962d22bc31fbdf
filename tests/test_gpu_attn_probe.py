"""hipops.attention_fwd / attention_bwd on the planted-key inputs of tests/attn_probe_cases.py: every round of a case, ctx, lse, dQ, dK and dV per (dataset, head)
against the f64 reference, inside the bound that the reference's own operand-rounded emulation sets (3 x max(e, u); f32: 4 x max(e, 2^-23)).
tests/test_host_attn_probe.py shows on the CPU that a lost or added key, tile, self key, head or dataset exceeds these bounds by >= 8 x on one of the tensors.

A bound that fails here is a finding: either the emulation lacks a rounding site of attention.hip (add it to oracle.pfn_oracle.ROUNDING_SITES with the line that
proves it) or a kernel is wrong (fix it; the failing (case, round, tensor, row) is its regression test).  The rule is not widened and no case is dropped.

lse is f32 in every format: |lse - ref| / max |score| < 4 x max(e_f32, 2^-23), e_f32 the same figure of the graph run in f32; the kernels' v_exp_f32 / v_log_f32 and
log2-domain scaling need no more (measured <= 0.20 of it).

Measured on an MI355X (profiles/attn_probe_parity_measured.json, value / bound, the largest over cases and rounds): bf16 ctx 0.33, dQ 0.71, dK 0.80, dV 0.70;
fp16 0.33, 0.69, 0.67, 0.67; f32 0.39, 0.38, 0.40, 0.42; lse 0.20.  The first f32 run stood at 1 - 20 x (dK at sep = 1: 350 x): the dense f32 graph lacked the
roundings of the row statistics, attn_probe_cases._FlashF32.  Slowest test 4.0 s (S520-sep512, 96 rounds).

The regression test of a kernel fix: S130-sep0.  Without train rows every query sees its own key alone and dQ, dK are identically zero in the reference; the
general kernels returned 0.002 (bf16), 0.015 (fp16), 0.125 (f32) x the bound there, not 0 (round self 0, every dataset and head): dS = P (dP - delta) with
delta = sum(dO o) from the stored output (attention.hip :743, :1392) is a difference of two f32 sums of the same products in different orders, ~2^-24 |dP|.
launch_attn_bwd now takes a batch without train rows (one eval position, no dropout) through attn_bwd_self_only_kernel: dV = dO, dQ = dK = 0."""
import pytest
import torch

import attn_probe_cases as P
import bounds
from transformerscandobayesianinference_amd import _hip, hipops

pytestmark = pytest.mark.gpu
PREC = {'bf16': _hip.PREC_BF16, 'fp16': _hip.PREC_FP16, 'f32': _hip.PREC_F32}


def launch(name, rnd, fmt):
    """{ctx, dQ, dK, dV: [B, H, S, D], lse: [B, H, S]} of the HIP kernels on the round's inputs, on the CPU; the case's checks on what a launch must not touch"""
    case = P.CASES[name]
    dev = torch.device('cuda:0')
    qkv64, dctx64 = P.inputs(name, rnd, fmt)
    qkv, dctx = qkv64.to(P.DTYPE[fmt]).to(dev), dctx64.to(P.DTYPE[fmt]).to(dev)
    q0 = P.q_first(case)
    if case.q_begin:
        ctx, lse = hipops.attention_fwd(qkv, case.H, case.sep, PREC[fmt], q_begin=case.sep)
        assert torch.isnan(ctx[:, :q0].float()).all() and torch.isnan(lse[:, :, :q0]).all(), 'a skipped row lost its fill'
        dctx[:, :q0] = float('nan')      # ... and is not read
        dqkv = hipops.attention_bwd(qkv, ctx, lse, dctx, case.H, case.sep, PREC[fmt], q_begin=case.sep)
        assert (dqkv[:, :q0, :case.E] == 0).all(), 'dQ below the first query block is not zero'
    else:
        ctx, lse = hipops.attention_fwd(qkv, case.H, case.sep, PREC[fmt])
        dqkv = hipops.attention_bwd(qkv, ctx, lse, dctx, case.H, case.sep, PREC[fmt])
    torch.cuda.synchronize()
    out = dict(zip(P.TENSORS, [P.heads(t.double().cpu(), case.H) for t in (ctx,) + dqkv.split(case.E, -1)]))
    out['lse'] = lse.double().cpu()
    return out


def compare(name, rnd, fmt, got, ref, bound):
    """({tensor: value / bound}, [what failed, in words]) of one round"""
    case = P.CASES[name]
    sc, q0 = P.scales(name, rnd, fmt), P.q_first(case)
    ratios, failed = {}, []
    where = f'round {rnd[0]} {rnd[1]}'
    for t in P.TENSORS:
        first = q0 if t == 'ctx' else 0
        if not torch.isfinite(got[t][:, :, first:]).all():
            b, h, i = [int(x) for x in (~torch.isfinite(got[t][:, :, first:])).any(-1).nonzero()[0]]
            failed.append(f'{t}, {where}: NaN or inf at dataset {b}, head {h}, row {i + first}')
        err, row = P.slice_errors(got[t], ref[t], sc[t], first)
        zero = P.zero_slices(ref[t])
        for b, h in zero.nonzero().tolist():      # an exact zero of the reference is an exact zero of the kernels
            if (got[t][b, h] != 0).any():
                failed.append(f'{t}, {where}: dataset {b}, head {h} is identically zero in the reference, not in the output')
        ratios[t] = (err / bound[t]).max().item()
        for b, h in (err >= bound[t]).nonzero().tolist():
            i = int(row[b, h])
            failed.append(f'{t}, {where}: dataset {b}, head {h}, worst row {i} (slab {i // P.SLAB}): {err[b, h].item():.3e} is not below the bound {bound[t]:.3e}')
    if not torch.isfinite(got['lse'][:, :, q0:]).all():
        failed.append(f'lse, {where}: NaN or inf')
    d = (got['lse'] - ref['lse'])[:, :, q0:].abs() / ref['smax']
    ratios['lse'] = torch.nan_to_num(d, nan=float('inf')).max().item() / bound['lse']
    if not ratios['lse'] < 1:
        b, h, i = [int(x) for x in (torch.nan_to_num(d, nan=float('inf')) == torch.nan_to_num(d, nan=float('inf')).max()).nonzero()[0]]
        failed.append(f'lse, {where}: dataset {b}, head {h}, row {i + q0} (slab {(i + q0) // P.SLAB}): {ratios["lse"] * bound["lse"]:.3e} is not below the bound {bound["lse"]:.3e}')
    return ratios, failed


def check(name, fmt, reference=P.reference):
    case = P.CASES[name]
    worst, failed = {}, []
    for rnd in P.rounds(case):
        ref, _, bound = reference(name, rnd, fmt)
        ratios, f = compare(name, rnd, fmt, launch(name, rnd, fmt), ref, bound)
        failed += f
        print(*f, sep='\n', end='\n' if f else '')
        worst = {t: max(v, worst.get(t, 0.0)) for t, v in ratios.items()}
    for t, v in worst.items():
        print(f'{name} {fmt} {t}: {v:.3f} x the bound')
        try:
            bounds.within(f'{t} value / bound', v, 1.0)
        except AssertionError as e:
            failed.append(f'{t}: the worst round: {e}')
    return failed


@pytest.mark.parametrize('fmt', P.FORMATS)
@pytest.mark.parametrize('name', list(P.CASES))
def test_planted_keys(name, fmt):
    failed = check(name, fmt)
    assert not failed, f'{len(failed)} failures\n' + '\n'.join(failed[:40])
