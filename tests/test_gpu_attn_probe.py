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
launch_attn_bwd now takes a batch without train rows (one eval position, no dropout) through attn_bwd_self_only_kernel: dV = dO, dQ = dK = 0.

Under dropout on the probabilities (test_planted_keys_under_dropout: attn_probe_cases.DROP_CASES x FORMATS x DROP_PAIRS through pfn_op_attention_fwd_dropout /
pfn_op_attention_bwd_dropout, the DROP = true kernels and the `drop` branches of attn_bwd_plain_*): the same rounds, statistic and bound rule, reference and
emulation under the masks the kernels regenerate from (pair seed, query, key).  tests/test_host_attn_probe.py shows that a mask read one key over, a key or query
index taken modulo 256, the mask of another head or dataset, an unmasked self key, a mask transposed in the backward, dV or dP without the mask and a missing
1 / (1 - p) each exceed these bounds by >= 8 x.  One rule differs, at S130-sep0: launch_attn_bwd sends a batch without train rows to the self-only kernel only
without dropout, so under dropout the general query-block pass runs and dQ, dK carry the dP - delta residue where the reference is 0; they are held to their
bound on the floored scale, not to an exact zero (attn_probe_cases.residue_tensors).  Everywhere else the exact-zero rule stands.

The first run under dropout was a finding of the first kind, a rounding site the emulation lacked: S200-sep1 and S130-sep0 at p = 0.2, bf16 and fp16, rounds
keys 0 and tail 0, dQ and dK of every dataset and head at 48 - 293 x the bound (f32, p = 0.5 and every other case passed).  In those rounds every row has one key
with mass, dS is 0 in the reference, and the kernels form dS = P (dP - delta) with delta = rowsum(dO o) from the STORED output (attn_delta_kernel, attention.hip
:719-724).  Without dropout that output is v itself, exact in the format; v / (1 - 0.2) is not, and delta misses sum_k P_k dP_k by u |dO o|: 1.2 u (dQ) to
7 u (dK) of the natural scale, read against the floor of 1e-2 of it (at p = 0.5 the factor 2 is exact).  The site is now 'delta' in
oracle.pfn_oracle.ROUNDING_SITES (_Sites.stored_delta), applied by attn_probe_cases.attention_graph under dropout only: the graph without dropout, its e and every
bound of test_planted_keys are what they were.  No kernel was changed.  With the site those dQ and dK stand at 0.333 x the bound = 1.00 x e in bf16 and fp16:
the kernels return the emulated residue itself.

Measured under dropout (profiles/attn_probe_dropout_parity_measured.json, value / bound, the largest over cases, pairs and rounds): bf16 ctx 0.33, dQ 0.66, dK 0.68,
dV 0.63; fp16 0.33, 0.63, 0.56, 0.61; f32 0.31, 0.33, 0.95, 0.61; lse 0.20.  The f32 dK of 0.95 is S200-sep1 at p = 0.2 (0.55 at p = 0.5, <= 0.35 in every other case): in its rounds
keys 0 and tail 0 every row has one key with mass, the reference dK lies under the floor, and both the kernels and _FlashF32 return the dP - delta noise of their
own summation order.  Slowest dropout test 4.4 - 4.7 s over three runs (S520-sep512 in 16 bit, 96 rounds; 4.2 - 4.3 s without dropout in the same runs), the 42 cases and the three p_drop = 0 tests 36 s together."""
import pytest
import torch

import attn_probe_cases as P
import bounds
from transformerscandobayesianinference_amd import _hip, hipops

pytestmark = pytest.mark.gpu
PREC = {'bf16': _hip.PREC_BF16, 'fp16': _hip.PREC_FP16, 'f32': _hip.PREC_F32}
PFN_ERR_ARGUMENT = -4      # include/pfn_hip.h


def launch(name, rnd, fmt, drop=None):
    """{ctx, dQ, dK, dV: [B, H, S, D], lse: [B, H, S]} of the HIP kernels on the round's inputs, on the CPU; the case's checks on what a launch must not touch.
    drop = (p, site seed): both launches with dropout on the probabilities"""
    case = P.CASES[name]
    dev = torch.device('cuda:0')
    qkv64, dctx64 = P.inputs(name, rnd, fmt)
    qkv, dctx = qkv64.to(P.DTYPE[fmt]).to(dev), dctx64.to(P.DTYPE[fmt]).to(dev)
    q0 = P.q_first(case)
    if drop is not None:
        assert not case.q_begin
        ctx, lse = hipops.attention_fwd(qkv, case.H, case.sep, PREC[fmt], p_drop=drop[0], drop_seed=drop[1])
        dqkv = hipops.attention_bwd(qkv, ctx, lse, dctx, case.H, case.sep, PREC[fmt], p_drop=drop[0], drop_seed=drop[1])
    elif case.q_begin:
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


def compare(name, rnd, fmt, got, ref, bound, residue=()):
    """({tensor: value / bound}, [what failed, in words]) of one round; residue: the tensors held to their bound where the reference is identically zero, not to
    an exact zero (attn_probe_cases.residue_tensors)"""
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
        for b, h in [] if t in residue else zero.nonzero().tolist():      # an exact zero of the reference is an exact zero of the kernels
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


def check(name, fmt, reference=P.reference, drop=None):
    case = P.CASES[name]
    worst, failed = {}, []
    for rnd in P.rounds(case):
        ref, _, bound = reference(name, rnd, fmt) if drop is None else reference(name, rnd, fmt, drop)
        ratios, f = compare(name, rnd, fmt, launch(name, rnd, fmt, drop), ref, bound, P.residue_tensors(name, drop))
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


@pytest.mark.parametrize('drop', P.DROP_PAIRS, ids=[f'p{p}-{seed:#x}' for p, seed in P.DROP_PAIRS])
@pytest.mark.parametrize('fmt', P.FORMATS)
@pytest.mark.parametrize('name', P.DROP_CASES)
def test_planted_keys_under_dropout(name, fmt, drop):
    failed = check(name, fmt, drop=drop)
    assert not failed, f'{len(failed)} failures\n' + '\n'.join(failed[:40])


@pytest.mark.parametrize('fmt', P.FORMATS)
def test_p_drop_zero_is_the_launch_without_dropout(fmt):
    """hipops with p_drop = 0.0 and pfn_op_attention_*_dropout with p_drop = 0 (whatever the seed) are the entry points without dropout, bit for bit; a p_drop
    outside [0, 1) is an argument error"""
    name, rnd = 'S333-sep301', ('self', 1)
    case = P.CASES[name]
    qkv64, dctx64 = P.inputs(name, rnd, fmt)
    qkv, dctx = qkv64.to(P.DTYPE[fmt]).cuda(), dctx64.to(P.DTYPE[fmt]).cuda()
    B, S, E, H, sep = case.B, case.S, case.E, case.H, case.sep
    ctx, lse = hipops.attention_fwd(qkv, H, sep, PREC[fmt])
    dqkv = hipops.attention_bwd(qkv, ctx, lse, dctx, H, sep, PREC[fmt])
    ctx0, lse0 = hipops.attention_fwd(qkv, H, sep, PREC[fmt], p_drop=0.0, drop_seed=P.DROP_PAIRS[1][1])
    dqkv0 = hipops.attention_bwd(qkv, ctx, lse, dctx, H, sep, PREC[fmt], p_drop=0.0, drop_seed=P.DROP_PAIRS[1][1])
    bits = lambda t: t.contiguous().view(torch.uint8)
    assert torch.equal(bits(ctx0), bits(ctx)) and torch.equal(bits(lse0), bits(lse)) and torch.equal(bits(dqkv0), bits(dqkv))
    lib, sp = _hip.lib(), _hip.stream_ptr()
    ctx1, lse1, dqkv1 = torch.empty_like(ctx), torch.empty_like(lse), torch.full_like(qkv, float('nan'))
    delta = torch.zeros(2, B, H, S, dtype=torch.float32, device=qkv.device)
    ds = torch.full((lib.pfn_op_attention_bwd_ws_bytes(B, S, H, PREC[fmt]),), 0xff, dtype=torch.uint8, device=qkv.device)
    fwd = lambda p: lib.pfn_op_attention_fwd_dropout(qkv.data_ptr(), ctx1.data_ptr(), lse1.data_ptr(), B, S, E, H, sep, PREC[fmt], p, P.DROP_PAIRS[1][1], sp)
    bwd = lambda p: lib.pfn_op_attention_bwd_dropout(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), dctx.data_ptr(), dqkv1.data_ptr(), delta.data_ptr(), ds.data_ptr(),
                                                     B, S, E, H, sep, PREC[fmt], 0, p, P.DROP_PAIRS[1][1], sp)
    assert fwd(0.0) == 0 and bwd(0.0) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(ctx1), bits(ctx)) and torch.equal(bits(lse1), bits(lse)) and torch.equal(bits(dqkv1), bits(dqkv))
    for p in (1.0, -0.25, float('nan')):
        assert fwd(p) == PFN_ERR_ARGUMENT and bwd(p) == PFN_ERR_ARGUMENT, p
    torch.cuda.synchronize()
    assert torch.equal(bits(ctx1), bits(ctx)) and torch.equal(bits(dqkv1), bits(dqkv))      # (a refused call launches nothing)
