"""The inputs of tests/test_gpu_attn_probe.py do what they are built for, shown on the CPU from the f64 reference alone (tests/attn_probe_cases.py holds the
construction, the matrix and the rules):

  1. concentration: for every query of every round the keys with p >= 1/16 number 1 - 16 and hold >= 1 - 1e-6 of the mass;
  2. coverage over the rounds: every (32-query slab, key j < sep) pair has a query of the slab with p_j >= 1/16 (the ragged last slab of a case, 2 - 28 queries,
     through the 'tail' rounds), and every test row has its self key at p >= 1/16 in one round and at p <= 1e-6 in another (a
     case without train rows has no other key: there the self key holds everything in its one round);
  3. sensitivity: every planted fault, in every format, moves one of ctx, dQ, dK, dV by >= 8 x the bound the GPU test asserts; every class of fault that removes or
     adds a key does so on ctx or dV alone; and over the faults of a class dQ and dK each reach >= 1 x their bound in fp16 and f32 (bf16: recorded).

The multiples go to profiles/attn_probe_fault_sensitivity.json when PFN_RECORD_FAULTS names that file."""
import json
import os

import pytest
import torch

import attn_probe_cases as P
from oracle import pfn_oracle as O

_record = {}
NAMES = list(P.CASES)


def teardown_module(module):
    path = os.environ.get('PFN_RECORD_FAULTS')
    if path and _record:
        sig = lambda v: float(f'{v:.4g}') if isinstance(v, float) else v
        json.dump({k: {kk: sig(vv) for kk, vv in v.items()} for k, v in sorted(_record.items())}, open(path, 'w'), indent=1)


def test_the_matrix_is_the_one_the_kernels_need():
    assert all(c.S <= 700 and c.E % c.H == 0 and P.head_dim(c) in (32, 64, 128, 256) for c in P.CASES.values())
    assert {P.head_dim(c) for c in P.CASES.values()} == {32, 64, 128, 256}
    assert [P.q_first(c) for c in P.CASES.values() if c.q_begin] == [256, 512]
    assert P.rounds(P.CASES['S130-sep0']) == [('self', 0)] and len(P.rounds(P.CASES['S700-sep600'])) == 19 + 19 + 22
    assert P.kv_tile(P.CASES['S520-sep512'], 'bf16') == 64 and P.kv_tile(P.CASES['S520-sep512'], 'f32') == 32 and P.kv_tile(P.CASES['S300-sep200-D256'], 'fp16') == 32


@pytest.mark.parametrize('name', NAMES)
def test_inputs_are_exact_in_every_format(name):
    case = P.CASES[name]
    for rnd in P.rounds(case)[::7]:
        for fmt in P.FORMATS:
            qkv, dctx = P.inputs(name, rnd, fmt)
            for t in (qkv, dctx):
                assert torch.equal(t.to(P.DTYPE[fmt]).double(), t)
            q, k, _ = qkv.split(case.E, -1)
            assert set(q.unique().tolist()) <= {0.0, 16.0, -16.0} and set(k.unique().tolist()) == {1.0, -1.0}
        if case.q_begin:
            assert (dctx[:, :case.sep] == 0).all() and (dctx[:, case.sep:] != 0).any()
    k0 = P.heads(P.qk(case, P.rounds(case)[0])[1], case.H)      # another head's or dataset's keys are other keys
    for dim in (0, 1):
        if k0.shape[dim] > 1:
            assert ((k0 != k0.roll(-1, dim)).any(-1).float().mean((-1,)) > 0.9).all()


@pytest.mark.parametrize('name', NAMES)
def test_concentration_and_coverage(name):
    case = P.CASES[name]
    S, sep = case.S, case.sep
    nslab = -(-S // P.SLAB)
    hit = torch.zeros(case.B, case.H, nslab, max(sep, 1), dtype=torch.bool)      # (slab, key): some query of the slab has p_j >= 1/16
    self_hi = torch.zeros(case.B, case.H, S, dtype=torch.bool)
    self_lo = torch.zeros(case.B, case.H, S, dtype=torch.bool)
    for rnd in P.rounds(case):
        p = P.probabilities(name, rnd)
        big = p >= 1 / 16
        count, mass = big.sum(-1), (p * big).sum(-1)
        assert count.min() >= 1 and count.max() <= 16, (rnd, count.min().item(), count.max().item())      # condition 1
        assert mass.min() >= 1 - 1e-6, (rnd, 1 - mass.min().item())
        for s in range(nslab):
            hit[:, :, s] |= big[:, :, P.SLAB * s:P.SLAB * s + P.SLAB, :max(sep, 1)].any(2)
        diag = p.diagonal(dim1=-2, dim2=-1)
        self_hi |= diag >= 1 / 16
        self_lo |= diag <= 1e-6
    if sep > 0:                                                                                            # condition 2
        assert hit.all(), f'{(~hit).sum().item()} (slab, key) pairs of {hit.numel()} are never chosen: {(~hit).nonzero()[:5].tolist()}'
        assert self_hi[:, :, sep:].all() and self_lo[:, :, sep:].all(), ((~self_hi[:, :, sep:]).sum().item(), (~self_lo[:, :, sep:]).sum().item())
    else:
        assert self_hi.all()


@pytest.mark.parametrize('name', NAMES)
def test_emulation_without_a_format_is_the_reference(name):
    case = P.CASES[name]
    rnd = P.rounds(case)[-1]
    qkv, dctx = P.inputs(name, rnd, 'bf16')
    a, b = qkv.clone().requires_grad_(True), qkv.clone().requires_grad_(True)
    ctx_a, lse_a, _ = P.attention_graph(a, case.H, case.sep)
    ctx_b, lse_b, _ = P.attention_graph(b, case.H, case.sep, O._Sites(O.Rounding(None), {}))
    ga, = torch.autograd.grad(ctx_a, a, dctx)
    gb, = torch.autograd.grad(ctx_b, b, dctx)
    assert torch.equal(lse_a, lse_b)
    for x, y in ((ctx_a, ctx_b), (ga, gb)):      # (the hooked softmax divides by the sum last: the last bits may differ)
        assert (x - y).abs().max() <= 1e-13 * max(x.abs().max().item(), 1e-30)
    want, want_lse = P.attention_reference(qkv, case.H, case.sep)
    assert torch.equal(want, ctx_a.detach()) and torch.equal(want_lse, lse_a.detach())


@pytest.mark.parametrize('fmt', P.FORMATS)
@pytest.mark.parametrize('name', NAMES)
def test_emulated_errors_are_those_of_the_format(name, fmt):
    """e per tensor: a small multiple of the format's unit roundoff in 16 bits (so the bound is a small multiple of it too).  f32: the statistics of a row are rounded
    at the size of the scores, s2 = max |score| log2(e) = 2^7 - 2^8.5 here (attn_probe_cases._FlashF32): lse, lse log2(e) and the product of the two f32 constants
    each move the backward's P of a row by <= s2 2^-24 ln 2 (x 2 for the constants), 2.8 s2 2^-24 together; a tensor whose every slice reaches the floor of the
    statistic is held to 4 s2 2^-24.  Where a slice of the reference lies under the floor (sep <= 1: dQ, dK are zero or nearly), e is the dP - delta noise against
    1e-2 of the scale -- the CPU's summation order, not the kernels': one realisation of a random quantity of that size -- and is held below the unit roundoff
    of fp16; what it must stay under is the planted faults, which the next test asserts"""
    case = P.CASES[name]
    u = 2.0 ** -24 if fmt == 'f32' else O.UNIT_ROUNDOFF[fmt]
    for rnd in (P.rounds(case)[0], P.rounds(case)[-1]):
        ref, e, bound = P.reference(name, rnd, fmt)
        sc = P.scales(name, rnd, fmt)
        _record[f'{name} {fmt} {rnd[0]} {rnd[1]}: emulated e in units of u'] = {t: v / u for t, v in e.items()}
        for t in P.TENSORS:
            if fmt == 'f32':
                floored = (ref[t].abs().amax((-1, -2)) < 1e-2 * sc[t]).any()
                assert e[t] < (O.UNIT_ROUNDOFF['fp16'] if floored else 4 * ref['smax'] * P.LOG2E_F32 * u), (t, e[t] / u)
            elif P.zero_slices(ref[t]).all():
                assert e[t] == 0
            else:
                assert e[t] < 8 * u, (t, e[t] / u)
        assert e['lse'] < 8 * 2.0 ** -24 and bound['lse'] <= 64 * 2.0 ** -23


@pytest.mark.parametrize('fmt', P.FORMATS)
@pytest.mark.parametrize('name', NAMES)
def test_planted_faults_exceed_the_bound(name, fmt):
    missed, by_class = [], {}
    for fault in P.planted_faults(name, fmt):
        rnds, mult = P.fault_multiples(name, fmt, fault)
        _record[f'{name} {fmt}: {fault.label}'] = dict(mult, rounds=', '.join(f'{k} {r}' for k, r in rnds))
        by_class.setdefault(fault.cls, []).append(mult)
        if not max(mult.values()) >= 8:
            missed.append(f'{fault.label}: {max(mult.values()):.3g} x the {fmt} bound on the best tensor, needs 8 ({rnds})')
    for cls, mults in by_class.items():
        best = {t: max(m[t] for m in mults) for t in P.TENSORS}
        _record[f'{name} {fmt} class: {cls}'] = best
        if cls in P.KEY_CLASSES and not max(best['ctx'], best['dV']) >= 8:
            missed.append(f'class {cls}: ctx {best["ctx"]:.3g}, dV {best["dV"]:.3g} x the {fmt} bound, one needs 8')
        if fmt != 'bf16' and (P.CASES[name].sep > 0 or cls in P.KEY_CLASSES):      # (a row with one visible key has dS = 0 whatever K holds: at sep = 0 only an added key moves dQ, dK)
            missed += [f'class {cls}: {t} {best[t]:.3g} x the {fmt} bound, needs 1' for t in ('dQ', 'dK') if not best[t] >= 1]
    assert not missed, '\n'.join(missed)
