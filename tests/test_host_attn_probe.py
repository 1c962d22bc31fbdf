"""The inputs of tests/test_gpu_attn_probe.py do what they are built for, shown on the CPU from the f64 reference alone (tests/attn_probe_cases.py holds the
construction, the matrix and the rules):

  1. concentration: for every query of every round the keys with p >= 1/16 number 1 - 16 and hold >= 1 - 1e-6 of the mass;
  2. coverage over the rounds: every (32-query slab, key j < sep) pair has a query of the slab with p_j >= 1/16 (the ragged last slab of a case, 2 - 28 queries,
     through the 'tail' rounds), and every test row has its self key at p >= 1/16 in one round and at p <= 1e-6 in another (a
     case without train rows has no other key: there the self key holds everything in its one round);
  3. sensitivity: every planted fault, in every format, moves one of ctx, dQ, dK, dV by >= 8 x the bound the GPU test asserts; every class of fault that removes or
     adds a key does so on ctx or dV alone; and over the faults of a class dQ and dK each reach >= 1 x their bound in fp16 and f32 (bf16: recorded).

The multiples go to profiles/attn_probe_fault_sensitivity.json when PFN_RECORD_FAULTS names that file (run with -k "not dropout").

Under dropout on the probabilities (the tests with `dropout` in their names; DROP_CASES x DROP_PAIRS of attn_probe_cases):

  4. the masks are the kernels' integers: keep_masks against mix32(s ^ i 0x9E3779B1 ^ j 0x85EBCA77) >= thr evaluated here in plain integers, at (i, j) on both
     sides of 256, and a keep rate within 0.01 of 1 - p;
  5. coverage, a condition on the inputs: in every round, (dataset, head) and full 32-query slab some query keeps a targeted key and some query loses one; the
     ragged last slab does both over the rounds of its case (attn_probe_cases.drop_coverage_gaps; a seed that fails is replaced, the condition is not);
  6. the emulation under the masks is the reference without a format, and of the order of the format's unit roundoff with one;
  7. sensitivity: every planted mask fault (the mask of key j + 1 inside one tile for one slab, key or query index modulo 256, the mask of the next head or dataset,
     the self key of the test rows unmasked), every backward-only fault (keep transposed, dV from the unmasked P, dP without keep, dP without 1 / (1 - p)) and
     ctx without 1 / (1 - p), planted into the f64 reference alone, moves one of ctx, dQ, dK, dV by >= 8 x the bound the GPU test asserts, in every format and for
     both pairs; a backward-only fault does so on a gradient.  A fault is planted where the arithmetic can show it (attn_probe_cases.drop_faults): the modulo-256
     ones at S > 256, the next head's or dataset's mask at H > 1, B > 1, and keep transposed and the two dP faults not at sep = 0, where only keep(i, i) is read
     and dS = 0 whatever dP is.

Their multiples go to profiles/attn_probe_dropout_fault_sensitivity.json the same way (run with -k dropout)."""
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


def emulation_without_a_format_is_the_reference(name, drop=None):
    case = P.CASES[name]
    rnd = P.rounds(case)[-1]
    qkv, dctx = P.inputs(name, rnd, 'bf16')
    masks = None if drop is None else P.drop_masks(case, drop)
    a, b = qkv.clone().requires_grad_(True), qkv.clone().requires_grad_(True)
    ctx_a, lse_a, _ = P.attention_graph(a, case.H, case.sep, masks=masks)
    ctx_b, lse_b, _ = P.attention_graph(b, case.H, case.sep, O._Sites(O.Rounding(None), {}), masks=masks)
    ga, = torch.autograd.grad(ctx_a, a, dctx)
    gb, = torch.autograd.grad(ctx_b, b, dctx)
    assert torch.equal(lse_a, lse_b)
    for x, y in ((ctx_a, ctx_b), (ga, gb)):      # (the hooked softmax divides by the sum last: the last bits may differ)
        assert (x - y).abs().max() <= 1e-13 * max(x.abs().max().item(), 1e-30)
    want, want_lse = P.attention_reference(qkv, case.H, case.sep, masks)
    assert torch.equal(want, ctx_a.detach()) and torch.equal(want_lse, lse_a.detach())
    return a, ctx_a, lse_a, ga


@pytest.mark.parametrize('name', NAMES)
def test_emulation_without_a_format_is_the_reference(name):
    emulation_without_a_format_is_the_reference(name)


@pytest.mark.parametrize('fmt', P.FORMATS)
@pytest.mark.parametrize('name', NAMES)
def test_emulated_errors_are_those_of_the_format(name, fmt):
    emulated_errors_are_those_of_the_format(name, fmt)


def emulated_errors_are_those_of_the_format(name, fmt, drop=None):
    """e per tensor: a small multiple of the format's unit roundoff in 16 bits (so the bound is a small multiple of it too).  f32: the statistics of a row are rounded
    at the size of the scores, s2 = max |score| log2(e) = 2^7 - 2^8.5 here (attn_probe_cases._FlashF32): lse, lse log2(e) and the product of the two f32 constants
    each move the backward's P of a row by <= s2 2^-24 ln 2 (x 2 for the constants), 2.8 s2 2^-24 together; a tensor whose every slice reaches the floor of the
    statistic is held to 4 s2 2^-24.  Where a slice of the reference lies under the floor (sep <= 1: dQ, dK are zero or nearly), e is the dP - delta noise against
    1e-2 of the scale -- the CPU's summation order, not the kernels': one realisation of a random quantity of that size -- and is held below the unit roundoff
    of fp16; what it must stay under is the planted faults, which the next test asserts"""
    case = P.CASES[name]
    u = 2.0 ** -24 if fmt == 'f32' else O.UNIT_ROUNDOFF[fmt]
    tag = '' if drop is None else f' p {drop[0]} seed {drop[1]:#x}'
    for rnd in (P.rounds(case)[0], P.rounds(case)[-1]):
        ref, e, bound = P.reference(name, rnd, fmt, drop)
        sc = P.scales(name, rnd, fmt)
        _record[f'{name} {fmt}{tag} {rnd[0]} {rnd[1]}: emulated e in units of u'] = {t: v / u for t, v in e.items()}
        for t in P.TENSORS:
            floored = (ref[t].abs().amax((-1, -2)) < 1e-2 * sc[t]).any()
            if fmt == 'f32':
                assert e[t] < (O.UNIT_ROUNDOFF['fp16'] if floored else 4 * ref['smax'] * P.LOG2E_F32 * u), (t, e[t] / u)
            elif drop is not None and floored and t in ('dQ', 'dK'):
                # (16 bit, dropout, sep <= 1: site 'delta'.  Without dropout the output of a row with one key is v itself, exact in the format; v / (1 - p) is
                # not (p = 0.5 aside), so delta = rowsum(dO rnd(o)) misses sum_k P_k dP_k by |c_i| <= u s_i, s_i = sum_d |dO_id o_id| of THESE inputs, and
                # dS = -c P where the reference has 0: |dQ_i| <= |c_i| max |k| / sqrt(D), |dK_j| <= sum_i P_ij |c_i| max |q| / sqrt(D); in units of the
                # tensors' scales (max |dO| max |v| max |k or q| / sqrt(D)) and read against 1e-2 of them, plus the 8 u of every other site.  The dQ figure is
                # what one row's roundings can do and sits 1.7 - 2.2 x over e; the dK one adds the |c_i| of a key's rows up, signs not cancelling: the same at sep = 0, 35 - 60 x over e at sep = 1 (199 rows on key 0).)
                s = (P.heads(P.inputs(name, rnd, fmt)[1], case.H) * ref['ctx']).abs().sum(-1)      # [B, H, S]
                worst = s.max() if t == 'dQ' else (P.probabilities(name, rnd) * s[..., None]).sum(-2).max()
                assert e[t] < 100 * u * worst.item() / (sc['ctx'] * sc['dV']) + 8 * u, (t, e[t] / u)
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


# ---- under dropout on the probabilities ------------------------------------------------------------------------------------------------------------------------------
DROP_IDS = [f'p{p}-{seed:#x}' for p, seed in P.DROP_PAIRS]
_M = 0xFFFFFFFF


def _mix32(h):
    """pfn_host.h mix32 in plain integers"""
    h &= _M
    h ^= h >> 16
    h = h * 0x7feb352d & _M
    h ^= h >> 15
    h = h * 0x846ca68b & _M
    return h ^ h >> 16


def test_dropout_matrix_is_the_one_the_kernels_need():
    assert set(P.DROP_CASES) <= set(P.CASES) and not any(P.CASES[n].q_begin for n in P.DROP_CASES)
    assert {P.head_dim(P.CASES[n]) for n in P.DROP_CASES} == {32, 64, 128, 256} and {P.CASES[n].sep for n in P.DROP_CASES} >= {0, 1, 257, 512}
    assert all(0 < p < 1 and 0 <= s <= _M for p, s in P.DROP_PAIRS) and P.DROP_PAIRS[1][1] >> 31 == 1
    assert P.residue_tensors('S130-sep0', P.DROP_PAIRS[0]) == ('dQ', 'dK') and not P.residue_tensors('S130-sep0', None) and not P.residue_tensors('S200-sep1', P.DROP_PAIRS[0])


@pytest.mark.parametrize('drop', P.DROP_PAIRS, ids=DROP_IDS)
def test_dropout_masks_are_the_kernels_integers(drop):
    p, seed = drop
    thr = min(int(float(torch.tensor(p, dtype=torch.float32).item()) * 4294967296.0), _M)      # pfn_kernels.h dropout_threshold
    for name in ('S520-sep512', 'S333-sep301', 'S100-sep70'):
        case = P.CASES[name]
        keep = P.keep_masks(case, seed, p)
        assert keep.shape == (case.B, case.H, case.S, case.S) and keep.dtype == torch.bool
        assert abs(keep.float().mean().item() - (1 - p)) < 0.01
        assert P.keep_masks(case, seed, p) is keep      # cached per (case, seed, p)
        top = case.S - 1
        for b, h in ((0, 0), (case.B - 1, case.H - 1), (0, case.H - 1)):
            s = _mix32(seed ^ (0xC2B2AE35 * (b * case.H + h + 1) & _M))      # dropout_pair_seed
            assert s == O.dropout_pair_seed(seed, b * case.H + h)
            for i, j in ((0, 0), (0, 1), (1, 0), (31, 63), (64, 32), (top, top), (top, 0), (0, top), (255, 256), (256, 255), (300, 257), (top, top - 1)):
                i, j = min(i, top), min(j, top)
                want = _mix32(s ^ (i * 0x9E3779B1 & _M) ^ (j * 0x85EBCA77 & _M)) >= thr      # dropout_keep
                assert bool(keep[b, h, i, j]) == want, (name, b, h, i, j)
    for pair in (0, 1, 7):      # different pairs, different masks
        assert O.dropout_pair_seed(seed, pair) != O.dropout_pair_seed(seed, pair + 1)


@pytest.mark.parametrize('drop', P.DROP_PAIRS, ids=DROP_IDS)
@pytest.mark.parametrize('name', P.DROP_CASES)
def test_dropout_coverage(name, drop):
    gaps = P.drop_coverage_gaps(name, drop)
    assert not gaps, f'{len(gaps)} gaps: choose another seed\n' + '\n'.join(gaps[:20])


@pytest.mark.parametrize('drop', P.DROP_PAIRS, ids=DROP_IDS)
@pytest.mark.parametrize('name', P.DROP_CASES)
def test_emulation_without_a_format_is_the_reference_under_dropout(name, drop):
    """... and the mask does what the kernels do with it: lse is that of the unmasked softmax, a masked key gives nothing to ctx, and the written-out backward
    (dV from P', dP = (dO V^T) keep / (1 - p)) is the gradient autograd takes through a plain product with P keep / (1 - p)"""
    case = P.CASES[name]
    a, ctx_a, lse_a, ga = emulation_without_a_format_is_the_reference(name, drop)
    qkv, dctx = a.detach(), P.inputs(name, P.rounds(case)[-1], 'bf16')[1]
    assert torch.equal(lse_a.detach(), P.attention_reference(qkv, case.H, case.sep)[1])
    b = qkv.clone().requires_grad_(True)
    q, k, v = [P.heads(t, case.H) for t in b.split(case.E, -1)]
    scores = (q @ k.transpose(-1, -2) / (P.head_dim(case) ** 0.5)).masked_fill(~P.visible(case.S, case.sep), float('-inf'))
    ctx_b = ((torch.softmax(scores, -1) * P.keep_masks(case, drop[1], drop[0]) * P.keep_scale(drop[0])) @ v).transpose(1, 2).reshape(case.B, case.S, case.E)
    gb, = torch.autograd.grad(ctx_b, b, dctx)
    for x, y in ((ctx_a, ctx_b), (ga, gb)):
        assert (x - y).abs().max() <= 1e-13 * max(x.abs().max().item(), 1e-30)


@pytest.mark.parametrize('drop', P.DROP_PAIRS, ids=DROP_IDS)
@pytest.mark.parametrize('fmt', P.FORMATS)
@pytest.mark.parametrize('name', P.DROP_CASES)
def test_emulated_errors_are_those_of_the_format_under_dropout(name, fmt, drop):
    emulated_errors_are_those_of_the_format(name, fmt, drop)


@pytest.mark.parametrize('drop', P.DROP_PAIRS, ids=DROP_IDS)
@pytest.mark.parametrize('fmt', P.FORMATS)
@pytest.mark.parametrize('name', P.DROP_CASES)
def test_planted_dropout_faults_exceed_the_bound(name, fmt, drop):
    faults = P.drop_faults(name)
    sep, S = P.CASES[name].sep, P.CASES[name].S
    have = {f.cls for f in faults}
    assert have >= {P.MASK_CLASSES[0], P.MASK_CLASSES[5], P.BACKWARD_CLASSES[1], P.FORWARD_CLASSES[0]}
    assert (sep == 0) == (not have >= set(P.BACKWARD_CLASSES)) and (S > 256) == (have >= set(P.MASK_CLASSES[1:3]))
    missed = []
    for fault in faults:
        rnds, mult = P.drop_fault_multiples(name, fmt, drop, fault)
        _record[f'{name} {fmt} p {drop[0]} seed {drop[1]:#x}: {fault.label}'] = dict(mult, rounds=', '.join(f'{k} {r}' for k, r in rnds))
        tensors = ('dQ', 'dK', 'dV') if fault.cls in P.BACKWARD_CLASSES else P.TENSORS
        best = max(mult[t] for t in tensors)
        if fault.cls in P.BACKWARD_CLASSES + P.FORWARD_CLASSES:      # (planted where they claim to be)
            assert all(mult[t] == 0 for t in (('ctx',) if fault.cls in P.BACKWARD_CLASSES else ('dQ', 'dK', 'dV')))
        if not best >= 8:
            missed.append(f'{fault.label}: {best:.3g} x the {fmt} bound on the best of {tensors}, needs 8 ({rnds})')
    assert not missed, '\n'.join(missed)
