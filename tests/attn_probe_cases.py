"""What tests/test_host_attn_probe.py (CPU) and tests/test_gpu_attn_probe.py (MI355X) share: training attention on CONSTRUCTED q / k / v, where every query puts all of
its softmax mass on a handful of chosen keys, so that a lost or misplaced key, tile, self key, head or dataset moves an output by 5 - 50 % of its scale in every
operand format (random inputs spread a row's mass over ~sep keys, and one key is then worth ~1 / sep of it: tests/test_gpu_ops.py cannot see such a fault).

Inputs per (dataset b, head h), D = E / H, n = D / 2, Hd the n x n Sylvester Hadamard matrix of +-1:
    code(j) = Hd[(j + o_bh) mod n] | Hd[((j + o_bh) div n) mod n]      n^2 distinct codes; two different codes agree in 0 or D / 2 places more than they disagree
    k_j = code(j),   q_i = A (code(t1(i)) + code(t2(i))),  A = 8       every value 0, +-1, +-16: exact in bf16, fp16 and f32, and so are the scores
    v, dctx = randn rounded to the operand type
The targeted keys tie at score A sqrt(D); every key of another code lies >= A sqrt(D) / 2 >= 22 below.  Keys that share a code (j, j + n^2, ...) and the two "cross"
codes (first half of one target, second half of the other) tie with the targets: ties between different keys are what make dS, hence dQ and dK, non-zero.
Rounds: 'keys' r = 0 .. ceil(sep / 32) - 1: t1(i) = (i + 32 r) mod sep, t2 = (t1 + n + 1) mod sep; 'self' r: the same, but every test row i >= sep has t1(i) = i;
'tail' r = 0 .. ceil(sep / m) - 1 where the last slab is ragged with m = S mod 32 queries: its row 32 floor(S / 32) + c has t1 = (c + m r) mod sep.

Statistic, per tensor (ctx, dQ, dK, dV): the largest over (b, h) of max |got - ref| over the slice / max(max |ref slice|, 1e-2 x the tensor's natural scale).
Bound (stack_cases.bound, from the reference only): 16-bit 3 x max(e, u), f32 4 x max(e, 2^-23), e = the same statistic of the emulation (the f64 graph under
oracle.pfn_oracle._Sites at the 'qkv', 'P', 'dS' and 'ctx' sites; f32: the graph run in torch.float32 with the softmax statistics rounded where the kernels round
them, _FlashF32) against the f64 reference.
"""
import functools
import math
from collections import namedtuple

import torch

import stack_cases
from oracle import pfn_oracle as O

A = 8.0
SLAB = 32
FORMATS = ('bf16', 'fp16', 'f32')
DTYPE = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'f32': torch.float32}
TENSORS = ('ctx', 'dQ', 'dK', 'dV')

Case = namedtuple('Case', 'B S E H sep q_begin')
CASES = {                                                     # what each reaches (16-bit, D <= 128: key tiles of 64, query blocks of 256; D = 256 and f32: 32 and 128; the kv pass: blocks of 256 keys)
    'S100-sep70': Case(2, 100, 128, 4, 70, False),            # D 32: one partial key tile; B H = 8
    'S130-sep129': Case(2, 130, 64, 2, 129, False),           # D 32: two tiles + 1 key; one test row per dataset
    'S333-sep301': Case(1, 333, 128, 4, 301, False),          # D 32: two query blocks; key blocks 256 + 45
    'S700-sep600': Case(1, 700, 128, 4, 600, False),          # D 32: three key blocks, the last ragged with 88; codes repeat (n^2 = 256 < sep)
    'S300-sep257': Case(1, 300, 128, 2, 257, False),          # D 64: the ragged last key block holds one key
    'S300-sep257-from': Case(1, 300, 128, 2, 257, True),      # ... from q_begin = sep (rounds down to 256)
    'S288-sep255': Case(1, 288, 64, 1, 255, False),           # D 64: sep one short of a block; 33 test rows
    'S520-sep512': Case(2, 520, 256, 2, 512, False),          # D 128: sep an exact multiple of 256; three query blocks
    'S520-sep512-from': Case(2, 520, 256, 2, 512, True),
    'S300-sep200-D256': Case(1, 300, 512, 2, 200, False),     # D 256: the four-wave kernels; f32: the split-V forward and attn_bwd_plain_*
    'S200-sep1': Case(2, 200, 64, 2, 1, False),               # D 32
    'S130-sep0': Case(2, 130, 64, 2, 0, False),               # D 32: ctx is v, dV is dctx, dQ and dK exactly zero
}


def head_dim(case):
    return case.E // case.H


def kv_tile(case, fmt):
    return 64 if fmt != 'f32' and head_dim(case) <= 128 else 32


def q_first(case):
    """the first query row a launch from q_begin = sep writes"""
    return case.sep // 256 * 256 if case.q_begin else 0


def rounds(case):
    """'tail' rounds: the ragged last slab has m = S mod 32 < 32 queries, which the shifts by 32 cannot walk over every key: ceil(sep / m) more rounds in which its
    rows step through the keys m at a time (the other rows repeat the 'keys' rounds)"""
    nr, m = -(-case.sep // SLAB), case.S % SLAB
    tail = [('tail', r) for r in range(-(-case.sep // m))] if m and case.sep else []
    return [('keys', r) for r in range(nr)] + [('self', r) for r in range(max(nr, 1))] + tail


# ---- the graph: reference, emulation and planted faults ----------------------------------------------------------------------------------------------------------
def visible(S, sep, device=None):
    """key j visible to query i iff j < sep or i == j: the mask of generate_D_q_matrix (transformer.py:34-41)"""
    allowed = torch.zeros(S, S, dtype=torch.bool, device=device)
    allowed[:, :sep] = True
    allowed |= torch.eye(S, dtype=torch.bool, device=device)
    return allowed


LOG2E_F32, LN2_F32 = 1.4426950216293335, 0.6931471824645996      # the f32 constants of attention.hip :146


class _FlashF32(torch.autograd.Function):
    """(q k^T unscaled, v) -> (softmax . v, lse) in f32 the way the exact-f32 kernels form them, which the dense f32 graph does not.  The scores here reach
    A sqrt(D) log2(e) ~ 65 - 370 in the kernels' log2 units, where an f32 carries 2^-18 .. 2^-16 absolutely, and the statistics are rounded there:
      forward, attention.hip :404-441  P = exp2(fma(S, c, -m)) against a running maximum m = f32(max S c): the product inside the fma is not rounded, m is;
               :306-307                the self key of a test row opens the state with m = f32(s c) and weight 1, so it weighs 2^r against a tied key, r the
                                       rounding of that product;
               :489                    lse = f32((m + log2 l) ln 2): rounded at the size of the scores;
      backward, :583 :601 :733 :1015   P = exp2(fma(S, c, -lse2)), lse2 = f32(lse log2 e): every P of a row is off by the factor 2^(rounding of lse2);
               :743                    dS = P (dP - delta), delta = sum(dO o) from the stored output: two f32 sums of the same products in different orders, so a
                                       row with one visible key has dS ~ 2^-24 |dP|, not 0.
    The 16-bit formats have the same roundings, 8 - 60 x below their unit roundoff.
    Dropout (masks = Masks in f32, or None), :447-453 :478: the numerators are masked after the row sums, which stay those of the unmasked softmax, and so does lse;
    the backward takes dV from P keep / (1 - p), dP = (dO V^T) keep / (1 - p) and delta from the stored (masked) output :849-850 :1058 :1506."""
    @staticmethod
    def forward(ctx, raw, v, allowed, self_rows, masks=None):
        D = v.shape[-1]
        c = (torch.tensor(float(D)).rsqrt() * torch.tensor(LOG2E_F32)).double()
        s2 = (raw.double() * c).masked_fill(~allowed, float('-inf'))      # the fma's exact product
        rounded = s2.float().double()
        eye = torch.eye(raw.shape[-1], dtype=torch.bool) & self_rows[:, None]
        m = rounded.amax(-1, keepdim=True)
        p = torch.exp2((torch.where(eye, rounded, s2) - m).float())
        l = p.sum(-1, keepdim=True)
        out = ((p if masks is None else p * masks.fwd) @ v) / l
        lse = (m.float() + torch.log2(l)) * LN2_F32
        ctx.save_for_backward(s2, lse * LOG2E_F32, v, out)
        ctx.masks = masks
        return out, lse.squeeze(-1)

    @staticmethod
    def backward(ctx, dout, _):
        s2, lse2, v, out = ctx.saved_tensors
        p = torch.exp2((s2 - lse2.double()).float())
        delta = (dout * out).sum(-1, keepdim=True)
        dp = dout @ v.transpose(-1, -2)
        if ctx.masks is None:
            return p * (dp - delta) / math.sqrt(v.shape[-1]), p.transpose(-1, -2) @ dout, None, None, None
        return p * (dp * ctx.masks.dp - delta) / math.sqrt(v.shape[-1]), (p * ctx.masks.dv).transpose(-1, -2) @ dout, None, None, None


Masks = namedtuple('Masks', 'fwd dv dp')      # keep / (1 - p) as [B, H, S, S] in the graph's dtype, once per use of the mask: the forward's P', the P' of dV, and dP


class _DropPV(torch.autograd.Function):
    """(P, V) -> P' V with P' = P keep / (1 - p), the backward written out, so that each of its uses of the mask can be faulted on its own:
        dV = P'^T dO,   dP = (dO V^T) keep / (1 - p);   dS = P (dP - rowsum(dP o P)) is then the softmax's own backward."""
    @staticmethod
    def forward(ctx, probs, v, masks):
        ctx.save_for_backward(probs, v)
        ctx.masks = masks
        return (probs * masks.fwd) @ v

    @staticmethod
    def backward(ctx, dout):
        probs, v = ctx.saved_tensors
        return (dout @ v.transpose(-1, -2)) * ctx.masks.dp, (probs * ctx.masks.dv).transpose(-1, -2) @ dout, None


def attention_graph(qkv, H, sep, sites=None, allowed=None, bias=None, roll=None, flash_f32=False, masks=None):
    """Dense masked attention on qkv [B, S, 3 E] in qkv's own dtype: (ctx [B, S, E], lse [B, H, S], probabilities [B, H, S, S]).  sites: the rounding hook
    (oracle.pfn_oracle._Sites; None = the plain graph).  allowed [S, S] bool, bias [S, S] added to the scores, roll = the [B, H, ...] dimension along which K and V
    are read from the next index: the planted faults.  flash_f32 (qkv in f32): softmax and lse as the exact-f32 kernels form them (_FlashF32).
    masks (Masks in qkv's dtype): dropout on the probabilities, P' = P keep / (1 - p) behind the 'P' site (the kernels zero the numerators in the accumulator and
    round what is left into the operand slots, attention.hip :447-453); lse and the returned probabilities are those of the unmasked softmax."""
    B, S, E3 = qkv.shape
    E = E3 // 3
    D = E // H
    st = O._NoSites() if sites is None else sites
    q, k, v = [t.view(B, S, H, D).transpose(1, 2) for t in st('qkv', qkv).split(E, dim=-1)]      # [B,H,S,D]
    if roll is not None:
        k, v = k.roll(-1, roll), v.roll(-1, roll)
    if flash_f32:
        out, lse = _FlashF32.apply(q @ k.transpose(-1, -2), v, visible(S, sep), torch.arange(S) >= sep, masks)
        return out.transpose(1, 2).reshape(B, S, E), lse, None
    scores = q @ k.transpose(-1, -2) / math.sqrt(D)
    if bias is not None:
        scores = scores + bias
    scores = scores.masked_fill(~(visible(S, sep, qkv.device) if allowed is None else allowed), float('-inf'))
    if masks is None:      # (the graph, hence e and every bound without dropout, as they were before the 'delta' site was found: see the site's entry)
        lse = torch.logsumexp(scores, -1)
        probs = st.softmax(scores)
        out = probs @ v
    else:
        scores = st('dS', scores)      # one rounding of all of dS: the softmax's share and the 'delta' site's, which reaches the scores through lse
        lse = torch.logsumexp(scores, -1)
        probs = st.softmax(scores, ds_site=False)
        out = st.stored_delta(_DropPV.apply(probs, v, masks), lse)
    return st('ctx', out.transpose(1, 2).reshape(B, S, E)), lse, probs


def attention_reference(qkv, H, sep, masks=None):
    """Dense masked attention in f64 with the mask of generate_D_q_matrix (transformer.py:34-41)."""
    out, lse, _ = attention_graph(qkv.double(), H, sep, masks=masks)
    return out, lse


def heads(t, H):
    """[B, S, H D] -> [B, H, S, D]"""
    B, S, E = t.shape
    return t.reshape(B, S, H, E // H).transpose(1, 2)


def hadamard(n):
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    assert h.shape[0] == n
    return h


def offset(case, b, h):
    """o_bh: n apart, so another head's or dataset's keys carry other codes, and such that sep + o_bh ends a run of n: key index sep, one past the train rows, then
    carries the cross code of the targets (sep - 2 n, sep - n + 1) of one query per slab, and admitting it shows"""
    n = head_dim(case) // 2
    return (n - 1 - case.sep) % n + n * (1 + h + case.H * b)


def targets(case, rnd):
    kind, r = rnd
    i = torch.arange(case.S)
    m = max(case.sep, 1)
    if kind == 'tail':
        first, rows = case.S // SLAB * SLAB, case.S % SLAB
        t1 = torch.where(i >= first, (i - first + rows * r) % m, (i + SLAB * (r % -(-case.sep // SLAB))) % m)
    else:
        t1 = (i + SLAB * r) % m
    if kind == 'self':
        t1 = torch.where(i >= case.sep, i, t1)
    return t1, (t1 + head_dim(case) // 2 + 1) % m


@functools.lru_cache(maxsize=8)
def _codes(case):
    """[B, H, S, D]"""
    n = head_dim(case) // 2
    hd = hadamard(n)
    j = torch.arange(case.S)
    return torch.stack([torch.stack([torch.cat([hd[(j + offset(case, b, h)) % n], hd[((j + offset(case, b, h)) // n) % n]], 1) for h in range(case.H)]) for b in range(case.B)])


def qk(case, rnd):
    """(q, k) as [B, S, E] f64"""
    c = _codes(case)
    t1, t2 = targets(case, rnd)
    flat = lambda t: t.transpose(1, 2).reshape(case.B, case.S, case.E)
    return flat(A * (c[:, :, t1] + c[:, :, t2])), flat(c)


def inputs(name, rnd, fmt):
    """(qkv [B, S, 3 E], dctx [B, S, E]) in f64, every value one of the operand type's"""
    case = CASES[name]
    q, k = qk(case, rnd)
    g = torch.Generator().manual_seed(1000 * list(CASES).index(name) + rounds(case).index(rnd))
    v, dctx = [torch.randn(case.B, case.S, case.E, generator=g).to(DTYPE[fmt]).double() for _ in range(2)]
    if case.q_begin:
        dctx[:, :case.sep] = 0      # the top encoder layer: its train rows feed nothing
    return torch.cat([q, k, v], -1), dctx


def probabilities(name, rnd, rows=None, fault=None):
    """the f64 softmax [B, H, rows, S] of a round (it depends on q and k alone, so on no format)"""
    case = CASES[name]
    q, k = qk(case, rnd)
    kw = fault_kwargs(case, fault)
    roll = kw.get('roll')
    qh, kh = heads(q, case.H), heads(k, case.H)
    if roll is not None:
        kh = kh.roll(-1, roll)
    rows = slice(None) if rows is None else rows
    scores = qh[:, :, rows] @ kh.transpose(-1, -2) / math.sqrt(head_dim(case))
    if 'bias' in kw:
        scores = scores + kw['bias'][rows]
    allowed = kw.get('allowed', visible(case.S, case.sep))
    return torch.softmax(scores.masked_fill(~allowed[rows], float('-inf')), -1)


def run(name, rnd, fmt, mode, fault=None, drop=None):
    """{ctx, dQ, dK, dV: [B, H, S, D], lse: [B, H, S], smax: the largest visible |score|} in f64.  mode 'ref': the f64 graph; 'emul': the format's emulation.
    drop = (p, site seed): dropout on the probabilities; fault is then a DropFault (or None)."""
    case = CASES[name]
    qkv, dctx = inputs(name, rnd, fmt)
    sites, kw = None, fault_kwargs(case, fault) if drop is None else {}
    if mode == 'emul':
        if fmt == 'f32':
            qkv, dctx, kw = qkv.float(), dctx.float(), dict(flash_f32=True)
        else:
            sites = O._Sites(O.Rounding(fmt), {})
    if drop is not None:
        kw['masks'] = drop_masks(case, drop, fault, qkv.dtype)
    qkv.requires_grad_(True)
    ctx, lse, probs = attention_graph(qkv, case.H, case.sep, sites, **kw)
    dqkv, = torch.autograd.grad(ctx, qkv, dctx)
    out = dict(zip(TENSORS, [heads(t.detach().double(), case.H) for t in (ctx,) + dqkv.split(case.E, -1)]))
    out['lse'] = lse.detach().double()
    q, k, _ = [heads(t.detach().double(), case.H) for t in qkv.split(case.E, -1)]
    s = (q @ k.transpose(-1, -2)).abs() / math.sqrt(head_dim(case))
    out['smax'] = s.masked_fill(~visible(case.S, case.sep), 0).max().item()
    return out


# ---- statistic and bound -----------------------------------------------------------------------------------------------------------------------------------------
def scales(name, rnd, fmt):
    """the natural scale of each tensor"""
    case = CASES[name]
    qkv, dctx = inputs(name, rnd, fmt)
    q, k, v = [t.abs().max().item() for t in qkv.split(case.E, -1)]
    d = dctx.abs().max().item()
    rd = math.sqrt(head_dim(case))
    return {'ctx': v, 'dV': d, 'dQ': d * v * k / rd, 'dK': d * v * q / rd}


def slice_errors(got, ref, scale, first=0):
    """per (b, h): (max |got - ref| over the slice's rows >= first / max(max |ref slice|, 1e-2 scale), the row of that maximum); a NaN counts as an infinite error"""
    d = torch.nan_to_num((got.double() - ref)[:, :, first:].abs(), nan=float('inf')).amax(-1)      # [B,H,rows]
    worst, row = d.max(-1)
    return worst / ref[:, :, first:].abs().amax((-1, -2)).clamp_min(1e-2 * scale), row + first


def statistic(got, ref, scale, first=0):
    return slice_errors(got, ref, scale, first)[0].max().item()


def zero_slices(ref):
    """[B, H] bool: the slices whose reference is identically zero (they must be exactly zero in the output)"""
    return ref.abs().amax((-1, -2)) == 0


def lse_error(got, ref, smax, first=0):
    return ((got.double() - ref)[:, :, first:].abs().max() / smax).item()


@functools.lru_cache(maxsize=48)
def reference(name, rnd, fmt, drop=None):
    """(the f64 reference of the round on the format's inputs, {tensor: e}, {tensor: bound}); 'lse': e and bound of the f32 graph, whatever the format.
    drop = (p, site seed): reference and emulation under the same dropout masks (lse is that of the unmasked softmax: no mask enters it)"""
    case = CASES[name]
    ref, emu, sc = run(name, rnd, fmt, 'ref', drop=drop), run(name, rnd, fmt, 'emul', drop=drop), scales(name, rnd, fmt)
    first = q_first(case)
    e = {t: statistic(emu[t], ref[t], sc[t], first if t == 'ctx' else 0) for t in TENSORS}
    bound = {t: stack_cases.bound(fmt, e[t]) for t in TENSORS}
    lse32 = emu['lse'] if fmt == 'f32' else _lse_f32(name, rnd)
    e['lse'] = lse_error(lse32, ref['lse'], ref['smax'], first)
    bound['lse'] = stack_cases.bound('f32', e['lse'])
    return ref, e, bound


@functools.lru_cache(maxsize=48)
def _lse_f32(name, rnd):
    """lse of the graph in f32: q and k are the same in every format"""
    case = CASES[name]
    qkv, _ = inputs(name, rnd, 'f32')
    return attention_graph(qkv.float(), case.H, case.sep, flash_f32=True)[1].double()


# ---- planted faults (CPU only, applied to the f64 reference) ---------------------------------------------------------------------------------------------------------
Fault = namedtuple('Fault', 'cls label kind rows keys')
KEY_CLASSES = ('key removed for one slab', 'self key removed for one slab', 'self key added twice', 'last partial tile removed', 'key index sep admitted')
CLASSES = KEY_CLASSES + ('K/V of head h + 1', 'K/V of dataset b + 1')


def fault_kwargs(case, fault):
    if fault is None:
        return {}
    if fault.kind == 'roll':
        return dict(roll=fault.keys)
    S = case.S
    lo, hi = fault.rows
    if fault.kind == 'twice':      # the self key counted twice: its numerator doubles
        bias = torch.zeros(S, S, dtype=torch.float64)
        i = torch.arange(lo, hi)
        bias[i, i] = math.log(2.0)
        return dict(bias=bias)
    allowed = visible(S, case.sep)
    if fault.kind == 'self':
        i = torch.arange(lo, hi)
        allowed[i, i] = False
    else:
        allowed[lo:hi, fault.keys[0]:fault.keys[1]] = fault.kind == 'admit'
    i = (~allowed.any(1)).nonzero().flatten()      # (a row never loses its only key: sep = 1)
    allowed[i, i] = True
    return dict(allowed=allowed)


@functools.lru_cache(maxsize=None)
def targeting_slabs(name, keys):
    """{key: the 32-query slabs, among the rows the launch writes, with a query that has p_key >= 1/16 in some round}"""
    case = CASES[name]
    nslab = -(-case.S // SLAB)
    hit = torch.zeros(nslab, len(keys), dtype=torch.bool)
    for rnd in rounds(case):
        first = case.S // SLAB * SLAB if rnd[0] == 'tail' else 0      # (a 'tail' round is new in the ragged slab alone)
        big = torch.zeros(case.S, len(keys), dtype=torch.bool)
        big[first:] = (probabilities(name, rnd, slice(first, None))[..., list(keys)] >= 1 / 16).any(0).any(0)
        big[:q_first(case)] = False
        for s in range(nslab):
            hit[s] |= big[SLAB * s:SLAB * s + SLAB].any(0)
    return {j: hit[:, c].nonzero().flatten().tolist() for c, j in enumerate(keys)}


def planted_faults(name, fmt):
    """(a launch from q_begin writes the rows from q_first on, and its d(ctx) is zero on the train rows: its faults sit on the rows it writes, and the self key of
    a train row, whose gradient is zero there, is left to the full launch of the same shape)"""
    case = CASES[name]
    S, sep, q0 = case.S, case.sep, q_first(case)
    last = (S - 1) // SLAB
    slab = lambda s: (max(SLAB * s, q0), min(SLAB * s + SLAB, S))
    out = []
    if sep > 0:
        keys = tuple(dict.fromkeys([0, sep - 1, (sep - 1) // 64 * 64, (sep - 1) // 32 * 32]))
        for j, slabs in targeting_slabs(name, keys).items():
            for s in dict.fromkeys(slabs[:1] + slabs[-1:]):      # the first and the last slab that targets it
                out.append(Fault(CLASSES[0], f'key {j} removed for queries {slab(s)[0]}..{slab(s)[1] - 1}', 'drop', slab(s), (j, j + 1)))
        out.append(Fault(CLASSES[1], f'self key removed for test rows {max(sep, slab(last)[0])}..{S - 1}', 'self', (max(sep, slab(last)[0]), S), None))
        if not case.q_begin and sep > 1:      # (the only key of its row, counted twice, is still everything)
            out.append(Fault(CLASSES[2], f'self key twice for train rows 0..{min(SLAB, sep) - 1}', 'twice', (0, min(SLAB, sep)), None))
        t0 = (sep - 1) // kv_tile(case, fmt) * kv_tile(case, fmt)
        out.append(Fault(CLASSES[3], f'keys {t0}..{sep - 1} removed for every query', 'drop', (q0, S), (t0, sep)))
    if q0 < sep or not case.q_begin:      # (of the rows a launch from q_begin = sep = q_first writes, only row sep itself chooses the code of key sep)
        out.append(Fault(CLASSES[4], f'key {sep} admitted for every query', 'admit', (q0, S), (sep, sep + 1)))
    if case.H > 1:
        out.append(Fault(CLASSES[5], 'K/V of head h + 1', 'roll', None, 1))
    if case.B > 1:
        out.append(Fault(CLASSES[6], 'K/V of dataset b + 1', 'roll', None, 0))
    return out


def fault_rounds(name, fault):
    """per kind of round, the one in which the fault moves a probability most (if it moves one at all): the suite runs every round, so a fault shows on a tensor
    if one round shows it there"""
    case, best = CASES[name], {}
    lo, hi = (0, case.S) if fault.rows is None else fault.rows
    if case.q_begin and max(lo, case.sep) < hi:      # (the gradients of such a launch come from the test rows alone)
        lo = max(lo, case.sep)
    for rnd in rounds(case):
        if rnd[0] == 'tail' and lo < case.S // SLAB * SLAB:      # (a 'tail' round is new in the ragged slab alone: it is for the faults planted there)
            continue
        rows = slice(lo, hi)
        d = (probabilities(name, rnd, rows, fault) - probabilities(name, rnd, rows)).abs().max().item()
        if d > best.get(rnd[0], (None, -1.0 if fault.kind == 'roll' else 1e-3))[1]:      # (other K and V show through V even where no probability moves: sep = 0)
            best[rnd[0]] = (rnd, d)
    return [rnd for rnd, _ in best.values()]


def fault_multiples(name, fmt, fault):
    """{tensor: the statistic of the faulted f64 reference against the right one / the bound the GPU test asserts}, the largest over fault_rounds, and those rounds"""
    first = q_first(CASES[name])
    out = dict.fromkeys(TENSORS, 0.0)
    for rnd in fault_rounds(name, fault):
        ref, _, bound = reference(name, rnd, fmt)
        bad, sc = run(name, rnd, fmt, 'ref', fault), scales(name, rnd, fmt)
        for t in TENSORS:
            out[t] = max(out[t], statistic(bad[t], ref[t], sc[t], first if t == 'ctx' else 0) / bound[t])
    return fault_rounds(name, fault), out


# ---- dropout on the probabilities (attn_fwd_kernel / attn_bwd_kv_kernel / attn_bwd_dq_kernel <DROP = true>, the `drop` branches of attn_bwd_plain_*) ----------------
# The mask is never stored: every pass regenerates keep(pair seed, query, key) from indices, in its own register layout.  The planted keys make one key worth
# 1/16 .. 1 of a row, so one wrong mask bit on a targeted key moves ctx, dV, and through dS dQ and dK, by a sizeable part of their scale.
DROP_CASES = ('S100-sep70', 'S333-sep301', 'S300-sep257', 'S520-sep512', 'S300-sep200-D256', 'S200-sep1', 'S130-sep0')      # (no q_begin: the stack never combines it with live dropout)
# (p, site seed = what dropout_site_seed(call seed, layer, 0) yields); the second seed has its top bit set.  Each seed is the first from 12345 / 0x9E3779B9 upwards
# that meets drop_coverage_gaps on every case: S130-sep0 has one round and a ragged last slab of two queries, of which one must keep its self key and the other lose
# it in each of the four (dataset, head) pairs -- 1 seed in 100 at p = 0.2 (12345 and 0x9E3779B9 themselves meet the condition everywhere else)
DROP_PAIRS = ((0.2, 12523), (0.5, 0x9E3779C8))
MASK_TILE = 64


def residue_tensors(name, drop):
    """the tensors whose exact zero in the reference the kernels do NOT return exactly: without train rows dQ and dK are zero, and launch_attn_bwd sends such a batch
    through the self-only kernel only without dropout (attention.hip launch_attn_bwd); under dropout the general query-block pass runs, and its
    dS = P (dP - delta), delta from the stored output, is ~2^-24 |dP|: held to the bound on the floored scale instead"""
    return ('dQ', 'dK') if drop is not None and CASES[name].sep == 0 else ()


def keep_scale(p):
    """1 / (1 - p) with p as the kernels see it (float32)"""
    return 1.0 / (1.0 - torch.tensor(p, dtype=torch.float32).item())


@functools.lru_cache(maxsize=None)
def keep_masks(case, site_seed, p):
    """[B, H, S, S] bool: keep(query i, key j) of every (dataset, head), the integers of pfn_kernels.h dropout_pair_seed / dropout_keep"""
    r = range(case.S)
    return torch.stack([torch.stack([O.dropout_keep_mask(O.dropout_pair_seed(site_seed, b * case.H + h), r, r, p) for h in range(case.H)]) for b in range(case.B)])


DropFault = namedtuple('DropFault', 'cls label kind arg')
MASK_CLASSES = ('mask of key j + 1', 'key index modulo 256', 'query index modulo 256', 'mask of head h + 1', 'mask of dataset b + 1', 'self key unmasked')
BACKWARD_CLASSES = ('keep transposed in the backward', 'dV from the unmasked P', 'dP without keep', 'dP without 1 / (1 - p)')
FORWARD_CLASSES = ('ctx without 1 / (1 - p)',)


def faulted_keep(case, keep, fault):
    S, out = case.S, keep.clone()
    if fault.kind == 'shift':      # the mask of key j + 1 for key j, inside one tile of 64 keys, for the queries of one slab
        (lo, hi), t0 = fault.arg
        j = torch.arange(t0, min(t0 + MASK_TILE, S - 1))
        out[:, :, lo:hi, j] = keep[:, :, lo:hi, j + 1]
    elif fault.kind == 'keymod':
        out[..., 256:] = keep[..., torch.arange(256, S) % 256]
    elif fault.kind == 'querymod':
        out[:, :, 256:] = keep[:, :, torch.arange(256, S) % 256]
    elif fault.kind == 'roll':
        out = keep.roll(-1, fault.arg)
    elif fault.kind == 'self':
        i = torch.arange(case.sep, S)
        out[:, :, i, i] = True
    elif fault.kind == 'transpose':
        out = keep.transpose(-1, -2)
    elif fault.kind == 'unmasked':
        out[:] = True
    return out


@functools.lru_cache(maxsize=6)
def _plain_masks(case, drop, dtype):
    m = keep_masks(case, drop[1], drop[0]).to(dtype) * keep_scale(drop[0])
    return Masks(m, m, m)


def drop_masks(case, drop, fault=None, dtype=torch.float64):
    """Masks of a (p, site seed) pair; fault (a DropFault): a mask fault goes into all three uses, a backward-only one into dV and / or dP, the forward-only one into ctx"""
    plain = _plain_masks(case, drop, dtype)
    if fault is None:
        return plain
    p, seed = drop
    keep, scale = keep_masks(case, seed, p), keep_scale(p)
    uses = {'transpose': ('dv', 'dp'), 'unmasked': (fault.arg,), 'unscaled': (fault.arg,)}.get(fault.kind, Masks._fields)
    bad = (keep if fault.kind == 'unscaled' else faulted_keep(case, keep, fault)).to(dtype) * (1.0 if fault.kind == 'unscaled' else scale)
    return Masks(*[bad if f in uses else getattr(plain, f) for f in Masks._fields])


def drop_faults(name):
    """(the same in every format: the mask knows no format).  Left out where the arithmetic cannot show them: an index taken modulo 256 needs a visible key or a
    query >= 256; without train rows only keep(i, i) is ever used, which a transposed mask leaves alone, and a row with one visible key has dS = 0 whatever dP is"""
    case = CASES[name]
    S, sep = case.S, case.sep
    full = S // SLAB - 1                                    # the last full slab
    slab = lambda s: (SLAB * s, SLAB * s + SLAB)
    t_last = ((sep - 1) if sep else SLAB * full) // MASK_TILE * MASK_TILE      # the tile of the last train key (without train rows: of the slab's self keys)
    out = [DropFault(MASK_CLASSES[0], f'mask of key j + 1 for keys 0..{MASK_TILE - 1}, queries 0..{SLAB - 1}', 'shift', (slab(0), 0)),
           DropFault(MASK_CLASSES[0], f'mask of key j + 1 for keys {t_last}..{t_last + MASK_TILE - 1}, queries {slab(full)[0]}..{slab(full)[1] - 1}', 'shift', (slab(full), t_last))]
    if S > 256:
        out.append(DropFault(MASK_CLASSES[1], 'key index modulo 256', 'keymod', None))
        out.append(DropFault(MASK_CLASSES[2], 'query index modulo 256', 'querymod', None))
    if case.H > 1:
        out.append(DropFault(MASK_CLASSES[3], 'mask of head h + 1', 'roll', 1))
    if case.B > 1:
        out.append(DropFault(MASK_CLASSES[4], 'mask of dataset b + 1', 'roll', 0))
    out.append(DropFault(MASK_CLASSES[5], f'self key of test rows {sep}..{S - 1} unmasked', 'self', None))
    if sep > 0:
        out.append(DropFault(BACKWARD_CLASSES[0], 'keep transposed in dV and dP', 'transpose', None))
    out.append(DropFault(BACKWARD_CLASSES[1], 'dV from the unmasked P', 'unmasked', 'dv'))
    if sep > 0:
        out.append(DropFault(BACKWARD_CLASSES[2], 'dP without keep', 'unmasked', 'dp'))
        out.append(DropFault(BACKWARD_CLASSES[3], 'dP without 1 / (1 - p)', 'unscaled', 'dp'))
    out.append(DropFault(FORWARD_CLASSES[0], 'ctx without 1 / (1 - p)', 'unscaled', 'fwd'))
    return out


@functools.lru_cache(maxsize=None)
def drop_fault_rounds(name, drop):
    """{fault label: per kind of round, the one in which the fault moves a masked probability P keep / (1 - p) most}: one pass over the rounds for all the faults of
    a case (the suite runs every round, so a fault shows on a tensor if one round shows it there)"""
    case = CASES[name]
    plain = drop_masks(case, drop)
    diffs = {}
    for f in drop_faults(name):
        bad = drop_masks(case, drop, f)
        diffs[f.label] = torch.stack([(getattr(bad, u) - getattr(plain, u)).abs() for u in Masks._fields]).amax(0)
    best = {label: {} for label in diffs}
    for rnd in rounds(case):
        p = probabilities(name, rnd)
        for label, d in diffs.items():
            moved = (p * d).max().item()
            if moved > best[label].get(rnd[0], (None, 1e-3))[1]:
                best[label][rnd[0]] = (rnd, moved)
    return {label: [rnd for rnd, _ in b.values()] for label, b in best.items()}


def drop_fault_multiples(name, fmt, drop, fault):
    """{tensor: the statistic of the faulted f64 reference against the right one / the bound the GPU test asserts}, the largest over drop_fault_rounds, and those rounds"""
    rnds = drop_fault_rounds(name, drop)[fault.label]
    out = dict.fromkeys(TENSORS, 0.0)
    for rnd in rnds:
        ref, _, bound = reference(name, rnd, fmt, drop)
        bad, sc = run(name, rnd, fmt, 'ref', fault, drop), scales(name, rnd, fmt)
        for t in TENSORS:
            out[t] = max(out[t], statistic(bad[t], ref[t], sc[t]) / bound[t])
    return rnds, out


def drop_coverage_gaps(name, drop):
    """What the masks of a (p, site seed) pair leave untested on a case, in words (empty: nothing).  A targeted key is one with p >= 1/16 in the unmasked softmax.
    In every round, every (dataset, head) and every full 32-query slab some query must keep a targeted key and some query must lose one; the ragged last slab
    must do both over the rounds of the case taken together."""
    case = CASES[name]
    keep = keep_masks(case, drop[1], drop[0])
    full = case.S // SLAB
    gaps, tail = [], torch.zeros(2, case.B, case.H, dtype=torch.bool)
    for rnd in rounds(case):
        big = probabilities(name, rnd) >= 1 / 16
        both = torch.stack([(big & keep).any(-1), (big & ~keep).any(-1)])      # [2, B, H, S]: the query keeps / loses a targeted key
        slabs = both[..., :full * SLAB].reshape(2, case.B, case.H, full, SLAB).any(-1)
        for w, b, h, s in (~slabs).nonzero().tolist():
            gaps.append(f'round {rnd[0]} {rnd[1]}, dataset {b}, head {h}, slab {s}: no query {("keeps", "loses")[w]} a targeted key')
        tail |= both[..., full * SLAB:].any(-1)
    if case.S % SLAB:
        gaps += [f'dataset {b}, head {h}, the ragged last slab: no query {("keeps", "loses")[w]} a targeted key in any round' for w, b, h in (~tail).nonzero().tolist()]
    return gaps
