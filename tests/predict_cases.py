"""What tests/test_host_predict_rows.py (CPU) and tests/test_gpu_predict_rows.py (MI355X) share: the case matrix of the per-test-row inference suite (condition /
predict, their ragged and chunked forms, the saved pass with its input gradient, the model.eval() forward), its models and inputs, the oracle runs (f64, f32 and
operand-rounded: oracle/pfn_oracle.py Rounding) cached per (case, format), the statistics, the planted faults and a Python restatement of the key-split arithmetic.

Statistics, per dataset b, on logits [n, B, n_out] and on dx [n, B, F]:
    worst row : max over t of |got[t, b] - want[t, b]|_2 / sqrt(mean over t of |want[t, b]|_2^2)   (the dataset's rms row norm: a small row cannot inflate it)
    rel l2    : |got[:, b] - want[:, b]| / |want[:, b]|
A case's value is the largest over its datasets.  Bound rule: stack_cases.bound(fmt, e), e = the same statistic of the operand-rounded f64 oracle (16 bit) or of the
oracle run in f32, against the plain f64 oracle -- from the reference only, never from a GPU figure.

The plan of the pass (transformerscandobayesianinference_amd/csrc/pfn_api.hip):
  * stack_predict_impl :942 runs the forward's schedule with make_plan(..., M = B n, 0.f) :987 on the test rows, layer by layer against the cached keys: its logits
    are pfn_oracle.forward on cat(train, test) at sep (a test row sees the train keys and itself).  No forward value depends on top_rows.
  * stack_predict_backward_impl :1055: the top layer's LayerNorm backward reads f32 rows (launch_scatter_test_rows -> gA, PFN_PREC_F32 :1088; view(): top -> gA
    :1094) -- Rounding(top_rows=True); d(src) leaves layer 0 in operand precision when predict_dsrc_is_t :371 :1098 :1117 -- the 'emb_grad' site, plan['emb_t'] =
    nlayers > 0; fuse_lnb = lnbwd_fusable(...) at M = B n :1097 -- gemm_lnbwd_supported (gemm.hip :1638) asks N = E in {128, 256, 512, 1024}, K = nhid and 3 E a
    multiple of 32, and 16-byte alignment of operands that carve_predict_grad aligns to 256 (take :279): nothing in it depends on M or on anything the oracle cannot see, so
    plan['fuse_lnb'] holds as Rounding.plan restates it (PREDICT_BACKWARD_FORM below, pinned by the CPU test).  fp16: the chain runs on dlogits 2^k, k from the
    largest |dlogits| of the call (launch_absmax :1075).
  * the partial (o, m, l) of a key split and the partial dQ are f32 (pfn_kernels.h :191-192 :228; attention.hip :466 :474 :676): no rounding site of their own.
"""
import math
from collections import namedtuple

import torch

import stack_cases
from oracle import pfn_oracle as O
from transformerscandobayesianinference_amd import bar_distribution, encoders
from transformerscandobayesianinference_amd.transformer import TransformerModel

F, NBARS, L = 5, 100, 2
SCALE = 2.0      # rows [0, 2E) of every in_proj_weight: with unscaled random weights the softmax is almost flat and a missing key moves a row by less than fp16 rounding
# a case whose bf16 bound misses a planted fault of >= 32 keys at scale 2 (tests/test_host_predict_rows.py) has its own scale, chosen on the CPU from the f64 oracle
# and its emulations alone: the smallest such multiple is then 1.2 (A), 1.4 (F), 1.3 (G), 1.3 (R2) and the emulated errors stay inside the window of the format (G and R2 at 3: their bf16 dx
# worst row reaches 2.1e-2)
CASE_SCALE = {'A': 3.0, 'F': 3.0, 'G': 2.5, 'R2': 2.5}
FORMATS = ('f32', 'fp16', 'bf16')

Case = namedtuple('Case', 'name E H sep n B')      # sep: the eval position, or a tuple of per-dataset train lengths (ragged: B = its length)
CASES = {c.name: c for c in [
    Case('A', 128, 4, 437, 7, 3),         # D 32, one key tile per split (14 splits f32, 7 in 16 bit), partial last tile
    Case('B', 128, 2, 0, 7, 3),           # no train rows, the self key alone
    Case('C', 128, 2, 1, 129, 1),         # one cached key; f32: a second query block of one row
    Case('D', 256, 2, 65, 257, 2),        # D 128; 16 bit: a second query block of one row; one key past a tile edge in every format
    Case('E', 256, 1, 129, 33, 2),        # D 256, two V slices in f32; a last tile of one key
    Case('F', 128, 4, 437, 300, 8),       # 2400 rows; f32: 5 splits of three tiles, the last of 53 keys
    Case('G', 128, 4, 437, 7, 24),        # 16-bit splits of two 64-key tiles, four splits where five were asked for, the last split one partial tile
    Case('H', 512, 4, 63, 40, 3),         # sep one key short of a tile; an fp16 model under eval_precision 'f32' and 'same'
    Case('I', 1024, 4, 63, 7, 3),         # fp16: the y16u sums ahead of a separate LayerNorm
    Case('J', 64, 2, 63, 7, 3),           # bf16: a width no fused kernel takes
    Case('R1', 128, 4, (437, 0, 64, 33, 1), 7, 5),
    Case('R2', 256, 2, (437, 0, 64, 65, 1), 7, 5),
    Case('R3', 256, 1, (63, 200, 0), 33, 3),
]}

Run = namedtuple('Run', 'case precision eval_precision cap')      # precision: the model's; eval_precision 'same' or 'f32'; cap: PFN_TUNE_ATTN_CACHE_SPLITS (0 = the rule)


def fmt_of(run):
    return run.precision if run.eval_precision == 'same' else run.eval_precision


def run_id(run):
    return f'{run.case}-{run.precision}' + ('' if run.eval_precision == 'same' else f'-eval_{run.eval_precision}') + (f'-cap{run.cap}' if run.cap else '')


def _runs(names, formats=FORMATS):
    return [Run(c, f, 'same', 0) for c in names for f in formats]


H_RUNS = [Run('H', 'fp16', 'f32', 0), Run('H', 'fp16', 'same', 0)]
PREDICT = (_runs('A') + [Run('A', 'f32', 'same', 1)] + _runs('BCDEF') + _runs('G', ('fp16', 'bf16')) + H_RUNS + [Run('I', 'fp16', 'same', 0), Run('J', 'bf16', 'same', 0)])
RAGGED = [Run('R1', 'f32', 'same', 0), Run('R2', 'fp16', 'same', 0), Run('R2', 'bf16', 'same', 0), Run('R3', 'f32', 'same', 0)]
CHUNKED = [Run('F', 'f32', 'same', 0), Run('F', 'fp16', 'same', 0)]
CHUNK_ROWS = 37                            # rows per dataset and chunk: TransformerModel._PREDICT_ROWS = 37 B
FORWARD = _runs('ADE') + H_RUNS
DX = (_runs('A') + [Run('A', 'f32', 'same', 1)] + _runs('CDE') + _runs('G', ('fp16', 'bf16')) + [Run('R1', 'f32', 'same', 0), Run('R2', 'fp16', 'same', 0),
                                                                                                 Run('R2', 'bf16', 'same', 0)])
DX_CASES = sorted({r.case for r in DX})
ALL_RUNS = PREDICT + RAGGED
CASE_FORMATS = {name: sorted({fmt_of(r) for r in ALL_RUNS if r.case == name}) for name in CASES}

# (E, nhid, schedule) -> the form of the predict backward: fuse_lnb as lnbwd_fusable decides it (pfn_api.hip :531-534 through lnb_eligible :360 -- width_ok :353 is
# E <= 512 under the default schedule -- and gemm_lnbwd_supported gemm.hip :1638-1641), emb_t = predict_dsrc_is_t :371, top_rows: always (:1088 :1094)
PREDICT_BACKWARD_FORM = {
    (64, 128, 0): dict(fuse_lnb=False, emb_t=True, top_rows=True),        # N = 64: no fused LayerNorm-backward kernel
    (128, 256, 0): dict(fuse_lnb=True, emb_t=True, top_rows=True),
    (256, 512, 0): dict(fuse_lnb=True, emb_t=True, top_rows=True),
    (512, 1024, 0): dict(fuse_lnb=True, emb_t=True, top_rows=True),
    (1024, 2048, 0): dict(fuse_lnb=False, emb_t=True, top_rows=True),     # width_ok fails without PFN_SCHED_FUSE_LN_WIDE
    (128, 256, O.SCHED_DETERMINISTIC): dict(fuse_lnb=False, emb_t=True, top_rows=True),
    (128, 256, O.SCHED_SEPARATE_LNBWD): dict(fuse_lnb=False, emb_t=True, top_rows=True),
}


def rounding(fmt, schedule=0):
    return O.Rounding(fmt, schedule, top_rows=True)


def lengths_of(case):
    return tuple(case.sep) if isinstance(case.sep, tuple) else (case.sep,) * case.B


def sep_max(case):
    return max(lengths_of(case))


# ---- models and inputs (test_gpu_predict.make / data, on the CPU, the in-projection scaled before anything moves to the device) -------------------------------------------
def make_model(case, precision='f32', eval_precision='same', scale=None):
    scale = CASE_SCALE.get(case.name, SCALE) if scale is None else scale
    torch.manual_seed(0)
    m = TransformerModel(encoders.Linear(F, case.E), NBARS, case.E, case.H, 2 * case.E, L, 0.0, y_encoder=encoders.Linear(1, case.E), precision=precision,
                         eval_precision=precision if eval_precision == 'same' else eval_precision)
    m.criterion = bar_distribution.FullSupportBarDistribution(torch.sort(torch.randn(NBARS + 1) * 1.5)[0])
    with torch.no_grad():
        for layer in m.transformer_encoder.layers:
            for t in (layer.linear2.weight, layer.self_attn.out_proj.weight):      # un-zero the residual branches
                t.normal_(0, 0.03)
            layer.self_attn.in_proj_weight[:2 * case.E] *= scale
    return m.eval()


def make_data(case, seed=1):
    """x [sep_max + n, B, F], y [sep_max + n, B] (ragged: the rows behind a dataset's own are whatever the generator drew -- they must not matter)"""
    g = torch.Generator().manual_seed(seed)
    t = sep_max(case) + case.n
    return torch.randn(t, case.B, F, generator=g), torch.randn(t, case.B, generator=g)


def cotangent(case):
    return torch.randn(case.n, case.B, NBARS, generator=torch.Generator().manual_seed(7))


_params = {}


def params_of(case):
    if case.name not in _params:
        _params[case.name] = {k: v.detach().clone() for k, v in make_model(case).state_dict().items() if not k.startswith('criterion.')}
    return _params[case.name]


# ---- the key-split arithmetic of the cached attention, restated (csrc/attention.hip attn_cache_splits :1835-1846, launch_fwd_cache_t :1696-1704) -------------------------
def tiles(fmt, D):
    """(query block, key tile, V slices) of AttnCfg<T, D> / attn_cache_splits"""
    small = fmt != 'f32' and D <= 128
    return (256 if small else 128), (64 if small else 32), (2 if fmt == 'f32' and D == 256 else 1)


def attn_cache_splits(B, n, E, H, sep, fmt):
    qblk, kvb, slices = tiles(fmt, E // H)
    wgs = -(-n // qblk) * H * B * slices
    if wgs >= 256:
        return 1
    return max(1, min(512 // wgs, -(-sep // kvb)))


def split_state(case, fmt, cap=0, n=None, backward=False):
    """what launch_fwd_cache_t launches for this case (ragged: on sep_max keys; a dataset's own count clamps inside the kernel); backward: launch_bwd_cache_t
    :1860-1868 -- the forward's split count and query blocks, but key tiles of BwdCacheCfg::KVB = 32 in every format (:537), so a 16-bit pass may cut elsewhere"""
    n = case.n if n is None else n
    sep = sep_max(case)
    qblk, kvb, slices = tiles(fmt, case.E // case.H)
    asked = attn_cache_splits(case.B, n, case.E, case.H, sep, fmt)
    if backward:
        kvb = 32
    nsplit = min(asked, cap) if cap > 0 else asked
    ntiles = -(-sep // kvb)
    split_keys = -(-ntiles // nsplit) * kvb if nsplit > 1 else max(sep, 1)
    nz = -(-sep // split_keys) if nsplit > 1 else 1
    return dict(asked=asked, splits=nz, split_keys=split_keys, keys_last_split=sep - (nz - 1) * split_keys, keys_last_tile=(sep - 1) % kvb + 1 if sep else 0,
                qblocks=-(-n // qblk), rows_last_block=(n - 1) % qblk + 1, qblk=qblk, kvb=kvb, slices=slices)


# the states the cases are in the matrix for: (case, format) -> the entries of split_state that must hold (tests/test_host_predict_rows.py asserts them)
STATES = {
    ('A', 'f32'): dict(splits=14, split_keys=32, keys_last_split=21, qblocks=1), ('A', 'fp16'): dict(splits=7, split_keys=64, keys_last_split=53),
    ('A', 'bf16'): dict(splits=7, split_keys=64, keys_last_split=53),
    ('B', 'f32'): dict(splits=1, keys_last_split=0), ('B', 'fp16'): dict(splits=1, keys_last_split=0),
    ('C', 'f32'): dict(splits=1, keys_last_split=1, qblocks=2, rows_last_block=1), ('C', 'fp16'): dict(splits=1, keys_last_split=1, qblocks=1),
    ('D', 'f32'): dict(splits=3, keys_last_split=1, keys_last_tile=1, qblocks=3, rows_last_block=1),
    ('D', 'fp16'): dict(splits=2, split_keys=64, keys_last_split=1, keys_last_tile=1, qblocks=2, rows_last_block=1),
    ('D', 'bf16'): dict(splits=2, split_keys=64, keys_last_split=1, keys_last_tile=1, qblocks=2, rows_last_block=1),
    ('E', 'f32'): dict(slices=2, splits=5, keys_last_split=1, keys_last_tile=1, kvb=32, qblk=128), ('E', 'fp16'): dict(slices=1, splits=5, keys_last_tile=1, kvb=32, qblk=128),
    ('F', 'f32'): dict(asked=5, splits=5, split_keys=96, keys_last_split=53, qblocks=3, rows_last_block=44),
    ('F', 'fp16'): dict(asked=7, splits=7, split_keys=64, keys_last_split=53, qblocks=2, rows_last_block=44),
    ('G', 'fp16'): dict(asked=5, splits=4, split_keys=128, keys_last_split=53), ('G', 'bf16'): dict(asked=5, splits=4, split_keys=128, keys_last_split=53),
    ('H', 'fp16'): dict(kvb=64, keys_last_tile=63, splits=1), ('H', 'f32'): dict(kvb=32, keys_last_tile=31, splits=2),
    ('R1', 'f32'): dict(splits=14, split_keys=32), ('R2', 'fp16'): dict(splits=7, split_keys=64), ('R3', 'f32'): dict(slices=2, splits=7, keys_last_tile=8),
}


def where(case, fmt, cap, t, b, backward=False):
    """which query block, and which key tile of its last split, test row t of dataset b sits in -- for a failure message"""
    st = split_state(case, fmt, cap, backward=backward)
    keys = lengths_of(case)[b]
    return (f'query block {t // st["qblk"]} of {st["qblocks"]} (row {t % st["qblk"]} of it), {keys} cached keys in {st["splits"]} split(s) of {st["split_keys"]}, '
            f'last key tile holds {(keys - 1) % st["kvb"] + 1 if keys else 0} of {st["kvb"]} keys')


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------------------------------------
def row_stats(got, want):
    """{'worst row': (value, b, t), 'rel l2': (value, b)} of got against want, both [n, B, W]; datasets whose `want` is identically zero are left out (zero_datasets)"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    err, ref = (got - want).norm(dim=-1), want.norm(dim=-1)      # [n, B]
    worst, rel = (0.0, -1, -1), (0.0, -1)
    for b in range(want.shape[1]):
        if ref[:, b].max() == 0:
            continue
        per = err[:, b] / (ref[:, b] ** 2).mean().sqrt()
        t = int(per.argmax())
        worst = max(worst, (per[t].item(), b, t))
        rel = max(rel, ((err[:, b].norm() / ref[:, b].norm()).item(), b))
    return {'worst row': worst, 'rel l2': rel}


def zero_datasets(want):
    return [b for b in range(want.shape[1]) if want[:, b].abs().max() == 0]


def rms_row_norm(want, b):
    return (want[:, b].double().norm(dim=-1) ** 2).mean().sqrt().item()


# ---- oracle runs, cached ------------------------------------------------------------------------------------------------------------------------------------------------
def loss_scale_exp(R):
    """fp16: the backward runs on dlogits 2^k with the largest |dlogits| 2^k in [4, 8) (pfn_oracle.loss_and_grads; pfn_device.h loss_scale_exp)"""
    amax = R.abs().max().item()
    return 2 - math.floor(math.log2(amax)) if 0 < amax < float('inf') else 0


def oracle_columns(params, H, x, y, sep, R, fmt, want_dx, k=0, schedule=0):
    """(logits [n, b, n_out], dx [n, b, F] or None) in f64 of pfn_oracle.forward on x [sep + n, b, F] at sep: fmt None = f64, 'f32' = the oracle in f32,
    'bf16' / 'fp16' = the operand-rounded f64 oracle under the plan of the predict pass; dx = d((logits . R).sum()) / d(test rows of x)"""
    kw, dtype = {}, torch.float64
    if fmt == 'f32':
        kw['dtype'] = dtype = torch.float32
    elif fmt is not None:
        kw['rounding'] = rounding(fmt, schedule)
    xo = x.to(dtype).clone().requires_grad_(want_dx)
    with torch.set_grad_enabled(want_dx):
        lo = O.forward(params, xo, y, sep, H, **kw)
    if not want_dx:
        return lo.detach().double(), None
    scale = 2.0 ** k if fmt == 'fp16' else 1.0
    dx, = torch.autograd.grad((lo * R.to(dtype)).sum() * scale, xo)
    return lo.detach().double(), (dx[sep:] / scale).double()


_cache = {}


def oracle(case, fmt=None, want_dx=False):
    """the case's (logits [n, B, n_out], dx [n, B, F] or None); ragged: every dataset alone on its own first `length` rows followed by its test rows"""
    key = (case.name, fmt)
    if key in _cache and (_cache[key][1] is not None or not want_dx):
        return _cache[key]
    params, (x, y), R = params_of(case), make_data(case), cotangent(case)
    k = loss_scale_exp(R)
    if not isinstance(case.sep, tuple):
        out = oracle_columns(params, case.H, x, y, case.sep, R, fmt, want_dx, k)
    else:
        top, cols = sep_max(case), []
        for b, length in enumerate(case.sep):
            xs, ys = torch.cat([x[:length, b:b + 1], x[top:, b:b + 1]]), torch.cat([y[:length, b:b + 1], y[top:, b:b + 1]])
            cols.append(oracle_columns(params, case.H, xs, ys, length, R[:, b:b + 1], fmt, want_dx, k))
        out = (torch.cat([c[0] for c in cols], 1), torch.cat([c[1] for c in cols], 1) if want_dx else None)
    _cache[key] = out
    return out


def emulated(case, fmt, want_dx=False):
    """{(tensor, statistic): e}: the statistics of the format's emulation against the plain f64 oracle, the largest over the datasets"""
    lo, dxo = oracle(case, None, want_dx)
    le, dxe = oracle(case, fmt, want_dx)
    e = {('logits', k): v[0] for k, v in row_stats(le, lo).items()}
    if want_dx:
        e.update({('dx', k): v[0] for k, v in row_stats(dxe, dxo).items()})
    return e


def bounds(case, fmt, want_dx=False):
    return {k: stack_cases.bound(fmt, v) for k, v in emulated(case, fmt, want_dx).items()}


# ---- planted faults: the f64 oracle on dataset b alone with a few of its test rows (test rows do not see each other), its mask or its train rows wrong ---------------
class _masked:
    """pfn_oracle.d_q_mask wrapped for the duration of a block: every test row additionally loses the keys `drop(sep)` (a list of key indices; 'self' = its own)"""

    def __init__(self, drop):
        self.drop = drop

    def __enter__(self):
        self.plain = O.d_q_mask
        def wrapped(T, sep, dtype, device):
            m = self.plain(T, sep, dtype, device)
            if self.drop == 'self':
                idx = torch.arange(sep, T)
                m[idx, idx] = float('-inf')
            elif len(self.drop):
                m[sep:, torch.as_tensor(self.drop)] = float('-inf')
            return m
        O.d_q_mask = wrapped

    def __exit__(self, *exc):
        O.d_q_mask = self.plain


_fault_cache = {}


def faulted(case, b, rows, drop=(), train_from=None, train_len=None, want_dx=False):
    """(logits [len(rows), n_out], dx [len(rows), F] or None) of test rows `rows` of dataset b under a planted fault: the keys `drop` missing ('self': a row's own
    key), the train rows of dataset `train_from` in place of its own, or `train_len` train rows in place of its own count"""
    key = (case.name, b, tuple(rows), drop if drop == 'self' else tuple(drop), train_from, train_len, want_dx)
    if key not in _fault_cache:
        x, y = make_data(case)
        length, top = lengths_of(case)[b] if train_len is None else train_len, sep_max(case)
        src = b if train_from is None else train_from
        rows_t = torch.as_tensor(rows) + top
        xs, ys = torch.cat([x[:length, src], x[rows_t, b]]).unsqueeze(1), torch.cat([y[:length, src], y[rows_t, b]]).unsqueeze(1)
        R = cotangent(case)[torch.as_tensor(rows), b].unsqueeze(1)
        with _masked(drop):
            lo, dx = oracle_columns(params_of(case), case.H, xs, ys, length, R, None, want_dx)
        _fault_cache[key] = (lo[:, 0], dx[:, 0] if want_dx else None)
    return _fault_cache[key]


def fault_statistics(case, b, rows, got, tensor='logits'):
    """per row of `rows`: the worst-row statistic a fault on that row alone produces, |got[i] - want[rows[i], b]| over the dataset's rms row norm"""
    want = oracle(case, None, tensor == 'dx')[0 if tensor == 'logits' else 1]
    return (got - want[torch.as_tensor(rows), b]).norm(dim=-1) / rms_row_norm(want, b)


def planted_faults(case, fmt, cap=0):
    """[(name, b, rows, kwargs of `faulted`, keys removed, whole)] for this case under this format's tiles: the five faults of the table at one row of the first and
    one row of the last query block, the last split missing for a whole query block, and (ragged) a dataset that reads sep_max keys.  whole False: `rows` is the
    query block the one faulted row is taken from -- the row of the block that the fault moves most in the f64 oracle (a row whose softmax puts no mass on the lost
    keys shows no fault in any format; which row it is goes to the record, with the block's median beside it); whole True: every row of `rows` is faulted."""
    st, lens = split_state(case, fmt, cap), lengths_of(case)
    b = max(range(case.B), key=lambda i: (lens[i], i))      # the dataset with the most keys (uniform: the last one)
    keys, out = lens[b], []
    block = lambda q: list(range(q * st['qblk'], min((q + 1) * st['qblk'], case.n)))
    spots = [('first block', block(0))] + ([('last block', block(st['qblocks'] - 1))] if st['qblocks'] > 1 else [])
    for spot, rows in spots:
        if case.B > 1 and keys > 0:
            out.append((f'other dataset\'s train rows, {spot}', b, rows, dict(train_from=(b - 1) % case.B), keys, False))
        for lo, hi in ((64, 128), (32, 64)):
            if keys > lo:
                out.append((f'keys [{lo}, {hi}) missing, {spot}', b, rows, dict(drop=range(lo, min(hi, keys))), min(hi, keys) - lo, False))
        if keys > 0:
            first = (keys - 1) // st['kvb'] * st['kvb']
            out.append((f'last key tile missing, {spot}', b, rows, dict(drop=range(first, keys)), keys - first, False))
            out.append((f'self key missing, {spot}', b, rows, dict(drop='self'), 1, False))
        if st['splits'] > 1:
            first = (st['splits'] - 1) * st['split_keys']
            out.append((f'last split missing, {spot}', b, rows, dict(drop=range(first, keys)), keys - first, True))
    if isinstance(case.sep, tuple):
        for d, length in enumerate(lens):
            if length < max(lens):
                out.append((f'dataset {d} ({length} keys) reads sep_max keys', d, block(0), dict(train_len=max(lens)), max(lens) - length, False))
    return out
