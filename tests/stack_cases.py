"""What tests/test_host_rounded_oracle.py (CPU) and tests/test_gpu_stack_grads.py (MI355X) share: the case matrix of the per-tensor stack-gradient suite, its models and
inputs, the oracle runs (f64, f32 and operand-rounded: oracle/pfn_oracle.py Rounding) cached per (case, sep, format, plan), the statistics and the bound rule.

Bound rule (from the reference only, never from what the kernels measure):
    16-bit : 3 x max(e, u)      e = the same statistic of the operand-rounded f64 oracle against the plain f64 oracle on the same inputs, u = 2^-9 (bf16) / 2^-12 (fp16)
    f32    : 4 x max(e, 2^-23)  e = the statistic of the oracle run in f32 against f64
3: the recorded global errors of the HIP stack are 1.2 - 1.5 x the emulation's (it leaves out the f32 accumulation order and the atomics); 3 leaves a factor 2 above
that and stays 5 - 30 x under what a wrong small tensor produces.
"""
import torch

from oracle import pfn_oracle as O
from transformerscandobayesianinference_amd import _hip, bar_distribution, encoders
from transformerscandobayesianinference_amd.transformer import TransformerModel

T, B, F, NBARS = 130, 3, 5, 20      # 390 token rows: a multiple of no tile
SEPS = (1, 64, 129)                 # the top layer on all rows / on the test rows / one test row per dataset
RAGGED_SEPS = [0, 77, 129]
PRECISIONS = ('f32', 'bf16', 'fp16')
SCHEDULES = {'default': 0, 'deterministic': _hip.SCHED_DETERMINISTIC, 'separate_lnbwd': _hip.SCHED_SEPARATE_LNBWD, 'top_layer_all_rows': _hip.SCHED_TOP_LAYER_ALL_ROWS,
             'fuse_q_projection': _hip.SCHED_FUSE_Q_PROJECTION, 'key_centering': _hip.SCHED_KEY_CENTERING, 'no_key_centering': _hip.SCHED_NO_KEY_CENTERING,
             'f32_residual': _hip.SCHED_F32_RESIDUAL, 'fuse_ln_wide': _hip.SCHED_FUSE_LN_WIDE}

# shape id -> (E, H in 16-bit, H in f32, nhid, L)
SHAPES = {'e64': (64, 2, 2, 72, 2), 'e128': (128, 4, 4, 256, 2), 'e128-L0': (128, 4, 4, 256, 0), 'e128-L1': (128, 4, 4, 256, 1), 'e192': (192, 3, 3, 200, 2),
          'e256': (256, 4, 4, 512, 2), 'e1024': (1024, 4, 8, 1024, 1)}      # (head dim 256 has no f32 backward: H 8 there)

# What each shape is in the matrix for, as the predicates of pfn_api.hip make_plan decide it for a 16-bit descriptor under the DEFAULT schedule (Rounding.plan restates
# them; the GPU suite checks that restatement against the launches the library records).  A later change of a dispatch rule that empties a row fails here.
INTENDED_FORM = {'e64': dict(fuse_ln=False, fuse_lnb=False, grouped=False),      # LayerNorm as its own kernel, one-by-one weight gradients, K = 72
                 'e128': dict(fuse_ln=True, fuse_lnb=True, grouped=False),       # gemm_nt_ln_kernel, gemm_nt_lnbwd_kernel; fp16: y16
                 'e128-L0': dict(fuse_ln=True), 'e128-L1': dict(fuse_ln=True, fuse_lnb=True),
                 'e192': dict(fuse_ln=False, fuse_lnb=False, grouped=False),     # a width no fused kernel covers, K = 200
                 'e256': dict(fuse_ln=True, fuse_lnb=True, grouped=True),        # the grouped 256 x 256 weight-gradient launch
                 'e1024': dict(fuse_ln=False, fuse_lnb=False, grouped=True)}     # fp16: y16u; PFN_SCHED_FUSE_LN_WIDE turns fuse_ln / fuse_lnb on
SCHEDULE_FORM = {'separate_lnbwd': dict(fuse_lnb=False), 'deterministic': dict(fuse_lnb=False), 'fuse_ln_wide': dict(fuse_ln=True, fuse_lnb=True)}


def _matrix():
    rows = []      # (shape, precision, schedule name, kind, T, seps, dropout)
    def add(shape, schedules, kind='single', t=T, seps=SEPS, dropout=0.0, only=None):
        for sched in schedules:
            for prec in PRECISIONS:
                if only is None or prec in only.get(sched, PRECISIONS):
                    rows.append((shape, prec, sched, kind, t, tuple(seps), dropout))
    add('e64', ['default', 'deterministic'])
    add('e128', ['default', 'deterministic', 'separate_lnbwd', 'top_layer_all_rows', 'fuse_q_projection', 'key_centering', 'no_key_centering', 'f32_residual'],
        only={'key_centering': ('bf16',), 'no_key_centering': ('fp16',), 'f32_residual': ('fp16',)})
    add('e128-L0', ['default'])
    add('e128-L1', ['default'])
    add('e192', ['default', 'deterministic'])
    add('e256', ['default', 'deterministic'])
    add('e1024', ['default', 'fuse_ln_wide', 'deterministic'], only={'fuse_ln_wide': ('bf16', 'fp16')})
    add('e128', ['default'], t=300, seps=(257,))                                  # q_begin 256: a skipped query block, scatter_rows with zero_from
    add('e128', ['default', 'deterministic'], seps=(0,))                          # no train rows: attn_bwd_self_only_kernel after the fused delta (zero_delta) / in place of attn_delta_kernel
    add('e128', ['default', 'deterministic'], kind='ragged', seps=RAGGED_SEPS)    # ragged sep_of: gather, scatter and zero prefix per dataset
    add('e256', ['default', 'deterministic'], kind='ragged', seps=RAGGED_SEPS)
    add('e64', ['default'], seps=(64,), dropout=0.3)                              # the three element-wise dropout sites and the attention masks
    add('e256', ['default'], seps=(64,), dropout=0.3)
    return rows


MATRIX = _matrix()


def case_id(row):
    shape, prec, sched, kind, t, seps, dropout = row
    return '-'.join([shape, prec, sched] + ([kind] if kind != 'single' else []) + ([f'T{t}'] if t != T else []) + ([f'p{dropout}'] if dropout else []) +
                    (['sep0'] if seps == (0,) else []))


def dims(shape, precision):
    E, h16, h32, nhid, L = SHAPES[shape]
    return E, (h32 if precision == 'f32' else h16), nhid, L


def make_model(shape, precision, schedule=0, dropout=0.0):
    E, H, nhid, L = dims(shape, precision)
    torch.manual_seed(E + 7 * L)
    borders = torch.sort(torch.randn(NBARS + 1) * 1.5)[0]
    m = TransformerModel(encoders.Linear(F, E), NBARS, E, H, nhid, L, dropout, y_encoder=encoders.Linear(1, E), precision=precision, eval_precision=precision)
    m.schedule = schedule
    m.criterion = bar_distribution.FullSupportBarDistribution(borders)
    with torch.no_grad():
        for layer in m.transformer_encoder.layers:      # un-zero the residual branches
            layer.linear2.weight.normal_(0, 0.03)
            layer.self_attn.out_proj.weight.normal_(0, 0.03)
    return m


def make_data(shape, t=T, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + SHAPES[shape][0] + t)
    return torch.randn(t, B, F, generator=g), torch.randn(t, B, generator=g)


def plan_of(shape, precision, schedule, t, sep, dropout=0.0, ragged=False):
    """the form the descriptor selects (pfn_api.hip make_plan and friends, restated by Rounding.plan) -- every flag False in the exact-f32 mode"""
    E, H, nhid, L = dims(shape, precision)
    if precision == 'f32':
        pl = dict.fromkeys(('fuse_ln', 'y16', 'y16u', 'fuse_lnb', 'center', 'emb_t', 'grouped'), False)
        pl['top_rows'] = O.Rounding(None, schedule).plan(E, H, nhid, L, t, sep, dropout)['top_rows'] and not ragged
        return pl
    pl = O.Rounding(precision, schedule, top_rows=False if ragged else None).plan(E, H, nhid, L, t, sep, dropout)      # (ragged: 4 min(sep_of) >= S decides; RAGGED_SEPS holds a 0)
    pl['grouped'] = E % 256 == 0 and nhid % 256 == 0      # tn_set_groupable: every P and Q (E, nhid, 3 E) a multiple of 256
    return pl


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------------------------------
def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def logits_err(got, want):
    """relative l2 per dataset, the largest; got / want: lists of [rows_b, n_out] (one per dataset)"""
    return max(relerr(g, w) for g, w in zip(got, want))


def worst_slab(got, want, block=32):
    """max over blocks of 32 rows and blocks of 32 columns of rms(got - want over the slab) / rms(want over the WHOLE tensor): some blocks have an exact gradient of
    zero (the K block of in_proj_bias's rows in in_proj_weight: softmax ignores a key bias), so the slab's own norm cannot be the denominator"""
    d = (got.detach().double().cpu() - want.double()) ** 2
    den = (want.double() ** 2).mean().sqrt().clamp_min(1e-300)
    worst = 0.0
    for axis in (0, 1):
        per = d.mean(1 - axis)
        for i in range(0, per.numel(), block):
            worst = max(worst, (per[i:i + block].mean().sqrt() / den).item())
    return worst


def statistics(logits, grads, logits_o, grads_o):
    """{label: value} of (logits: list per dataset, grads: dict) against the f64 oracle's; tensors whose exact gradient is identically zero are left out (zero_tensors)"""
    out = {'logits rel l2 per dataset': logits_err(logits, logits_o)}
    for k, w in grads_o.items():
        if w.abs().max() == 0:
            continue
        out[f'{k} grad rel l2'] = relerr(grads[k], w)
        if w.dim() == 2 and min(w.shape) > 1:
            out[f'{k} grad worst 32-slab'] = worst_slab(grads[k], w)
    return out


def zero_tensors(grads_o):
    return [k for k, w in grads_o.items() if w.abs().max() == 0]


def bound(precision, e):
    return 4 * max(e, 2.0 ** -23) if precision == 'f32' else 3 * max(e, O.UNIT_ROUNDOFF[precision])


# ---- oracle runs, cached ------------------------------------------------------------------------------------------------------------------------------------------------
_cache = {}


def _run(sd, x, y, sep, H, ragged, **kw):
    """(logits per dataset, grads) of pfn_oracle.loss_and_grads; ragged: sep is a list, one dataset each, the sum of the per-dataset gradients"""
    if not ragged:
        _, lg, g = O.loss_and_grads(sd, x, y, y, sep, H, sd['criterion.borders'], **kw)
        return [lg[:, b] for b in range(lg.shape[1])], g
    runs = [O.loss_and_grads(sd, x[:, b:b + 1], y[:, b:b + 1], y[:, b:b + 1], s, H, sd['criterion.borders'], **kw) for b, s in enumerate(sep)]
    return [r[1][:, 0] for r in runs], {k: sum(r[2][k] for r in runs) for k in runs[0][2]}


def oracle(row, sep, sd, x, y, fmt=None, dropout_seed=None):
    """fmt None: the f64 oracle; 'f32': the oracle in f32; 'bf16' / 'fp16': the operand-rounded f64 oracle under the plan of this row.  sd, x, y: the row's (they key
    the cache through the row's shape, T and dropout only -- make_model / make_data are deterministic)."""
    shape, prec, sched, kind, t, seps, dropout = row
    ragged = kind == 'ragged'
    H = dims(shape, prec)[1]
    if fmt in ('bf16', 'fp16'):
        pl = plan_of(shape, fmt, SCHEDULES[sched], t, 0 if ragged else sep, dropout, ragged)
        plan_key = tuple(sorted(pl.items()))
    else:
        plan_key = ()
    key = (shape, H, kind, t, tuple(sep) if ragged else sep, dropout, dropout_seed, fmt, plan_key)
    if key not in _cache:
        kw = {}
        if dropout:
            kw['dropout'] = (dropout, dropout_seed)
        if fmt == 'f32':
            kw['dtype'] = torch.float32
        elif fmt is not None:
            kw['rounding'] = O.Rounding(fmt, SCHEDULES[sched], top_rows=False if ragged else None)
        _cache[key] = _run(sd, x, y, sep, H, ragged, **kw)
    return _cache[key]


def bounds_for(row, sep, sd, x, y, dropout_seed=None):
    """(f64 logits, f64 grads, {label: bound}) for the row's precision at this eval position (ragged: sep = the list)"""
    prec = row[1]
    logits_o, grads_o = oracle(row, sep, sd, x, y, None, dropout_seed)
    logits_e, grads_e = oracle(row, sep, sd, x, y, prec, dropout_seed)
    e = statistics(logits_e, grads_e, logits_o, grads_o)
    return logits_o, grads_o, e, {k: bound(prec, v) for k, v in e.items()}
