"""Inference on the MI355X, one test row at a time: condition / predict, their ragged and chunked forms, the saved pass with its input gradient and the model.eval()
forward against the f64 oracle (oracle/pfn_oracle.py) on cat(train, test) -- the kernels no training test reaches: attn_fwd_kernel<..., CACHE> over
attn_cache_splits key ranges, attn_merge_kernel, attn_bwd_cache_kernel and its merge, EPI_ROWSHIFT on the self key, the per-dataset key counts of a ragged context.
The matrix, the models (in-projection scaled: a missing key must move a row by more than rounding does), the statistics and the bound rule live in
tests/predict_cases.py, shared with tests/test_host_predict_rows.py, which shows on the CPU what each bound catches.

The existing predict tests assert one relative l2 over the whole logits tensor, at 2 x what the code under test measured: one wrong row among 2400, or a query that
loses a partial key tile, passes them.  Here every dataset has two statistics, on logits [n, B, n_out] and on dx [n, B, F]:

    worst row : max over t of |got[t, b] - want[t, b]| / (the dataset's rms row norm of want)          rel l2 : |got[:, b] - want[:, b]| / |want[:, b]|
    16-bit    : below 3 x max(e, u),  e = the same statistic of the OPERAND-ROUNDED f64 oracle under the plan of the pass against the plain f64 oracle
    f32       : below 4 x max(e, 2^-23),  e = the oracle run in f32 against f64                          (stack_cases.bound: the rule of the stack-gradient suite)

Bounds come from the reference only.  The f32 bounds catch any indexing error by three orders of magnitude, the fp16 bounds every tile-granular one, the bf16 bounds
only the large ones (another dataset's rows, a run of >= 32 keys): profiles/predict_row_fault_sensitivity.json has the multiple per case and fault.  A row beyond
its bound is a finding: a rounding site the table lacks, or a wrong kernel or dispatch rule.  Every value is recorded as value / bound
(profiles/predict_row_parity_measured.json, PFN_RECORD_BOUNDS); a failure names the dataset, the row, its query block and the key tile of its last split."""
import pytest
import torch

import predict_cases as P
from bounds import within
from test_gpu_predict_grad import predict_vjp, split_cap
from transformerscandobayesianinference_amd.transformer import TransformerModel

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _setup(run):
    case = P.CASES[run.case]
    model = P.make_model(case, run.precision, run.eval_precision).to(DEV).eval()
    x, y = P.make_data(case)
    return case, model, x.to(DEV), y.to(DEV)


def _condition(case, model, x, y):
    top = P.sep_max(case)
    if isinstance(case.sep, tuple):
        return model.condition((x[:top], y[:top]), train_lengths=case.sep)
    return model.condition((x[:top], y[:top]))


def _check(run, got, tensors):
    """got: {'logits': [n, B, n_out], 'dx': [n, B, F]} of the run; every statistic of every tensor in `tensors` against its bound, the failures collected"""
    case, fmt = P.CASES[run.case], P.fmt_of(run)
    want_dx = 'dx' in tensors
    want = dict(zip(('logits', 'dx'), P.oracle(case, None, want_dx)))
    e, bounds = P.emulated(case, fmt, want_dx), P.bounds(case, fmt, want_dx)
    failures = []
    for tensor in tensors:
        g, w = got[tensor].detach().double().cpu(), want[tensor]
        assert g.shape == w.shape and torch.isfinite(g).all(), tensor
        for b in P.zero_datasets(w):
            assert torch.count_nonzero(g[:, b]) == 0, f'{tensor}: dataset {b} has an identically zero exact value'
        for stat, value in P.row_stats(g, w).items():
            v, b = value[0], value[1]
            spot = f'dataset {b}'
            if stat == 'worst row':
                spot += f', row {value[2]}: ' + P.where(case, fmt, run.cap, value[2], b, backward=tensor == 'dx')
            print(f'{P.run_id(run)} {tensor} {stat}: {v:.3e} (emulated {e[(tensor, stat)]:.3e}, bound {bounds[(tensor, stat)]:.3e}) at {spot}')
            try:
                within(f'{fmt} {tensor} {stat} / bound', v / bounds[(tensor, stat)], 1.0)
            except AssertionError:
                failures.append(f'{tensor} {stat}: {v:.3e} is not below the bound {bounds[(tensor, stat)]:.3e} (emulated {e[(tensor, stat)]:.3e}) at {spot}')
    return failures


@pytest.mark.parametrize('run', P.PREDICT, ids=P.run_id)
def test_predict_logits_per_row_vs_oracle(run):
    case, model, x, y = _setup(run)
    with split_cap(run.cap):
        got = model.predict(_condition(case, model, x, y), x[P.sep_max(case):])
    failures = _check(run, dict(logits=got), ['logits'])
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('run', P.RAGGED, ids=P.run_id)
def test_ragged_predict_logits_per_row_vs_oracle(run):
    """the oracle: every dataset alone on its own first `length` rows"""
    case, model, x, y = _setup(run)
    ctx = _condition(case, model, x, y)
    assert ctx.lengths == tuple(case.sep)
    failures = _check(run, dict(logits=model.predict(ctx, x[P.sep_max(case):])), ['logits'])
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('run', P.CHUNKED, ids=P.run_id)
def test_chunked_predict_logits_per_row_vs_oracle(run, monkeypatch):
    case, model, x, y = _setup(run)
    ctx = _condition(case, model, x, y)
    monkeypatch.setattr(TransformerModel, '_PREDICT_ROWS', P.CHUNK_ROWS * case.B)      # 37 rows per dataset and chunk: 9 chunks, the last one of 4 rows
    failures = _check(run, dict(logits=model.predict(ctx, x[case.sep:])), ['logits'])
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('run', P.FORWARD, ids=P.run_id)
def test_inference_forward_logits_per_row_vs_oracle(run):
    """model.eval() under torch.no_grad(): the pass the existing predict tests use as their reference"""
    case, model, x, y = _setup(run)
    with torch.no_grad():
        got = model((x, y), single_eval_pos=case.sep)
    assert not got.requires_grad
    failures = _check(run, dict(logits=got), ['logits'])
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('run', P.DX, ids=P.run_id)
def test_predict_input_gradient_per_row_vs_oracle(run):
    case, model, x, y = _setup(run)
    top = P.sep_max(case)
    R = P.cotangent(case).to(DEV)
    with split_cap(run.cap):
        ctx = _condition(case, model, x, y)
        out, dx = predict_vjp(model, ctx, x[top:], R)
        with torch.no_grad():
            plain = model.predict(ctx, x[top:])
    assert torch.equal(out.detach(), plain)      # the saved pass returns the plain pass's bits
    failures = _check(run, dict(logits=out, dx=dx), ['logits', 'dx'])
    assert not failures, '\n'.join(failures)
