"""The bounds of tests/test_gpu_predict_rows.py have teeth, shown on the CPU before anything runs on a GPU (tests/predict_cases.py holds the matrix and the rules):
the emulated per-row errors that the bounds are made of lie in the window the two formats' significands predict; every case is in the state of the cached-attention
kernels it is in the matrix for (a Python restatement of attn_cache_splits / launch_fwd_cache_t); the form of the predict backward is the one the restated predicates
select; and faults planted into the f64 oracle alone -- a wrapped d_q_mask, another dataset's train rows -- move one test row beyond the bound the GPU test asserts:

    f32  : every fault exceeds the f32 bound by at least 100 x (logits, and dx on the dx cases)
    fp16 : every fault exceeds the fp16 bound
    bf16 : another dataset's train rows, and a missing run of >= 32 keys, exceed the bf16 bound; every other bf16 multiple is recorded, nothing is asserted about it

The multiples go to profiles/predict_row_fault_sensitivity.json when PFN_RECORD_FAULTS names that file."""
import json
import math
import os

import pytest
import torch

import predict_cases as P
import stack_cases
from oracle import pfn_oracle as O

U = O.UNIT_ROUNDOFF
_record = {}


def _case_formats():
    return [(name, fmt) for name in P.CASES for fmt in P.CASE_FORMATS[name]]


def teardown_module(module):
    path = os.environ.get('PFN_RECORD_FAULTS')
    if path and _record:
        sig = lambda v: float(f'{v:.4g}') if isinstance(v, float) else v
        json.dump({k: {kk: sig(vv) for kk, vv in v.items()} if isinstance(v, dict) else sig(v) for k, v in sorted(_record.items())}, open(path, 'w'), indent=1)


def test_every_run_names_a_case_and_a_format():
    for run in P.PREDICT + P.RAGGED + P.CHUNKED + P.FORWARD + P.DX:
        assert run.case in P.CASES and P.fmt_of(run) in P.FORMATS
        assert P.fmt_of(run) in P.CASE_FORMATS[run.case], run      # (its bound is one the window test below has seen)
    assert all(isinstance(P.CASES[r.case].sep, tuple) for r in P.RAGGED)


def test_the_model_does_not_depend_on_its_precision():
    """the oracle's parameters are those of the f32 model of the case: the 16-bit models must draw the same ones"""
    case = P.CASES['A']
    want = P.params_of(case)
    for prec, ev in (('fp16', 'same'), ('bf16', 'same'), ('fp16', 'f32')):
        sd = P.make_model(case, prec, ev).state_dict()
        assert all(torch.equal(sd[k], v) for k, v in want.items())
    plain = P.make_model(case, scale=1.0).state_dict()
    k = 'transformer_encoder.layers.1.self_attn.in_proj_weight'
    assert torch.equal(want[k][:256], plain[k][:256] * P.CASE_SCALE['A']) and torch.equal(want[k][256:], plain[k][256:])


@pytest.mark.parametrize('name,fmt', sorted(P.STATES), ids=lambda v: str(v))
def test_cases_reach_the_states_they_are_in_the_matrix_for(name, fmt):
    st = P.split_state(P.CASES[name], fmt)
    assert {k: st[k] for k in P.STATES[(name, fmt)]} == P.STATES[(name, fmt)], st


def test_split_arithmetic_in_words():
    """the states the issue names, spelled out once more against the restated rule"""
    A, F_, G = P.CASES['A'], P.CASES['F'], P.CASES['G']
    assert P.split_state(A, 'f32', cap=1)['splits'] == 1 and P.split_state(A, 'f32', cap=1)['split_keys'] == 437
    f = P.split_state(F_, 'f32')
    assert (f['splits'], f['split_keys'] // f['kvb'], f['keys_last_split']) == (5, 3, 53)
    g = P.split_state(G, 'fp16')
    assert (g['asked'], g['splits'], g['split_keys'] // g['kvb'], g['keys_last_split']) == (5, 4, 2, 53)
    chunk = P.split_state(F_, 'f32', n=P.CHUNK_ROWS)      # a chunk of 37 rows per dataset: one query block, more splits than the whole call
    assert chunk['qblocks'] == 1 and chunk['splits'] > f['splits'] and F_.n % P.CHUNK_ROWS != 0
    gb, db = P.split_state(G, 'fp16', backward=True), P.split_state(P.CASES['D'], 'bf16', backward=True)      # the backward cuts 32-key tiles in every format
    assert (gb['asked'], gb['splits'], gb['split_keys'], gb['keys_last_split']) == (5, 5, 96, 53) and (db['splits'], db['split_keys'], db['keys_last_split']) == (2, 64, 1)
    assert P.split_state(A, 'f32', backward=True) == P.split_state(A, 'f32')
    assert P.attn_cache_splits(32, 260, 128, 4, 64, 'f32') == 1      # >= 256 workgroups: one pass
    assert P.tiles('f32', 256) == (128, 32, 2) and P.tiles('fp16', 256) == (128, 32, 1) and P.tiles('bf16', 128) == (256, 64, 1) and P.tiles('f32', 32) == (128, 32, 1)


def test_the_form_of_the_predict_backward():
    """PREDICT_BACKWARD_FORM against the restated predicates (pfn_oracle.Rounding.plan under top_rows=True): lnbwd_fusable at M = B n depends on the widths and the
    schedule alone (predict_cases' docstring), predict_dsrc_is_t on nlayers > 0, and the top layer's LayerNorm backward always reads f32 rows"""
    for (E, nhid, sched), want in P.PREDICT_BACKWARD_FORM.items():
        for fmt in ('fp16', 'bf16'):
            for M, sep in ((7, 437), (2400, 0)):
                pl = P.rounding(fmt, sched).plan(E, 2, nhid, P.L, sep + M, sep, 0.0)
                assert {k: pl[k] for k in want} == want, (E, nhid, sched, fmt, pl)
    widths = {(c.E, 2 * c.E, 0) for c in P.CASES.values()}
    assert widths <= set(P.PREDICT_BACKWARD_FORM)      # every case of the matrix has its row
    assert P.rounding('fp16').plan(1024, 4, 2048, P.L, 70, 63, 0.0)['y16u'] and not P.rounding('fp16').plan(512, 4, 1024, P.L, 70, 63, 0.0)['y16u']
    for site in ('emb_grad', 'out_grad', 'x1_grad', 'qkv', 'ctx', 'dS', 'P', 'y_grad', 'pre_grad', 'dlog'):
        assert site in O.ROUNDING_SITES


@pytest.mark.parametrize('name,fmt', _case_formats(), ids=lambda v: str(v))
def test_emulated_row_errors_lie_in_the_window_of_the_format(name, fmt):
    case = P.CASES[name]
    want_dx = name in P.DX_CASES
    e = P.emulated(case, fmt, want_dx)
    assert len(e) == (4 if want_dx else 2)
    for label, v in e.items():
        _record[f'{name} {fmt} {label[0]} {label[1]}: emulated e, and the bound asserted on the GPU'] = dict(e=v, bound=stack_cases.bound(fmt, v))
        assert math.isfinite(v) and v > 0, (label, v)
        if fmt == 'f32':
            assert 2.0 ** -26 < v < 1e-5, (label, v)
        else:
            assert U[fmt] / 4 < v < 0.02, (label, v)
    lo, dxo = P.oracle(case, None, want_dx)
    assert torch.isfinite(lo).all() and not P.zero_datasets(lo)
    if want_dx:
        assert torch.isfinite(dxo).all() and not P.zero_datasets(dxo)


@pytest.mark.parametrize('name', [n for n in P.CASES if {'fp16', 'bf16'} <= set(P.CASE_FORMATS[n])])
def test_bf16_to_fp16_error_ratio_is_the_three_bits_between_them(name):
    case = P.CASES[name]
    want_dx = name in P.DX_CASES
    eb, ef = P.emulated(case, 'bf16', want_dx), P.emulated(case, 'fp16', want_dx)
    for tensor in ('logits', 'dx') if want_dx else ('logits',):
        ratio = eb[(tensor, 'rel l2')] / ef[(tensor, 'rel l2')]
        assert 4 < ratio < 16, (tensor, ratio)


def _must_exceed(fmt, fault, removed):
    """the multiple of the bound a planted fault has to reach in this format; None: recorded only"""
    if fmt == 'f32':
        return 100.0
    if fmt == 'fp16':
        return 1.0
    return 1.0 if fault.startswith('other dataset') or removed >= 32 and not fault.startswith('dataset') and not fault.startswith('self') else None


@pytest.mark.parametrize('name,fmt', _case_formats(), ids=lambda v: str(v))
def test_planted_faults_move_a_row_beyond_the_bound(name, fmt):
    case = P.CASES[name]
    want_dx = name in P.DX_CASES
    bounds = P.bounds(case, fmt, want_dx)
    dx_bound_f32 = P.bounds(case, 'f32', True)[('dx', 'worst row')] if want_dx else None
    missed = []
    for fault, b, rows, kw, removed, whole in P.planted_faults(case, fmt):
        lo, dx = P.faulted(case, b, rows, want_dx=want_dx, **kw)
        per_row = P.fault_statistics(case, b, rows, lo) / bounds[('logits', 'worst row')]
        i = int(per_row.argmax())
        multiple = per_row[i].item()
        _record[f'{name} {fmt} logits: {fault}'] = dict(multiple_of_bound=multiple, dataset=b, row=rows[i], median_over_the_block=per_row.median().item(),
                                                       rows='every row of the block' if whole else 'one row')
        need = _must_exceed(fmt, fault, removed)
        if need is not None and not multiple >= need:
            missed.append(f'{fault}: logits worst row {multiple:.3g} x the {fmt} bound, needs {need:g}')
        if want_dx:      # the same fault at the same row
            stat = (P.fault_statistics(case, b, rows, dx, 'dx').max() if whole else P.fault_statistics(case, b, rows, dx, 'dx')[i]).item()
            _record[f'{name} {fmt} dx: {fault}'] = dict(multiple_of_bound=stat / bounds[('dx', 'worst row')], multiple_of_f32_bound=stat / dx_bound_f32)
            if not stat / dx_bound_f32 >= 100.0:
                missed.append(f'{fault}: dx worst row {stat / dx_bound_f32:.3g} x the f32 bound, needs 100')
    assert not missed, '\n'.join(missed)


def test_a_case_without_train_rows_has_no_key_to_lose():
    assert P.planted_faults(P.CASES['B'], 'f32') == []
    assert stack_cases.bound('f32', 0.0) == 4 * 2.0 ** -23 and stack_cases.bound('fp16', 1e-3) == 3e-3      # the rule is the stack suite's, imported
