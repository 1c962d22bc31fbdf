"""The encoder stack and the decoder, one gradient tensor at a time: logits and every parameter gradient of a whole forward + backward against the f64 oracle
(oracle/pfn_oracle.py), on every form of the backward that pfn_api.hip's make_plan / top_layer_on_test_rows* / tn_set_groupable / lnbwd_fusable can select -- the
matrix, its models and the bound rule live in tests/stack_cases.py, shared with the CPU checks of the oracle hook (tests/test_host_rounded_oracle.py).

The model tests assert the 16-bit gradients as ONE number, the relative l2 error of the flat gradient, to which a LayerNorm weight or a bias contributes 1 - 5 %: a
20 % error in norm1.bias, or one wrong 32-row slab of a weight gradient, passes them.  Here every tensor has its own bound, and every 2-D tensor a second one for its
worst block of 32 rows or 32 columns:

    16-bit : 3 x max(e, u),  e = the same statistic of the OPERAND-ROUNDED f64 oracle (the stack's 16-bit stores emulated site by site, pfn_oracle.ROUNDING_SITES,
             under the same plan predicates) against the plain f64 oracle on the same inputs, u = 2^-9 (bf16) / 2^-12 (fp16)
    f32    : 4 x max(e, 2^-23),  e = the oracle run in f32 against f64

Bounds come from the reference only.  A tensor beyond its bound is a finding: a rounding site the table lacks (add it, with the line that proves it) or a wrong kernel.
Tensors whose exact gradient is identically zero (y_encoder.* without train rows, or without an encoder layer to carry them to a test row) must be exactly zero.
Every value is recorded as value / bound (profiles/stack_grad_parity_measured.json, PFN_RECORD_BOUNDS) under its class -- logits, weights, biases, LayerNorm
parameters, worst slab: the largest of the class per case; a failure names the tensor and the eval position.
"""
import ctypes
import re

import pytest
import torch

import stack_cases as C
from bounds import within
from transformerscandobayesianinference_amd import _hip

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
# include/pfn_hip.h PFN_PROF_*: launches that only one form of the schedule records (slot + 1: the top layer on the compact test rows)
PROF_GEMM_OUT_LN, PROF_GEMM_LIN1, PROF_GEMM_DY1, PROF_WGRAD = 10, 12, 18, 24


def _launches(slot):
    ms, n = ctypes.c_double(), ctypes.c_int64()
    _hip.check(_hip.lib().pfn_profile_read(slot, ctypes.byref(ms), ctypes.byref(n)), 'pfn_profile_read')
    return n.value


def _recorded_form():
    """what the launches of the last pass say about the form it took (and clears the record)"""
    got = dict(fuse_ln=_launches(PROF_GEMM_OUT_LN) + _launches(PROF_GEMM_OUT_LN + 1) > 0, fuse_lnb=_launches(PROF_GEMM_DY1) + _launches(PROF_GEMM_DY1 + 1) > 0,
               top_rows=_launches(PROF_GEMM_LIN1 + 1) > 0, grouped=_launches(PROF_WGRAD) + _launches(PROF_WGRAD + 1) > 0)
    for slot in range(26):
        _launches(slot)
    return got


def _run_single(model, x, y, sep):
    model.zero_grad()
    logits = model((x, y), single_eval_pos=sep)
    loss = model.criterion(logits.reshape(-1, C.NBARS), y[sep:].reshape(-1)).mean()
    loss.backward()
    return [logits[:, b].detach() for b in range(logits.shape[1])], {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def _run_ragged(model, x, y, seps):
    """forward_batches with one eval position per dataset: the sum of the per-batch losses (its gradient: the sum of the per-dataset oracle gradients)"""
    model.zero_grad()
    outs = model.forward_batches([(x[:, b:b + 1], y[:, b:b + 1]) for b in range(C.B)], seps)
    loss = sum(model.criterion(o.reshape(-1, C.NBARS), y[s:, b:b + 1].reshape(-1)).mean() for b, (o, s) in enumerate(zip(outs, seps)))
    loss.backward()
    return [o[:, 0].detach() for o in outs], {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def _group(label):
    """the label a value is RECORDED under (the failure message names the tensor itself): the classes a global figure dilutes, kept apart"""
    if label.startswith('logits'):
        return 'logits rel l2 per dataset'
    if label.endswith('worst 32-slab'):
        return 'weight grads, worst 32-slab'
    name = label.split(' ')[0]
    if re.search(r'norm\d\.(weight|bias)$', name):
        return 'LayerNorm weight / bias grads rel l2'
    return 'bias grads rel l2' if name.endswith('bias') else 'weight grads rel l2'


@pytest.mark.parametrize('row', C.MATRIX, ids=C.case_id)
def test_stack_gradients_per_tensor_vs_oracle(row):
    shape, prec, sched, kind, t, seps, dropout = row
    ragged = kind == 'ragged'
    model = C.make_model(shape, prec, C.SCHEDULES[sched], dropout)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    x, y = C.make_data(shape, t)
    xd, yd = x.to(DEV), y.to(DEV)
    nlayers = C.SHAPES[shape][4]
    failures = []
    _hip.check(_hip.lib().pfn_profile_enable(1), 'pfn_profile_enable')
    try:
        _recorded_form()
        for sep in ([list(seps)] if ragged else seps):
            logits, grads = _run_ragged(model, xd, yd, sep) if ragged else _run_single(model, xd, yd, sep)
            torch.cuda.synchronize()
            # the form this row is in the matrix for is the one the descriptor selected: the launches recorded against the restated predicates
            pl = C.plan_of(shape, prec, C.SCHEDULES[sched], t, 0 if ragged else sep, dropout, ragged)
            want_form = {k: bool(pl[k]) and nlayers > 0 for k in ('fuse_ln', 'fuse_lnb', 'top_rows', 'grouped')}
            assert _recorded_form() == want_form, (sep, pl)
            if prec != 'f32' and sched == 'default' and not dropout:
                assert {k: pl[k] for k in C.INTENDED_FORM[shape]} == C.INTENDED_FORM[shape], pl
            seed = model._last_dropout_seed if dropout else None
            logits_o, grads_o, e, bounds = C.bounds_for(row, sep, sd, x, y, dropout_seed=seed)
            assert all(torch.isfinite(g).all() for g in grads.values()) and all(torch.isfinite(l).all() for l in logits)
            for k in C.zero_tensors(grads_o):
                assert torch.count_nonzero(grads[k]) == 0, f'sep {sep}: {k} has an identically zero exact gradient'
            got = C.statistics(logits, grads, logits_o, grads_o)
            assert got.keys() == bounds.keys()
            for label, value in got.items():
                print(f'{C.case_id(row)} sep {sep} {label}: {value:.3e} (emulated {e[label]:.3e}, bound {bounds[label]:.3e})')
                try:
                    within(f'{_group(label)} / bound', value / bounds[label], 1.0)
                except AssertionError:
                    failures.append(f'sep {sep} {label}: {value:.3e} is not below the bound {bounds[label]:.3e} (emulated {e[label]:.3e})')
    finally:
        _hip.check(_hip.lib().pfn_profile_enable(0), 'pfn_profile_enable')
        _recorded_form()
    assert not failures, '\n'.join(failures)
