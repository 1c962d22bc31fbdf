"""The operand-rounded f64 oracle (oracle/pfn_oracle.py Rounding / ROUNDING_SITES) that bounds tests/test_gpu_stack_grads.py, checked on the CPU: inert by default,
the identity when nothing rounds, errors of the size the two formats' significands predict, and a live, finite error on every tensor of every case of the matrix."""
import math

import pytest
import torch

import stack_cases as C
from oracle import pfn_oracle as O
from transformerscandobayesianinference_amd import _hip


def _inputs(row):
    shape, prec, sched, kind, t, seps, dropout = row
    model = C.make_model(shape, prec, C.SCHEDULES[sched], dropout)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x, y = C.make_data(shape, t)
    return sd, x, y


def test_schedule_bits_are_the_bindings():
    names = ('SCHED_TOP_LAYER_ALL_ROWS', 'SCHED_FUSE_LN_WIDE', 'SCHED_SEPARATE_LNBWD', 'SCHED_DETERMINISTIC', 'SCHED_NO_KEY_CENTERING', 'SCHED_FUSE_Q_PROJECTION',
             'SCHED_KEY_CENTERING', 'SCHED_F32_RESIDUAL')
    assert [getattr(O, n) for n in names] == [getattr(_hip, n) for n in names]


@pytest.mark.parametrize('shape', ['e64', 'e128', 'e128-L0'])
def test_hook_is_inert_without_a_format(shape):
    """rounding=None IS the plain oracle (same operations: bit-identical to a second call); Rounding(None) walks the hooked graph -- softmax as numerators over their sum,
    GELU through its stored derivative, the key shift -- with identity roundings and reproduces it to f64 round-off, dropout included"""
    row = (shape, 'fp16', 'default', 'single', C.T, C.SEPS, 0.0)
    sd, x, y = _inputs(row)
    H, borders = C.dims(shape, 'fp16')[1], sd['criterion.borders']
    for sep in (0, 64):
        for dropout in (None, (0.3, 1234567)):
            loss0, logits0, grads0 = O.loss_and_grads(sd, x, y, y, sep, H, borders, dropout=dropout)
            loss1, logits1, grads1 = O.loss_and_grads(sd, x, y, y, sep, H, borders, dropout=dropout, rounding=None)
            assert torch.equal(loss0, loss1) and torch.equal(logits0, logits1) and all(torch.equal(grads0[k], grads1[k]) for k in grads0)
            for sched in (0, O.SCHED_DETERMINISTIC | O.SCHED_KEY_CENTERING):
                loss2, logits2, grads2 = O.loss_and_grads(sd, x, y, y, sep, H, borders, dropout=dropout, rounding=O.Rounding(None, sched))
                assert abs(loss2 - loss0) < 1e-13 * abs(loss0) and C.relerr(logits2, logits0) < 1e-13
                for k in grads0:
                    assert C.relerr(grads2[k], grads0[k]) < 1e-12 or (grads0[k].abs().max() == 0 and grads2[k].abs().max() == 0), k


def test_every_site_names_its_kind_and_line():
    for name, (kind, when, where) in O.ROUNDING_SITES.items():
        assert kind in ('R', 'Rg', 'Rv', None) and (':' in where), name
        assert when in (None, 'emb_t', 'y16', 'y16u', 'not fuse_lnb', 'per layer', 'dropout', 'center'), name


def test_intended_forms_are_what_the_predicates_select():
    """every shape is in the matrix for a form of the backward (C.INTENDED_FORM); the restated make_plan predicates must select it"""
    for shape, want in C.INTENDED_FORM.items():
        for prec in ('bf16', 'fp16'):
            pl = C.plan_of(shape, prec, 0, C.T, 64)
            assert {k: pl[k] for k in want} == want, (shape, prec, pl)
            for sched, form in C.SCHEDULE_FORM.items():
                if SHAPE_HAS_LAYERS[shape] and (sched != 'fuse_ln_wide' or shape == 'e1024'):
                    pl = C.plan_of(shape, prec, C.SCHEDULES[sched], C.T, 64)
                    assert {k: pl[k] for k in form} == form, (shape, prec, sched, pl)
    assert C.plan_of('e128', 'fp16', 0, C.T, 64)['y16'] and not C.plan_of('e128', 'bf16', 0, C.T, 64)['y16']
    assert not C.plan_of('e128', 'fp16', _hip.SCHED_F32_RESIDUAL, C.T, 64)['y16']
    assert C.plan_of('e1024', 'fp16', 0, C.T, 64)['y16u'] and not C.plan_of('e1024', 'fp16', _hip.SCHED_FUSE_LN_WIDE, C.T, 64)['y16u']
    assert C.plan_of('e1024', 'fp16', _hip.SCHED_FUSE_LN_WIDE, C.T, 64)['y16']
    assert C.plan_of('e128', 'fp16', 0, C.T, 64)['center'] and not C.plan_of('e128', 'bf16', 0, C.T, 64)['center']
    assert C.plan_of('e128', 'bf16', _hip.SCHED_KEY_CENTERING, C.T, 64)['center'] and not C.plan_of('e128', 'fp16', _hip.SCHED_NO_KEY_CENTERING, C.T, 64)['center']
    # the eval positions: 1 keeps the top layer on all rows, 64 and 129 put it on the test rows; PFN_SCHED_TOP_LAYER_ALL_ROWS and dropout keep every row
    assert [C.plan_of('e128', 'fp16', 0, C.T, s)['top_rows'] for s in C.SEPS] == [False, True, True]
    assert not C.plan_of('e128', 'fp16', _hip.SCHED_TOP_LAYER_ALL_ROWS, C.T, 64)['top_rows'] and not C.plan_of('e64', 'fp16', 0, C.T, 64, 0.3)['top_rows']
    assert C.plan_of('e128', 'fp16', 0, 300, 257)['top_rows']


SHAPE_HAS_LAYERS = {k: v[4] > 0 for k, v in C.SHAPES.items()}
_ROWS16 = [r for r in C.MATRIX if r[1] != 'f32']


@pytest.mark.parametrize('row', _ROWS16, ids=C.case_id)
def test_every_tensor_has_a_finite_nonzero_emulated_error(row):
    shape, prec, sched, kind, t, seps, dropout = row
    sd, x, y = _inputs(row)
    for sep in ([list(seps)] if kind == 'ragged' else seps):
        logits_o, grads_o, e, bounds = C.bounds_for(row, sep, sd, x, y, dropout_seed=424242 if dropout else None)
        _, grads_e = C.oracle(row, sep, sd, x, y, prec, 424242 if dropout else None)
        for k in C.zero_tensors(grads_o):
            assert grads_e[k].abs().max() == 0, k
        assert len(e) >= 1 + len(grads_o) - len(C.zero_tensors(grads_o))
        for label, v in e.items():
            assert math.isfinite(v) and 0 < v < 0.05, (label, v)


@pytest.mark.parametrize('shape', sorted(C.SHAPES))
def test_bf16_to_fp16_error_ratio_is_the_three_bits_between_them(shape):
    """fp16 keeps 11 significand bits where bf16 keeps 8: the same sites rounded in either format must differ by about 2^3 on every tensor -- between 4 and 16.
    (A site that rounds in one format only, or a loss scale that does not cancel, breaks this.)  Both under their default plans, fp16's extras -- centred keys,
    16-bit pre-LayerNorm sums -- included.  Eval positions 1 and 64: at 129 the decoder's bias gradients sum three rounded rows per dataset, and the ratio of two
    error norms over 60 roundings scatters by more than the factor 2 this window allows (measured 23 at e128-L0)."""
    fp16_row = (shape, 'fp16', 'default', 'single', C.T, C.SEPS, 0.0)
    sd, x, y = _inputs(fp16_row)
    H, borders = C.dims(shape, 'fp16')[1], sd['criterion.borders']
    for sep in (1, 64):
        _, _, g0 = O.loss_and_grads(sd, x, y, y, sep, H, borders)
        _, _, gb = O.loss_and_grads(sd, x, y, y, sep, H, borders, rounding=O.Rounding('bf16'))
        _, _, gf = O.loss_and_grads(sd, x, y, y, sep, H, borders, rounding=O.Rounding('fp16'))
        for k in g0:
            if g0[k].abs().max() > 0:
                ratio = C.relerr(gb[k], g0[k]) / C.relerr(gf[k], g0[k])
                assert 4 < ratio < 16, (sep, k, ratio)
