"""Operand staging of the grouped weight-gradient kernels (gemm_tn_big_kernel / gemm_tn_wide_kernel, csrc/gemm_tn.hip TnStager).

A workgroup stages its operands through one buffer descriptor per operand that it advances by a stage per step and that ends at the last token
row of its token split; rows past that end fail the descriptor's range check and arrive as zeros.  What that can get wrong: the end of the range
(a ragged last stage, a split that ends inside the tensor), the row pitch (operands that are column slices of wider tensors), the per-lane offsets
(a permuted row or column) and the bias gradient that rides on the A tiles.  Every case runs for bf16 and fp16 operands and for both wave shapes
(pfn_set_tuning key 14 = 8 / 4), against an f64 product of the same rounded operands at the bound of tests/test_gpu_ops.py::test_gemm_tn_group
(3e-6 relative: f32 accumulation order only, the products of two 16-bit operands are exact in f32).

Not reachable from the single-op entry point: TnProblem::Pv < P (A ending in zero-padding columns).  Only the stack sets it, for the decoder's
weight gradient, and the stack-level parity tests run that on a ragged token count with its bias gradient.
"""
import functools

import pytest
import torch

from transformerscandobayesianinference_amd import _hip
from transformerscandobayesianinference_amd import hipops

pytestmark = pytest.mark.gpu
BF, FP16 = _hip.PREC_BF16, _hip.PREC_FP16
SHAPES = [(256, 256), (512, 256)]      # (P, Q) of the group's problems
BOUND = 3e-6
RAGGED = [(1, 1), (63, 1), (64, 1), (65, 1), (127, 1), (129, 1), (191, 1), (257, 3), (4100, 3)]      # (M, splits)


@pytest.fixture(params=[BF, FP16], ids=['bf16', 'fp16'])
def op16(request):
    return request.param


@pytest.fixture(params=[8, 4], ids=['8-waves-128x64', '4-waves-128x128'])
def wgrad_waves(request):
    _hip.check(_hip.lib().pfn_set_tuning(14, request.param), 'pfn_set_tuning')
    yield request.param
    _hip.check(_hip.lib().pfn_set_tuning(14, 8), 'pfn_set_tuning')


def dev():
    return torch.device('cuda:0')


def relerr(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def operands(M, prec, strided):
    """[(A, B, C_ref, colsum_ref)] per problem of the group; computed once per (M, format, layout) and only read afterwards.
    strided: every operand is the column slice [:M, 256:256 + width] of an [M + 3, width + 512] tensor that is NaN everywhere else."""
    out = []
    for i, (P, Q) in enumerate(SHAPES):
        g = torch.Generator(device='cpu')
        g.manual_seed(1000 * i + M)
        ops = []
        for width in (P, Q):
            x = torch.randn(M, width, generator=g).to(dev()).to(hipops.TDT[prec])
            if strided:
                buf = torch.full((M + 3, width + 512), float('nan'), dtype=x.dtype, device=dev())
                buf[:M, 256:256 + width] = x
                x = buf[:M, 256:256 + width]
            ops.append(x)
        A, B = ops
        out.append((A, B, A.double().t() @ B.double(), A.double().sum(0)))
    return out


def run_group(ops, splits, colsum):
    probs = [(A, B, torch.zeros(A.shape[1], B.shape[1], device=dev()), torch.zeros(A.shape[1], device=dev()) if colsum else None) for A, B, _, _ in ops]
    hipops.gemm_tn_group(probs, splits)
    return probs


def check(ops, probs):
    for (A, B, rc, rs), (_, _, C, cs) in zip(ops, probs):
        e = relerr(C, rc)
        print(f'P={A.shape[1]} M={A.shape[0]} C rel. error {e:.3e}')
        assert e < BOUND, e
        if cs is not None:
            e = relerr(cs, rs)
            print(f'P={A.shape[1]} M={A.shape[0]} colsum rel. error {e:.3e}')
            assert e < BOUND, e


@pytest.mark.parametrize('M,splits', RAGGED)
def test_token_counts_and_splits(M, splits, op16, wgrad_waves):
    """every position of the last row inside a 64-token stage; split ends inside the tensor"""
    ops = operands(M, op16, False)
    check(ops, run_group(ops, splits, colsum=False))


@pytest.mark.parametrize('M,splits', [(65, 1), (191, 1), (257, 3), (4100, 1), (4100, 3)])
def test_strided_views_in_nan(M, splits, op16, wgrad_waves):
    """Column slices of wider tensors, NaN all around (the rows at and beyond M included): a read past a split's last row or with a wrong pitch
    puts NaN into C; a split that reads on into its neighbour's rows counts them twice and breaks the bound."""
    ops = operands(M, op16, True)
    probs = run_group(ops, splits, colsum=True)
    for _, _, C, cs in probs:
        assert torch.isfinite(C).all() and torch.isfinite(cs).all()
    check(ops, probs)


@pytest.mark.parametrize('M', [130, 200])
def test_exact_shifted_identity(M, op16, wgrad_waves):
    """A is a shifted identity, B holds small integers over 8: every entry of C is one element of B, so a permuted token row or column shows exactly"""
    dt = hipops.TDT[op16]
    A = torch.zeros(M, 256, dtype=dt, device=dev())
    A[torch.arange(M), (torch.arange(M) + 5) % 256] = 1
    B = (torch.arange(M * 512, device=dev()).float().view(M, 512) % 127 / 8).to(dt)
    C = torch.zeros(256, 512, device=dev())
    hipops.gemm_tn_group([(A, B, C, None)], 1)
    assert torch.equal(C, A.float().t() @ B.float())


@pytest.mark.parametrize('M,splits', [(37, 1), (130, 1), (257, 3)])
def test_bias_gradient_on_ragged_tail(M, splits, op16, wgrad_waves):
    """the column sums of A from the tiles the product stages: the zero rows behind a ragged tail add nothing"""
    ops = operands(M, op16, False)
    check(ops, run_group(ops, splits, colsum=True))


def test_repeatable(op16, wgrad_waves):
    """no token split: no atomics between workgroups of a tile, the summation order is fixed -- two runs into fresh C agree bit for bit"""
    ops = operands(4100, op16, False)
    a, b = run_group(ops, 1, colsum=False), run_group(ops, 1, colsum=False)
    for (_, _, Ca, _), (_, _, Cb, _) in zip(a, b):
        assert torch.equal(Ca, Cb)
