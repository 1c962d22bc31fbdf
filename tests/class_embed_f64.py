"""The class embedding of the few-shot study restated in torch, for the tests of csrc/class_embed.hip (no GPU code here):

    src[t, b, :] = Wx . x[t, b, :] + bx + (t < sep ? table[labels[t, b], :] : 0)

and its three gradients dWx = sum d(src)^T x, dbx = sum d(src), dtable[c] = sum of d(src) over the train rows of class c, written out -- no autograd -- in
whatever dtype the operands come in (f64: the reference; f32: the CPU run whose error sets the f32 bound).  A train-row label outside [0, C) selects no class
row, as the kernels treat it.  `rounded_*`: the same after x, Wx and table (and, for the backward, d(src)) went through the operand format -- fp16 d(src) under
the power-of-two loss scale the kernels take from max|d(src)| (csrc/pfn_device.h).  `error`: max |difference| over max |f64 value|, the tests' measure."""
import math

import torch

UNIT_ROUNDOFF = {'fp16': 2.0 ** -11, 'bf16': 2.0 ** -8, 'f32': 2.0 ** -24}
F32_FLOOR = 2.0 ** -23
OPERAND = {'fp16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}
LOSS_SCALE_TARGET_LOG2 = 2      # rowwise.hip g_loss_scale_target: max|d(src)| lands in [2^2, 2^3)


def onehot(labels, C, sep, dtype):
    """[S, B, C]: 1 at (t, b, labels[t, b]) for t < sep and a label inside [0, C), else 0."""
    S, B = labels.shape
    valid = (labels >= 0) & (labels < C) & (torch.arange(S)[:, None] < sep)
    out = torch.zeros(S, B, C, dtype=dtype)
    t, b = torch.nonzero(valid, as_tuple=True)
    out[t, b, labels[t, b]] = 1
    return out


def forward(x, labels, wx, bx, table, sep):
    return x @ wx.t() + bx + onehot(labels, table.shape[0], sep, x.dtype) @ table


def backward(x, labels, C, sep, dsrc):
    """(dWx [E, F], dbx [E], dtable [C, E])"""
    return (torch.einsum('sbe,sbf->ef', dsrc, x), dsrc.sum((0, 1)), torch.einsum('sbc,sbe->ce', onehot(labels, C, sep, x.dtype), dsrc))


def round_to(t, precision):
    """t through the operand format and back (fp16 saturates at +-65504, as the kernels' stores do)."""
    if precision == 'fp16':
        t = t.clamp(-65504.0, 65504.0)
    return t.to(OPERAND[precision]).to(t.dtype)


def round_scaled(dsrc, precision):
    """d(src) as the backward's GEMM reads it: fp16 under 2^k with max|d(src)| 2^k in [2^target, 2^(target + 1)), the other formats as they are."""
    amax = float(dsrc.abs().max())
    if precision != 'fp16' or amax == 0 or not math.isfinite(amax):
        return round_to(dsrc, precision)
    k = LOSS_SCALE_TARGET_LOG2 - math.floor(math.log2(amax))
    return round_to(dsrc * 2.0 ** k, precision) * 2.0 ** -k


def rounded_forward(x, labels, wx, bx, table, sep, precision):
    return forward(round_to(x, precision), labels, round_to(wx, precision), bx, round_to(table, precision), sep)


def rounded_backward(x, labels, C, sep, dsrc, precision):
    return backward(round_to(x, precision), labels, C, sep, round_scaled(dsrc, precision))


def error(got, want64):
    scale = float(want64.abs().max())
    return float((got.double() - want64).abs().max()) / scale if scale > 0 else float((got.double() - want64).abs().max())


def bound(precision, e):
    """The project's rule (README): 16-bit 3 max(e, u) with e the operand-rounded restatement's error, f32 4 max(e, 2^-23) with e the f32 CPU run's."""
    return 4 * max(e, F32_FLOOR) if precision == 'f32' else 3 * max(e, UNIT_ROUNDOFF[precision])
