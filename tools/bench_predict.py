"""Condition once, predict many, timed at the configs[1] model shape (18 features, emsize 512, 4 heads, nhid 1024, 6 layers, 1000 bars), sep = 2000:
one inference forward at sep + n rows, `condition` once, `predict` repeated -- for n in {1, 16, 256, 2048}, B in {1, 64}, exact-f32 inference and fp16.
HIP events around the calls; one JSON line per (format, B, n) and a last line with the summary.
    python tools/bench_predict.py [--quick] [--reps R] [--no-split] [--grad]
--quick: B = 1, n in {1, 16} only (the rocprofv3 kernel-trace run); --no-split: PFN_TUNE_ATTN_CACHE_SPLITS = 1 (one pass over the keys, no merge).
--grad: the input gradient at B = 64, n = 256 instead: predict_saved + predict_backward (pfn_stack_predict_backward) against predict, and against the only
alternative without them, a full forward + backward over sep + n rows with x requiring grad (which runs the training-precision kernels, fp16)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from transformerscandobayesianinference_amd import _hip, encoders  # noqa: E402
from transformerscandobayesianinference_amd.transformer import TransformerModel  # noqa: E402

PFN_TUNE_ATTN_CACHE_SPLITS = 17
F, E, H, NHID, L, NBARS, SEP = 18, 512, 4, 1024, 6, 1000, 2000


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def model_for(fmt):
    torch.manual_seed(0)
    m = TransformerModel(encoders.Linear(F, E), NBARS, E, H, NHID, L, 0.0, y_encoder=encoders.Linear(1, E), precision='fp16',
                         eval_precision='f32' if fmt == 'f32' else 'fp16')
    with torch.no_grad():
        for layer in m.transformer_encoder.layers:
            for t in (layer.linear2.weight, layer.self_attn.out_proj.weight):
                t.normal_(0, 0.03)
    return m.cuda().eval()


def splits(B, n, prec):
    """the rule of csrc/attention.hip attn_cache_splits, restated for the record (the library does not export it)"""
    D = E // H
    w16 = prec != _hip.PREC_F32
    qblk, kvb = (256, 64) if (w16 and D <= 128) else (128, 32)
    wgs = -(-n // qblk) * H * B * (2 if (not w16 and D == 256) else 1)
    return 1 if wgs >= 256 else max(1, min(512 // wgs, -(-SEP // kvb)))


def grad_rows(reps):
    B, n = 64, 256
    rows = []
    for fmt in ('fp16', 'f32'):
        model = model_for(fmt)
        g = torch.Generator().manual_seed(B)
        x = torch.randn(SEP + n, B, F, generator=g).cuda()
        y = torch.randn(SEP + n, B, generator=g).cuda()
        R = torch.randn(n, B, NBARS, generator=g).cuda()
        with torch.no_grad():
            ctx = model.condition((x[:SEP], y[:SEP]))
            pred_ms = timed(lambda: model.predict(ctx, x[SEP:]), reps)
        xt = x[SEP:].clone().requires_grad_(True)
        saved_ms = timed(lambda: model.predict(ctx, xt), reps)

        def fwd_bwd():
            out = model.predict(ctx, xt)
            torch.autograd.grad(out, xt, R)
        grad_ms = timed(fwd_bwd, reps)
        xf = x.clone().requires_grad_(True)

        def full():
            out = model((xf, y), single_eval_pos=SEP)
            torch.autograd.grad(out, xf, R)
        full_ms = timed(full, max(2, reps // 2))
        backward_ms = grad_ms - saved_ms
        r = dict(format=fmt, B=B, n=n, sep=SEP, predict_ms=pred_ms, predict_saved_ms=saved_ms, predict_backward_ms=backward_ms,
                 saved_plus_backward_ms=grad_ms, backward_over_predict=backward_ms / pred_ms, full_forward_backward_ms=full_ms,
                 full_over_saved_plus_backward=full_ms / grad_ms)
        rows.append(r)
        print(json.dumps(r), flush=True)
        del ctx, model
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-split', action='store_true')
    ap.add_argument('--grad', action='store_true')
    args = ap.parse_args()
    if args.no_split:
        _hip.check(_hip.lib().pfn_set_tuning(PFN_TUNE_ATTN_CACHE_SPLITS, 1), 'pfn_set_tuning')
    if args.grad:
        rows = grad_rows(args.reps)
        print(json.dumps(dict(summary='bench_predict --grad', no_split=args.no_split, rows=len(rows), device=torch.cuda.get_device_name(0))), flush=True)
        return
    ns = (1, 16) if args.quick else (1, 16, 256, 2048)
    Bs = (1,) if args.quick else (1, 64)
    fmts = ('f32', 'fp16')
    rows = []
    for fmt in fmts:
        model = model_for(fmt)
        prec = _hip.PREC_F32 if fmt == 'f32' else _hip.PREC_FP16
        for B in Bs:
            g = torch.Generator().manual_seed(B)
            x = torch.randn(SEP + max(ns), B, F, generator=g).cuda()
            y = torch.randn(SEP + max(ns), B, generator=g).cuda()
            with torch.no_grad():
                cond_ms = timed(lambda: model.condition((x[:SEP], y[:SEP])), max(2, args.reps // 2))
                ctx = model.condition((x[:SEP], y[:SEP]))
                for n in ns:
                    xs, ys = x[:SEP + n], y[:SEP + n]
                    fwd_ms = timed(lambda: model((xs, ys), single_eval_pos=SEP), max(2, args.reps // 2)) if not args.quick else None
                    pred_ms = timed(lambda: model.predict(ctx, xs[SEP:]), args.reps)
                    ns_ = 1 if args.no_split else splits(B, n, prec)
                    r = dict(format=fmt, B=B, n=n, sep=SEP, forward_ms=fwd_ms, condition_ms=cond_ms, predict_ms=pred_ms,
                             forward_over_predict=(fwd_ms / pred_ms) if fwd_ms else None, attn_splits=ns_,
                             context_mb=ctx.buffer.numel() / 2 ** 20, cache_bytes_per_layer=B * SEP * 2 * E * (4 if fmt == 'f32' else 2))
                    rows.append(r)
                    print(json.dumps(r), flush=True)
            del ctx
        del model
        torch.cuda.empty_cache()
    print(json.dumps(dict(summary='bench_predict', no_split=args.no_split, rows=len(rows),
                          device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == '__main__':
    main()
