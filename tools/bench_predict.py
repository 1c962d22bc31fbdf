"""Condition once, predict many, timed at the configs[1] model shape (18 features, emsize 512, 4 heads, nhid 1024, 6 layers, 1000 bars), sep = 2000:
one inference forward at sep + n rows, `condition` once, `predict` repeated -- for n in {1, 16, 256, 2048}, B in {1, 64}, exact-f32 inference and fp16.
HIP events around the calls; one JSON line per (format, B, n) and a last line with the summary.
    python tools/bench_predict.py [--quick] [--reps R] [--no-split] [--grad] [--ragged [--uniform-only] [--rounds K]]
--quick: B = 1, n in {1, 16} only (the rocprofv3 kernel-trace run); --no-split: PFN_TUNE_ATTN_CACHE_SPLITS = 1 (one pass over the keys, no merge).
--grad: the input gradient at B = 64, n = 256 instead: predict_saved + predict_backward (pfn_stack_predict_backward) against predict, and against the only
alternative without them, a full forward + backward over sep + n rows with x requiring grad (which runs the training-precision kernels, fp16).
--ragged: datasets of different sizes as one batch (condition(src, train_lengths) + predict) at B = 64, n = 256, seeded lengths spread over [200, 2000] with the
maximum 2000, fp16 and f32: (a) the ragged calls, (b) the uniform calls at sep = 2000, (d) what a user does without them, 64 x (condition + predict) at B = 1 with
every dataset's own length.  (a), (b) and (d) alternate over --rounds rounds in one process; the spread of (b) over the rounds is the noise floor the others are
read against.  --uniform-only times (b) alone and uses nothing but the uniform calls, so the same file also runs against an older library."""
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


def ragged_lengths(B, lo=200, hi=SEP, seed=0):
    v = torch.randint(lo, hi + 1, (B,), generator=torch.Generator().manual_seed(seed)).tolist()
    v[0], v[1] = lo, hi
    return v


def ragged_rows(reps, rounds, uniform_only):
    B, n = 64, 256
    lengths = ragged_lengths(B)
    rows = []

    def stats(v):
        v = sorted(v)
        med = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
        return dict(median_ms=med, min_ms=v[0], max_ms=v[-1], spread=(v[-1] - v[0]) / med, rounds=v)

    for fmt in ('fp16', 'f32'):
        model = model_for(fmt)
        g = torch.Generator().manual_seed(B)
        x = torch.randn(SEP + n, B, F, generator=g).cuda()
        y = torch.randn(SEP + n, B, generator=g).cuda()
        xt = x[SEP:]
        singles = [(x[:s, b:b + 1].contiguous(), y[:s, b:b + 1].contiguous(), xt[:, b:b + 1].contiguous()) for b, s in enumerate(lengths)]
        t = dict(a_condition=[], a_predict=[], b_condition=[], b_predict=[], d_total=[])
        with torch.no_grad():
            cu = model.condition((x[:SEP], y[:SEP]))
            cr = None if uniform_only else model.condition((x[:SEP], y[:SEP]), train_lengths=lengths)

            def per_dataset():
                for xs, ys, xq in singles:
                    model.predict(model.condition((xs, ys)), xq)
            for _ in range(rounds):
                if not uniform_only:
                    t['a_condition'].append(timed(lambda: model.condition((x[:SEP], y[:SEP]), train_lengths=lengths), max(2, reps // 2)))
                    t['a_predict'].append(timed(lambda: model.predict(cr, xt), reps))
                t['b_condition'].append(timed(lambda: model.condition((x[:SEP], y[:SEP])), max(2, reps // 2)))
                t['b_predict'].append(timed(lambda: model.predict(cu, xt), reps))
                if not uniform_only:
                    t['d_total'].append(timed(per_dataset, 2))
        r = dict(format=fmt, B=B, n=n, sep_max=SEP, lengths_min=min(lengths), lengths_max=max(lengths), lengths_mean=sum(lengths) / B,
                 uniform_condition=stats(t['b_condition']), uniform_predict=stats(t['b_predict']))
        r['uniform_total_ms'] = r['uniform_condition']['median_ms'] + r['uniform_predict']['median_ms']
        if not uniform_only:
            r.update(ragged_condition=stats(t['a_condition']), ragged_predict=stats(t['a_predict']), per_dataset_B1=stats(t['d_total']))
            r['ragged_total_ms'] = r['ragged_condition']['median_ms'] + r['ragged_predict']['median_ms']
            r['per_dataset_over_ragged'] = r['per_dataset_B1']['median_ms'] / r['ragged_total_ms']
            r['ragged_predict_over_uniform_predict'] = r['ragged_predict']['median_ms'] / r['uniform_predict']['median_ms']
        rows.append(r)
        print(json.dumps(r), flush=True)
        del cu, cr, model
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-split', action='store_true')
    ap.add_argument('--grad', action='store_true')
    ap.add_argument('--ragged', action='store_true')
    ap.add_argument('--uniform-only', action='store_true')
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    if args.no_split:
        _hip.check(_hip.lib().pfn_set_tuning(PFN_TUNE_ATTN_CACHE_SPLITS, 1), 'pfn_set_tuning')
    if args.ragged:
        rows = ragged_rows(args.reps, args.rounds, args.uniform_only)
        print(json.dumps(dict(summary='bench_predict --ragged', uniform_only=args.uniform_only, rows=len(rows), device=torch.cuda.get_device_name(0))), flush=True)
        return
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
