"""Times the class-label embedding (csrc/class_embed.hip, hipops.class_embed) at the few-shot notebook's shape -- B 1000, T 26, F 784, E 1024, C 5, sep 25 -- in
fp16 and f32, against the PyTorch embedding of custom encoders (`fuse_class_embedding = False`: nn.Linear on the vendor BLAS, the nn.Embedding lookup, torch.cat
and autograd's backward), which is what such a model ran before:

  1. the op alone, forward and forward + backward;
  2. one whole training step of the notebook's model (emsize 1024, nhead 4, nhid 2048, 6 layers; cross-entropy on the test row, FusedClipAdam), both ways.

The two arms alternate inside one process; a figure is the median over `--rounds` rounds (>= 5) of `--reps` calls between two device events, with the smallest and
largest round beside it.  Also recorded: the largest difference between the two arms' outputs and gradients at this shape, the embedding's share of the step
before and after, and the op's rate against the MFMA roof for the FLOPs the result needs (2 M F E forward; the same again backward -- the weight gradient; no
arm computes a gradient for x).  No ratio is promised anywhere: what comes out is what is written.

    python tools/bench_class_embed.py [--out profiles/r21_class_embed.json] [--rounds 5] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from transformerscandobayesianinference_amd import encoders, hipops      # noqa: E402
from transformerscandobayesianinference_amd.optim import FusedClipAdam      # noqa: E402
from transformerscandobayesianinference_amd.priors import stroke      # noqa: E402
from transformerscandobayesianinference_amd.transformer import TransformerModel      # noqa: E402

MFMA_ROOF = {'fp16': 2516.6e12, 'f32': 157.3e12}      # FLOP/s, dense: v_mfma_f32_32x32x16_f16 and v_mfma_f32_32x32x2_f32 on 256 CUs at 2.4 GHz
B, T, F, E, C, SEP, NHEAD, NHID, NLAYERS = 1000, 26, 784, 1024, 5, 25, 4, 2048, 6


def window(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps      # ms


def alternate(arms, rounds, reps):
    """{name: dict(median_ms, min_ms, max_ms, rounds)}: every round times each arm once, in turn."""
    for fn in arms.values():      # code objects, BLAS algorithm choice, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    seen = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            seen[k].append(window(fn, reps))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), rounds=v) for k, v in seen.items()}


def torch_embedding(x, y, enc, emb, sep):
    """The four lines of TransformerModel.forward for custom encoders (reference transformer.py:68-74)."""
    x_emb, y_emb = enc(x), emb(y.unsqueeze(-1))
    return torch.cat([x_emb[:sep] + y_emb[:sep], x_emb[sep:]], 0)


def bench_op(x, y, precision, rounds, reps):
    dev = x.device
    torch.manual_seed(1)
    enc, emb = torch.nn.Linear(F, E).to(dev), encoders.CanEmb(1, C, E).to(dev)
    dsrc = 1e-4 * torch.randn(T, B, E, device=dev)
    params = (enc.weight, enc.bias, emb.weight)

    def fused_fwd():
        with torch.no_grad():
            return hipops.class_embed(x, y, *params, SEP, precision)

    def torch_fwd():
        with torch.no_grad():
            return torch_embedding(x, y, enc, emb, SEP)

    def both(make):
        for p in params:
            p.grad = None
        src = make()
        src.backward(dsrc)
        return src.detach(), [p.grad.clone() for p in params]
    fused = lambda: both(lambda: hipops.class_embed(x, y, *params, SEP, precision))
    torch_ = lambda: both(lambda: torch_embedding(x, y, enc, emb, SEP))
    out = dict(forward=alternate({'fused': fused_fwd, 'torch': torch_fwd}, rounds, reps), forward_backward=alternate({'fused': fused, 'torch': torch_}, rounds, reps))
    # faster and different is not faster: the two arms on the same inputs, per tensor, over the PyTorch arm's largest magnitude
    (sf, gf), (st, gt) = fused(), torch_()
    diff = lambda a, b: float((a - b).abs().max() / b.abs().max())
    out['difference_fused_vs_torch'] = dict(src=diff(sf, st), encoder_weight_grad=diff(gf[0], gt[0]), encoder_bias_grad=diff(gf[1], gt[1]), table_grad=diff(gf[2], gt[2]))
    flops = 2.0 * T * B * F * E
    for name, work in (('forward', flops), ('forward_backward', 2 * flops)):
        for arm in ('fused', 'torch'):
            rate = work / (out[name][arm]['median_ms'] * 1e-3)
            out[name][arm].update(flop=work, flop_per_s=rate, share_of_mfma_roof=rate / MFMA_ROOF[precision])
    return out


def bench_step(x, y, target, precision, rounds, reps):
    dev = x.device

    def build(fuse):
        torch.manual_seed(0)
        m = TransformerModel(encoders.Linear(F, E), C, E, NHEAD, NHID, NLAYERS, 0.0, y_encoder=encoders.get_Canonical(C)(1, E), precision=precision)
        with torch.no_grad():
            for layer in m.transformer_encoder.layers:
                layer.linear2.weight.normal_(0, 0.02)
                layer.self_attn.out_proj.weight.normal_(0, 0.02)
        m.fuse_class_embedding = fuse
        m = m.to(dev).train()
        return m, FusedClipAdam(m, lr=1e-5)
    models = {'fused': build(True), 'torch': build(False)}
    tgt = target[SEP:].reshape(-1)
    losses = {}

    def step(name):
        m, opt = models[name]
        logits = m((x, y), single_eval_pos=SEP)
        loss = Fn.cross_entropy(logits.reshape(-1, C), tgt)
        loss.backward()
        opt.step(zero_grad=True)
        losses[name] = loss.detach()
    out = alternate({k: (lambda k=k: step(k)) for k in models}, rounds, reps)
    out['last_loss'] = {k: float(v) for k, v in losses.items()}
    out['class_embedding_status'] = list(models['fused'][0].class_embedding_status())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r21_class_embed.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--step-reps', type=int, default=3)
    ap.add_argument('--precisions', nargs='*', default=['fp16', 'f32'])
    args = ap.parse_args()
    assert args.rounds >= 5, 'the median of at least five rounds'
    if not torch.cuda.is_available():
        raise SystemExit('bench_class_embed: no GPU is visible; a timing taken anywhere else says nothing (not measured)')
    dev = 'cuda'
    torch.manual_seed(0)
    x, y, target = stroke.get_batch(B, T, num_features=F, num_outputs=C, only_train_for_last_idx=True, normalize_x=True, device=dev, seed=1)
    result = dict(device=torch.cuda.get_device_name(0), shape=dict(B=B, T=T, F=F, E=E, C=C, sep=SEP, nhead=NHEAD, nhid=NHID, nlayers=NLAYERS),
                  rounds=args.rounds, reps=args.reps, step_reps=args.step_reps, mfma_roof_flop_per_s=MFMA_ROOF,
                  torch_arm='fuse_class_embedding = False: nn.Linear (vendor BLAS) + nn.Embedding + torch.cat under autograd', precisions={})
    for precision in args.precisions:
        op = bench_op(x, y, precision, args.rounds, args.reps)
        step = bench_step(x, y, target, precision, args.rounds, args.step_reps)
        share = {arm: op['forward_backward'][arm]['median_ms'] / step[arm]['median_ms'] for arm in ('fused', 'torch')}
        result['precisions'][precision] = dict(op=op, step=step, embedding_share_of_step=share)
        print(json.dumps({precision: dict(
            op_forward_ms={a: op['forward'][a]['median_ms'] for a in ('fused', 'torch')}, op_forward_backward_ms={a: op['forward_backward'][a]['median_ms'] for a in ('fused', 'torch')},
            step_ms={a: step[a]['median_ms'] for a in ('fused', 'torch')}, embedding_share_of_step=share, difference=op['difference_fused_vs_torch'])}))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(result, open(args.out, 'w'), indent=1)      # (after every precision: a later one that runs out of time loses nothing)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
