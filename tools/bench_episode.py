"""Times the Omniglot episode loader (csrc/episode.hip, hipops.episode_sample / episode_gather) at the few-shot notebook's shapes -- B 1000 (get_acc) and B 100
(fine-tuning), T 26, size 28, 5-way 5-shot -- over a synthetic bank of the real data set's extent (1623 x 20 x 28^2) in both bank formats: ms per
episode_sample call, ms of the image kernel alone (episode_gather of the same images into a preallocated x), and its bytes (x written plus bank read) per
second beside the rate measured for plain stores on this chip (6.0-6.2 TB/s, profiles/r19_stroke_prior.json).  The arms are alternated in one process; the
figures are the median and the minimum of `--rounds` rounds.  The numpy restatement's loop (tests/episode_ref.py) over the same number of images on one host
core is timed once and quoted beside.  There is no earlier implementation here, so no ratio to one is claimed.  Also records the chi-square values of
tests/test_gpu_episode.py's distribution test from the device's own draws.

    python tools/bench_episode.py [--out profiles/r22_episode.json] [--reps 200] [--rounds 5]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import episode_ref as E      # noqa: E402

from transformerscandobayesianinference_amd import hipops      # noqa: E402
from transformerscandobayesianinference_amd.priors import omniglot      # noqa: E402

HBM_WRITE_ROOF = 6.1e12      # bytes/s: plain stores, measured on an MI355X (the chip's data-sheet rate is 8.0e12)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps      # ms


def host_loop(values, B, n_way, k_shot, size):
    """One step of the standard style with translations, the reference's way, through the restatement on one host core: seconds."""
    C, n_img = values.shape[0], values.shape[1]
    t0 = time.perf_counter()
    for _ in range(B):
        classes = random.sample(range(1200), n_way)
        support, query = [], []
        for c in classes:
            picked, k = random.sample(range(n_img), k_shot + 1), random.randint(0, 3)
            support += [np.rot90(values[c, i], k, axes=(-2, -1)) for i in picked[:k_shot]]
            query.append(np.rot90(values[c, picked[k_shot]], k, axes=(-2, -1)))
        random.shuffle(support)
        for rot in support + query[:1]:
            (xlo, xhi), (ylo, yhi) = E.shift_range(E.bounding_box(rot), size)
            E.shifted(rot, random.randint(xlo, xhi), random.randint(ylo, yhi))
    assert C >= 1200
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r22_episode.json'))
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_episode: no GPU is visible; a timing taken anywhere else says nothing (not measured)')
    dev, size, n_way, k_shot, C, n_img = 'cuda', 28, 5, 5, 1623, 20
    T, px = n_way * k_shot + 1, size * size
    raw = E.synthetic_bank(C, n_img, size, 0)
    values = E.TABLE[raw]
    banks = {'uint8': omniglot.ImageBank.from_arrays(raw, E.TABLE, 1200, device=dev), 'f32': omniglot.ImageBank.from_arrays(values, None, 1200, device=dev)}
    arms = {}
    for B in (1000, 100):
        for form, bank in banks.items():
            r = hipops.episode_sample(bank, B, n_way, k_shot, 'standard', True, True, 1, offset=2)
            src, shift = r['src'].reshape(-1), r['shift'].reshape(-1, 2)
            rot = torch.gather(r['rotations'], 1, r['labels'].long()).reshape(-1).contiguous()
            out = torch.empty(B * T, px, device=dev)
            again = hipops.episode_gather(bank, src, rot, shift, out=out, check=False, want_status=False)
            assert torch.equal(again['x'].view(B, T, px).transpose(0, 1), r['x'])      # the timed kernel computes what the sampler returned
            arms[f'B{B}_{form}_sample'] = lambda bank=bank, B=B: hipops.episode_sample(bank, B, n_way, k_shot, 'standard', True, True, 1, offset=2)
            arms[f'B{B}_{form}_image_kernel'] = lambda bank=bank, src=src, rot=rot, shift=shift, out=out: hipops.episode_gather(bank, src, rot, shift, out=out, check=False, want_status=False)
    times = {name: [] for name in arms}
    for _ in range(args.rounds):      # the arms alternate: one round times every arm once
        for name, fn in arms.items():
            times[name].append(timed(fn, args.reps))
    result = dict(device=torch.cuda.get_device_name(0), size=size, T=T, n_way=n_way, k_shot=k_shot, bank=[C, n_img, size, size], rounds=args.rounds, reps=args.reps,
                  hbm_write_roof_bytes_per_s=HBM_WRITE_ROOF, method='device events around reps calls, arms alternated in one process, median and min of the rounds',
                  sample_call_includes='the draw kernel, the image kernel, the status kernel and the allocation of nine outputs',
                  image_kernel_includes='the image kernel and the allocation of bbox and shift', shapes={})
    for B in (1000, 100):
        entry = dict(images=B * T)
        for form in banks:
            ms, ms_k = times[f'B{B}_{form}_sample'], times[f'B{B}_{form}_image_kernel']
            moved = B * T * px * (4 + (1 if form == 'uint8' else 4))
            entry[form] = dict(sample_call_ms_median=statistics.median(ms), sample_call_ms_min=min(ms), image_kernel_ms_median=statistics.median(ms_k),
                               image_kernel_ms_min=min(ms_k), image_kernel_bytes=moved, image_kernel_bytes_per_s=moved / (statistics.median(ms_k) * 1e-3),
                               image_kernel_share_of_write_roof=moved / (statistics.median(ms_k) * 1e-3) / HBM_WRITE_ROOF,
                               images_per_s=B * T / (statistics.median(ms) * 1e-3))
        entry['restatement_host_loop_s'] = host_loop(values, B, n_way, k_shot, size)
        entry['restatement_host_loop_over_sample_call_uint8'] = entry['restatement_host_loop_s'] / (entry['uint8']['sample_call_ms_median'] * 1e-3)
        result['shapes'][f'B{B}'] = entry
        print(json.dumps({f'B{B}': entry}))
    k = E.DIST
    bank = omniglot.ImageBank.from_arrays(E.distribution_bank(), E.TABLE, k['n_train'], k['train_offsets'], k['test_offsets'], device=dev)
    calls = [hipops.episode_sample(bank, k['B'], k['n_way'], k['k_shot'], mode, train, True, k['seed'], offset=offset) for mode, train, offset in E.DIST_CALLS]
    stats = E.distribution_statistics(*[{key: v.cpu().numpy() for key, v in r.items() if key != 'x'} for r in calls])
    result['distribution_test'] = dict(seed=k['seed'], B=k['B'], p={name: float(p) for name, (_, p) in stats.items()}, smallest_p=float(min(p for _, p in stats.values())))
    print(json.dumps(result['distribution_test']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, 'w'), indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
