"""Times the stroke prior (csrc/stroke_prior.hip, priors/stroke.get_batch) at the few-shot notebook's shape (B 1000, T 26, size 28, 5 classes) and at B 64:
images/s and ms per get_batch (device events around calls that end in a synchronise), the image kernel's written bytes per second beside the HBM write rate
measured for plain stores on this chip (MI355X: 6.0-6.2 TB/s, one dword per lane; the 8 TB/s of the data sheet is not reachable), and the same number of
images drawn by a Pillow loop on the host cores of the same box, timed once.  There is no earlier implementation here, so no ratio to one is claimed; the
ratio to the Pillow loop is reported as measured.  Also records the chi-square values and the normalised-output error of tests/test_gpu_stroke.py's checks.

    python tools/bench_stroke_prior.py [--out profiles/r19_stroke_prior.json] [--reps 50]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import stroke_ref as R      # noqa: E402

from transformerscandobayesianinference_amd import hipops      # noqa: E402
from transformerscandobayesianinference_amd.priors import stroke      # noqa: E402

HBM_WRITE_ROOF = 6.1e12      # bytes/s: plain stores, measured on an MI355X (the chip's data-sheet rate is 8.0e12)


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps      # ms


def pillow_loop(B, T, size, C, bounds):
    """The same number of images through the restated class loop and Pillow, on one host core -- the reference's way (priors/stroke.py of the reference: a Python
    loop over datasets and positions)."""
    try:
        from PIL import Image, ImageDraw, ImageFilter
    except ImportError:
        return None
    import random
    t0 = time.perf_counter()
    for _ in range(B):
        classes = [R.class_loop(size, bounds, random.randint, lambda: random.random() * 2 * math.pi)[:3] for _ in range(C)]
        for _ in range(T):
            lens, starts, angles = classes[random.randint(0, C - 1)]
            width = random.randint(*bounds['width'])
            offset = (random.randint(*bounds['offset']), random.randint(*bounds['offset']))
            jitters = [(random.randint(*bounds['jitter']), random.randint(*bounds['jitter'])) for _ in lens]
            im = Image.fromarray(np.zeros((size, size), dtype=np.uint8))
            draw = ImageDraw.Draw(im)
            for seg in R.image_segments(lens, starts, angles, offset, jitters)[0]:
                draw.line(list(seg), fill=128, width=width)
            a = np.array(im)
            a[a == 128] = np.random.randint(200, 255, size=a.shape)[a == 128]
            torch.from_numpy(np.array(Image.fromarray(a).filter(ImageFilter.GaussianBlur(.2)))).to(torch.float32).div(255)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r19_stroke_prior.json'))
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--merge', nargs='*', default=[], help='JSON files (e.g. a PFN_RECORD_BOUNDS dump, a chi-square table) stored under their file names')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_stroke_prior: no GPU is visible; a timing taken anywhere else says nothing (not measured)')
    dev, size, T, C = 'cuda', 28, 26, 5
    bounds = stroke.integer_bounds(size)
    result = dict(device=torch.cuda.get_device_name(0), size=size, T=T, classes=C, hbm_write_roof_bytes_per_s=HBM_WRITE_ROOF, shapes={})
    for B in (1000, 64):
        kw = dict(num_features=size * size, num_outputs=C, only_train_for_last_idx=True, device=dev)
        ms_batch = timed(lambda: stroke.get_batch(B, T, **kw), args.reps)
        labels = stroke.draw_labels(B, T, C, True, dev)[0].to(torch.int32).contiguous()
        ms_sample = timed(lambda: hipops.stroke_prior_sample(labels, size, bounds, C, 1, offset=2), args.reps)
        r = hipops.stroke_prior_sample(labels, size, bounds, C, 1, offset=2)
        n = r['cls_n'].gather(1, labels.long()).view(-1).int().contiguous()
        segs, width, out = r['segs'].view(-1, 8, 4), r['width'].view(-1), torch.empty(B * T, size * size, device=dev)
        ms_render = timed(lambda: hipops.stroke_render(segs, n, width, size, out=out, seed=1, offset=2, check=False), args.reps)
        written = B * T * size * size * 4
        host_s = pillow_loop(B, T, size, C, bounds)
        result['shapes'][f'B{B}'] = dict(
            images=B * T, get_batch_ms=ms_batch, images_per_s=B * T / (ms_batch * 1e-3), sample_call_ms=ms_sample, sample_call_includes='the class kernel, the image kernel and the allocation of ten outputs',
            render_kernel_ms=ms_render, render_written_bytes=written, render_bytes_per_s=written / (ms_render * 1e-3),
            render_share_of_write_roof=written / (ms_render * 1e-3) / HBM_WRITE_ROOF, pillow_loop_s=host_s,
            pillow_loop_over_get_batch=None if host_s is None else host_s / (ms_batch * 1e-3))
        print(json.dumps({f'B{B}': result['shapes'][f'B{B}']}))
    for path in args.merge:
        if os.path.exists(path):
            result[os.path.splitext(os.path.basename(path))[0]] = json.load(open(path))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, 'w'), indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
