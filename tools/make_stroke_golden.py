"""Records tests/golden/stroke_pillow.pt: what Pillow draws for hand-picked and random stroke sets (part a) and what the reference's own stroke prior
draws, with every random draw it made logged (part b).  Needs Pillow; part (b) also needs a checkout of the reference (--reference DIR), whose
priors/stroke.py is loaded by path and RUN, never copied: torchvision's ToTensor is stubbed by "array / 255" and the package's __init__ is not executed.
Only integer and float arrays go into the file.

    python tools/make_stroke_golden.py --reference /path/to/reference [--out tests/golden/stroke_pillow.pt]

Part (a), per image size: segs [n,8,4], n_strokes [n], width [n], raw [n,size^2] (the noise byte under every lit pixel, 0 elsewhere), img [n,size^2] (Pillow's
GaussianBlur(0.2) of raw), contract_differs [n] (the restatement lights other pixels when an edge's x is rounded once, as an FMA would: the strokes that tell a
contracted kernel from a correct one).  The noise of an unlit pixel never reaches an image, so it is not stored: tests rebuild a full field with a
fixed filler (stroke_ref.noise_field), under which a wrongly lit pixel shows.
Part (b): the class tuples, labels, per-image draws, noise fields, blurred bytes and x (normalize_x off and on) of 3 datasets x 11 positions x 5 classes."""
import argparse
import importlib.util
import math
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image, ImageDraw, ImageFilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import stroke_ref as R      # noqa: E402

SIZES = (8, 28, 31, 64)
HAND_PICKED_STRIDE = {8: 2, 28: 1, 31: 3}
RANDOM_PER_SIZE = {8: 100, 28: 20, 31: 10, 64: 2}
FLAGGED_PER_SIZE = {8: 0, 28: 10, 31: 4, 64: 2}


def pillow_image(size, segs, n, width, noise):
    im = Image.fromarray(np.zeros((size, size), dtype=np.uint8))
    draw = ImageDraw.Draw(im)
    for s in range(n):
        draw.line([int(c) for c in segs[s]], fill=128, width=int(width))
    a = np.array(im)
    raw = np.where(a == 128, noise.reshape(size, size), 0).astype(np.uint8)
    return raw, np.array(Image.fromarray(raw).filter(ImageFilter.GaussianBlur(.2)))


def hand_picked(size):
    m = size - 1
    h = size // 2
    lines = {'horizontal': (1, h, m - 1, h), 'vertical': (h, 1, h, m - 1), 'diagonal': (1, 1, m - 1, m - 1), 'antidiagonal': (m - 1, 1, 1, m - 1),
             'shallow': (0, 2, m, 4), 'steep': (2, m, 4, 0), 'reversed shallow': (m, 3, 0, 1), 'point': (h, h, h, h), 'corner point': (0, 0, 0, 0),
             'partly off': (-4, h - 2, h, m + 5), 'off the right': (h, 2, size + 6, 5), 'wholly off': (-9, -3, -2, -8), 'wholly off below': (1, size + 2, m, size + 4),
             'point off': (-1, 3, -1, 3), 'full row': (0, h, m, h), 'full column': (h, 0, h, m), 'beyond both ends': (-5, 3, size + 5, 3)}
    if size == 64:      # (8 KB an image: only what this size alone can show)
        return [([lines['full row']], 1), ([lines['full row']], 2), ([lines['full row']], 64), ([lines['full column']], 1), ([lines['full column']], 3),
                ([lines['diagonal']], 1), ([lines['diagonal']], 4), ([lines['full column'], lines['full row']], 5)]
    cases = []
    for i, seg in enumerate(lines.values()):
        for width in (0, 1, 2, 3, 4) if i < 3 else (1, 2, 3, 4):
            cases.append(([seg], width))
    cases.append(([lines['shallow']], 7))
    cases.append(([lines['diagonal']], 7))
    cases.append(([lines['diagonal'], lines['antidiagonal'], lines['horizontal']], 3))      # three overlapping strokes
    cases.append(([lines['shallow'], lines['steep'], lines['vertical']], 1))
    cases.append(([], 2))      # no stroke at all
    cases.append(([lines['horizontal']] * 8, 2))      # the most strokes an image may have
    return cases[::HAND_PICKED_STRIDE[size]]


def part_a(size, rng):
    cases = hand_picked(size)
    n_random, n_flagged = RANDOM_PER_SIZE[size], FLAGGED_PER_SIZE[size]
    flagged = 0
    while n_random > 0 or flagged < n_flagged:
        n = int(rng.integers(1, 4))
        width = int(rng.integers(0, 5))
        segs = [tuple(int(c) for c in rng.integers(-4, size + 4, 4)) for _ in range(n)]
        differs = (R.image_mask(size, segs, n, width, contract=True) != R.image_mask(size, segs, n, width)).any()
        if differs and flagged < n_flagged:
            flagged += 1
            cases.append((segs, width))
        elif n_random > 0:
            n_random -= 1
            cases.append((segs, width))
    out = dict(segs=np.zeros((len(cases), R.MAX_STROKES, 4), dtype=np.int32), n_strokes=np.zeros(len(cases), dtype=np.int32), width=np.zeros(len(cases), dtype=np.int32),
               raw=np.zeros((len(cases), size * size), dtype=np.uint8), img=np.zeros((len(cases), size * size), dtype=np.uint8),
               contract_differs=np.zeros(len(cases), dtype=bool))
    for i, (segs, width) in enumerate(cases):
        n = len(segs)
        out['segs'][i, :n] = np.asarray(segs, dtype=np.int32).reshape(n, 4)
        out['n_strokes'][i], out['width'][i] = n, width
        noise = rng.integers(R.NOISE_LO, R.NOISE_LO + R.NOISE_N, size * size).astype(np.uint8)
        raw, img = pillow_image(size, out['segs'][i], n, width, noise)
        out['raw'][i], out['img'][i] = raw.reshape(-1), img.reshape(-1)
        # the restatement is checked where it is recorded
        assert (R.raw_image(size, out['segs'][i], n, width, noise) == raw).all() and (R.blur(raw) == img).all(), (size, segs, width)
        assert (R.raw_image(size, out['segs'][i], n, width, R.noise_field(raw)) == raw).all()
        out['contract_differs'][i] = (R.image_mask(size, out['segs'][i], n, width, contract=True) != (raw != 0)).any()
    return {k: torch.from_numpy(v) for k, v in out.items()}


# ---- part (b): the reference's own get_batch, its draws logged ----------------------------------------------------------------------------------------------
def load_reference_stroke(reference):
    """priors/stroke.py of the checkout as a module of a stand-in package: its relative import of `.utils` and its torchvision import meet stubs."""
    tv = types.ModuleType('torchvision')
    tvt = types.ModuleType('torchvision.transforms')

    class ToTensor:
        def __call__(self, image):      # an 8-bit image as f32 in [0, 1], channel first: array / 255
            return torch.from_numpy(np.array(image)).to(torch.float32).div(255).unsqueeze(0)
    tvt.ToTensor, tvt.ToPILImage, tv.transforms = ToTensor, object, tvt
    pkg = types.ModuleType('reference_priors')
    pkg.__path__ = []
    utils = types.ModuleType('reference_priors.utils')
    utils.get_batch_to_dataloader = lambda get_batch: types.SimpleNamespace(get_batch_method=get_batch)
    sys.modules.update({'torchvision': tv, 'torchvision.transforms': tvt, 'reference_priors': pkg, 'reference_priors.utils': utils})
    spec = importlib.util.spec_from_file_location('reference_priors.stroke', os.path.join(reference, 'priors', 'stroke.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules['reference_priors.stroke'] = mod
    spec.loader.exec_module(mod)
    return mod


class DrawLog:
    """Wraps random.randint, random.random and np.random.randint while active; every call is logged as (name, arguments, value)."""

    def __enter__(self):
        self.log = []
        self.saved = (random.randint, random.random, np.random.randint)

        def randint(a, b):
            v = self.saved[0](a, b)
            self.log.append(('randint', (a, b), v))
            return v

        def rnd():
            v = self.saved[1]()
            self.log.append(('random', (), v))
            return v

        def np_randint(*args, **kwargs):
            v = self.saved[2](*args, **kwargs)
            self.log.append(('np_randint', args, v))
            return v
        random.randint, random.random, np.random.randint = randint, rnd, np_randint
        return self

    def __exit__(self, *exc):
        random.randint, random.random, np.random.randint = self.saved


def part_b(reference, size=28, B=3, T=11, C=5):
    mod = load_reference_stroke(reference)
    runs = {}
    for normalize in (False, True):
        random.seed(20260), np.random.seed(20260), torch.manual_seed(20260)
        with DrawLog() as dl:
            x, y, target = mod.get_batch(B, T, num_features=size * size, only_train_for_last_idx=True, normalize_x=normalize, num_outputs=C)
        runs[normalize] = (x, y, target, dl.log)
    (x_off, y, target, log), (x_on, y_on, _, log_on) = runs[False], runs[True]
    assert torch.equal(y, y_on) and len(log) == len(log_on) and all(a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) for a, b in zip(log, log_on))
    bounds = R.int_bounds(size)
    it = iter(log)

    def randint(lo, hi):
        name, args, v = next(it)
        assert name == 'randint' and args == (lo, hi), (name, args, lo, hi)
        return v

    def rand_angle():
        name, _, v = next(it)
        assert name == 'random'
        return v * 2 * math.pi
    rec = dict(size=size, cls_n=np.zeros((B, C), dtype=np.int32), cls_len=np.zeros((B, C, 8), dtype=np.int32), cls_start=np.zeros((B, C, 8, 2), dtype=np.int32),
               cls_dir=np.zeros((B, C, 8)), labels=y.t().contiguous().numpy().astype(np.int32), targets=target.t().contiguous().numpy().astype(np.int64),
               width=np.zeros((B, T), dtype=np.int32), offset=np.zeros((B, T, 2), dtype=np.int32), jitter=np.zeros((B, T, 8, 2), dtype=np.int32),
               segs=np.zeros((B, T, 8, 4), dtype=np.int32), noise=np.zeros((B, T, size * size), dtype=np.uint8), img=np.zeros((B, T, size * size), dtype=np.uint8))
    passes = 0
    for b in range(B):
        classes = []
        for c in range(C):
            lens, starts, angles, capped = R.class_loop(size, bounds, randint, rand_angle, predraw=True)
            n = len(lens)
            assert capped == 0
            classes.append((lens, starts, angles))
            rec['cls_n'][b, c] = n
            rec['cls_len'][b, c, :n], rec['cls_start'][b, c, :n], rec['cls_dir'][b, c, :n] = lens, starts, angles
        assert randint(0, C - 1) == rec['labels'][b, T - 1]      # the last label (the others come from random.shuffle, which is not logged: y holds them)
        for t in range(T):
            lens, starts, angles = classes[rec['labels'][b, t]]
            n = len(lens)
            width = randint(*bounds['width'])
            offset = (randint(*bounds['offset']), randint(*bounds['offset']))
            jitters = [(randint(*bounds['jitter']), randint(*bounds['jitter'])) for _ in range(n)]
            name, _, noise = next(it)
            assert name == 'np_randint' and noise.shape == (size, size)
            segs, _ = R.image_segments(lens, starts, angles, offset, jitters)
            rec['width'][b, t], rec['offset'][b, t], rec['jitter'][b, t, :n], rec['segs'][b, t, :n] = width, offset, jitters, segs
            rec['noise'][b, t] = noise.reshape(-1).astype(np.uint8)
            got = x_off[t, b].numpy()
            img = np.rint(got.astype(np.float64) * 255).astype(np.uint8)
            assert (R.BYTE_TO_X[img] == got).all()
            rec['img'][b, t] = img
            # the replay through the restatement gives the reference's image
            mine = R.blur(R.raw_image(size, rec['segs'][b, t], n, width, rec['noise'][b, t]))
            assert (mine.reshape(-1) == img).all(), (b, t)
            passes += 1
    assert next(it, None) is None and passes == B * T
    rec['x'] = x_off.permute(1, 0, 2).contiguous().numpy()            # [B, T, size^2]
    rec['x_normalized'] = x_on.permute(1, 0, 2).contiguous().numpy()
    return {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in rec.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='a checkout of the reference implementation (its priors/stroke.py is run, not copied)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'stroke_pillow.pt'))
    args = ap.parse_args()
    import PIL
    rng = np.random.default_rng(19)
    a = {size: part_a(size, rng) for size in SIZES}
    b = part_b(args.reference)
    torch.save(dict(pillow_version=[int(v) for v in PIL.__version__.split('.')[:3]], strokes=a, reference=b), args.out)
    n = sum(v['width'].numel() for v in a.values())
    print(f'{args.out}: {n} stroke sets ({sum(int(v["contract_differs"].sum()) for v in a.values())} flagged), {b["img"].shape[0] * b["img"].shape[1]} reference images, '
          f'{os.path.getsize(args.out)} bytes')


if __name__ == '__main__':
    main()
