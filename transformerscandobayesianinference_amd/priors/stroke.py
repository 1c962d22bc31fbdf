"""The stroke prior of the few-shot study (reference priors/stroke.py): every dataset has `num_outputs` classes, a class is one to three straight strokes,
an image of a class is those strokes shifted, jittered, drawn with a random width, filled with noise and blurred.  The reference draws every glyph with
Pillow on the host (:47-60) from a Python loop over datasets and positions (:95-110); here one call of the C ABI draws the batch on the GPU
(csrc/stroke_prior.hip, hipops.stroke_prior_sample), pixel for pixel what Pillow draws from the same parameters.  Only the labels are made with torch ops.

The notebook's call (FewShotOmniglot.ipynb):
    train(priors.stroke.DataLoader, Losses.ce, encoders.Linear, y_encoder_generator=encoders.get_Canonical(5), bptt=26, single_eval_pos_gen=25, emsize=1024,
          extra_prior_kwargs_dict={'num_features': 784, 'num_outputs': 5, 'only_train_for_last_idx': True, ...})
"""
import math
import random
from os import listdir, path

import torch

from transformerscandobayesianinference_amd import _hip, hipops
from transformerscandobayesianinference_amd.priors.utils import get_batch_to_dataloader

_call_counter = [0]


def integer_bounds(size, min_max_strokes=(1, 3), min_max_len=(5 / 28, 20 / 28), min_max_start=(2 / 28, 25 / 28), min_max_width=(1 / 28, 4 / 28), max_offset=4 / 28,
                   max_target_offset=2 / 28):
    """The inclusive integer ranges the prior draws from, by the reference's own arithmetic (:13-16, :49-54): int(size * fraction), truncating towards zero --
    so the lower offset bound int(-size * max_offset) is minus the upper one, not its floor."""
    return dict(strokes=(int(min_max_strokes[0]), int(min_max_strokes[1])), len=(int(size * min_max_len[0]), int(size * min_max_len[1])),
                start=(int(size * min_max_start[0]), int(size * min_max_start[1])), width=(int(size * min_max_width[0]), int(size * min_max_width[1])),
                offset=(int(-size * max_offset), int(size * max_offset)), jitter=(int(-size * max_target_offset), int(size * max_target_offset)))


def image_size(num_features):
    size = math.isqrt(num_features)
    assert size * size == num_features, 'num_features needs to be the square of an integer.'
    return size


def draw_labels(batch_size, seq_len, num_outputs, only_train_for_last_idx=False, device='cpu', generator=None):
    """(labels [B, T] int64, targets [B, T] int64) with torch ops on `device` (reference :97-105).  With only_train_for_last_idx every class appears
    (seq_len - 1) / num_outputs times among the first seq_len - 1 positions, in a uniform shuffle, the last label is uniform, and only it is a target (-100
    elsewhere); otherwise labels are i.i.d. uniform and all of them targets."""
    if only_train_for_last_idx:
        assert (seq_len - 1) % num_outputs == 0
        balanced = (torch.arange(seq_len - 1, device=device) % num_outputs).expand(batch_size, seq_len - 1)
        shuffle = torch.rand(batch_size, seq_len - 1, device=device, generator=generator).argsort(1)      # one uniform permutation per dataset
        last = torch.randint(0, num_outputs, (batch_size, 1), device=device, generator=generator)
        labels = torch.cat([torch.gather(balanced, 1, shuffle), last], 1)
        targets = torch.full_like(labels, -100)
        targets[:, -1] = labels[:, -1]
        return labels, targets
    labels = torch.randint(0, num_outputs, (batch_size, seq_len), device=device, generator=generator)
    return labels, labels


def get_batch(batch_size, seq_len, num_features=None, noisy_std=None, only_train_for_last_idx=False, normalize_x=False, num_outputs=2, use_saved_from=None,
              device='cuda:0', seed=None, **kwargs):      # num_features = 28 * 28 = 784
    """(x [T, B, F] f32, y [T, B] int64, target_y [T, B] int64) on `device`.  kwargs: the reference's min_max_strokes, min_max_len, min_max_start,
    min_max_width, max_offset, max_target_offset (fractions of the image size).  The draw is seeded from torch's global seed plus a per-call counter, or
    from `seed`."""
    if use_saved_from is not None:
        directory = path.join(use_saved_from, f'len_{seq_len}_out_{num_outputs}_features_{num_features}_bs_{batch_size}')
        filename = random.choice(listdir(directory))
        return torch.load(path.join(directory, filename))
    size = image_size(num_features)
    if only_train_for_last_idx:
        assert (seq_len - 1) % num_outputs == 0
    bounds = integer_bounds(size, **kwargs)
    hipops.stroke_check(size, bounds['strokes'][1], bounds['width'][1], num_outputs)
    if torch.device(device).type != 'cuda':
        raise _hip.HipExtensionError(f'the stroke prior is drawn on the GPU only (got device {device}); no CPU fallback')
    labels, targets = draw_labels(batch_size, seq_len, num_outputs, only_train_for_last_idx, device)
    if seed is None:
        seed = torch.initial_seed()
    _call_counter[0] += 1
    r = hipops.stroke_prior_sample(labels.to(torch.int32).contiguous(), size, bounds, num_outputs, seed, offset=_call_counter[0], normalize=normalize_x)
    return r['x'], labels.t().contiguous(), targets.t().contiguous()


DataLoader = get_batch_to_dataloader(get_batch)
DataLoader.num_outputs = 2
