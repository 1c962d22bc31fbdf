"""The Omniglot episode loader of the few-shot study (reference priors/omniglot.py with datasets/omniglotNshot.py): fine-tuning and evaluation episodes of
n_way classes x k_shot support images and one query, each class rotated by a multiple of 90 degrees (standard style) and every image shifted inside its frame
(translation augmentation).  The reference assembles a step in a numpy loop over datasets, classes and images with one torchvision affine() per image; here
the images live on the device in an ImageBank and one call of the C ABI draws the batch (csrc/episode.hip, hipops.episode_sample).

Only reading the images needs files: ImageBank.from_directory reads the reference's `processed/images_background` / `processed/images_evaluation` layout once,
on the host, with Pillow; ImageBank.from_arrays takes any array.  Nothing here downloads.

The notebook's calls (FewShotOmniglot.ipynb):
    train(priors.omniglot.DataLoader, Losses.ce, encoders.Linear, y_encoder_generator=encoders.get_Canonical(5), bptt=26, single_eval_pos_gen=25,
          load_weights_from_this_state_dict=..., extra_prior_kwargs_dict={'num_features': 784, 'num_outputs': 5, 'translations': True, 'jonas_style': True})
    priors.omniglot.DataLoader(num_steps, batch_size=1000, seq_len=26, num_features=784, num_outputs=5, train=False).validate(model)      # get_acc
"""
import math
import os

import numpy as np
import torch

from transformerscandobayesianinference_amd import _hip, hipops
from transformerscandobayesianinference_amd.priors.prior import PriorDataLoader
from transformerscandobayesianinference_amd.utils import set_locals_in_self

_call_counter = [0]
REFERENCE_TRAIN_CLASSES = 1200      # datasets/omniglotNshot.py:134: x[:num_train_classes_used] trains, x[1200:] tests


def inverted_byte_table():
    """float32(1 - b / 255.) evaluated in f64 as numpy evaluates the reference's transform chain (x / 255., then 1 - x, then astype(float32)): paper, byte 255,
    is exactly 0.0f -- the background."""
    return (1.0 - np.arange(256, dtype=np.float64) / 255.).astype(np.float32)


class ImageBank:
    """images [n_classes, n_img, size, size] on `device`: uint8 with `table` [256] f32 (a pixel's value is table[byte]) or f32 with table None; the background is
    the value 0.0.  Classes [0, n_train_classes) are the standard style's training classes, the rest its test classes.  The jonas style draws an alphabet and
    takes its first n_way classes: train_alphabet_offsets / test_alphabet_offsets [A + 1] int32 give each split's alphabets as class ranges of the bank."""

    def __init__(self, images, table, n_train_classes, train_alphabet_offsets=None, test_alphabet_offsets=None):
        self.images, self.table, self.n_train_classes = images, table, int(n_train_classes)
        self._offsets_host = {True: None if train_alphabet_offsets is None else [int(v) for v in train_alphabet_offsets],
                              False: None if test_alphabet_offsets is None else [int(v) for v in test_alphabet_offsets]}
        on = lambda o: None if o is None else torch.tensor(o, dtype=torch.int32, device=images.device)
        self.train_alphabet_offsets, self.test_alphabet_offsets = on(self._offsets_host[True]), on(self._offsets_host[False])

    n_classes = property(lambda self: self.images.shape[0])
    n_img = property(lambda self: self.images.shape[1])
    size = property(lambda self: self.images.shape[2])

    def alphabet_offsets_host(self, train):
        return self._offsets_host[bool(train)]

    @classmethod
    def from_arrays(cls, images, table=None, n_train_classes=None, train_alphabet_offsets=None, test_alphabet_offsets=None, device='cuda:0'):
        """images: array or tensor [n_classes, n_img, size, size], uint8 (with table [256]) or float.  Checks the limits of the kernels and, on the host, that
        every alphabet lies inside the bank (how many classes an alphabet must hold depends on n_way: checked per call)."""
        images = torch.as_tensor(np.ascontiguousarray(images) if isinstance(images, np.ndarray) else images)
        if images.dtype != torch.uint8:
            images = images.to(torch.float32)
        if table is not None:
            table = torch.as_tensor(np.asarray(table, dtype=np.float32) if not torch.is_tensor(table) else table).to(torch.float32).contiguous()
        if images.dim() != 4 or images.shape[2] != images.shape[3]:
            raise ValueError('images [n_classes, n_img, size, size]')
        if (images.dtype == torch.uint8) != (table is not None):
            raise ValueError('a uint8 bank needs its 256-entry f32 table, an f32 bank takes none')
        if table is not None and tuple(table.shape) != (256,):
            raise ValueError('table [256] f32')
        C = images.shape[0]
        hipops.episode_check(images.shape[2], images.shape[1], C)
        n_train = C if n_train_classes is None else int(n_train_classes)
        if not 0 <= n_train <= C:
            raise ValueError(f'n_train_classes = {n_train} outside 0 .. {C}')
        for offsets in (train_alphabet_offsets, test_alphabet_offsets):
            if offsets is not None:
                hipops.episode_check(images.shape[2], images.shape[1], C, alphabet_offsets=offsets)
        dev = torch.device(device)
        return cls(images.contiguous().to(dev), None if table is None else table.to(dev), n_train, train_alphabet_offsets, test_alphabet_offsets)

    @classmethod
    def from_directory(cls, root, imgsz, device='cuda:0', n_train_classes=None):
        """Reads <root>/processed/images_background and <root>/processed/images_evaluation (alphabet / character / *.png), once, with Pillow on the host:
        convert('L'), resize((imgsz, imgsz)) as the reference's transform chain does; the bytes are kept and the rest of the chain (x / 255., 1 - x) is the
        table.  Alphabets, characters and files are taken in sorted order, background first.  The standard style's split follows the reference: the first 1200
        classes train when the bank holds more than 1200, else the background classes do.  Never downloads."""
        from PIL import Image
        splits = [os.path.join(root, 'processed', name) for name in ('images_background', 'images_evaluation')]
        for directory in splits:
            if not os.path.isdir(directory):
                raise FileNotFoundError(f'Omniglot images not found: {directory} is no directory (expected {root}/processed/images_background and '
                                        f'images_evaluation, alphabet/character/*.png; nothing is downloaded)')
        classes, offsets = [], []
        for directory in splits:
            split_offsets = [len(classes)]
            for alphabet in sorted(os.listdir(directory)):
                a_dir = os.path.join(directory, alphabet)
                if not os.path.isdir(a_dir):
                    continue
                for character in sorted(os.listdir(a_dir)):
                    c_dir = os.path.join(a_dir, character)
                    files = sorted(f for f in os.listdir(c_dir) if f.endswith('png')) if os.path.isdir(c_dir) else []
                    if files:
                        classes.append([np.asarray(Image.open(os.path.join(c_dir, f)).convert('L').resize((imgsz, imgsz)), dtype=np.uint8) for f in files])
                split_offsets.append(len(classes))
            offsets.append(split_offsets)
        if not classes:
            raise FileNotFoundError(f'Omniglot images not found: no alphabet/character/*.png under {splits[0]} or {splits[1]}')
        counts = {len(c) for c in classes}
        if len(counts) != 1:
            raise ValueError(f'every character needs the same number of images, found {sorted(counts)}')
        n_background = offsets[0][-1]
        if n_train_classes is None:
            n_train_classes = REFERENCE_TRAIN_CLASSES if len(classes) > REFERENCE_TRAIN_CLASSES else n_background
        return cls.from_arrays(np.asarray(classes, dtype=np.uint8), inverted_byte_table(), n_train_classes, offsets[0], offsets[1], device)


def get_batch(batch_size, seq_len, num_features, num_outputs, bank, num_classes_used=REFERENCE_TRAIN_CLASSES, train=True, translations=True, jonas_style=False,
              device='cuda:0', seed=None):
    """One step: (x [T, B, F] f32, y [T, B] int64, target_y [T, B] int64) on the bank's device (`device` is what train() hands every loader; the draw happens
    where the bank lives).  The draw is seeded from torch's initial seed plus a per-call counter, or from `seed`."""
    n_way, k_shot = num_outputs, (seq_len - 1) // num_outputs
    assert bank.size * bank.size == num_features, f'the bank holds {bank.size} x {bank.size} images, num_features = {num_features}'
    if bank.images.device.type != 'cuda':
        hipops.episode_check(bank.size, bank.n_img, bank.n_classes, n_way, k_shot)
        raise _hip.HipExtensionError(f'the episode loader draws on the GPU only (the bank lives on {bank.images.device}); no CPU fallback')
    if seed is None:
        seed = torch.initial_seed()
    _call_counter[0] += 1
    r = hipops.episode_sample(bank, batch_size, n_way, k_shot, 'jonas' if jonas_style else 'standard', train, translations and train, seed,
                              offset=_call_counter[0], num_classes_used=num_classes_used)
    return r['x'], r['labels'].t().long(), r['targets'].t().long()


class DataLoader(PriorDataLoader):
    """The reference's loader (priors/omniglot.py:37-98) with its signature; `bank` (an ImageBank; default: ImageBank.from_directory(root, imgsz, device)),
    `root`, `device` and `seed` are added."""
    get_batch_method = staticmethod(get_batch)

    def __init__(self, num_steps, batch_size, seq_len, num_features, num_outputs, num_classes_used=REFERENCE_TRAIN_CLASSES, fuse_x_y=False, train=True,
                 translations=True, jonas_style=False, bank=None, root='omniglot', device='cuda:0', seed=None):
        set_locals_in_self(locals())
        assert not fuse_x_y, 'So far don\' support fusing.'
        imgsz = math.isqrt(num_features)
        assert imgsz * imgsz == num_features
        assert ((seq_len - 1) // num_outputs) * num_outputs == seq_len - 1
        if torch.device(device).type != 'cuda':
            raise _hip.HipExtensionError(f'the episode loader draws on the GPU only (got device {device}); no CPU fallback')
        if bank is None:
            self.bank = ImageBank.from_directory(root, imgsz, device)

    def __len__(self):
        return self.num_steps

    def __iter__(self):
        def step():
            x, y, target_y = get_batch(self.batch_size, self.seq_len, self.num_features, self.num_outputs, self.bank, self.num_classes_used, self.train,
                                       self.translations, self.jonas_style, self.device, self.seed)
            return (x, y), target_y
        return (step() for _ in range(self.num_steps))

    @torch.no_grad()
    def validate(self, finetuned_model, eval_pos=-1):
        """Accuracy at `eval_pos` over num_steps test batches (reference :75-98) -- the inner loader is built with train=False and, as there, the DEFAULT
        jonas_style=False whatever this loader's style is.  Logits and labels stay on the device; one host read at the end."""
        finetuned_model.eval()
        device = next(iter(finetuned_model.parameters())).device
        if not hasattr(self, 't_dl'):
            self.t_dl = DataLoader(num_steps=self.num_steps, batch_size=self.batch_size, seq_len=self.seq_len, num_features=self.num_features,
                                   num_outputs=self.num_outputs, fuse_x_y=self.fuse_x_y, train=False, bank=self.bank, device=self.device, seed=self.seed)
        ps, ys = [], []
        for x, y in self.t_dl:
            ps.append(finetuned_model(tuple(e.to(device) for e in x), single_eval_pos=eval_pos))
            ys.append(y)
        ps, ys = torch.cat(ps, 1), torch.cat(ys, 1)
        return (ps[eval_pos].argmax(-1) == ys[eval_pos].to(ps.device)).float().mean().cpu()
