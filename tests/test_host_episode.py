"""Host-side checks of the Omniglot episode loader (csrc/episode.hip, hipops.episode_*, priors/omniglot.py): the C ABI, the build and the kernels' descriptor
budgets; the argument checks that must answer without a GPU, one per limit; the numpy restatement (tests/episode_ref.py) against its own invariants; ImageBank
from a directory of PNGs; the loader's assertions.  No GPU (validate needs episode_sample: tests/test_gpu_episode.py)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_ref as E      # noqa: E402

from transformerscandobayesianinference_amd import _hip, hipops, priors      # noqa: E402
from transformerscandobayesianinference_amd.priors import omniglot      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc')
PFN_ERR_UNSUPPORTED, PFN_ERR_ARGUMENT = -1, -4


def test_the_symbols_are_declared_exported_and_bound_at_abi_10():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    source = open(os.path.join(CSRC, 'episode.hip')).read()
    lib = _hip.lib()
    for symbol, nargs in (('pfn_episode_gather', 19), ('pfn_episode_sample', 28)):
        assert re.search(r'\b%s\s*\(' % symbol, header)
        assert symbol in _hip.SIGNATURES and hasattr(lib, symbol) and len(_hip.SIGNATURES[symbol][1]) == nargs
        assert re.search(r'^int %s\s*\(' % symbol, source, re.M), symbol
        declared = re.search(r'^int %s\s*\((.*?)\);' % symbol, header, re.M | re.S).group(1)
        assert declared.count(',') + 1 == nargs, symbol
    assert _hip.ABI_VERSION == 10 and lib.pfn_abi_version() == 10 and '#define PFN_ABI_VERSION 10' in header
    for name, value in (('MIN_SIZE', 8), ('MAX_SIZE', 64), ('MAX_WAY', 16), ('MAX_IMAGES', 64), ('STANDARD', 0), ('JONAS', 1)):
        assert f'#define PFN_EPISODE_{name} {value}\n' in header and getattr(hipops, 'EPISODE_' + name) == value, name
    assert (E.MAX_WAY, E.MAX_IMAGES) == (16, 64)
    build = open(os.path.join(CSRC, 'build.sh')).read()
    assert 'episode.hip' in build and '../_build/episode.o' in build
    assert priors.omniglot is omniglot and callable(omniglot.DataLoader.validate)


def test_the_kernels_keep_their_register_scratch_and_lds_budgets(tmp_path):
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    asm = str(tmp_path / 'episode.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', os.path.join(CSRC, 'episode.hip'), '-o', asm], check=True,
                   capture_output=True)
    found = dict(re.findall(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', open(asm).read(), re.S))
    assert len(found) == 4 and sum('episode_image_kernel' in k for k in found) == 2      # the f32 and the uint8 instantiation of one kernel
    assert sum('episode_draw_kernel' in k for k in found) == 1 and sum('episode_count_kernel' in k for k in found) == 1
    for name, body in found.items():
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name      # no scratch
        assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 64, name      # eight waves per SIMD
        lds = int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1))
        # the image kernel's LDS is dynamic (the table and four padded images: hipops.episode_lds_bytes); the draw kernel's lists and the count kernel's
        # per-wave partial sums are static
        assert lds == (4 * 16 * 3 + 2 * 16 * 64 + 2 * 16 * 64 if 'draw' in name else 4 * 16 if 'count' in name else 0), name
    assert hipops.episode_lds_bytes(28) == (256 + 4 * 28 * 29) * 4 and hipops.episode_lds_bytes(64) == (256 + 4 * 64 * 65) * 4 <= 160 * 1024


def test_argument_errors_return_before_any_launch():
    lib = _hip.lib()
    buf = torch.zeros(4096)      # host memory: a refused call never looks at it
    p = buf.data_ptr()
    assert p % 16 == 0

    def gather(bank=p, table=0, C=10, n_img=20, size=28, src=p, N=4, stride=None, x=p, bbox=p, shift=p, status=p):
        return lib.pfn_episode_gather(bank, table, C, n_img, size, src, p, 0, N, 1, size * size if stride is None else stride, 0, 0, 0, x, bbox, shift, status, 0)

    def sample(bank=p, table=0, C=10, n_img=20, size=28, B=2, n_way=5, k_shot=5, mode=0, pool=(0, 10), offsets=0, A=0, x=p, labels=p, status=p):
        return lib.pfn_episode_sample(bank, table, C, n_img, size, B, n_way, k_shot, mode, 1, 1, pool[0], pool[1], offsets, A, 0, 0, 0, x, labels, p, p, p, p, p, p,
                                      status, 0)
    for kw in (dict(size=7), dict(size=65), dict(n_img=0), dict(n_img=65)):
        assert gather(**kw) == PFN_ERR_UNSUPPORTED and sample(**kw) == PFN_ERR_UNSUPPORTED, kw
    assert sample(size=7) == PFN_ERR_UNSUPPORTED and b'8 .. 64' in lib.pfn_last_error_string()
    for kw in (dict(n_way=0), dict(n_way=17), dict(mode=2)):
        assert sample(**kw) == PFN_ERR_UNSUPPORTED, kw
    for kw in (dict(k_shot=0), dict(k_shot=20), dict(pool=(0, 4)), dict(pool=(-1, 10)), dict(pool=(0, 11)), dict(pool=(8, 10)), dict(B=-1), dict(B=2 ** 27, n_way=16),
               dict(C=0), dict(C=2 ** 27, n_img=64, pool=(0, 10)), dict(bank=0), dict(bank=p + 2), dict(table=p + 2), dict(x=0), dict(x=p + 2), dict(labels=0),
               dict(status=0), dict(status=p + 2), dict(mode=1), dict(mode=1, offsets=p, A=0), dict(mode=1, offsets=p + 2, A=3)):
        assert sample(**kw) == PFN_ERR_ARGUMENT, kw
    for kw in (dict(N=-1), dict(N=2 ** 31), dict(stride=783), dict(src=0), dict(x=0), dict(bbox=0), dict(shift=0), dict(src=p + 2), dict(x=p + 2), dict(status=p + 2),
               dict(C=0), dict(C=2 ** 27, n_img=64), dict(bank=0), dict(bank=p + 2)):
        assert gather(**kw) == PFN_ERR_ARGUMENT, kw
    assert gather(bank=p + 1, table=p, N=0) == 0      # a uint8 bank needs no alignment (N = 0 keeps the accepted call from launching)
    assert gather(size=7, src=0) == PFN_ERR_UNSUPPORTED      # the shapes first, before any pointer is looked at
    assert gather(N=0) == 0 and sample(B=0) == 0      # nothing to do: nothing launched


def bank_on_cpu(C=12, n_img=6, size=12, **kw):
    return omniglot.ImageBank.from_arrays(E.synthetic_bank(C, n_img, size, 3), E.TABLE, device='cpu', **kw)


def test_python_checks_raise_before_the_device_is_asked_for():
    bank = bank_on_cpu(n_train_classes=8, train_alphabet_offsets=[0, 5, 8], test_alphabet_offsets=[8, 12])
    src = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match='8 .. 64'):
        hipops.episode_gather(torch.zeros(2, 3, 7, 7), src)
    with pytest.raises(ValueError, match='n_img = 65'):
        hipops.episode_gather(torch.zeros(2, 65, 8, 8), src)
    with pytest.raises(ValueError, match='table'):
        hipops.episode_gather(torch.zeros(2, 3, 8, 8, dtype=torch.uint8), src)
    with pytest.raises(ValueError, match='table'):
        hipops.episode_gather(torch.zeros(2, 3, 8, 8), src, table=torch.zeros(256))
    with pytest.raises(ValueError, match='shift'):
        hipops.episode_gather(bank, src, shift=torch.zeros(2, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match='shift'):
        hipops.episode_gather(bank, src, shift='random')
    for kw, match in ((dict(n_way=17, k_shot=1), 'n_way = 17'), (dict(n_way=0, k_shot=1), 'n_way = 0'), (dict(n_way=2, k_shot=6), 'k_shot = 6'),
                      (dict(n_way=2, k_shot=0), 'k_shot = 0'), (dict(n_way=9, k_shot=2), 'pool'), (dict(n_way=5, k_shot=2, train=False), 'pool'),
                      (dict(n_way=4, k_shot=2, mode='jonas'), 'alphabet'), (dict(n_way=5, k_shot=2, mode='jonas', train=False), 'alphabet'),
                      (dict(n_way=2, k_shot=2, num_classes_used=1), 'pool')):
        args = dict(B=2, mode='standard', train=True, translate=True, seed=0)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            hipops.episode_sample(bank, **args)
    with pytest.raises(ValueError, match='alphabet'):
        bank_on_cpu(train_alphabet_offsets=[0, 5, 13])
    with pytest.raises(ValueError, match='n_train_classes'):
        bank_on_cpu(n_train_classes=13)
    with pytest.raises(ValueError, match='jonas'):
        hipops.episode_sample(bank_on_cpu(), 2, 2, 2, 'jonas', True, True, 0)
    # with sound arguments the product path asks for the GPU: there is no CPU fall-back
    with pytest.raises(_hip.HipExtensionError):
        hipops.episode_gather(bank, src)
    with pytest.raises(_hip.HipExtensionError):
        hipops.episode_sample(bank, 2, 3, 2, 'standard', True, True, 0)
    with pytest.raises(_hip.HipExtensionError):
        hipops.episode_sample(bank, 2, 3, 2, 'jonas', False, False, 0)


def test_dataloader_assertions():
    bank = bank_on_cpu()
    ok = dict(num_steps=2, batch_size=3, seq_len=7, num_features=144, num_outputs=3, bank=bank)
    with pytest.raises(AssertionError, match='fusing'):
        omniglot.DataLoader(**{**ok, 'fuse_x_y': True})
    with pytest.raises(AssertionError):
        omniglot.DataLoader(**{**ok, 'num_features': 143})      # no square
    with pytest.raises(AssertionError):
        omniglot.DataLoader(**{**ok, 'seq_len': 8})      # (8 - 1) % 3 != 0
    with pytest.raises(_hip.HipExtensionError, match='GPU only'):
        omniglot.DataLoader(**{**ok, 'device': 'cpu'})
    dl = omniglot.DataLoader(**ok)
    assert len(dl) == 2 and dl.num_features == 144 and dl.num_outputs == 3 and dl.fuse_x_y is False and dl.train and dl.translations and not dl.jonas_style
    assert dl.num_classes_used == 1200
    with pytest.raises(_hip.HipExtensionError, match='GPU only'):      # the bank lives on the host
        next(iter(dl))
    with pytest.raises(AssertionError, match='12 x 12'):
        next(iter(omniglot.DataLoader(**{**ok, 'num_features': 64, 'bank': bank})))
    with pytest.raises(FileNotFoundError, match='no_such_directory'):
        omniglot.DataLoader(**{**ok, 'bank': None, 'root': '/no_such_directory/omniglot'})
    import inspect
    names = list(inspect.signature(omniglot.DataLoader.__init__).parameters)
    assert names[1:11] == ['num_steps', 'batch_size', 'seq_len', 'num_features', 'num_outputs', 'num_classes_used', 'fuse_x_y', 'train', 'translations', 'jonas_style']
    assert names[11:] == ['bank', 'root', 'device', 'seed']


def test_image_bank_from_a_directory_of_pngs(tmp_path):
    PIL = pytest.importorskip('PIL')
    from PIL import Image
    rng = np.random.default_rng(5)
    layout = {'images_background': {'Alpha': 3, 'Beta': 2}, 'images_evaluation': {'Gamma': 2}}
    written = {}
    for split, alphabets in layout.items():
        for alphabet, n_chars in alphabets.items():
            for c in range(n_chars):
                d = tmp_path / 'processed' / split / alphabet / f'character{c + 1:02d}'
                d.mkdir(parents=True)
                for i in range(4):
                    a = np.where(rng.random((20, 20)) < 0.2, rng.integers(0, 200, (20, 20)), 255).astype(np.uint8)
                    Image.fromarray(a).save(str(d / f'{c:04d}_{i + 1:02d}.png'))
                    written[(split, alphabet, c, i)] = a
    bank = omniglot.ImageBank.from_directory(str(tmp_path), 20, device='cpu')
    assert tuple(bank.images.shape) == (7, 4, 20, 20) and bank.images.dtype == torch.uint8 and (bank.n_classes, bank.n_img, bank.size) == (7, 4, 20)
    order = [('images_background', 'Alpha', 0), ('images_background', 'Alpha', 1), ('images_background', 'Alpha', 2), ('images_background', 'Beta', 0),
             ('images_background', 'Beta', 1), ('images_evaluation', 'Gamma', 0), ('images_evaluation', 'Gamma', 1)]
    for cls, key in enumerate(order):
        for i in range(4):
            assert (bank.images[cls, i].numpy() == written[key + (i,)]).all(), (cls, i)      # resize to its own size: the bytes of the file
    assert bank.alphabet_offsets_host(True) == [0, 3, 5] and bank.alphabet_offsets_host(False) == [5, 7] and bank.n_train_classes == 5
    assert bank.train_alphabet_offsets.tolist() == [0, 3, 5] and bank.train_alphabet_offsets.dtype == torch.int32 and bank.test_alphabet_offsets.tolist() == [5, 7]
    b = np.arange(256)
    assert (bank.table.numpy() == (1 - b / 255.).astype(np.float32)).all() and bank.table[255] == 0 and bank.table[0] == 1 and bank.table.dtype == torch.float32
    # the reference's transform chain on one file: convert('L'), resize, / 255., 1 - x, astype(float32)
    half = omniglot.ImageBank.from_directory(str(tmp_path), 10, device='cpu')
    path = str(tmp_path / 'processed' / 'images_background' / 'Beta' / 'character02' / '0001_03.png')
    want = (1 - np.reshape(Image.open(path).convert('L').resize((10, 10)), (10, 10, 1)).transpose(2, 0, 1) / 255.)[0].astype(np.float32)
    assert (half.table[half.images[4, 2].long()].numpy() == want).all()
    with pytest.raises(FileNotFoundError, match=re.escape(str(tmp_path / 'nothing'))):
        omniglot.ImageBank.from_directory(str(tmp_path / 'nothing'), 20, device='cpu')
    (tmp_path / 'processed' / 'images_background' / 'Beta' / 'character02' / '0001_04.png').unlink()
    with pytest.raises(ValueError, match='same number of images'):
        omniglot.ImageBank.from_directory(str(tmp_path), 20, device='cpu')
    assert PIL.__version__


# ---- the restatement against its own invariants ---------------------------------------------------------------------------------------------------------------
def glyphs(size):
    bank = np.concatenate([E.synthetic_bank(6, 4, size, 17).reshape(-1, size, size), E.special_images(size)])
    return E.TABLE[bank]      # f32 values, background 0.0


@pytest.mark.parametrize('size', [8, 28, 31, 64])
def test_restated_shift_is_inverted_by_the_opposite_shift_and_keeps_the_content_in_frame(size):
    for image in glyphs(size):
        for k in range(4):
            rot = np.rot90(image, k, axes=(-2, -1))
            bbox = E.bounding_box(rot)
            assert bbox == E.rotated_bbox(image, k)
            (xlo, xhi), (ylo, yhi) = E.shift_range(bbox, size)
            if bbox == E.EMPTY_BBOX:
                assert (image == 0).all() and (xlo, xhi, ylo, yhi) == (0, 0, 0, 0)
                continue
            c0, c1, r0, r1 = bbox
            assert xlo <= 0 <= xhi and ylo <= 0 <= yhi and (rot[r0] != 0).any() and (rot[r1] != 0).any() and (rot[:, c0] != 0).any() and (rot[:, c1] != 0).any()
            assert (rot[:r0] == 0).all() and (rot[r1 + 1:] == 0).all() and (rot[:, :c0] == 0).all() and (rot[:, c1 + 1:] == 0).all()
            for tx in (xlo, xhi):
                for ty in (ylo, yhi):
                    out = E.transform(image, k, tx, ty)
                    # at either extreme of the drawn range nothing leaves the frame: the same multiset of values, the box moved by exactly (tx, ty) ...
                    assert (np.sort(out.reshape(-1)) == np.sort(rot.reshape(-1))).all()
                    assert E.bounding_box(out) == (c0 + tx, c1 + tx, r0 + ty, r1 + ty)
                    # ... and the opposite shift restores the image
                    assert (E.shifted(out, -tx, -ty) == rot).all()
            # one step beyond the range loses content
            if (rot[:, c0] != 0).any():
                assert (E.shifted(rot, xlo - 1, 0) != 0).sum() < (rot != 0).sum()
                assert (E.shifted(rot, 0, yhi + 1) != 0).sum() < (rot != 0).sum()


def test_restated_shift_is_the_stated_index_rule():
    rot = np.arange(1, 26, dtype=np.float32).reshape(5, 5)
    out = E.shifted(rot, 2, -1)
    for y in range(5):
        for x in range(5):
            inside = 0 <= y + 1 < 5 and 0 <= x - 2 < 5
            assert out[y, x] == (rot[y + 1, x - 2] if inside else 0)
    assert (E.shifted(rot, 0, 0) == rot).all() and (E.shifted(rot, 5, 0) == 0).all() and (E.shifted(rot, 0, -5) == 0).all()
    # rot90 as csrc/episode.hip states it
    a = np.arange(16).reshape(4, 4)
    r1, r2, r3 = (np.rot90(a, k, axes=(-2, -1)) for k in (1, 2, 3))
    for i in range(4):
        for j in range(4):
            assert r1[i, j] == a[j, 3 - i] and r2[i, j] == a[3 - i, 3 - j] and r3[i, j] == a[3 - j, i]


def test_replayed_draws_are_selections_without_replacement_and_permutations():
    rng = np.random.default_rng(0)
    for _ in range(200):
        n = int(rng.integers(1, 65))
        k = int(rng.integers(1, n + 1))
        w = rng.integers(0, 2 ** 32, 64, dtype=np.uint64)
        chosen = E.take_subset(k, n, w)
        assert len(set(chosen)) == k and min(chosen) >= 0 and max(chosen) < n
        assert sorted(E.permutation(n, w)) == list(range(n))
    # the rank rule: word 0 -> the value itself, later words skip what is taken
    top = 2 ** 32 - 1
    assert E.take_subset(3, 5, [0, 0, 0]) == [0, 1, 2] and E.take_subset(3, 5, [top, top, top]) == [4, 3, 2] and E.take_subset(2, 5, [2 ** 31, 0]) == [2, 0]
    # every ordered selection of 2 from 3 equally often over a grid of words
    grid = [int((i + 0.5) * 2 ** 32 / 6) for i in range(6)]
    seen = [tuple(E.take_subset(2, 3, [a, b])) for a in grid for b in grid]
    assert sorted(set(seen)) == [(a, b) for a in range(3) for b in range(3) if a != b] and all(seen.count(s) == 6 for s in set(seen))
    seen = [tuple(E.permutation(3, [a, b])) for a in grid for b in grid]
    assert len(set(seen)) == 6 and all(seen.count(s) == 6 for s in set(seen))


@pytest.mark.parametrize('mode,train', [('standard', True), ('standard', False), ('jonas', True), ('jonas', False)])
def test_replayed_episode_follows_the_modes_layout(mode, train):
    n_way, k_shot, n_img = 5, 3, 20
    offsets = [10, 17, 22, 40]
    for d in range(40):
        e = E.device_episode(11, 2, d, n_way, k_shot, n_img, mode, train, pool=(3, 30), alphabet_offsets=offsets)
        S_, q = n_way * k_shot, e['query']
        assert len(set(e['classes'])) == n_way and e['targets'] == [-100] * S_ + [q] and e['labels'][-1] == q and 0 <= q < n_way
        assert sorted(e['labels'][:S_]) == sorted(list(range(n_way)) * k_shot)
        for j in range(n_way):
            mine = [s - e['classes'][j] * n_img for s, lab in zip(e['src'], e['labels']) if lab == j]
            assert len(set(mine)) == len(mine) == k_shot + (j == q) and all(0 <= i < n_img for i in mine)
        if mode == 'standard':
            assert all(3 <= c < 30 for c in e['classes']) and all(0 <= r <= 3 for r in e['rotations'])
        else:
            first = offsets[e['alphabet']]
            assert sorted(e['classes']) == list(range(first, first + n_way)) and e['rotations'] == [0] * n_way
            assert e['labels'][:S_] == [j for j in range(n_way) for _ in range(k_shot)]      # class-major, unshuffled
            if not train:
                support = [s % n_img for s in e['src'][:S_]]
                assert all(sorted(support[j * k_shot:(j + 1) * k_shot]) == list(range(k_shot)) for j in range(n_way)) and k_shot <= e['src'][-1] % n_img < n_img


def test_the_host_replay_passes_the_distribution_test_at_its_seed():
    """tests/test_gpu_episode.py applies these chi-square tests to the device's draws at E.DIST['seed']; the draws are a function of the seed and the replay
    reproduces them, so the seed was chosen here, on the CPU, such that the replay passes."""
    results = E.distribution_statistics(*E.replayed_distribution_calls())
    for name, (chi2, p) in results.items():
        print(f'{name}: chi2 {chi2:.2f}, p {p:.4f}')
    assert len(results) == 14 and min(p for _, p in results.values()) > 1e-4
