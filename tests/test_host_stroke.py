"""Host-side checks of the stroke prior (csrc/stroke_prior.hip, priors/stroke.py, hipops.stroke_*): the numpy restatement (tests/stroke_ref.py) against the
recorded Pillow images and the recorded run of the reference's own get_batch, byte for byte; fresh random strokes against Pillow where it is installed; the
label and bound helper on CPU tensors; the C ABI, the build and the kernels' descriptor budgets; the argument checks that must answer without a GPU.  No GPU."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stroke_ref as R      # noqa: E402

from transformerscandobayesianinference_amd import _hip, hipops, priors      # noqa: E402
from transformerscandobayesianinference_amd.priors import stroke      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc')
PFN_ERR_UNSUPPORTED, PFN_ERR_ARGUMENT = -1, -4


@pytest.fixture(scope='module')
def recorded():
    return torch.load(os.path.join(ROOT, 'tests', 'golden', 'stroke_pillow.pt'), weights_only=False)


def test_the_fixture_covers_the_cases(recorded):
    a = recorded['strokes']
    assert sorted(a) == [8, 28, 31, 64] and 250 <= sum(v['width'].numel() for v in a.values()) <= 350
    widths = torch.cat([v['width'] for v in a.values()])
    assert set(range(5)) <= set(widths.tolist()) and 7 in widths.tolist()
    segs28, n28 = a[28]['segs'].numpy(), a[28]['n_strokes'].numpy()
    first = segs28[n28 >= 1, 0]
    dx, dy = np.abs(first[:, 2] - first[:, 0]), np.abs(first[:, 3] - first[:, 1])
    assert ((dy == 0) & (dx > 0)).any() and ((dx == 0) & (dy > 0)).any() and ((dx == dy) & (dx > 0)).any() and ((dx == 0) & (dy == 0)).any()
    assert ((dx > 4 * dy) & (dy > 0)).any() and ((dy > 4 * dx) & (dx > 0)).any()      # shallow and steep
    off = (first < 0) | (first > 27)
    assert (off.any(1) & ~off.all(1)).any() and off.all(1).any()      # partly and wholly off the canvas
    assert (n28 == 3).any() and (n28 == 0).any() and (n28 == 8).any()
    rows64 = a[64]['segs'][:, 0].tolist()
    assert [0, 32, 63, 32] in rows64 and [32, 0, 32, 63] in rows64      # a full row and a full column at size 64
    assert (a[64]['raw'].view(-1, 64, 64)[rows64.index([0, 32, 63, 32]), 32] != 0).all()
    assert int(sum(v['contract_differs'].sum() for v in a.values())) >= 10
    b = recorded['reference']
    assert b['size'] == 28 and tuple(b['img'].shape) == (3, 11, 784) and tuple(b['cls_n'].shape) == (3, 5)
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'stroke_pillow.pt')) < 1 << 20


def test_the_restatement_draws_every_recorded_pillow_image(recorded):
    for size, v in recorded['strokes'].items():
        for i in range(v['width'].numel()):
            raw = v['raw'][i].numpy().reshape(size, size)
            mine = R.raw_image(size, v['segs'][i].numpy(), int(v['n_strokes'][i]), int(v['width'][i]), R.noise_field(raw))
            assert (mine == raw).all(), (size, i)
            assert (R.blur(mine).reshape(-1) == v['img'][i].numpy()).all(), (size, i)


def test_the_flagged_strokes_differ_under_contracted_arithmetic(recorded):
    """The fixture can tell a kernel that fuses the edge intersection into one FMA from a correct one."""
    flagged = 0
    for size, v in recorded['strokes'].items():
        for i in torch.nonzero(v['contract_differs']).flatten().tolist():
            lit = v['raw'][i].numpy().reshape(size, size) != 0
            args = (size, v['segs'][i].numpy(), int(v['n_strokes'][i]), int(v['width'][i]))
            assert (R.image_mask(*args) == lit).all() and (R.image_mask(*args, contract=True) != lit).any(), (size, i)
            flagged += 1
    assert flagged >= 10


def replay(b, d, t):
    """Image (d, t) of the recorded reference run from its recorded draws: (segs, n, tie distance)."""
    c = int(b['labels'][d, t])
    n = int(b['cls_n'][d, c])
    segs, tie = R.image_segments(b['cls_len'][d, c, :n].tolist(), [tuple(p) for p in b['cls_start'][d, c, :n].tolist()], b['cls_dir'][d, c, :n].tolist(),
                                 tuple(b['offset'][d, t].tolist()), [tuple(p) for p in b['jitter'][d, t, :n].tolist()])
    return np.asarray(segs, dtype=np.int32).reshape(n, 4), n, tie


def test_the_restatement_replays_the_references_own_run(recorded):
    b = recorded['reference']
    size, worst, worst_ref = b['size'], 0., 0.
    bounds = R.int_bounds(size)
    for d in range(3):
        for c in range(5):
            n = int(b['cls_n'][d, c])
            assert bounds['strokes'][0] <= n <= bounds['strokes'][1]
            for s in range(n):      # what the class loop accepted lies on the canvas
                length, (sx, sy), th = int(b['cls_len'][d, c, s]), b['cls_start'][d, c, s].tolist(), float(b['cls_dir'][d, c, s])
                assert bounds['len'][0] <= length <= bounds['len'][1] and all(bounds['start'][0] <= v <= bounds['start'][1] for v in (sx, sy))
                assert 0 <= sx + math.cos(th) * length <= size - 1 and 0 <= sy + math.sin(th) * length <= size - 1
        for t in range(11):
            segs, n, _ = replay(b, d, t)
            assert (segs == b['segs'][d, t, :n].numpy()).all()
            img = R.blur(R.raw_image(size, segs, n, int(b['width'][d, t]), b['noise'][d, t].numpy()))
            assert (img.reshape(-1) == b['img'][d, t].numpy()).all(), (d, t)
            assert (R.to_x(img).view(np.uint32) == b['x'][d, t].numpy().view(np.uint32)).all(), (d, t)      # bit for bit
            # normalize_x: the reference's f32 result has an error e of its own against f64; nothing better than 3 max(e, u) is asked of anyone
            x64 = R.normalized_f64(img)
            e = R.normalized_error(b['x_normalized'][d, t].numpy(), x64)
            worst_ref = max(worst_ref, e)
            worst = max(worst, R.normalized_error(x64.astype(np.float32), x64) / (3 * max(e, R.F32_UNIT_ROUNDOFF)))
    print(f'normalize_x: the reference\'s own f32 error {worst_ref:.3e}; the rounded f64 value uses {worst:.3f} of the bound')
    assert worst < 1 and worst_ref < 1e-5
    assert (b['targets'][:, :-1] == -100).all() and (b['targets'][:, -1] == b['labels'][:, -1].long()).all()


def test_fresh_random_strokes_against_pillow():
    PIL = pytest.importorskip('PIL')
    from PIL import Image, ImageDraw, ImageFilter
    seed = int.from_bytes(os.urandom(4), 'little')      # fresh strokes on every run; a failure names the seed
    rng = np.random.default_rng(seed)
    differing = 0
    for i in range(2000):
        size = int(rng.choice([8, 28, 31, 64]))
        width = int(rng.integers(0, 5))
        seg = [int(c) for c in rng.integers(-5, size + 5, 4)]
        im = Image.fromarray(np.zeros((size, size), dtype=np.uint8))
        ImageDraw.Draw(im).line(seg, fill=128, width=width)
        differing += int(((np.array(im) == 128) != R.line_mask(size, seg, width)).any())
        if i % 40 == 0:
            raw = np.where(np.array(im) == 128, rng.integers(200, 255, (size, size)), 0).astype(np.uint8)
            differing += int((np.array(Image.fromarray(raw).filter(ImageFilter.GaussianBlur(.2))) != R.blur(raw)).any())
    assert differing == 0, (PIL.__version__, seed)


def test_blur_constants_follow_from_the_radius():
    assert R.blur_constants() == (R.BLUR_WW, R.BLUR_FW) == (16553519, 111848)
    assert 255 * (R.BLUR_WW + 2 * R.BLUR_FW) + (1 << 23) == 4286578433 and 2 ** 31 < 4286578433 < 2 ** 32
    text = open(os.path.join(CSRC, 'stroke_prior.hip')).read()
    assert '16553519u' in text and '111848u' in text
    # byte * (1 / 255.f) is not byte / 255.f for every byte: why the kernel divides
    assert (R.BYTE_TO_X != np.arange(256, dtype=np.float32) * (np.float32(1) / np.float32(255))).any()


def test_labels_and_targets_on_cpu():
    g = torch.Generator().manual_seed(3)
    labels, targets = stroke.draw_labels(64, 26, 5, only_train_for_last_idx=True, generator=g)
    assert labels.shape == targets.shape == (64, 26) and labels.dtype == targets.dtype == torch.int64
    counts = torch.stack([(labels[:, :-1] == c).sum(1) for c in range(5)], 1)
    assert (counts == 5).all() and (targets[:, :-1] == -100).all() and (targets[:, -1] == labels[:, -1]).all()
    assert 0 <= int(labels.min()) and int(labels.max()) <= 4 and len(set(map(tuple, labels[:, :-1].tolist()))) > 60      # shuffled per dataset
    assert set(labels[:, -1].tolist()) == set(range(5))
    with pytest.raises(AssertionError):
        stroke.draw_labels(4, 26, 4, only_train_for_last_idx=True)      # (26 - 1) % 4 != 0
    labels, targets = stroke.draw_labels(200, 7, 3, generator=g)
    assert targets is labels and set(labels.flatten().tolist()) == {0, 1, 2}


@pytest.mark.parametrize('size', [28, 10])
def test_integer_bounds_are_the_references_expressions(size):
    min_max_strokes, min_max_len, min_max_start, min_max_width, max_offset, max_target_offset = (1, 3), (5 / 28, 20 / 28), (2 / 28, 25 / 28), (1 / 28, 4 / 28), 4 / 28, 2 / 28
    want = dict(strokes=min_max_strokes, len=(int(size * min_max_len[0]), int(size * min_max_len[1])), start=(int(size * min_max_start[0]), int(size * min_max_start[1])),
                width=(int(size * min_max_width[0]), int(size * min_max_width[1])), offset=(int(-size * max_offset), int(size * max_offset)),
                jitter=(int(-size * max_target_offset), int(size * max_target_offset)))
    assert stroke.integer_bounds(size) == want == R.int_bounds(size)
    if size == 28:
        assert want == dict(strokes=(1, 3), len=(5, 20), start=(2, 25), width=(1, 4), offset=(-4, 4), jitter=(-2, 2))
    else:
        assert want == dict(strokes=(1, 3), len=(1, 7), start=(0, 8), width=(0, 1), offset=(-1, 1), jitter=(0, 0))      # int(-1.43) = -1: truncation, not floor
    assert stroke.integer_bounds(28, min_max_width=(2 / 28, 9 / 28), max_offset=0.3)['width'] == (2, 9)
    assert stroke.integer_bounds(28, max_offset=0.3)['offset'] == (-8, 8)


def test_the_symbols_are_declared_exported_and_bound_at_abi_10():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    source = open(os.path.join(CSRC, 'stroke_prior.hip')).read()      # the entry points stand beside their kernels
    lib = _hip.lib()
    for symbol, nargs in (('pfn_stroke_render', 14), ('pfn_stroke_prior_sample', 30)):
        assert re.search(r'\b%s\s*\(' % symbol, header)
        assert symbol in _hip.SIGNATURES and hasattr(lib, symbol) and len(_hip.SIGNATURES[symbol][1]) == nargs
        assert re.search(r'^int %s\s*\(' % symbol, source, re.M), symbol      # defined there ...
    assert re.search(r'\blaunch_stroke_render\s*\(', source) and re.search(r'\blaunch_stroke_prior\s*\(', source)      # ... and wired to its launcher
    assert _hip.ABI_VERSION == 10 and lib.pfn_abi_version() == 10 and '#define PFN_ABI_VERSION 10' in header
    for name, value in (('MAX_STROKES', 8), ('MAX_CLASSES', 16), ('MAX_WIDTH', 64), ('MAX_PASSES', 256), ('COORD_LIMIT', 4096)):
        assert f'#define PFN_STROKE_{name} {value}\n' in header and getattr(hipops, 'STROKE_' + name) == value, name
    assert (R.MAX_STROKES, R.MAX_CLASSES, R.MAX_PASSES, R.COORD_LIMIT) == (8, 16, 256, 4096)
    build = open(os.path.join(CSRC, 'build.sh')).read()
    assert 'stroke_prior.hip' in build and '../_build/stroke_prior.o' in build      # compiled and linked
    assert priors.stroke is stroke and stroke.DataLoader.num_outputs == 2 and callable(stroke.get_batch)
    from transformerscandobayesianinference_amd import train
    assert "'stroke': priors.stroke.DataLoader" in open(train.__file__).read()


def test_the_kernels_keep_their_register_scratch_and_lds_budgets(tmp_path):
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    asm = str(tmp_path / 'stroke_prior.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', os.path.join(CSRC, 'stroke_prior.hip'), '-o', asm], check=True,
                   capture_output=True)
    found = dict(re.findall(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', open(asm).read(), re.S))
    assert len(found) == 3 and sum('stroke_render_kernel' in k for k in found) == 1 and sum('stroke_classes_kernel' in k for k in found) == 1 and \
        sum('stroke_images_kernel' in k for k in found) == 1
    for name, body in found.items():
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name      # no scratch
        assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 128, name      # four waves per SIMD
        lds = int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1))
        # four waves x two 4 KB images + the 256-entry byte / 255 table: four blocks per CU
        assert lds == (0 if 'classes' in name else 4 * 2 * 4096 + 1024), name


def test_argument_errors_return_before_any_launch():
    lib = _hip.lib()
    buf = torch.zeros(4096)      # host memory: a refused call never looks at it
    p = buf.data_ptr()
    assert p % 16 == 0

    def render(N=4, size=28, stride=None, segs=p, x=p):
        return lib.pfn_stroke_render(segs, p, p, 0, N, size, 0, size * size if stride is None else stride, 0, 0, x, 0, 0, 0)

    def sample(B=2, T=3, C=2, size=28, strokes=(1, 3), length=(5, 20), start=(2, 25), width=(1, 4), off=4, toff=2, labels=p, status=p):
        return lib.pfn_stroke_prior_sample(labels, B, T, C, size, 0, *strokes, *length, *start, *width, off, toff, 0, 0, 0, p, p, p, p, p, p, p, 0, 0, status, 0)
    for kw in (dict(size=7), dict(size=65)):
        assert render(**kw) == PFN_ERR_UNSUPPORTED and sample(**kw) == PFN_ERR_UNSUPPORTED, kw
        assert b'8 .. 64' in lib.pfn_last_error_string()
    for kw in (dict(width=(1, 65)), dict(strokes=(1, 9)), dict(C=0), dict(C=17), dict(length=(5, 1025)), dict(off=1025)):
        assert sample(**kw) == PFN_ERR_UNSUPPORTED, kw
    for kw in (dict(B=0), dict(T=0), dict(strokes=(3, 1)), dict(width=(-1, 4)), dict(off=-1), dict(toff=-1), dict(labels=0), dict(status=0), dict(status=p + 2)):
        assert sample(**kw) == PFN_ERR_ARGUMENT, kw
    for kw in (dict(N=-1), dict(stride=783), dict(segs=0), dict(x=0), dict(segs=p + 4), dict(x=p + 2)):
        assert render(**kw) == PFN_ERR_ARGUMENT, kw
    assert render(size=7, segs=0) == PFN_ERR_UNSUPPORTED      # the shapes first, before any pointer is looked at
    assert render(N=0) == 0      # nothing to draw: nothing launched


def test_python_checks_raise_before_the_device_is_asked_for():
    segs, n, w = torch.zeros(2, 8, 4, dtype=torch.int32), torch.ones(2, dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    for size in (7, 65):
        with pytest.raises(ValueError, match='8 .. 64'):
            hipops.stroke_render(segs, n, w, size)
        with pytest.raises(ValueError, match='8 .. 64'):
            stroke.get_batch(2, 3, num_features=size * size)
    with pytest.raises(AssertionError, match='square'):
        stroke.get_batch(2, 3, num_features=783)
    with pytest.raises(ValueError, match='width = 65'):
        stroke.get_batch(2, 3, num_features=784, min_max_width=(1 / 28, 65 / 28))
    with pytest.raises(ValueError, match='strokes = 9'):
        stroke.get_batch(2, 3, num_features=784, min_max_strokes=(1, 9))
    with pytest.raises(ValueError, match='num_classes = 17'):
        stroke.get_batch(2, 3, num_features=784, num_outputs=17)
    with pytest.raises(AssertionError):
        stroke.get_batch(2, 26, num_features=784, num_outputs=4, only_train_for_last_idx=True)
    with pytest.raises(ValueError):
        hipops.stroke_render(torch.zeros(2, 7, 4, dtype=torch.int32), n, w, 28)
    # with sound arguments the product path asks for the GPU: there is no CPU fall-back
    with pytest.raises(_hip.HipExtensionError):
        hipops.stroke_render(segs, n, w, 28)
    with pytest.raises(_hip.HipExtensionError):
        stroke.get_batch(2, 3, num_features=784, device='cpu')


def test_use_saved_from_round_trip(tmp_path):
    directory = tmp_path / 'len_11_out_5_features_784_bs_4'
    directory.mkdir()
    batch = (torch.rand(11, 4, 784), torch.randint(0, 5, (11, 4)), torch.randint(0, 5, (11, 4)))
    torch.save(batch, str(directory / 'batch_0.pt'))
    x, y, target = stroke.get_batch(4, 11, num_features=784, num_outputs=5, use_saved_from=str(tmp_path))
    assert torch.equal(x, batch[0]) and torch.equal(y, batch[1]) and torch.equal(target, batch[2])
    with pytest.raises(FileNotFoundError):
        stroke.get_batch(5, 11, num_features=784, num_outputs=5, use_saved_from=str(tmp_path))


def test_the_device_draws_restated_on_the_host_are_uniform_and_independent_of_the_batch():
    """stroke_ref's Philox is the generator of csrc/pfn_device.h (Random123's known-answer vectors) and its integer map covers [lo, hi] exactly."""
    assert R.philox4x32_10(0, 0, 0).tolist() == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = R.philox4x32_10(0xffffffffffffffff, 0xffffffffffffffff, 0xffffffffffffffff)
    assert ones.tolist() == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert R.u_int(0, -4, 4) == -4 and R.u_int(2 ** 32 - 1, -4, 4) == 4 and R.u_int(2 ** 31, 0, 1) == 1 and R.u_int(2 ** 31 - 1, 0, 1) == 0
    noise = R.device_noise(31, 5, 2, 77)
    assert noise.shape == (31, 31) and noise.min() >= 200 and noise.max() <= 254
