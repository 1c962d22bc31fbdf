"""The Omniglot episode loader on the device (csrc/episode.hip, hipops.episode_gather / episode_sample, priors/omniglot.py) against the numpy restatement
(tests/episode_ref.py): output bits equal for every rotation, extreme shift, size, stride and special image; the sampler's draws replayed on the host from the
same counters; its distribution against the exact uniform laws at a fixed seed; validate with stand-in models; the notebook's fine-tuning call at a small
shape.  Nothing is pinned to reference output (episode_ref says why)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_ref as E      # noqa: E402

from transformerscandobayesianinference_amd import encoders, hipops, priors      # noqa: E402
from transformerscandobayesianinference_amd.priors import omniglot      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
P_MIN = 1e-4
FORMS = ['uint8', 'f32']
_cache = {}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def gather_bytes(size):
    """uint8 [12, 6, size, size]: ten classes of random glyphs and two of the special images (tests/episode_ref.py)."""
    if ('bytes', size) not in _cache:
        _cache['bytes', size] = np.concatenate([E.synthetic_bank(10, 6, size, 100 + size), E.special_images(size).reshape(2, 6, size, size)])
    return _cache['bytes', size]


def device_bank(raw, form):
    """(bank tensor, table or None) on the device: the bytes with the table, or the f32 values the table gives them."""
    if form == 'uint8':
        return torch.from_numpy(raw).to(DEV), torch.from_numpy(E.TABLE).to(DEV)
    return torch.from_numpy(E.TABLE[raw]).to(DEV), None


def gather_cases(size):
    """Every image x four rotations x the four extreme shifts and no shift: (src, rot, shift, want x [N, size^2] f32, bbox [N, 4]), computed once per size."""
    if ('cases', size) not in _cache:
        values = E.TABLE[gather_bytes(size)].reshape(-1, size, size)
        src, rot, shift, want, boxes = [], [], [], [], []
        for s, image in enumerate(values):
            for k in range(4):
                bbox = E.rotated_bbox(image, k)
                (xlo, xhi), (ylo, yhi) = E.shift_range(bbox, size)
                for tx, ty in ((xlo, ylo), (xlo, yhi), (xhi, ylo), (xhi, yhi), (0, 0)):
                    src.append(s), rot.append(k), shift.append((tx, ty)), boxes.append(bbox)
                    want.append(E.transform(image, k, tx, ty).reshape(-1))
        _cache['cases', size] = (torch.tensor(src, dtype=torch.int32), torch.tensor(rot, dtype=torch.int32), torch.tensor(shift, dtype=torch.int32),
                                 torch.from_numpy(np.stack(want)), torch.tensor(boxes, dtype=torch.int32))
    return _cache['cases', size]


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('size', [8, 28, 31, 64])
def test_gather_equals_the_restatement_bit_for_bit(size, form):
    """72 images -- random glyphs, a glyph on each edge, a pixel in each corner, a full frame, an all-background image, a full row and column (at size 64 a row
    mask of 64 set bits) -- x 4 rotations x every extreme shift."""
    src, rot, shift, want, boxes = gather_cases(size)
    bank, table = device_bank(gather_bytes(size), form)
    r = hipops.episode_gather(bank, src.to(DEV), rot.to(DEV), shift.to(DEV), table=table)
    assert torch.equal(r['bbox'].cpu(), boxes)
    assert torch.equal(r['shift'].cpu(), shift)
    wrong = torch.nonzero((bits(r['x']) != bits(want)).any(1)).flatten().tolist()
    assert not wrong, (size, form, len(wrong), [(int(src[i]), int(rot[i]), shift[i].tolist()) for i in wrong[:5]])
    empties = int((boxes[:, 1] < boxes[:, 0]).sum())
    assert empties == 4 * 5 and int(r['status'].item()) == empties      # the one all-background image, in every rotation and shift
    assert (r['x'][torch.nonzero(boxes[:, 1] < boxes[:, 0]).flatten().to(DEV)] == 0).all()
    # no shift and no rotation asked for: the bank's own values
    plain = hipops.episode_gather(bank, torch.arange(72, dtype=torch.int32, device=DEV), table=table)
    assert torch.equal(bits(plain['x']), bits(torch.from_numpy(E.TABLE[gather_bytes(size)].reshape(72, -1)))) and (plain['shift'] == 0).all()


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('N,size,stride', [(1, 28, 784), (257, 28, 784 + 16), (257, 28, 784 + 3), (257, 31, 961), (5, 31, 961 + 3), (257, 8, 64), (3, 64, 4096 + 3),
                                           (2, 64, 4096 + 16)])
def test_gather_block_tails_and_image_strides(N, size, stride, form):
    """N = 1 and N = 257 leave the last block of four images partly empty; a stride above size^2 writes into a wider layout and leaves the floats between
    images alone; a stride that is no multiple of four floats takes the dword-store path at a size that otherwise stores 16 bytes."""
    src, rot, shift, want, boxes = gather_cases(size)
    pick = (torch.arange(N) * 7) % src.numel()
    bank, table = device_bank(gather_bytes(size), form)
    out = torch.full((N, stride), -7.0, device=DEV)
    r = hipops.episode_gather(bank, src[pick].to(DEV), rot[pick].to(DEV), shift[pick].to(DEV), table=table, out=out)
    assert r['x'] is out and torch.equal(bits(out[:, :size * size]), bits(want[pick])) and (out[:, size * size:] == -7.0).all()
    assert torch.equal(r['bbox'].cpu(), boxes[pick])


@pytest.mark.parametrize('form', FORMS)
def test_gather_from_a_bank_that_is_not_16_byte_aligned(form):
    """size % 4 == 0 reads the bank 16 (f32) or 4 (uint8) bytes at a time only when the bank is aligned for it."""
    size = 28
    src, rot, shift, want, _ = gather_cases(size)
    bank, table = device_bank(gather_bytes(size), form)
    room = torch.zeros(bank.numel() + 8, dtype=bank.dtype, device=DEV)
    moved = room[1:1 + bank.numel()].view(bank.shape)
    moved.copy_(bank)
    assert moved.is_contiguous() and moved.data_ptr() % (16 if form == 'f32' else 4) != 0
    r = hipops.episode_gather(moved, src.to(DEV), rot.to(DEV), shift.to(DEV), table=table)
    assert torch.equal(bits(r['x']), bits(want))


def test_gather_clamps_what_it_reads_from_device_memory():
    size = 28
    bank, table = device_bank(gather_bytes(size), 'uint8')
    src = torch.tensor([-5, 10 ** 6, 3, 4], dtype=torch.int32, device=DEV)
    rot = torch.tensor([1, 2, -1, 9], dtype=torch.int32, device=DEV)
    for t, match in ((dict(src=src, rot=None), 'src outside'), (dict(src=src.clamp(0, 71), rot=rot), 'rot outside')):
        with pytest.raises(ValueError, match=match):
            hipops.episode_gather(bank, t['src'], t['rot'], table=table)
    got = hipops.episode_gather(bank, src, rot, table=table, check=False)
    want = hipops.episode_gather(bank, src.clamp(0, 71), rot.clamp(0, 3), table=table)
    assert torch.equal(bits(got['x']), bits(want['x'])) and torch.equal(got['bbox'], want['bbox'])
    far = hipops.episode_gather(bank, src.clamp(0, 71), shift=torch.tensor([[10 ** 6, 0], [0, -10 ** 6], [28, 0], [0, 0]], dtype=torch.int32, device=DEV), table=table)
    assert (far['x'][:3] == 0).all() and far['shift'].tolist() == [[28, 0], [0, -28], [28, 0], [0, 0]]


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('size', [8, 31])
def test_gather_draws_its_shifts_from_the_stated_counters(size, form):
    src, rot, _, _, boxes = gather_cases(size)
    pick = torch.arange(0, src.numel(), 5)      # every image and rotation once
    bank, table = device_bank(gather_bytes(size), form)
    seed, offset, first = 77, 3, 1000
    r = hipops.episode_gather(bank, src[pick].to(DEV), rot[pick].to(DEV), 'draw', table=table, seed=seed, offset=offset, first_image=first)
    values = E.TABLE[gather_bytes(size)].reshape(-1, size, size)
    got = r['shift'].cpu()
    moved = 0
    for n, i in enumerate(pick.tolist()):
        bbox = tuple(boxes[i].tolist())
        tx, ty = E.device_shift(seed, offset, first + n, bbox, size)
        (xlo, xhi), (ylo, yhi) = E.shift_range(bbox, size)
        assert got[n].tolist() == [tx, ty] and xlo <= tx <= xhi and ylo <= ty <= yhi, (n, i)
        assert (r['x'][n].cpu().numpy().view(np.uint32) == E.transform(values[int(src[i])], int(rot[i]), tx, ty).reshape(-1).view(np.uint32)).all(), (n, i)
        moved += (tx, ty) != (0, 0)
    assert moved > pick.numel() // 2
    other = hipops.episode_gather(bank, src[pick].to(DEV), rot[pick].to(DEV), 'draw', table=table, seed=seed, offset=offset + 1, first_image=first)
    assert not torch.equal(other['shift'], r['shift'])


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------------------------------
SAMPLE = dict(C=27, n_img=8, size=28, n_train=16, train_offsets=[0, 5, 11, 16], test_offsets=[16, 21, 27], n_way=5, k_shot=2, B=16, used=14, seed=20261, offset=4)
CASES = [('standard', True), ('standard', False), ('jonas', True), ('jonas', False)]


def sample_bank(form):
    if ('sample_bank', form) not in _cache:
        k = SAMPLE
        raw = E.synthetic_bank(k['C'], k['n_img'], k['size'], 9)
        images, table = (raw, E.TABLE) if form == 'uint8' else (E.TABLE[raw], None)
        _cache['sample_bank', form] = (raw, omniglot.ImageBank.from_arrays(images, table, k['n_train'], k['train_offsets'], k['test_offsets'], device=DEV))
    return _cache['sample_bank', form]


def sampled(mode, train, form='uint8', **change):
    key = ('sampled', mode, train, form, tuple(sorted(change.items())))
    if key not in _cache:
        k = {**SAMPLE, **change}
        _cache[key] = hipops.episode_sample(sample_bank(form)[1], k['B'], k['n_way'], k['k_shot'], mode, train, True, k['seed'], offset=k['offset'],
                                            first_dataset=k.get('first', 0), num_classes_used=k['used'])
    return _cache[key]


@pytest.mark.parametrize('mode,train', CASES)
def test_sample_equals_the_host_replay_and_gather_of_what_it_returns(mode, train):
    k = SAMPLE
    raw, bank = sample_bank('uint8')
    r = sampled(mode, train)
    n_way, k_shot, n_img, size, B = k['n_way'], k['k_shot'], k['n_img'], k['size'], k['B']
    T, S_ = n_way * k_shot + 1, n_way * k_shot
    assert tuple(r['x'].shape) == (T, B, size * size) and (r['status'] == 0).all()
    # x is gather of the returned (src, rotation of the label's class, shift), bit for bit
    rot = torch.gather(r['rotations'], 1, r['labels'].long())
    again = hipops.episode_gather(bank, r['src'].reshape(-1), rot.reshape(-1).contiguous(), r['shift'].reshape(-1, 2))
    assert torch.equal(bits(again['x'].view(B, T, -1).transpose(0, 1)), bits(r['x'])) and torch.equal(again['bbox'].view(B, T, 4), r['bbox'])
    host = {key: v.cpu().numpy() for key, v in r.items()}
    values = E.TABLE[raw].reshape(-1, size, size)
    pool = (0, k['used']) if train else (k['n_train'], k['C'])
    offsets = k['train_offsets'] if train else k['test_offsets']
    for b in range(B):
        e = E.device_episode(k['seed'], k['offset'], b, n_way, k_shot, n_img, mode, train, pool=pool, alphabet_offsets=offsets)
        for key in ('classes', 'rotations', 'labels', 'targets', 'src'):
            assert host[key][b].tolist() == e[key], (b, key)
        # the mode's layout
        assert (host['targets'][b, :-1] == -100).all() and host['targets'][b, -1] == host['labels'][b, -1]
        assert len(set(e['classes'])) == n_way and sorted(host['labels'][b, :S_].tolist()) == sorted(list(range(n_way)) * k_shot)
        for j in range(n_way):
            mine = host['src'][b][host['labels'][b] == j]
            assert (mine // n_img == e['classes'][j]).all() and len(set(mine.tolist())) == mine.size
        if mode == 'standard':
            assert all(pool[0] <= c < pool[1] for c in e['classes'])
        else:
            first = offsets[e['alphabet']]
            assert sorted(e['classes']) == list(range(first, first + n_way)) and (host['rotations'][b] == 0).all()
            assert host['labels'][b, :S_].tolist() == [j for j in range(n_way) for _ in range(k_shot)]
            if not train:
                assert (host['src'][b, :S_] % n_img < k_shot).all() and host['src'][b, -1] % n_img >= k_shot
        for t in range(T):
            kq = int(host['rotations'][b, host['labels'][b, t]])
            bbox = E.rotated_bbox(values[host['src'][b, t]], kq)
            want_shift = E.device_shift(k['seed'], k['offset'], b * T + t, bbox, size)
            assert tuple(host['bbox'][b, t].tolist()) == bbox and tuple(host['shift'][b, t].tolist()) == want_shift, (b, t)
            if b < 3:
                assert (host['x'][t, b].view(np.uint32) == E.transform(values[host['src'][b, t]], kq, *want_shift).reshape(-1).view(np.uint32)).all(), (b, t)
    if mode == 'standard':
        assert len(set(host['rotations'].reshape(-1).tolist())) == 4 and len({tuple(row) for row in host['labels'][:, :S_].tolist()}) > B // 2


def test_sample_translates_only_when_asked():
    k = SAMPLE
    bank = sample_bank('uint8')[1]
    r = hipops.episode_sample(bank, 4, k['n_way'], k['k_shot'], 'standard', True, False, k['seed'], offset=k['offset'], num_classes_used=k['used'])
    on = sampled('standard', True)
    assert (r['shift'] == 0).all() and torch.equal(r['src'], on['src'][:4]) and (on['shift'] != 0).any()


@pytest.mark.parametrize('mode,train', CASES)
def test_sample_is_a_function_of_seed_offset_and_dataset_index_in_both_bank_formats(mode, train):
    r = sampled(mode, train)
    f32 = sampled(mode, train, 'f32')
    for key in r:
        assert torch.equal(bits(f32[key]), bits(r[key])), key      # the two bank formats are two instantiations of the same kernels
    one = sampled(mode, train, B=1, first=5)
    for key in r:
        whole = r[key][:, 5:6] if key == 'x' else r[key][5:6]
        assert torch.equal(bits(one[key]), bits(whole)), key
    other = sampled(mode, train, offset=SAMPLE['offset'] + 1)
    assert not torch.equal(other['src'], r['src']) and not torch.equal(other['x'], r['x']) and not torch.equal(other['classes'], r['classes'])


def test_sample_distribution_at_a_fixed_seed():
    """chi-square against the exact uniform laws at one fixed seed (a fixed outcome, not a flaky one), all accepted at p > 1e-4.  The draws are a function of
    the seed, so the seed was chosen on the CPU such that the host replay passes (tests/test_host_episode.py runs that replay through the same statistics)."""
    k = E.DIST
    bank = omniglot.ImageBank.from_arrays(E.distribution_bank(), E.TABLE, k['n_train'], k['train_offsets'], k['test_offsets'], device=DEV)
    calls = [hipops.episode_sample(bank, k['B'], k['n_way'], k['k_shot'], mode, train, True, k['seed'], offset=offset) for mode, train, offset in E.DIST_CALLS]
    results = E.distribution_statistics(*[{key: v.cpu().numpy() for key, v in r.items() if key != 'x'} for r in calls])
    for name, (chi2, p) in results.items():
        print(f'{name}: chi2 {chi2:.2f}, p {p:.4f}')
    print(f'smallest p {min(p for _, p in results.values()):.4f}')
    for name, (chi2, p) in results.items():
        assert p > P_MIN, (name, chi2, p)
    # a few datasets of the big batch against the host replay
    host = calls[0]
    for b in (0, 1, k['B'] - 1):
        e = E.device_episode(k['seed'], E.DIST_CALLS[0][2], b, k['n_way'], k['k_shot'], k['n_img'], 'standard', True, pool=(0, k['n_train']))
        assert host['src'][b].tolist() == e['src'] and host['rotations'][b].tolist() == e['rotations']


# ---- the loader -------------------------------------------------------------------------------------------------------------------------------------------------
class StandIn(torch.nn.Module):
    """A model for validate: logits from the labels it is shown (one-hot of y: every query right) or a constant class."""

    def __init__(self, n_out, constant=None):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=DEV))
        self.n_out, self.constant, self.seen = n_out, constant, []

    def forward(self, data, single_eval_pos=None):
        x, y = data
        assert x.is_cuda and y.is_cuda and not self.training
        self.seen.append((x, y))
        shown = y[single_eval_pos:] if self.constant is None else torch.full_like(y[single_eval_pos:], self.constant)
        return torch.nn.functional.one_hot(shown, self.n_out).float()


def test_validate_with_stand_in_models():
    bank = sample_bank('uint8')[1]
    dl = omniglot.DataLoader(num_steps=3, batch_size=64, seq_len=11, num_features=784, num_outputs=5, jonas_style=True, bank=bank, device=DEV, seed=5)
    right = StandIn(5)
    score = dl.validate(right)
    assert not score.is_cuda and float(score) == 1.0 and len(right.seen) == 3
    # the inner loader: test split, the default style whatever this loader's is, no translation
    assert dl.t_dl.train is False and dl.t_dl.jonas_style is False and dl.t_dl.bank is bank and len(dl.t_dl) == 3
    x, y = right.seen[0]
    assert tuple(x.shape) == (11, 64, 784) and x.dtype == torch.float32 and tuple(y.shape) == (11, 64) and y.dtype == torch.int64
    constant = StandIn(5, constant=0)
    score = dl.validate(constant)
    last = torch.cat([y[-1] for _, y in constant.seen])
    assert last.numel() == 192 and float(score) == float((last == 0).float().mean()) and 0 < float(score) < 0.5
    # one step of the loader itself
    (x, y), target = next(iter(dl))
    assert tuple(x.shape) == (11, 64, 784) and x.is_cuda and y.dtype == target.dtype == torch.int64 and tuple(target.shape) == (11, 64)
    assert (target[:-1] == -100).all() and torch.equal(target[-1], y[-1]) and y[:-1].t().tolist() == [[j for j in range(5) for _ in range(2)]] * 64
    assert not torch.equal(next(iter(dl))[0][0], x)      # a fresh draw on every step


class RecordingLoader(omniglot.DataLoader):
    scores = []

    def validate(self, model, eval_pos=-1):
        score = super().validate(model, eval_pos)
        RecordingLoader.scores.append(float(score))
        return score


def test_the_notebooks_fine_tuning_call_at_a_small_shape():
    """FewShotOmniglot.ipynb's second half through the public surface: pre-train one step on the stroke prior, then fine-tune on episodes with translation
    augmentation in the notebook's style, validating after the epoch.  The plumbing, not learning."""
    from transformerscandobayesianinference_amd.train import Losses, train
    torch.manual_seed(0)
    model_kwargs = dict(bptt=11, single_eval_pos_gen=10, emsize=64, nhead=2, nhid=128, nlayers=2, batch_size=32, epochs=1, verbose=False)
    _, _, pretrained = train(priors.stroke.DataLoader, Losses.ce, encoders.Linear, y_encoder_generator=encoders.get_Canonical(5), steps_per_epoch=1, **model_kwargs,
                             extra_prior_kwargs_dict={'num_features': 784, 'num_outputs': 5, 'only_train_for_last_idx': True})
    bank = sample_bank('uint8')[1]
    RecordingLoader.scores.clear()
    loss, positional, model = train(RecordingLoader, Losses.ce, encoders.Linear, y_encoder_generator=encoders.get_Canonical(5), steps_per_epoch=4, **model_kwargs,
                                    load_weights_from_this_state_dict=pretrained.state_dict(), validation_period=1,
                                    extra_prior_kwargs_dict={'num_features': 784, 'num_outputs': 5, 'translations': True, 'jonas_style': True, 'bank': bank})
    print(f'loss {loss:.4f}, validation score {RecordingLoader.scores}')
    assert math.isfinite(loss) and 0 < loss < 2 * math.log(5)
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert len(RecordingLoader.scores) == 1 and 0 <= RecordingLoader.scores[0] <= 1
