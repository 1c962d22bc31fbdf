"""The Omniglot episode loader restated in numpy (csrc/episode.hip, priors/omniglot.py): the per-image transform -- np.rot90 itself, the bounding box and shift
range of reference priors/omniglot.py:13-22, the integer shift that torchvision's affine(angle=0, translate=[tx, ty], NEAREST, fill=0) performs -- and a host
replay of the device sampler's Philox counters (the generator and the integer map are tests/stroke_ref.py's), so that a host test can replay a whole call.
Nothing here is pinned to reference OUTPUT: the reference's loader imports torchvision and reads the image files, and neither is available; the shift rule is
restated, not checked against torchvision.  No GPU."""
import numpy as np
from scipy import stats

import stroke_ref as S

MAX_WAY, MAX_IMAGES = 16, 64      # PFN_EPISODE_MAX_WAY, PFN_EPISODE_MAX_IMAGES
STREAM_CLASS, STREAM_IMAGE, STREAM_MISC, STREAM_ROT, STREAM_SHUFFLE, STREAM_SHIFT = range(6)      # csrc/episode.hip: stream word = offset * 8 + purpose
EMPTY_BBOX = (0, -1, 0, -1)


# ---- the per-image transform --------------------------------------------------------------------------------------------------------------------------------
def bounding_box(rot):
    """(c0, c1, r0, r1) of the pixels != 0 (reference _compute_maxtranslations: rows / columns that are not all background), EMPTY_BBOX without content --
    where the reference raises an IndexError."""
    content = np.asarray(rot) != 0
    rows, cols = np.nonzero(content.any(1))[0], np.nonzero(content.any(0))[0]
    if rows.size == 0:
        return EMPTY_BBOX
    return int(cols[0]), int(cols[-1]), int(rows[0]), int(rows[-1])


def shift_range(bbox, size):
    """((tx_lo, tx_hi), (ty_lo, ty_hi)): [-begin, size - end - 1] per axis; (0, 0) twice without content."""
    c0, c1, r0, r1 = bbox
    if c1 < c0:
        return (0, 0), (0, 0)
    return (-c0, size - 1 - c1), (-r0, size - 1 - r1)


def shifted(rot, tx, ty):
    """out[y][x] = rot[y - ty][x - tx] inside the frame, else 0 of the same dtype."""
    rot = np.asarray(rot)
    size = rot.shape[0]
    out = np.zeros_like(rot)
    ys, xs = np.arange(size) - ty, np.arange(size) - tx
    oky, okx = (ys >= 0) & (ys < size), (xs >= 0) & (xs < size)
    out[np.ix_(oky, okx)] = rot[np.ix_(ys[oky], xs[okx])]
    return out


def transform(image, k, tx, ty):
    return shifted(np.rot90(image, k, axes=(-2, -1)), tx, ty)


def rotated_bbox(image, k):
    return bounding_box(np.rot90(image, k, axes=(-2, -1)))


# ---- the device sampler's draws -----------------------------------------------------------------------------------------------------------------------------
def words(base, stream, seed, count):
    """Word m of a run: component m % 4 of the block at base + m / 4."""
    blocks = (count + 3) // 4
    return S.philox4x32_10(base + np.arange(max(blocks, 1)), stream, seed).reshape(-1)[:count]


def take_subset(k, n, w):
    """The rank rule: draw j takes r = mulhi(word j, n - j), the rank among the values not yet taken."""
    taken, order = [], []
    for j in range(k):
        r = S.u_int(w[j], 0, n - j - 1)
        pos = 0
        while pos < len(taken) and r >= taken[pos]:
            r += 1
            pos += 1
        taken.insert(pos, r)
        order.append(r)
    return order


def permutation(n, w):
    """Fisher-Yates: for i = n-1 .. 1 swap(a[i], a[mulhi(word n-1-i, i + 1)])."""
    a = list(range(n))
    for i in range(n - 1, 0, -1):
        j = S.u_int(w[n - 1 - i], 0, i)
        a[i], a[j] = a[j], a[i]
    return a


def device_episode(seed, offset, dataset, n_way, k_shot, n_img, mode, train, pool=None, alphabet_offsets=None):
    """Dataset `dataset` as the device draws it: dict of classes [n_way], rotations [n_way], labels [T], targets [T], src [T], query class, alphabet."""
    S_, d = n_way * k_shot, dataset
    misc = S.philox4x32_10(d, offset * 8 + STREAM_MISC, seed)
    q = S.u_int(misc[0], 0, n_way - 1)
    alphabet = None
    if mode == 'jonas':
        alphabet = S.u_int(misc[1], 0, len(alphabet_offsets) - 2)
        classes = [alphabet_offsets[alphabet] + c for c in permutation(n_way, words(d * 4, offset * 8 + STREAM_CLASS, seed, 16))]
        perm, rotations = list(range(S_)), [0] * n_way
    else:
        classes = [pool[0] + c for c in take_subset(n_way, pool[1] - pool[0], words(d * 4, offset * 8 + STREAM_CLASS, seed, 16))]
        perm = permutation(S_, words(d * 256, offset * 8 + STREAM_SHUFFLE, seed, max(S_, 1)))
        rotations = [S.u_int(u, 0, 3) for u in words(d * 4, offset * 8 + STREAM_ROT, seed, 16)[:n_way]]
    images = []
    for j in range(n_way):
        w = words((d * 16 + j) * 16, offset * 8 + STREAM_IMAGE, seed, 64)
        if mode == 'jonas' and not train:
            chosen = permutation(k_shot, w)
            if j == q:
                chosen.append(k_shot + S.u_int(w[k_shot - 1], 0, n_img - k_shot - 1))
        else:
            chosen = take_subset(k_shot + (1 if j == q else 0), n_img, w)
        images.append(chosen)
    labels = [perm[p] // k_shot for p in range(S_)] + [q]
    within = [perm[p] % k_shot for p in range(S_)] + [k_shot]
    src = [classes[j] * n_img + images[j][i] for j, i in zip(labels, within)]
    return dict(classes=classes, rotations=rotations, labels=labels, targets=[-100] * S_ + [q], src=src, query=q, alphabet=alphabet, images=images)


def device_shift(seed, offset, image, bbox, size):
    """(tx, ty) of global image index `image` (sample: dataset * T + t; gather: first_image + n) inside the range of `bbox`."""
    (xlo, xhi), (ylo, yhi) = shift_range(bbox, size)
    if bbox[1] < bbox[0]:
        return 0, 0
    u = S.philox4x32_10(image, offset * 8 + STREAM_SHIFT, seed)
    return S.u_int(u[0], xlo, xhi), S.u_int(u[1], ylo, yhi)


# ---- a synthetic bank ---------------------------------------------------------------------------------------------------------------------------------------
TABLE = (1.0 - np.arange(256, dtype=np.float64) / 255.).astype(np.float32)      # the reference's chain x / 255., 1 - x in f64, then f32: byte 255 is the background


def synthetic_bank(n_classes, n_img, size, seed):
    """uint8 [n_classes, n_img, size, size] of random sparse glyphs on paper (byte 255): each a random box, about 40 % of its pixels inked with bytes 0 .. 254."""
    rng = np.random.default_rng(seed)
    bank = np.full((n_classes, n_img, size, size), 255, dtype=np.uint8)
    for c in range(n_classes):
        for i in range(n_img):
            h, w = rng.integers(1, size + 1, 2)
            y0, x0 = rng.integers(0, size - h + 1), rng.integers(0, size - w + 1)
            ink = rng.random((h, w)) < 0.4
            ink[rng.integers(0, h), rng.integers(0, w)] = True      # never empty
            bank[c, i, y0:y0 + h, x0:x0 + w] = np.where(ink, rng.integers(0, 255, (h, w)), 255)
    return bank


def special_images(size):
    """uint8 [n, size, size] on paper 255: a glyph touching each edge, a single pixel in each corner, a full frame, an all-background image, a full row
    (at size 64 the row mask with all 64 bits set), a full column."""
    m, out = size - 1, []
    blank = np.full((size, size), 255, dtype=np.uint8)
    for sl in ((0, slice(2, 5)), (m, slice(1, 4)), (slice(2, 6), 0), (slice(3, 5), m)):      # top, bottom, left, right edge
        im = blank.copy()
        im[sl] = 7
        im[size // 2, size // 2] = 100
        out.append(im)
    for y, x in ((0, 0), (0, m), (m, 0), (m, m)):
        im = blank.copy()
        im[y, x] = 1
        out.append(im)
    out.append(np.full((size, size), 3, dtype=np.uint8))
    out.append(blank.copy())
    im = blank.copy()
    im[size // 2, :] = 9
    out.append(im)
    im = blank.copy()
    im[:, size // 3] = 11
    out.append(im)
    return np.stack(out)


# ---- the distribution test's bank and statistics (shared by the device test and the host replay that chose its seed) -----------------------------------------
def chi2_uniform(values, lo, hi):
    counts = np.bincount(np.asarray(values).reshape(-1) - lo, minlength=hi - lo + 1)
    assert counts.size == hi - lo + 1
    return stats.chisquare(counts)


DIST = dict(C=32, n_img=8, size=8, n_train=20, train_offsets=[0, 5, 9, 14, 20], test_offsets=[20, 26, 32], n_way=4, k_shot=2, B=1024, seed=1, box=(3, 4))
DIST_CALLS = (('standard', True, 1), ('jonas', True, 2), ('jonas', False, 3))      # (mode, train, offset): three independent calls


def distribution_bank():
    """Glyphs whose bounding box is a 3 x 4 box at a random place (its corners inked): without rotation every image has the same shift range, five values of tx
    and six of ty, so the drawn shift can be tested against ONE uniform law."""
    k = DIST
    rng = np.random.default_rng(2)
    h, w = k['box']
    raw = np.full((k['C'], k['n_img'], k['size'], k['size']), 255, dtype=np.uint8)
    for c in range(k['C']):
        for i in range(k['n_img']):
            y0, x0 = rng.integers(0, k['size'] - h + 1), rng.integers(0, k['size'] - w + 1)
            box = np.where(rng.random((h, w)) < 0.5, rng.integers(0, 255, (h, w)), 255)
            box[[0, 0, -1, -1], [0, -1, 0, -1]] = 0
            raw[c, i, y0:y0 + h, x0:x0 + w] = box
    return raw


def distribution_statistics(standard, jonas, jonas_test):
    """name -> (chi2, p) from the integer outputs of three calls (numpy arrays): standard train, jonas train, jonas test."""
    k = DIST
    n_way, k_shot, n_img, size = k['n_way'], k['k_shot'], k['n_img'], k['size']
    h, w = k['box']
    alphabet = np.searchsorted(np.asarray(k['train_offsets']), jonas['classes'].min(1), side='right') - 1
    first_support = standard['src'][np.arange(standard['src'].shape[0]), np.argmax(standard['labels'][:, :-1] == 0, 1)]      # first listed image of class 0
    return {
        'class choice, first pick': chi2_uniform(standard['classes'][:, 0], 0, k['n_train'] - 1),
        'class choice, last pick': chi2_uniform(standard['classes'][:, -1], 0, k['n_train'] - 1),
        'image choice, support': chi2_uniform(first_support % n_img, 0, n_img - 1),
        'image choice, query': chi2_uniform(standard['src'][:, -1] % n_img, 0, n_img - 1),
        'image choice, jonas test query': chi2_uniform(jonas_test['src'][:, -1] % n_img, k_shot, n_img - 1),
        'image choice, jonas test support': chi2_uniform(jonas_test['src'][:, 0] % n_img, 0, k_shot - 1),
        'rotation': chi2_uniform(standard['rotations'], 0, 3),
        'support permutation, first position': chi2_uniform(standard['labels'][:, 0], 0, n_way - 1),
        'query class': chi2_uniform(standard['labels'][:, -1], 0, n_way - 1),
        'query class, jonas': chi2_uniform(jonas['labels'][:, -1], 0, n_way - 1),
        'jonas class order, first': chi2_uniform(jonas['classes'][:, 0] - np.asarray(k['train_offsets'])[alphabet], 0, n_way - 1),
        'alphabet': chi2_uniform(alphabet, 0, len(k['train_offsets']) - 2),
        # no rotation in jonas mode: the shifted box's corner c0 + tx is uniform over 0 .. size - w, r0 + ty over 0 .. size - h
        'shift x': chi2_uniform(jonas['bbox'][..., 0] + jonas['shift'][..., 0], 0, size - w),
        'shift y': chi2_uniform(jonas['bbox'][..., 2] + jonas['shift'][..., 1], 0, size - h),
    }


def replayed_distribution_calls(seed=None):
    """The integer outputs of the three calls of DIST_CALLS replayed on the host (shift and bbox only where distribution_statistics reads them)."""
    k = DIST
    seed = k['seed'] if seed is None else seed
    values = TABLE[distribution_bank()].reshape(-1, k['size'], k['size'])
    boxes = np.array([bounding_box(v) for v in values])
    T = k['n_way'] * k['k_shot'] + 1
    out = []
    for mode, train, offset in DIST_CALLS:
        r = {key: [] for key in ('classes', 'rotations', 'labels', 'src', 'bbox', 'shift')}
        for b in range(k['B']):
            e = device_episode(seed, offset, b, k['n_way'], k['k_shot'], k['n_img'], mode, train, pool=(0, k['n_train']),
                               alphabet_offsets=k['train_offsets'] if train else k['test_offsets'])
            for key in ('classes', 'rotations', 'labels', 'src'):
                r[key].append(e[key])
            if mode == 'jonas' and train:
                r['bbox'].append(boxes[e['src']])
                r['shift'].append([device_shift(seed, offset, b * T + t, tuple(boxes[e['src'][t]]), k['size']) for t in range(T)])
        out.append({key: np.asarray(v) for key, v in r.items() if v})
    return out
