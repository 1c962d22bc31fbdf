"""The stroke prior of the few-shot study restated in numpy (csrc/stroke_prior.hip, priors/stroke.py): what Pillow does for ImageDraw.line(fill, width) on
an 8-bit canvas and for ImageFilter.GaussianBlur(0.2), the reference's class loop and per-image draws (reference priors/stroke.py:9-63), the scaling to [0, 1]
and the per-image normalisation in f64, and the counter-based draws of the device sampler (Philox4x32-10) so that a host test can replay a whole call.  No GPU,
no Pillow (tools/make_stroke_golden.py checks this file against it).

f32 is used exactly where Pillow uses it: an edge's slope, its intersection with a scan line (a multiply and an add that round separately -- `contract=True`
rounds them once, as a fused multiply-add would, which is NOT what Pillow computes) and the rounding of a span's ends."""
import math

import numpy as np

MAX_STROKES = 8          # PFN_STROKE_MAX_STROKES
MAX_PASSES = 256         # PFN_STROKE_MAX_PASSES: the cap on the class loop's retries
COORD_LIMIT = 4096       # PFN_STROKE_COORD_LIMIT: a stroke with a coordinate beyond +-this is not drawn
NOISE_LO, NOISE_N = 200, 55      # np.random.randint(200, 255): 200 .. 254
BLUR_WW, BLUR_FW = 16553519, 111848
F32 = np.float32
F32_UNIT_ROUNDOFF = 2.0 ** -24


# ---- Pillow's two roundings (Draw.c ROUND_UP / ROUND_DOWN) --------------------------------------------------------------------------------------------------
def ru(f):
    """f64: floor(f + 1/2) away from zero."""
    return int(math.floor(f + 0.5)) if f >= 0 else -int(math.floor(abs(f) + 0.5))


def rd(f):
    return int(math.ceil(f - 0.5)) if f >= 0 else -int(math.ceil(abs(f) - 0.5))


def ru32(f):
    """The same on an f32 value with the sum rounded to f32, as a span's ends are."""
    f = F32(f)
    return int(np.floor(F32(f + F32(0.5)))) if f >= 0 else -int(np.floor(F32(np.abs(f) + F32(0.5))))


def rd32(f):
    f = F32(f)
    return int(np.ceil(F32(f - F32(0.5)))) if f >= 0 else -int(np.ceil(F32(np.abs(f) - F32(0.5))))


# ---- the rasteriser -----------------------------------------------------------------------------------------------------------------------------------------
def _span(mask, y, xa, xb):
    size = mask.shape[0]
    if not 0 <= y < size or xa >= size or xb < 0:
        return
    xa, xb = max(xa, 0), min(xb, size - 1)
    if xa <= xb:
        mask[y, xa:xb + 1] = True


def _point(mask, x, y):
    size = mask.shape[0]
    if 0 <= x < size and 0 <= y < size:
        mask[y, x] = True


def _thin_line(mask, x0, y0, x1, y1):
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    xs, ys = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
    x, y = x0, y0
    if dx == 0:
        for _ in range(dy):
            _point(mask, x, y)
            y += ys
    elif dy == 0:
        for _ in range(dx):
            _point(mask, x, y)
            x += xs
    elif dx > dy:
        e = 2 * dy - dx
        for _ in range(dx):
            _point(mask, x, y)
            if e >= 0:
                y += ys
                e -= 2 * dx
            e += 2 * dy
            x += xs
    else:
        e = 2 * dx - dy
        for _ in range(dy):
            _point(mask, x, y)
            if e >= 0:
                x += xs
                e -= 2 * dy
            e += 2 * dx
            y += ys
    _point(mask, x1, y1)


def wide_line_vertices(x0, y0, x1, y1, width):
    dx, dy = x1 - x0, y1 - y0
    h = math.sqrt(float(dx * dx + dy * dy))      # hypot of two integers: the sum of squares is exact
    s = (width - 1) / 2.0
    rmax, rmin = ru(s) / h, rd(s) / h
    dxmin, dxmax = rd(rmin * dy), rd(rmax * dy)
    dymin, dymax = ru(rmin * dx), ru(rmax * dx)
    return [(x0 - dxmin, y0 + dymax), (x1 - dxmin, y1 + dymax), (x1 + dxmax, y1 - dymin), (x0 + dxmax, y0 - dymin)]


def edge_x(y, x0, y0, x1, y1, contract=False):
    m = F32(F32(x1 - x0) / F32(y1 - y0))
    if contract:      # one rounding: the product of two f32 is exact in f64
        return F32(np.float64(F32(y - y0)) * np.float64(m) + np.float64(x0))
    return F32(F32(F32(y - y0) * m) + F32(x0))


def _fill_polygon(mask, v, contract=False):
    size = mask.shape[0]
    n = len(v)
    edges = []
    pymin, pymax = min(p[1] for p in v), max(p[1] for p in v)
    for i in range(n):
        (x0, y0), (x1, y1) = v[i], v[(i + 1) % n]
        if y0 == y1:
            _span(mask, y0, min(x0, x1), max(x0, x1))
        else:
            edges.append((x0, y0, x1, y1))
    for y in range(max(pymin, 0), min(pymax, size - 1) + 1):
        xs = []
        for x0, y0, x1, y1 in edges:
            if min(y0, y1) <= y <= max(y0, y1):
                xs.append(edge_x(y, x0, y0, x1, y1, contract))
                if y == max(y0, y1) and y < pymax:
                    xs.append(xs[-1])
        xs.sort()
        for i in range(1, len(xs), 2):
            _span(mask, y, ru32(xs[i - 1]), rd32(xs[i]))


def line_mask(size, seg, width, contract=False, mask=None):
    """The pixels ImageDraw.line([x0, y0, x1, y1], width=width) lights on a size x size canvas, OR-ed into `mask` [y, x]."""
    if mask is None:
        mask = np.zeros((size, size), dtype=bool)
    x0, y0, x1, y1 = (int(c) for c in seg)
    if max(abs(x0), abs(y0), abs(x1), abs(y1)) > COORD_LIMIT:
        return mask
    if width <= 1:
        _thin_line(mask, x0, y0, x1, y1)
    elif (x0, y0) == (x1, y1):
        _point(mask, x0, y0)
    else:
        _fill_polygon(mask, wide_line_vertices(x0, y0, x1, y1, width), contract)
    return mask


def image_mask(size, segs, n_strokes, width, contract=False):
    mask = np.zeros((size, size), dtype=bool)
    for s in range(int(n_strokes)):
        line_mask(size, segs[s], int(width), contract, mask)
    return mask


def raw_image(size, segs, n_strokes, width, noise, contract=False):
    """uint8 [size, size]: the noise byte where a stroke lit the pixel, else 0."""
    mask = image_mask(size, segs, n_strokes, width, contract)
    return np.where(mask, np.asarray(noise, dtype=np.uint8).reshape(size, size), 0).astype(np.uint8)


def noise_field(raw):
    """A full noise field from a recorded raw image: the recorded byte where a pixel is lit, a fixed filler in 200 .. 254 elsewhere (the noise of an unlit pixel
    reaches no image, so fixtures do not store it; under the filler a wrongly lit pixel shows)."""
    raw = np.asarray(raw, dtype=np.uint8)
    filler = (NOISE_LO + (np.arange(raw.size) * 7) % NOISE_N).astype(np.uint8).reshape(raw.shape)
    return np.where(raw != 0, raw, filler)


# ---- GaussianBlur(0.2) --------------------------------------------------------------------------------------------------------------------------------------
def blur_constants(sigma=0.2, passes=3):
    """Pillow's box radius for one of `passes` passes (the fractional part `a`; the integer part is 0 here) and its two 8.24 fixed-point weights."""
    sigma2 = F32(sigma) * F32(sigma) / passes
    box = math.sqrt(12.0 * sigma2 + 1.0)
    l = math.floor((box - 1.0) / 2.0)
    a = (2 * l + 1) * (l * (l + 1) - 3.0 * sigma2) / (6 * (sigma2 - (l + 1) * (l + 1)))
    assert l == 0
    radius = F32(l + a)
    ww = int(F32(1 << 24) / F32(radius * F32(2) + F32(1)))
    return ww, ((1 << 24) - ww) // 2


def _box_pass_rows(img):
    c = img.astype(np.uint64)
    left = np.concatenate([c[:, :1], c[:, :-1]], 1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out = (c * BLUR_WW + (left + right) * BLUR_FW + (1 << 23)) >> 24
    assert int((c * BLUR_WW + (left + right) * BLUR_FW + (1 << 23)).max()) < 2 ** 32
    return out.astype(np.uint8)


def blur(raw):
    img = np.asarray(raw, dtype=np.uint8)
    for _ in range(3):
        img = _box_pass_rows(img)
    img = img.T
    for _ in range(3):
        img = _box_pass_rows(img)
    return np.ascontiguousarray(img.T)


# ---- output -------------------------------------------------------------------------------------------------------------------------------------------------
BYTE_TO_X = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)      # byte / 255, correctly rounded in f32


def to_x(img):
    return BYTE_TO_X[np.asarray(img, dtype=np.uint8)].reshape(-1)


def normalized_f64(img):
    """(x - mean) / (std + 1e-6) over the image, std the unbiased one, in f64 from the f32 values of to_x."""
    x = to_x(img).astype(np.float64)
    return (x - x.mean()) / (x.std(ddof=1) + 1e-6)


def normalized_error(x, x64):
    """The statistic the bound 3 max(e, u) is about: the largest error of an image relative to its largest magnitude."""
    x64 = np.asarray(x64, dtype=np.float64)
    return float(np.abs(np.asarray(x, dtype=np.float64) - x64).max() / max(np.abs(x64).max(), 1e-30))


# ---- the reference's draws ----------------------------------------------------------------------------------------------------------------------------------
def int_bounds(size, min_max_strokes=(1, 3), min_max_len=(5 / 28, 20 / 28), min_max_start=(2 / 28, 25 / 28), min_max_width=(1 / 28, 4 / 28), max_offset=4 / 28,
               max_target_offset=2 / 28):
    """The integer ranges the reference draws from, with its own truncating arithmetic (note int(-size * f), not -int(size * f))."""
    return dict(strokes=(int(min_max_strokes[0]), int(min_max_strokes[1])), len=(int(size * min_max_len[0]), int(size * min_max_len[1])),
                start=(int(size * min_max_start[0]), int(size * min_max_start[1])), width=(int(size * min_max_width[0]), int(size * min_max_width[1])),
                offset=(int(-size * max_offset), int(size * max_offset)), jitter=(int(-size * max_target_offset), int(size * max_target_offset)))


def class_loop(size, bounds, randint, rand_angle, max_passes=MAX_PASSES, predraw=False):
    """One class: (lens, starts, angles, capped).  randint(lo, hi) is inclusive; rand_angle() is uniform in [0, 2 pi).  `predraw` also makes the draws the
    reference makes before its loop (n lengths, then n starts), which the loop's first pass overwrites: needed only to replay a log of its draws."""
    n = randint(*bounds['strokes'])
    if predraw:
        for lo, hi in [bounds['len']] * n + [bounds['start']] * (2 * n):
            randint(lo, hi)
    lens, starts, angles, capped = [], [], [], 0
    for _ in range(n):
        length, sp, theta = 0, (0, 0), 0.0
        for counter in range(max_passes):
            if counter % 3 == 0:
                length = randint(*bounds['len'])
                sp = (randint(*bounds['start']), randint(*bounds['start']))
            theta = rand_angle()
            p = (sp[0] + math.cos(theta) * length, sp[1] + math.sin(theta) * length)
            if all(0 <= c <= size - 1 for c in p):
                break
        else:
            capped += 1
        lens.append(length), starts.append(sp), angles.append(theta)
    return lens, starts, angles, capped


def image_segments(lens, starts, angles, offset, jitters):
    """p0 = start + offset; p1 = round_half_even(p0 + (len (cos, sin) + jitter)) in the reference's order of operations.  Also returns the smallest distance
    of an unrounded coordinate from a rounding tie."""
    segs, tie = [], 1.0
    for length, sp, theta, jit in zip(lens, starts, angles, jitters):
        p0 = (sp[0] + offset[0], sp[1] + offset[1])
        f = (p0[0] + (math.cos(theta) * length + jit[0]), p0[1] + (math.sin(theta) * length + jit[1]))
        tie = min(tie, *(abs(abs(c - math.floor(c)) - 0.5) for c in f))
        segs.append((p0[0], p0[1], round(f[0]), round(f[1])))
    return segs, tie


# ---- the device sampler's draws -----------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(idx, stream, seed):
    """csrc/pfn_device.h philox4x32_10 on arrays of counters: returns uint32 [..., 4]."""
    idx = np.asarray(idx, dtype=np.uint64)
    stream = np.uint64(stream)
    m32 = np.uint64(0xFFFFFFFF)
    c = [idx & m32, idx >> np.uint64(32), np.broadcast_to(stream & m32, idx.shape), np.broadcast_to(stream >> np.uint64(32), idx.shape)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def u_int(u, lo, hi):
    """lo + mulhi(u, hi - lo + 1): every value's probability is within 2^-32 of uniform (a bias below n 2^-32 over n values)."""
    return int(lo) + int((int(u) * (int(hi) - int(lo) + 1)) >> 32)


def u_angle(u):
    return float(int(u)) * (2.0 * math.pi / 4294967296.0)


STREAM_CLASS_N, STREAM_CLASS_PASS, STREAM_IMAGE, STREAM_JITTER, STREAM_NOISE = 0, 1, 2, 3, 4      # csrc/stroke_prior.hip: stream word = offset * 8 + purpose
MAX_CLASSES = 16


def device_class(size, bounds, seed, offset, dataset, c, num_classes):
    """The class (dataset, c) as the device draws it: (lens, starts, angles, capped)."""
    n = u_int(philox4x32_10(dataset * num_classes + c, offset * 8 + STREAM_CLASS_N, seed)[0], *bounds['strokes'])
    lens, starts, angles, capped = [], [], [], 0
    for s in range(n):
        base = ((dataset * MAX_CLASSES + c) * MAX_STROKES + s) * MAX_PASSES
        r = philox4x32_10(base + np.arange(MAX_PASSES), offset * 8 + STREAM_CLASS_PASS, seed)
        length, sp, theta = 0, (0, 0), 0.0
        for p in range(MAX_PASSES):
            if p % 3 == 0:
                length = u_int(r[p, 0], *bounds['len'])
                sp = (u_int(r[p, 1], *bounds['start']), u_int(r[p, 2], *bounds['start']))
            theta = u_angle(r[p, 3])
            q = (sp[0] + math.cos(theta) * length, sp[1] + math.sin(theta) * length)
            if all(0 <= v <= size - 1 for v in q):
                break
        else:
            capped += 1
        lens.append(length), starts.append(sp), angles.append(theta)
    return lens, starts, angles, capped


def device_image_draws(bounds, seed, offset, image):
    """(width, offset (x, y), jitters [8] of (x, y)) of global image index `image` = dataset * T + t."""
    r = philox4x32_10(image, offset * 8 + STREAM_IMAGE, seed)
    width = u_int(r[0], *bounds['width'])
    off = (u_int(r[1], *bounds['offset']), u_int(r[2], *bounds['offset']))
    j = philox4x32_10(image * 4 + np.arange(4), offset * 8 + STREAM_JITTER, seed).reshape(8, 2)
    return width, off, [(u_int(a, *bounds['jitter']), u_int(b, *bounds['jitter'])) for a, b in j]


def device_noise(size, seed, offset, image):
    """uint8 [size, size]: word k of the block at counter (image * 64 + y) * 16 + x // 4 is pixel x = 4 (x // 4) + k of row y."""
    y, xq = np.meshgrid(np.arange(size), np.arange((size + 3) // 4), indexing='ij')
    r = philox4x32_10((image * 64 + y) * 16 + xq, offset * 8 + STREAM_NOISE, seed).reshape(size, -1)[:, :size]
    return (NOISE_LO + ((r.astype(np.uint64) * NOISE_N) >> np.uint64(32))).astype(np.uint8)
