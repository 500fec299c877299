"""Output sharpening (risp_bgr8_sharpen; include/risp.h has the definition) restated in numpy int64, the named wrong variants a
test must be able to tell from it, and the case table tests/test_sharpen_reference_cpu.py and tests/test_gpu_sharpen.py share.

    L = (77 R + 150 G + 29 B + 128) >> 8
    S = sum over the (2 radius + 1)^2 window, indices clamped into the image, of w * L        (w sums to 256, no rounding)
    D = 256 L - S;  A = max(|D| - 256 threshold, 0);  E = min((A * amount + 32768) >> 16, limit)
    c' = clamp(c + sign(D) * E, 0, 255) for B, G and R alike
"""
import numpy as np

RADII = (1, 2)
MAX_AMOUNT = 4095
MAX_DETAIL = 65280                      # |D| <= 256 * 255
TAPS = {1: (1, 2, 1), 2: (1, 4, 6, 4, 1)}
SCALE = {1: 16, 2: 1}                   # radius 1: 16 * ([1 2 1] (x) [1 2 1]), radius 2: [1 4 6 4 1] (x) [1 4 6 4 1]; both sum to 256

VARIANTS = ('luma_without_rounding', 'rb_not_swapped', 'reflected_border', 'hard_coring', 'limit_before_gain',
            'gain_without_rounding', 'rounded_separable_blur', 'per_channel_detail')


def luma(img, channels='bgr', variant=None):
    """(..,H,W,3) uint8 -> (..,H,W) int64 in 0 .. 255"""
    c = img.astype(np.int64)
    first, g, third = c[..., 0], c[..., 1], c[..., 2]
    r, b = (first, third) if channels == 'rgb' and variant != 'rb_not_swapped' else (third, first)
    return (77 * r + 150 * g + 29 * b + (0 if variant == 'luma_without_rounding' else 128)) >> 8


def _index(n, d, reflect):
    """the source index of every position 0 .. n-1 moved by d: clamped (replicate), or reflected about the border pixel"""
    i = np.arange(n, dtype=np.int64) + d
    if reflect:
        i = np.where(i < 0, -i, i)
        i = np.where(i > n - 1, 2 * (n - 1) - i, i)
    return np.clip(i, 0, n - 1)


def _pass(x, axis, radius, reflect):
    out = np.zeros_like(x)
    for t, w in enumerate(TAPS[radius]):
        out += w * np.take(x, _index(x.shape[axis], t - radius, reflect), axis=axis)
    return out


def blur(L, radius, variant=None):
    """(..,H,W) int64 luma -> the Q8 blur S"""
    reflect = variant == 'reflected_border'
    h = _pass(L, L.ndim - 1, radius, reflect)
    if variant == 'rounded_separable_blur':             # the horizontal pass rounded to a code in between
        total = sum(TAPS[radius])
        h = (h + total // 2) // total
        return _pass(h, L.ndim - 2, radius, reflect) * (256 // total)
    return _pass(h, L.ndim - 2, radius, reflect) * SCALE[radius]


def step(D, amount, threshold, limit, variant=None):
    """the signed step sign(D) * E of a detail D"""
    mag = np.abs(D)
    if variant == 'hard_coring':
        A = np.where(mag > 256 * threshold, mag, 0)
    else:
        A = np.maximum(mag - 256 * threshold, 0)
    assert int(A.max(initial=0)) * MAX_AMOUNT + 32768 < 2 ** 32
    rnd = 0 if variant == 'gain_without_rounding' else 32768
    if variant == 'limit_before_gain':
        E = (np.minimum(A, 256 * limit) * amount + rnd) >> 16
    else:
        E = np.minimum((A * amount + rnd) >> 16, limit)
    return np.sign(D) * E


def sharpen(img, params, channels='bgr', variant=None):
    """(N,H,W,3) or (H,W,3) uint8, params = (amount, threshold, limit, radius) -> the same shape, uint8"""
    amount, threshold, limit, radius = params
    assert img.dtype == np.uint8 and img.shape[-1] == 3 and radius in RADII
    assert 0 <= amount <= MAX_AMOUNT and 0 <= threshold <= 255 and 0 <= limit <= 255
    c = img.astype(np.int64)
    if variant == 'per_channel_detail':
        st = np.stack([step(256 * c[..., k] - blur(c[..., k], radius), amount, threshold, limit) for k in range(3)], axis=-1)
    else:
        L = luma(img, channels, variant)
        D = 256 * L - blur(L, radius, variant)
        assert int(np.abs(D).max(initial=0)) <= MAX_DETAIL
        st = step(D, amount, threshold, limit, variant)[..., None]
    return np.clip(c + st, 0, 255).astype(np.uint8)


def events(img, params, channels='bgr'):
    """how often each thing the definition provides for happens on an image: a dict of counts"""
    amount, threshold, limit, radius = params
    c = img.astype(np.int64)
    L = luma(img, channels)
    D = 256 * L - blur(L, radius)
    A = np.maximum(np.abs(D) - 256 * threshold, 0)
    gained = (A * amount + 32768) >> 16
    st = step(D, amount, threshold, limit)
    H, W = L.shape[-2:]
    y = np.arange(H).reshape((1,) * (L.ndim - 2) + (H, 1))
    x = np.arange(W).reshape((1,) * (L.ndim - 2) + (1, W))
    moved = st != 0
    return {
        'cored': int(((D != 0) & (A == 0)).sum()), 'limited': int((gained > limit).sum()),
        'clamped_at_0': int((c + st[..., None] < 0).sum()), 'clamped_at_255': int((c + st[..., None] > 255).sum()),
        'positive': int((D > 0).sum()), 'negative': int((D < 0).sum()),
        'top': int((moved & (y < radius)).sum()), 'bottom': int((moved & (y > H - 1 - radius)).sum()),
        'left': int((moved & (x < radius)).sum()), 'right': int((moved & (x > W - 1 - radius)).sum()),
    }


EVENTS = ('cored', 'limited', 'clamped_at_0', 'clamped_at_255', 'positive', 'negative', 'top', 'bottom', 'left', 'right')

# ---------------------------------------------------------------- the cases both test files share
# the kernel's tile is 64 x 16: one pixel, sizes below the blur's window, a row, a column-poor image, exactly one tile, one more
# and one less than a tile on both axes, and more than one tile on both axes with neither a multiple
SIZES = ((1, 1), (2, 2), (1, 7), (5, 3), (16, 64), (17, 65), (15, 63), (33, 130))
N_IMAGES = 3
# (amount, threshold, limit): a moderate gain that the limit cuts, a strong one with a wide limit, a gain below 1.0
_SETTINGS = ((384, 4, 40), (1024, 12, 96), (200, 2, 255))


def _cases():
    out = []
    for si, (h, w) in enumerate(SIZES):
        for radius in RADII:
            for ci, channels in enumerate(('bgr', 'rgb')):
                a, t, l = _SETTINGS[(si + radius + ci) % len(_SETTINGS)]
                out.append(dict(name='%dx%d-r%d-%s' % (h, w, radius, channels), size=(h, w), params=(a, t, l, radius),
                                channels=channels, seed=100 * si + 10 * radius + ci, identity=(h, w) == (1, 1)))
    # the extremes, on the size that is one more than a tile
    for radius in RADII:
        for tag, (a, t, l), ident in (('amount4095', (4095, 0, 255), False), ('threshold255', (4095, 255, 255), True),
                                      ('limit0', (300, 10, 0), True), ('amount0', (0, 0, 255), True),
                                      ('limit1', (4095, 0, 1), False)):
            out.append(dict(name='17x65-r%d-%s' % (radius, tag), size=(17, 65), params=(a, t, l, radius), channels='bgr',
                            seed=900 + radius, identity=ident))
    return out


CASES = _cases()
NV12_SIZES = ((2, 2), (4, 6), (18, 66))
NV12_MATRICES = ('bt601_full', 'bt709_video')


def case_image(case, n=N_IMAGES):
    """the images of a case: uniform random bytes, (n,H,W,3) uint8"""
    h, w = case['size']
    return np.random.RandomState(case['seed']).randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)
