"""Lens-shading correction restated in numpy, integers only - the definition of include/risp.h, independent of the kernels.

A map is ``gains`` (GH,GW,4) uint16 in Q12 and ``k`` = log2 of the cell size; node (i,j) sits at sensor pixel (i << k, j << k),
GH == ((H-1) >> k) + 2, GW == ((W-1) >> k) + 2; the plane of pixel (y,x) is 2 * (y & 1) + (x & 1) in the coordinates of the frame
as stored.  Every intermediate is held in uint64 and asserted to fit unsigned 32 bits, which is what the definition promises."""
import numpy as np

U32 = (1 << 32) - 1


def map_shape(h, w, k):
    return ((h - 1) >> k) + 2, ((w - 1) >> k) + 2


def _check(gains, k, h, w):
    gains = np.asarray(gains)
    assert gains.dtype == np.uint16 and 2 <= k <= 8, (gains.dtype, k)
    assert gains.shape == map_shape(h, w, k) + (4,), (gains.shape, map_shape(h, w, k))
    return gains.astype(np.uint64)


def gain_ref(gains, k, h, w, variant=None):
    """(H,W) uint64 Q12 gain of every pixel.  ``variant`` names one of the wrong forms a test tells apart from the definition:
    'swap_x' (the planes swapped along x) or 'nearest' (the node at the cell's corner instead of the interpolation)"""
    g = _check(gains, k, h, w)
    cell = 1 << k
    y, x = np.mgrid[0:h, 0:w].astype(np.uint64)
    c = (2 * (y & 1) + ((x & 1) ^ (1 if variant == 'swap_x' else 0))).astype(np.int64)
    i, j = (y >> k).astype(np.int64), (x >> k).astype(np.int64)
    fy, fx = y & (cell - 1), x & (cell - 1)
    if variant == 'nearest':
        return g[i, j, c]
    top = (cell - fx) * g[i, j, c] + fx * g[i, j + 1, c]
    bot = (cell - fx) * g[i + 1, j, c] + fx * g[i + 1, j + 1, c]
    num = (cell - fy) * top + fy * bot + (1 << (2 * k - 1))
    assert num.max() <= U32
    return num >> (2 * k)


def shade_ref(raw, black_level, gains, k, variant=None):
    """(..,H,W) integer samples 0 .. 65535 -> (..,H,W) uint16 shaded samples.  ``variant``: those of ``gain_ref`` and 'trunc'
    (the product truncated instead of rounded)"""
    raw = np.asarray(raw)
    assert raw.min() >= 0 and raw.max() <= 65535 and 0 <= black_level <= 65535
    h, w = raw.shape[-2:]
    g = gain_ref(gains, k, h, w, None if variant == 'trunc' else variant)
    d = np.maximum(raw.astype(np.int64) - int(black_level), 0).astype(np.uint64)
    prod = d * g + (0 if variant == 'trunc' else 2048)
    assert prod.max() <= U32
    return np.minimum(prod >> 12, 65535).astype(np.uint16)


def shade_signed32(raw, black_level, gains, k):
    """what the definition gives when the two sums are held in signed 32 bits (wrapped, arithmetic shifts): the mistake the
    extremes are there to show"""
    raw = np.asarray(raw)
    h, w = raw.shape[-2:]
    g = _check(gains, k, h, w).astype(np.int64)
    cell = 1 << k
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    c, i, j, fy, fx = 2 * (y & 1) + (x & 1), y >> k, x >> k, y & (cell - 1), x & (cell - 1)

    def wrap(v):
        return ((v + (1 << 31)) & U32) - (1 << 31)

    top = (cell - fx) * g[i, j, c] + fx * g[i, j + 1, c]
    bot = (cell - fx) * g[i + 1, j, c] + fx * g[i + 1, j + 1, c]
    gq = wrap((cell - fy) * top + fy * bot + (1 << (2 * k - 1))) >> (2 * k)
    d = np.maximum(raw.astype(np.int64) - int(black_level), 0)
    return np.clip(wrap(d * gq + 2048) >> 12, 0, 65535).astype(np.uint16)


def random_map(h, w, k, seed, lo=2048, hi=32767):
    """a map of random gains ``lo`` .. ``hi``, different in every plane and node"""
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi + 1, size=map_shape(h, w, k) + (4,), dtype=np.uint16)


def nearest_bytes(shaded, divisor, cfa_flip=0):
    """The bytes a nearest-demosaic, stage-free pipeline serves for shaded RGGB samples (``cfa_flip`` 0): per 2 x 2 quad R, the
    G of the pixel's own row and B, as B G R, each clip(float32(s') / float32(divisor) * 255) truncated - the expression of
    risp_serve_classical_u8 restated.  (H,W) -> (H,W,3) uint8"""
    assert cfa_flip == 0
    s = np.asarray(shaded).astype(np.float32) / np.float32(divisor)
    h, w = s.shape
    out = np.zeros((h, w, 3), dtype=np.float32)
    r, g0, g1, b = s[0::2, 0::2], s[0::2, 1::2], s[1::2, 0::2], s[1::2, 1::2]
    for py in range(2):
        for px in range(2):
            out[py::2, px::2, 0] = b
            out[py::2, px::2, 1] = g0 if py == 0 else g1
            out[py::2, px::2, 2] = r
    return np.clip(out * np.float32(255), 0, 255).astype(np.uint8)
