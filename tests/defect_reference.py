"""Defective-pixel correction restated in numpy int64 - the definition of include/risp.h, independent of the kernels.

S(y,x) is the raw sample; an index outside the frame reflects without repeating the edge.  The pairs, in this order:
H S(y,x-2), S(y,x+2); V S(y-2,x), S(y+2,x); D S(y-2,x-2), S(y+2,x+2); A S(y-2,x+2), S(y+2,x-2).  mx / mn are the extremes of the
eight, T(v) = threshold + ((v * slope) >> 8); hot: p > mx + T(mx); dead: p + T(mn) < mn; listed: the pixel's bit of the map.  Such
a pixel becomes (a + b + 1) >> 1 of the pair with the smallest |a - b|, the first in the order above on a tie.  Every sum is
asserted to fit unsigned 32 bits, which is what the definition promises."""
import numpy as np

U32 = (1 << 32) - 1
VARIANTS = ('clamp', 'dist1', 'vfirst', 'afirst', 'lasttie', 'trunc', 'ge', 'slope_p', 'hotonly', 'wrap16', 'recursive')


def map_ref(coords, H, W):
    """(y, x) pairs -> the (H, (W+31)//32) int32 bitmap: bit x & 31 of word x >> 5 of row y"""
    words = [[0] * ((W + 31) // 32) for _ in range(H)]
    for y, x in coords:
        assert 0 <= y < H and 0 <= x < W
        words[y][x >> 5] |= 1 << (x & 31)
    return np.array(words, dtype=np.uint32).reshape(H, (W + 31) // 32).view(np.int32)


def listed_ref(bitmap, H, W):
    """the (H,W) bool plane of a bitmap (None: nothing listed)"""
    if bitmap is None:
        return np.zeros((H, W), dtype=bool)
    b = np.asarray(bitmap)
    assert b.shape == (H, (W + 31) // 32) and b.dtype in (np.int32, np.uint32), (b.shape, b.dtype)
    x = np.arange(W)
    return ((b.view(np.uint32).astype(np.int64)[:, x >> 5] >> (x & 31)) & 1).astype(bool)


def _decide(p, pairs, listed, threshold, slope, variant):
    """the corrected value of samples p (any shape, int64) given their four pairs in the order H, V, D, A"""
    if variant == 'vfirst':
        pairs = [pairs[1], pairs[0], pairs[2], pairs[3]]
    if variant == 'afirst':
        pairs = [pairs[0], pairs[1], pairs[3], pairs[2]]
    wrap = (lambda v: v & 0xFFFF) if variant == 'wrap16' else (lambda v: v)
    flat = [v for pair in pairs for v in pair]
    mx, mn = np.maximum.reduce(flat), np.minimum.reduce(flat)
    bad = np.broadcast_to(np.asarray(listed, dtype=bool), np.shape(p)).copy()
    if threshold is not None:
        def T(v):
            return wrap(threshold + ((v * slope) >> 8))
        up, down = wrap(mx + T(p if variant == 'slope_p' else mx)), wrap(p + T(p if variant == 'slope_p' else mn))
        assert max(int(np.max(up)), int(np.max(down))) <= U32
        bad |= (p >= up) if variant == 'ge' else (p > up)
        if variant != 'hotonly':
            bad |= (down <= mn) if variant == 'ge' else (down < mn)
    best, fix = None, None
    for a, b in pairs:
        d = np.abs(a - b)
        m = wrap(a + b + (0 if variant == 'trunc' else 1)) >> 1
        if best is None:
            best, fix = d, m
        else:
            take = (d <= best) if variant == 'lasttie' else (d < best)
            best, fix = np.where(take, d, best), np.where(take, m, fix)
    return np.where(bad, fix, p)


def dpc_ref(frames, threshold, slope, bitmap, variant=None):
    """(..,H,W) integer samples 0 .. 65535 -> (..,H,W) uint16 corrected samples.  ``threshold`` None: no dynamic test; ``bitmap``
    None: no map.  ``variant`` names one of the wrong forms (``VARIANTS``) a test tells apart from the definition: 'clamp' (the edge
    replicated), 'dist1' (neighbours at distance 1), 'vfirst' (V before H), 'afirst' (A before D), 'lasttie' (the last pair wins a
    tie), 'trunc' (no + 1), 'ge' (>= and <=), 'slope_p' (the slope on p), 'hotonly' (no dead test), 'wrap16' (sums held in uint16),
    'recursive' (neighbours taken from already-corrected pixels in raster order)"""
    assert variant is None or variant in VARIANTS, variant
    s = np.asarray(frames).astype(np.int64)
    assert s.min() >= 0 and s.max() <= 65535
    h, w = s.shape[-2:]
    assert h >= 3 and w >= 4 and w % 4 == 0, (h, w)
    assert threshold is None or (0 <= threshold <= 65535 and 0 <= slope <= 255)
    assert threshold is not None or bitmap is not None
    listed = listed_ref(bitmap, h, w)
    if variant == 'recursive':
        return _recursive(s, threshold, slope, listed)
    r = 1 if variant == 'dist1' else 2
    pad = np.pad(s, [(0, 0)] * (s.ndim - 2) + [(2, 2), (2, 2)], mode='edge' if variant == 'clamp' else 'reflect')

    def at(dy, dx):
        return pad[..., 2 + dy:2 + dy + h, 2 + dx:2 + dx + w]

    pairs = [(at(0, -r), at(0, r)), (at(-r, 0), at(r, 0)), (at(-r, -r), at(r, r)), (at(-r, r), at(r, -r))]
    return _decide(s, pairs, listed, threshold, slope, variant).astype(np.uint16)


def _recursive(s, threshold, slope, listed):
    """the in-place form: a pixel's neighbours are read from the frame being corrected, in raster order"""
    h, w = s.shape[-2:]
    out = s.reshape((-1, h, w)).copy()

    def ry(i):
        return -i if i < 0 else (2 * (h - 1) - i if i >= h else i)

    def rx(i):
        return -i if i < 0 else (2 * (w - 1) - i if i >= w else i)

    for f in out:
        for y in range(h):
            for x in range(w):
                g = lambda dy, dx: f[ry(y + dy), rx(x + dx)]
                pairs = [(g(0, -2), g(0, 2)), (g(-2, 0), g(2, 0)), (g(-2, -2), g(2, 2)), (g(-2, 2), g(2, -2))]
                f[y, x] = _decide(f[y, x], pairs, listed[y, x], threshold, slope, None)
    return out.reshape(s.shape).astype(np.uint16)


# ---------------------------------------------------------------- the input sets of tests/test_gpu_serve_defect.py
SHAPES = [(3, 4), (4, 4), (4, 8), (6, 12), (3, 20), (34, 68)]
LAUNCH_SHAPES = SHAPES + [(37, 132)]        # the launch walks 8 rows per thread: 37 % 8 != 0, and 33 column groups are no multiple of a wave's lanes
PARAMS = [(0, 0), (1, 0), (16, 32), (0, 255), (65535, 255)]
KINDS = ('full', 'ten', 'low')


def frames(kind, n, h, w, seed):
    """'full': full-range 16-bit with 65535 and 0 planted; 'ten': 10-bit; 'low': codes 0 .. 7"""
    rng = np.random.default_rng(seed)
    if kind == 'full':
        f = rng.integers(0, 65536, (n, h, w))
        f[0, 0, 0], f[0, -1, -1], f[-1, 1, 1], f[-1, h // 2, w // 2] = 65535, 0, 0, 65535
    elif kind == 'ten':
        f = rng.integers(0, 1024, (n, h, w))
    else:
        assert kind == 'low'
        f = rng.integers(0, 8, (n, h, w))
    return f.astype(np.uint16)


def random_bitmap(h, w, seed):
    """a map with about 5 % of its bits set, (0,0), (H-1,W-1) and x = 31 / 32 of every other row among them; the bits behind W
    of the last word are all set: they are ignored"""
    rng = np.random.default_rng(seed)
    ys, xs = np.nonzero(rng.random((h, w)) < 0.05)
    coords = list(zip(ys.tolist(), xs.tolist())) + [(0, 0), (h - 1, w - 1)]
    coords += [(y, x) for y in range(0, h, 2) for x in (31, 32) if x < w]
    m = map_ref(coords, h, w).view(np.uint32).copy()
    if w % 32:
        m[:, -1] |= np.uint32((U32 << (w % 32)) & U32)
    return m.view(np.int32)


def frame_set(kind, h, w, n=3):
    """the frames of ``kind`` every test uses at (h, w): one seed per kind and shape"""
    return frames(kind, n, h, w, seed=1000 * h + 10 * w + KINDS.index(kind))
