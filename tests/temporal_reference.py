"""Temporal noise reduction restated in numpy int64 - the definition of include/risp.h, independent of the kernel.

c is the current frame, p the state (the previous filtered frame).  The window is the full 5 x 5 around (y,x); an index outside the
frame reflects without repeating the edge.

    A  = sum over the window of (c - p)
    B  = sum over the window of p
    Bs = max(B - 25 * black_level, 0)
    lo = 25 * threshold + ((Bs * slope) >> 8)
    e  = min(max(|A| - lo, 0), 65535)
    k  = min(strength + ((e * ramp) >> 8), 256)
    out = (p * (256 - k) + c * k + 128) >> 8

The new state is out; a state that was never filled is primed: out = c, state = c.  Every intermediate is asserted to fit unsigned
32 bits, which is what the definition promises."""
import numpy as np

U32 = (1 << 32) - 1
VARIANTS = ('clamp', 'win3', 'nopedestal', 'shiftfirst', 'noround', 'frozen', 'inplace')


def _window_sum(v, radius, mode):
    """the sum of v (..,H,W) int64 over the (2 radius + 1)^2 window around every pixel"""
    h, w = v.shape[-2:]
    pad = np.pad(v, [(0, 0)] * (v.ndim - 2) + [(radius, radius)] * 2, mode=mode)
    total = np.zeros_like(v)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            total += pad[..., dy:dy + h, dx:dx + w]
    return total


def gain_ref(A, B, strength, threshold, slope, ramp, black_level, variant=None):
    """k, the Q8 share of the new frame, from the window sums (int64, any shape)"""
    bs = B if variant == 'nopedestal' else np.maximum(B - 25 * black_level, 0)
    assert int(np.max(bs * slope)) <= U32
    lo = 25 * threshold + ((bs * slope) >> 8)
    excess = np.maximum(np.abs(A) - lo, 0)
    if variant == 'shiftfirst':
        step = np.minimum((excess * ramp) >> 8, 65535)
    else:
        e = np.minimum(excess, 65535)
        assert int(np.max(e * ramp)) <= U32
        step = (e * ramp) >> 8
    return np.minimum(strength + step, 256)


def blend_ref(c, p, k, variant=None):
    total = p * (256 - k) + c * k + (0 if variant == 'noround' else 128)
    assert int(np.max(total)) <= (1 << 24) + 128
    return total >> 8


def _check(c, p, strength, threshold, slope, ramp, black_level):
    assert c.shape == p.shape and min(c.min(), p.min()) >= 0 and max(c.max(), p.max()) <= 65535
    h, w = c.shape[-2:]
    assert h >= 3 and w >= 4 and w % 4 == 0, (h, w)
    assert 0 <= strength <= 256 and 0 <= threshold <= 65535 and 0 <= slope <= 255 and 0 <= ramp <= 65535
    assert 0 <= black_level <= 65535


def gains(cur, state, strength, threshold, slope, ramp, black_level=0):
    """the (..,H,W) int64 plane of k the definition takes for ``cur`` over ``state``"""
    c, p = np.asarray(cur).astype(np.int64), np.asarray(state).astype(np.int64)
    _check(c, p, strength, threshold, slope, ramp, black_level)
    return gain_ref(_window_sum(c - p, 2, 'reflect'), _window_sum(p, 2, 'reflect'), strength, threshold, slope, ramp, black_level)


def tnr_ref(cur, state, strength, threshold, slope, ramp, black_level=0, variant=None):
    """one step: (..,H,W) integer samples ``cur`` over the state ``state`` -> (..,H,W) uint16, the filtered frame and new state.
    ``variant`` names one of the wrong forms of a step (``VARIANTS`` but 'frozen', which is a fault of the sequence): 'clamp' (the
    edge replicated), 'win3' (a 3 x 3 window), 'nopedestal' (Bs = B), 'shiftfirst' (the excess times ramp >> 8, clamped behind the
    shift), 'noround' (no + 128), 'inplace' (the state updated in place in raster order: a pixel's window reads state values this
    step wrote)"""
    assert variant is None or (variant in VARIANTS and variant != 'frozen'), variant
    c, p = np.asarray(cur).astype(np.int64), np.asarray(state).astype(np.int64)
    _check(c, p, strength, threshold, slope, ramp, black_level)
    if variant == 'inplace':
        return _inplace(c, p, strength, threshold, slope, ramp, black_level)
    radius, mode = (1 if variant == 'win3' else 2), ('edge' if variant == 'clamp' else 'reflect')
    A, B = _window_sum(c - p, radius, mode), _window_sum(p, radius, mode)
    assert int(np.max(np.abs(A))) <= 25 * 65535
    k = gain_ref(A, B, strength, threshold, slope, ramp, black_level, variant)
    return blend_ref(c, p, k, variant).astype(np.uint16)


def _inplace(c, p, strength, threshold, slope, ramp, black_level):
    h, w = c.shape[-2:]
    cs, ps = c.reshape((-1, h, w)), p.reshape((-1, h, w)).copy()
    ry = [(-i if i < 0 else (2 * (h - 1) - i if i >= h else i)) for i in range(-2, h + 2)]
    rx = [(-i if i < 0 else (2 * (w - 1) - i if i >= w else i)) for i in range(-2, w + 2)]
    for cf, pf in zip(cs, ps):
        for y in range(h):
            rows = ry[y:y + 5]
            for x in range(w):
                win_p = pf[np.ix_(rows, rx[x:x + 5])]
                win_c = cf[np.ix_(rows, rx[x:x + 5])]
                k = gain_ref((win_c - win_p).sum(), win_p.sum(), strength, threshold, slope, ramp, black_level)
                pf[y, x] = blend_ref(cf[y, x], pf[y, x], k)
    return ps.reshape(c.shape).astype(np.uint16)


def run_ref(sequence, strength, threshold, slope, ramp, black_level=0, variant=None, state=None):
    """the recursion over ``sequence`` (frames of one shape): ([the filtered frames], the state behind the last).  Without a
    ``state`` the first frame primes: it is returned as it is and becomes the state.  'frozen': the state is never advanced
    behind the priming"""
    outs = []
    for frame in sequence:
        if state is None:
            out = state = np.asarray(frame).astype(np.uint16)
        else:
            out = tnr_ref(frame, state, strength, threshold, slope, ramp, black_level, None if variant == 'frozen' else variant)
            if variant != 'frozen':
                state = out
        outs.append(out)
    return outs, state


# ---------------------------------------------------------------- the inputs of tests/test_gpu_temporal.py
# (1,3,4): the smallest legal frame, every neighbour a reflection; (3,37,260): 37 rows are no multiple of the 8 a thread walks and
# 65 column groups pass a wave; (1,16,1028): 257 column groups pass a workgroup of 256 threads
SHAPES = [(1, 3, 4), (2, 6, 8), (3, 37, 260), (1, 16, 1028)]
# (strength, threshold, slope, ramp): on independent uniform 10-bit frames each puts a good part of the pixels into each regime -
# k == strength, strictly between, k == 256 (tests/test_temporal_reference_cpu.py holds the inputs to that)
PARAMS = [(64, 40, 0, 24), (64, 20, 10, 24)]
BLACK = 64
STEPS = 5               # the priming frame and four behind it


def sequence(shape, seed=None, steps=STEPS):
    """``steps`` independent uniform 10-bit frame stacks of ``shape``: one seed per shape"""
    n, h, w = shape
    rng = np.random.default_rng(7000 + 100 * h + w if seed is None else seed)
    return [rng.integers(0, 1024, (n, h, w)).astype(np.uint16) for _ in range(steps)]


# the unsigned extremes: (cur value, state value, (strength, threshold, slope, ramp), black_level, the k and the result of every pixel)
EXTREMES = [
    (65535, 0, (0, 0, 255, 65535), 0, 256, 65535),          # Bs = 0, e clamps at 65535, e * ramp = 65535^2
    (0, 65535, (0, 0, 255, 65535), 0, 256, 0),              # Bs * slope = 25 * 65535 * 255: lo = 1631975, e = 6400
    (65535, 65535, (77, 0, 255, 65535), 0, 77, 65535),      # A = 0: the blend of equals, 65535 * 256 + 128 below 2^24 + 128
    (65535, 0, (0, 0, 0, 1), 0, 255, 65279),                # e = min(25 * 65535, 65535), (65535 * 1) >> 8 = 255; 65535 * 255 + 128 >> 8
    (65535, 0, (3, 65535, 0, 65535), 0, 3, 768),            # lo = 25 * 65535 = |A|: e = 0, k = strength; (65535 * 3 + 128) >> 8
    (0, 65535, (0, 0, 255, 65535), 65535, 256, 0),          # the pedestal takes all of B: Bs = 0
]
