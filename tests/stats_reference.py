"""The 3A statistics of the sensor frame restated in numpy int64 - the definition of include/risp.h, independent of the kernel.

s(y,x) = max(S(y,x) - black_level, 0); the plane of a pixel is c = 2 * (y & 1) + (x & 1); pixel (y,x) lies in zone
(y // zone_h, x // zone_w), ZH = ceil(H / zone_h), ZW = ceil(W / zone_w).  Per image, zone and plane: ``count`` the samples with
lo <= s <= hi, ``sum`` their sum, ``sharp`` the sum of |2 s(y,x) - s(y,x-2) - s(y,x+2)| over the pixels with 2 <= x < W - 2,
whatever lo and hi are.  Per image and plane: hist[min(s >> hist_shift, bins - 1)] += 1 over every sample.

``VARIANTS`` are plausible mistakes.  ``LAUNCH_CASES``, ``EXTREME_CASES`` and ``case_frames`` are the inputs of
tests/test_gpu_serve_stats.py; tests/test_stats_reference_cpu.py shows that they tell every variant from the definition."""
import numpy as np

VARIANTS = ('hi_exclusive', 'lo_ignored', 'plane_swapped', 'no_clamp', 'zone_floor', 'reflect', 'focus_range', 'hist_drop',
            'wrap32', 'dist1')
U32 = (1 << 32) - 1


def grid(h, w, zone):
    """(ZH, ZW)"""
    return -(-h // zone[0]), -(-w // zone[1])


def stats_ref(frames, black_level, zone, bins, hist_shift, lo, hi, variant=None):
    """(N,H,W) or (H,W) samples -> (zones (N,ZH,ZW,4,3) int64 [sum, count, sharp], hist (N,4,bins) int32).  ``variant``: None for
    the definition, or a name of ``VARIANTS`` for that mistake."""
    assert variant is None or variant in VARIANTS, variant
    x = np.asarray(frames).astype(np.int64)
    if x.ndim == 2:
        x = x[None]
    n, h, w = x.shape
    zone_h, zone_w = zone
    gh, gw = grid(h, w, zone)
    s = x - int(black_level)
    # (no_clamp: the subtraction as unsigned 32-bit arithmetic does it)
    s = (s & U32) if variant == 'no_clamp' else np.maximum(s, 0)
    yy, xx = np.mgrid[0:h, 0:w]
    plane = 2 * (xx & 1) + (yy & 1) if variant == 'plane_swapped' else 2 * (yy & 1) + (xx & 1)
    if variant == 'zone_floor':
        zy, zx = np.minimum(yy // max(h // gh, 1), gh - 1), np.minimum(xx // max(w // gw, 1), gw - 1)
    else:
        zy, zx = yy // zone_h, xx // zone_w
    key = ((zy * gw + zx) * 4 + plane).ravel()
    inside = s < hi if variant == 'hi_exclusive' else s <= hi
    if variant != 'lo_ignored':
        inside &= s >= lo
    d = 1 if variant == 'dist1' else 2
    focus = np.zeros_like(s)
    if variant == 'reflect':
        p = np.pad(s, ((0, 0), (0, 0), (d, d)), mode='reflect')
        focus = np.abs(2 * s - p[:, :, :w] - p[:, :, 2 * d:])
    elif w > 2 * d:
        focus[:, :, d:w - d] = np.abs(2 * s[:, :, d:w - d] - s[:, :, :w - 2 * d] - s[:, :, 2 * d:])
    if variant == 'focus_range':
        focus = focus * inside
    zones = np.zeros((n, gh * gw * 4, 3), dtype=np.int64)
    hist = np.zeros((n, 4 * bins), dtype=np.int64)
    b = s >> hist_shift

    def total(keys, values, size):
        # bincount adds in float64: exact, since every partial sum is an integer below 2^53
        assert float(values.max(initial=0)) * values.size < 2.0 ** 53
        return np.bincount(keys, weights=values.astype(np.float64), minlength=size).astype(np.int64)

    for k in range(n):
        zones[k, :, 0] = total(key, (s[k] * inside[k]).ravel(), gh * gw * 4)
        zones[k, :, 1] = total(key, inside[k].ravel().astype(np.int64), gh * gw * 4)
        zones[k, :, 2] = total(key, focus[k].ravel(), gh * gw * 4)
        keep = (b[k] < bins).ravel() if variant == 'hist_drop' else np.ones(h * w, dtype=bool)
        hist[k] = np.bincount((plane.ravel() * bins + np.minimum(b[k], bins - 1).ravel())[keep], minlength=4 * bins)
    hist = hist.reshape(n, 4, bins)
    if variant == 'wrap32':
        zones[:, :, 0] &= U32
        zones[:, :, 2] &= U32
    assert hist.max() < 1 << 31
    return zones.reshape(n, gh, gw, 4, 3), hist.astype(np.int32)


# ---- the inputs of the GPU test: (frames shape, zone, bins, hist_shift, lo, hi, black level, bits of the data)
# (1,2,4): one quad, no focus term; (2,6,12): partial zones on both axes, 6 // 2 != 4; (1,38,52): 247 zones, many per workgroup;
# (3,130,260): more than a workgroup's tile of 256 columns x 16 rows on both axes, and zone borders every 6 rows and 20 columns
# fall on no tile border but the first.  bins 1, 16 and 1024, hist_shift 0 and 6, black levels above some samples, lo and hi
# inside the data's range
LAUNCH_CASES = [
    ((1, 2, 4), (2, 4), 16, 6, 0, 65535, 0, 10),
    ((1, 2, 4), (2, 4), 1, 0, 200, 800, 64, 10),
    ((2, 6, 12), (4, 8), 1, 0, 64, 900, 64, 10),
    ((2, 6, 12), (4, 8), 16, 6, 16, 60000, 300, 16),
    ((1, 38, 52), (2, 4), 1024, 0, 100, 1000, 100, 12),
    ((1, 38, 52), (2, 4), 16, 6, 0, 65535, 0, 10),
    ((3, 130, 260), (6, 20), 16, 6, 70, 1000, 64, 12),
    ((3, 130, 260), (6, 20), 1024, 0, 5, 700, 0, 10),
    ((3, 130, 260), (6, 20), 16, 6, 1000, 50000, 4096, 16),
    ((3, 130, 260), (128, 256), 256, 2, 0, 65535, 64, 10),
]
# the extremes: one zone over (1,512,1024); all 65535 - every plane's sum is 131072 * 65535 = 2^33 - 2^17, twice what 32 bits hold -, and columns x % 4 < 2 at
# 65535 beside zeros - every pixel's focus term is 131070, the bound the kernel's 32-bit partials rest on
EXTREME_SHAPE, EXTREME_ZONE = (1, 512, 1024), (512, 1024)
EXTREME_CASES = ['full', 'stripes']


def case_frames(shape, bits, seed):
    """samples uniform in 0 .. 2^bits - 1, the extremes present"""
    f = np.random.default_rng(seed).integers(0, 1 << bits, shape).astype(np.uint16)
    f[0, 0, 0], f[0, -1, -1] = (1 << bits) - 1, 0
    return f


def extreme_frames(kind):
    f = np.full(EXTREME_SHAPE, 65535, dtype=np.uint16)
    if kind == 'stripes':
        f[:, :, (np.arange(EXTREME_SHAPE[2]) % 4) >= 2] = 0
    return f
