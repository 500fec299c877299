"""The scaled, cropped output of the serving path, restated in numpy - the yardstick of tests/test_gpu_serve_resize.py.

Written from the definition in include/risp.h, not from the product.  One axis: a source window of S samples at offset o of the
image is resampled to D samples.  In float64, with the kernel f of radius r (box 0.5, triangle 1, bicubic 2):

    scale = S / D, fs = max(scale, 1), support = r * fs;  for output i:  c = (i + 0.5) * scale
    lo = max(int(c - support + 0.5), 0), hi = min(int(c + support + 0.5), S)
    w_k = f((k + lo - c + 0.5) / fs), k < hi - lo;  s = their sum from left to right
    q_k = floor(w_k / s * 16384 + 0.5); 16384 - sum(q) goes to the largest q_k (the first on a tie)
    zero taps at both ends are trimmed; T is the longest row; start_i = min(lo_i, S - T); the row stands at column
    lo_i - start_i of T zeros; then start_i += o

    h(y,j,c)   = clamp((sum_k wx[j][k] * img(y, xs[j]+k, c) + 8192) >> 14, 0, 255)
    out(i,j,c) = clamp((sum_k wy[i][k] * h(ys[i]+k, j, c)   + 8192) >> 14, 0, 255)

``variant`` switches one deliberate mistake on, for the tests that show each of them would be seen:
    'vertical_first'  the vertical pass runs first
    'truncate'        no + 8192
    'no_clamp'        the low byte of the shifted sum is kept instead of the clamp
    'no_mid_round'    no code between the passes: one sum of products, + 2^27, >> 28
    'no_renorm'       the residue is not added: rows do not sum to 16384
    'window_image'    taps reach past the window into the image: lo and hi clamp to the image, not to the window
"""
import numpy as np

KERNELS = ('box', 'triangle', 'bicubic')
RADIUS = {'box': 0.5, 'triangle': 1.0, 'bicubic': 2.0}
VARIANTS = ('vertical_first', 'truncate', 'no_clamp', 'no_mid_round', 'no_renorm', 'window_image')


def kernel_values(kernel, x):
    """f on a float64 array"""
    x = np.asarray(x, dtype=np.float64)
    if kernel == 'box':
        return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)
    t = np.abs(x)
    if kernel == 'triangle':
        return np.where(t < 1.0, 1.0 - t, 0.0)
    assert kernel == 'bicubic'
    a = -0.5
    inner = ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    outer = (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return np.where(t < 1.0, inner, np.where(t < 2.0, outer, 0.0))


def taps(S, D, kernel, offset=0, variant=None, image=None):
    """-> (start (D,) int64, weight (D,T) int64).  ``image``: the image's length along the axis, read by 'window_image' only"""
    assert kernel in KERNELS and S >= 1 and D >= 1 and offset >= 0
    left, right = 0, S                                      # where taps may lie, in window coordinates
    if variant == 'window_image':
        left, right = -offset, image - offset
    scale = np.float64(S) / np.float64(D)
    fs = max(scale, np.float64(1.0))
    support = np.float64(RADIUS[kernel]) * fs
    los, rows = [], []
    for i in range(D):
        c = (np.float64(i) + 0.5) * scale
        lo, hi = max(int(c - support + 0.5), left), min(int(c + support + 0.5), right)
        w = kernel_values(kernel, (np.arange(hi - lo, dtype=np.float64) + lo - c + 0.5) / fs)
        s = np.cumsum(w)[-1]                                # cumsum adds from left to right
        q = np.floor(w / s * 16384 + 0.5).astype(np.int64)
        if variant != 'no_renorm':
            q[int(np.argmax(q))] += 16384 - q.sum()         # argmax is the first maximum
        nz = np.nonzero(q)[0]
        los.append(lo + int(nz[0]))
        rows.append(q[nz[0]:nz[-1] + 1])
    T = max(len(q) for q in rows)
    start, weight = np.zeros(D, dtype=np.int64), np.zeros((D, T), dtype=np.int64)
    for i, (lo, q) in enumerate(zip(los, rows)):
        at = min(lo, right - T)
        weight[i, lo - at:lo - at + len(q)] = q
        start[i] = at + offset
    return start, weight


def longest_window(S, D, kernel):
    """the largest hi - lo of any output, before quantisation and trimming: what the product's 32-sample limit is judged on"""
    scale = np.float64(S) / np.float64(D)
    support = np.float64(RADIUS[kernel]) * max(scale, np.float64(1.0))
    c = (np.arange(D, dtype=np.float64) + 0.5) * scale
    lo = np.maximum(np.trunc(c - support + 0.5), 0)
    hi = np.minimum(np.trunc(c + support + 0.5), S)
    return int((hi - lo).max())


def _sums(src, start, weight, axis):
    """(N,H,W,3) int64 -> the sums of products along ``axis`` (1 rows, 2 columns)"""
    idx = start[:, None] + np.arange(weight.shape[1])[None, :]          # (D,T)
    if axis == 2:
        return (src[:, :, idx, :] * weight[None, None, :, :, None]).sum(axis=3)
    return (src[:, idx, :, :] * weight[None, :, :, None, None]).sum(axis=2)


def _code(s, variant, shift=14):
    v = (s + (0 if variant == 'truncate' else 1 << (shift - 1))) >> shift
    return v & 255 if variant == 'no_clamp' else np.clip(v, 0, 255)


def resize(img, out_size=None, out_window=None, kernel='triangle', variant=None):
    """(N,H,W,3) uint8 -> (N,OH,OW,3) uint8: the window (y0, x0, h, w) of every image (default: all of it) to out_size
    (default: the window's size)"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 4 and img.shape[3] == 3
    H, W = img.shape[1:3]
    y0, x0, wh, ww = (0, 0, H, W) if out_window is None else out_window
    assert 0 <= y0 and 0 <= x0 and wh >= 1 and ww >= 1 and y0 + wh <= H and x0 + ww <= W
    oh, ow = (wh, ww) if out_size is None else out_size
    xs, wx = taps(ww, ow, kernel, x0, variant, W)
    ys, wy = taps(wh, oh, kernel, y0, variant, H)
    v = img.astype(np.int64)
    if variant == 'no_mid_round':
        return _code(_sums(_sums(v, xs, wx, 2), ys, wy, 1), variant, 28).astype(np.uint8)
    order = ((ys, wy, 1), (xs, wx, 2)) if variant == 'vertical_first' else ((xs, wx, 2), (ys, wy, 1))
    for start, weight, axis in order:
        v = _code(_sums(v, start, weight, axis), variant)
    return v.astype(np.uint8)


def resize_nv12(img, out_size, out_window, kernel, coef, channels='bgr'):
    """the NV12 form: tests/nv12_reference.py on the resized codes"""
    import nv12_reference as NR
    return NR.nv12(resize(img, out_size, out_window, kernel), coef, channels)


# the kernel cases of tests/test_gpu_serve_resize.py: (image shape (N,H,W), out_size, out_window)
CASES = (
    ((2, 24, 40), (10, 18), None),
    ((1, 12, 16), (30, 46), None),
    ((1, 30, 44), (8, 12), None),
    ((2, 24, 40), (24, 40), None),                  # equals the input
    ((1, 64, 64), (8, 8), None),                    # bicubic at the 32-tap limit
    ((1, 16, 20), (2, 2), None),
    ((1, 37, 31), (19, 1), None),
    ((1, 5, 3), (1, 7), None),
    ((2, 24, 40), (10, 18), (3, 5, 17, 29)),
    ((2, 24, 40), None, (3, 5, 17, 29)),            # the same window alone: a crop
)
# 53 -> 1 needs 53 taps with every kernel: refused, not served
REFUSED_CASE = ((1, 37, 53), (19, 1), None)


def make_image(n, h, w, seed):
    """random bytes with one quadrant of 0 / 255 noise, so that bicubic overshoots: the inputs of the GPU tests"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    img[:, :(h + 1) // 2, :(w + 1) // 2] = rng.integers(0, 2, size=(n, (h + 1) // 2, (w + 1) // 2, 3), dtype=np.uint8) * 255
    return img
