"""The mesh warp of the serving path restated in numpy int64 (include/risp.h has the definition): the per-pixel Q8 coordinate
interpolated from the mesh, the replicate border, the bilinear and the Q11 Catmull-Rom taps.  Nothing here imports the product.

``CASES`` is shared by the CPU and the GPU tests; ``WRONG`` holds deliberate mistakes, each of which must change at least one
byte on ``CASES``; ``HARMLESS`` holds two mistakes that provably cannot change a byte (they are kept to say so):
  * truncation toward zero instead of floor at the per-pixel shift: the two differ for negative values only, both results are
    then <= 0, and the clamp to 0 follows.  The mistake that DOES show is the same truncation where a mesh is quantised (a
    negative node enters the interpolation unclamped), so ``WRONG['truncation']`` makes it there.
  * ``x1 = x0 + 1`` without the clamp: x0 = W-1 only for the clamped coordinate (W-1) << 8, whose phase is 0, so the tap past
    the image has weight 0 - the clamp keeps the READ inside the image, it does not change the value.  Here the tap past the
    edge reads a guard byte.
"""
import numpy as np

KERNELS = ('bilinear', 'bicubic')


def cubic_table(fixup=True):
    """(256,4) int64: Q11 Catmull-Rom rows from the integer formula, each summing to 2048 (with the fix-up)"""
    f = np.arange(256, dtype=np.int64)
    n = np.stack([-f ** 3 + 512 * f ** 2 - 65536 * f, 3 * f ** 3 - 1280 * f ** 2 + (1 << 25),
                  -3 * f ** 3 + 1024 * f ** 2 + 65536 * f, f ** 3 - 256 * f ** 2], axis=1)
    assert (n.sum(axis=1) == 1 << 25).all() and (np.abs(n) < 1 << 31).all()
    q = (n + 8192) >> 14
    if fixup:
        for row in q:
            row[int(np.argmax(row))] += 2048 - row.sum()          # argmax: the first index of the largest
    return q


def coords(mesh, k, size, H, W, rounding=True, clamp_first=False, swap=False, truncate=False, clamp=True):
    """the per-pixel Q8 coordinates (uy, ux), each (WH,WW) int64, of a (MH,MW,2) int32 mesh with cells of 1 << k"""
    wh, ww = size
    m = np.asarray(mesh).astype(np.int64)
    assert m.shape == (((wh - 1) >> k) + 2, ((ww - 1) >> k) + 2, 2), m.shape
    cell = 1 << k
    y, x = np.arange(wh, dtype=np.int64)[:, None], np.arange(ww, dtype=np.int64)[None, :]
    i, fy, j, fx = y >> k, y & (cell - 1), x >> k, x & (cell - 1)
    out = []
    for c, S in ((0, H), (1, W)):
        hi = (S - 1) << 8
        node = m[..., 1 - c if swap else c]
        if clamp_first:
            node = np.clip(node, 0, hi)
        top = (cell - fx) * node[i, j] + fx * node[i, j + 1]
        bot = (cell - fx) * node[i + 1, j] + fx * node[i + 1, j + 1]
        v = (cell - fy) * top + fy * bot + ((1 << (2 * k - 1)) if rounding else 0)
        assert (np.abs(v) < 1 << 48).all()
        u = np.where(v < 0, -((-v) >> (2 * k)), v >> (2 * k)) if truncate else v >> (2 * k)
        out.append(np.clip(u, 0, hi) if clamp else u)
    return out[0], out[1]


def _bilinear(p, uy, ux, x1_clamped=True):
    H, W = p.shape[1:3]
    y0, ty, x0, tx = uy >> 8, (uy & 255)[None, ..., None], ux >> 8, (ux & 255)[None, ..., None]
    y1 = np.minimum(y0 + 1, H - 1)
    if x1_clamped:
        x1 = np.minimum(x0 + 1, W - 1)
    else:
        p = np.concatenate([p, np.full(p.shape[:2] + (1, 3), 0xA5, dtype=p.dtype)], axis=2)     # the byte behind the row
        x1 = x0 + 1
    top = (256 - tx) * p[:, y0, x0] + tx * p[:, y0, x1]
    bot = (256 - tx) * p[:, y1, x0] + tx * p[:, y1, x1]
    v = (256 - ty) * top + ty * bot + 32768
    assert (v < 1 << 24).all()
    return v >> 16


def _bicubic(p, uy, ux, fixup=True, round_between=False, pair_clamp=False):
    H, W = p.shape[1:3]
    q = cubic_table(fixup)
    y0, ty, x0, tx = uy >> 8, uy & 255, ux >> 8, ux & 255
    if pair_clamp and H >= 4:
        y0 = np.clip(y0, 1, H - 3)
    if pair_clamp and W >= 4:
        x0 = np.clip(x0, 1, W - 3)
    v = 0
    for r in range(4):
        yy = np.clip(y0 - 1 + r, 0, H - 1)
        h = 0
        for c in range(4):
            h = h + q[tx, c][None, ..., None] * p[:, yy, np.clip(x0 - 1 + c, 0, W - 1)]
        if round_between:
            h = np.clip((h + 1024) >> 11, 0, 255)
        v = v + q[ty, r][None, ..., None] * h
    if round_between:
        return np.clip((v + 1024) >> 11, 0, 255)
    assert (np.abs(v) + (1 << 21) < 1 << 31).all()
    return np.clip((v + (1 << 21)) >> 22, 0, 255)


def warp(img, mesh, k, size, kernel, **wrong):
    """(N,H,W,3) or (H,W,3) uint8 -> (N,WH,WW,3) or (WH,WW,3) uint8; ``wrong``: the switches of ``coords`` and of the taps"""
    img = np.asarray(img)
    single = img.ndim == 3
    p = (img[None] if single else img).astype(np.int64)
    assert p.ndim == 4 and p.shape[3] == 3 and kernel in KERNELS
    ck = {n: wrong.pop(n) for n in ('rounding', 'clamp_first', 'swap', 'truncate') if n in wrong}
    H, W = p.shape[1:3]
    uy, ux = coords(mesh, k, size, H, W, **ck)
    if ck.get('swap'):                                        # (a swapped pair is clamped with the swapped sizes: back into the image)
        uy, ux = np.clip(uy, 0, (H - 1) << 8), np.clip(ux, 0, (W - 1) << 8)
    out = _bilinear(p, uy, ux, **wrong) if kernel == 'bilinear' else _bicubic(p, uy, ux, **wrong)
    assert out.min() >= 0 and out.max() <= 255
    out = np.ascontiguousarray(out.astype(np.uint8))          # (indexing with arrays leaves another memory order behind)
    return out[0] if single else out


# ---------------------------------------------------------------- inputs
def quantise(v, truncate=False):
    """float64 source coordinates -> Q8 int32 nodes: floor(v * 256 + 0.5), saturated (``truncate``: toward zero, the mistake)"""
    q = v * 256.0 + 0.5
    q = np.trunc(q) if truncate else np.floor(q)
    return np.clip(q, -2147483648.0, 2147483647.0).astype(np.int64).astype(np.int32)


def make_mesh(kind, hw, size, k, seed=0, truncate=False):
    """a (MH,MW,2) int32 mesh of one of the kinds below for H x W images and a WH x WW output with cells of 1 << k"""
    (H, W), (wh, ww) = hw, size
    mh, mw = ((wh - 1) >> k) + 2, ((ww - 1) >> k) + 2
    y = (np.arange(mh, dtype=np.float64) * (1 << k))[:, None] + np.zeros((1, mw))
    x = (np.arange(mw, dtype=np.float64) * (1 << k))[None, :] + np.zeros((mh, 1))
    ky, kx = (H - 1) / max(wh - 1, 1), (W - 1) / max(ww - 1, 1)
    rng = np.random.default_rng(seed)
    if kind == 'identity':
        sy, sx = y, x
    elif kind == 'flip':
        sy, sx = H - 1 - y, W - 1 - x
    elif kind == 'transpose':
        sy, sx = x, y
    elif kind == 'smooth':                                    # the frames mapped onto each other, perturbed by a few pixels
        sy = y * ky + 1.7 * np.sin(x / 9.0 + 0.3) + rng.uniform(-0.5, 0.5, y.shape)
        sx = x * kx + 2.3 * np.cos(y / 7.0) + rng.uniform(-0.5, 0.5, y.shape)
    elif kind == 'rot_radial':                                # 3 degrees about the middle, then a barrel term
        cy, cx, a = (H - 1) / 2.0, (W - 1) / 2.0, np.deg2rad(3.0)
        dy, dx = y * ky - cy, x * kx - cx
        ry, rx = np.cos(a) * dy + np.sin(a) * dx, -np.sin(a) * dy + np.cos(a) * dx
        s = 1.0 + 0.12 * (ry * ry + rx * rx) / (cy * cy + cx * cx)
        sy, sx = cy + ry * s, cx + rx * s
    elif kind == 'reduce8':
        sy, sx = y * 8.0, x * 8.0
    elif kind == 'half':                                      # left half identity, right half 8:1: the node columns from 40 on
        sy, sx = np.where(x < 40, y, y * 8.0), np.where(x < 40, x, x * 8.0)
    elif kind == 'int32':                                     # uniform over all of int32: every mesh is a defined input
        return rng.integers(-2 ** 31, 2 ** 31, size=(mh, mw, 2), dtype=np.int64).astype(np.int32)
    elif kind == 'outside':                                   # the output spans the image and 20 pixels beyond it on every side
        sy, sx = -20.0 + y * (H - 1 + 40.0) / max(wh - 1, 1), -20.0 + x * (W - 1 + 40.0) / max(ww - 1, 1)
        sy, sx = sy + 0.37 * np.sin(x / 5.0), sx + 0.41 * np.cos(y / 4.0)
    elif kind == 'affine':                                    # a small rotation with a shift: the 2 x 2 node case
        sy, sx = 3.25 + 0.98 * y + 0.03 * x, -2.5 - 0.03 * y + 0.985 * x
    elif kind == 'point':
        sy, sx = 3.3 + 0.0 * y, 4.7 + 0.0 * x
    else:
        raise ValueError(kind)
    return quantise(np.stack([sy, sx], axis=-1), truncate)


def make_image(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


# (source (N,H,W), output (WH,WW), cell_log2, mesh kind): the smallest shapes at which the launch can go wrong
CASES = [
    ((2, 37, 53), (19, 45), 2, 'smooth'),          # one ragged tile; rows of 159 bytes: every row starts at another alignment
    ((2, 100, 300), (58, 214), 4, 'rot_radial'),   # three whole tiles and a ragged one on both axes, N = 2
    ((1, 160, 600), (20, 75), 2, 'reduce8'),       # 8:1: the wide tiles' boxes pass the LDS budget (196 KB) and sample global memory
    ((1, 160, 600), (20, 75), 2, 'half'),          # staged and global tiles in one launch
    ((1, 37, 53), (19, 45), 2, 'int32'),           # total definition, clamps
    ((1, 40, 64), (23, 37), 3, 'outside'),         # the replicate border, both kernels' tap clamps
    ((1, 200, 256), (200, 256), 8, 'affine'),      # 2 x 2 nodes
    ((1, 8, 8), (1, 1), 2, 'point'),               # one output pixel
    ((1, 1, 53), (5, 40), 2, 'smooth'),            # one source row
    ((1, 37, 1), (30, 3), 2, 'smooth'),            # one source column
]


def case_inputs(ci, truncate=False):
    """(image, mesh, k, size) of case ci; the image and the mesh are seeded by ci"""
    (n, h, w), size, k, kind = CASES[ci]
    return make_image(n, h, w, 100 + ci), make_mesh(kind, (h, w), size, k, 200 + ci, truncate), k, size


def want(ci, kernel):
    img, mesh, k, size = case_inputs(ci)
    return warp(img, mesh, k, size, kernel)


def _variant(**wrong):
    def run(ci, kernel):
        img, mesh, k, size = case_inputs(ci)
        return warp(img, mesh, k, size, kernel, **wrong)
    return run


def _truncated_nodes(ci, kernel):
    img, mesh, k, size = case_inputs(ci, truncate=True)
    return warp(img, mesh, k, size, kernel)


# name -> (fn(case index, kernel) -> bytes, the kernels it concerns)
WRONG = {
    'no rounding term in the coordinate': (_variant(rounding=False), KERNELS),
    'clamp before the interpolation': (_variant(clamp_first=True), KERNELS),
    'y and x swapped': (_variant(swap=True), KERNELS),
    'truncation toward zero instead of floor for negative coordinates': (_truncated_nodes, KERNELS),
    'Q11 rows without the fix-up': (_variant(fixup=False), ('bicubic',)),
    'bicubic with a rounding between the passes': (_variant(round_between=True), ('bicubic',)),
    'bicubic border by clamping the coordinate pair instead of each tap': (_variant(pair_clamp=True), ('bicubic',)),
}
HARMLESS = {
    'truncation toward zero at the per-pixel shift': (_variant(truncate=True), KERNELS),
    'x1 = x0 + 1 without the clamp': (_variant(x1_clamped=False), ('bilinear',)),
}
