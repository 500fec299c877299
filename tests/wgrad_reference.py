"""``convnets.conv_wgrad`` (risp_conv2d_wgrad, risp_conv_wgrad.hip) over its argument space, stated without the GPU: the float64 / float32
restatement of the weight gradient, which template instance the dispatch takes, the size of its scratch, what the entry point refuses,
and the table of cases tests/test_gpu_wgrad_space.py runs.  Plain torch on the CPU; checked by tests/test_wgrad_reference_cpu.py.

The operation (include/risp.h):

    dW[co][ci][ky][kx] = sum over (n, y, x) of gy[n, co, y, x] * X[n, ci, y + ky - p, x + kx - p]        p = k // 2, X zero outside the image
    db[co]             = sum over (n, y, x) of gy[n, co, y, x]

where X is x itself (PLAIN), or x's ``cin_img`` image channels followed by planes that hold the per-image constants ``cvals[n, j]``
(CONSTCH: channel cin_img + j).  A constant plane is zero outside the image like every other channel.

The dispatch (risp_conv2d_wgrad): k = 1 alone, then per k in 3 / 5 / 9 three forms - 'thin_in' where cin * k <= 32 (matrix columns are
(ci, kx) pairs), 'thin_out' where cout * k <= 32 and the layer is not thin-in (rows are (co, kx) pairs), 'plain' otherwise."""
import functools
import os

import numpy as np
import torch

PLAIN, UNSHUFFLE, CONSTCH = 0, 1, 2                 # include/risp.h: RISP_LOAD_*
BAR = 3e-6                                          # max |dW - ref| / max|ref|: the bar of the fp32-accumulating conv kernels (test_gpu_toep.py)
WG_TOTAL, SLOT, GW, GH = 768, 1024, 16, 8           # workgroups of a launch, floats of a slot, the pixel tile
FORMS = ('k1', 'plain', 'thin_in', 'thin_out')


# ----------------------------------------------------------------------------------------------------------------------------
# the restatement
def restate(x, gy, k, cvals=None, cin_img=0, dtype=torch.float64):
    """(dW (cout, cin, k, k), db (cout,)) in ``dtype`` from the definition: constant planes materialised, k // 2 zeros on every side, per tap
    one shifted window and one sum over (n, y, x).  No autograd."""
    x, gy = x.to(dtype), gy.to(dtype)
    n, _, h, w = gy.shape
    if cvals is not None:
        assert cin_img == x.shape[1] and cvals.shape[0] == n
        x = torch.cat([x, cvals.to(dtype)[:, :, None, None].expand(-1, -1, h, w)], dim=1)
    cin, cout, p = x.shape[1], gy.shape[1], k // 2
    xp = torch.zeros((n, cin, h + 2 * p, w + 2 * p), dtype=dtype)
    xp[:, :, p:p + h, p:p + w] = x
    dw = torch.empty((cout, cin, k, k), dtype=dtype)
    for ky in range(k):
        for kx in range(k):
            dw[:, :, ky, kx] = torch.einsum('nohw,nihw->oi', gy, xp[:, :, ky:ky + h, kx:kx + w])
    return dw, gy.sum(dim=(0, 2, 3))


def never_lands(k, h, w):
    """(k, k) bool: taps whose window lies in the padding for every pixel of an h x w plane - their gradient is exactly zero"""
    p = k // 2
    ky, kx = torch.arange(k).view(k, 1), torch.arange(k).view(1, k)
    return ((ky - p).abs() >= h) | ((kx - p).abs() >= w)


# ----------------------------------------------------------------------------------------------------------------------------
# the header's contract
def form(cin, cout, k):
    if k == 1:
        return 'k1'
    if cin * k <= 32:
        return 'thin_in'
    return 'thin_out' if cout * k <= 32 else 'plain'


def scratch_floats(cin, cout, k):
    """slots of 1024 floats, one per workgroup and tap chain: k * k chains in the plain form, k where the filter column is in the matrix"""
    return WG_TOTAL * (k if form(cin, cout, k) in ('thin_in', 'thin_out') else k * k) * SLOT


def lds_floats(cin, k):
    """the gy tile (32 planes of 16 x 8 + 1) and the input tile with its halo (at most 32 planes, odd stride)"""
    return 32 * (GW * GH + 1) + min(cin, 32) * (((GW + k - 1) * (GH + k - 1)) | 1)


def accepts(case):
    """what risp_conv2d_wgrad and the bias sums behind ``conv_wgrad`` (risp_plane_sums) take; ``case``: k, cin, cout, n, h, w, load, cin_img,
    cvals (whether the constants are passed)"""
    c = case
    return (c['n'] > 0 and c['h'] > 0 and c['w'] > 0 and 1 <= c['cin'] <= 64 and 1 <= c['cout'] <= 64 and c['k'] in (1, 3, 5, 9)
            and lds_floats(c['cin'], c['k']) * 4 <= 64 * 1024
            and c['n'] * c['cout'] <= 65535
            and (c['load'] == PLAIN or (c['load'] == CONSTCH and bool(c.get('cvals', True)) and c['cin_img'] > 0)))


def shortcut(case):
    """``conv_wgrad``'s first-layer shortcut: the image channels through the matrix kernel (thin-in), the constant planes as cvals^T @
    rectangle sums of gy (risp_rect_sums: H, W >= k // 2, W <= 8192)"""
    c = case
    return c['load'] == CONSTCH and c['cin_img'] * c['k'] <= 32 and c['h'] >= c['k'] // 2 and c['k'] // 2 <= c['w'] <= 8192


def launched(case):
    """(cin, cout, k) of the one risp_conv2d_wgrad launch of a case"""
    return (case['cin_img'] if shortcut(case) else case['cin'], case['cout'], case['k'])


# ----------------------------------------------------------------------------------------------------------------------------
# the case table
LAYERS = [                                                          # (k, literal form, [(cin, cout), ...])
    (1, 'k1', [(64, 32), (5, 5), (33, 1), (1, 64)]),
    (3, 'plain', [(64, 64), (11, 11), (33, 40)]),
    (3, 'thin_in', [(3, 64), (10, 10), (1, 1), (10, 33)]),
    (3, 'thin_out', [(64, 3), (11, 10), (40, 1)]),
    (5, 'plain', [(64, 32), (7, 7), (33, 33)]),
    (5, 'thin_in', [(6, 40), (1, 3), (6, 6)]),                       # (6, 6): both thin - thin-in wins
    (5, 'thin_out', [(32, 3), (40, 6), (7, 6)]),
    (9, 'plain', [(17, 64), (4, 4), (31, 64)]),                      # 31: the largest cin the LDS check admits at 9x9
    (9, 'thin_in', [(3, 64), (1, 1), (3, 3)]),
    (9, 'thin_out', [(24, 3), (31, 3), (4, 1)]),
]
REFUSED_LAYERS = [(32, 64, 9), (64, 3, 9), (17, 64, 7), (3, 3, 7), (65, 8, 3), (65, 64, 1)]       # (cin, cout, k)
# (1, 8, 16) is exactly one tile, (1, 9, 17) one past it on both axes
COMMON = [(2, 3, 4), (1, 8, 16), (1, 9, 17), (3, 7, 15)]
ROTATING = [(1, 1, 1), (1, 1, 4), (5, 2, 70), (2, 20, 36), (1, 33, 30)]
MANY = (771, 8, 16)                                                 # one tile per image, more tiles than any slice count (<= 768)
MANY_LAYERS = [(64, 64, 3), (3, 64, 9), (32, 3, 5), (64, 32, 1), (17, 64, 9)]
CASES = {}


def _case(k, cin, cout, n, h, w, frm, load=PLAIN, cin_img=0, short=False, table=None, tag=''):
    name = '%s%dx%d_%dto%d %s %dx%dx%d' % (tag, k, k, cin, cout, frm or 'walk', n, h, w) + (' constch %d' % cin_img if load == CONSTCH else '')
    table = CASES if table is None else table
    assert name not in table, name
    table[name] = dict(name=name, k=k, cin=cin, cout=cout, n=n, h=h, w=w, form=frm, load=load, cin_img=cin_img, shortcut=short)
    return table[name]


_i = 0
for _k, _form, _pairs in LAYERS:
    for _ci, _co in _pairs:
        for _n, _h, _w in COMMON + [ROTATING[_i % len(ROTATING)]]:
            _case(_k, _ci, _co, _n, _h, _w, _form)
        _i += 1
for _ci, _co, _k in MANY_LAYERS:
    _case(_k, _ci, _co, *MANY, form(_ci, _co, _k))
# SRCNNRes' first layer (3 image channels, then min / mean / max of each and P parameters): the shortcut at the smallest shape it accepts and at
# a ragged one; at h < 4 the kernel's own CONSTCH branch.  ``form`` is the form of the launch: thin-in on the 3 image channels
for _P in (0, 1, 5):
    for _n, _h, _w in ((2, 4, 4), (3, 20, 36)):
        _case(9, 12 + _P, 64, _n, _h, _w, 'thin_in', CONSTCH, 3, short=True)
    _case(9, 12 + _P, 64, 2, 3, 9, 'plain', CONSTCH, 3)
# the kernel's branch by construction (cin_img * k > 32), the last with constants on both sides of the 32-channel block in the thin-out
# form.  The same 40 -> 6 layer with 3 image channels (3 * 5 <= 32) takes the shortcut wherever the image holds the halo, and the kernel
# on a one-row image; last, the thin-in form of the branch (an image lower than the 9x9 halo)
for _k, _ci, _co, _img, _form in ((9, 17, 64, 4, 'plain'), (3, 20, 33, 12, 'plain'), (5, 40, 6, 3 + 8, 'thin_out')):
    for _n, _h, _w in ((2, 9, 17), (3, 7, 15)):
        _case(_k, _ci, _co, _n, _h, _w, _form, CONSTCH, _img)
for _n, _h, _w in ((2, 3, 4), (3, 7, 15)):
    _case(5, 40, 6, _n, _h, _w, 'thin_in', CONSTCH, 3, short=True)                   # 3 * 5 <= 32: the shortcut, with 37 constant planes
_case(5, 40, 6, 2, 1, 17, 'thin_out', CONSTCH, 3)                                    # ... and h < 2: the kernel, constants across the block
_case(9, 3, 64, 2, 3, 9, 'thin_in', CONSTCH, 2)

SEEDS = int(os.environ.get('RISP_TEST_SEEDS', '8'))


def walk(seed=20262, draws=6 * SEEDS):
    """a seeded walk: (k, cin, cout, n <= 4, h <= 40, w <= 70, load mode) uniform over what ``accepts`` admits"""
    rng = np.random.default_rng(seed)
    out = {}
    while len(out) < draws:
        k = (1, 3, 5, 9)[int(rng.integers(4))]
        cin, cout, n, h, w = (int(rng.integers(1, hi + 1)) for hi in (64, 64, 4, 40, 70))
        load = (PLAIN, CONSTCH)[int(rng.integers(2))]
        cin_img = int(rng.integers(1, cin)) if load == CONSTCH and cin > 1 else 0
        c = dict(k=k, cin=cin, cout=cout, n=n, h=h, w=w, load=load, cin_img=cin_img)
        if (load == CONSTCH and cin_img == 0) or not accepts(c):
            continue
        _case(k, cin, cout, n, h, w, None, load, cin_img, short=None, table=out, tag='walk %02d ' % len(out))
    return out


WALK = walk()
ALL = dict(CASES)
ALL.update(WALK)


# ----------------------------------------------------------------------------------------------------------------------------
# inputs and references, computed once and shared
def rnd(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def hash_name(name):
    v = 0
    for ch in name.encode():
        v = (v * 131 + ch) % (2 ** 31 - 1)
    return v


# table cases whose draw put the float32 restatement itself past a quarter of the bar (tests/test_wgrad_reference_cpu.py: 7.7e-7 of max|ref| on
# 306 pixels, where the CPU's float32 sum runs in sequence): other inputs, not a wider bar
RESEED = {'5x5_40to6 thin_out 2x9x17 constch 11': 1}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = ALL[name]
    rng = np.random.Generator(np.random.PCG64(hash_name(name) + RESEED.get(name, 0)))
    img = c['cin_img'] if c['load'] == CONSTCH else c['cin']
    x, gy = rnd(rng, c['n'], img, c['h'], c['w']), rnd(rng, c['n'], c['cout'], c['h'], c['w'])
    return x, gy, (rnd(rng, c['n'], c['cin'] - img) if c['load'] == CONSTCH else None)


def inputs(case):
    """(x, gy, cvals or None): CPU float32 standard normals (cached, shared by every test that needs them: do not write into them)"""
    return _inputs(case['name'])


@functools.lru_cache(maxsize=None)
def _ref64(name):
    x, gy, cv = _inputs(name)
    return restate(x, gy, ALL[name]['k'], cv, ALL[name]['cin_img'])


def ref64(case):
    """the float64 restatement (dW, db) of a case, computed once (do not write into it)"""
    return _ref64(case['name'])


def ref32(case):
    """the same in float32 with float32 accumulation: what fp32 arithmetic costs on these inputs"""
    x, gy, cv = inputs(case)
    return restate(x, gy, case['k'], cv, case['cin_img'], dtype=torch.float32)


def errors(dw, ref):
    """(rms, max) of dW - ref relative to max|ref|"""
    m = ref.abs().max().item() or 1.0
    e = dw.double().cpu() - ref
    return e.pow(2).mean().sqrt().item() / m, e.abs().max().item() / m
