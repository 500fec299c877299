"""The case table of the denoise serving route's argument space and its tie budget: plain CPU code (numpy and
tests/serve_reference.py), in the shape of tests/serve_space_cases.py, whose input and parameter builders, depths and stage
vocabulary it takes over and whose CASES, E32 and TAU it leaves alone.

Cases of risp_serve_denoise_u8 - shape, white and black level, Bayer phase, demosaic, denoiser, the stages in front of it and
behind it, channel order - with their inputs, parameter blocks and float64 reference (serve_reference.serve with
``denoise=``), and the recorded float32 error E32 of the new quantisation points that sets their TAU.  The comparison rule
and the caps are those of tests/serve_space_cases.py (serve_reference.check, TIE_CAP, FINAL_CAP, 8 draws).

tests/test_gpu_serve_denoise_space.py runs every case through the C ABI, the functional wrapper and the composed route built
by hand; tests/test_serve_denoise_reference_cpu.py checks the coverage, the caps of every input, E32, and that the rule tells
wrong variants of the reference apart."""
import functools

import numpy as np

import serve_reference as S
import serve_space_cases as B
from serve_space_cases import (DEPTHS, WB, GA, GT, WQ, G3, CR, FI, make_raw, make_params)
from serve_reference import OP_SKIP

# ---------------------------------------------------------------------------------------------------- the axes
# a thread owns a 2 x 4 patch, a workgroup a 64 x 32 pixel tile that it stages in LDS with a ring of 2 rows / 4 columns:
#   1x4x4     every tap and every ring pixel reflects, on both sides at once
#   3x4x8     a left and a right border patch
#   3x6x12    the first interior patch
#   3x34x68   12 tiles (not the XCD-aware order); the last tile row has 2 rows and the last tile column 4 columns, so the
#             reflection source of the far ring lies in the opposite ring, not in the tile
#   1x66x132  the only shape with a tile that takes no border branch at all
#   8x32x64   8 tiles along z, the XCD-aware order
#   2x64x128  8 tiles across x, y and z, the XCD-aware order
SHAPES = ['1x4x4', '3x4x8', '3x6x12', '3x34x68', '1x66x132', '8x32x64', '2x64x128']
# BIG: mostly random pixels.  Their rows hold at most one further quantisation point beside the denoiser's (no tone curve behind
# a stencil demosaic, no float in front of the median behind one), and they keep off what alone fills TIE_CAP there: the 10-bit
# depths behind the bilinear demosaic (a 2-sample mean x 255 / 1023 is an exact half code when the sum is an odd multiple of
# 341, and every such pixel reaches its neighbours through the denoiser) and behind the nearest one (a gamma of 1024 levels
# puts whole levels within TAU of a boundary whatever the draw).  Both stand in the rows of the smaller shapes
BIG = SHAPES[4:]
DENOISERS = list(S.DENOISERS)
PRE = {'none': [], 'wb': [WB], 'gamma': [GA], 'wb-filmic': [WB, FI], 'crysis': [CR], 'skip-gamma': [OP_SKIP, GA]}
# WbQuadratic stands only behind the denoiser's code (bounded by 1) and nothing follows it: serve_space_cases.TAILS has the reason
POST = {'none': [], 'gamma': [GA], 'gamma-wbq': [GA, WQ], 'filmic-wb-gamma': [FI, WB, GA], 'crysis-gtm': [CR, GT], 'gain3': [G3],
        'skip': [OP_SKIP]}
# per-image values that differ across the batch, at both ends of the plugin rule 1 + 99 p (tests/test_gpu_serve_denoise.py)
SIGMA_COLOR, SIGMA_SPACE, DECAY = [1.0, 37.5, 100.0], [100.0, 1.0, 12.25], [1.0, 20.0, 100.0]

# (shape, white/black, phase, demosaic, denoiser, stages in front, stages behind, reverse).  The bilateral directly behind the
# nearest demosaic belongs to risp_serve_u8 and is not here.  Coverage is checked by tests/test_serve_denoise_reference_cpu.py
CASES = [
    ('1x4x4', '1023/0', 'rggb', 'nearest', 'bilateral', 'wb', 'none', 0),
    ('1x4x4', '1023/64', 'grbg', 'bilinear', 'bilateral', 'wb', 'crysis-gtm', 1),
    ('1x4x4', '16383/512', 'gbrg', 'laplacian', 'bilateral', 'gamma', 'gamma', 1),
    ('1x4x4', '65535/0', 'bggr', 'nearest', 'bilateral', 'wb-filmic', 'gain3', 1),
    ('1x4x4', '1023/0', 'rggb', 'bilinear', 'bilateral', 'crysis', 'gamma-wbq', 0),
    ('1x4x4', '16383/512', 'grbg', 'bilinear', 'median', 'wb', 'gamma-wbq', 0),
    ('1x4x4', '65535/0', 'gbrg', 'laplacian', 'median', 'gamma', 'skip', 0),
    ('1x4x4', '1023/0', 'bggr', 'nearest', 'median', 'wb-filmic', 'filmic-wb-gamma', 1),
    ('1x4x4', '1023/64', 'rggb', 'bilinear', 'median', 'crysis', 'none', 0),
    ('1x4x4', '16383/512', 'grbg', 'laplacian', 'median', 'skip-gamma', 'crysis-gtm', 0),
    ('1x4x4', '1023/0', 'gbrg', 'laplacian', 'fastnlm', 'gamma', 'crysis-gtm', 1),
    ('1x4x4', '1023/64', 'bggr', 'nearest', 'fastnlm', 'wb-filmic', 'gamma', 1),
    ('1x4x4', '16383/512', 'rggb', 'bilinear', 'fastnlm', 'crysis', 'gain3', 0),
    ('1x4x4', '65535/0', 'grbg', 'laplacian', 'fastnlm', 'skip-gamma', 'gamma-wbq', 1),
    ('1x4x4', '1023/0', 'gbrg', 'nearest', 'fastnlm', 'none', 'skip', 1),
    ('3x4x8', '65535/0', 'rggb', 'bilinear', 'bilateral', 'wb-filmic', 'filmic-wb-gamma', 1),
    ('3x4x8', '1023/0', 'grbg', 'laplacian', 'bilateral', 'crysis', 'none', 0),
    ('3x4x8', '1023/64', 'gbrg', 'nearest', 'bilateral', 'skip-gamma', 'crysis-gtm', 0),
    ('3x4x8', '16383/512', 'bggr', 'bilinear', 'bilateral', 'none', 'gamma', 0),
    ('3x4x8', '65535/0', 'rggb', 'laplacian', 'bilateral', 'wb', 'gain3', 1),
    ('3x4x8', '1023/64', 'grbg', 'laplacian', 'median', 'crysis', 'gain3', 0),
    ('3x4x8', '16383/512', 'gbrg', 'nearest', 'median', 'skip-gamma', 'gamma-wbq', 1),
    ('3x4x8', '65535/0', 'bggr', 'bilinear', 'median', 'none', 'skip', 1),
    ('3x4x8', '1023/0', 'rggb', 'laplacian', 'median', 'wb', 'filmic-wb-gamma', 1),
    ('3x4x8', '1023/64', 'grbg', 'nearest', 'median', 'gamma', 'none', 0),
    ('3x4x8', '65535/0', 'gbrg', 'nearest', 'fastnlm', 'skip-gamma', 'none', 0),
    ('3x4x8', '1023/0', 'bggr', 'bilinear', 'fastnlm', 'none', 'crysis-gtm', 0),
    ('3x4x8', '1023/64', 'rggb', 'laplacian', 'fastnlm', 'wb', 'gamma', 1),
    ('3x4x8', '16383/512', 'grbg', 'nearest', 'fastnlm', 'gamma', 'gain3', 0),
    ('3x4x8', '65535/0', 'gbrg', 'bilinear', 'fastnlm', 'wb-filmic', 'gamma-wbq', 0),
    ('3x6x12', '16383/512', 'rggb', 'laplacian', 'bilateral', 'none', 'skip', 1),
    ('3x6x12', '65535/0', 'grbg', 'nearest', 'bilateral', 'wb', 'filmic-wb-gamma', 1),
    ('3x6x12', '1023/0', 'gbrg', 'bilinear', 'bilateral', 'gamma', 'none', 0),
    ('3x6x12', '1023/64', 'bggr', 'laplacian', 'bilateral', 'wb-filmic', 'crysis-gtm', 1),
    ('3x6x12', '16383/512', 'rggb', 'nearest', 'bilateral', 'crysis', 'gamma', 1),
    ('3x6x12', '1023/0', 'grbg', 'nearest', 'median', 'wb', 'gamma', 1),
    ('3x6x12', '1023/64', 'gbrg', 'bilinear', 'median', 'gamma', 'gain3', 0),
    ('3x6x12', '16383/512', 'bggr', 'laplacian', 'median', 'wb-filmic', 'gamma-wbq', 0),
    ('3x6x12', '65535/0', 'rggb', 'nearest', 'median', 'crysis', 'skip', 0),
    ('3x6x12', '1023/0', 'grbg', 'bilinear', 'median', 'skip-gamma', 'filmic-wb-gamma', 1),
    ('3x6x12', '16383/512', 'gbrg', 'bilinear', 'fastnlm', 'gamma', 'filmic-wb-gamma', 0),
    ('3x6x12', '65535/0', 'bggr', 'laplacian', 'fastnlm', 'wb-filmic', 'none', 1),
    ('3x6x12', '1023/0', 'rggb', 'nearest', 'fastnlm', 'crysis', 'crysis-gtm', 1),
    ('3x6x12', '1023/64', 'grbg', 'bilinear', 'fastnlm', 'skip-gamma', 'gamma', 1),
    ('3x6x12', '16383/512', 'gbrg', 'laplacian', 'fastnlm', 'none', 'gain3', 0),
    ('3x34x68', '1023/64', 'rggb', 'nearest', 'bilateral', 'wb-filmic', 'gamma-wbq', 0),
    ('3x34x68', '16383/512', 'grbg', 'bilinear', 'bilateral', 'crysis', 'skip', 0),
    ('3x34x68', '65535/0', 'gbrg', 'laplacian', 'bilateral', 'skip-gamma', 'filmic-wb-gamma', 1),
    ('3x34x68', '1023/0', 'bggr', 'nearest', 'bilateral', 'wb', 'none', 0),
    ('3x34x68', '1023/64', 'rggb', 'bilinear', 'bilateral', 'wb', 'crysis-gtm', 0),
    ('3x34x68', '65535/0', 'grbg', 'bilinear', 'median', 'crysis', 'crysis-gtm', 1),
    ('3x34x68', '1023/0', 'gbrg', 'laplacian', 'median', 'skip-gamma', 'gamma', 1),
    ('3x34x68', '1023/64', 'bggr', 'nearest', 'median', 'none', 'gain3', 0),
    ('3x34x68', '16383/512', 'rggb', 'bilinear', 'median', 'wb', 'gamma-wbq', 1),
    ('3x34x68', '65535/0', 'grbg', 'laplacian', 'median', 'gamma', 'skip', 1),
    ('3x34x68', '1023/64', 'gbrg', 'laplacian', 'fastnlm', 'skip-gamma', 'skip', 1),
    ('3x34x68', '16383/512', 'bggr', 'nearest', 'fastnlm', 'none', 'filmic-wb-gamma', 0),
    ('3x34x68', '65535/0', 'rggb', 'bilinear', 'fastnlm', 'wb', 'none', 0),
    ('3x34x68', '1023/0', 'grbg', 'laplacian', 'fastnlm', 'gamma', 'crysis-gtm', 0),
    ('3x34x68', '1023/64', 'gbrg', 'nearest', 'fastnlm', 'wb-filmic', 'gamma', 1),
    ('1x66x132', '16383/512', 'rggb', 'bilinear', 'bilateral', 'none', 'gain3', 0),
    ('1x66x132', '1023/64', 'grbg', 'laplacian', 'bilateral', 'wb', 'gamma-wbq', 1),
    ('1x66x132', '16383/512', 'gbrg', 'nearest', 'bilateral', 'gamma', 'skip', 1),
    ('1x66x132', '16383/512', 'bggr', 'bilinear', 'bilateral', 'skip-gamma', 'gain3', 1),
    ('1x66x132', '1023/0', 'rggb', 'laplacian', 'bilateral', 'skip-gamma', 'none', 0),
    ('1x66x132', '16383/512', 'grbg', 'laplacian', 'median', 'none', 'none', 0),
    ('1x66x132', '16383/512', 'gbrg', 'nearest', 'median', 'gamma', 'crysis-gtm', 0),
    ('1x66x132', '16383/512', 'bggr', 'bilinear', 'median', 'none', 'gamma', 1),
    ('1x66x132', '1023/64', 'rggb', 'laplacian', 'median', 'none', 'gain3', 0),
    ('1x66x132', '65535/0', 'grbg', 'nearest', 'median', 'skip-gamma', 'gamma-wbq', 0),
    ('1x66x132', '16383/512', 'gbrg', 'nearest', 'fastnlm', 'gamma', 'gamma-wbq', 1),
    ('1x66x132', '16383/512', 'bggr', 'bilinear', 'fastnlm', 'skip-gamma', 'skip', 1),
    ('1x66x132', '16383/512', 'rggb', 'laplacian', 'fastnlm', 'skip-gamma', 'gain3', 0),
    ('1x66x132', '65535/0', 'grbg', 'nearest', 'fastnlm', 'skip-gamma', 'none', 1),
    ('1x66x132', '16383/512', 'gbrg', 'bilinear', 'fastnlm', 'none', 'gain3', 1),
    ('8x32x64', '65535/0', 'rggb', 'laplacian', 'bilateral', 'skip-gamma', 'gamma', 1),
    ('8x32x64', '16383/512', 'grbg', 'nearest', 'bilateral', 'crysis', 'gain3', 0),
    ('8x32x64', '16383/512', 'gbrg', 'bilinear', 'bilateral', 'skip-gamma', 'gamma-wbq', 0),
    ('8x32x64', '16383/512', 'bggr', 'laplacian', 'bilateral', 'none', 'skip', 0),
    ('8x32x64', '65535/0', 'rggb', 'nearest', 'bilateral', 'wb', 'filmic-wb-gamma', 1),
    ('8x32x64', '16383/512', 'grbg', 'nearest', 'median', 'crysis', 'gain3', 0),
    ('8x32x64', '16383/512', 'gbrg', 'bilinear', 'median', 'none', 'none', 1),
    ('8x32x64', '65535/0', 'bggr', 'laplacian', 'median', 'none', 'gain3', 1),
    ('8x32x64', '65535/0', 'rggb', 'nearest', 'median', 'wb', 'gamma', 1),
    ('8x32x64', '16383/512', 'grbg', 'bilinear', 'median', 'none', 'gain3', 0),
    ('8x32x64', '16383/512', 'gbrg', 'bilinear', 'fastnlm', 'skip-gamma', 'gain3', 0),
    ('8x32x64', '1023/0', 'bggr', 'laplacian', 'fastnlm', 'none', 'gamma-wbq', 0),
    ('8x32x64', '65535/0', 'rggb', 'nearest', 'fastnlm', 'wb', 'skip', 1),
    ('8x32x64', '16383/512', 'grbg', 'bilinear', 'fastnlm', 'gamma', 'gain3', 0),
    ('8x32x64', '65535/0', 'gbrg', 'laplacian', 'fastnlm', 'skip-gamma', 'none', 0),
    ('2x64x128', '16383/512', 'rggb', 'nearest', 'bilateral', 'wb', 'crysis-gtm', 1),
    ('2x64x128', '16383/512', 'grbg', 'bilinear', 'bilateral', 'wb', 'gamma', 1),
    ('2x64x128', '1023/0', 'gbrg', 'laplacian', 'bilateral', 'gamma', 'gain3', 0),
    ('2x64x128', '65535/0', 'bggr', 'nearest', 'bilateral', 'wb-filmic', 'gamma-wbq', 1),
    ('2x64x128', '16383/512', 'rggb', 'bilinear', 'bilateral', 'skip-gamma', 'skip', 1),
    ('2x64x128', '16383/512', 'grbg', 'bilinear', 'median', 'none', 'skip', 1),
    ('2x64x128', '1023/64', 'gbrg', 'laplacian', 'median', 'none', 'gain3', 0),
    ('2x64x128', '65535/0', 'bggr', 'nearest', 'median', 'wb-filmic', 'none', 0),
    ('2x64x128', '16383/512', 'rggb', 'bilinear', 'median', 'none', 'gain3', 0),
    ('2x64x128', '1023/0', 'grbg', 'laplacian', 'median', 'none', 'gamma', 1),
    ('2x64x128', '16383/512', 'gbrg', 'laplacian', 'fastnlm', 'gamma', 'gamma', 0),
    ('2x64x128', '65535/0', 'bggr', 'nearest', 'fastnlm', 'wb-filmic', 'gain3', 1),
    ('2x64x128', '16383/512', 'rggb', 'bilinear', 'fastnlm', 'skip-gamma', 'gamma-wbq', 1),
    ('2x64x128', '1023/64', 'grbg', 'laplacian', 'fastnlm', 'skip-gamma', 'skip', 1),
    ('2x64x128', '16383/512', 'gbrg', 'nearest', 'fastnlm', 'none', 'filmic-wb-gamma', 0),
]
WALK = 16

# ---------------------------------------------------------------------------------------------------- the tie budget
# E32[kind] as tests/serve_space_cases.py defines it, for the quantisation points this route adds: the largest |v32 - v64|,
# in codes, over every input of CASES and the walk, where v32 is the reference's own expression evaluated in float32 on the
# CPU (exp as exp2(x * log2 e) in float32; every segment started from the float64 run's codes) and v64 the float64
# reference.  'den-bilateral' and 'fastnlm': the denoiser's weighted mean; 'median-in/<op>': the median's input x 255 where
# a float stands in front of it (behind a carried code the median is exact and has no point).  TAU = 2 x E32, the project's
# factor.  These values come from the CPU float32 evaluation only; nothing here is taken from a run of the kernels.
# tests/test_serve_denoise_reference_cpu.py re-measures them.  Every other kind keeps the TAU of tests/serve_space_cases.py.
E32 = {
    'den-bilateral': 7.60e-5, 'fastnlm': 8.25e-5, 'median-in/nearest': 1.47e-5, 'median-in/wb_manual': 2.34e-5, 'median-in/gamma': 2.42e-5,
    # kinds of tests/serve_space_cases.py whose float32 error over THIS table's inputs is larger than over that table's (there
    # 2.91e-5, 5.67e-5 and 3.19e-4): the largest of a sample grows with the sample.  Here they take this table's value
    'bilinear': 3.23e-5, 'laplacian': 6.73e-5, 'final/wb_quadratic': 3.49e-4,
}
TAU = {**B.TAU, **{k: 2.0 * v for k, v in E32.items()}}


# ---------------------------------------------------------------------------------------------------- builders (CPU)
def make_input(n, h, w, white, black, seed):
    """serve_space_cases.make_raw (image 1 all zero, image 2 constant, planted black- and white-level samples); in a batch of
    two or more the lower right quarter of image 0 is made of flat 2 x 4 blocks of four levels, as _frames of
    tests/test_gpu_serve_denoise.py: medians with many equal codes, a normaliser near its maximum beside one near 1"""
    raw = make_raw(n, h, w, white, black, seed)
    if n > 1:
        rng = np.random.default_rng(seed + 7)
        levels = black + (np.array([0, 29, 59, 88]) * (white - black)) // 100 + rng.integers(0, 3, size=4)
        bh, bw = (h // 2 + 1) // 2, (w // 2 + 3) // 4
        blocks = levels[rng.integers(0, 4, size=(bh, bw))]
        raw[0, h // 2:, w // 2:] = np.repeat(np.repeat(blocks, 2, axis=0), 4, axis=1)[:h - h // 2, :w - w // 2]
        raw[0, -1, -1] = black
    return raw


def denoise_args(name, n):
    pick = lambda vals: np.array([vals[i % len(vals)] for i in range(n)], np.float32)
    return {'bilateral': (pick(SIGMA_COLOR), pick(SIGMA_SPACE)), 'median': (), 'fastnlm': (pick(DECAY),)}[name]


def _build(row, seed0, what):
    shape, depth, phase, demosaic, name, pre, post, reverse = row
    n, h, w = B._shape(shape)
    white, black = (int(v) for v in depth.split('/'))
    pre = list(PRE[pre]) if isinstance(pre, str) else list(pre)              # the walk hands its op lists over
    post = list(POST[post]) if isinstance(post, str) else list(post)
    ops = pre + post
    case = dict(n=n, h=h, w=w, white=white, black=black, phase=phase, demosaic=demosaic, ops=ops, reverse=bool(reverse), what=what,
                params=make_params(ops, n, np.random.default_rng(seed0 + 1)), denoise=(name, len(pre), denoise_args(name, n)))
    for attempt in range(8):                                # an input over a cap is drawn again (the input's property alone)
        case['raw'] = make_input(n, h, w, white, black, seed0 + 100 * attempt)
        case['ref'] = reference(case)
        inner, loose = S.tie_shares(case['ref'], TAU)
        if inner <= S.TIE_CAP and loose <= S.FINAL_CAP:
            case['draws'] = attempt + 1
            return case
    raise AssertionError('%s: no input under the caps in 8 draws (inner %.3e, +-1 bytes %.3e)' % (what, inner, loose))


def reference(case, dtype=np.float64, sync=None, reverse=None):
    return S.serve(case['raw'], case['white'], case['black'], case['phase'], case['demosaic'], None, case['ops'], case['params'],
                   case['reverse'] if reverse is None else reverse, dtype, sync, denoise=case['denoise'])


@functools.lru_cache(maxsize=None)
def sweep_case(index):
    return _build(CASES[index], 17000 + 13 * index, 'case %d: %s %s %s %s %s %s %s reverse %d' % ((index,) + CASES[index]))


@functools.lru_cache(maxsize=None)
def walk_case(seed):
    """one step of the seeded walk over the same axes, from the five smaller shapes (at the eight-tile shapes and 1x66x132 the
    ties of a random list's quantisation points alone reach the cap)"""
    rng = np.random.default_rng(19100 + seed)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    shape, demosaic, name = pick(SHAPES[:5]), pick(list(S.DEMOSAIC)), pick(DENOISERS)
    pre, post = pick(list(PRE)), pick(list(POST))
    depth = pick(DEPTHS)
    if name == 'bilateral' and demosaic == 'nearest' and pre == 'none':     # risp_serve_u8's
        pre = 'gamma'
    if shape in BIG:                                         # the rules of the table's large shapes
        tone_pre, tone_post = pre in ('wb-filmic', 'crysis'), post in ('filmic-wb-gamma', 'crysis-gtm')
        if tone_post and (demosaic != 'nearest' or tone_pre):
            post = 'gamma'
        if demosaic != 'nearest' and (tone_pre or name == 'median'):
            pre = 'none'
        if demosaic == 'bilinear':
            depth = '16383/512'
        elif demosaic == 'nearest' and depth.startswith('1023'):
            depth = '65535/0'
    row = (shape, depth, pick(list(S.SITES)), demosaic, name, pre, post, int(rng.integers(0, 2)))
    return _build(row, 19500 + 17 * seed, 'walk %d: %s %s %s %s %s %s %s reverse %d' % ((seed,) + row))
