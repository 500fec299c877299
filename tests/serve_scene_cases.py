"""The case table of the scene route of the serving path (risp_serve_scene_stats / _finish / _u8) and its tie budget: plain
CPU code (numpy, tests/serve_scene_reference.py, and the builders of tests/serve_space_cases.py).

A case is a shape, a white / black level, a Bayer phase, a demosaic kind, a stage list with one or two scene stages
(gray-world, white-world, Reinhard) and a channel order, with its input, parameter blocks and float64 reference.  The
comparison rule is serve_reference.check, the caps TIE_CAP / FINAL_CAP are that file's, and the reference is evaluated in
three worlds (serve_scene_reference.worlds): a whole-image statistic couples the pixels, so a byte is decided only if it
is the same however the inner ties in front of the statistic fall.

Shapes (a thread owns a 2 x 4 patch, a workgroup a 64 x 32 pixel tile and writes one partial row):
  1x4x4     every tap reflects; one workgroup that is almost all idle threads
  3x6x12    several images at a small ragged size
  3x34x68   four ragged workgroups per image
  8x32x64   eight workgroups in total: the XCD remap is active
  2x66x132  nine partials per image; a total that is no multiple of 8
Image 1 is all zero and image 2 constant (serve_space_cases.make_raw): the 1e-6 / 1e-3 / 1e-4 floors are exercised.

Two properties of the inputs keep the reference alone under TIE_CAP.  Reinhard's keys sit at the dark end (make_scene_params): the
float32 sum of logarithms costs about 2e-6 relative in exp(mean), 255 times that in codes at the top of the range, and with a
bright curve TAU['reinhard'] alone would put more than TIE_CAP of uniformly spread pixels within TAU of a boundary.  The
eight-tile shape with its 16384 pixels meets the 10-bit depths where a stencil demosaic is followed by another quantisation
point: at 16 bits the exact ties of a 2-sample mean alone reach the cap (serve_space_cases.walk_case says the same).
"""
import functools

import numpy as np

import serve_reference as S
import serve_scene_reference as SC
import serve_space_cases as T
from serve_scene_reference import GRAYWORLD as GW, WHITEWORLD as WW, REINHARD as RH
from serve_space_cases import WB, GA, GT, WQ, G3, CR, FI, DEPTHS
from serve_reference import OP_SKIP

SHAPES = ['1x4x4', '3x6x12', '3x34x68', '8x32x64', '2x66x132']
PIPES = {
    # the scene stage directly behind the demosaic
    'gw': [GW], 'ww': [WW], 'rh': [RH],
    # ... behind an element-wise prefix that includes WbQuadratic (its input bounded by 1, nothing steep behind it)
    'gamma-wbq-gw': [GA, WQ, GW], 'gamma-wbq-ww': [GA, WQ, WW], 'gtm-wbq-rh': [GT, WQ, RH],
    # ... followed by a tail
    'gw-gamma': [GW, GA], 'ww-crysis-gtm': [WW, CR, GT], 'rh-gamma': [RH, GA], 'skip-wb-gw-skip-gtm': [OP_SKIP, WB, GW, OP_SKIP, GT],
    'filmic-ww-gain3': [FI, WW, G3],
    # two scene stages: the second statistic runs its prefix through the first stage with that stage's constants
    'gw-rh': [GW, RH], 'ww-gw': [WW, GW], 'wb-gw-gamma-rh': [WB, GW, GA, RH], 'ww-gamma-gw-gtm': [WW, GA, GW, GT],
}
# (shape, white/black, phase, demosaic, pipe, reverse).  Coverage is checked by tests/test_serve_scene_reference_cpu.py
CASES = [
    ('1x4x4', '1023/0', 'rggb', 'nearest', 'gw', 0),
    ('3x6x12', '65535/0', 'grbg', 'bilinear', 'ww', 1),
    ('3x34x68', '16383/512', 'gbrg', 'laplacian', 'rh', 0),
    ('8x32x64', '1023/64', 'bggr', 'nearest', 'gamma-wbq-gw', 1),
    ('2x66x132', '16383/512', 'grbg', 'laplacian', 'gamma-wbq-ww', 0),
    ('1x4x4', '65535/0', 'gbrg', 'laplacian', 'gtm-wbq-rh', 1),
    ('3x6x12', '16383/512', 'bggr', 'nearest', 'gw-gamma', 0),
    ('3x34x68', '1023/64', 'rggb', 'bilinear', 'ww-crysis-gtm', 1),
    ('8x32x64', '1023/0', 'gbrg', 'laplacian', 'rh-gamma', 0),
    ('2x66x132', '65535/0', 'bggr', 'nearest', 'skip-wb-gw-skip-gtm', 1),
    ('1x4x4', '16383/512', 'rggb', 'bilinear', 'filmic-ww-gain3', 0),
    ('3x6x12', '1023/64', 'grbg', 'laplacian', 'gw-rh', 1),
    ('2x66x132', '1023/0', 'bggr', 'nearest', 'ww-gw', 0),
    ('8x32x64', '65535/0', 'rggb', 'laplacian', 'wb-gw-gamma-rh', 1),
    ('2x66x132', '16383/512', 'grbg', 'laplacian', 'ww-gamma-gw-gtm', 0),
    ('2x66x132', '1023/64', 'gbrg', 'bilinear', 'gw', 1),
    ('3x34x68', '1023/0', 'bggr', 'laplacian', 'ww', 0),
    ('8x32x64', '65535/0', 'rggb', 'nearest', 'rh', 1),
    ('2x66x132', '16383/512', 'grbg', 'bilinear', 'gamma-wbq-gw', 0),
    ('1x4x4', '1023/64', 'bggr', 'laplacian', 'gamma-wbq-ww', 1),
    ('3x6x12', '1023/0', 'rggb', 'nearest', 'gtm-wbq-rh', 0),
    ('3x34x68', '65535/0', 'grbg', 'bilinear', 'gw-gamma', 1),
    ('8x32x64', '16383/512', 'gbrg', 'laplacian', 'ww-crysis-gtm', 0),
    ('2x66x132', '1023/64', 'rggb', 'nearest', 'rh-gamma', 1),
    ('1x4x4', '1023/0', 'grbg', 'bilinear', 'skip-wb-gw-skip-gtm', 0),
    ('3x6x12', '65535/0', 'gbrg', 'laplacian', 'filmic-ww-gain3', 1),
    ('3x34x68', '16383/512', 'bggr', 'nearest', 'gw-rh', 0),
    ('1x4x4', '1023/64', 'grbg', 'bilinear', 'ww-gw', 1),
    ('2x66x132', '1023/0', 'gbrg', 'laplacian', 'wb-gw-gamma-rh', 0),
    ('1x4x4', '65535/0', 'bggr', 'nearest', 'ww-gamma-gw-gtm', 1),
    ('2x66x132', '16383/512', 'rggb', 'laplacian', 'gw', 0),
    ('8x32x64', '1023/64', 'grbg', 'nearest', 'ww', 1),
    ('2x66x132', '16383/512', 'gbrg', 'bilinear', 'rh', 0),
    ('1x4x4', '65535/0', 'bggr', 'laplacian', 'gamma-wbq-gw', 1),
    ('3x6x12', '16383/512', 'grbg', 'nearest', 'gamma-wbq-ww', 0),
    ('3x34x68', '1023/64', 'gbrg', 'bilinear', 'gtm-wbq-rh', 1),
    ('8x32x64', '1023/0', 'bggr', 'laplacian', 'gw-gamma', 0),
    ('2x66x132', '65535/0', 'rggb', 'nearest', 'ww-crysis-gtm', 1),
    ('1x4x4', '16383/512', 'gbrg', 'bilinear', 'rh-gamma', 0),
    ('3x6x12', '1023/64', 'bggr', 'laplacian', 'skip-wb-gw-skip-gtm', 1),
    ('3x34x68', '1023/0', 'rggb', 'nearest', 'filmic-ww-gain3', 0),
    ('8x32x64', '1023/64', 'grbg', 'laplacian', 'gw-rh', 1),
    ('2x66x132', '16383/512', 'bggr', 'laplacian', 'ww-gw', 0),
    ('1x4x4', '1023/64', 'rggb', 'nearest', 'wb-gw-gamma-rh', 1),
    ('3x6x12', '1023/0', 'grbg', 'bilinear', 'ww-gamma-gw-gtm', 0),
    ('8x32x64', '65535/0', 'gbrg', 'nearest', 'gw', 1),
    ('2x66x132', '16383/512', 'bggr', 'bilinear', 'ww', 0),
    ('1x4x4', '1023/64', 'rggb', 'laplacian', 'rh', 1),
    ('3x6x12', '1023/0', 'grbg', 'nearest', 'gamma-wbq-gw', 0),
    ('3x34x68', '65535/0', 'bggr', 'nearest', 'gamma-wbq-ww', 1),
    ('3x6x12', '16383/512', 'rggb', 'laplacian', 'gtm-wbq-rh', 0),
    ('2x66x132', '1023/64', 'grbg', 'nearest', 'gw-gamma', 1),
    ('1x4x4', '1023/0', 'gbrg', 'bilinear', 'ww-crysis-gtm', 0),
    ('3x6x12', '65535/0', 'rggb', 'laplacian', 'rh-gamma', 1),
    ('3x34x68', '16383/512', 'grbg', 'nearest', 'skip-wb-gw-skip-gtm', 0),
    ('8x32x64', '1023/64', 'gbrg', 'nearest', 'filmic-ww-gain3', 1),
    ('2x66x132', '1023/0', 'bggr', 'laplacian', 'gw-rh', 0),
    ('1x4x4', '65535/0', 'grbg', 'nearest', 'ww-gw', 1),
    ('3x6x12', '16383/512', 'gbrg', 'bilinear', 'wb-gw-gamma-rh', 0),
    ('3x34x68', '1023/64', 'bggr', 'laplacian', 'ww-gamma-gw-gtm', 1),
    ('2x66x132', '1023/0', 'rggb', 'bilinear', 'gw', 0),
    ('1x4x4', '65535/0', 'grbg', 'laplacian', 'ww', 1),
    ('3x6x12', '16383/512', 'gbrg', 'nearest', 'rh', 0),
    ('3x34x68', '1023/64', 'bggr', 'bilinear', 'gamma-wbq-gw', 1),
    ('8x32x64', '1023/0', 'grbg', 'nearest', 'gamma-wbq-ww', 0),
    ('2x66x132', '65535/0', 'gbrg', 'nearest', 'gtm-wbq-rh', 1),
    ('1x4x4', '16383/512', 'bggr', 'bilinear', 'gw-gamma', 0),
    ('3x6x12', '1023/64', 'rggb', 'laplacian', 'ww-crysis-gtm', 1),
    ('3x34x68', '1023/0', 'gbrg', 'nearest', 'rh-gamma', 0),
    ('8x32x64', '1023/64', 'bggr', 'laplacian', 'skip-wb-gw-skip-gtm', 1),
    ('2x66x132', '16383/512', 'rggb', 'laplacian', 'filmic-ww-gain3', 0),
    ('1x4x4', '1023/64', 'grbg', 'nearest', 'gw-rh', 1),
    ('2x66x132', '1023/0', 'bggr', 'bilinear', 'ww-gw', 0),
    ('3x34x68', '65535/0', 'rggb', 'laplacian', 'wb-gw-gamma-rh', 1),
    ('8x32x64', '16383/512', 'grbg', 'nearest', 'ww-gamma-gw-gtm', 0),
]
WALK = 8

# ---------------------------------------------------------------------------------------------------- the tie budget
# E32[kind], measured as serve_space_cases.E32 was: the largest |v32 - v64|, in codes, at that kind of quantisation point
# over every input of CASES and the walk, v32 the reference's own expressions in float32 on the CPU - statistics included:
# numpy.sum on float32, the log in float32, exp as exp2(x log2 e) - every segment started from the float64 run's codes.
# The kinds serve_space_cases.E32 already holds are measured again over THESE cases (a stage behind a scene stage sees
# other values).  TAU = 2 x E32 (conftest.ErrorBudget's factor).  Nothing here is taken from a run of the kernels.
# CONST_E32: the largest relative error of a scene stage's float32 constants against the float64 ones, by stat, over the
# same cases; CONST_TAU = 2 x CONST_E32 bounds the kernels' constants in tests/test_gpu_serve_scene.py.
E32 = {
    'bilinear': 3.30e-05, 'crysis': 2.58e-05, 'filmic': 1.05e-04, 'final/gain3': 2.63e-05, 'final/gamma': 5.91e-04,
    'final/grayworld': 1.40e-03, 'final/gtm_manual': 7.21e-05, 'laplacian': 6.96e-05, 'reinhard': 2.02e-04, 'whiteworld': 2.24e-04,
}
TAU = {k: 2.0 * v for k, v in E32.items()}
CONST_E32 = {
    0: 8.90e-06, 1: 3.17e-06, 2: 4.44e-04,
}
CONST_TAU = {k: 2.0 * v for k, v in CONST_E32.items()}


# ---------------------------------------------------------------------------------------------------- builders (CPU)
def make_scene_params(ops, n, rng):
    """serve_space_cases.make_params for the stages it knows; white-world (N,1): ratio 0, 1 and in between; Reinhard (N,2):
    white_point 0 and 0.005 (below the 0.01 floor) and 1, middle_grey 0.005 (below the floor) and small keys"""
    pick = lambda vals: np.array([vals[i % len(vals)] for i in range(n)], np.float32)
    out = []
    for op in ops:
        if op == GW:
            out.append(None)
        elif op == WW:
            out.append(pick([rng.uniform(), 0.0, 1.0, rng.uniform()])[:, None])
        elif op == RH:
            # keys at the dark end: the float32 sum of logarithms (numpy.sum over H W values) is off by about 2e-6 relative in
            # exp(mean), which costs 255 x 2e-6 codes at the top of the range and nothing near its foot; a key of 0.02 .. 0.06
            # (and 0.005, below the floor) keeps the curve's output under about 40 codes, so the reference's own float32 error -
            # and with it TAU and the share of pixels within TAU of a boundary - stays where TIE_CAP can be met
            out.append(np.stack([pick([rng.uniform(0.3, 1.0), 0.0, 0.005, 1.0]), pick([rng.uniform(0.02, 0.06), 0.03, 0.005, 0.04])], axis=1))
        elif op == WQ:
            # a gentle polynomial (coefficients within +-0.2, constant terms 0.3 .. 0.6): its fp32 cancellation error is multiplied
            # by whatever follows, and a scene stage behind a channel that is nearly 0 throughout is as steep as a stage gets
            p = rng.uniform(0.48, 0.52, size=(n, 30)).astype(np.float32)
            p[:, 9::10] = rng.uniform(0.53, 0.56, size=(n, 3)).astype(np.float32)
            out.append(p)
        else:
            out.append(T.make_params([op], n, rng)[0])
    return out


def reference(case, dtype=np.float64, sync=None, reverse=None, single=False):
    run = lambda bias: SC.serve(case['raw'], case['white'], case['black'], case['phase'], case['demosaic'], case['ops'],
                                case['params'], case['reverse'] if reverse is None else reverse, dtype, sync, bias, TAU)
    return run(0) if single or dtype != np.float64 else SC.worlds(run, TAU)


def _build(row, seed0, what):
    shape, depth, phase, demosaic, pipe, reverse = row
    n, h, w = T._shape(shape)
    white, black = (int(v) for v in depth.split('/'))
    ops = list(PIPES[pipe]) if isinstance(pipe, str) else list(pipe)
    case = dict(n=n, h=h, w=w, white=white, black=black, phase=phase, demosaic=demosaic, ops=ops, reverse=bool(reverse), what=what)
    for attempt in range(8):                                # an input over a cap - frames and blocks - is drawn again (its property alone)
        case['params'] = make_scene_params(ops, n, np.random.default_rng(seed0 + 1 + 100 * attempt))
        case['raw'] = T.make_raw(n, h, w, white, black, seed0 + 100 * attempt)
        case['ref'] = reference(case)
        inner, loose = S.tie_shares(case['ref'], TAU)
        if inner <= S.TIE_CAP and loose <= S.FINAL_CAP:
            case['draws'] = attempt + 1
            return case
    raise AssertionError('%s: no input under the caps in 8 draws (inner %.3e, +-1 bytes %.3e)' % (what, inner, loose))


def gw_behind_codes(ops):
    """does a gray-world stage follow a stage that leaves 8-bit codes (a stencil demosaic counts: any demosaic kind may be drawn)"""
    last_codes = True
    for op in ops:
        if op == GW and last_codes:
            return True
        if op != OP_SKIP:
            last_codes = op in (CR, FI, WW, RH)
    return False


@functools.lru_cache(maxsize=None)
def sweep_case(index):
    return _build(CASES[index], 17000 + 13 * index, 'case %d: %s %s %s %s %s reverse %d' % ((index,) + CASES[index]))


@functools.lru_cache(maxsize=None)
def walk_case(seed):
    """one step of the seeded walk over the same axes: a random prefix, one or two scene stages, a random tail"""
    rng = np.random.default_rng(19100 + seed)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    pool = [WB, GA, GT, G3, OP_SKIP, CR, FI]
    ops = [pick(pool) for _ in range(int(rng.integers(0, 3)))] + [pick(SC.SCENE)]
    ops += [pick(pool) for _ in range(int(rng.integers(0, 2)))]
    if rng.random() < 0.5:
        ops += [pick(SC.SCENE)] + [pick([GA, GT, OP_SKIP]) for _ in range(int(rng.integers(0, 2)))]
    # gray-world right behind a stage that leaves codes has gain 1 on a constant image and so puts every byte of it on a boundary
    # of the final truncation: such a list meets the shapes without the constant image (N <= 2) only, as in the table
    shapes = [SHAPES[0], SHAPES[4]] if gw_behind_codes(ops) else SHAPES[:3] + SHAPES[4:]
    row = (pick(shapes), pick(DEPTHS), pick(list(S.SITES)), pick(list(S.DEMOSAIC)), ops, int(rng.integers(0, 2)))
    return _build(row, 19500 + 17 * seed, 'walk %d: %s %s %s %s %s reverse %d' % ((seed,) + row))


def kernel_stages(case, consts):
    """the case's stage list as the C ABI takes it: (ops, blocks) with each scene stage's op code and ``consts[i]`` in the
    place of its block (None while the stage's statistics have not been taken)"""
    ops, blocks, s = [], [], 0
    for op, par in zip(case['ops'], case['params']):
        if op in SC.SCENE:
            ops.append(SC.SCENE_OP[op])
            blocks.append(consts[s] if s < len(consts) else None)
            s += 1
        else:
            ops.append(op)
            blocks.append(par)
    return ops, blocks
