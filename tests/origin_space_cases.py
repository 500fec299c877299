"""The argument space of the five classical Origin entry points (risp_origin.hip) as a table: plain CPU code, imported
by tests/test_origin_reference_cpu.py (coverage, tie budget, the yardstick E32) and tests/test_gpu_origin_space.py.

A case is one call: an entry point, a shape, its sizes and parameters, an input family and a scale magnitude (1: the
plugin boundary, samples in 0..255; 255: the fused pipeline, samples in [0,1] - the input is divided by 255 first).  It
runs in the code form (out_div > 0) and the raw form (out_div < 0), each in every alignment form: aligned (the 4-pixel
kernels where W % 4 == 0), and the same call with the output, and separately the input, moved by one float (the
general kernels).  risp_origin_tonemap refuses a misaligned pointer, so its cases have the aligned form only.

judge() is THE rule: the GPU test applies it to what the kernels stored, the CPU test to the float32 restatement (which
must pass) and to wrong variants of the OPSPEC (which must fail).
"""
import os

import numpy as np
import torch

import isp_oracle as O
import origin_reference as R

TIE_CAP = 2e-3                   # the share of the codes of one case that may differ (test_gpu_fused_segment.TIE_CAP)
# (sigma_color, sigma_space): SIGMAS of test_gpu_fused_segment.py (restated: that module is marked gpu as a whole)
SIGMAS = [(1.0, 1.0), (100.0, 100.0), (1.0, 100.0), (100.0, 1.0), (0.05, 0.05), (0.05, 100.0)]
DECAYS = [1.0, 8.0, 50.5, 100.0]
SCALES = (1.0, 255.0)
FUZZ = int(os.environ.get('RISP_TEST_SEEDS', '8'))                # soak runs: RISP_TEST_SEEDS=64

# ---------------------------------------------------------------------------------------------------- the tie budget
# E32[family][size]: the largest |float32 restatement - float64 restatement| in codes over every input of the tables
# below, both scale magnitudes, measured through the raw store form (fp32 value * fp32(1 / |out_div|)).  Measured by
# tests/test_origin_reference_cpu.py::test_e32_is_what_the_tables_measure on the CPU - never from a kernel - which
# re-measures them (25 % either way for another CPU's exp and summation order).  TAU = 2 x E32: the factor of
# conftest.ErrorBudget, as in the fused-segment suite - the HIP path may cost at most twice what fp32 arithmetic costs
# the restatement itself.  (The constants are the measured values rounded up in the third digit.)
E32 = {
    'bilinear': {0: 3.05e-5},
    'laplacian': {0: 7.10e-5},
    'bilateral': {1: 1.53e-5, 3: 7.71e-5, 5: 8.22e-5, 7: 1.263e-4, 9: 1.242e-4, 11: 2.208e-4, 13: 1.849e-4, 15: 2.129e-4,
                  17: 1.344e-4},
    'fastnlm': {(1, 1): 3.04e-5, (1, 3): 4.00e-5, (1, 5): 5.27e-5, (3, 1): 2.93e-5, (3, 3): 5.63e-5, (3, 5): 8.63e-5,
                (3, 17): 2.112e-4, (5, 1): 3.04e-5, (5, 3): 8.06e-5, (5, 5): 9.44e-5, (7, 7): 1.553e-4, (9, 9): 2.080e-4,
                (17, 3): 4.96e-5, (17, 17): 2.119e-4},
    'reinhard': {0: 1.332e-4}, 'crysis': {0: 3.19e-5}, 'filmic': {0: 1.057e-4}, 'whiteworld': {0: 5.25e-5},
}
E32_FACTOR = 2.0
# at |out_div| = 255 the raw form stores fl(v * fl(1 / 255)): two roundings of 2^-24 relative each, so 255 x the stored
# value is v (1 + d), |d| <= 2^-23 + 2^-48 - at most 255 x 1.1921e-7 = 3.04e-5 codes from the kernel's own v inside the
# 8-bit range.  Within that distance of a rounding boundary the code form cannot be re-derived from the raw form.
RAW_REDERIVE = {1.0: 0.0, 255.0: 3.1e-5}


def raw_error(got, ref):
    """|got - ref| in codes; for a value beyond the 8-bit range (the tone curves with a white point of 0 and white-world
    with a floored channel maximum reach 1e7 codes, all of it clipped) relative to that value's own size: one code at
    255, |ref| / 255 codes beyond.  The yardstick E32 and the GPU rule measure with this same function."""
    return (got - ref).abs() / (ref.abs() / 255.0).clamp_min(1.0)


def tau(family, size):
    return E32_FACTOR * E32[family][size]


# ---------------------------------------------------------------------------------------------------- shapes
def _smallest(radius):
    """the two smallest shapes the guards H, W > radius admit: square, and with the next multiple of 4 above the radius"""
    return [(1, radius + 1, radius + 1), (1, radius + 1, 4 * (radius // 4 + 1))]


STENCIL_SHAPES = [(1, 2, 4), (2, 5, 7), (1, 9, 17), (3, 6, 12), (1, 15, 20), (1, 16, 64), (1, 34, 132), (2, 33, 45),
                  (2, 300, 4)]
DEMOSAIC_SHAPES = [(1, 4, 4), (1, 4, 6), (2, 6, 10), (1, 34, 50), (1, 34, 132), (1, 16, 64), (2, 300, 4)]
# 1x1x4: one vector; 1x20x64: 320 vectors, six of the eight log-luminance shares empty; 2x260x256: 16640 vectors per
# plane, more than 64 x 256 - the stride loop of tonemap_kernel makes a second trip
TONE_SHAPES = [(1, 1, 4), (3, 2, 6), (1, 9, 20), (1, 20, 64), (1, 34, 132), (2, 260, 256)]
INPUTS = ('uniform', 'wide', 'constant', 'step', 'synthetic')

# ---------------------------------------------------------------------------------------------------- the tables
# bilateral: (shape, per-image windows (cycled), max_window, input, first sigma pair)
BILATERAL = []
for _k in range(1, 18, 2):
    for _j, _s in enumerate(_smallest(_k // 2)):
        BILATERAL.append((_s, [_k], _k, INPUTS[(_k // 2 + _j) % 2], _k // 2 + _j))
BILATERAL += [
    ((1, 2, 4), [3], 3, 'uniform', 0), ((2, 5, 7), [5, 3], 5, 'wide', 1), ((1, 9, 17), [17], 17, 'synthetic', 2),
    ((3, 6, 12), [3, 1, 5], 5, 'uniform', 3), ((3, 9, 12), [17, 3, 9], 17, 'wide', 4), ((3, 9, 13), [17, 3, 9], 17, 'uniform', 5),
    ((1, 15, 20), [13], 13, 'wide', 0), ((1, 15, 20), [15], 15, 'step', 1), ((1, 16, 64), [3], 3, 'synthetic', 2),
    ((1, 16, 64), [11], 11, 'uniform', 3), ((1, 34, 132), [5], 5, 'wide', 4), ((1, 34, 132), [3], 7, 'uniform', 5),
    ((2, 33, 45), [7, 9], 9, 'synthetic', 0), ((2, 33, 45), [3], 3, 'constant', 1), ((2, 300, 4), [3], 3, 'step', 2),
    ((2, 300, 4), [1], 1, 'uniform', 3), ((2, 5, 7), [3], 7, 'uniform', 4), ((1, 34, 132), [3], 3, 'constant', 5),
    ((3, 6, 12), [5], 5, 'step', 0),
]
# median: (shape, size, input)
MEDIAN = []
for _k in range(1, 18, 2):
    for _j, _s in enumerate(_smallest(_k // 2)):
        MEDIAN.append((_s, _k, INPUTS[(_k // 2 + _j) % 2]))
MEDIAN += [
    ((1, 2, 4), 3, 'uniform'), ((2, 5, 7), 5, 'wide'), ((1, 9, 17), 17, 'synthetic'), ((3, 6, 12), 7, 'uniform'),
    ((1, 15, 20), 15, 'wide'), ((1, 15, 20), 13, 'half'), ((1, 16, 64), 9, 'synthetic'), ((1, 16, 64), 3, 'half'),
    ((1, 34, 132), 5, 'wide'), ((1, 34, 132), 11, 'uniform'), ((2, 33, 45), 3, 'step'), ((2, 33, 45), 7, 'half'),
    ((2, 300, 4), 3, 'wide'), ((2, 300, 4), 7, 'constant'), ((1, 16, 64), 5, 'half'), ((1, 34, 132), 3, 'synthetic'),
]
# fastnlm: (shape, per-image (block, search) (cycled), input, first decay).  max_block / max_search: the maxima
PAIRS = [(1, 1), (5, 1), (1, 5), (3, 3), (3, 5), (5, 3), (5, 5), (7, 7), (9, 9), (3, 17), (17, 3), (17, 17)]
FASTNLM = []
for _i, _p in enumerate(PAIRS):
    for _j, _s in enumerate(_smallest(_p[0] // 2 + _p[1] // 2)):
        FASTNLM.append((_s, [_p], INPUTS[(_i + _j) % 2], _i + _j))
FASTNLM += [
    ((1, 1, 1), [(1, 1)], 'uniform', 0), ((1, 2, 4), [(1, 3)], 'wide', 1), ((2, 5, 7), [(3, 3), (1, 3)], 'uniform', 2),
    ((3, 6, 12), [(3, 3), (1, 3), (3, 1)], 'wide', 3),         # the fast and the general branch in one fastnlm4<true> launch
    ((3, 6, 13), [(3, 3), (1, 3), (3, 1)], 'uniform', 0),
    ((1, 9, 17), [(5, 5)], 'synthetic', 1), ((1, 15, 20), [(9, 9)], 'wide', 2), ((1, 15, 20), [(7, 7)], 'step', 3),
    ((1, 16, 64), [(3, 3)], 'synthetic', 0), ((1, 16, 64), [(1, 5)], 'uniform', 1), ((1, 34, 132), [(5, 1)], 'wide', 2),
    ((1, 34, 132), [(3, 5)], 'uniform', 3), ((1, 34, 132), [(1, 1)], 'wide', 0),
    ((2, 33, 45), [(5, 3), (3, 5)], 'synthetic', 1),           # the maxima come from different images: R = 4, used by none
    ((2, 16, 64), [(5, 3), (3, 5)], 'uniform', 2),
    ((2, 33, 45), [(3, 3)], 'constant', 3), ((2, 300, 4), [(3, 3)], 'step', 0), ((2, 300, 4), [(5, 3)], 'uniform', 1),
    ((1, 34, 132), [(3, 3)], 'constant', 2), ((1, 15, 20), [(3, 17)], 'uniform', 3), ((1, 17, 20), [(17, 17)], 'constant', 0),
]
# demosaic: (shape, laplacian, input)
DEMOSAIC = []
for _i, _s in enumerate(DEMOSAIC_SHAPES):
    for _lap in (0, 1):
        DEMOSAIC.append((_s, _lap, (INPUTS + ('codes',))[(_i + 3 * _lap) % 6]))
DEMOSAIC += [((1, 4, 4), 0, 'codes'), ((1, 4, 6), 0, 'codes'), ((1, 34, 132), 0, 'codes'), ((1, 34, 50), 0, 'codes'),
             ((2, 6, 10), 1, 'constant'), ((1, 16, 64), 1, 'codes'), ((2, 300, 4), 0, 'codes')]
# tone curves and white-world: (shape, mode, input, first parameter corner)
TONE_PARAMS = {                  # (a, b) as risp_origin_tonemap takes them: the corners and the middle of each range
    R.REINHARD: [(wp, mg) for wp in (0.0, 0.5, 1.0) for mg in (0.0, 0.5, 1.0)],          # (white_point, middle_grey)
    R.CRYSIS: [(la, None) for la in (0.0, 0.5, 1.0)],                                    # lum_adapted
    R.FILMIC: [(wp, eb) for wp in (0.0, 0.5, 1.0) for eb in (1.0, 5.5, 10.0)],           # (white_point, exposure_bias)
    R.WHITEWORLD: [(r, None) for r in (0.0, 0.5, 1.0)],                                  # ratio
}
MODE_NAMES = {R.REINHARD: 'reinhard', R.CRYSIS: 'crysis', R.FILMIC: 'filmic', R.WHITEWORLD: 'whiteworld'}
TONEMAP = []
for _m in range(4):
    for _i, _s in enumerate(TONE_SHAPES):
        TONEMAP.append((_s, _m, INPUTS[(_i + _m) % 5], 2 * _i + _m))
    # every corner of the mode's parameters once more on a small shape (per-image corners: N = their number)
    TONEMAP.append(((len(TONE_PARAMS[_m]), 4, 8), _m, 'wide', 0))
    TONEMAP.append(((len(TONE_PARAMS[_m]), 4, 8), _m, 'uniform', 0))
TONEMAP += [((1, 9, 20), R.REINHARD, 'zero', 4), ((2, 4, 8), R.WHITEWORLD, 'zero', 1), ((3, 9, 20), R.WHITEWORLD, 'negchan', 0),
            ((1, 34, 132), R.WHITEWORLD, 'negchan', 2)]
TABLES = {'bilateral': BILATERAL, 'median': MEDIAN, 'fastnlm': FASTNLM, 'demosaic': DEMOSAIC, 'tonemap': TONEMAP}
ENTRIES = tuple(TABLES)


# ---------------------------------------------------------------------------------------------------- inputs
def make_input(kind, c, n, h, w, seed):
    """fp32 (N,C,H,W) in the 0..255 domain"""
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == 'uniform':
        return torch.from_numpy(rng.uniform(0.0, 255.0, size=(n, c, h, w)).astype(np.float32))
    if kind == 'wide':                       # clips on both sides of the 8-bit range
        return torch.from_numpy(rng.uniform(-40.0, 300.0, size=(n, c, h, w)).astype(np.float32))
    if kind == 'codes':                      # integer codes
        return torch.from_numpy(rng.integers(0, 256, size=(n, c, h, w)).astype(np.float32))
    if kind == 'half':                       # exactly on the rounding boundaries k + 0.5 (and a few codes)
        v = rng.integers(0, 255, size=(n, c, h, w)).astype(np.float32) + 0.5
        return torch.from_numpy(np.where(rng.random((n, c, h, w)) < 0.2, v - 0.5, v).astype(np.float32))
    if kind == 'zero':
        return torch.zeros(n, c, h, w)
    if kind == 'negchan':                    # channel i % C of image i is negative everywhere: white-world's floor
        x = rng.uniform(0.0, 255.0, size=(n, c, h, w)).astype(np.float32)
        for i in range(n):
            x[i, i % c] = -1.0 - x[i, i % c] / 8.0
        return torch.from_numpy(x)
    if kind == 'synthetic':
        bay, gt = O.synthetic_raw(n, max(h + h % 2, 16), max(w + w % 2, 16), seed=seed)
        return ((bay if c == 1 else gt)[:, :, :h, :w] * 255.0).contiguous()
    # constant / step: flat integer codes, per image and channel.  The step is 208 = 13 x 16 codes: every coefficient of
    # either demosaic is a multiple of 1 / 16, so no demosaiced step lands on a half-integer
    lo = rng.integers(0, 48, size=(n, c))
    x = torch.empty(n, c, h, w)
    for i in range(n):
        for ch in range(c):
            x[i, ch] = float(lo[i, ch])
            if kind == 'step':               # two flat halves
                if i % 2 and h >= 2:
                    x[i, ch, h // 2:] = float(lo[i, ch] + 208)
                else:
                    x[i, ch, :, w // 2:] = float(lo[i, ch] + 208)
    return x


def _handed_over(x255, si):
    """what the caller passes at this scale magnitude: the 0..255 image, divided by 255 first for in_scale 255"""
    return x255 if si == 1.0 else (x255 / 255.0)


def _off_half(x, si, rng):
    """median inputs: no x * in_scale within 1e-3 codes of a half-integer (the fp32 product is within 1.5e-5 codes of
    the float64 one - half an ulp of 255): such samples are drawn again"""
    x = x.clone()
    for _ in range(64):
        v = x.double() * si
        bad = ((v - torch.floor(v) - 0.5).abs() < 1e-3)
        if not bad.any():
            return x
        new = torch.from_numpy(rng.uniform(0.0, 255.0, size=int(bad.sum())).astype(np.float32))
        x[bad] = new if si == 1.0 else new / 255.0
    raise AssertionError('median input: samples stay on a half-integer')


# ---------------------------------------------------------------------------------------------------- cases
def _cycle(seq, n, start=0):
    return [seq[(start + i) % len(seq)] for i in range(n)]


def build(entry, row, si, seed, what=None):
    """one table row at one scale magnitude -> the case dict (x: what the caller hands over, fp32)"""
    shape = row[0]
    n, h, w = shape
    case = dict(entry=entry, shape=shape, si=si, seed=seed, row=row)
    kind = row[2] if entry in ('median', 'fastnlm', 'demosaic', 'tonemap') else row[3]
    case['input'] = kind
    x = _handed_over(make_input(kind, 1 if entry == 'demosaic' else 3, n, h, w, seed), si)
    if entry == 'bilateral':
        _, wins, mw, _, s0 = row
        sig = _cycle(SIGMAS, n, s0)
        case.update(window=torch.tensor(_cycle(wins, n), dtype=torch.int32), max_window=mw,
                    sc=torch.tensor([s[0] for s in sig]), ss=torch.tensor([s[1] for s in sig]))
        case['keys'] = [('bilateral', int(k)) for k in case['window']]
    elif entry == 'median':
        case['size'] = row[1]
        if kind == 'half':
            assert si == 1.0
        else:
            x = _off_half(x, si, np.random.Generator(np.random.PCG64(seed + 77)))
        case['keys'] = [('median', row[1])] * n
    elif entry == 'fastnlm':
        _, pairs, _, d0 = row
        pairs = _cycle(pairs, n)
        case.update(block=torch.tensor([p[0] for p in pairs], dtype=torch.int32),
                    search=torch.tensor([p[1] for p in pairs], dtype=torch.int32),
                    decay=torch.tensor(_cycle(DECAYS, n, d0)), max_block=max(p[0] for p in pairs),
                    max_search=max(p[1] for p in pairs))
        case['keys'] = [('fastnlm', p) for p in pairs]
        case['identity'] = all(p[1] == 1 for p in pairs)        # search 1: the output is the input
    elif entry == 'demosaic':
        case['laplacian'] = row[1]
        case['keys'] = [('laplacian' if row[1] else 'bilinear', 0)] * n
        # integer codes at in_scale 1: every expression of either demosaic is exact in fp32 (integers and halves below
        # 2^24, divisions by 2, 4, 8) and half-integers occur: no tie excuse, round-half-up is pinned
        case['exact'] = kind == 'codes' and si == 1.0
    else:
        _, mode, _, p0 = row
        par = _cycle(TONE_PARAMS[mode], n, p0)
        case.update(mode=mode, a=torch.tensor([p[0] for p in par]),
                    b=torch.tensor([p[1] for p in par]) if par[0][1] is not None else None)
        case['keys'] = [(MODE_NAMES[mode], 0)] * n
    case['x'] = x.contiguous()
    case['flat'] = kind == 'zero' or (kind == 'constant' and entry != 'tonemap')   # constant in, the same constant out
    case['what'] = what or '%s %s %s scale %g' % (entry, 'x'.join(map(str, shape)), '/'.join(map(str, row[1:])), si)
    return case


def table_case(entry, index, si):
    """row ``index`` of an entry point's table.  An input that puts more than TIE_CAP of its codes within TAU of a
    rounding boundary is drawn again, up to 8 times (a property of the input and the float64 restatement alone).
    The deliberate ties - the integer-code demosaic and the medians - are exempt: they must match exactly."""
    row = TABLES[entry][index]
    if row[2 if entry != 'bilateral' else 3] == 'half' and si != 1.0:
        return None                           # the k + 0.5 family exists at in_scale 1 only
    base = 1000 * (1 + ENTRIES.index(entry)) + 8 * index + (0 if si == 1.0 else 500000)
    for attempt in range(8):
        case = build(entry, row, si, base + attempt)
        if entry == 'median' or case.get('exact') or near_tie_share(case) <= TIE_CAP:
            return case
    raise AssertionError('%s: no input under the tie cap in 8 draws' % case['what'])


def all_cases(entry):
    """[(index, si)] of every table case of an entry point: rows alternate between the scale magnitudes, and the first
    rows run at both"""
    out = []
    for i, row in enumerate(TABLES[entry]):
        half = row[2 if entry != 'bilateral' else 3] == 'half'
        exact_codes = entry == 'demosaic' and row[2] == 'codes'
        ident = entry == 'fastnlm' and all(p[1] == 1 for p in row[1])
        sis = (1.0,) if half or exact_codes else ((1.0, 255.0) if i < 4 or ident else (SCALES[i % 2],))
        out += [(i, si) for si in sis]
    return out


def case_id(entry, index, si):
    row = TABLES[entry][index]
    return ('%s-%d-%s-%s-s%g' % (entry, index, 'x'.join(map(str, row[0])), '_'.join(str(v) for v in row[1:]), si)).replace(
        ' ', '').replace('/', '_')


def walk_case(seed):
    """one step of the seeded walk over the same axes: any entry point, shapes up to 2 x 60 x 80 of any parity, sizes
    up to 9 (bilateral, median) and R <= 4 (fastnlm), parameters anywhere in their ranges"""
    rng = np.random.default_rng(9100 + seed)
    entry = ENTRIES[seed % len(ENTRIES)]
    si = SCALES[int(rng.integers(0, 2))]
    n = int(rng.integers(1, 3))
    kind = INPUTS[int(rng.integers(0, len(INPUTS)))]
    if entry == 'bilateral':
        wins = [int(k) for k in rng.choice([1, 3, 5, 7, 9], size=n)]
        mw = max(wins) if rng.random() < 0.7 else 9
        h, w = int(rng.integers(mw // 2 + 1, 61)), int(rng.integers(mw // 2 + 1, 81))
        row = ((n, h, w), wins, mw, kind, int(rng.integers(0, 6)))
    elif entry == 'median':
        k = int(rng.choice([1, 3, 5, 7, 9, 11]))
        row = ((n, int(rng.integers(k // 2 + 1, 61)), int(rng.integers(k // 2 + 1, 81))), k, kind)
    elif entry == 'fastnlm':
        pairs = [[(1, 1), (1, 3), (3, 1), (3, 3), (3, 5), (5, 3), (5, 5), (1, 5), (5, 1)][int(j)] for j in rng.integers(0, 9, size=n)]
        r = max(p[0] for p in pairs) // 2 + max(p[1] for p in pairs) // 2
        row = ((n, int(rng.integers(r + 1, 61)), int(rng.integers(r + 1, 81))), pairs, kind, int(rng.integers(0, 4)))
    elif entry == 'demosaic':
        row = ((n, 2 * int(rng.integers(2, 31)), 2 * int(rng.integers(2, 41))), int(rng.integers(0, 2)), kind)
    else:
        h, w = int(rng.integers(1, 61)), 4 * int(rng.integers(1, 21))
        mode = int(rng.integers(0, 4))
        row = ((n, h, w), mode, kind, int(rng.integers(0, 9)))
    if rng.random() < 0.5 and entry in ('bilateral', 'median', 'fastnlm'):
        row = ((row[0][0], row[0][1], 4 * ((row[0][2] + 3) // 4)),) + tuple(row[1:])   # half of the steps: the 4-pixel forms
    for attempt in range(8):
        case = build(entry, row, si, 70000 + 8 * seed + attempt, what='walk %d: %s %r scale %g' % (seed, entry, row, si))
        if entry == 'tonemap' and rng.random() < 0.7:        # parameters anywhere in their ranges
            lo, hi = (1.0, 10.0) if case['mode'] == R.FILMIC else (0.0, 1.0)
            case['a'] = torch.from_numpy(rng.uniform(0.0, 1.0, size=n).astype(np.float32))
            if case['b'] is not None:
                case['b'] = torch.from_numpy(rng.uniform(lo, hi, size=n).astype(np.float32))
        if entry == 'median' or near_tie_share(case) <= TIE_CAP:
            return case
    raise AssertionError('%s: no input under the tie cap in 8 draws' % case['what'])


# ---------------------------------------------------------------------------------------------------- the restatement
def reference(case, dtype=R.F64, **variant):
    """the restatement's value in front of the clip-and-round, in codes (the median: its codes)"""
    v = R.scaled(case['x'], case['si'], dtype)
    e = case['entry']
    if e == 'bilateral':
        return R.bilateral(v, case['window'], case['sc'], case['ss'], dtype, **variant)
    if e == 'median':
        return R.median(v, case['size'], dtype, **variant)
    if e == 'fastnlm':
        return R.fastnlm(v, case['block'], case['search'], case['decay'], dtype, **variant)
    if e == 'demosaic':
        return R.demosaic(v, case['laplacian'], dtype, **variant)
    if case['mode'] == R.WHITEWORLD:
        return R.whiteworld(v, case['a'], dtype, **variant)
    return R.tonemap(v, case['mode'], case['a'], case['b'], dtype, **variant)


_REF = {}


def ref64(case):
    """computed once per case and shared (never modified)"""
    key = case['what'] + '#%d' % case['seed']
    if key not in _REF:
        if len(_REF) > 64:
            _REF.clear()
        _REF[key] = reference(case)
    return _REF[key]


def case_tau(case):
    if case['entry'] == 'median':
        return torch.zeros(len(case['keys']), 1, 1, 1, dtype=torch.float64)
    return torch.tensor([tau(*k) for k in case['keys']], dtype=torch.float64).view(-1, 1, 1, 1)


def near_tie_share(case):
    return (R.tie_distance(ref64(case)) <= case_tau(case)).double().mean().item()


# ---------------------------------------------------------------------------------------------------- dispatch (coverage only)
def kernel_of(case, aligned):
    """Restates the dispatch of the five entry points - form, template argument, fast branch - to COUNT which kernel
    instantiations the tables reach.  It decides no verdict."""
    e, w = case['entry'], case['shape'][2]
    four = aligned and w % 4 == 0
    if e == 'demosaic':
        return ('demosaic4<%d>' if four else 'origin_demosaic<%d>') % case['laplacian']
    if e == 'bilateral':
        r = case['max_window'] // 2
        return 'bilateral4<%d>' % (r if r in (1, 2) else 0) if four else 'bilateral'
    if e == 'median':
        k = case['size']
        if not four or k == 1:
            return 'median'
        return 'median3x4' if k == 3 else 'median4<%d>' % k
    if e == 'fastnlm':
        r = case['max_block'] // 2 + case['max_search'] // 2
        if not four:
            return 'fastnlm'
        if r != 2:
            return 'fastnlm4<false>'
        fast = [bool(b // 2 == 1 and s // 2 == 1) for b, s in zip(case['block'].tolist(), case['search'].tolist())]
        return 'fastnlm4<true>' + ('/fast' if all(fast) else '/mixed' if any(fast) else '/general')
    return 'tonemap<%d>' % case['mode']


KERNELS = (['bilateral4<0>', 'bilateral4<1>', 'bilateral4<2>', 'median3x4'] + ['median4<%d>' % k for k in range(5, 18, 2)] +
           ['fastnlm4<true>', 'fastnlm4<false>', 'demosaic4<0>', 'demosaic4<1>', 'origin_demosaic<0>', 'origin_demosaic<1>',
            'bilateral', 'median', 'fastnlm'] + ['tonemap<%d>' % m for m in range(4)])


# ---------------------------------------------------------------------------------------------------- the rule
def judge(case, raw_stored, code_stored, exact_code=None):
    """Holds what one form of a case stored to the float64 restatement.  raw_stored / code_stored: fp32 CPU tensors as
    the raw form (out_div = -si) and the code form (out_div = +si) store them.  -> (failures, figures)."""
    what, od = case['what'], case['si']
    ref = ref64(case)
    rinv = float(R.rinv(od))
    n = ref.shape[0]
    failed, fig = [], dict(raw_err=0.0, ratio=0.0, share=0.0, images=[(0.0, 0.0, 0.0)] * n)      # images: the three per image

    def check(ok, message, *args):
        if not ok:
            failed.append('%s: ' % what + (message % args if args else message))

    check(not torch.isnan(raw_stored).any().item() and not torch.isnan(code_stored).any().item(), 'elements left unwritten')
    # ---- the code form holds fp32(code) * fp32(1 / out_div), to the bit
    k = torch.round(code_stored.double() * od)
    held = torch.equal(R.stored_code(k, od), code_stored) and k.min().item() >= 0 and k.max().item() <= 255
    check(held, 'the code form does not store fp32(code) * fp32(1 / %g) (%d elements)', od,
          int((R.stored_code(k, od) != code_stored).sum()))
    if case['entry'] == 'median':
        check(torch.equal(k, ref), 'median: %d codes differ from the restatement (max %g)', int((k != ref).sum()),
              (k - ref).abs().max().item())
        check(torch.equal(raw_stored, code_stored), 'median: the raw form differs from the code form')
        return failed, fig
    # ---- raw form against float64
    got = raw_stored.double() * od
    t = case_tau(case)
    err = raw_error(got, ref)
    fig['raw_err'] = err.max().item()
    fig['ratio'] = (err / t.clamp_min(1e-300)).max().item() if (t > 0).all() else (0.0 if err.max().item() == 0 else float('inf'))
    over = err > t
    check(not over.any().item(), '[raw] %d values beyond TAU: largest error %.3e codes (TAU %s)', int(over.sum()),
          err.max().item(), sorted(set(t.flatten().tolist())))
    if case.get('identity'):                  # search 1: the output IS the input times in_scale, then the store scale
        want = R.stored_raw(R.scaled(case['x'], case['si'], R.F32), od)
        check(torch.equal(raw_stored, want), '[raw] identity: %d values are not the input', int((raw_stored != want).sum()))
    # ---- code form against float64
    d = (k - R.code(ref)).abs()
    differ = d > 0
    fig['share'] = differ.double().mean().item()
    ratio = err / t.clamp_min(1e-300)
    fig['images'] = [(err[i].max().item(), ratio[i].max().item(), differ[i].double().mean().item()) for i in range(n)]
    check(d.max().item() <= 1, '[codes] a code differs by %g', d.max().item())
    if case.get('exact') or case.get('identity') or case.get('flat'):
        check(not differ.any().item(), '[codes] %d codes differ where the case admits no tie excuse', int(differ.sum()))
    dist = R.tie_distance(ref)
    away = differ & (dist > t)
    check(not away.any().item(), '[codes] %d codes differ away from a rounding tie (tie distance up to %.3e, TAU %s)',
          int(away.sum()), dist[away].max().item() if away.any() else 0.0, sorted(set(t.flatten().tolist())))
    check(fig['share'] <= TIE_CAP, '[codes] %.4f%% of the codes differ', 100 * fig['share'])
    # ---- the code form is the rounding of the kernel's OWN raw form
    own = R.code(got)
    undecided = R.tie_distance(got) <= RAW_REDERIVE[od]
    wrong = (own != k) & ~undecided
    check(not wrong.any().item(), '[codes] %d codes are not floor(clamp(raw form, 0, 255) + 0.5)', int(wrong.sum()))
    return failed, fig


# ---------------------------------------------------------------------------------------------------- refusals
# One row per RISP_CHECK_ARG line of the five entry points (several per line where the line holds several rules) and per
# _check_odd / _check_bgr refusal of the wrappers.  ('abi', entry, overrides, needle) calls the C ABI on a valid 1x3x16x16
# call with the named arguments replaced; ('wrapper', ...) calls reconfigisp_amd.functional.  Each must raise before a
# launch: the NaN-filled guarded output stays untouched.  (risp_origin_fastnlm's second line - the LDS tile of R <= 16
# is 30 KB - cannot be reached through the first.)
REFUSED = [
    ('abi', 'demosaic', dict(H=2), 'risp_origin_demosaic'), ('abi', 'demosaic', dict(W=2), 'risp_origin_demosaic'),
    ('abi', 'demosaic', dict(H=15), 'risp_origin_demosaic'), ('abi', 'demosaic', dict(W=6, H=5), 'risp_origin_demosaic'),
    ('abi', 'demosaic', dict(N=0), 'risp_origin_demosaic'), ('abi', 'demosaic', dict(N=65536), 'risp_origin_demosaic'),
    ('abi', 'demosaic', dict(x=None), 'risp_origin_demosaic'), ('abi', 'demosaic', dict(y=None), 'risp_origin_demosaic'),
    ('abi', 'bilateral', dict(max_window=4), 'risp_origin_bilateral'), ('abi', 'bilateral', dict(max_window=19), 'risp_origin_bilateral'),
    ('abi', 'bilateral', dict(max_window=0), 'risp_origin_bilateral'), ('abi', 'bilateral', dict(max_window=17, H=8), 'risp_origin_bilateral'),
    ('abi', 'bilateral', dict(max_window=5, W=2), 'risp_origin_bilateral'), ('abi', 'bilateral', dict(window=None), 'risp_origin_bilateral'),
    ('abi', 'bilateral', dict(sc=None), 'risp_origin_bilateral'), ('abi', 'bilateral', dict(ss=None), 'risp_origin_bilateral'),
    ('abi', 'bilateral', dict(N=0), 'risp_origin_bilateral'),
    ('abi', 'median', dict(size=2), 'risp_origin_median'), ('abi', 'median', dict(size=19), 'risp_origin_median'),
    ('abi', 'median', dict(size=0), 'risp_origin_median'), ('abi', 'median', dict(size=17, W=8), 'risp_origin_median'),
    ('abi', 'median', dict(size=3, H=1), 'risp_origin_median'), ('abi', 'median', dict(x=None), 'risp_origin_median'),
    ('abi', 'median', dict(N=65536), 'risp_origin_median'),
    ('abi', 'fastnlm', dict(max_block=19), 'risp_origin_fastnlm'), ('abi', 'fastnlm', dict(max_search=19), 'risp_origin_fastnlm'),
    ('abi', 'fastnlm', dict(max_block=0), 'risp_origin_fastnlm'), ('abi', 'fastnlm', dict(max_search=0), 'risp_origin_fastnlm'),
    ('abi', 'fastnlm', dict(max_block=17, max_search=17), 'risp_origin_fastnlm'),       # R = 16 on 16 x 16
    ('abi', 'fastnlm', dict(max_block=5, max_search=5, H=4), 'risp_origin_fastnlm'), ('abi', 'fastnlm', dict(block=None), 'risp_origin_fastnlm'),
    ('abi', 'fastnlm', dict(search=None), 'risp_origin_fastnlm'), ('abi', 'fastnlm', dict(decay=None), 'risp_origin_fastnlm'),
    ('abi', 'tonemap', dict(HW=254), 'risp_origin_tonemap'), ('abi', 'tonemap', dict(HW=0), 'risp_origin_tonemap'),
    ('abi', 'tonemap', dict(mode=4), 'risp_origin_tonemap'), ('abi', 'tonemap', dict(mode=-1), 'risp_origin_tonemap'),
    ('abi', 'tonemap', dict(a=None), 'risp_origin_tonemap'), ('abi', 'tonemap', dict(scratch=None), 'risp_origin_tonemap'),
    ('abi', 'tonemap', dict(mode=0, b=None), 'second parameter'), ('abi', 'tonemap', dict(mode=2, b=None), 'second parameter'),
    ('abi', 'tonemap', dict(mode=3, stats=None), 'channel statistics'),
    ('abi', 'tonemap', dict(x_off=1), 'x must be 16-byte aligned'), ('abi', 'tonemap', dict(y_off=1), 'y must be 16-byte aligned'),
    ('abi', 'tonemap', dict(x_off=2), 'x must be 16-byte aligned'), ('abi', 'tonemap', dict(y_off=3), 'y must be 16-byte aligned'),
    ('wrapper', 'median', dict(size=4), 'odd size'), ('wrapper', 'median', dict(size=19), 'odd size'),
    ('wrapper', 'median', dict(size=0), 'odd size'), ('wrapper', 'bilateral', dict(max_window=6), 'odd size'),
    ('wrapper', 'bilateral', dict(window=19), 'odd size'), ('wrapper', 'fastnlm', dict(max_block=2), 'odd size'),
    ('wrapper', 'fastnlm', dict(max_search=21), 'odd size'), ('wrapper', 'median', dict(shape=(1, 4, 8, 8)), 'BGR'),
    ('wrapper', 'bilateral', dict(shape=(3, 8, 8)), 'BGR'), ('wrapper', 'tonemap', dict(shape=(1, 3, 3, 5)), 'multiple of 4'),
    ('wrapper', 'whiteworld', dict(shape=(1, 3, 1, 6)), 'multiple of 4'), ('wrapper', 'tonemap', dict(shape=(1, 1, 4, 4)), 'BGR'),
    ('wrapper', 'whiteworld', dict(shape=(2, 4, 4)), 'BGR'),
]
