"""``convnets.conv_small`` over its argument space, stated without the GPU: the float32 / float64 restatement of the operation, what
each entry point of the library accepts, and the table of cases tests/test_gpu_conv_small_space.py runs.  Plain torch on the CPU;
checked by tests/test_conv_small_reference_cpu.py.

The operation (include/risp.h, the epilogue in the order the kernels apply it - risp_conv_small.hip::small_reduce_kernel):

    z = conv2d(x, w, padding k // 2)            a forward pack, or conv_transpose2d(x, w[:, :keep], padding k // 2) for the
                                                backward-data pack of a FORWARD weight, SmallConv(transpose=True, keep=...)
    z += bias                                   unless the layer has none (EPI_NOBIAS)
    EPI_SHUFFLE2: y = PixelShuffle(2)(z)        cout 4 g + 2 i + j -> plane g, pixel (2 y + i, 2 x + j); after the ReLU where
                                                risp_conv2d_narrow3 takes RELU | SHUFFLE2 - no other kernel has that pair
    EPI_ADD:   z[:, :add_c] += add              the residual reaches the first add_c couts only
    EPI_RELU:  z = max(z, 0)
    EPI_MASK:  z = z where mask > 0, else 0

``ENTRY_ACCEPTS`` restates the argument checks of the entry points (risp_conv_tapout.hip, risp_conv_toep.hip, risp_conv_narrow3.hip,
risp_conv_small.hip: the RISP_CHECK_ARG lines, and the text of include/risp.h) on a ``launch`` - it knows nothing of ``route_small``.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as TF

RELU, ADD, MASK, SHUFFLE2, NOBIAS = 1, 2, 4, 8, 16               # include/risp.h: RISP_EPI_*
TAPOUT, TOEP, NARROW3, SMALL, SPLIT = ('risp_conv2d_tapout', 'risp_conv2d_toep', 'risp_conv2d_narrow3', 'risp_conv2d_small',
                                       'risp_conv2d_small_split')
BAR = {TAPOUT: 5e-6, TOEP: 5e-6, NARROW3: 2e-6, SMALL: 3e-6, SPLIT: 3e-6}       # max error / max|ref|: the kernels' own files


# ----------------------------------------------------------------------------------------------------------------------------
# what each entry point accepts.  launch: dict(k, cin, cout, n (images of the launch, all members), h, w, epi (with NOBIAS), add_c,
# has_add, has_mask, has_bias, seg_rows (tap-row kernel), groups (the channel split))
def _common(L):
    return L['n'] > 0 and L['h'] > 0 and L['w'] > 0 and L['cin'] > 0 and L['cout'] > 0


def _bias_add(L):
    return (bool(L['epi'] & NOBIAS) or L['has_bias']) and (not (L['epi'] & ADD) or (L['has_add'] and 0 < L['add_c'] <= L['cout']))


def accepts_tapout(L):
    seg = L.get('seg_rows', 0)
    return (_common(L) and L['w'] % 4 == 0 and L['cin'] % 16 == 0 and L['cout'] <= 3 and L['k'] in (5, 9)
            and L['cin'] * L['h'] * L['w'] < 2 ** 30 and L['h'] * L['w'] < 2 ** 24
            and seg >= 0 and (seg % 4 == 0 or seg >= L['h'])              # 0 = the launch's choice; a multiple of 4; or the image kept whole
            and not (L['epi'] & ~(RELU | ADD | NOBIAS)) and _bias_add(L))


def accepts_toep(L):
    return (_common(L) and L['w'] % 4 == 0 and (L['cout'] <= 4 or (L['cout'] <= 12 and L['k'] == 5)) and L['k'] in (5, 9)
            and L['cin'] * L['h'] * L['w'] < 2 ** 30
            and not (L['epi'] & ~(RELU | ADD | NOBIAS | SHUFFLE2))
            and (not (L['epi'] & SHUFFLE2) or (L['cout'] % 4 == 0 and not (L['epi'] & (RELU | ADD)))) and _bias_add(L))


def accepts_narrow3(L):
    return (_common(L) and L['k'] == 3 and 16 <= L['cin'] <= 64 and L['cin'] % 16 == 0 and L['cout'] <= 4
            and not (L['epi'] & ~(RELU | SHUFFLE2 | NOBIAS)) and (not (L['epi'] & SHUFFLE2) or L['cout'] == 4)
            and (bool(L['epi'] & NOBIAS) or L['has_bias'])
            and L['cin'] * L['h'] * L['w'] * 4 < 2 ** 31)                 # one image side through a buffer resource


def accepts_small(L):
    return (_common(L) and L['n'] <= 65535 and L['cout'] <= 12
            and not (L['epi'] & ~(RELU | ADD | MASK | NOBIAS | SHUFFLE2))
            and (not (L['epi'] & SHUFFLE2) or (L['cout'] % 4 == 0 and not (L['epi'] & (RELU | ADD | MASK))))
            and _bias_add(L) and (not (L['epi'] & MASK) or L['has_mask'])
            and L['k'] in ((3, 5, 9) if L['cout'] <= 4 else (3, 5)))


def accepts_small_split(L):
    g = L.get('groups', 1)
    return accepts_small(L) and (g <= 1 or (g <= 16 and L['n'] * g <= 65535))


ENTRY_ACCEPTS = {TAPOUT: accepts_tapout, TOEP: accepts_toep, NARROW3: accepts_narrow3, SMALL: accepts_small, SPLIT: accepts_small_split}


def launch_of(case, **over):
    """the launch a case asks of ``conv_small``, as ``ENTRY_ACCEPTS`` reads it"""
    L = dict(k=case['k'], cin=case['cin'], cout=case['cout'], n=case['n'] * (case['group'] or 1), h=case['h'], w=case['w'],
             epi=case['epi'] | (0 if case['bias'] else NOBIAS), add_c=case['add_c'], has_add=bool(case['epi'] & ADD),
             has_mask=case['mask'], has_bias=case['bias'])
    L.update(over)
    return L


def pack_flags(CN, k, cin, cout, epi, has_add):
    """(has_toep, has_tapout, has_narrow3) as ``conv_small`` hands them to ``route_small``: the packs the layer holds (the public
    ``small_has_*``) whose kernel has the launch's epilogue - no PixelShuffle store on the tap-row kernel, RELU | SHUFFLE2 | NOBIAS
    and no residual on the 3x3 tail's"""
    return (CN.small_has_toep(k, cout), CN.small_has_tapout(k, cin, cout) and not (epi & SHUFFLE2),
            CN.small_has_narrow3(k, cin, cout) and not (epi & ~(RELU | SHUFFLE2 | NOBIAS)) and not has_add)


def routed(case, images=None, split=None):
    """``convnets.route_small`` as ``conv_small`` asks it for a case (under the arithmetic the caller has set)"""
    from reconfigisp_amd import convnets as CN
    epi = case['epi'] | (0 if case['bias'] else NOBIAS)
    has_toep, has_tapout, has_narrow3 = pack_flags(CN, case['k'], case['cin'], case['cout'], epi, bool(epi & ADD))
    images = case['n'] * (case['group'] or 1) if images is None else images
    return CN.route_small(case['k'], case['cin'], case['cout'], case['h'], case['w'], images, case['infer'], case['mask'], has_toep, split,
                          has_tapout, has_narrow3)


def small_groups(cin, n, h, w):
    """risp_conv_small_groups (risp_conv_small.hip): the channel split of the vector kernel on a small training grid"""
    if cin < 32:
        return 1
    tx = (w + 63) // 64
    if tx * ((h + 15) // 16) * n >= 768:
        return 1
    g = min(8, 1024 // max(1, tx * ((h + 31) // 32) * n))
    while g > 1 and cin // g < 8:
        g -= 1
    return max(g, 1)


def chain_groups(k, cin, n):
    """``convnets.small_chain_groups``: a vector-kernel launch that its grid does not split still runs in channel groups of 16 where the
    chain of an output is long (9 x 9 taps x 32 channels and more), whatever the grid and the mode"""
    g = min(8, cin // 16) if k == 9 and cin >= 32 else 1
    return g if n * g <= 65535 else 1


def vector_groups(case):
    """channel groups of a case's launch when the vector kernel serves it"""
    n = case['n'] * (case['group'] or 1)
    g = 1 if case['infer'] else small_groups(case['cin'], n, case['h'], case['w'])
    return g if g > 1 else chain_groups(case['k'], case['cin'], n)


# ----------------------------------------------------------------------------------------------------------------------------
# the case table
def _case(name, k, cin, cout, n, h, w, expect, epi=0, add_c=0, mask=False, bias=True, infer=False, arith='f16x2', transpose=False,
          extra=0, group=None, split=False, table=None):
    """``transpose``: the pack is the backward-data layer of a FORWARD (cin, cout + extra, k, k) weight with keep = cout (None when
    extra == 0); ``group``: members of a grouped launch (n images each); ``split``: the launch is expected to split its channels"""
    table = CASES if table is None else table
    assert name not in table, name
    table[name] = dict(name=name, k=k, cin=cin, cout=cout, n=n, h=h, w=w, expect=expect, epi=epi | (MASK if mask else 0), add_c=add_c,
                       mask=mask, bias=bias, infer=infer, arith=arith, transpose=transpose, extra=extra, group=group, split=split)


CASES = {}
TAPROW_LAYERS = [(5, 32, 3), (9, 64, 3), (9, 16, 2), (5, 48, 1)]
BAND_LAYERS = [(9, 64, 4), (5, 32, 12), (5, 7, 1), (9, 17, 3)]
NARROW_LAYERS = [(3, 64, 4), (3, 64, 3), (3, 16, 1)]
VECTOR_LAYERS = [(3, 24, 3), (3, 32, 8)]
ALL_LAYERS = TAPROW_LAYERS + BAND_LAYERS + NARROW_LAYERS + VECTOR_LAYERS
# the entry of a layer on the vector kernel in an inference launch: the 9x9 64-channel layers (5184 products per output) always in channel
# groups, everything else unsplit
VECTOR_ENTRY = {(9, 64, 3): SPLIT, (9, 64, 4): SPLIT}
_vec = lambda k, cin, cout: VECTOR_ENTRY.get((k, cin, cout), SMALL)
# the transposed packs of the models: SRCNNRes' 9x9 first layer to its 3 image channels (12 + P in all: keep = 3), SRCNNDemosaic's 9x9
# first layer (keep = 4 = all), Path-Restore's 3x3 first layers (keep = all)
EXTRA = {(9, 64, 3): 9, (9, 64, 4): 0, (3, 64, 4): 0, (3, 64, 3): 0, (5, 32, 3): 2, (5, 7, 1): 1, (3, 24, 3): 1}
# every H and W of the list once, the segment edges of inference launches (one 64-row segment: 50 below it and H % 4 = 2, 63, 66 = one
# + 2 rows, 130 = two + 2 rows) at several widths
SHAPES = [(1, 4), (2, 8), (3, 68), (5, 132), (13, 260), (31, 8), (50, 68), (63, 132), (66, 260), (130, 68), (50, 260), (66, 8), (130, 132),
          (64, 68), (128, 8)]                                  # ... and exactly one and two segments (the list above holds no multiple of 4)
FEW = [(3, 4), (50, 68), (66, 8), (130, 132), (64, 68)]
_l = lambda k, cin, cout: '%dx%d_%dto%d' % (k, k, cin, cout)

for _layers, _entry, _tag in ((TAPROW_LAYERS, TAPOUT, 'taprow'), (BAND_LAYERS, TOEP, 'band'), (NARROW_LAYERS, NARROW3, 'narrow3')):
    for _i, (_k, _ci, _co) in enumerate(_layers):
        for _h, _w in (SHAPES if _i == 0 else FEW):                        # inference: the matrix-pipe kernel whatever the grid
            _case('%s %s infer 1x%dx%d' % (_tag, _l(_k, _ci, _co), _h, _w), _k, _ci, _co, 1, _h, _w, _entry, infer=True)
        _case('%s %s infer 3x13x68' % (_tag, _l(_k, _ci, _co)), _k, _ci, _co, 3, 13, 68, _entry, infer=True)
        if (_k, _ci, _co) in EXTRA:
            for _h, _w in FEW[1:]:
                _case('%s %s transposed infer 2x%dx%d' % (_tag, _l(_k, _ci, _co), _h, _w), _k, _ci, _co, 2, _h, _w, _entry, infer=True,
                      transpose=True, extra=EXTRA[(_k, _ci, _co)], bias=False)
for _k, _ci, _co in VECTOR_LAYERS:                                         # no matrix-pipe pack: cin % 16, 8 couts on 3 taps
    for _h, _w in FEW:
        _case('vector %s infer 2x%dx%d' % (_l(_k, _ci, _co), _h, _w), _k, _ci, _co, 2, _h, _w, SMALL, infer=True)
_case('vector 3x3_24to3 train 2x31x132', 3, 24, 3, 2, 31, 132, SMALL)
_case('vector 3x3_32to8 train 2x31x132', 3, 32, 8, 2, 31, 132, SPLIT, split=True)                # 32 channels on 6 tiles: 4 channel groups
_case('vector 3x3_24to3 transposed train 2x13x68', 3, 24, 3, 2, 13, 68, SMALL, transpose=True, extra=1, bias=False)
for _h, _w in ((5, 6), (50, 30), (66, 6), (130, 30)):                      # W % 4 != 0: every layer on the vector kernel
    _case('vector 5x5_32to12 W%%4 infer 1x%dx%d' % (_h, _w), 5, 32, 12, 1, _h, _w, SMALL, infer=True)
    _case('vector 5x5_32to3 W%%4 infer 1x%dx%d' % (_h, _w), 5, 32, 3, 1, _h, _w, SMALL, infer=True)
_case('vector 3x3_64to4 W%4 infer 2x13x30', 3, 64, 4, 2, 13, 30, SMALL, infer=True)        # (its kernel takes any W; the dispatch asks W % 4 of all three)
_case('vector 9x9_64to4 W%4 infer 2x13x30', 9, 64, 4, 2, 13, 30, SPLIT, infer=True, split=True)
for _k, _ci, _co in ALL_LAYERS:                                            # the fp32 arithmetic and a mask keep every layer on the vector kernel
    _e = _vec(_k, _ci, _co)
    _case('f32 %s infer 2x50x68' % _l(_k, _ci, _co), _k, _ci, _co, 2, 50, 68, _e, infer=True, arith='f32', split=_e == SPLIT)
    _case('mask %s infer 2x66x8' % _l(_k, _ci, _co), _k, _ci, _co, 2, 66, 8, _e, infer=True, mask=True, split=_e == SPLIT)
_case('mask 5x5_32to3 train 2x13x68', 5, 32, 3, 2, 13, 68, SPLIT, mask=True, split=True)         # (32 channels and more: 4 .. 8 channel groups)
_case('mask 9x9_64to4 train 2x13x68', 9, 64, 4, 2, 13, 68, SPLIT, mask=True, split=True)
_case('mask 9x9_16to2 train 2x13x68', 9, 16, 2, 2, 13, 68, SMALL, mask=True)
_case('mask 3x3_24to3 train 2x13x68', 3, 24, 3, 2, 13, 68, SMALL, mask=True)

# epilogues, per route: every combination the route's kernel has, and one it has not (which must land on the vector kernel)
for _tag, (_k, _ci, _co), _entry, _tr in (('taprow', (5, 32, 3), TAPOUT, False), ('taprow', (9, 64, 3), TAPOUT, True),
                                          ('band', (9, 64, 4), TOEP, False), ('band', (9, 64, 4), TOEP, True), ('band', (9, 17, 3), TOEP, False),
                                          ('vector', (3, 24, 3), SMALL, False), ('vector', (3, 24, 3), SMALL, True)):
    _kw = dict(infer=True, transpose=_tr, extra=EXTRA.get((_k, _ci, _co), 0) if _tr else 0)
    _nm = '%s %s%s epi ' % (_tag, _l(_k, _ci, _co), ' transposed' if _tr else '')
    for _h, _w in ((50, 68), (13, 132)):
        _s = ' 2x%dx%d' % (_h, _w)
        _case(_nm + 'relu' + _s, _k, _ci, _co, 2, _h, _w, _entry, epi=RELU, **_kw)
        _case(_nm + 'add' + _s, _k, _ci, _co, 2, _h, _w, _entry, epi=ADD, add_c=_co, **_kw)
        _case(_nm + 'add_narrow' + _s, _k, _ci, _co, 2, _h, _w, _entry, epi=ADD, add_c=_co - 1, **_kw)
        _case(_nm + 'add_relu' + _s, _k, _ci, _co, 2, _h, _w, _entry, epi=ADD | RELU, add_c=_co, **_kw)
        _case(_nm + 'nobias' + _s, _k, _ci, _co, 2, _h, _w, _entry, bias=False, **_kw)
        _e = _vec(_k, _ci, _co)
        _case(_nm + 'mask (not the kernel\'s)' + _s, _k, _ci, _co, 2, _h, _w, _e, mask=True, split=_e == SPLIT, **_kw)
        _case(_nm + 'add_relu_mask' + _s, _k, _ci, _co, 2, _h, _w, _e, epi=ADD | RELU, add_c=_co, mask=True, split=_e == SPLIT, **_kw)
for _h, _w in ((50, 68), (13, 132), (66, 8)):
    _s = ' 2x%dx%d' % (_h, _w)
    for _k, _ci, _co in NARROW_LAYERS[:2]:
        _nm = 'narrow3 %s epi ' % _l(_k, _ci, _co)
        _case(_nm + 'relu' + _s, _k, _ci, _co, 2, _h, _w, NARROW3, epi=RELU, infer=True)
        _case(_nm + 'nobias' + _s, _k, _ci, _co, 2, _h, _w, NARROW3, bias=False, infer=True)
        _case(_nm + 'add (not the kernel\'s)' + _s, _k, _ci, _co, 2, _h, _w, SMALL, epi=ADD, add_c=_co, infer=True)
        _case(_nm + 'add_narrow_relu (not the kernel\'s)' + _s, _k, _ci, _co, 2, _h, _w, SMALL, epi=ADD | RELU, add_c=2, infer=True)
    _case('narrow3 3x3_64to4 epi shuffle2' + _s, 3, 64, 4, 2, _h, _w, NARROW3, epi=SHUFFLE2, infer=True)
    _case('narrow3 3x3_64to4 epi relu_shuffle2' + _s, 3, 64, 4, 2, _h, _w, NARROW3, epi=RELU | SHUFFLE2, infer=True)
    _case('narrow3 3x3_64to4 transposed epi shuffle2 nobias' + _s, 3, 64, 4, 2, _h, _w, NARROW3, epi=SHUFFLE2, infer=True, transpose=True, bias=False)
    _case('narrow3 3x3_64to4 train epi shuffle2' + _s, 3, 64, 4, 2, _h, _w, SPLIT, epi=SHUFFLE2, split=True)    # training: the vector kernel
    # PixelShuffle stores: 4 couts (9 taps: the band kernel has it, the tap-row kernel has no 4-cout layer), 8 and 12 (5 taps)
    _case('band 9x9_64to4 epi shuffle2' + _s, 9, 64, 4, 2, _h, _w, TOEP, epi=SHUFFLE2, infer=True)
    _case('band 9x9_64to4 transposed epi shuffle2 nobias' + _s, 9, 64, 4, 2, _h, _w, TOEP, epi=SHUFFLE2, infer=True, transpose=True, bias=False)
    _case('band 5x5_32to8 epi shuffle2' + _s, 5, 32, 8, 2, _h, _w, TOEP, epi=SHUFFLE2, infer=True)
    _case('band 5x5_32to12 epi shuffle2' + _s, 5, 32, 12, 2, _h, _w, TOEP, epi=SHUFFLE2, infer=True)
    _case('band 5x5_32to12 epi relu' + _s, 5, 32, 12, 2, _h, _w, TOEP, epi=RELU, infer=True)
    _case('band 5x5_32to12 epi add_narrow' + _s, 5, 32, 12, 2, _h, _w, TOEP, epi=ADD, add_c=5, infer=True)
    for _ci, _co in ((24, 4), (32, 8), (32, 12)):            # (3x3 32 -> 4 holds a (filter row, cout) pack: 24 channels do not)
        _case('vector 3x3_%dto%d epi shuffle2' % (_ci, _co) + _s, 3, _ci, _co, 2, _h, _w, SMALL, epi=SHUFFLE2, infer=True)
    _case('vector 5x5_32to12 f32 epi shuffle2' + _s, 5, 32, 12, 2, _h, _w, SMALL, epi=SHUFFLE2, infer=True, arith='f32')

# training launches: both sides of both grid thresholds on 12 x 8 planes (TAPOUT_MIN_ITEMS = 128 work items: one per image; TOEP_MIN_TILES
# = 256 tiles: one per image), a channel split of more than 1, and a grid with too few tap-row work items and band tiles enough
_case('train taprow 5x5_32to3 127x12x8', 5, 32, 3, 127, 12, 8, SPLIT, epi=ADD, add_c=3, split=True)
_case('train taprow 5x5_32to3 128x12x8', 5, 32, 3, 128, 12, 8, TAPOUT, epi=ADD, add_c=3)
_case('train taprow 9x9_64to3 transposed 127x12x8', 9, 64, 3, 127, 12, 8, SPLIT, epi=ADD, add_c=3, transpose=True, extra=9, bias=False, split=True)
_case('train taprow 9x9_64to3 transposed 128x12x8', 9, 64, 3, 128, 12, 8, TAPOUT, epi=ADD, add_c=3, transpose=True, extra=9, bias=False)
_case('train taprow 9x9_16to2 255x12x8', 9, 16, 2, 255, 12, 8, TAPOUT)
_case('train band 9x9_64to4 255x12x8', 9, 64, 4, 255, 12, 8, SPLIT, split=True)
_case('train band 9x9_64to4 256x12x8', 9, 64, 4, 256, 12, 8, TOEP)
_case('train band 5x5_32to12 255x12x8', 5, 32, 12, 255, 12, 8, SPLIT, epi=SHUFFLE2, split=True)
_case('train band 5x5_32to12 256x12x8', 5, 32, 12, 256, 12, 8, TOEP, epi=SHUFFLE2)
_case('train band 5x5_7to1 255x12x8', 5, 7, 1, 255, 12, 8, SMALL)
_case('train band 5x5_7to1 256x12x8', 5, 7, 1, 256, 12, 8, TOEP)
_case('train narrow3 3x3_64to3 256x12x8', 3, 64, 3, 256, 12, 8, SPLIT, split=True)                  # 3x3 tails train on the vector kernel
_case('train taprow 9x9_64to3 split 2x24x64', 9, 64, 3, 2, 24, 64, SPLIT, split=True)               # 8 channel groups
_case('train taprow 9x9_16to2 grid fails, band holds 32x63x260', 9, 16, 2, 32, 63, 260, TOEP)
_case('train taprow 5x5_32to3 whole H%4 128x50x8', 5, 32, 3, 128, 50, 8, TAPOUT, epi=ADD, add_c=3)  # the launch keeps 50 rows whole
_case('train taprow 5x5_32to3 f32 128x12x8', 5, 32, 3, 128, 12, 8, SPLIT, arith='f32', split=True)

# grouped launches against their per-member form (G members of n images: G * n on both sides of the thresholds; 127 is prime, so 126)
GROUPED = {}
for _name, _k, _ci, _co, _G, _n, _h, _w, _entry, _kw in (
        ('taprow 5x5_32to3 below 2x63x12x8', 5, 32, 3, 2, 63, 12, 8, SPLIT, dict(epi=ADD, add_c=3)),
        ('taprow 5x5_32to3 above 2x64x12x8', 5, 32, 3, 2, 64, 12, 8, TAPOUT, dict(epi=ADD, add_c=3)),
        ('taprow 9x9_64to3 transposed above 2x64x12x8', 9, 64, 3, 2, 64, 12, 8, TAPOUT, dict(epi=ADD, add_c=3, transpose=True, extra=9, bias=False)),
        ('band 9x9_64to4 below 3x85x12x8', 9, 64, 4, 3, 85, 12, 8, SPLIT, dict(epi=SHUFFLE2, transpose=True, bias=False)),
        ('band 9x9_64to4 above 2x128x12x8', 9, 64, 4, 2, 128, 12, 8, TOEP, dict(epi=SHUFFLE2, transpose=True, bias=False)),
        ('band 5x5_32to12 above 2x128x12x8', 5, 32, 12, 2, 128, 12, 8, TOEP, dict(epi=SHUFFLE2)),
        ('taprow 5x5_32to3 whole H%4 2x64x50x8', 5, 32, 3, 2, 64, 50, 8, TAPOUT, dict(epi=ADD, add_c=3)),
        ('taprow 9x9_16to2 grid fails, band holds 2x16x63x260', 9, 16, 2, 2, 16, 63, 260, TOEP, dict())):
    _case('grouped ' + _name, _k, _ci, _co, _n, _h, _w, _entry, group=_G, split=_entry == SPLIT, table=GROUPED, **_kw)


def walk(seed=20261, draws=16):
    """a short seeded walk over layer x shape x epilogue x mode; ``expect`` None: the test holds the launch to ``route_small`` and to
    ``ENTRY_ACCEPTS`` alone"""
    rng = np.random.default_rng(seed)
    out = {}
    hs, ws = [1, 2, 3, 5, 13, 31, 50, 63, 66, 130], [4, 8, 68, 132, 260, 6, 30]
    for i in range(draws):
        k, cin, cout = ALL_LAYERS[int(rng.integers(len(ALL_LAYERS)))]
        h, w, n = hs[int(rng.integers(len(hs)))], ws[int(rng.integers(len(ws)))], int(rng.integers(1, 4))
        epis = [(0, 0), (RELU, 0), (ADD, cout), (ADD, max(1, cout - 1)), (ADD | RELU, cout)] + ([(SHUFFLE2, 0)] if cout % 4 == 0 else [])
        epi, add_c = epis[int(rng.integers(len(epis)))]
        tr = (k, cin, cout) in EXTRA and rng.random() < 0.4
        mask = epi != SHUFFLE2 and rng.random() < 0.15
        c = dict(name='walk %02d %s %dx%dx%d epi %d' % (i, _l(k, cin, cout), n, h, w, epi), k=k, cin=cin, cout=cout, n=n, h=h, w=w, expect=None,
                 epi=epi | (MASK if mask else 0), add_c=add_c, mask=mask, bias=bool(rng.random() < 0.7), infer=bool(rng.random() < 0.6),
                 arith='f32' if rng.random() < 0.15 else 'f16x2', transpose=bool(tr), extra=EXTRA.get((k, cin, cout), 0) if tr else 0,
                 group=None, split=None)
        out[c['name']] = c
    return out


WALK = walk()
ALL = dict(CASES)
ALL.update(WALK)


# ----------------------------------------------------------------------------------------------------------------------------
# inputs and the restatement
def _rnd(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _inputs(name, table):
    case = (GROUPED if table == 'grouped' else ALL)[name]
    rng = np.random.default_rng(abs(hash_name(name)))
    G, n, h, w, k, cin, cout = case['group'] or 1, case['n'], case['h'], case['w'], case['k'], case['cin'], case['cout']
    shape = (cin, cout + case['extra'], k, k) if case['transpose'] else (cout, cin, k, k)
    # the recipe of the kernels' own files: standard-normal x, 0.05 x standard-normal weights, 0.1 x bias.  The mask is an activation
    # after its ReLU (half its elements are exactly 0: what tells mask > 0 from mask >= 0), the residual standard normal
    d = dict(weights=[_rnd(rng, *shape) * 0.05 for _ in range(G)], bias=[_rnd(rng, cout) * 0.1 if case['bias'] else None for _ in range(G)],
             x=_rnd(rng, G * n, cin, h, w))
    d['add'] = _rnd(rng, G * n, case['add_c'], h, w) if case['epi'] & ADD else None
    d['mask'] = torch.relu(_rnd(rng, G * n, cout, h, w)) if case['mask'] else None
    return d


def hash_name(name):
    v = 0
    for ch in name.encode():
        v = (v * 131 + ch) % (2 ** 31 - 1)
    return v


def inputs(case):
    """CPU float32 tensors of a case (cached, shared by every test that needs them: do not write into them)"""
    return _inputs(case['name'], 'grouped' if case['group'] else 'all')


def keep_of(case):
    return case['cout'] if case['transpose'] and case['extra'] else None


def out_shape(case):
    G, n, h, w, cout = case['group'] or 1, case['n'], case['h'], case['w'], case['cout']
    return (G * n, cout // 4, 2 * h, 2 * w) if case['epi'] & SHUFFLE2 else (G * n, cout, h, w)


def shuffle2(z, swapped=False):
    n, c, h, w = z.shape
    v = z.view(n, c // 4, 2, 2, h, w)                       # cout 4 g + 2 i + j
    v = v.permute(0, 1, 4, 3, 5, 2) if swapped else v.permute(0, 1, 4, 2, 5, 3)       # -> (n, g, y, i, x, j)
    return v.reshape(n, c // 4, 2 * h, 2 * w)


def _linear(case, dtype, wrong=None):
    """the convolution alone, per member of the group"""
    d, k, cout, n = inputs(case), case['k'], case['cout'], case['n']
    zs = []
    for g in range(case['group'] or 1):
        wt, x = d['weights'][g].to(dtype), d['x'][g * n:(g + 1) * n].to(dtype)
        if wrong == 'flip':
            wt = wt.flip(2, 3)
        if case['transpose']:
            zs.append(TF.conv_transpose2d(x, wt[:, -cout:] if wrong == 'keep' else wt[:, :cout], padding=k // 2))
        else:
            zs.append(TF.conv2d(x, wt, padding=k // 2))
    return tuple(zs)


@functools.lru_cache(maxsize=None)
def _linear64(name, table):
    return _linear((GROUPED if table == 'grouped' else ALL)[name], torch.float64)


def reference(case, dtype=torch.float64, wrong=None):
    """the operation of a case in ``dtype`` on the CPU.  ``wrong``: one of WRONG - the same with one deliberate mistake (what
    tests/test_conv_small_reference_cpu.py uses to show that the restatement would notice it)"""
    d, cout, n = inputs(case), case['cout'], case['n']
    if dtype == torch.float64 and wrong not in ('flip', 'keep'):
        zs = _linear64(case['name'], 'grouped' if case['group'] else 'all')          # (shared by the variants of the epilogue)
    else:
        zs = _linear(case, dtype, wrong)
    outs = []
    for g, z in enumerate(zs):
        s = slice(g * n, (g + 1) * n)
        if d['bias'][g] is not None and wrong != 'bias':
            z = z + d['bias'][g].to(dtype).view(1, -1, 1, 1)
        if wrong == 'relu_first' and case['epi'] & RELU:
            z = torch.relu(z)
        if case['epi'] & ADD:
            a, c = d['add'][s].to(dtype), case['add_c']
            if wrong == 'add_all':
                z = z + a[:, [co % c for co in range(cout)]]
            else:
                z = torch.cat([z[:, :c] + a, z[:, c:]], 1)
        if case['epi'] & RELU and wrong != 'relu_first':
            z = torch.relu(z)
        if case['epi'] & MASK:
            m = d['mask'][s]
            z = z * ((m >= 0) if wrong == 'mask_ge' else (m > 0)).to(dtype)
        if case['epi'] & SHUFFLE2:
            z = shuffle2(z, swapped=wrong == 'shuffle')
        outs.append(z)
    return torch.cat(outs)


@functools.lru_cache(maxsize=None)
def _ref64(name, table):
    return reference((GROUPED if table == 'grouped' else ALL)[name], torch.float64)


def ref64(case):
    """the float64 restatement, computed once per case and shared (do not write into it)"""
    return _ref64(case['name'], 'grouped' if case['group'] else 'all')


# deliberate mistakes and the cases that have the feature each one touches
WRONG = {
    'flip': lambda c: True,                                                       # taps flipped
    'bias': lambda c: c['bias'],                                                  # bias dropped
    'add_all': lambda c: bool(c['epi'] & ADD) and c['add_c'] < c['cout'],         # residual added to all couts instead of add_c
    'relu_first': lambda c: (c['epi'] & (ADD | RELU)) == (ADD | RELU),            # ReLU before the residual
    'mask_ge': lambda c: c['mask'],                                               # mask applied as >= 0
    'shuffle': lambda c: bool(c['epi'] & SHUFFLE2),                               # the two sub-pixel indices swapped
    'keep': lambda c: c['transpose'] and c['extra'] > 0,                          # keep ignored: other channels of the forward weight
}


def rect_sums64(g, k):
    """float64 rectangle sums (include/risp.h: risp_rect_sums): out[p][ky][kx] = the sum of plane p over the pixels q with
    q + (ky - k/2, kx - k/2) inside the plane"""
    n, c, h, w = g.shape
    g, p = g.double(), k // 2
    out = torch.empty(n, c, k, k, dtype=torch.float64)
    for ky in range(k):
        y0, y1 = max(0, p - ky), min(h, h + p - ky)
        for kx in range(k):
            x0, x1 = max(0, p - kx), min(w, w + p - kx)
            out[:, :, ky, kx] = g[:, :, y0:y1, x0:x1].sum(dim=(2, 3))
    return out.view(n, c * k * k)
