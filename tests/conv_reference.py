"""``convnets.conv`` over its argument space, stated without the GPU: the float32 / float64 restatement of the operation, what each of
the eight entry points of the library accepts, the dispatch as ``conv`` asks it, and the table of cases tests/test_gpu_conv_space.py
runs.  Plain torch on the CPU; checked by tests/test_conv_reference_cpu.py.

The operation (include/risp.h, in the order the kernels apply it - risp_conv.hip, the epilogue of conv_mfma_kernel):

    the load        PLAIN;  UNSHUFFLE2: plane 4 c + 2 i + j = x[c][2 y + i][2 x + j];  CONSTCH: channels >= cin_img are
                    cvals[n, ci - cin_img] inside the image and 0 in the padding
    z = conv2d(planes, w, padding k // 2), or conv_transpose2d(planes, w, padding k // 2) for the backward-data pack of a FORWARD weight
    z += bias                                       unless EPI_NOBIAS (``conv`` sets it itself when ``transpose``)
    EPI_CASEBIAS:  z += cvals[n, co, case(y), case(x)]      ``border_case`` of risp_conv.hip
    EPI_ADD:       z[:, :add_c] += add              the residual reaches the first add_c couts only
    EPI_RELU:      z = max(z, 0)
    EPI_MASK:      z = z where mask > 0, else 0
    EPI_SHUFFLE2:  cout 4 g + 2 i + j -> plane g, pixel (2 y + i, 2 x + j)

A case names the channels as the LAUNCH sees them: ``cin`` planes in, ``cout`` planes out.  With ``transpose`` the layer's weight is the
FORWARD (cin, cout, k, k) tensor - ``PackedConv`` then has pc.cout = cin and pc.cin = cout.

``ENTRY_ACCEPTS`` restates the argument checks of the entry points (the RISP_CHECK_ARG lines of risp_conv.hip, risp_conv_wino.hip,
risp_conv_f16x2.hip, risp_conv_thin5.hip, risp_conv_k3.hip, risp_conv_toep_first.hip, and RISP_CHECK_GROUP of risp_common.h) on a
``launch`` - it knows nothing of ``route``."""
import functools
import itertools
import os

import numpy as np
import torch
import torch.nn.functional as TF

from wino_emulate import wino43_emulate, wino45_emulate

RELU, ADD, MASK, SHUFFLE2, NOBIAS, CASEBIAS = 1, 2, 4, 8, 16, 32                # include/risp.h: RISP_EPI_*
PLAIN, UNSHUFFLE2, CONSTCH = 0, 1, 2                                            # RISP_LOAD_*
SHARED_X, SHARED_ADD = 1, 2                                                     # RISP_GROUP_SHARED_*
GEN, W43, W45, F16X2, THIN5, K3, TF1, TF1X = ('risp_conv2d', 'risp_conv2d_wino43', 'risp_conv2d_wino45', 'risp_conv2d_f16x2',
                                              'risp_conv2d_thin5', 'risp_conv2d_k3', 'risp_conv2d_toep_first', 'risp_conv2d_toep_first_exact')
ENTRIES = (GEN, W43, W45, F16X2, THIN5, K3, TF1, TF1X)
# max error / max|ref| of the split-precision entries: the bars of their own files (test_gpu_f16x2.py, test_gpu_thin5.py, test_gpu_toep.py)
SPLIT_BAR = {F16X2: 5e-6, THIN5: 2e-6, TF1: 3e-6, TF1X: 3e-6}
# the fp32 entries have no bar of their own: conftest.ErrorBudget's rule against the CPU float32 yardstick of the same algorithm class
FACTOR, ATOL, CAP = 2.0, 4e-6, 1e-4


def bound(entry, e32):
    """the accuracy bound of a case served by ``entry``, given the error ``e32`` of its float32 yardstick"""
    return SPLIT_BAR[entry] if entry in SPLIT_BAR else min(FACTOR * e32, CAP) + ATOL


# ----------------------------------------------------------------------------------------------------------------------------
# what each entry point accepts.  launch: dict(k, cin, cout, n (images of the launch, all members), h, w, load, cin_img, epi (with NOBIAS),
# add_c, has_add, has_mask, has_bias, has_cvals, al (the 16-byte alignment of x, y, add, mask: absent tensors count as aligned),
# group_n (0: not grouped), wpack_gs (floats))
def _shape(L):
    return L['n'] > 0 and L['h'] > 0 and L['w'] > 0 and L['cin'] > 0 and L['cout'] > 0


def _group(L):                                                                  # RISP_CHECK_GROUP
    return L['group_n'] == 0 or (L['group_n'] > 0 and L['n'] % L['group_n'] == 0 and L['wpack_gs'] >= 0 and L['wpack_gs'] % 4 == 0)


def _tensors(L):
    return ((bool(L['epi'] & NOBIAS) or L['has_bias']) and (not (L['epi'] & ADD) or (L['has_add'] and L['add_c'] > 0))
            and (not (L['epi'] & MASK) or L['has_mask']))


def _aligned(L, names=('x', 'y', 'add', 'mask')):
    return all(L['al'][t] for t in names)


def _ncb(L):
    return (L['cout'] + 31) // 32


def accepts_gen(L):
    P = L['k'] // 2
    return (_group(L) and _shape(L) and L['n'] <= 65535 and L['cout'] <= 64 and _tensors(L)
            and (not (L['epi'] & SHUFFLE2) or (L['cout'] % 4 == 0 and not (L['epi'] & MASK)))
            and (L['load'] != UNSHUFFLE2 or L['cin'] % 4 == 0)
            and (L['load'] != CONSTCH or (L['has_cvals'] and 0 < L['cin_img'] <= L['cin']))
            and (not (L['epi'] & CASEBIAS) or (L['has_cvals'] and L['load'] != CONSTCH and L['h'] >= 2 * P and L['w'] >= 2 * P))
            and L['k'] in (1, 3, 5, 9))


def _wino(L):
    return (_shape(L) and L['w'] % 4 == 0 and L['cout'] <= 64 and L['n'] * _ncb(L) <= 65535 and L['load'] == PLAIN
            and not (L['epi'] & ~(RELU | ADD | MASK | NOBIAS)) and _tensors(L) and _aligned(L))


def accepts_wino43(L):
    return L['group_n'] == 0 and _wino(L) and L['k'] == 3


def accepts_wino45(L):
    return _group(L) and _wino(L) and L['k'] == 5 and (L['cin'] % 4 == 0 or L['cin'] < 4)


def accepts_f16x2(L):
    return (_group(L) and _shape(L) and L['w'] % 4 == 0 and L['cin'] % 16 == 0 and L['cout'] in (32, 64) and L['k'] in (3, 5)
            and max(L['cin'], L['cout']) * L['h'] * L['w'] * 4 < 2 ** 31 and (not (L['epi'] & ADD) or L['add_c'] == L['cout'])
            and L['load'] == PLAIN and not (L['epi'] & ~(RELU | ADD | MASK | NOBIAS)) and _tensors(L) and _aligned(L))


def accepts_thin5(L):
    items = L['n'] * ((L['w'] + 127) // 128) * ((L['h'] + 31) // 32) * (L['cout'] // 32)
    return (_group(L) and _shape(L) and L['k'] == 5 and 1 <= L['cin'] <= 3 and L['cout'] in (32, 64) and L['load'] == PLAIN
            and not (L['epi'] & ~(RELU | MASK | NOBIAS)) and (not (L['epi'] & MASK) or L['has_mask'])
            and (bool(L['epi'] & NOBIAS) or L['has_bias']) and L['cout'] * L['h'] * L['w'] * 4 < 2 ** 31 and items <= 2 ** 31 - 1)


def _first_epi(L):
    return (not (L['epi'] & ~(RELU | NOBIAS | CASEBIAS)) and (bool(L['epi'] & NOBIAS) or L['has_bias'])
            and (not (L['epi'] & CASEBIAS) or (L['has_cvals'] and L['h'] >= L['k'] - 1 and L['w'] >= L['k'] - 1)) and _aligned(L, ('x', 'y')))


def accepts_k3(L):
    unshuf = L['load'] == UNSHUFFLE2
    return (_group(L) and L['n'] > 0 and L['h'] > 0 and L['w'] > 0 and L['w'] % 4 == 0 and 0 < L['cout'] <= 64 and L['n'] * 2 <= 65535
            and L['k'] in (3, 9) and ((L['cin'] == 3 and not unshuf) or (L['cin'] == 4 and unshuf)) and L['load'] in (PLAIN, UNSHUFFLE2)
            and _first_epi(L))


def accepts_toep_first(L):
    return (_group(L) and (L['load'] == PLAIN or (L['load'] == UNSHUFFLE2 and L['cin'] == 4)) and _shape(L) and L['w'] % 4 == 0
            and L['cin'] <= 16 and L['k'] == 9 and L['cin'] * L['h'] * L['w'] < 2 ** 30 and _first_epi(L))


def accepts_toep_first_exact(L):
    return accepts_toep_first(L) and L['n'] * L['cout'] * L['h'] * L['w'] < 2 ** 32


ENTRY_ACCEPTS = {GEN: accepts_gen, W43: accepts_wino43, W45: accepts_wino45, F16X2: accepts_f16x2, THIN5: accepts_thin5, K3: accepts_k3,
                 TF1: accepts_toep_first, TF1X: accepts_toep_first_exact}


def launch_epi(case):
    """the epilogue word ``conv`` writes into the descriptor"""
    return case['epi'] | (NOBIAS if case['transpose'] else 0)


def launch_of(case, **over):
    """the launch a case asks of ``conv``, as ``ENTRY_ACCEPTS`` reads it"""
    G, mis = case['group'] or 1, case['misalign']
    L = dict(k=case['k'], cin=case['cin'], cout=case['cout'], n=case['n'] * G, h=case['h'], w=case['w'], load=case['load'],
             cin_img=case['cin_img'], epi=launch_epi(case), add_c=case['add_c'], has_add=bool(case['epi'] & ADD),
             has_mask=bool(case['epi'] & MASK), has_bias=True, has_cvals=case['load'] == CONSTCH or bool(case['epi'] & CASEBIAS),
             al=dict(x=mis != 'x', y=mis != 'out', add=mis != 'add', mask=mis != 'mask'), group_n=case['n'] if case['group'] else 0, wpack_gs=0)
    L.update(over)
    return L


def layer_of(case):
    """(k, cin, cout) of the FORWARD layer whose ``PackedConv`` serves the case"""
    return (case['k'], case['cout'], case['cin']) if case['transpose'] else (case['k'], case['cin'], case['cout'])


def have_of(case):
    """``have`` as ``conv`` hands it to ``route``: ``pack_kinds`` of the layer, without the 3x3 Winograd pack on stacked layers"""
    from reconfigisp_amd import convnets as CN
    have = CN.pack_kinds(*layer_of(case), case['transpose'])
    return [p for p in have if not (case['group'] and p == 'wino43')]


def routed(case, **over):
    """``convnets.route`` as ``conv`` asks it for a case, under the CONV_ARITH / TOEP_FIRST the caller has set - and the one decision
    ``conv`` adds: the exact first layer counts its outputs in 32 bits"""
    from reconfigisp_amd import convnets as CN
    c = dict(case, **over)
    entry = CN.route(c['k'], c['cin'], c['cout'], c['h'], c['w'], c['transpose'], c['load'], launch_epi(c), c['add_c'], c['infer'],
                     c['misalign'] is None, have_of(c))
    if entry == TF1X and c['n'] * (c['group'] or 1) * c['cout'] * c['h'] * c['w'] >= 2 ** 32:
        entry = TF1
    return entry


def gen_instance(case):
    """(k, ck, cb, fast): the template instance of risp_conv2d that serves a case - ``conv_cfg`` and ``launch_conv`` of risp_conv.hip"""
    k, cb = case['k'], 2 if case['cout'] > 32 else 1
    ck = 2 if k == 9 else 8 if k == 1 else 2 if (k == 5 and cb == 2) else 4
    return k, ck, cb, case['load'] != UNSHUFFLE2 and case['w'] % 4 == 0 and case['misalign'] != 'x'


GEN_INSTANCES = {(k, ck, cb, f) for (k, ck, cb) in ((3, 4, 2), (3, 4, 1), (5, 4, 1), (5, 2, 2), (9, 2, 2), (9, 2, 1), (1, 8, 2), (1, 8, 1))
                 for f in (True, False)}


def gen_vector_stores(case):
    """does the general kernel store 16 bytes per lane (its second switch: W % 4, no PixelShuffle, y | add | mask aligned)"""
    return case['w'] % 4 == 0 and not (case['epi'] & SHUFFLE2) and case['misalign'] not in ('out', 'add', 'mask')


def wino43_form(case):
    """which kernel risp_conv2d_wino43 launches: both cout blocks per wave ('b2'), LDS-DMA staging ('glds'), or the plain one"""
    return 'plain' if case['cin'] % 4 else ('b2' if case['cout'] > 32 else 'glds')


# ----------------------------------------------------------------------------------------------------------------------------
# the case table
CASES, GROUPED = {}, {}
GEOMS = [(2, 13, 132), (2, 50, 68), (2, 66, 8), (1, 64, 68), (3, 13, 68), (1, 130, 132)]     # tile edges of every kernel (the siblings' list)
TINY = [(1, 1, 4), (1, 3, 4)]
ODD = [(2, 9, 10), (2, 17, 66), (1, 33, 30)]                                                # W % 4 != 0: the general kernel's scalar forms
TWO = [(2, 50, 68), (3, 13, 68)]
MANY = (300, 8, 64)                                     # more tiles than persistent workgroups: every workgroup walks several


def _case(name, k, cin, cout, nhw, expect, epi=0, add_c=None, load=PLAIN, cin_img=0, transpose=False, infer=False, arith='f16x2',
          toep='train', misalign=None, group=None, gflags=0, scale=False, table=None):
    """``add_c`` None: all couts where the epilogue has ADD; ``scale``: half of the input channels scaled by 1e-3 (the running exponent
    of the split-precision kernels moves between the chunks); ``misalign``: the tensor handed over as a view 4 bytes off 16"""
    table = CASES if table is None else table
    n, h, w = nhw
    name = '%s %dx%dx%d' % (name, n, h, w)
    assert name not in table, name
    table[name] = dict(name=name, k=k, cin=cin, cout=cout, n=n, h=h, w=w, expect=expect, epi=epi,
                       add_c=(cout if add_c is None else add_c) if epi & ADD else 0, load=load, cin_img=cin_img, transpose=transpose,
                       infer=infer, arith=arith, toep=toep, misalign=misalign, group=group, gflags=gflags, scale=scale)


_l = lambda k, cin, cout: '%dx%d_%dto%d' % (k, k, cin, cout)
_EPI_NAMES = ((RELU, 'relu'), (ADD, 'add'), (MASK, 'mask'), (SHUFFLE2, 'shuffle2'), (NOBIAS, 'nobias'), (CASEBIAS, 'casebias'))
_e = lambda epi: '+'.join(nm for bit, nm in _EPI_NAMES if epi & bit) or 'none'
SUBSETS = [r | a | m for r in (0, RELU) for a in (0, ADD) for m in (0, MASK)]

# --- the general kernel, every template instance in both staging forms.  What keeps a layer off the other entries is in the tag
GEN_LAYERS = [('1x1', 1, 64, 64, {}), ('1x1', 1, 5, 13, {}), ('cin%4', 5, 5, 13, {}), ('cin%4', 5, 13, 31, {}), ('cin%4', 5, 17, 33, {}),
              ('cin%4', 5, 13, 48, {}), ('cin%4', 5, 17, 64, {}), ('9x9', 9, 13, 64, {}), ('9x9', 9, 17, 31, {}),
              ('constch', 3, 13, 48, dict(load=CONSTCH, cin_img=3)), ('constch', 3, 8, 31, dict(load=CONSTCH, cin_img=3)),
              ('shuffle2', 3, 8, 16, dict(epi=SHUFFLE2)), ('shuffle2', 3, 17, 64, dict(epi=SHUFFLE2)),
              ('casebias', 3, 13, 31, dict(epi=CASEBIAS)), ('casebias', 3, 5, 33, dict(epi=CASEBIAS | RELU))]
for _i, (_tag, _k, _ci, _co, _kw) in enumerate(GEN_LAYERS):
    for _g in (GEOMS + TINY if _i in (0, 4) else TWO):                         # 16-byte staging
        if _kw.get('epi', 0) & CASEBIAS and (_g[1] < _k - 1 or _g[2] < _k - 1):
            continue
        _case('gen %s %s' % (_tag, _l(_k, _ci, _co)), _k, _ci, _co, _g, GEN, **_kw)
    for _g in (ODD if _i in (0, 4, 7) else ODD[:2]):                           # W % 4 != 0: element staging and element stores
        _case('gen %s %s' % (_tag, _l(_k, _ci, _co)), _k, _ci, _co, _g, GEN, **_kw)
for _k, _ci, _co in ((3, 17, 33), (3, 5, 13), (3, 64, 64), (5, 12, 40), (5, 3, 32), (9, 3, 20)):       # W % 4 != 0 takes every layer here
    for _g in ODD[:2]:
        _case('gen W%%4 %s' % _l(_k, _ci, _co), _k, _ci, _co, _g, GEN, epi=RELU)
# the space-to-depth load on the general kernel (element staging whatever W): 8 and 64 planes of a 2 / 16-plane mosaic
for _ci, _co in ((8, 13), (64, 64), (8, 48)):
    for _g in ((2, 13, 132), (2, 50, 68), (2, 9, 10)):
        _case('gen unshuffle2 %s' % _l(3, _ci, _co), 3, _ci, _co, _g, GEN, load=UNSHUFFLE2, epi=RELU)
_case('gen unshuffle2 %s shuffle2' % _l(3, 8, 16), 3, 8, 16, (2, 13, 68), GEN, load=UNSHUFFLE2, epi=SHUFFLE2)
# SRCNNRes: the first layer over 3 image planes and 9 + P broadcast constants, and its backward-data launch - 9x9, 64 -> 12 + P couts,
# the residual on the 3 image channels only
for _P in (0, 1, 5):
    for _g in ((2, 13, 68), (2, 9, 10)):
        _case('gen constch srcnn P=%d %s' % (_P, _l(9, 12 + _P, 64)), 9, 12 + _P, 64, _g, GEN, load=CONSTCH, cin_img=3, epi=RELU)
    for _g in ((2, 13, 68), (2, 50, 68), (2, 17, 66)):
        _case('gen srcnn backward-data P=%d %s' % (_P, _l(9, 64, 12 + _P)), 9, 64, 12 + _P, _g, GEN, transpose=True, epi=ADD, add_c=3)
# the epilogue of the general kernel in its vector and its element form
for _g in ((2, 50, 68), (2, 17, 66)):
    for _s in SUBSETS:
        _case('gen epi %s %s' % (_e(_s), _l(5, 17, 33)), 5, 17, 33, _g, GEN, epi=_s)
    _case('gen epi add_narrow+relu %s' % _l(5, 17, 33), 5, 17, 33, _g, GEN, epi=ADD | RELU, add_c=5)
    _case('gen epi add_narrow+mask %s' % _l(5, 13, 31), 5, 13, 31, _g, GEN, epi=ADD | MASK, add_c=30)
    _case('gen epi nobias %s' % _l(5, 17, 33), 5, 17, 33, _g, GEN, epi=NOBIAS)
    _case('gen epi nobias+relu+add %s' % _l(1, 64, 64), 1, 64, 64, _g, GEN, epi=NOBIAS | RELU | ADD)
    _case('gen epi casebias %s' % _l(9, 13, 64), 9, 13, 64, _g, GEN, epi=CASEBIAS)                # interior and edge tiles at 50 x 68
    _case('gen epi casebias+relu %s' % _l(5, 17, 33), 5, 17, 33, _g, GEN, epi=CASEBIAS | RELU)
    _case('gen epi casebias+add+mask %s' % _l(3, 13, 31), 3, 13, 31, _g, GEN, epi=CASEBIAS | ADD | MASK)
    _case('gen epi shuffle2+relu %s' % _l(3, 8, 16), 3, 8, 16, _g, GEN, epi=SHUFFLE2 | RELU)
    _case('gen epi shuffle2+add %s' % _l(5, 17, 64), 5, 17, 64, _g, GEN, epi=SHUFFLE2 | ADD, add_c=7)
    _case('gen epi shuffle2+casebias %s' % _l(9, 13, 64), 9, 13, 64, _g, GEN, epi=SHUFFLE2 | CASEBIAS)
_case('gen epi casebias edge tiles only %s' % _l(3, 13, 31), 3, 13, 31, (2, 13, 28), GEN, epi=CASEBIAS)
_case('gen epi casebias smallest %s' % _l(9, 13, 64), 9, 13, 64, (1, 8, 8), GEN, epi=CASEBIAS | RELU)

# --- fp32 Winograd F(4,3): cout blocks of 32; both cout blocks per wave (33 .. 64 couts, cin % 4 == 0), LDS-DMA staging, plain staging
W43_LAYERS = [(17, 33, 'f16x2'), (64, 64, 'f32'), (4, 32, 'f16x2'), (64, 20, 'f16x2'), (17, 64, 'f16x2'), (4, 33, 'f16x2'), (64, 33, 'f16x2'),
              (17, 20, 'f16x2'), (64, 32, 'f32')]
for _i, (_ci, _co, _ar) in enumerate(W43_LAYERS):
    for _g in (GEOMS + TINY if _i < 2 else TWO):
        _case('wino43 %s %s' % (_l(3, _ci, _co), _ar), 3, _ci, _co, _g, W43, arith=_ar, epi=RELU if _i % 2 else 0)
for _s in SUBSETS:
    _case('wino43 epi %s %s' % (_e(_s), _l(3, 17, 33)), 3, 17, 33, (2, 50, 68), W43, epi=_s)
    _case('wino43 epi %s %s f32' % (_e(_s), _l(3, 64, 64)), 3, 64, 64, (3, 13, 68), W43, epi=_s, arith='f32')
for _g in TWO:
    _case('wino43 epi add_narrow (not the split kernel\'s) %s' % _l(3, 64, 64), 3, 64, 64, _g, W43, epi=ADD | RELU, add_c=3, scale=True)
    _case('wino43 epi nobias %s' % _l(3, 17, 33), 3, 17, 33, _g, W43, epi=NOBIAS | RELU)
    _case('wino43 backward-data %s' % _l(3, 33, 17), 3, 33, 17, _g, W43, transpose=True, epi=ADD | MASK)
    _case('wino43 backward-data %s f32' % _l(3, 64, 64), 3, 64, 64, _g, W43, transpose=True, epi=MASK, arith='f32')

# --- fp32 Winograd F(4,5): two output rows per wave
W45_LAYERS = [(12, 40, 'f16x2'), (64, 64, 'f32'), (3, 32, 'f32'), (1, 64, 'f32'), (12, 32, 'f16x2'), (64, 40, 'f16x2'), (12, 64, 'f16x2'),
              (3, 40, 'f16x2'), (1, 40, 'f16x2')]
for _i, (_ci, _co, _ar) in enumerate(W45_LAYERS):
    for _g in (GEOMS + TINY if _i < 2 else TWO):
        _case('wino45 %s %s' % (_l(5, _ci, _co), _ar), 5, _ci, _co, _g, W45, arith=_ar, epi=RELU if _i % 2 else 0)
for _s in SUBSETS:
    _case('wino45 epi %s %s' % (_e(_s), _l(5, 12, 40)), 5, 12, 40, (2, 50, 68), W45, epi=_s)
for _g in TWO:
    _case('wino45 epi add_narrow (not the split kernel\'s) %s' % _l(5, 32, 32), 5, 32, 32, _g, W45, epi=ADD, add_c=31, scale=True)
    _case('wino45 epi add (not the thin kernel\'s) %s' % _l(5, 3, 32), 5, 3, 32, _g, W45, epi=ADD | RELU)
    _case('wino45 epi nobias %s' % _l(5, 12, 40), 5, 12, 40, _g, W45, epi=NOBIAS)
    _case('wino45 backward-data %s' % _l(5, 40, 12), 5, 40, 12, _g, W45, transpose=True, epi=ADD | MASK)

# --- split precision on the f16 matrix pipe: 8 x 64 tiles, one and two cout blocks, 3 and 5 taps
F16_LAYERS = [(3, 32, 64), (5, 64, 32), (3, 16, 32), (3, 64, 64), (3, 64, 32), (3, 16, 64), (5, 16, 32), (5, 32, 64), (5, 64, 64)]
for _i, (_k, _ci, _co) in enumerate(F16_LAYERS):
    for _g in (GEOMS + TINY if _i < 2 else TWO):
        _case('f16x2 %s' % _l(_k, _ci, _co), _k, _ci, _co, _g, F16X2, scale=True, epi=RELU if _i % 2 else 0, infer=bool(_i % 3 == 0))
_case('f16x2 many tiles %s' % _l(3, 32, 32), 3, 32, 32, MANY, F16X2, scale=True, epi=RELU)
for _s in SUBSETS:
    _case('f16x2 epi %s %s' % (_e(_s), _l(3, 64, 64)), 3, 64, 64, (2, 50, 68), F16X2, epi=_s, scale=True)
    _case('f16x2 epi %s %s' % (_e(_s), _l(5, 32, 32)), 5, 32, 32, (3, 13, 68), F16X2, epi=_s, scale=True)
for _g in TWO:
    _case('f16x2 epi nobias %s' % _l(3, 32, 64), 3, 32, 64, _g, F16X2, epi=NOBIAS | RELU, scale=True)
    _case('f16x2 backward-data %s' % _l(5, 64, 32), 5, 64, 32, _g, F16X2, transpose=True, epi=ADD | MASK, scale=True)
    _case('f16x2 backward-data %s' % _l(3, 64, 64), 3, 64, 64, _g, F16X2, transpose=True, epi=MASK, scale=True)

# --- 5x5 over at most 3 planes in split precision: 128 columns x 32 rows per work item
for _i, (_ci, _co) in enumerate(((3, 32), (1, 64), (2, 32), (3, 64), (1, 32), (2, 64))):
    for _g in (GEOMS + TINY if _i < 2 else TWO):
        _case('thin5 %s' % _l(5, _ci, _co), 5, _ci, _co, _g, THIN5, epi=RELU if _i % 2 else 0)
_case('thin5 many items %s' % _l(5, 3, 32), 5, 3, 32, MANY, THIN5)
for _s in (0, RELU, MASK, RELU | MASK, NOBIAS, NOBIAS | RELU | MASK):
    _case('thin5 epi %s %s' % (_e(_s), _l(5, 3, 64)), 5, 3, 64, (2, 50, 68), THIN5, epi=_s)
for _g in TWO:
    _case('thin5 backward-data %s' % _l(5, 3, 32), 5, 3, 32, _g, THIN5, transpose=True, epi=MASK)
    _case('thin5 backward-data %s' % _l(5, 1, 64), 5, 1, 64, _g, THIN5, transpose=True)

# --- first layers: 3 plain planes or the 4 planes of the space-to-depth mosaic, 3x3 and 9x9, under every TOEP_FIRST and both arithmetics
FIRST_SMALLEST = {3: (1, 2, 4), 9: (1, 8, 8)}


def first_entry(k, arith, toep, infer):
    """rule 1 of ``route``, written out as the table's literal expectation"""
    if k == 9 and arith == 'f16x2':
        if toep == 'train':
            return TF1 if infer else TF1X
        if toep == 'plain' or (toep == 'infer' and infer):
            return TF1
    return K3


for _k, (_ci, _ld) in itertools.product((3, 9), ((3, PLAIN), (4, UNSHUFFLE2))):
    _t = 'first %s%s' % (_l(_k, _ci, 40), ' mosaic' if _ld else '')
    for _ar, _tp, _inf in itertools.product(('f16x2', 'f32'), ('0', 'infer', 'train', 'plain'), (False, True)):
        _case('%s %s TOEP_FIRST=%s%s' % (_t, _ar, _tp, ' infer' if _inf else ''), _k, _ci, 40, (3, 13, 68), first_entry(_k, _ar, _tp, _inf),
              load=_ld, epi=RELU, arith=_ar, toep=_tp, infer=_inf)
    for _co, _ar, _inf in itertools.product((20, 64), ('f16x2', 'f32'), (False, True)):
        _t = 'first %s%s' % (_l(_k, _ci, _co), ' mosaic' if _ld else '')
        for _g in ((GEOMS + [FIRST_SMALLEST[_k]]) if _co == 64 and _inf and _k == 9 else [(2, 50, 68), FIRST_SMALLEST[_k]]):
            _case('%s %s%s' % (_t, _ar, ' infer' if _inf else ''), _k, _ci, _co, _g, first_entry(_k, _ar, 'train', _inf), load=_ld, epi=RELU,
                  arith=_ar, infer=_inf)
    for _s, (_ar, _inf) in itertools.product((0, NOBIAS, CASEBIAS, CASEBIAS | RELU, CASEBIAS | RELU | NOBIAS),
                                             (('f16x2', False), ('f16x2', True), ('f32', False)) if _k == 9 else (('f32', False),)):
        _case('first %s%s epi %s %s%s' % (_l(_k, _ci, 20), ' mosaic' if _ld else '', _e(_s), _ar, ' infer' if _inf else ''), _k, _ci, 20,
              (2, 17, 68), first_entry(_k, _ar, 'train', _inf), load=_ld, epi=_s, arith=_ar, infer=_inf)
_case('first many tiles %s infer' % _l(9, 3, 20), 9, 3, 20, MANY, TF1, epi=RELU, infer=True)
_case('first many tiles %s mosaic' % _l(9, 4, 40), 9, 4, 40, (150, 8, 64), TF1X, load=UNSHUFFLE2, epi=RELU)
# what a first layer does not take goes on: a residual / a mask, the backward-data direction
_case('first %s add (not the kernel\'s)' % _l(9, 3, 20), 9, 3, 20, (2, 13, 68), GEN, epi=ADD | RELU)
_case('first %s mask (not the kernel\'s)' % _l(3, 3, 64), 3, 3, 64, (2, 13, 68), W43, epi=MASK)
_case('first backward-data %s' % _l(9, 20, 3), 9, 20, 3, (2, 13, 68), GEN, transpose=True)
_case('first %s below the halo' % _l(9, 3, 20), 9, 3, 20, (2, 7, 68), GEN, epi=RELU)              # h < k - 1

# --- 4 bytes off 16: every vector kernel's layer goes to risp_conv2d, whose staging looks at x and whose stores look at y | add | mask
UNALIGNED = [(3, 17, 33, ADD | MASK, {}), (5, 12, 40, ADD | MASK | RELU, {}), (3, 32, 32, ADD | MASK, dict(scale=True)),
             (5, 32, 64, ADD | RELU, dict(scale=True)), (5, 3, 32, MASK | RELU, {}), (9, 3, 20, CASEBIAS | RELU, dict(infer=True)),
             (9, 4, 64, RELU, dict(load=UNSHUFFLE2)), (3, 3, 64, RELU, {}), (1, 64, 64, ADD, {})]
for _k, _ci, _co, _s, _kw in UNALIGNED:
    for _mis in ('x', 'out') + (('add',) if _s & ADD else ()) + (('mask',) if _s & MASK else ()):
        _case('unaligned %s %s %s' % (_mis, _l(_k, _ci, _co), _e(_s)), _k, _ci, _co, (2, 17, 68), GEN, epi=_s, misalign=_mis, **_kw)

# --- grouped launches: G members of n images through ``stack_packed`` (3x3 layers have none)
for _tag, _k, _ci, _co, _entry, _s, _kw in (
        ('wino45', 5, 12, 40, W45, ADD | RELU, {}), ('f16x2', 5, 32, 32, F16X2, ADD | MASK, dict(scale=True)), ('thin5', 5, 3, 32, THIN5, RELU | MASK, {}),
        ('thin5 backward-data', 5, 3, 64, THIN5, MASK, dict(transpose=True)),
        ('k3', 9, 3, 20, K3, CASEBIAS | RELU, dict(arith='f32')), ('k3 mosaic', 9, 4, 40, K3, RELU, dict(arith='f32', load=UNSHUFFLE2)),
        ('toep_first', 9, 3, 64, TF1, CASEBIAS | RELU, dict(infer=True)), ('toep_first mosaic', 9, 4, 40, TF1, RELU, dict(infer=True, load=UNSHUFFLE2)),
        ('toep_first_exact', 9, 3, 20, TF1X, RELU, {}),
        ('gen 1x1', 1, 64, 64, GEN, ADD | RELU, {}), ('gen', 5, 17, 33, GEN, ADD | MASK, {}),
        ('gen srcnn backward-data', 9, 64, 15, GEN, ADD, dict(transpose=True, add_c=3))):
    for _G, _fl in ((2, 0), (3, SHARED_X), (2, SHARED_ADD), (3, SHARED_X | SHARED_ADD)):
        if _fl & SHARED_ADD and not _s & ADD:
            continue
        _case('grouped %s %s G=%d flags=%d' % (_tag, _l(_k, _ci, _co), _G, _fl), _k, _ci, _co, (2, 13, 68), _entry, epi=_s, group=_G, gflags=_fl,
              table=GROUPED, **_kw)

# --- the contract tests' layers, one per entry: three images for "an inference result does not depend on the batch" (the exact first layer
# is no inference launch: tests/test_conv_reference_cpu.py), two for "a NaN stays under its footprint" (no ReLU, no mask: either would eat it)
BATCH, NANLOC = {}, {}
for _tag, _k, _ci, _co, _entry, _s, _kw in (
        ('gen', 5, 17, 33, GEN, ADD | RELU, {}), ('gen 9x9', 9, 13, 64, GEN, CASEBIAS, {}), ('wino43', 3, 17, 33, W43, RELU, {}),
        ('wino43 b2', 3, 64, 64, W43, ADD, dict(arith='f32')), ('wino45', 5, 12, 40, W45, ADD | RELU, {}),
        ('f16x2', 3, 64, 64, F16X2, ADD | RELU, dict(scale=True)), ('f16x2 5x5', 5, 32, 32, F16X2, RELU, dict(scale=True)),
        ('thin5', 5, 3, 32, THIN5, RELU, {}), ('k3', 9, 3, 20, K3, CASEBIAS | RELU, dict(arith='f32')),
        ('k3 3x3 mosaic', 3, 4, 40, K3, RELU, dict(load=UNSHUFFLE2)), ('toep_first', 9, 3, 20, TF1, CASEBIAS | RELU, {}),
        ('toep_first mosaic', 9, 4, 40, TF1, RELU, dict(load=UNSHUFFLE2))):
    for _g in ((3, 50, 68), (3, 13, 132)):
        _case('batch %s %s' % (_tag, _l(_k, _ci, _co)), _k, _ci, _co, _g, _entry, epi=_s, infer=True, table=BATCH, **_kw)
NAN_AT = (1, 9, 70)                                                           # image, row, column of the NaN (in channel cin // 2)
for _tag, _k, _ci, _co, _entry, _kw in (
        ('gen', 5, 17, 33, GEN, {}), ('wino43', 3, 17, 33, W43, {}), ('wino45', 5, 12, 40, W45, {}), ('f16x2', 3, 64, 64, F16X2, {}),
        ('thin5', 5, 3, 32, THIN5, {}), ('k3', 9, 3, 20, K3, dict(arith='f32')), ('toep_first', 9, 3, 20, TF1, dict(infer=True)),
        ('toep_first_exact', 9, 3, 20, TF1X, {})):
    _case('nan %s %s' % (_tag, _l(_k, _ci, _co)), _k, _ci, _co, (2, 24, 132), _entry, table=NANLOC, **_kw)

SEEDS = int(os.environ.get('RISP_TEST_SEEDS', '8'))
WALK_LAYERS = ([(k, ci, co) for _, k, ci, co, _ in GEN_LAYERS[:9]] + [(3, ci, co) for ci, co, _ in W43_LAYERS] + [(5, ci, co) for ci, co, _ in W45_LAYERS]
               + F16_LAYERS + [(5, 3, 32), (5, 1, 64), (5, 2, 32), (3, 3, 64), (9, 3, 20), (9, 3, 64), (3, 4, 40), (9, 4, 40), (9, 64, 15)])


def walk(seed=20263, draws=4 * SEEDS):
    """a seeded walk over layer x shape x epilogue x direction x mode; ``expect`` None: the test holds the launch to ``route`` and
    ``ENTRY_ACCEPTS`` alone"""
    rng = np.random.default_rng(seed)
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    out = {}
    while len(out) < draws:
        k, cin, cout = pick(WALK_LAYERS)
        n, h, w = pick(GEOMS + ODD + TWO)
        epi = pick(SUBSETS + [NOBIAS, NOBIAS | RELU]) | (SHUFFLE2 if cout % 4 == 0 and rng.random() < 0.1 else 0)
        if epi & SHUFFLE2:
            epi &= ~MASK
        load, tr = PLAIN, bool(rng.random() < 0.3)
        if cin % 4 == 0 and rng.random() < 0.2:
            load = UNSHUFFLE2
        c = {}
        _case('walk %02d %s%s %s' % (len(out), _l(k, cin, cout), ' backward-data' if tr else '', _e(epi)), k, cin, cout, (n, h, w), None, epi=epi,
              add_c=pick((cout, cout, max(1, cout - 1), 3)), load=load, transpose=tr, infer=bool(rng.random() < 0.5),
              arith=pick(('f16x2', 'f16x2', 'f32')), toep=pick(('train', 'train', 'infer', 'plain', '0')), scale=bool(rng.random() < 0.5), table=c)
        out.update(c)
    return out


WALK = walk()
ALL = dict(CASES)
ALL.update(WALK)
EVERY = dict(ALL)
for _t in (GROUPED, BATCH, NANLOC):
    assert not set(_t) & set(EVERY)
    EVERY.update(_t)


# ----------------------------------------------------------------------------------------------------------------------------
# inputs and the restatement
def _rnd(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def hash_name(name):
    v = 0
    for ch in name.encode():
        v = (v * 131 + ch) % (2 ** 31 - 1)
    return v


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = EVERY[name]
    rng = np.random.Generator(np.random.PCG64(hash_name(name)))
    G, n, h, w, k, cin, cout = c['group'] or 1, c['n'], c['h'], c['w'], c['k'], c['cin'], c['cout']
    nx, na = (n if c['gflags'] & SHARED_X else G * n), (n if c['gflags'] & SHARED_ADD else G * n)
    shape = (cin, cout, k, k) if c['transpose'] else (cout, cin, k, k)
    # the recipe of the kernels' own files: standard-normal x, 0.05 x standard-normal weights, 0.1 x bias and tables.  The mask is an
    # activation after its ReLU (half its elements are exactly 0: what tells mask > 0 from mask >= 0), the residual standard normal
    d = dict(weights=[_rnd(rng, *shape) * 0.05 for _ in range(G)], bias=[_rnd(rng, shape[0]) * 0.1 for _ in range(G)])
    if c['load'] == UNSHUFFLE2:
        x = _rnd(rng, nx, cin // 4, 2 * h, 2 * w)
    else:
        x = _rnd(rng, nx, c['cin_img'] if c['load'] == CONSTCH else cin, h, w)
    if c['scale']:
        x[:, :x.shape[1] // 2] *= 1e-3
    d['x'] = x
    d['cvals'] = (_rnd(rng, G * n, cin - c['cin_img']) if c['load'] == CONSTCH else
                  _rnd(rng, G * n, cout, k, k) * 0.1 if c['epi'] & CASEBIAS else None)
    d['add'] = _rnd(rng, na, c['add_c'], h, w) if c['epi'] & ADD else None
    d['mask'] = torch.relu(_rnd(rng, G * n, cout, h, w)) if c['epi'] & MASK else None
    return d


def inputs(case):
    """CPU float32 tensors of a case (cached, shared by every test that needs them: do not write into them)"""
    return _inputs(case['name'])


def out_shape(case):
    N, h, w, cout = case['n'] * (case['group'] or 1), case['h'], case['w'], case['cout']
    return (N, cout // 4, 2 * h, 2 * w) if case['epi'] & SHUFFLE2 else (N, cout, h, w)


def shuffle2(z, swapped=False):
    n, c, h, w = z.shape
    v = z.view(n, c // 4, 2, 2, h, w)                       # cout 4 g + 2 i + j
    v = v.permute(0, 1, 4, 3, 5, 2) if swapped else v.permute(0, 1, 4, 2, 5, 3)       # -> (n, g, y, i, x, j)
    return v.reshape(n, c // 4, 2 * h, 2 * w)


def unshuffle2(x):
    n, c, h2, w2 = x.shape
    return x.view(n, c, h2 // 2, 2, w2 // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(n, 4 * c, h2 // 2, w2 // 2)      # plane 4 c + 2 i + j


def border_case(v, L, P):
    return v if v < P else (2 * P - (L - 1 - v) if v >= L - P else P)


def planes_of(case, x, cvals):
    """the load: what the convolution sees"""
    if case['load'] == UNSHUFFLE2:
        return unshuffle2(x)
    if case['load'] == CONSTCH:                              # constants inside the image (the padding of the convolution stays zero)
        n, _, h, w = x.shape
        return torch.cat([x, cvals[:, :, None, None].expand(n, cvals.shape[1], h, w)], 1)
    return x


def reference(case, dtype=torch.float64, algo='direct', wrong=None, pre=False, start=None):
    """the operation of a case in ``dtype`` on the CPU.  ``algo``: 'direct', or 'wino43' / 'wino45' - the convolution through the
    emulation of that kernel (tests/wino_emulate.py) from the pack ``convnets`` builds.  ``wrong``: one of WRONG - the same with one
    deliberate mistake (tests/test_conv_reference_cpu.py shows that the restatement would notice it)"""
    from reconfigisp_amd import convnets as CN
    d, k, cout, n, h, w = inputs(case), case['k'], case['cout'], case['n'], case['h'], case['w']
    outs = []
    for g in range(case['group'] or 1):
        s = slice(g * n, (g + 1) * n)
        if start is not None:                                   # the cached pre-activation: only ReLU, mask and the store are left
            outs.append(_finish(case, start[s], d['mask'][s] if d['mask'] is not None else None, None))
            continue
        x = d['x'][slice(0, n) if case['gflags'] & SHARED_X else s].to(dtype)
        cv = d['cvals'][s].to(dtype) if d['cvals'] is not None else None
        planes, wt = planes_of(case, x, cv), d['weights'][g]
        if wrong == 'flip':
            wt = wt.flip(2, 3)
        if algo == 'wino43':
            z = wino43_emulate(planes, CN.wino43_weights(wt.to(dtype), case['transpose'], 4), 4, cout)
        elif algo == 'wino45':
            z = wino45_emulate(planes, CN.wino45_weights(wt.to(dtype), case['transpose'], 4, 0), 4, cout, 0)
        elif case['transpose']:
            z = TF.conv_transpose2d(planes, wt.to(dtype), padding=k // 2)
        else:
            z = TF.conv2d(planes, wt.to(dtype), padding=k // 2)
        if not (launch_epi(case) & NOBIAS) and wrong != 'bias':
            z = z + d['bias'][g].to(dtype).view(1, -1, 1, 1)
        if case['epi'] & CASEBIAS:
            iy = torch.tensor([border_case(y, h, k // 2) for y in range(h)])
            ix = torch.tensor([border_case(xx, w, k // 2) for xx in range(w)])
            if wrong == 'case_swapped':
                iy, ix = (torch.tensor([border_case(y, w, k // 2) for y in range(h)]).clamp(0, k - 1),
                          torch.tensor([border_case(xx, h, k // 2) for xx in range(w)]).clamp(0, k - 1))
            z = z + cv[:, :, iy][:, :, :, ix]
        if wrong == 'relu_first' and case['epi'] & RELU:
            z = torch.relu(z)
        if case['epi'] & ADD:
            a, c = d['add'][slice(0, n) if case['gflags'] & SHARED_ADD else s].to(dtype), case['add_c']
            if wrong == 'add_all':
                z = z + a[:, [co % c for co in range(cout)]]
            else:
                z = torch.cat([z[:, :c] + a, z[:, c:]], 1)
        outs.append(z if pre else _finish(case, z, d['mask'][s] if d['mask'] is not None else None, wrong))
    return torch.cat(outs)


def _finish(case, z, m, wrong):
    if case['epi'] & RELU and wrong != 'relu_first':
        z = torch.relu(z)
    if case['epi'] & MASK:
        z = z * ((m >= 0) if wrong == 'mask_ge' else (m > 0)).to(z.dtype)
    if case['epi'] & SHUFFLE2:
        z = shuffle2(z, swapped=wrong == 'shuffle')
    return z


@functools.lru_cache(maxsize=None)
def _pre64(name):
    return reference(EVERY[name], torch.float64, pre=True)


@functools.lru_cache(maxsize=None)
def _ref64(name):
    return reference(EVERY[name], torch.float64, start=_pre64(name))


def ref64(case):
    """the float64 restatement, computed once per case and shared (do not write into it)"""
    return _ref64(case['name'])


def pre64(case):
    """the float64 pre-activation of a case (bias, table and residual in; ReLU and mask not yet), in the layout of the output"""
    z = _pre64(case['name'])
    return shuffle2(z) if case['epi'] & SHUFFLE2 else z


def algo_of(entry):
    """the algorithm class of an entry: its float32 yardstick"""
    return {W43: 'wino43', W45: 'wino45'}.get(entry, 'direct')


@functools.lru_cache(maxsize=None)
def _e32(name, algo):
    ref = _ref64(name)
    return (reference(EVERY[name], torch.float32, algo).double() - ref).abs().max().item() / (ref.abs().max().item() or 1.0)


def E32(case, entry=None):
    """max|e32 - ref64| / max|ref64|: what float32 arithmetic costs on this case in the algorithm class of ``entry`` (default: the entry
    the case expects, or the one ``routed`` names under the case's own switches - the caller sets them)"""
    entry = entry or case['expect'] or routed(case)
    return _e32(case['name'], algo_of(entry))


# deliberate mistakes and the cases that have the feature each one touches
WRONG = {
    'flip': lambda c: c['k'] > 1,                                                 # taps flipped
    'bias': lambda c: not (launch_epi(c) & NOBIAS),                               # bias dropped
    'add_all': lambda c: bool(c['epi'] & ADD) and c['add_c'] < c['cout'],         # residual added to all couts instead of add_c
    'relu_first': lambda c: (c['epi'] & (ADD | RELU)) == (ADD | RELU),            # ReLU before the residual
    'mask_ge': lambda c: bool(c['epi'] & MASK),                                   # mask applied as >= 0
    'shuffle': lambda c: bool(c['epi'] & SHUFFLE2),                               # the two sub-pixel indices swapped
    'case_swapped': lambda c: bool(c['epi'] & CASEBIAS) and c['h'] != c['w'],     # the row's case taken from the width and the reverse
}
