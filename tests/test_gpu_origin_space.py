"""GPU: the classical Origin kernels (risp_origin.hip: 13 kernels behind risp_origin_demosaic / _bilateral / _median /
_fastnlm / _tonemap) over their argument space, against the float64 restatement of tests/origin_reference.py.

The table, the inputs, the yardstick and the rule are plain CPU code in tests/origin_space_cases.py (checked without a
GPU by tests/test_origin_reference_cpu.py).  Every case of the table (and of the seeded walk) is launched through the
C ABI into NaN-filled outputs between guard bands (tests/guarded.py), in the code form and in the raw form, each in
every alignment form its arguments admit, and held to:

  1. same bits across forms: the aligned call (the 4-pixel kernels where W % 4 == 0), the output moved by one float and
     the input moved by one float (the general kernels) - risp_origin.hip's "the two forms give identical bits" - and
     the same bits through the reconfigisp_amd.functional wrappers, odd shapes included;
  2. raw form (out_div < 0) against float64: |got x |out_div| - ref64| <= TAU codes per family and size (beyond the
     8-bit range relative to the value, origin_space_cases.raw_error); the identity cases (search 1) are the input exactly;
  3. code form against float64: no code off by more than 1, a code differs only where tie_distance(ref64) <= TAU, at
     most TIE_CAP of a case's codes differ, none at all for constant inputs, identities and the integer-code
     demosaics; the stored value is fp32(code) x fp32(1 / out_div) to the bit and the code is floor(clamp(raw form, 0,
     255) + 0.5) of the kernel's own raw output;
  4. median: equal to the restatement, stored as code x fp32(1 / |out_div|) in both forms;
  5. the REFUSED table: raised before a launch, the output untouched.

Constant inputs are held exactly in the CODE form: in the raw form a weighted mean sum(w c) x (1 / sum(w)) of a
constant c is c only to an fp32 rounding or two, in any arithmetic - there the bound is TAU like everywhere else.

RISP_BUDGET_REPORT=1 prints per family the case count, the largest raw error, its ratio to TAU and the largest
tie-excused share (profiles/origin_space_budget.txt).  RISP_TEST_SEEDS sets the length of the walk.
"""
import ctypes as C
import os

import pytest
import torch

import origin_reference as R
import origin_space_cases as S
from guarded import Guarded, off16

pytestmark = pytest.mark.gpu

BUDGET = {}                      # family -> [cases, largest raw error, largest ratio to TAU, largest tie-excused share]
_TONE_OPTION = {R.REINHARD: ('reinhard', 'white_point', 'middle_grey'), R.CRYSIS: ('crysisengine', 'lum_adapted', None),
                R.FILMIC: ('filmic', 'white_point', 'exposure_bias')}


@pytest.fixture(scope='module', autouse=True)
def _budget_report():
    yield
    if os.environ.get('RISP_BUDGET_REPORT') == '1':
        print('\nBUDGET %-22s %6s %12s %8s %10s %12s' % ('family / size', 'cases', 'raw err', 'TAU', 'ratio', 'tie share'))
        for key in sorted(BUDGET, key=str):
            n, err, ratio, share = BUDGET[key]
            t = 0.0 if key[0] == 'median' else S.tau(*key)
            print('BUDGET %-22s %6d %12.3e %8.2e %10.3f %12.2e' % ('%s %s' % key, n, err, t, ratio, share))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _device_args(case):
    """the per-image parameter arrays of a case on the device"""
    keys = {'bilateral': ('window', 'sc', 'ss'), 'fastnlm': ('block', 'search', 'decay'), 'tonemap': ('a', 'b')}
    return {k: (case[k].cuda() if case[k] is not None else None) for k in keys.get(case['entry'], ())}


def launch(case, d, x, y, od):
    """one C ABI call of the case: input x, output y, out_div od"""
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    n, h, w = case['shape']
    e, si, st = case['entry'], case['si'], F._stream()
    if e == 'demosaic':
        L.call('risp_origin_demosaic', _p(x), _p(y), case['laplacian'], n, h, w, si, od, st)
    elif e == 'bilateral':
        L.call('risp_origin_bilateral', _p(x), _p(y), _p(d['window']), _p(d['sc']), _p(d['ss']), case['max_window'], n, h, w,
               si, od, st)
    elif e == 'median':
        L.call('risp_origin_median', _p(x), _p(y), case['size'], n, h, w, si, od, st)
    elif e == 'fastnlm':
        L.call('risp_origin_fastnlm', _p(x), _p(y), _p(d['block']), _p(d['search']), _p(d['decay']), case['max_block'],
               case['max_search'], n, h, w, si, od, st)
    else:
        stats = F.channel_stats(x, want_arg=False)[0] if case['mode'] == R.WHITEWORLD else None
        ws = torch.empty(L.load().risp_origin_tonemap_scratch_floats(n), device='cuda')
        L.call('risp_origin_tonemap', _p(x), _p(y), case['mode'], _p(d['a']), _p(d['b']), _p(stats), _p(ws), n, h * w, si,
               od, st)


def through_wrapper(case, d, x, od):
    import reconfigisp_amd.functional as F
    e, sc = case['entry'], (case['si'], od)
    if e == 'demosaic':
        return F.origin_demosaic(x, 'laplacian' if case['laplacian'] else 'bilinear', sc)
    if e == 'bilateral':
        return F.origin_denoise(x, 'bilateral', {'window_length': d['window'], 'sigma_color': d['sc'], 'sigma_space': d['ss'],
                                                 'max_window': case['max_window']}, sc)
    if e == 'median':
        return F.origin_denoise(x, 'median', {'size': case['size']}, sc)
    if e == 'fastnlm':
        return F.origin_denoise(x, 'fastnlm', {'block_size': d['block'], 'search_block': d['search'], 'decay_factor': d['decay'],
                                               'max_block': case['max_block'], 'max_search': case['max_search']}, sc)
    if case['mode'] == R.WHITEWORLD:
        return F.origin_whiteworld(x, d['a'], sc)
    option, ka, kb = _TONE_OPTION[case['mode']]
    return F.origin_tonemap(x, option, {ka: d['a'], **({kb: d['b']} if kb else {})}, sc)


def run_case(case):
    what, (n, h, w) = case['what'], case['shape']
    x = case['x'].cuda()
    assert x.data_ptr() % 16 == 0
    d = _device_args(case)
    oshape = (n, 3, h, w)
    failed, stored = [], {}
    # (name, input moved by, output moved by): risp_origin_tonemap refuses the moved pointers (the REFUSED table)
    forms = [('aligned', 0, 0)] + ([('output + 1 float', 0, 1), ('input + 1 float', 1, 0)] if case['entry'] != 'tonemap' else [])
    for sign in (1.0, -1.0):
        od, outs = sign * case['si'], []
        for name, xoff, yoff in forms:
            g = Guarded(*oshape, off=yoff)
            launch(case, d, off16(x, xoff) if xoff else x, g.t, od)
            torch.cuda.synchronize()
            if not g.bands_intact():
                failed.append('%s [%s, out_div %g]: wrote outside the output' % (what, name, od))
            outs.append(g.t.clone())
        for (name, _, _), o in zip(forms[1:], outs[1:]):
            if not torch.equal(outs[0], o):               # NaN (unwritten) never compares equal
                failed.append('[1: bits across forms] %s out_div %g: aligned and %s differ in %d elements' % (
                    what, od, name, int((outs[0] != o).sum())))
        wrapped = through_wrapper(case, d, x, od)
        if not torch.equal(outs[0], wrapped):
            failed.append('[1: bits across forms] %s out_div %g: the wrapper differs in %d elements' % (
                what, od, int((outs[0] != wrapped).sum())))
        stored[sign] = outs[0].cpu()
    bad, fig = S.judge(case, stored[-1.0], stored[1.0])
    failed += bad
    print('%s: raw error %.3e codes (%.3f of TAU), %.2e of the codes differ' % (what, fig['raw_err'], fig['ratio'], fig['share']))
    for key in set(case['keys']):
        BUDGET.setdefault(key, [0, 0.0, 0.0, 0.0])[0] += 1
    for key, (err, ratio, share) in zip(case['keys'], fig['images']):
        b = BUDGET[key]
        b[1], b[2], b[3] = max(b[1], err), max(b[2], ratio), max(b[3], share)
    assert not failed, '%d checks failed:\n  %s' % (len(failed), '\n  '.join(failed))


def _params(entry):
    return [pytest.param(entry, i, si, id=S.case_id(entry, i, si)) for i, si in S.all_cases(entry)]


@pytest.mark.parametrize('entry,index,si', [p for e in S.ENTRIES for p in _params(e)])
def test_table(entry, index, si):
    run_case(S.table_case(entry, index, si))


@pytest.mark.parametrize('seed', range(S.FUZZ))
def test_random_walk(seed):
    run_case(S.walk_case(seed))


# ---------------------------------------------------------------------------------------------------- refusals
def _refused_abi(entry, ov):
    """a valid 1 x 3 x 16 x 16 call with the named arguments replaced -> (the call, its guarded output)"""
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    dev = 'cuda'
    a = dict(N=1, H=16, W=16, x=torch.full((1, 3, 16, 16), 0.5, device=dev), max_window=3, size=3, max_block=3, max_search=3,
             mode=1, HW=256, window=torch.tensor([3], dtype=torch.int32, device=dev), sc=torch.tensor([10.0], device=dev),
             ss=torch.tensor([10.0], device=dev), block=torch.tensor([3], dtype=torch.int32, device=dev),
             search=torch.tensor([3], dtype=torch.int32, device=dev), decay=torch.tensor([10.0], device=dev),
             a=torch.tensor([0.5], device=dev), b=torch.tensor([0.5], device=dev), stats=torch.ones(1, 3, 4, device=dev),
             scratch=torch.zeros(L.load().risp_origin_tonemap_scratch_floats(1), device=dev))
    g = Guarded(1, 3, 16, 16, off=ov.get('y_off', 0))
    a['y'] = g.t
    if 'x_off' in ov:
        a['x'] = off16(a['x'], ov['x_off'])
    a.update({k: v for k, v in ov.items() if k not in ('x_off', 'y_off')})
    st, p = F._stream(), lambda k: _p(a[k])
    call = {
        'demosaic': lambda: L.call('risp_origin_demosaic', p('x'), p('y'), 0, a['N'], a['H'], a['W'], 1.0, 1.0, st),
        'bilateral': lambda: L.call('risp_origin_bilateral', p('x'), p('y'), p('window'), p('sc'), p('ss'), a['max_window'], a['N'],
                                    a['H'], a['W'], 1.0, 1.0, st),
        'median': lambda: L.call('risp_origin_median', p('x'), p('y'), a['size'], a['N'], a['H'], a['W'], 1.0, 1.0, st),
        'fastnlm': lambda: L.call('risp_origin_fastnlm', p('x'), p('y'), p('block'), p('search'), p('decay'), a['max_block'],
                                  a['max_search'], a['N'], a['H'], a['W'], 1.0, 1.0, st),
        'tonemap': lambda: L.call('risp_origin_tonemap', p('x'), p('y'), a['mode'], p('a'), p('b'), p('stats'), p('scratch'),
                                  a['N'], a['HW'], 1.0, 1.0, st),
    }[entry]
    return call, g, a


def _refused_wrapper(entry, ov):
    import reconfigisp_amd.functional as F
    x = torch.full(ov.get('shape', (1, 3, 16, 16)), 0.5, device='cuda')
    one = torch.tensor([0.5], device='cuda')
    if entry == 'median':
        return lambda: F.origin_denoise(x, 'median', {'size': ov.get('size', 3)})
    if entry == 'bilateral':
        return lambda: F.origin_denoise(x, 'bilateral', {'window_length': torch.tensor([ov.get('window', 3)]), 'sigma_color': one * 20,
                                                         'sigma_space': one * 20, 'max_window': ov.get('max_window')})
    if entry == 'fastnlm':
        return lambda: F.origin_denoise(x, 'fastnlm', {'block_size': torch.tensor([3]), 'search_block': torch.tensor([3]),
                                                       'decay_factor': one * 20, 'max_block': ov.get('max_block'),
                                                       'max_search': ov.get('max_search')})
    if entry == 'tonemap':
        return lambda: F.origin_tonemap(x, 'crysisengine', {'lum_adapted': one})
    return lambda: F.origin_whiteworld(x, one)


@pytest.mark.parametrize('row', range(len(S.REFUSED)), ids=lambda i: '%s-%s-%s' % (S.REFUSED[i][0], S.REFUSED[i][1], '_'.join(
    '%s=%s' % (k, v if not isinstance(v, tuple) else 'x'.join(map(str, v))) for k, v in S.REFUSED[i][2].items())))
def test_refused_arguments_raise_before_any_launch(row):
    from reconfigisp_amd import lib as L
    how, entry, ov, needle = S.REFUSED[row]
    if how == 'abi':
        call, g, keep = _refused_abi(entry, ov)
        with pytest.raises(RuntimeError, match=needle):
            call()
        torch.cuda.synchronize()
        assert g.untouched(), 'the refused call wrote its output'
        return
    call = _refused_wrapper(entry, ov)
    before, L.CALLS = L.CALLS, {}
    try:
        with pytest.raises(ValueError, match=needle):
            call()
        assert not [k for k in L.CALLS if k.startswith('risp_origin')], 'the refused call reached an entry point: %s' % L.CALLS
    finally:
        L.CALLS = before


# ---------------------------------------------------------------------------------------------------- the alignment fixes
@pytest.mark.parametrize('off', [1, 2, 3])
def test_misaligned_views_through_the_tone_wrappers(off):
    """risp_origin_tonemap reads 16-byte vectors and refuses a misaligned pointer (REFUSED); the wrappers copy a
    contiguous view whose storage offset is no multiple of 4 floats to a fresh tensor.  The view's result has the bits
    of the aligned call and passes the rule against float64."""
    import reconfigisp_amd.functional as F
    for mode in range(4):
        index = [i for i, row in enumerate(S.TONEMAP) if row[0] == (1, 34, 132) and row[1] == mode][0]
        case = S.table_case('tonemap', index, 255.0)
        x, d = case['x'].cuda(), _device_args(case)
        v = off16(x, off)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
        out = {}
        for sign in (1.0, -1.0):
            out[sign] = through_wrapper(case, d, v, sign * case['si'])
            assert torch.equal(out[sign], through_wrapper(case, d, x, sign * case['si'])), case['what']
        bad, _ = S.judge(case, out[-1.0].cpu(), out[1.0].cpu())
        assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('shape', [(2, 3, 34, 132), (1, 3, 1, 4), (3, 1, 16, 64)])
@pytest.mark.parametrize('off', [1, 2, 3])
def test_channel_stats_on_a_misaligned_view(shape, off):
    """risp_channel_stats takes the element loads when x is not 16-byte aligned.  Min, max and their first indices are
    those of the aligned call and of float64; the sum is added in another order, so it may differ from the aligned
    call's in the last bits: it is held to float64 at the rounding bound of its own summation tree."""
    import numpy as np
    import reconfigisp_amd.functional as F
    rng = np.random.Generator(np.random.PCG64(31 + off))
    x = torch.from_numpy(rng.uniform(-40.0, 300.0, size=shape).astype(np.float32))
    xd = x.cuda()
    v = off16(xd, off)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    (sa, aa), (sv, av) = F.channel_stats(xd), F.channel_stats(v)
    n, c = shape[:2]
    flat = x.double().view(n, c, -1)
    assert torch.equal(sv[..., 0].cpu().double(), flat.min(dim=2).values) and torch.equal(sv[..., 2].cpu().double(), flat.max(dim=2).values)
    assert torch.equal(sv[..., [0, 2, 3]], sa[..., [0, 2, 3]]) and torch.equal(av, aa)
    first = lambda m: (flat == m.unsqueeze(-1)).int().argmax(dim=2)          # the first index of the extreme
    assert torch.equal(av[..., 0].cpu().long(), first(flat.min(dim=2).values)) and torch.equal(av[..., 1].cpu().long(), first(flat.max(dim=2).values))
    # the element-load kernel: one workgroup per plane below 16384 pixels, every thread adds ceil(HW / 256) values in a
    # row, then 6 shuffle steps, 3 adds across the waves and 6 steps of the final kernel: each addition costs at most
    # 2^-24 of the sum of the magnitudes
    want, mags = flat.sum(dim=2), flat.abs().sum(dim=2)
    adds = -(-flat.shape[2] // 256) + 15
    err = (sv[..., 1].cpu().double() - want).abs()
    assert flat.shape[2] < 16384 and (err <= adds * 2.0 ** -24 * mags).all(), 'sum: %s beyond %d roundings' % (err.tolist(), adds)
