"""CPU: the float64 restatement of the classical Origin kernels (tests/origin_reference.py), the table of
tests/origin_space_cases.py and the rule of tests/test_gpu_origin_space.py, checked without a GPU:

  * the restatement agrees with the oracle (oracle/isp_oracle.py on float64 tensors, unquantized) to 1e-9 codes, the
    median exactly, and with hand-worked vectors;
  * E32, the yardstick of the tie budget, is what the float32 restatement costs on the inputs of the table - measured
    here, never from a kernel - and the float32 restatement itself passes the GPU rule on every input;
  * every input keeps the share of near-tie codes under TIE_CAP;
  * the table reaches every kernel instantiation in both forms;
  * the rule rejects every listed wrong reading of the OPSPEC.
"""
import math

import numpy as np
import pytest
import torch

import fused_segment_reference as FS
import isp_oracle as O
import origin_reference as R
import origin_space_cases as S

_CASES = {}


def cases(entry):
    """every table case of an entry point, built once: [(index, si, case)]"""
    if entry not in _CASES:
        _CASES[entry] = [(i, si, S.table_case(entry, i, si)) for i, si in S.all_cases(entry)]
    return _CASES[entry]


def stored(case, value):
    """what a kernel computing ``value`` in front of the clip-and-round would store: (raw form, code form)"""
    if case['entry'] == 'median':
        return R.stored_code(value, case['si']), R.stored_code(value, case['si'])
    return R.stored_raw(value, case['si']), R.stored_code(R.code(value.float().double()), case['si'])


# ---------------------------------------------------------------------------------------------------- against the oracle
def _oracle(case):
    v = R.scaled(case['x'], case['si'])
    e = case['entry']
    with O.unquantized():
        if e == 'demosaic':
            return O.origin_demosaic(v, 'laplacian' if case['laplacian'] else 'bilinear')
        if e == 'bilateral':
            return O.origin_denoise(v, 'bilateral', {'window_length': case['window'], 'sigma_color': case['sc'].double(),
                                                     'sigma_space': case['ss'].double()})
        if e == 'median':
            return O.origin_denoise(v, 'median', {'size': case['size']})
        if e == 'fastnlm':
            return O.origin_denoise(v, 'fastnlm', {'block_size': case['block'], 'search_block': case['search'],
                                                   'decay_factor': case['decay'].double()})
        a = case['a'].double().numpy()
        if case['mode'] == R.WHITEWORLD:
            return O.origin_whiteworld(v, a)
        b = case['b'].double().numpy() if case['b'] is not None else None
        params = {R.REINHARD: {'white_point': a, 'middle_grey': b}, R.CRYSIS: {'lum_adapted': a},
                  R.FILMIC: {'white_point': a, 'exposure_bias': b}}[case['mode']]
        return O.origin_tonemap(v, {R.REINHARD: 'reinhard', R.CRYSIS: 'crysisengine', R.FILMIC: 'filmic'}[case['mode']], params)


@pytest.mark.parametrize('entry', S.ENTRIES)
def test_restatement_agrees_with_the_oracle(entry):
    """a subset of the table: every third case, and every case of the smallest admitted shapes up to radius 4"""
    worst = 0.0
    for k, (index, si, case) in enumerate(cases(entry)):
        n, h, w = case['shape']
        if k % 3 and not (h <= 5 and w <= 8):
            continue
        if entry == 'fastnlm' and max(case['max_block'], case['max_search']) > 9 and k % 2:
            continue
        want, got = _oracle(case), S.ref64(case)
        if entry == 'median':
            assert torch.equal(got, want), case['what']
            continue
        err = S.raw_error(got, want).max().item()
        worst = max(worst, err)
        assert err <= 1e-9, '%s: %.3e codes from the oracle' % (case['what'], err)
    print('%s: largest distance from the oracle %.3e codes' % (entry, worst))


def test_box_sum_fastnlm_is_the_four_loop_form():
    rng = np.random.Generator(np.random.PCG64(5))
    x = torch.from_numpy(rng.uniform(-40.0, 300.0, size=(3, 3, 5, 6)))
    blk, srch, dec = [3, 1, 5], [3, 5, 1], [8.0, 50.5, 1.0]
    a, b = R.fastnlm(x, blk, srch, dec), R.fastnlm_direct(x, blk, srch, dec)
    assert (a - b).abs().max().item() <= 1e-10
    assert torch.equal(R.bilateral(x, [3, 5, 1], [8.0, 50.0, 1.0], [2.0, 1.0, 9.0]),
                       FS.bilateral_raw(x, [3, 5, 1], [8.0, 50.0, 1.0], [2.0, 1.0, 9.0]))


# ---------------------------------------------------------------------------------------------------- hand-worked vectors
def test_hand_worked_stencils_on_3x3():
    imp = torch.zeros(1, 3, 3, 3, dtype=torch.float64)
    imp[:, :, 1, 1] = 90.0
    # bilateral 3, sigma_color 270 (L1 distance 270 -> exponent -0.5), sigma_space 1: centre 90 / (1 + 4 e^-1 + 4 e^-1.5)
    y = R.bilateral(imp, [3], [270.0], [1.0])
    assert abs(y[0, 0, 1, 1].item() - 90.0 / (1 + 4 * math.exp(-1.0) + 4 * math.exp(-1.5))) < 1e-12
    # the corner (0,0) sees rows {1,0,1} x columns {1,0,1}: the impulse four times, all on diagonals
    assert abs(y[0, 2, 0, 0].item() - 4 * 90.0 * math.exp(-1.5) / (1 + 4 * math.exp(-1.5) + 4 * math.exp(-0.5))) < 1e-12
    # fastnlm block 1, search 3, decay 90: d2 = 3 x 90^2 to the impulse -> weight e^-1
    y = R.fastnlm(imp, [1], [3], [90.0])
    assert abs(y[0, 1, 1, 1].item() - 90.0 / (1 + 8 * math.exp(-1.0))) < 1e-12
    # the edge (0,1) sees rows {1,0,1} x columns {0,1,2}: the impulse twice among 9 taps, 3 taps equal to itself (0)
    assert abs(y[0, 0, 0, 1].item() - 2 * 90.0 * math.exp(-1.0) / (7 + 2 * math.exp(-1.0))) < 1e-12
    # median 3 of 1..9: the centre 5; the corner's window is {1, 2, 2, 4, 4, 5, 5, 5, 5} -> 4; the edge (0,1): rows {1,0,1}
    # of columns 0..2 = {4,5,6, 1,2,3, 4,5,6} -> 4
    ramp = torch.arange(1.0, 10.0, dtype=torch.float64).view(1, 1, 3, 3).repeat(1, 3, 1, 1)
    m = R.median(ramp, 3)
    # (0,2): rows {1,0,1} of columns {1,2,1} = {5,6,5, 2,3,2, 5,6,5} -> 5; the far corner by symmetry 10 - 4
    assert [m[0, 0, 0, 0].item(), m[0, 0, 0, 1].item(), m[0, 0, 0, 2].item(), m[0, 0, 1, 1].item(), m[0, 0, 2, 2].item()] == [4.0, 4.0, 5.0, 5.0, 6.0]
    assert torch.equal(R.median(ramp + 0.5, 3), m + 1.0)        # k + 0.5 rounds UP before the median
    assert torch.equal(R.median(ramp - 400.0, 1), torch.zeros_like(ramp))


def test_hand_worked_demosaic_4x4():
    bay = torch.arange(16.0, dtype=torch.float64).view(1, 1, 4, 4)          # v = 4 y + x
    y = R.demosaic(bay, 0)
    assert y[0, :, 1, 1].tolist() == [5.0, 5.0, 5.0]            # a blue site: G = (1 + 9 + 4 + 6) / 4, R = (0 + 2 + 8 + 10) / 4
    assert y[0, :, 1, 2].tolist() == [6.0, 6.0, 6.0]            # green on the blue row: B = (5 + 7) / 2, R = (2 + 10) / 2
    assert y[0, :, 0, 0].tolist() == [5.0, 2.5, 0.0]            # the red corner: B = 4 x v(1,1) / 4, G = (4 + 4 + 1 + 1) / 4
    assert y[0, :, 0, 1].tolist() == [5.0, 1.0, 1.0]            # green on the red row: R = (0 + 2) / 2, B = (5 + 5) / 2
    z = R.demosaic(bay, 1)
    # the blue site (1,1): c 5, cross 20, diag 20, fh = v(1,1) + v(1,3) = 12, fv = v(1,1) + v(3,1) = 18
    assert z[0, :, 1, 1].tolist() == [5.0, (20 + 40 - 30) / 8, (30 + 40 - 45) / 8]
    # green on the blue row (1,2): c 6, hor 12, ver 12, diag 24, fh = v(1,0) + v(1,2) = 10, fv = v(1,2) + v(3,2) = 20
    assert z[0, :, 1, 2].tolist() == [(30 + 48 - 24 - 10 + 10) / 8, 6.0, (30 + 48 - 24 - 20 + 5) / 8]


def test_hand_worked_curves_on_one_pixel():
    px = torch.tensor([51.0, 102.0, 204.0], dtype=torch.float64).view(1, 3, 1, 1)      # (b, g, r) = (0.2, 0.4, 0.8)
    y = R.tonemap(px, R.CRYSIS, [0.45])                          # 0.5 / (0.45 + 0.05) = 1
    assert np.allclose(y.flatten().tolist(), [255 * (1 - math.exp(-t)) for t in (0.2, 0.4, 0.8)], rtol=0, atol=1e-12)
    L = 0.114 * 0.2 + 0.587 * 0.4 + 0.299 * 0.8
    ls = 0.5 * L / (L + 1e-4)                                    # one pixel: the log-average is L + 1e-4
    ld = ls * (1 + ls / 25.0) / (1 + ls)                         # white_point 0.5 -> Lw = 5
    y = R.tonemap(px, R.REINHARD, [0.5], [0.5])
    assert np.allclose(y.flatten().tolist(), [255 * t * ld / L for t in (0.2, 0.4, 0.8)], rtol=0, atol=1e-11)
    y0 = R.tonemap(px, R.REINHARD, [0.0], [0.0])                 # both clamp at 0.01: key 0.01, Lw 0.1
    ls0 = 0.01 * L / (L + 1e-4)
    assert np.allclose(y0.flatten().tolist(), [255 * t * ls0 * (1 + ls0 / 0.01) / (1 + ls0) / L for t in (0.2, 0.4, 0.8)], rtol=0, atol=1e-11)
    f = lambda t: (t * (0.15 * t + 0.05) + 0.004) / (t * (0.15 * t + 0.5) + 0.06) - 0.02 / 0.3
    y = R.tonemap(px, R.FILMIC, [0.5], [2.0])                    # white 5.6, exposure bias 2
    assert np.allclose(y.flatten().tolist(), [255 * f(2 * t) / f(5.6) for t in (0.2, 0.4, 0.8)], rtol=0, atol=1e-11)
    assert np.allclose(R.whiteworld(px, [1.0]).flatten().tolist(), [204.0] * 3, rtol=0, atol=1e-12)
    assert np.allclose(R.whiteworld(px, [0.5]).flatten().tolist(), [127.5, 153.0, 204.0], rtol=0, atol=1e-12)
    neg = px.clone()
    neg[0, 0] = -7.0                                             # a negative channel: its maximum is floored at 1e-3
    assert np.allclose(R.whiteworld(neg, [1.0]).flatten().tolist(), [-7.0 * 204.0 / 1e-3, 204.0, 204.0], rtol=1e-14, atol=0)
    assert R.tonemap(neg, R.CRYSIS, [0.45])[0, 0].item() == 0.0  # the curves take max(sample, 0)


def test_constants_stay_constant_and_size_1_is_the_identity():
    flat = torch.full((2, 3, 7, 9), 77.0, dtype=torch.float64)
    for y in (R.bilateral(flat, [5, 3], [3.0, 50.0], [2.0, 9.0]), R.fastnlm(flat, [3, 5], [5, 3], [8.0, 1.0]), R.median(flat, 7)):
        assert (y - 77.0).abs().max().item() <= 1e-12
    for lap in (0, 1):
        assert torch.equal(R.demosaic(torch.full((1, 1, 6, 8), 77.0, dtype=torch.float64), lap), torch.full((1, 3, 6, 8), 77.0, dtype=torch.float64))
    for mode, a, b in ((R.REINHARD, [0.3, 0.9], [0.5, 0.1]), (R.CRYSIS, [0.3, 0.9], None), (R.FILMIC, [0.3, 0.9], [2.0, 9.0])):
        y = R.tonemap(flat, mode, a, b)
        assert (y - y[:, :, :1, :1]).abs().max().item() <= 1e-12
    rng = np.random.Generator(np.random.PCG64(6))
    x = torch.from_numpy(rng.uniform(-40.0, 300.0, size=(2, 3, 5, 6)))
    assert torch.equal(R.bilateral(x, [1, 1], [3.0, 50.0], [2.0, 9.0]), x)
    assert torch.equal(R.fastnlm(x, [1, 5], [1, 1], [8.0, 1.0]), x)
    assert torch.equal(R.median(x, 1), R.code(x))
    assert torch.equal(R.whiteworld(x, [0.0, 0.0]), x)


# ---------------------------------------------------------------------------------------------------- E32, the rule on fp32
def test_e32_is_what_the_tables_measure_and_float32_passes_the_rule():
    """E32 re-measured: per family and size the largest |float32 - float64| of the restatement over every input of the
    tables, through the raw store form.  The committed constant is that measurement (25 % either way for another CPU's
    exp and summation order, as tests/test_fused_segment_reference_cpu.py allows).  The float32 restatement, stored as a kernel would store it, must
    pass the rule of the GPU suite on every input: a rule the restatement's own fp32 arithmetic fails would measure
    nothing."""
    measured, failures = {}, []
    for entry in S.ENTRIES:
        for index, si, case in cases(entry):
            v32 = S.reference(case, R.F32)
            raw, cod = stored(case, v32)
            if entry != 'median':
                err = S.raw_error(raw.double() * si, S.ref64(case))
                for i, (fam, size) in enumerate(case['keys']):
                    d = measured.setdefault(fam, {})
                    d[size] = max(d.get(size, 0.0), err[i].max().item())
            failures += S.judge(case, raw, cod)[0]
    for fam in sorted(measured):
        print('E32 %-10s %s' % (fam, ', '.join('%s: %.3e' % kv for kv in sorted(measured[fam].items()))))
    assert not failures, 'the float32 restatement fails the rule:\n  ' + '\n  '.join(failures)
    for fam, sizes in measured.items():
        assert set(sizes) == set(S.E32[fam]), '%s: sizes %s measured, %s committed' % (fam, sorted(sizes), sorted(S.E32[fam]))
        for size, e in sizes.items():
            assert S.E32[fam][size] / 1.25 <= e <= S.E32[fam][size] * 1.25, '%s %s: measured %.4e, committed %.4e' % (fam, size, e, S.E32[fam][size])


def test_every_input_is_under_the_tie_cap():
    """table_case and walk_case draw an input again (8 times at most, then fail) when more than TIE_CAP of the codes of
    the float64 result lie within TAU of a rounding boundary.  Exempt: the medians and the integer-code demosaics, whose
    ties are deliberate and admit no excuse."""
    worst = 0.0
    for entry in S.ENTRIES:
        for index, si, case in cases(entry):
            if entry == 'median' or case.get('exact'):
                continue
            share = S.near_tie_share(case)
            worst = max(worst, share)
            assert share <= S.TIE_CAP, '%s: %.4f%% of the codes within TAU of a tie' % (case['what'], 100 * share)
    for seed in range(S.FUZZ):
        case = S.walk_case(seed)
        if case['entry'] != 'median':
            assert S.near_tie_share(case) <= S.TIE_CAP, case['what']
    print('largest near-tie share of a table input: %.2e' % worst)


# ---------------------------------------------------------------------------------------------------- coverage
def test_the_tables_reach_every_kernel_in_both_forms():
    """every kernel instantiation by at least one case (each case runs in the code form and the raw form), every kernel
    family at both scale magnitudes, and every axis value of the tables"""
    seen = {}
    for entry in S.ENTRIES:
        for index, si, case in cases(entry):
            for aligned in ((True, False) if entry != 'tonemap' else (True,)):
                name = S.kernel_of(case, aligned)
                seen.setdefault(name.split('/')[0], set()).add(si)
                seen.setdefault(name, set()).add(si)
    for name in S.KERNELS + ['fastnlm4<true>/fast', 'fastnlm4<true>/mixed', 'fastnlm4<true>/general']:
        assert seen.get(name), '%s: reached by no case' % name
    for fam in ('bilateral4', 'bilateral', 'median3x4', 'median4', 'median', 'fastnlm4', 'fastnlm', 'demosaic4', 'origin_demosaic', 'tonemap'):
        scales = set().union(*[v for k, v in seen.items() if k.split('<')[0] == fam])
        assert scales == {1.0, 255.0}, '%s: reached at scales %s only' % (fam, sorted(scales))
    assert {k for c in cases('bilateral') for _, k in c[2]['keys']} == set(range(1, 18, 2))
    for entry in ('bilateral', 'median', 'fastnlm'):
        assert {c[2]['shape'] for c in cases(entry)} >= set(S.STENCIL_SHAPES) | {(1, 1, 1)}, entry
    assert {c[2]['shape'] for c in cases('demosaic')} == set(S.DEMOSAIC_SHAPES)
    assert {c[2]['shape'] for c in cases('tonemap')} >= set(S.TONE_SHAPES)
    assert {c[2]['size'] for c in cases('median')} == set(range(1, 18, 2))
    assert {k for c in cases('fastnlm') for _, k in c[2]['keys']} >= set(S.PAIRS)
    both = [c[2] for c in cases('fastnlm') if c[2]['max_block'] // 2 + c[2]['max_search'] // 2 >
            max(b // 2 + s // 2 for b, s in zip(c[2]['block'].tolist(), c[2]['search'].tolist()))]
    assert both, 'no fastnlm batch whose maxima come from different images'
    assert any(c[2]['max_window'] > int(c[2]['window'].max()) for c in cases('bilateral'))
    for entry in S.ENTRIES:                                      # every sample family the entry point admits
        kinds = {c[2]['input'] for c in cases(entry)}
        assert kinds >= set(S.INPUTS), (entry, kinds)
    assert {'zero', 'negchan'} <= {c[2]['input'] for c in cases('tonemap')}
    assert any(c[2]['input'] == 'half' for c in cases('median')) and any(c[2].get('exact') for c in cases('demosaic'))
    for mode, corners in S.TONE_PARAMS.items():                  # every corner of every curve's parameters
        got = {(round(float(a), 3), None if c[2]['b'] is None else round(float(c[2]['b'][i]), 3))
               for c in cases('tonemap') if c[2]['mode'] == mode for i, a in enumerate(c[2]['a'].tolist())}
        assert got >= {(a, b) for a, b in corners}, (mode, got)


# ---------------------------------------------------------------------------------------------------- wrong variants
def _edge_repeat(i, n):                      # -1 -> 0
    i = np.where(i < 0, -i - 1, i)
    return np.where(i >= n, 2 * n - 1 - i, i)


def _clamped(i, n):
    return np.clip(i, 0, n - 1)


def _reflect_then_clamp(i, n):               # the low side reflected, the far side clamped
    return np.clip(np.abs(i), 0, n - 1)


def _half_even(case, v):
    raw = R.stored_raw(v, case['si'])
    return raw, R.stored_code(torch.round(v.clamp(0.0, 255.0)), case['si'])


def _f64_division(case, v):
    return R.stored_raw(v, case['si']), (R.code(v) / case['si']).float()


# name: (entry points, a filter on the case, how the variant's stored pair is made)
_border = lambda fn, only=None: (('bilateral', 'median', 'fastnlm', 'demosaic'), only, ('border', fn))
VARIANTS = {
    'edge-repeating reflection': _border(_edge_repeat),
    'clamped border': _border(_clamped),
    'one reflection, then a clamp, at H = R + 1': _border(_reflect_then_clamp, lambda c: c['entry'] != 'demosaic' and c['shape'][1] == _radius(c) + 1),
    'L2 colour distance': (('bilateral',), None, ('variant', 'l2')),
    'fastnlm without the factor 3': (('fastnlm',), None, ('variant', 'no3')),
    'fastnlm, centre patch not reflected': (('fastnlm',), None, ('variant', 'centre')),
    'fastnlm normalised by the clamped radius (3 x 3 at most)': (('fastnlm',), None, ('variant', 'norm1')),
    'median of unquantised samples': (('median',), None, ('variant', 'unquantised')),
    'round-half-even': (('demosaic', 'median'), None, ('store', _half_even)),
    'rb_hor / rb_ver swapped': (('demosaic',), None, ('variant', 'swap')),
    'RGB output order': (('demosaic',), None, ('variant', 'rgb')),
    'Reinhard without the 1e-4': (('tonemap',), lambda c: c['mode'] == R.REINHARD, ('variant', 'no_eps')),
    'Reinhard with Lw = white_point': (('tonemap',), lambda c: c['mode'] == R.REINHARD, ('variant', 'lw_white')),
    "Hable's white 11.2 dropped": (('tonemap',), lambda c: c['mode'] == R.FILMIC, ('variant', 'no_112')),
    'white-world from means': (('tonemap',), lambda c: c['mode'] == R.WHITEWORLD, ('variant', 'means')),
    'Crysis without the 0.05': (('tonemap',), lambda c: c['mode'] == R.CRYSIS, ('variant', 'no_005')),
    'out_div as a float64 division': (S.ENTRIES, lambda c: c['si'] == 255.0, ('store', _f64_division)),
}


def _radius(c):
    return {'bilateral': lambda: c['max_window'] // 2, 'median': lambda: c['size'] // 2,
            'fastnlm': lambda: c['max_block'] // 2 + c['max_search'] // 2, 'demosaic': lambda: 2}[c['entry']]()


@pytest.mark.parametrize('name', sorted(VARIANTS))
def test_the_rule_rejects_a_wrong_reading(name, monkeypatch):
    """each wrong reading of the OPSPEC, evaluated in float64 and stored as a kernel would store it, in place of the
    device result: the rule must fail on at least one case of the table (and the truth itself must pass there)"""
    entries, only, (kind, arg) = VARIANTS[name]
    rejected = 0
    for entry in entries:
        for index, si, case in cases(entry):
            if only is not None and not only(case):
                continue
            truth = S.ref64(case)
            assert not S.judge(case, *stored(case, truth))[0], 'the truth fails on %s' % case['what']
            if kind == 'border':
                with monkeypatch.context() as m:
                    m.setattr(R, '_reflect101', arg)
                    m.setattr(FS, '_reflect101', arg)
                    pair = stored(case, S.reference(case))
            elif kind == 'variant':
                value = S.reference(case, R.F64, _variant=arg)
                pair = (R.stored_code(value, si),) * 2 if entry == 'median' else stored(case, value)
            else:
                if entry == 'median':
                    v = R.scaled(case['x'], si)              # the rounding under test is the median's input rounding
                    pair = (R.stored_code(R.median(torch.round(v.clamp(0, 255)) if arg is _half_even else v, case['size']), si),) * 2
                    if arg is _f64_division:
                        pair = ((truth / si).float(),) * 2
                else:
                    pair = arg(case, truth)
            rejected += bool(S.judge(case, *pair)[0])
        if rejected:
            break
    assert rejected, '%s: the rule accepts it on every case' % name
