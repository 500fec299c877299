"""CPU: the float64 restatement of the fused stencil segment (tests/fused_segment_reference.py) against oracle/isp_oracle.py
run in float64, the coverage of the sweep table of tests/test_gpu_fused_segment.py, and the tie budget (TAU) that file
grants the HIP kernels - measured here on the fp32 oracle, not on the kernel."""
import os

import numpy as np
import pytest
import torch

import fused_segment_reference as R
import isp_oracle as O
import test_gpu_fused_segment as T
from conftest import assert_close

_FUZZ = int(os.environ.get('RISP_TEST_SEEDS', '8'))
_ORACLE_OP = {R.OP_GAMMA: 'gamma', R.OP_GTM_MANUAL: 'gtmmanual', R.OP_WB_QUADRATIC: 'wbquadratic'}


def _oracle_bilateral(case, dtype):
    """the oracle's own pipeline in ``dtype``: (stage list, unquantised bilateral in codes)"""
    idx = case['ref_images']
    x = case['x'][idx].to(dtype)
    stages = []
    if case['from_bayer']:
        x = O.demosaic_nearest(x)
        stages.append(x)
    p = {'window_length': case['window'][idx], 'sigma_color': case['sc'][idx], 'sigma_space': case['ss'][idx]}
    with O.unquantized():
        raw = O.origin_denoise(x * 255.0, 'bilateral', p)
    stages.append(O.origin_denoise(x * 255.0, 'bilateral', p) / 255.0)
    return stages, raw


def _all_cases():
    return [('sweep', i) for i in range(len(T.CASES))] + [('walk', s) for s in range(_FUZZ)]


def _case(kind, i):
    return T.sweep_case(i) if kind == 'sweep' else T.walk_case(i)


@pytest.mark.parametrize('kind,i', _all_cases())
def test_restatement_equals_the_oracle_in_float64(kind, i):
    case = _case(kind, i)
    idx = case['ref_images']
    params = [p[idx] if p is not None else None for p in case['params']]
    ref, raw = R.segment(case['x'][idx], case['from_bayer'], case['window'][idx], case['sc'][idx], case['ss'][idx],
                         case['ops'], params)
    ora, ora_raw = _oracle_bilateral(case, torch.float64)
    k = 0
    if case['from_bayer']:
        assert torch.equal(ref[0], ora[0]), 'demosaic'
        k = 1
    # float64 against float64: the margin only has to absorb the order of summation
    assert (raw - ora_raw).abs().max().item() <= 1e-9
    clear = R.tie_distance(raw) > 1e-6
    assert clear.double().mean().item() > 0.99
    assert torch.equal((ref[k] * 255.0).round()[clear], (ora[k] * 255.0).round()[clear]), 'bilateral codes'
    assert torch.equal(ref[k], R.code(raw) / 255.0)
    for j, (op, p) in enumerate(zip(case['ops'], params)):        # element-wise stages, started from identical inputs
        src, got = ref[k + j], ref[k + j + 1]
        if op == R.OP_SKIP:
            assert got is src
        elif op == R.OP_WB_MANUAL:
            assert_close(got, O.apply_op('wbmanual', src, p.double() / 5.0), what='wb_manual')
        elif op == R.OP_GAIN3:
            assert_close(got, (src * p.double().view(-1, 3, 1, 1)).clamp(0, 1), what='gain3')
        else:
            assert_close(got, O.apply_op(_ORACLE_OP[op], src, p.double()), what=R.OP_NAMES[op])


def test_gain3_with_grayworld_gains_is_the_oracles_grayworld():
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).uniform(0.01, 1.0, size=(3, 3, 10, 12)))
    m = x.mean(dim=(2, 3))
    gains = m.mean(dim=1, keepdim=True) / m.clamp_min(O.GRAY_EPS)
    assert_close(R.elementwise(R.OP_GAIN3, x, gains), O.grayworld(x), what='grayworld')


def test_restatement_on_hand_computed_values():
    """a 2 x 4 mosaic small enough to follow by hand: the demosaic index map, reflect-101, the rounding rule"""
    bay = torch.tensor([[[[0.1, 0.2, 0.5, 0.6], [0.3, 0.4, 0.7, 0.8]]]], dtype=torch.float64)
    dem = R.demosaic(bay)[0]
    assert dem[2].tolist() == [[0.1, 0.1, 0.5, 0.5]] * 2                     # R
    assert dem[1].tolist() == [[0.2, 0.2, 0.6, 0.6], [0.3, 0.3, 0.7, 0.7]]     # G1 on the even row, G2 on the odd row
    assert dem[0].tolist() == [[0.4, 0.4, 0.8, 0.8]] * 2                     # B
    assert R._reflect101(np.arange(-2, 6), 4).tolist() == [2, 1, 0, 1, 2, 3, 2, 1]
    assert R.code(torch.tensor([-3.0, 0.49, 0.5, 1.5, 254.5, 300.0], dtype=torch.float64)).tolist() == [0, 0, 1, 2, 255, 255]
    assert R.tie_distance(torch.tensor([-1.0, 0.5, 2.25, 256.0], dtype=torch.float64)).tolist() == [1.5, 0.0, 0.25, 1.5]
    # sigma_color huge, sigma_space huge: the 3 x 3 box mean with reflected borders; one pixel by hand
    v = torch.arange(12, dtype=torch.float64).view(1, 1, 3, 4).repeat(1, 3, 1, 1)
    raw = R.bilateral_raw(v, [3], [1e9], [1e9])
    assert abs(raw[0, 0, 0, 0].item() - (5 + 4 + 5 + 1 + 0 + 1 + 5 + 4 + 5) / 9.0) < 1e-9
    assert abs(raw[0, 1, 1, 1].item() - 5.0) < 1e-9


def test_sweep_covers_every_pair():
    fam_of = {}
    for c in T.CASES:
        shape, kind, win, tail, samples, s0 = c
        n = T.SHAPES[shape][0]
        mw, pattern = T.WINDOWS[win]
        for fam, aligned in T.forms(shape, kind, mw):
            f = fam_of.setdefault(fam, dict(shape=set(), tail=set(), win=set(), samples=set(), sigma=set(), input=set()))
            f['shape'].add(shape), f['tail'].add(tail), f['win'].add(win), f['samples'].add(samples)
            f['sigma'].update((s0 + i) % len(T.SIGMAS) for i in range(n))
            f['input'].add((kind, aligned))
            assert all(min(T.SHAPES[shape][1:]) > k // 2 for k in pattern + [mw])      # the header's guard
    assert set(fam_of) == {'quad', 'lds1', 'lds0'}
    common = set(T.SHAPES) - {'64x256x256', '1x10x12', '1x12x16'}
    for fam, f in fam_of.items():
        assert f['tail'] == set(T.TAILS), (fam, set(T.TAILS) - f['tail'])
        assert f['shape'] >= common, (fam, common - f['shape'])
        assert f['samples'] == set(T.SAMPLES), fam
        assert f['sigma'] == set(range(len(T.SIGMAS))), fam
    assert '64x256x256' in fam_of['quad']['shape'] and {'1x10x12', '1x12x16'} <= fam_of['lds0']['shape']
    assert fam_of['quad']['win'] == fam_of['lds1']['win'] == {'1/mw3', '3', '1-3'}
    assert fam_of['lds0']['win'] == {'1/mw1', '5', '3-5-7', '9', '17'}
    assert fam_of['quad']['input'] == {('mosaic', True)}
    assert fam_of['lds1']['input'] == {('mosaic', False), ('bgr', True)}
    assert fam_of['lds0']['input'] == {('mosaic', True), ('mosaic', False), ('bgr', True)}
    assert sum(1 for c in T.CASES if c[0] == '64x256x256') == 1
    sizes = sorted(len(t) for t in T.TAILS.values())
    assert sizes[0] == 0 and sizes[-1] == 8


def measure_e32(case):
    """{window: largest |v32 - v64| in codes} of the oracle's bilateral on one case, and its float32 codes"""
    (_, raw32), (_, raw64) = _oracle_bilateral(case, torch.float32), _oracle_bilateral(case, torch.float64)
    err = (raw32.double() - raw64).abs().flatten(1).max(dim=1).values
    out = {}
    for k, e in zip(case['window'][case['ref_images']].tolist(), err.tolist()):
        out[k] = max(out.get(k, 0.0), e)
    return out, O._code(raw32).double()


def test_recorded_e32_is_the_fp32_oracles_error_on_the_sweep():
    """E32 of the GPU file, measured again: the largest |v32 - v64| of the oracle's bilateral per window size over the
    sweep's inputs (25 % either way for another CPU's exp and summation order); TAU is twice it."""
    assert all(T.TAU[k] == 2.0 * T.E32[k] for k in T.E32)
    worst = {}
    for i in range(len(T.CASES)):
        for k, e in measure_e32(T.sweep_case(i))[0].items():
            worst[k] = max(worst.get(k, 0.0), e)
    print({k: '%.4e' % v for k, v in sorted(worst.items())})
    assert set(worst) == set(T.E32)
    for k, e in worst.items():
        assert T.E32[k] / 1.25 <= e <= T.E32[k] * 1.25, 'window %d: measured %.3e, recorded %.3e' % (k, e, T.E32[k])


@pytest.mark.parametrize('kind,i', _all_cases())
def test_fp32_oracle_passes_the_tie_rule(kind, i):
    """The float32 oracle itself passes the GPU file's bilateral rule against the restatement with the chosen TAU - codes
    differ by at most 1, only within TAU of a rounding boundary, on at most TIE_CAP of the codes - and the input leaves
    at most TIE_CAP of its codes within TAU of a boundary at all."""
    case = _case(kind, i)
    _, codes32 = measure_e32(case)
    idx = case['ref_images']
    _, raw = R.segment(case['x'][idx], case['from_bayer'], case['window'][idx], case['sc'][idx], case['ss'][idx], [], [])
    d = (codes32 - R.code(raw)).abs()
    tau = torch.tensor([T.TAU[int(k)] for k in case['window'][idx]], dtype=torch.float64).view(-1, 1, 1, 1)
    assert d.max().item() <= 1
    assert not ((d > 0) & (R.tie_distance(raw) > tau)).any().item()
    assert (d > 0).double().mean().item() <= T.TIE_CAP
    share = T.near_tie_share(case)
    print('%s: %.3e of the codes within TAU of a rounding boundary' % (case['what'], share))
    assert share <= T.TIE_CAP
