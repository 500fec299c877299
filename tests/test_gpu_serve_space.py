"""GPU: the serving entry points (risp_serve_u8, risp_serve_u8_cfa, risp_serve_classical_u8, serve() of the pipelines) over
their argument space, against the float64 statement of tests/serve_reference.py - from the uint16 sensor frame to the bytes.

Every other serving test compares two GPU routes with torch.equal; a mistake shared by both passes.  Here the truth is
computed on the CPU, a Bayer phase is a table of colour sites (no mirror), and the comparison is the rule of
tests/serve_space_cases.py (decided pixels equal the reference, a byte at a final tie may differ by 1, a pixel at an inner
tie is excused, both kinds of tie capped), with the table, the walk and TAU of that file.

Each case runs through the C ABI into a guard-banded buffer and through the functional wrapper, and is checked for full
writes (two fills, 0xA5 and 0x5A: an unwritten byte would differ between them), bit determinism, batch independence and
``reverse``.  Every case prints one line (pytest -s; tools/serve_space_budget_report.py condenses them into profiles/)."""
import ctypes as C

import numpy as np
import pytest
import torch

import serve_reference as S
from serve_reference import OP_GTM_MANUAL
from serve_space_cases import CASES, WALK, TAU, make_raw, reference, sweep_case, walk_case

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- the checks (GPU)
GUARD = 64


def _abi(case, raw, params, fill, reverse, force_cfa=False, rows=None):
    """one call of the entry point through the C ABI into a guard-banded buffer -> (bytes (n,H,W,3), guards intact)"""
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    n, h, w = raw.shape
    size = n * h * w * 3
    big = torch.full((size + 2 * GUARD,), fill, device='cuda', dtype=torch.uint8)
    out = big[GUARD:GUARD + size]
    p = lambda t: C.c_void_p(t.data_ptr())
    ops = case['ops']
    oparr = (C.c_int * max(1, len(ops)))(*ops)
    blocks = L.ptr_array([t.data_ptr() if t is not None else None for t in params] or [None])
    divisor, code = float(case['white'] - case['black']), S.CFA[case['phase']]
    if case['entry'] == 'c':
        L.call('risp_serve_classical_u8', p(raw), divisor, S.DEMOSAIC[case['demosaic']], len(ops), oparr, blocks, p(out),
               int(reverse), n, h, w, case['black'], code, F._stream())
    else:
        bil = (None, None, None, 0)
        keep = None
        if case['bilateral'] is not None:
            sl = slice(None) if rows is None else rows
            keep = [torch.from_numpy(np.ascontiguousarray(a[sl])).cuda() for a in case['bilateral']]
            bil = (p(keep[0]), p(keep[1]), p(keep[2]), case['max_window'])
        args = (p(raw), divisor, *bil, len(ops), oparr, blocks, p(out), int(reverse), n, h, w)
        if code or case['black'] or force_cfa:
            L.call('risp_serve_u8_cfa', *args, case['black'], code, F._stream())
        else:
            L.call('risp_serve_u8', *args, F._stream())
    torch.cuda.synchronize()
    ok = bool((big[:GUARD] == fill).all().item() and (big[GUARD + size:] == fill).all().item())
    return out.view(n, h, w, 3).clone(), ok


def _wrapper(case, raw, params, reverse):
    import reconfigisp_amd.functional as F
    divisor = float(case['white'] - case['black'])
    if case['entry'] == 'c':
        return F.serve_classical_u8(raw, divisor, case['demosaic'], case['ops'], params, reverse, black_level=case['black'],
                                    cfa=case['phase'])
    bil = None
    if case['bilateral'] is not None:
        bil = tuple(torch.from_numpy(a).cuda() for a in case['bilateral']) + (case['max_window'],)
    return F.serve_u8(raw, divisor, case['ops'], params, bil, reverse, black_level=case['black'], cfa=case['phase'])


def run_case(case):
    dev = torch.from_numpy(case['raw'].astype(np.uint16)).cuda()
    params = [None if p is None else torch.from_numpy(p).cuda() for p in case['params']]
    n, rev = case['n'], case['reverse']
    got, guards = _abi(case, dev, params, 0xA5, rev)
    bad, rep = S.check(got, case['ref'], TAU)
    print('SERVE_SPACE %-100s draws %d differ %6d share %.3e worst-tie %.3e inner-tie-pixels %.3e final-tie-bytes %.3e %s' % (
        case['what'], case['draws'], rep['differ'], rep['share'], rep['worst'], rep['inner_share'], rep['loose_share'],
        'OK' if not bad else 'OUTSIDE THE RULE'))
    assert not bad, '%s: %s' % (case['what'], '; '.join(bad))
    assert guards, '%s: a guard band was written' % case['what']
    # full writes and bit determinism: a second call into a buffer filled with another byte gives the same bytes
    again, guards = _abi(case, dev, params, 0x5A, rev)
    assert guards and torch.equal(again, got), '%s: two calls differ, or a byte was left unwritten' % case['what']
    if case['entry'] == 's' and not case['black'] and case['phase'] == 'rggb':      # the _cfa entry point with zero keywords
        assert torch.equal(_abi(case, dev, params, 0xA5, rev, force_cfa=True)[0], got)
    assert torch.equal(_wrapper(case, dev, params, rev), got), '%s: the functional wrapper gives other bytes' % case['what']
    # reverse: the channel-swapped bytes
    swapped, _ = _abi(case, dev, params, 0xA5, not rev)
    assert torch.equal(swapped, got.flip(-1)), '%s: reverse is not the channel swap' % case['what']
    # batch independence: image i alone gives image i's bytes (GtmManual takes its knots from row 0 of its block)
    for i in range(n if n > 1 else 0):
        one = [None if p is None else (p[0:1] if op == OP_GTM_MANUAL else p[i:i + 1]).contiguous()
               for op, p in zip(case['ops'], params)]
        alone, _ = _abi(case, dev[i:i + 1].contiguous(), one, 0xA5, rev, rows=slice(i, i + 1))
        assert torch.equal(alone[0], got[i]), '%s: image %d alone gives other bytes' % (case['what'], i)


@pytest.mark.parametrize('index', range(len(CASES)), ids=lambda i: '%03d-%s' % (i, '-'.join(str(v) for v in CASES[i])))
def test_sweep(index):
    run_case(sweep_case(index))


@pytest.mark.parametrize('seed', range(WALK))
def test_walk(seed):
    run_case(walk_case(seed))


# ---------------------------------------------------------------------------------------------------- serve() of the pipelines
HEADLINE = 'Demosaic_01_sRGB_07_11_01_14'
PIPELINES = [('Demosaic_02_sRGB_11_01_14', 'classical'), ('Demosaic_03_sRGB_11_04_01', 'classical'),
             ('Demosaic_03_sRGB_13_10_03_01', 'classical'), ('Demosaic_01_sRGB_03_01', 'classical'), (HEADLINE, 'fused')]


@pytest.mark.parametrize('phase,black', [('grbg', 64), ('rggb', 0)])
@pytest.mark.parametrize('arch,route', PIPELINES)
def test_pipeline_serve(arch, route, phase, black):
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as CL
    assert [a for a, _ in PIPELINES[:4]] == CL.ARCHS and HEADLINE == CF.HEADLINE
    net = CF._pipeline(arch)
    n, h, w, white = 3, 34, 68, 1023
    blocks = [None if p is None else p.detach().cpu().numpy() for p in net._stage_params(n)]
    demosaic, bilateral, ops, params = S.plugin_stages(net.step_names, blocks)
    case = dict(white=white, black=black, phase=phase, demosaic=demosaic, bilateral=bilateral, ops=ops, params=params, reverse=False)
    for attempt in range(8):
        case['raw'] = make_raw(n, h, w, white, black, 31000 + len(arch) + 100 * attempt)
        ref = reference(case)
        inner, loose = S.tie_shares(ref, TAU)
        if inner <= S.TIE_CAP and loose <= S.FINAL_CAP:
            break
    else:
        raise AssertionError('%s: no input under the caps in 8 draws' % arch)
    dev = torch.from_numpy(case['raw'].astype(np.uint16)).cuda()
    got = net.serve(dev, float(white), black_level=black, cfa=phase)
    assert net.last_serve_route == route
    bad, rep = S.check(got, ref, TAU)
    print('SERVE_SPACE %-100s draws %d differ %6d share %.3e worst-tie %.3e inner-tie-pixels %.3e final-tie-bytes %.3e %s' % (
        'serve() %s %s black %d' % (arch, phase, black), attempt + 1, rep['differ'], rep['share'], rep['worst'], rep['inner_share'],
        rep['loose_share'], 'OK' if not bad else 'OUTSIDE THE RULE'))
    assert not bad, '%s %s black %d: %s' % (arch, phase, black, '; '.join(bad))
    assert torch.equal(net.serve(dev, float(white), reverse_channels=True, black_level=black, cfa=phase), got.flip(-1))
