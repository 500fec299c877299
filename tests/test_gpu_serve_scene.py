"""GPU: the scene route of the serving path (risp_serve_scene_stats / _finish / _u8, serve(fast_scene=True)) against the
float64 statement of tests/serve_scene_reference.py, over the table and the walk of tests/serve_scene_cases.py with that
file's TAU and the comparison rule of serve_reference.check.

Each case runs through the C ABI - per scene stage a statistics and a finish launch, then the serving launch - into
guard-banded ``out``, ``partials`` and ``consts``, and is checked for full writes (two fills: an unwritten byte or float
would differ between them), bit determinism, batch independence, the constants against the float64 statistics, and the
functional wrappers.  Every case prints one line (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import serve_reference as S
import serve_scene_reference as SC
from serve_reference import OP_GTM_MANUAL
from serve_scene_cases import CASES, WALK, TAU, CONST_TAU, kernel_stages, sweep_case, walk_case

pytestmark = pytest.mark.gpu
GUARD = 64


def _guarded(count, dtype, fill):
    big = torch.full((count + 2 * GUARD,), fill, device='cuda', dtype=dtype)
    return big, big[GUARD:GUARD + count]


def _intact(big, count, fill):
    ref = torch.full((GUARD,), fill, device='cuda', dtype=big.dtype)
    return bool(torch.equal(big[:GUARD].view(torch.uint8), ref.view(torch.uint8))
                and torch.equal(big[GUARD + count:].view(torch.uint8), ref.view(torch.uint8)))


def _abi(case, raw, params, fill, reverse):
    """the 2 S + 1 launches through the C ABI -> (bytes, [consts per scene stage], [partials], guards intact)"""
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    n, h, w = raw.shape
    g = L.load().risp_serve_scene_groups(h, w)
    assert g == ((w // 4 + 15) // 16) * ((h // 2 + 15) // 16)
    p = lambda t: C.c_void_p(t.data_ptr())
    divisor, code, kind = float(case['white'] - case['black']), S.CFA[case['phase']], S.DEMOSAIC[case['demosaic']]
    ffill = float(np.frombuffer(bytes([fill] * 4), np.float32)[0])
    keep, consts, parts, ok = [], [], [], True
    scene = [(k, op) for k, op in enumerate(case['ops']) if op in SC.SCENE]
    for k, op in scene:
        ops, blocks = kernel_stages(dict(case, ops=case['ops'][:k], params=params[:k]), consts)
        oparr = (C.c_int * max(1, len(ops)))(*ops)
        barr = L.ptr_array([t.data_ptr() if t is not None else None for t in blocks] or [None])
        pbig, part = _guarded(n * g * 4, torch.float32, ffill)
        cbig, cst = _guarded(n * 4, torch.float32, ffill)
        assert part.data_ptr() % 16 == 0 and cst.data_ptr() % 16 == 0
        L.call('risp_serve_scene_stats', p(raw), divisor, kind, len(ops), oparr, barr, SC.SCENE_STAT[op], p(part), n, h, w,
               case['black'], code, F._stream())
        a = params[k][:, 0].contiguous() if params[k] is not None else None
        b = params[k][:, 1].contiguous() if op == SC.REINHARD else None
        L.call('risp_serve_scene_finish', SC.SCENE_STAT[op], p(part), p(a) if a is not None else None,
               p(b) if b is not None else None, p(cst), n, g, h * w, F._stream())
        torch.cuda.synchronize()
        ok = ok and _intact(pbig, n * g * 4, ffill) and _intact(cbig, n * 4, ffill)
        keep += [pbig, cbig, a, b]
        parts.append(part.view(n, g, 4))
        consts.append(cst[:3 * n].view(n, 3) if op == SC.GRAYWORLD else cst.view(n, 4))
    ops, blocks = kernel_stages(dict(case, params=params), consts)
    size = n * h * w * 3
    obig, out = _guarded(size, torch.uint8, fill)
    L.call('risp_serve_scene_u8', p(raw), divisor, kind, len(ops), (C.c_int * max(1, len(ops)))(*ops),
           L.ptr_array([t.data_ptr() if t is not None else None for t in blocks] or [None]), p(out), int(reverse), n, h, w,
           case['black'], code, F._stream())
    torch.cuda.synchronize()
    ok = ok and _intact(obig, size, fill)
    return out.view(n, h, w, 3).clone(), [c.clone() for c in consts], [q.clone() for q in parts], ok, keep


def _wrappers(case, raw, params, reverse):
    import reconfigisp_amd.functional as F
    n, h, w = raw.shape
    divisor, consts = float(case['white'] - case['black']), []
    for k, op in enumerate(case['ops']):
        if op not in SC.SCENE:
            continue
        ops, blocks = kernel_stages(dict(case, ops=case['ops'][:k], params=params[:k]), consts)
        part = F.serve_scene_stats(raw, divisor, case['demosaic'], ops, blocks, SC.SCENE_STAT[op], None, case['black'], case['phase'])
        a = params[k][:, 0] if params[k] is not None else None
        b = params[k][:, 1] if op == SC.REINHARD else None
        consts.append(F.serve_scene_finish(SC.SCENE_STAT[op], part, h * w, a, b, tag=len(consts)))
    ops, blocks = kernel_stages(dict(case, params=params), consts)
    return F.serve_scene_u8(raw, divisor, case['demosaic'], ops, blocks, reverse, black_level=case['black'], cfa=case['phase'])


def run_case(case):
    dev = torch.from_numpy(case['raw'].astype(np.uint16)).cuda()
    params = [None if p is None else torch.from_numpy(p).cuda() for p in case['params']]
    n, rev = case['n'], case['reverse']
    got, consts, parts, guards, _ = _abi(case, dev, params, 0xA5, rev)
    bad, rep = S.check(got, case['ref'], TAU)
    # the constants against the float64 statistics
    worst = 0.0
    stages = [op for op in case['ops'] if op in SC.SCENE]
    for stage, c, want in zip(stages, consts, case['ref'].consts):
        have = c.cpu().numpy().astype(np.float64)[:, :want.shape[1]]
        rel = (np.abs(have - want) / np.maximum(np.abs(want), 1e-30)).max()
        worst = max(worst, rel / CONST_TAU[SC.SCENE_STAT[stage]])
    print('SERVE_SCENE %-90s draws %d differ %6d share %.3e worst-tie %.3e inner-tie-pixels %.3e final-tie-bytes %.3e consts/bound %.3f %s' % (
        case['what'], case['draws'], rep['differ'], rep['share'], rep['worst'], rep['inner_share'], rep['loose_share'], worst,
        'OK' if not bad else 'OUTSIDE THE RULE'))
    assert not bad, '%s: %s' % (case['what'], '; '.join(bad))
    assert guards, '%s: a guard band was written' % case['what']
    assert worst <= 1.0, '%s: a constant is %.3f x its bound away from the float64 statistic' % (case['what'], worst)
    # full writes and bit determinism: a second run into buffers filled with another pattern gives the same bits
    again, consts2, parts2, guards, _ = _abi(case, dev, params, 0x5A, rev)
    assert guards and torch.equal(again, got), '%s: two calls differ, or a byte was left unwritten' % case['what']
    for a, b in zip(consts + parts, consts2 + parts2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), '%s: a partial row or a constant was left unwritten' % case['what']
    assert torch.equal(_wrappers(case, dev, params, rev), got), '%s: the functional wrappers give other bytes' % case['what']
    swapped = _abi(case, dev, params, 0xA5, not rev)[0]
    assert torch.equal(swapped, got.flip(-1)), '%s: reverse is not the channel swap' % case['what']
    # batch independence: image i alone gives image i's bytes (GtmManual takes its knots from row 0 of its block)
    for i in range(n if n > 1 else 0):
        one = [None if p is None else (p[0:1] if op == OP_GTM_MANUAL else p[i:i + 1]).contiguous()
               for op, p in zip(case['ops'], params)]
        alone = _abi(case, dev[i:i + 1].contiguous(), one, 0xA5, rev)[0]
        assert torch.equal(alone[0], got[i]), '%s: image %d alone gives other bytes' % (case['what'], i)


@pytest.mark.parametrize('index', range(len(CASES)), ids=lambda i: '%03d-%s' % (i, '-'.join(str(v) for v in CASES[i])))
def test_sweep(index):
    run_case(sweep_case(index))


@pytest.mark.parametrize('seed', range(WALK))
def test_walk(seed):
    run_case(walk_case(seed))


# ---------------------------------------------------------------------------------------------------- partial rows
@pytest.mark.parametrize('sign', [-1.0, 1.0], ids=['negative-prefix', 'positive-prefix'])
@pytest.mark.parametrize('shape', [(1, 4, 4), (3, 34, 68), (2, 66, 132)], ids=lambda v: '%dx%dx%d' % v)
def test_partial_rows_against_numpy(shape, sign):
    """the rows of risp_serve_scene_stats against numpy, tile by tile, on ragged shapes whose workgroups are partly (1x4x4:
    almost wholly) idle.  The prefix is WbManual with gains of one sign through the C ABI - the operator does not clamp, so
    with negative gains every live value is negative: an idle thread that held 0 instead of -inf would turn a row's maximum
    into 0.  The stage input is reproduced bit for bit in float32 (an integer over a float, times a gain: two correctly
    rounded operations), so the maxima must be EQUAL; a sum of at most 2048 float32 values in any order is within
    (count - 1) x 2^-24 x sum|x| of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4)"""
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    import serve_scene_cases as T
    n, h, w = shape
    white, black, phase = 1023, 0, 'grbg'
    raw = np.maximum(T.T.make_raw(n, h, w, white, black, 47000 + h), 1)      # no zero sample: every live value has the gain's sign
    gain = (sign * np.random.default_rng(5).uniform(0.3, 1.7, size=(n, 3))).astype(np.float32)
    x32, _ = S.normalise(raw, white, black, np.float32)
    val = S.demosaic_nearest(x32, phase) * gain[:, :, None, None]
    assert val.dtype == np.float32 and (np.sign(val) == sign).all()
    # the kernel works in the mirrored image, which is RGGB (risp.h): its tiles are anchored at that image's origin
    code = S.CFA[phase]
    val = np.ascontiguousarray(val[:, :, ::-1 if code & 2 else 1, ::-1 if code & 1 else 1])
    dev, gdev = torch.from_numpy(raw.astype(np.uint16)).cuda(), torch.from_numpy(gain).cuda()
    g = L.load().risp_serve_scene_groups(h, w)
    for stat in (SC.SCENE_STAT[SC.WHITEWORLD], SC.SCENE_STAT[SC.GRAYWORLD]):
        big, part = _guarded(n * g * 4, torch.float32, 123.0)
        L.call('risp_serve_scene_stats', C.c_void_p(dev.data_ptr()), float(white - black), S.DEMOSAIC['nearest'], 1,
               (C.c_int * 1)(S.OP_WB_MANUAL), L.ptr_array([gdev.data_ptr()]), stat, C.c_void_p(part.data_ptr()), n, h, w, black,
               S.CFA[phase], F._stream())
        torch.cuda.synchronize()
        assert _intact(big, n * g * 4, 123.0)
        got = part.view(n, g, 4).cpu().numpy()
        assert (got[:, :, 3] == 0).all()
        if stat == 1:
            want = SC.tile_partials(val, 1, np.float32)
            assert np.array_equal(got, want), 'maxima: got %s want %s' % (got[0, 0], want[0, 0])
            assert (np.sign(got[:, :, :3]) == sign).all()            # (a row of 0 would be the idle threads' doing)
        else:
            want = SC.tile_partials(val, 0, np.float64)
            mass = SC.tile_partials(np.abs(val), 0, np.float64)
            bound = (SC.TILE_H * SC.TILE_W - 1) * 2.0 ** -24 * mass
            assert (np.abs(got - want) <= bound).all(), 'sums: worst %.3e of the bound' % (np.abs(got - want) / np.maximum(bound, 1e-300)).max()


def test_scene_u8_is_classical_u8_without_scene_stages():
    """risp.h: for the stages both accept, risp_serve_scene_u8 has risp_serve_classical_u8's bytes - over every classical row
    of tests/serve_space_cases.py (three demosaic kinds, four phases, black levels, every stage both take)"""
    import reconfigisp_amd.functional as F
    import serve_space_cases as SP
    rows = [i for i, c in enumerate(SP.CASES) if c[0] == 'c']
    assert len(rows) >= 90
    for i in rows:
        case = SP.sweep_case(i)
        dev = torch.from_numpy(case['raw'].astype(np.uint16)).cuda()
        params = [None if p is None else torch.from_numpy(p).cuda() for p in case['params']]
        args = (dev, float(case['white'] - case['black']), case['demosaic'], case['ops'], params, case['reverse'])
        kw = dict(black_level=case['black'], cfa=case['phase'])
        assert torch.equal(F.serve_scene_u8(*args, **kw), F.serve_classical_u8(*args, **kw)), case['what']


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    n, h, w = 1, 4, 8
    raw = torch.zeros((n, h, w), device='cuda', dtype=torch.int16).view(torch.uint16)
    part = torch.zeros((n * 1 * 4 + 4,), device='cuda')
    cst = torch.zeros((n * 4 + 4,), device='cuda')
    out = torch.zeros((n * h * w * 3 + 4,), device='cuda', dtype=torch.uint8)
    a = torch.zeros((n,), device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    one = (C.c_int * 1)
    none = L.ptr_array([None])

    def stats(**kw):
        d = dict(raw=p(raw), div=1023.0, kind=1, n_ops=0, ops=one(0), par=none, stat=0, part=p(part), n=n, h=h, w=w, black=0, cfa=0)
        d.update(kw)
        L.call('risp_serve_scene_stats', d['raw'], d['div'], d['kind'], d['n_ops'], d['ops'], d['par'], d['stat'], d['part'], d['n'],
               d['h'], d['w'], d['black'], d['cfa'], F._stream())

    def finish(**kw):
        d = dict(stat=1, part=p(part), a=p(a), b=p(a), cst=p(cst), n=n, g=1, hw=h * w)
        d.update(kw)
        L.call('risp_serve_scene_finish', d['stat'], d['part'], d['a'], d['b'], d['cst'], d['n'], d['g'], d['hw'], F._stream())

    def serve(**kw):
        d = dict(raw=p(raw), div=1023.0, kind=1, n_ops=0, ops=one(0), par=none, out=p(out), n=n, h=h, w=w, black=0, cfa=0)
        d.update(kw)
        L.call('risp_serve_scene_u8', d['raw'], d['div'], d['kind'], d['n_ops'], d['ops'], d['par'], d['out'], 0, d['n'], d['h'], d['w'],
               d['black'], d['cfa'], F._stream())

    stats(), finish(), serve()                      # the arguments the refusals vary are good
    torch.cuda.synchronize()
    for call, kw, text in [
        (stats, dict(raw=None), 'null'), (stats, dict(part=None), 'null'), (stats, dict(stat=3), 'stat 3'), (stats, dict(stat=-1), 'stat -1'),
        (stats, dict(h=5), 'H=5'), (stats, dict(w=6), 'W=6'), (stats, dict(h=2), 'H=2'), (stats, dict(n=65536), 'N=65536'),
        (stats, dict(kind=3), 'demosaic 3'), (stats, dict(cfa=4), 'cfa 4'), (stats, dict(black=70000), 'black_level 70000'),
        (stats, dict(div=0.0), 'divisor'), (stats, dict(n_ops=9), 'n_ops 9'),
        (stats, dict(part=C.c_void_p(part.data_ptr() + 4)), '16-byte'),
        (stats, dict(n_ops=1, ops=one(9)), 'op 9'), (stats, dict(n_ops=1, ops=one(10)), 'op 10'), (stats, dict(n_ops=1, ops=one(11)), 'op 11'),
        (stats, dict(n_ops=1, ops=one(1)), 'op 1'), (stats, dict(n_ops=1, ops=one(3)), 'no parameter block'),
        (stats, dict(n_ops=1, ops=one(9), par=L.ptr_array([cst.data_ptr() + 4])), '16-byte'),
        (finish, dict(stat=5), 'stat 5'), (finish, dict(part=None), 'null'), (finish, dict(cst=None), 'null'), (finish, dict(a=None), 'parameter a'),
        (finish, dict(stat=2, b=None), 'parameter b'), (finish, dict(n=0), 'N=0'), (finish, dict(g=0), 'G=0'), (finish, dict(hw=0), 'HW=0'),
        (finish, dict(cst=C.c_void_p(cst.data_ptr() + 4)), '16-byte'), (finish, dict(part=C.c_void_p(part.data_ptr() + 8)), '16-byte'),
        (serve, dict(out=None), 'null'), (serve, dict(out=C.c_void_p(out.data_ptr() + 1)), '4-byte'), (serve, dict(n_ops=1, ops=one(10)), 'op 10'),
        (serve, dict(n_ops=1, ops=one(12)), 'op 12'), (serve, dict(w=10), 'W=10'), (serve, dict(raw=C.c_void_p(raw.data_ptr() + 2)), '8-byte'),
    ]:
        with pytest.raises(RuntimeError, match=text):
            call(**kw)
    assert L.load().risp_serve_scene_groups(5, 8) == 0 and L.load().risp_serve_scene_groups(3000, 4000) == 5922
    # risp_serve_classical_u8 keeps refusing the codes above 8
    with pytest.raises(RuntimeError, match='op 9 not allowed'):
        F.serve_classical_u8(raw, 1023.0, 'bilinear', [9], [cst[:4].view(1, 4)])
    with pytest.raises(ValueError):
        F.serve_scene_stats(raw, 1023.0, 'bilinear', [], [], 7)
    with pytest.raises(ValueError):
        F.serve_scene_finish(F.SCENE_MAX3, part[:4].view(1, 1, 4), h * w)


# ---------------------------------------------------------------------------------------------------- serve() of the pipelines
COMPOSED_CALLS = ('risp_raw_crop_cfa', 'risp_raw_crop', 'risp_origin_demosaic', 'risp_chain_fwd', 'risp_channel_stats', 'risp_origin_tonemap',
                  'risp_quantise_u8', 'risp_quantise_u8_flip', 'risp_grayworld_gains_fwd', 'risp_serve_classical_u8', 'risp_serve_u8')
PIPELINES = [('Demosaic_02_sRGB_05_01', 'origin', 1), ('Demosaic_03_sRGB_06_02_01', 'origin', 2), ('Demosaic_01_sRGB_05', 'isp', 1),
             ('Demosaic_02_sRGB_05_02', 'origin', 2)]


def _net(arch, kind):
    import test_gpu_serve_cfa as CF
    return CF._pipeline(arch, 'OriginUniversal' if kind == 'origin' else 'IspUniversal')


def _stages(net, n):
    """the pipeline's stage list for the reference: (demosaic, ops, params), by the mapping the modules apply"""
    blocks = [None if p is None else p.detach().cpu().numpy() for p in net._stage_params(n)]
    scene = {'grayworld': SC.GRAYWORLD, 'whiteworld': SC.WHITEWORLD, 'reinhard': SC.REINHARD}
    names = [('skip', None) if nm in scene else (nm, b) for nm, b in zip(net.step_names, blocks)]
    demosaic, bilateral, ops, params = S.plugin_stages([a for a, _ in names], [b for _, b in names])
    assert bilateral is None
    k = 0
    for nm, b in zip(net.step_names, blocks):
        if nm in S.DEMOSAIC:
            continue
        if nm in scene:
            ops[k] = scene[nm]
            params[k] = None if nm == 'grayworld' else np.asarray(b, np.float32)[:, :SC.PARAM_WIDTH[scene[nm]]]
        k += 1
    return demosaic, ops, params


@pytest.mark.parametrize('phase,black', [('grbg', 64), ('rggb', 0)])
@pytest.mark.parametrize('arch,kind,scenes', PIPELINES)
def test_pipeline_serve_scene(arch, kind, scenes, phase, black):
    from reconfigisp_amd import lib as L
    import serve_scene_cases as T
    net = _net(arch, kind)
    n, h, w, white = 2, 34, 68, 1023
    demosaic, ops, params = _stages(net, n)
    assert sum(op in SC.SCENE for op in ops) == scenes
    case = dict(white=white, black=black, phase=phase, demosaic=demosaic, ops=ops, params=params, reverse=False)
    for attempt in range(8):
        case['raw'] = T.T.make_raw(n, h, w, white, black, 41000 + len(arch) + 100 * attempt)
        ref = T.reference(case)
        inner, loose = S.tie_shares(ref, TAU)
        if inner <= S.TIE_CAP and loose <= S.FINAL_CAP:
            break
    else:
        raise AssertionError('%s: no input under the caps in 8 draws' % arch)
    dev = torch.from_numpy(case['raw'].astype(np.uint16)).cuda()
    # the default call is today's: composed
    base = net.serve(dev, float(white), black_level=black, cfa=phase)
    assert net.last_serve_route == 'composed'
    L.CALLS = {}
    try:
        got = net.serve(dev, float(white), black_level=black, cfa=phase, fast_scene=True)
        calls = dict(L.CALLS)
    finally:
        L.CALLS = None
    assert net.last_serve_route == 'scene'
    assert sum(calls.values()) == 2 * scenes + 1 and calls == {
        'risp_serve_scene_stats': scenes, 'risp_serve_scene_finish': scenes, 'risp_serve_scene_u8': 1}, calls
    assert not set(calls) & set(COMPOSED_CALLS)
    bad, rep = S.check(got, ref, TAU)
    print('SERVE_SCENE %-90s draws %d differ %6d share %.3e worst-tie %.3e inner-tie-pixels %.3e final-tie-bytes %.3e differ-from-composed %d %s' % (
        'serve() %s %s black %d' % (arch, phase, black), attempt + 1, rep['differ'], rep['share'], rep['worst'], rep['inner_share'],
        rep['loose_share'], int((got != base).sum().item()), 'OK' if not bad else 'OUTSIDE THE RULE'))
    assert not bad, '%s %s black %d: %s' % (arch, phase, black, '; '.join(bad))
    assert torch.equal(net.serve(dev, float(white), reverse_channels=True, black_level=black, cfa=phase, fast_scene=True), got.flip(-1))
    # a warm call with out= allocates nothing
    out = torch.empty_like(got)
    net.serve(dev, float(white), out=out, black_level=black, cfa=phase, fast_scene=True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    res = net.serve(dev, float(white), out=out, black_level=black, cfa=phase, fast_scene=True)
    assert res.data_ptr() == out.data_ptr() and torch.cuda.memory_allocated() == before
    torch.cuda.synchronize()
    assert torch.equal(out, got)
    # a parameter changed in place reaches the next call
    live = [p for p in net.all_params if p.numel()]
    if live:                                                # (nearest + gray-world has no parameter to change)
        with torch.no_grad():
            live[-1].add_(1.5)
        changed = net.serve(dev, float(white), black_level=black, cfa=phase, fast_scene=True)
        assert net.last_serve_route == 'scene' and not torch.equal(changed, got)
        want = net.serve(dev, float(white), black_level=black, cfa=phase)
        assert (changed.int() - want.int()).abs().max().item() <= 1


def test_whiteworld_only_is_the_composed_route_byte_for_byte():
    net = _net('Demosaic_03_sRGB_06_01', 'origin')
    import serve_scene_cases as T
    n, h, w, white = 3, 34, 68, 1023
    for phase, black in [('rggb', 0), ('grbg', 0), ('gbrg', 64), ('bggr', 64)]:
        dev = torch.from_numpy(T.T.make_raw(n, h, w, white, black, 43000).astype(np.uint16)).cuda()
        want = net.serve(dev, float(white), black_level=black, cfa=phase)
        assert net.last_serve_route == 'composed'
        got = net.serve(dev, float(white), black_level=black, cfa=phase, fast_scene=True)
        assert net.last_serve_route == 'scene' and torch.equal(got, want), (phase, black)


def test_fast_scene_elsewhere_is_todays_route():
    import serve_scene_cases as T
    white = 1023
    net = _net('Demosaic_02_sRGB_11_01_14', 'origin')           # no scene stage
    dev = torch.from_numpy(T.T.make_raw(2, 34, 68, white, 0, 44000).astype(np.uint16)).cuda()
    want = net.serve(dev, float(white))
    route = net.last_serve_route
    assert torch.equal(net.serve(dev, float(white), fast_scene=True), want) and net.last_serve_route == route == 'classical'
    net = _net('Demosaic_01_sRGB_05_01', 'origin')              # gray-world, W % 4 != 0: the kernels' shape rule fails
    dev = torch.from_numpy(T.T.make_raw(2, 34, 66, white, 0, 44001).astype(np.uint16)).cuda()
    want = net.serve(dev, float(white))
    assert net.last_serve_route == 'composed'
    assert torch.equal(net.serve(dev, float(white), fast_scene=True), want) and net.last_serve_route == 'composed'
