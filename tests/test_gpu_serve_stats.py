"""GPU: the 3A statistics of the sensor frame - the launch (risp_raw_stats, from uint16 and from MIPI-packed frames) and
``serve(statistics=...)`` / ``serve_frame``.

Everything is a count or a sum of integers (include/risp.h), so every comparison is ``torch.equal``: the launch against
tests/stats_reference.py (numpy int64), a serving call's image against the same call without the keyword, and its statistics
against the reference on the frames that call demosaics - ``functional.raw_unpack`` / ``raw_defect`` / ``raw_shade`` of the
input.  Nothing here has a tolerance.  The launch's inputs are ``LAUNCH_CASES`` and the extremes of tests/stats_reference.py;
tests/test_stats_reference_cpu.py asserts that they tell every wrong variant of the definition apart.

uint16 frames lie at byte 8 (the 8-byte loads) and at byte 2 (single loads) of a larger allocation, packed frames start at an odd
byte and have an odd stride whose padding holds junk.  The outputs are taken once as ``RawStatistics`` allocates them - one
memset - and once as views inside two allocations of a pattern - two memsets, and a write outside shows."""
import ctypes as C

import numpy as np
import pytest
import torch

import raw_packed_reference as PR
import stats_reference as SR
from raw_placement import _place16, _place_packed

pytestmark = pytest.mark.gpu


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


PATTERN64, PATTERN32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


def _guarded(st):
    """``st`` with its outputs moved into two allocations of a pattern, four words from either end; returns the allocations"""
    big_z = torch.full((st.zones.numel() + 8,), PATTERN64, dtype=torch.int64, device='cuda')
    big_h = torch.full((st.hist.numel() + 8,), PATTERN32, dtype=torch.int32, device='cuda')
    st.zones = big_z[4:4 + st.zones.numel()].view(st.zones.shape)
    st.hist = big_h[4:4 + st.hist.numel()].view(st.hist.shape)
    return big_z, big_h


def _assert_guards(big_z, big_h):
    assert (big_z[:4] == PATTERN64).all() and (big_z[-4:] == PATTERN64).all(), 'zones: written outside'
    assert (big_h[:4] == PATTERN32).all() and (big_h[-4:] == PATTERN32).all(), 'hist: written outside'


def _assert_stats(st, want, what):
    zones, hist = want
    got_z, got_h = st.zones.cpu(), st.hist.cpu()
    assert got_z.dtype == torch.int64 and got_h.dtype == torch.int32
    assert torch.equal(got_h, torch.from_numpy(hist)), '%s: %d histogram counts differ' % (what, (got_h.numpy() != hist).sum())
    assert torch.equal(got_z, torch.from_numpy(zones)), '%s: %d zone values differ, first at %s' % (
        what, (got_z.numpy() != zones).sum(), np.argwhere(got_z.numpy() != zones)[:1].tolist())


def _reference(st, frames, black):
    return SR.stats_ref(frames, black, (st.zone_h, st.zone_w), st.bins, st.hist_shift, st.lo, st.hi)


# ---------------------------------------------------------------- 1. the launch
@pytest.mark.parametrize('case', range(len(SR.LAUNCH_CASES)),
                         ids=['%dx%dx%d-zone%dx%d-bins%d-%dbit' % (c[0] + c[1] + (c[2], c[7])) for c in SR.LAUNCH_CASES])
def test_raw_stats_equals_the_reference(case):
    import reconfigisp_amd.functional as F
    shape, zone, bins, shift, lo, hi, black, bits = SR.LAUNCH_CASES[case]
    n, h, w = shape
    x = SR.case_frames(shape, bits, seed=case)
    want = SR.stats_ref(x, black, zone, bins, shift, lo, hi)
    assert want[1].sum() == n * h * w and (black == 0 or (x < black).any())
    sources = [('u16 at byte 8', _place16(x, 4), 16), ('u16 at byte 2', _place16(x, 1), 16)]
    for pbits in (10, 12):
        if bits <= pbits:
            used = w * pbits // 8
            sources.append(('raw%d' % pbits, _place_packed(x, pbits, (used + 4) | 1, 1), pbits))
    for what, dev, fbits in sources:
        for guarded in (False, True):
            st = F.raw_statistics(n, h, w, zone=zone, bins=bins, hist_shift=shift, lo=lo, hi=hi)
            guards = _guarded(st) if guarded else None
            st.zones.fill_(-7), st.hist.fill_(-7)           # both are overwritten, whatever they held
            got, calls = _counted(lambda: F.raw_stats(dev, st, black, fbits, None if fbits == 16 else w))
            assert got is st and calls == {'risp_raw_stats': 1}
            _assert_stats(st, want, '%s %s' % (what, 'guarded' if guarded else 'joined'))
            if guarded:
                _assert_guards(*guards)
    # a second call does not accumulate, and a single (H,W) frame is one image
    st = F.raw_statistics(1, h, w, zone=zone, bins=bins, hist_shift=shift, lo=lo, hi=hi)
    one = torch.from_numpy(x[n - 1]).cuda()
    F.raw_stats(one, st, black)
    F.raw_stats(one, st, black)
    _assert_stats(st, SR.stats_ref(x[n - 1], black, zone, bins, shift, lo, hi), 'a single frame, called twice')


@pytest.mark.parametrize('kind', SR.EXTREME_CASES)
def test_the_extremes_pass_32_bits(kind):
    import reconfigisp_amd.functional as F
    n, h, w = SR.EXTREME_SHAPE
    x = SR.extreme_frames(kind)
    st = F.raw_statistics(n, h, w, zone=SR.EXTREME_ZONE, bins=16, hist_shift=6)
    F.raw_stats(torch.from_numpy(x).cuda(), st)
    want = _reference(st, x, 0)
    assert want[0][..., 0 if kind == 'full' else 2].min() > 1 << 32
    _assert_stats(st, want, kind)


@pytest.mark.parametrize('shape,zone,bins', [((1, 2048, 4096), (38, 100), 256), ((64, 256, 256), (32, 32), 256),
                                             ((128, 256, 256), (2, 4), 1024)], ids=['frame-zone38x100', 'batch-zone32x32', 'batch-zone2x4'])
def test_inputs_large_enough_for_the_taller_tiles(shape, zone, bins):
    """A taller tile is taken while the launch keeps 512 tiles and the tile's zone table fits beside the histogram: the frame has
    512 tiles of 256 x 64, the first batch 512 of 256 x 32, and the second batch stays at 16 rows - 64 x 8 zones a tile and 1024
    bins, the largest LDS request there is"""
    import reconfigisp_amd.functional as F
    n, h, w = shape
    x = SR.case_frames(shape, 12, seed=5)
    st = F.raw_statistics(n, h, w, zone=zone, bins=bins, hist_shift=2, lo=16, hi=4000)
    F.raw_stats(torch.from_numpy(x).cuda(), st, 64)
    _assert_stats(st, _reference(st, x, 64), 'the large frame')


def test_a_batch_of_many_small_images():
    """3000 tiles of 64 rows, 18 of them inside a frame, two tiles an image: the tile index is split into image, row and column"""
    import reconfigisp_amd.functional as F
    n, h, w = 1500, 18, 260
    x = SR.case_frames((n, h, w), 10, seed=6)
    st = F.raw_statistics(n, h, w, zone=(6, 20), bins=16, hist_shift=6, lo=64, hi=900)
    F.raw_stats(torch.from_numpy(x).cuda(), st, 64)
    _assert_stats(st, _reference(st, x, 64), 'the batch')


# ---------------------------------------------------------------- 2. serve(statistics=...)
N, H, W, BLACK, WHITE, ZONE = 2, 36, 72, 64, 1023.0, (8, 20)


def _frames(seed):
    return PR.full_range_frame(N, H, W, 10, seed=seed)


def _new_stats(n=N):
    import reconfigisp_amd.functional as F
    return F.raw_statistics(n, H, W, zone=ZONE, bins=64, hist_shift=4, lo=BLACK, hi=900)


def _route_case(what):
    import test_gpu_serve_shade as SH
    return SH._route_case(what)


def _serve_both(net, src, st, want_stats, route, extra_calls=(), **kw):
    """the call without and with the keyword: the same image, the launches of the plain call plus ``extra_calls`` and one
    risp_raw_stats, ``last_serve_stats`` on both, the statistics equal to ``want_stats``; returns the image"""
    net.serve(src, WHITE, **kw)                             # (the stage parameters are made once per parameter version)
    plain, plain_calls = _counted(lambda: net.serve(src, WHITE, **kw))
    plain = plain.clone()
    assert net.last_serve_route == route and net.last_serve_stats is None
    st.zones.fill_(-3), st.hist.fill_(-3)
    got, calls = _counted(lambda: net.serve(src, WHITE, statistics=st, **kw))
    assert net.last_serve_route == route and net.last_serve_stats == 'pass'
    expect = dict(plain_calls, risp_raw_stats=1)
    for name in extra_calls:
        expect[name] = expect.get(name, 0) + 1
    assert calls == expect, (calls, plain_calls)
    assert torch.equal(got, plain), '%d image bytes differ' % (got != plain).sum().item()
    _assert_stats(st, want_stats, route)
    none, none_calls = _counted(lambda: net.serve(src, WHITE, statistics=None, **kw))
    assert torch.equal(none, plain) and none_calls == plain_calls and net.last_serve_stats is None
    assert len(torch.unique(plain)) > 8
    return plain


@pytest.mark.parametrize('what', ['fused', 'classical', 'composed', 'denoise'])
def test_serve_fills_the_statistics_on_every_kind_of_route(what):
    net, kw, route = _route_case(what)
    x, st = _frames(71), _new_stats()
    src = torch.from_numpy(x).cuda()
    want = _reference(st, x, BLACK)
    assert (x < BLACK).any() and (x > 900 + BLACK).any()
    _serve_both(net, src, st, want, route, black_level=BLACK, cfa='grbg', **kw)
    # out= given: a warm call allocates nothing
    buf = torch.empty((N, H, W, 3), device='cuda', dtype=torch.uint8)
    net.serve(src, WHITE, out=buf, statistics=st, black_level=BLACK, cfa='grbg', **kw)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert net.serve(src, WHITE, out=buf, statistics=st, black_level=BLACK, cfa='grbg', **kw) is buf
    if what != 'composed':                                  # (the composed route allocates its fp32 planes either way)
        assert torch.cuda.memory_allocated() == before
    _assert_stats(st, want, what)


def test_the_planes_do_not_move_with_the_phase():
    import reconfigisp_amd.functional as F
    net, kw, route = _route_case('classical')
    x, st = _frames(72), _new_stats()
    want = _reference(st, x, BLACK)
    for phase in ('bggr', 'rggb'):
        _serve_both(net, torch.from_numpy(x).cuda(), st, want, route, black_level=BLACK, cfa=phase)
    assert F.stats_planes('bggr')[0] == 'b' and F.stats_planes('rggb')[0] == 'r'


@pytest.mark.parametrize('what', ['fused', 'classical'])
def test_packed_frames_are_read_as_given(what):
    import reconfigisp_amd.functional as F
    net, kw, route = _route_case(what)
    x, st = _frames(73), _new_stats()
    pk = _place_packed(x, 10, W * 10 // 8 + 3, 1)
    assert torch.equal(F.raw_unpack(pk, 10, W).cpu(), torch.from_numpy(x))
    _serve_both(net, pk, st, _reference(st, x, BLACK), route, black_level=BLACK, raw_format='raw10', raw_width=W)
    assert net.last_serve_load == ('fused' if what == 'classical' else 'pass')        # the route's load is chosen as without


@pytest.mark.parametrize('fmt', ['u16', 'raw10'])
@pytest.mark.parametrize('table', ['fused_shade', 'shade_launch'])
def test_behind_a_lens_shading_the_shade_launch_runs(table, fmt, monkeypatch):
    import test_gpu_serve_shade as SH
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    monkeypatch.setattr(PF, '_FUSED_SHADE', frozenset({('classical', 'u16')}) if table == 'fused_shade' else frozenset())
    net, kw, route = _route_case('classical')
    x, st = _frames(74), _new_stats()
    _, shading = SH._map(H, W, 16, seed=75)
    if fmt == 'u16':
        src, fkw, bits = torch.from_numpy(x).cuda(), {}, 16
    else:
        src, fkw, bits = _place_packed(x, 10, W * 10 // 8 + 3, 1), dict(raw_format='raw10', raw_width=W), 10
    shaded = F.raw_shade(src, shading, BLACK, bits, W).cpu().numpy()
    assert not np.array_equal(shaded, x)
    want = _reference(st, shaded, 0)                        # behind a shading the black level is 0
    fused = table == 'fused_shade' and fmt == 'u16'         # the plain call shades in its load there
    net.serve(src, WHITE, black_level=BLACK, lens_shading=shading, **fkw)
    plain, plain_calls = _counted(lambda: net.serve(src, WHITE, black_level=BLACK, lens_shading=shading, **fkw))
    plain = plain.clone()
    assert net.last_serve_shade == ('fused' if fused else 'pass') and net.last_serve_stats is None
    assert plain_calls == ({'risp_serve_classical_shaded': 1} if fused else {'risp_raw_shade': 1, 'risp_serve_classical_u8': 1})
    got, calls = _counted(lambda: net.serve(src, WHITE, black_level=BLACK, lens_shading=shading, statistics=st, **fkw))
    assert net.last_serve_shade == 'pass' and net.last_serve_stats == 'pass' and net.last_serve_route == route
    assert calls == {'risp_raw_shade': 1, 'risp_raw_stats': 1, 'risp_serve_classical_u8': 1}, calls
    assert torch.equal(got, plain)
    _assert_stats(st, want, 'behind the shade launch')


def test_behind_a_defect_correction_and_behind_both():
    import test_gpu_serve_defect as DF
    import test_gpu_serve_shade as SH
    import defect_reference as DR
    import reconfigisp_amd.functional as F
    net, kw, route = _route_case('classical')
    x, st = _frames(76), _new_stats()
    src = torch.from_numpy(x).cuda()
    dc = (16, 32, DF._place_bitmap(DR.random_bitmap(H, W, 77)))
    _, shading = SH._map(H, W, 16, seed=78)
    fixed = F.raw_defect(src, dc)
    assert not torch.equal(fixed, src)
    _serve_both(net, src, st, _reference(st, fixed.cpu().numpy(), BLACK), route, black_level=BLACK, defect_correction=dc)
    assert net.last_serve_defect == 'pass'
    both = F.raw_shade(fixed, shading, BLACK).cpu().numpy()
    _serve_both(net, src, st, _reference(st, both, 0), route, black_level=BLACK, defect_correction=dc, lens_shading=shading)
    pk = _place_packed(x, 12, W * 12 // 8 + 3, 1)
    _serve_both(net, pk, st, _reference(st, both, 0), route, black_level=BLACK, defect_correction=dc, lens_shading=shading,
                raw_format='raw12', raw_width=W)


@pytest.mark.parametrize('what', ['fused', 'composed'])
def test_nv12_and_a_resized_output_leave_the_statistics_alone(what):
    net, kw, route = _route_case(what)
    x, st = _frames(79), _new_stats()
    src, want = torch.from_numpy(x).cuda(), _reference(_new_stats(), x, BLACK)
    img = _serve_both(net, src, st, want, route, black_level=BLACK, out_format='nv12', yuv_matrix='bt709_full', **kw)
    assert tuple(img.shape) == (N, H + H // 2, W)
    img = _serve_both(net, src, st, want, route, black_level=BLACK, out_size=(18, 40), out_window=(2, 4, 30, 60), **kw)
    assert tuple(img.shape) == (N, 18, 40, 3)


def test_refusals_come_before_any_launch():
    import reconfigisp_amd.functional as F
    net, kw, route = _route_case('classical')
    src = torch.from_numpy(_frames(80)).cuda()
    wrong_n, wrong_dev = _new_stats(N + 1), F.raw_statistics(N, H, W, zone=ZONE, device='cpu')
    changed = _new_stats()
    changed.bins = 2000
    short = _new_stats()
    short.hist = short.hist[:, :, :32]
    for st, word in ((wrong_n, 'statistics.zones'), (wrong_dev, 'lives on cpu'), (changed, 'bins 2000'), (short, 'statistics.hist'),
                     ('zones', 'RawStatistics')):
        from reconfigisp_amd import lib as L
        L.CALLS = {}
        try:
            with pytest.raises(ValueError, match=word):
                net.serve(src, WHITE, statistics=st)
            assert L.CALLS == {}, 'launched before the refusal: %s' % L.CALLS
            with pytest.raises(ValueError, match=word):
                net.serve_frame(src, WHITE, 20, 14, statistics=st)
            assert L.CALLS == {}, 'launched before the refusal: %s' % L.CALLS
        finally:
            L.CALLS = None
    odd = torch.zeros((N, H, W + 2), dtype=torch.uint16, device='cuda')
    with pytest.raises(ValueError, match='wide'):
        net.serve(odd, WHITE, statistics=_new_stats())


# ---------------------------------------------------------------- 3. full frames in tiles
@pytest.mark.parametrize('single', [True, False], ids=['HW', 'NHW'])
@pytest.mark.parametrize('fmt', ['u16', 'raw10'])
def test_serve_frame_takes_the_statistics_of_the_whole_frames(fmt, single):
    import test_gpu_serve_frame as SF
    import test_gpu_serve_shade as SH
    import reconfigisp_amd.functional as F
    model = SF._model('classical')
    net = model.netG
    x = _frames(81)
    size, stride = (20, 40), (14, 28)
    if fmt == 'u16':
        src, fkw, bits = torch.from_numpy(x).cuda(), {}, 16
    else:
        src, fkw, bits = _place_packed(x, 10, W * 10 // 8 + 3, 1), dict(raw_format='raw10', raw_width=W), 10
    if single:
        src, x = src[1], x[1]
    st = _new_stats(1 if single else N)
    kw = dict(black_level=BLACK, cfa='gbrg', tile_batch=3, **fkw)
    plain = model.serve_frame(src, WHITE, size, stride, **kw).clone()
    assert net.last_serve_stats is None
    got, calls = _counted(lambda: model.serve_frame(src, WHITE, size, stride, statistics=st, **kw))
    assert net.last_serve_route == 'tiled' and net.last_serve_stats == 'pass' and calls.get('risp_raw_stats') == 1
    assert tuple(got.shape) == ((H, W, 3) if single else (N, H, W, 3)) and torch.equal(got, plain)
    _assert_stats(st, _reference(st, x, BLACK), 'serve_frame')
    # behind a shading: the statistics of the shaded frame, black level 0
    _, shading = SH._map(H, W, 16, seed=82)
    shaded = F.raw_shade(src, shading, BLACK, bits, W).cpu().numpy()
    plain = model.serve_frame(src, WHITE, size, stride, lens_shading=shading, **kw).clone()
    got, calls = _counted(lambda: model.serve_frame(src, WHITE, size, stride, lens_shading=shading, statistics=st, **kw))
    assert calls.get('risp_raw_stats') == 1 and calls.get('risp_raw_shade') == 1 and torch.equal(got, plain)
    _assert_stats(st, _reference(st, shaded, 0), 'serve_frame behind a shading')


def test_the_model_wrapper_passes_the_keyword_on():
    import test_gpu_serve_frame as SF
    model = SF._model('classical')
    x, st = _frames(83), _new_stats()
    src = torch.from_numpy(x).cuda()
    plain = model.serve(src, WHITE, black_level=BLACK).clone()
    assert model.netG.last_serve_stats is None
    assert torch.equal(model.serve(src, WHITE, black_level=BLACK, statistics=st), plain) and model.netG.last_serve_stats == 'pass'
    _assert_stats(st, _reference(st, x, BLACK), 'IspModel.serve')


# ---------------------------------------------------------------- 4. a captured graph
@pytest.mark.parametrize('shaded', [False, True], ids=['plain', 'shaded'])
def test_a_replayed_graph_does_not_accumulate(shaded):
    import test_gpu_serve_shade as SH
    import reconfigisp_amd.functional as F
    net, kw, route = _route_case('classical')
    xa, xb = _frames(84), _frames(85)
    st = _new_stats()
    sensor = dict(black_level=BLACK, cfa='grbg')
    if shaded:
        _, shading = SH._map(H, W, 16, seed=86)
        sensor['lens_shading'] = shading
        want = [_reference(st, F.raw_shade(torch.from_numpy(x).cuda(), shading, BLACK).cpu().numpy(), 0) for x in (xa, xb)]
    else:
        want = [_reference(st, x, BLACK) for x in (xa, xb)]
    assert not np.array_equal(want[0][0], want[1][0])
    slot, buf = torch.from_numpy(xa).cuda(), torch.zeros((N, H, W, 3), device='cuda', dtype=torch.uint8)
    eager = [net.serve(torch.from_numpy(x).cuda(), WHITE, **sensor).clone() for x in (xa, xb)]
    net.serve(slot, WHITE, out=buf, statistics=st, **sensor)               # fills the caches
    _assert_stats(st, want[0], 'eager')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.serve(slot, WHITE, out=buf, statistics=st, **sensor)
    assert net.last_serve_stats == 'pass'
    for k in (1, 0, 0):                                                    # two contents, the second one twice
        slot.copy_(torch.from_numpy((xa, xb)[k]))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf, eager[k])
        _assert_stats(st, want[k], 'replay of content %d' % k)


# ---------------------------------------------------------------- 5. refusals through the C ABI
def test_refusals_through_the_c_abi_leave_the_outputs_alone():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    lib = L.load()
    n, h, w = 2, 8, 16
    x = SR.case_frames((n, h, w), 10, seed=9)
    raw = torch.from_numpy(x).cuda()
    st = F.raw_statistics(n, h, w, zone=(4, 8), bins=16, hist_shift=6)
    big_z, big_h = _guarded(st)
    st.zones.fill_(PATTERN64), st.hist.fill_(PATTERN32)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def stats(raw_p=p(raw), bits=16, stride=2 * w, black=0, zones=p(st.zones), hist=p(st.hist), zh=4, zw=8, bins=16, shift=6, lo=0,
              hi=65535, N=n, H=h, W=w):
        return lib.risp_raw_stats(raw_p, bits, stride, black, zones, hist, zh, zw, bins, shift, lo, hi, N, H, W, F._stream())

    refused = {'null input': (dict(raw_p=None), b'null'), 'null zones': (dict(zones=None), b'null'), 'null hist': (dict(hist=None), b'null'),
               'bits 14': (dict(bits=14), b'bits 14'), 'H 7': (dict(H=7), b'H=7'), 'W 6': (dict(W=6), b'W 6'), 'W 0': (dict(W=0), b'W 0'),
               'a short stride': (dict(stride=2 * w - 2), b'stride'), 'black -1': (dict(black=-1), b'black_level -1'),
               'zone_h 3': (dict(zh=3), b'zone_h 3'), 'zone_h 0': (dict(zh=0), b'zone_h 0'), 'zone_w 6': (dict(zw=6), b'zone_w 6'),
               'zone_w 0': (dict(zw=0), b'zone_w 0'), 'too many zones': (dict(H=1024, W=1024, zh=2, zw=4, stride=2048), b'65536'),
               'bins 0': (dict(bins=0), b'bins 0'), 'bins 1025': (dict(bins=1025), b'bins 1025'),
               'shift 17': (dict(shift=17), b'hist_shift 17'), 'shift -1': (dict(shift=-1), b'hist_shift -1'),
               'lo -1': (dict(lo=-1), b'lo -1'), 'hi 65536': (dict(hi=65536), b'hi 65536'), 'lo above hi': (dict(lo=9, hi=8), b'lo 9, hi 8'),
               'zones 4-byte aligned': (dict(zones=C.c_void_p(st.zones.data_ptr() + 4)), b'aligned'),
               'a packed row too short': (dict(bits=10, stride=w * 10 // 8 - 1), b'stride')}
    for what, (kw, word) in refused.items():
        assert stats(**kw) != 0, '%s was accepted' % what
        err = lib.risp_last_error()
        assert b'risp_raw_stats' in err and word in err, (what, err)
    torch.cuda.synchronize()
    assert (big_z == PATTERN64).all().item() and (big_h == PATTERN32).all().item(), 'a refused call wrote to its outputs'
    assert stats(black=100, lo=5, hi=700) == 0, lib.risp_last_error()
    torch.cuda.synchronize()
    _assert_guards(big_z, big_h)
    _assert_stats(st, SR.stats_ref(x, 100, (4, 8), 16, 6, 5, 700), 'the accepted call')
