"""GPU: defective-pixel correction in the serving path - the launch (risp_raw_defect, from uint16 and from MIPI-packed frames, with
and without the gains of a lens shading) and ``serve(defect_correction=...)`` / ``serve_frame`` on every route.

The correction is an integer function of the frame (include/risp.h) and everything behind the corrected sample is unchanged, so
every comparison is ``torch.equal`` / ``np.array_equal``: the launch against tests/defect_reference.py (numpy), every serving call
against the same call on the frames that reference corrects.  Nothing here has a tolerance.  The inputs are those of
tests/defect_reference.py (``frame_set``, ``PARAMS``, ``random_bitmap``); tests/test_defect_reference_cpu.py asserts that they tell
every wrong variant of the definition apart.

Shapes: (3,4) - every index reflects, the smallest legal frame, one thread; (4,4), (4,8), (6,12); (3,20) - odd H, five column
groups; (34,68) - crosses the serving tile, W % 32 != 0, two map words and a partial third per row; (37,132), for the launch only:
a thread walks 8 rows, 37 % 8 = 5 leaves a short last strip, and 33 column groups put a strip change inside a wave.  Every frame,
map and gain tensor lies inside a larger allocation of 0xFF bytes - uint16 frames at byte 0, 8 (the 8-byte loads) and 2 (single
loads), packed frames at odd bytes with odd strides - so that a read outside shows."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import defect_reference as DR
import lens_shading_reference as LS
import raw_packed_reference as PR
from raw_placement import _place16, _place_packed

pytestmark = pytest.mark.gpu

PHASES = ['rggb', 'grbg', 'gbrg', 'bggr']
ROUTES = ['fused', 'classical', 'composed', 'scene', 'denoise', 'median', 'cond', 'denoise_scene']
ALL_FUSED = frozenset({'u16', 'raw10', 'raw12'})


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


def _place_bitmap(m):
    """the numpy (H,words) int32 bitmap as a contiguous device view one word into an allocation of 0xFF bytes"""
    big = torch.full((m.size + 2,), -1, dtype=torch.int32).cuda()
    view = big[1:1 + m.size].view(m.shape)
    view.copy_(torch.from_numpy(m))
    assert view.is_contiguous()
    return view


def _gains(h, w, cell, seed, full=False):
    """(numpy map, (device gains, cell)) of tests/test_gpu_serve_shade.py"""
    import test_gpu_serve_shade as SH
    return SH._map(h, w, cell, seed, full)


def _settings(h, w, seed):
    """[(threshold, slope, numpy bitmap or None)]: the dynamic test alone, the map alone, both"""
    m = DR.random_bitmap(h, w, seed)
    return [(t, s, None) for t, s in DR.PARAMS] + [(None, 0, m), (16, 32, m)]


def _dc(setting, dev_maps):
    thr, slope, m = setting
    if m is None:
        return (thr, slope, None)
    key = id(m)
    if key not in dev_maps:
        dev_maps[key] = _place_bitmap(m)
    return (thr, slope, dev_maps[key])


# ---------------------------------------------------------------- 1. the launch
@pytest.mark.parametrize('h,w', DR.LAUNCH_SHAPES, ids=lambda v: str(v))
def test_raw_defect_equals_the_reference(h, w):
    import reconfigisp_amd.functional as F
    settings, dev_maps = _settings(h, w, seed=h + w), {}
    corrected = 0
    for n in (1, 3):
        # uint16 in: byte 0 and 8 (8-byte loads) and byte 2 (single loads) of a larger allocation
        for kind in DR.KINDS:
            x = DR.frame_set(kind, h, w)[:n]
            devs = [_place16(x, at) for at in (0, 4, 1)]
            for setting in settings:
                want = DR.dpc_ref(x, *setting)
                corrected += int((want != x).sum())
                for at, dev in zip((0, 4, 1), devs):
                    got, calls = _counted(lambda: F.raw_defect(dev, _dc(setting, dev_maps)))
                    assert calls == {'risp_raw_defect': 1}
                    assert got.dtype == torch.uint16 and tuple(got.shape) == (n, h, w)
                    assert np.array_equal(got.cpu().numpy(), want), 'u16 %s %dx%dx%d %s at %d: %d differ' % (
                        kind, n, h, w, setting[:2], at, (got.cpu().numpy() != want).sum())
        # RAW10 / RAW12 in: the launch decodes; odd strides, the base one byte into a larger allocation
        for bits in (10, 12):
            used = w * bits // 8
            frames = [DR.frame_set('ten', h, w)[:n], DR.frame_set('low', h, w)[:n]]
            if bits == 12:
                frames.append(PR.full_range_frame(n, h, w, 12, seed=h))
            for x in frames:
                pks = [(stride, offset, _place_packed(x, bits, stride, offset))
                       for stride, offset in ((used, 0), (used + 3, 1), ((used + 63) // 64 * 64, 1))]
                for setting in settings:
                    want = DR.dpc_ref(x, *setting)
                    for stride, offset, pk in pks:
                        got, calls = _counted(lambda: F.raw_defect(pk, _dc(setting, dev_maps), bits, w))
                        assert calls == {'risp_raw_defect': 1}
                        assert np.array_equal(got.cpu().numpy(), want), 'raw%d %dx%dx%d %s stride %d offset %d' % (
                            bits, n, h, w, setting[:2], stride, offset)
    assert corrected > 0
    # a single (H,W) frame; out= is honoured and nothing beside it written; an aliasing out is refused
    x = DR.frame_set('ten', h, w)[:2]
    dev, dc = torch.from_numpy(x).cuda(), _dc(settings[-1], dev_maps)
    want = torch.from_numpy(DR.dpc_ref(x, *settings[-1]))
    assert torch.equal(F.raw_defect(dev[1], dc).cpu(), want[1])
    big = torch.full((2 * h * w + 8,), 0xA5A5, dtype=torch.uint16).cuda()
    out = big[4:4 + 2 * h * w].view(2, h, w)
    assert F.raw_defect(dev, dc, out=out) is out
    assert torch.equal(out.cpu(), want) and (big[:4].cpu() == 0xA5A5).all() and (big[4 + 2 * h * w:].cpu() == 0xA5A5).all()
    with pytest.raises(ValueError, match='aligned'):
        F.raw_defect(dev, dc, out=big[1:1 + 2 * h * w].view(2, h, w))           # 2-byte aligned only
    both = torch.zeros((3, h, w), dtype=torch.uint16).cuda()
    for alias in (both[:2], both[1:]) if (h * w) % 4 == 0 else (both[:2],):
        with pytest.raises(ValueError, match='shares memory'):
            F.raw_defect(both[:2], dc, out=alias)
    with pytest.raises(ValueError, match='black_level'):
        F.raw_defect(dev, dc, black_level=64)                                   # a black level has no meaning without gains


# ---------------------------------------------------------------- 2. with gains: corrected and shaded in the one launch
@pytest.mark.parametrize('h,w', DR.SHAPES + [(37, 132)], ids=lambda v: str(v))
@pytest.mark.parametrize('cell', [4, 64])
def test_raw_defect_with_gains_equals_shading_the_corrected_frames(cell, h, w):
    import reconfigisp_amd.functional as F
    k = cell.bit_length() - 1
    settings, dev_maps = _settings(h, w, seed=h + w + 1), {}
    for n, black in itertools.product((1, 3), (0, 64)):
        gains, shading = _gains(h, w, cell, seed=10 * n + black + h)
        for kind in DR.KINDS:
            x = DR.frame_set(kind, h, w)[:n]
            devs = [_place16(x, at) for at in (0, 1)]
            packed = None if kind == 'full' else _place_packed(x, 10, w * 10 // 8 + 3, 1)
            for setting in settings[2:]:
                want = LS.shade_ref(DR.dpc_ref(x, *setting), black, gains, k)
                dc = _dc(setting, dev_maps)
                for dev in devs:
                    got, calls = _counted(lambda: F.raw_defect(dev, dc, shading=shading, black_level=black))
                    assert calls == {'risp_raw_defect': 1}
                    assert np.array_equal(got.cpu().numpy(), want), (kind, n, h, w, cell, black, setting[:2])
                if packed is not None:
                    got = F.raw_defect(packed, dc, 10, w, shading, black)
                    assert np.array_equal(got.cpu().numpy(), want), ('raw10', kind, n, h, w, cell, black, setting[:2])
    # the overflow of the shading: an all-65535 map under the full-range frame
    gains, shading = _gains(h, w, cell, seed=1, full=True)
    x = DR.frame_set('full', h, w)
    for setting in (settings[0], settings[-1]):
        want = LS.shade_ref(DR.dpc_ref(x, *setting), 0, gains, k)
        assert np.array_equal(F.raw_defect(_place16(x, 0), _dc(setting, dev_maps), shading=shading).cpu().numpy(), want)


# ---------------------------------------------------------------- 3. serve(defect_correction=...) on every route
def _route_case(what):
    """(net, keywords of serve(), the route they take) - the route constructors of the existing GPU tests"""
    import test_gpu_serve_median as MD
    import test_gpu_serve_shade as SH
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    if what == 'median':
        return MD._net(sorted(PF._MEDIAN_SIZES)[0] if PF._MEDIAN_SIZES else 5), dict(fast_median=True), 'denoise'
    return SH._route_case(what)


def _asymmetric_map(h, w, seed):
    m = DR.random_bitmap(h, w, seed)
    listed = DR.listed_ref(m, h, w)
    assert not np.array_equal(listed, listed[:, ::-1]) and not np.array_equal(listed, listed[::-1])
    return m


def _sources(x, w):
    """[(raw_format, device frames, keywords)]: uint16 and both packed formats, the packed ones at odd bytes and strides"""
    out = [('u16', torch.from_numpy(x).cuda(), {})]
    for fmt, bits in (('raw10', 10), ('raw12', 12)):
        out.append((fmt, _place_packed(x, bits, w * bits // 8 + 3, 1), dict(raw_format=fmt, raw_width=w)))
    return out


@pytest.mark.parametrize('what', ROUTES)
def test_serve_corrects_defects_on_every_route(what):
    n, h, w, black, white = 2, 34, 68, 64, 1023.0
    net, kw, route = _route_case(what)
    x = PR.full_range_frame(n, h, w, 10, seed=61)
    m = _asymmetric_map(h, w, seed=62)
    dc = (16, 32, _place_bitmap(m))
    fixed = DR.dpc_ref(x, 16, 32, m)
    assert 0.05 < (fixed != x).mean() < 0.3
    ref = torch.from_numpy(fixed).cuda()
    sensor = dict(black_level=black, cfa='grbg')
    want = net.serve(ref, white, **sensor, **kw).clone()
    assert net.last_serve_route == route and net.last_serve_defect is None
    _, plain_calls = _counted(lambda: net.serve(ref, white, **sensor, **kw))
    for fmt, src, fkw in _sources(x, w):
        got, calls = _counted(lambda: net.serve(src, white, defect_correction=dc, **sensor, **fkw, **kw))
        assert net.last_serve_route == route and net.last_serve_defect == 'pass' and net.last_serve_shade is None
        assert net.last_serve_load == (None if fmt == 'u16' else 'pass')
        assert calls == dict(plain_calls, risp_raw_defect=1), (fmt, calls, plain_calls)
        assert 'risp_raw_unpack' not in calls
        assert torch.equal(got, want), '%s %s: %d bytes differ' % (fmt, what, (got != want).sum().item())
        # 5. None passed explicitly is the call without the keyword: today's bytes, today's calls
        plain, today = _counted(lambda: net.serve(src, white, **sensor, **fkw, **kw))
        plain = plain.clone()
        none, none_calls = _counted(lambda: net.serve(src, white, defect_correction=None, **sensor, **fkw, **kw))
        assert torch.equal(none, plain) and none_calls == today and net.last_serve_defect is None
        assert 'risp_raw_defect' not in none_calls and not torch.equal(plain, want)
    assert len(torch.unique(want)) > 8
    src = torch.from_numpy(x).cuda()
    # all four phases: the map belongs to the frame as stored - a mirrored map fails
    for phase in PHASES:
        want_p = net.serve(ref, white, black_level=black, cfa=phase, **kw).clone()
        got_p = net.serve(src, white, black_level=black, cfa=phase, defect_correction=dc, **kw)
        assert net.last_serve_route == route and torch.equal(got_p, want_p), (what, phase)
    # the map alone, the dynamic test alone
    for thr, slope, bitmap, dev_map in ((None, 0, m, dc[2]), (0, 255, None, None)):
        want_s = net.serve(torch.from_numpy(DR.dpc_ref(x, thr, slope, bitmap)).cuda(), white, **sensor, **kw).clone()
        assert torch.equal(net.serve(src, white, defect_correction=(thr, slope, dev_map), **sensor, **kw), want_s), (what, thr)
    # NV12 out, on the same route
    want12 = net.serve(ref, white, out_format='nv12', yuv_matrix='bt709_full', **sensor, **kw).clone()
    got12 = net.serve(src, white, out_format='nv12', yuv_matrix='bt709_full', defect_correction=dc, **sensor, **kw)
    assert net.last_serve_route == route and net.last_serve_defect == 'pass' and torch.equal(got12, want12)
    # out= given: the same bytes, and a warm call allocates nothing
    buf = torch.empty_like(want)
    net.serve(src, white, out=buf, defect_correction=dc, **sensor, **kw)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert net.serve(src, white, out=buf, defect_correction=dc, **sensor, **kw) is buf
    if what != 'composed':                                 # (the composed route allocates its fp32 planes either way)
        assert torch.cuda.memory_allocated() == before
    assert torch.equal(buf, want)


@pytest.mark.parametrize('what', ROUTES)
def test_serve_corrects_in_front_of_a_lens_shading_with_one_launch_or_two(what, monkeypatch):
    """both answers of ``defect_shade``, whatever the measured table holds today"""
    import test_gpu_serve_shade as SH
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    n, h, w, cell, black, white = 2, 34, 68, 16, 64, 1023.0
    net, kw, route = _route_case(what)
    x = PR.full_range_frame(n, h, w, 10, seed=63)
    m = _asymmetric_map(h, w, seed=64)
    dc = (16, 32, _place_bitmap(m))
    gains, shading = _gains(h, w, cell, seed=65)
    ref = SH._shaded(DR.dpc_ref(x, 16, 32, m), black, gains, cell)
    want = net.serve(ref, white - black, black_level=0, cfa='gbrg', **kw).clone()
    _, plain_calls = _counted(lambda: net.serve(ref, white - black, black_level=0, cfa='gbrg', **kw))
    sensor = dict(black_level=black, cfa='gbrg', lens_shading=shading, defect_correction=dc)
    for table in (frozenset(), ALL_FUSED, frozenset({'raw10'})):
        monkeypatch.setattr(PF, '_DEFECT_SHADE_FUSED', table)
        for fmt, src, fkw in _sources(x, w):
            got, calls = _counted(lambda: net.serve(src, white, **sensor, **fkw, **kw))
            answer = PF.defect_shade(fmt)
            assert answer == ('fused' if fmt in table else 'pass')
            assert net.last_serve_route == route and net.last_serve_defect == answer and net.last_serve_shade == 'pass'
            assert net.last_serve_load == (None if fmt == 'u16' else 'pass')
            expect = dict(plain_calls, risp_raw_defect=1)
            if answer == 'pass':
                expect['risp_raw_shade'] = 1
            assert calls == expect, (fmt, table, calls, plain_calls)
            assert torch.equal(got, want), '%s %s %s: %d bytes differ' % (fmt, what, answer, (got != want).sum().item())
    assert len(torch.unique(want)) > 8


def test_the_model_wrapper_passes_the_keyword_on():
    import test_gpu_serve_frame as SF
    model = SF._model('classical')
    n, h, w = 1, 6, 12
    x = DR.frame_set('ten', h, w)[:n]
    dev = torch.from_numpy(x).cuda()
    want = model.serve(torch.from_numpy(DR.dpc_ref(x, 0, 0, None)).cuda(), 1023.0, black_level=64).clone()
    assert torch.equal(model.serve(dev, 1023.0, black_level=64, defect_correction=(0, 0, None)), want)
    assert model.netG.last_serve_defect == 'pass'
    assert not torch.equal(model.serve(dev, 1023.0, black_level=64), want) and model.netG.last_serve_defect is None
    # (65535, 255) corrects nothing: the bytes of the call without the keyword
    assert torch.equal(model.serve(dev, 1023.0, black_level=64, defect_correction=(65535, 255, None)),
                       model.serve(dev, 1023.0, black_level=64))


# ---------------------------------------------------------------- 4. full frames in tiles
@pytest.mark.parametrize('fmt', ['u16', 'raw10', 'raw12'])
@pytest.mark.parametrize('shaded', [False, True], ids=['plain', 'shaded'])
def test_serve_frame_corrects_once_in_front_of_the_tiles(shaded, fmt, monkeypatch):
    import test_gpu_serve_frame as SF
    import test_gpu_serve_shade as SH
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    model = SF._model('classical')
    net = model.netG
    n, h, w, cell, black, white = 2, 34, 68, 16, 64, 1023.0
    size, stride = (20, 40), (14, 28)                       # a 2 x 2 tile geometry
    assert PF.frame_geometry(h, w, size, stride, 'gbrg', 'cuda')[0].shape[0] == 4
    x = PR.full_range_frame(n, h, w, 10, seed=66)
    m = _asymmetric_map(h, w, seed=67)
    dc = (16, 32, _place_bitmap(m))
    fixed = DR.dpc_ref(x, 16, 32, m)
    kw = dict(tile_batch=3, cfa='gbrg')
    if shaded:
        gains, shading = _gains(h, w, cell, seed=68)
        want = net.serve_frame(SH._shaded(fixed, black, gains, cell), white - black, size, stride, black_level=0, **kw).clone()
        extra = dict(lens_shading=shading)
    else:
        want = net.serve_frame(torch.from_numpy(fixed).cuda(), white, size, stride, black_level=black, **kw).clone()
        extra = {}
    assert net.last_serve_route == 'tiled' and net.last_serve_defect is None
    bits = {'u16': 16, 'raw10': 10, 'raw12': 12}[fmt]
    if fmt == 'u16':
        src, fkw = torch.from_numpy(x).cuda(), {}
    else:
        src, fkw = _place_packed(x, bits, w * bits // 8 + 3, 1), dict(raw_format=fmt, raw_width=w)
    for table in (frozenset(), ALL_FUSED):
        monkeypatch.setattr(PF, '_DEFECT_SHADE_FUSED', table)
        got, calls = _counted(lambda: net.serve_frame(src, white, size, stride, black_level=black, defect_correction=dc, **extra,
                                                      **fkw, **kw))
        answer = (PF.defect_shade(fmt) if shaded else 'pass')
        assert net.last_serve_route == 'tiled' and net.last_serve_defect == answer
        assert net.last_serve_shade == ('pass' if shaded else None) and net.last_serve_load == (None if fmt == 'u16' else 'pass')
        assert calls.get('risp_raw_defect') == 1 and 'risp_raw_unpack' not in calls, calls
        assert calls.get('risp_raw_shade', 0) == (1 if shaded and answer == 'pass' else 0), calls
        assert tuple(got.shape) == (n, h, w, 3) and torch.equal(got, want), (fmt, shaded, table)
    one = model.serve_frame(src[0], white, size, stride, black_level=black, defect_correction=dc, **extra, **fkw, **kw)
    assert tuple(one.shape) == (h, w, 3) and torch.equal(one, want[0])                   # (H,W) / (H,stride)
    plain = net.serve_frame(src, white, size, stride, black_level=black, **extra, **fkw, **kw).clone()
    assert torch.equal(net.serve_frame(src, white, size, stride, black_level=black, defect_correction=None, **extra, **fkw, **kw), plain)
    assert net.last_serve_defect is None and not torch.equal(plain, want)


# ---------------------------------------------------------------- 6. a captured graph
@pytest.mark.parametrize('route', ['fused', 'classical'])
@pytest.mark.parametrize('shaded', [False, True], ids=['plain', 'shaded'])
def test_a_corrected_call_replays_from_a_graph(shaded, route):
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    import test_gpu_serve_shade as SH
    n, h, w, cell, black, white = 3, 34, 68, 16, 64, 1023.0
    net = CF._pipeline(CF.HEADLINE if route == 'fused' else SC.ARCHS[0])
    m = _asymmetric_map(h, w, seed=69)
    dc = (16, 32, _place_bitmap(m))
    xa, xb = PR.full_range_frame(n, h, w, 10, seed=1), PR.full_range_frame(n, h, w, 10, seed=2)
    sensor = dict(black_level=black, cfa='grbg', defect_correction=dc)
    if shaded:
        gains, shading = _gains(h, w, cell, seed=8)
        sensor['lens_shading'] = shading
        eager = [net.serve(SH._shaded(DR.dpc_ref(x, 16, 32, m), black, gains, cell), white - black, cfa='grbg').clone() for x in (xa, xb)]
    else:
        eager = [net.serve(torch.from_numpy(DR.dpc_ref(x, 16, 32, m)).cuda(), white, black_level=black, cfa='grbg').clone()
                 for x in (xa, xb)]
    assert not torch.equal(eager[0], eager[1])
    slot, buf = torch.from_numpy(xa).cuda(), torch.zeros((n, h, w, 3), device='cuda', dtype=torch.uint8)
    net.serve(slot, white, out=buf, **sensor)               # fills the caches
    assert net.last_serve_route == route and torch.equal(buf, eager[0])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    net.serve(slot, white, out=buf, **sensor)
    assert torch.cuda.memory_allocated() == before
    buf.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.serve(slot, white, out=buf, **sensor)
    slot.copy_(torch.from_numpy(xb))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager[1])


# ---------------------------------------------------------------- 7. refusals through the C ABI
def test_refusals_through_the_c_abi_leave_the_output_alone():
    import test_gpu_serve_shade as SH
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    lib = L.load()
    n, h, w, k = 2, 4, 8, 2
    gh, gw = LS.map_shape(h, w, k)
    raw = torch.from_numpy(DR.frame_set('ten', h, w)[:n]).cuda()
    bitmap = _place_bitmap(DR.random_bitmap(h, w, 1))
    gains = SH._place_map(LS.random_map(h, w, k, 1))
    out = torch.full((n * h * w + 8,), 0x5A5A, dtype=torch.uint16).cuda()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def defect(raw_p=p(raw), bits=16, stride=2 * w, out_p=p(out), thr=16, slope=32, defects=bitmap, gains=None, k=0, GH=0, GW=0,
               black=0, H=h, W=w):
        return lib.risp_raw_defect(raw_p, bits, stride, out_p, thr, slope, p(defects), p(gains), k, GH, GW, black, n, H, W, F._stream())

    refused = {'null input': (dict(raw_p=None), b'null'), 'null out': (dict(out_p=None), b'null'),
               'bits 14': (dict(bits=14), b'bits 14'), 'H 2': (dict(H=2), b'H=2'), 'W 6': (dict(W=6), b'W 6'),
               'W 0': (dict(W=0), b'W 0'), 'a short stride': (dict(stride=2 * w - 2), b'stride'),
               'threshold 65536': (dict(thr=65536), b'threshold 65536'), 'threshold -2': (dict(thr=-2), b'threshold -2'),
               'slope 256': (dict(slope=256), b'slope 256'), 'slope -1': (dict(slope=-1), b'slope -1'),
               'neither mode': (dict(thr=-1, defects=None), b'neither'),
               'a cell without gains': (dict(k=2), b'without gains'), 'a map size without gains': (dict(GH=gh, GW=gw), b'without gains'),
               'a black level without gains': (dict(black=64), b'without gains'),
               'gains with k 1': (dict(gains=gains, k=1, GH=gh, GW=gw), b'cell_log2 1'),
               'gains one row short': (dict(gains=gains, k=k, GH=gh - 1, GW=gw), ('a %d x %d map' % (gh - 1, gw)).encode()),
               'out 2-byte aligned': (dict(out_p=C.c_void_p(out.data_ptr() + 2)), b'aligned'),
               'a packed row too short': (dict(bits=10, stride=w * 10 // 8 - 1), b'stride')}
    for what, (kw, word) in refused.items():
        assert defect(**kw) != 0, '%s was accepted' % what
        err = lib.risp_last_error()
        assert b'risp_raw_defect' in err and word in err, (what, err)
    torch.cuda.synchronize()
    assert (out.cpu() == 0x5A5A).all().item(), 'a refused call wrote to its output'
    # the same arguments without the fault are accepted and write the frames alone
    x = raw.cpu().numpy()
    for kw, want in ((dict(), DR.dpc_ref(x, 16, 32, DR.random_bitmap(h, w, 1))),
                     (dict(thr=-1, slope=255), DR.dpc_ref(x, None, 0, DR.random_bitmap(h, w, 1))),
                     (dict(defects=None), DR.dpc_ref(x, 16, 32, None)),
                     (dict(gains=gains, k=k, GH=gh, GW=gw, black=64),
                      LS.shade_ref(DR.dpc_ref(x, 16, 32, DR.random_bitmap(h, w, 1)), 64, LS.random_map(h, w, k, 1), k))):
        out.fill_(0x5A5A)
        assert defect(**kw) == 0, lib.risp_last_error()
        torch.cuda.synchronize()
        assert (out[n * h * w:].cpu() == 0x5A5A).all().item()
        assert np.array_equal(out[:n * h * w].cpu().numpy().reshape(n, h, w), want), kw
