"""GPU: lens-shading correction in the serving path - the shade launch (risp_raw_shade, from uint16 and from MIPI-packed frames),
the fused shading load of the classical one-launch kernel (risp_serve_classical_shaded) and ``serve(lens_shading=...)`` on every
route.

Shading is an integer function of the sample, its place and the map (include/risp.h), and everything behind the sample is
unchanged, so every comparison is ``torch.equal``: the shade launch against tests/lens_shading_reference.py (numpy), every serving
call against the same call on the frames that reference shades, with black level 0 and the divisor white - black.  Nothing here
has a tolerance.

Shapes as in tests/test_gpu_serve_packed.py: a thread of the serving kernel owns a 2 x 4 patch and reads columns px-2 .. px+5, a
workgroup a 64 x 32 pixel tile - (4,4) is one patch, both border pairs reflected into it; (4,8) and (6,12) have border and
interior patches; (34,68) crosses the tile both ways.  The shade launch owns 16 pixels of a row per thread: (3,20) and (34,68) end
a row with a shorter chunk, (2,64) has full chunks only, (1,4) is one group.  Cells: 4 (a thread's eight columns span three
cells, a chunk four), 8 (a cell border inside a thread's span at px = 4), 16, and 64 (one cell larger than every frame here,
GH = GW = 2).  Maps: random gains 2048 .. 32767, different in every plane and node, so a plane or a node taken wrongly shows;
and one all-65535 map under a full-range 16-bit frame, whose sums pass 2^31.  Every map lies inside a larger allocation of 0xFFFF
words, so that a node read outside it shows."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import lens_shading_reference as LS
import raw_packed_reference as PR
from raw_placement import _place16, _place_packed

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4), (4, 8), (6, 12), (34, 68)]
CELLS = [4, 8, 16, 64]
PHASES = ['rggb', 'grbg', 'gbrg', 'bggr']


def _log2(cell):
    return cell.bit_length() - 1


def _place_map(gains):
    """the numpy (GH,GW,4) map as a contiguous device view 8 bytes into an allocation of 0xFFFF words"""
    big = torch.full((gains.size + 8,), 0xFFFF, dtype=torch.uint16).cuda()
    view = big[4:4 + gains.size].view(gains.shape)
    view.copy_(torch.from_numpy(gains))
    assert view.is_contiguous() and view.data_ptr() % 8 == 0
    return view


def _map(h, w, cell, seed, full=False):
    """(numpy map, (device gains, cell))"""
    g = LS.random_map(h, w, _log2(cell), seed)
    if full:
        g[...] = 65535
    return g, (_place_map(g), cell)


def _frames16(n, h, w, seed):
    """full-range 16-bit frames, the extremes present"""
    f = np.random.default_rng(seed).integers(0, 65536, (n, h, w)).astype(np.uint16)
    f[0, 0, 0], f[0, -1, -1] = 65535, 0
    return f


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


def _shaded(x, black, gains, cell):
    """the reference's shaded frames on the device"""
    return torch.from_numpy(LS.shade_ref(x, black, gains, _log2(cell))).cuda()


# ---------------------------------------------------------------- 1. the shade launch
@pytest.mark.parametrize('h,w', SHAPES + [(1, 4), (3, 20), (2, 64)], ids=lambda v: str(v))
@pytest.mark.parametrize('cell', CELLS)
def test_raw_shade_equals_the_reference(cell, h, w):
    import reconfigisp_amd.functional as F
    k = 0
    for n, black in itertools.product((1, 3), (0, 64)):
        k += 1
        gains, shading = _map(h, w, cell, seed=10 * k + h)
        # uint16 in: an 8-byte aligned base (the vector load) and one a word into a larger allocation (single loads)
        x = _frames16(n, h, w, seed=k)
        want = LS.shade_ref(x, black, gains, _log2(cell))
        for at in (0, 4, 1):
            dev = _place16(x, at)
            got, calls = _counted(lambda: F.raw_shade(dev, shading, black))
            assert calls == {'risp_raw_shade': 1}
            assert got.dtype == torch.uint16 and tuple(got.shape) == (n, h, w)
            assert np.array_equal(got.cpu().numpy(), want), 'u16 %dx%dx%d cell %d black %d at %d' % (n, h, w, cell, black, at)
        # RAW10 / RAW12 in: the launch decodes and shades; odd strides, the base one byte into a larger allocation
        for bits in (10, 12):
            xp = PR.full_range_frame(n, h, w, bits, seed=k + bits)
            used = w * bits // 8
            for stride, offset in ((used, 0), (used + 3, 1), ((used + 63) // 64 * 64, 1)):
                pk = _place_packed(xp, bits, stride, offset)
                got, calls = _counted(lambda: F.raw_shade(pk, shading, black, bits, w))
                assert calls == {'risp_raw_shade': 1}
                assert np.array_equal(got.cpu().numpy(), LS.shade_ref(xp, black, gains, _log2(cell))), \
                    'raw%d %dx%dx%d cell %d black %d stride %d offset %d' % (bits, n, h, w, cell, black, stride, offset)
    # the overflow: an all-65535 map under a full-range 16-bit frame - both sums pass 2^31
    gains, shading = _map(h, w, cell, seed=1, full=True)
    x = _frames16(2, h, w, seed=77)
    want = LS.shade_ref(x, 0, gains, _log2(cell))
    assert not np.array_equal(want, LS.shade_signed32(x, 0, gains, _log2(cell)))
    assert np.array_equal(F.raw_shade(torch.from_numpy(x).cuda(), shading).cpu().numpy(), want)
    # a single (H,W) frame; out= is honoured and nothing beside it written
    gains, shading = _map(h, w, cell, seed=3)
    dev = torch.from_numpy(x).cuda()
    want = torch.from_numpy(LS.shade_ref(x, 64, gains, _log2(cell)))
    assert torch.equal(F.raw_shade(dev[1], shading, 64).cpu(), want[1])
    big = torch.full((2 * h * w + 8,), 0xA5A5, dtype=torch.uint16).cuda()
    out = big[4:4 + 2 * h * w].view(2, h, w)
    assert F.raw_shade(dev, shading, 64, out=out) is out
    assert torch.equal(out.cpu(), want) and (big[:4].cpu() == 0xA5A5).all() and (big[4 + 2 * h * w:].cpu() == 0xA5A5).all()
    with pytest.raises(ValueError):
        F.raw_shade(dev, shading, 64, out=big[1:1 + 2 * h * w].view(2, h, w))       # 2-byte aligned only


# ---------------------------------------------------------------- 2. the fused shading load, entry point against entry point
@pytest.mark.parametrize('h,w', SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize('cell', CELLS)
def test_serve_classical_shaded_equals_serve_classical_u8_on_the_shaded_frames(cell, h, w):
    """H != W at three shapes and the map is random: a map mirrored with the mosaic fails on every phase but rggb"""
    import reconfigisp_amd.functional as F
    import test_gpu_serve_classical as SC
    WB, GA, FI, WQ = F.OP_WB_MANUAL, F.OP_GAMMA, F.OP_TONE_FILMIC, F.OP_WB_QUADRATIC
    k = 0
    for black in (0, 64):
        for phase in PHASES:
            for demosaic in SC.KINDS:
                for ops in ([WB, FI, GA], [WQ, FI]):
                    k += 1
                    n = (1, 3)[k % 2]
                    gains, shading = _map(h, w, cell, seed=k)
                    x = PR.full_range_frame(n, h, w, 12, seed=k)
                    white = 16383                           # gains reach 8: a part of the samples stays below the white level
                    pars = SC._params(n, 200 + k, k % 3)
                    params = [pars[op] for op in ops]
                    reverse = bool(k & 2)
                    want = F.serve_classical_u8(_shaded(x, black, gains, cell), float(white - black), demosaic, ops, params, reverse,
                                                black_level=0, cfa=phase)
                    got, calls = _counted(lambda: F.serve_classical_shaded(torch.from_numpy(x).cuda(), shading, float(white - black),
                                                                           demosaic, ops, params, reverse, black_level=black,
                                                                           cfa=phase))
                    assert calls == {'risp_serve_classical_shaded': 1}
                    assert torch.equal(got, want), '%dx%dx%d cell %d black %d %s %s: %d bytes differ' % (
                        n, h, w, cell, black, phase, demosaic, (got != want).sum().item())
    assert h * w < 64 or len(torch.unique(got)) > 4, 'a flat image would prove nothing'
    # the overflow, through the serving kernel
    gains, shading = _map(h, w, cell, seed=1, full=True)
    x = _frames16(1, h, w, seed=5)
    for demosaic in SC.KINDS:
        want = F.serve_classical_u8(_shaded(x, 0, gains, cell), 65535.0, demosaic, [], [], cfa='bggr')
        assert torch.equal(F.serve_classical_shaded(torch.from_numpy(x).cuda(), shading, 65535.0, demosaic, [], [], cfa='bggr'), want)


@pytest.mark.parametrize('h,w', [(4, 4), (6, 12), (34, 68)], ids=lambda v: str(v))
@pytest.mark.parametrize('cell', CELLS)
def test_serve_classical_shaded_stores_nv12(cell, h, w):
    import reconfigisp_amd.functional as F
    import test_gpu_serve_classical as SC
    matrices = list(F.NV12_MATRIX)
    for k, (phase, black) in enumerate(itertools.product(PHASES, (0, 64))):
        n = (1, 3)[k % 2]
        gains, shading = _map(h, w, cell, seed=300 + k)
        x = PR.full_range_frame(n, h, w, 12, seed=300 + k)
        matrix, div = matrices[k % 4], float(16383 - black)
        pars = SC._params(n, 300 + k, k % 3)
        ops = [F.OP_WB_MANUAL, F.OP_TONE_FILMIC, F.OP_GAMMA]
        params = [pars[op] for op in ops]
        for demosaic in SC.KINDS:
            want = F.serve_classical_nv12(_shaded(x, black, gains, cell), div, demosaic, ops, params, matrix, black_level=0, cfa=phase)
            got = F.serve_classical_shaded(torch.from_numpy(x).cuda(), shading, div, demosaic, ops, params, matrix=matrix,
                                           black_level=black, cfa=phase)
            assert tuple(got.shape) == (n, h + h // 2, w) and torch.equal(got, want), (cell, h, w, phase, black, demosaic)
    with pytest.raises(ValueError, match='reverse_channels'):
        F.serve_classical_shaded(torch.from_numpy(x).cuda(), shading, div, 'bilinear', [], [], reverse_channels=True, matrix='bt601_full')


# ---------------------------------------------------------------- 3. serve(lens_shading=...) on every route
def _route_case(what):
    """(net, keywords of serve(), the route they take) - the module lists of tests/test_gpu_serve_nv12.py"""
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    import test_gpu_serve_nv12 as NV
    if what == 'fused':
        return CF._pipeline(CF.HEADLINE), {}, 'fused'
    if what == 'classical':
        return CF._pipeline(SC.ARCHS[0]), {}, 'classical'
    net, _, kw, route = NV._pass_case(what)
    return net, kw, route


@pytest.mark.parametrize('what', ['fused', 'classical', 'scene', 'denoise', 'cond', 'denoise_scene', 'composed'])
@pytest.mark.parametrize('fmt', ['u16', 'raw10'])
def test_serve_takes_a_lens_shading_on_every_route(fmt, what):
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    n, h, w, cell, black, white = 2, 34, 68, 16, 64, 4095.0
    net, kw, route = _route_case(what)
    gains, shading = _map(h, w, cell, seed=40)
    x = PR.full_range_frame(n, h, w, 10, seed=41)
    ref = _shaded(x, black, gains, cell)
    if fmt == 'u16':
        src, fkw = torch.from_numpy(x).cuda(), {}
    else:
        src = _place_packed(x, 10, w * 10 // 8 + 3, 1)
        fkw = dict(raw_format=fmt, raw_width=w)
    want = net.serve(ref, white - black, black_level=0, cfa='grbg', **kw).clone()
    assert net.last_serve_route == route and net.last_serve_shade is None
    _, plain_calls = _counted(lambda: net.serve(ref, white - black, black_level=0, cfa='grbg', **kw))
    sensor = dict(black_level=black, cfa='grbg', lens_shading=shading)
    got, calls = _counted(lambda: net.serve(src, white, **sensor, **fkw, **kw))
    shade = PF.serve_shade(route, fmt)
    assert shade in ('fused', 'pass') and (shade == 'pass' or (route, fmt) == ('classical', 'u16'))
    assert net.last_serve_route == route and net.last_serve_shade == shade
    assert net.last_serve_load == (None if fmt == 'u16' else 'pass')
    if shade == 'pass':
        assert calls == dict(plain_calls, risp_raw_shade=1), (calls, plain_calls)
    else:
        assert calls == {'risp_serve_classical_shaded': 1}, calls
    assert 'risp_raw_unpack' not in calls
    assert torch.equal(got, want), '%s %s: %d bytes differ' % (fmt, what, (got != want).sum().item())
    assert len(torch.unique(got)) > 8
    # NV12 out, on the same route
    want12 = net.serve(ref, white - black, black_level=0, cfa='grbg', out_format='nv12', yuv_matrix='bt709_full', **kw).clone()
    got12 = net.serve(src, white, out_format='nv12', yuv_matrix='bt709_full', **sensor, **fkw, **kw)
    assert net.last_serve_route == route and net.last_serve_shade == shade and torch.equal(got12, want12)
    # out= given: the same bytes, and a warm call allocates nothing
    buf = torch.empty_like(want)
    net.serve(src, white, out=buf, **sensor, **fkw, **kw)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert net.serve(src, white, out=buf, **sensor, **fkw, **kw) is buf
    if what != 'composed':                                 # (the composed route allocates its fp32 planes, shaded or not)
        assert torch.cuda.memory_allocated() == before
    assert torch.equal(buf, want)
    # 7. None passed explicitly is the call without the keyword
    plain = net.serve(src, white, black_level=black, cfa='grbg', **fkw, **kw).clone()
    none, none_calls = _counted(lambda: net.serve(src, white, black_level=black, cfa='grbg', lens_shading=None, **fkw, **kw))
    assert torch.equal(none, plain) and net.last_serve_shade is None and 'risp_raw_shade' not in none_calls
    assert not torch.equal(plain, want)


def test_serve_shades_in_the_classical_launch_where_the_table_says_so(monkeypatch):
    """the branch of ``serve`` behind ``serve_shade(..) == 'fused'``, whatever the measured table holds today: one launch, the same
    bytes, NV12 out included; packed frames and frames that are not 8-byte aligned still take the shade launch"""
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    monkeypatch.setattr(PF, '_FUSED_SHADE', frozenset({('classical', 'u16')}))
    n, h, w, cell, black, white = 2, 34, 68, 8, 64, 4095.0
    gains, shading = _map(h, w, cell, seed=50)
    x = PR.full_range_frame(n, h, w, 10, seed=51)
    ref = _shaded(x, black, gains, cell)
    sensor = dict(black_level=black, cfa='bggr', lens_shading=shading)
    for arch in SC.ARCHS:
        net = CF._pipeline(arch)
        want = net.serve(ref, white - black, cfa='bggr').clone()
        assert net.last_serve_route == 'classical'
        got, calls = _counted(lambda: net.serve(torch.from_numpy(x).cuda(), white, **sensor))
        assert calls == {'risp_serve_classical_shaded': 1} and net.last_serve_route == 'classical' and net.last_serve_shade == 'fused'
        assert torch.equal(got, want), arch
        want12 = net.serve(ref, white - black, cfa='bggr', out_format='nv12').clone()
        got12, calls = _counted(lambda: net.serve(torch.from_numpy(x).cuda(), white, out_format='nv12', **sensor))
        assert calls == {'risp_serve_classical_shaded': 1} and torch.equal(got12, want12), arch
    big = torch.zeros((x.size + 4,), dtype=torch.uint16).cuda()
    odd = big[1:1 + x.size].view(x.shape)
    odd.copy_(torch.from_numpy(x))
    got, calls = _counted(lambda: net.serve(odd, white, **sensor))
    assert calls.get('risp_raw_shade') == 1 and 'risp_serve_classical_shaded' not in calls and net.last_serve_shade == 'pass'
    assert torch.equal(got, want)
    packed = torch.from_numpy(PR.pack(x, 10, None, None)).cuda()
    got, calls = _counted(lambda: net.serve(packed, white, raw_format='raw10', raw_width=w, **sensor))
    assert calls.get('risp_raw_shade') == 1 and 'risp_serve_classical_shaded' not in calls and net.last_serve_shade == 'pass'
    assert torch.equal(got, want)


def test_the_model_wrapper_and_a_flat_map():
    """IspModel passes the keyword on; a map of 4096 everywhere serves the bytes of the call without it"""
    import test_gpu_serve_frame as SF
    model = SF._model('classical')
    n, h, w = 1, 6, 12
    x = PR.full_range_frame(n, h, w, 12, seed=9)
    dev = torch.from_numpy(x).cuda()
    flat = (_place_map(np.full(LS.map_shape(h, w, 3) + (4,), 4096, dtype=np.uint16)), 8)
    assert torch.equal(model.serve(dev, 4095.0, black_level=64, lens_shading=flat), model.serve(dev, 4095.0, black_level=64))
    assert model.netG.last_serve_shade is None
    gains, shading = _map(h, w, 8, seed=2)
    want = model.serve(_shaded(x, 64, gains, 8), 4095.0 - 64)
    assert torch.equal(model.serve(dev, 4095.0, black_level=64, lens_shading=shading), want)
    assert model.netG.last_serve_shade in ('fused', 'pass')


# ---------------------------------------------------------------- 4. full frames in tiles
@pytest.mark.parametrize('fmt', ['u16', 'raw12'])
def test_serve_frame_shades_once_in_front_of_the_tiles(fmt):
    import test_gpu_serve_frame as SF
    model = SF._model('classical')
    net = model.netG
    h, w, cell, black, white = 64, 96, 16, 64, 4095.0
    gains, shading = _map(h, w, cell, seed=6)
    x = PR.full_range_frame(1, h, w, 12, seed=6)
    ref = _shaded(x, black, gains, cell)
    if fmt == 'u16':
        src, fkw = torch.from_numpy(x).cuda(), {}
    else:
        src, fkw = torch.from_numpy(PR.pack(x, 12, w * 12 // 8 + 3, None)).cuda(), dict(raw_format=fmt, raw_width=w)
    kw = dict(tile_batch=4, cfa='gbrg')
    want = net.serve_frame(ref, white - black, 48, 32, black_level=0, **kw).clone()
    assert net.last_serve_route == 'tiled' and net.last_serve_shade is None
    got, calls = _counted(lambda: net.serve_frame(src, white, 48, 32, black_level=black, lens_shading=shading, **fkw, **kw))
    assert net.last_serve_route == 'tiled' and net.last_serve_shade == 'pass'
    assert calls.get('risp_raw_shade') == 1 and 'risp_raw_unpack' not in calls, calls
    assert tuple(got.shape) == (1, h, w, 3) and torch.equal(got, want)
    one = model.serve_frame(src[0], white, 48, 32, black_level=black, lens_shading=shading, **fkw, **kw)       # (H,W) / (H,stride)
    assert tuple(one.shape) == (h, w, 3) and torch.equal(one, want[0])
    plain = net.serve_frame(src, white, 48, 32, black_level=black, **fkw, **kw).clone()
    assert torch.equal(net.serve_frame(src, white, 48, 32, black_level=black, lens_shading=None, **fkw, **kw), plain)
    assert net.last_serve_shade is None and not torch.equal(plain, want)


# ---------------------------------------------------------------- 5. a captured graph
@pytest.mark.parametrize('route', ['fused', 'classical'])
def test_a_shaded_call_replays_from_a_graph(route):
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    n, h, w, cell, black, white = 3, 34, 68, 16, 64, 4095.0
    net = CF._pipeline(CF.HEADLINE if route == 'fused' else SC.ARCHS[0])
    gains, shading = _map(h, w, cell, seed=8)
    xa, xb = PR.full_range_frame(n, h, w, 12, seed=1), PR.full_range_frame(n, h, w, 12, seed=2)
    eager_a = net.serve(_shaded(xa, black, gains, cell), white - black, cfa='grbg').clone()
    eager_b = net.serve(_shaded(xb, black, gains, cell), white - black, cfa='grbg').clone()
    assert not torch.equal(eager_a, eager_b)
    slot, buf = torch.from_numpy(xa).cuda(), torch.zeros((n, h, w, 3), device='cuda', dtype=torch.uint8)
    sensor = dict(black_level=black, cfa='grbg', lens_shading=shading)
    net.serve(slot, white, out=buf, **sensor)               # fills the caches
    assert net.last_serve_route == route and torch.equal(buf, eager_a)
    buf.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.serve(slot, white, out=buf, **sensor)
    slot.copy_(torch.from_numpy(xb))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager_b)


# ---------------------------------------------------------------- 6. refusals through the C ABI
def test_refusals_through_the_c_abi_leave_the_output_alone():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    lib = L.load()
    n, h, w, k = 2, 4, 8, 2
    gh, gw = LS.map_shape(h, w, k)
    raw = torch.from_numpy(PR.full_range_frame(n, h, w, 12, seed=5)).cuda()
    gains = _place_map(LS.random_map(h, w, k, 1))
    u16 = torch.full((n * h * w + 8,), 0x5A5A, dtype=torch.uint16).cuda()
    out = torch.full((n * (h + h // 2) * w * 3 + 16,), 0x5A, device='cuda', dtype=torch.uint8)
    gam = torch.full((n, 1), 0.5).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    good = F.NV12_MATRIX['bt601_full']
    mat = lambda coef: (C.c_int * 12)(*coef) if coef is not None else None
    one, blk = (C.c_int * 1)(F.OP_GAMMA), L.ptr_array([gam.data_ptr()])

    def shade(raw_p=p(raw), out_p=p(u16), gains_p=p(gains), bits=16, k=k, GH=gh, GW=gw, H=h, coef=None):
        return lib.risp_raw_shade(raw_p, bits, 2 * w, out_p, gains_p, k, GH, GW, 0, n, H, w, F._stream())

    def classical(raw_p=p(raw), out_p=p(out), gains_p=p(gains), bits=16, k=k, GH=gh, GW=gw, H=h, coef=None):
        return lib.risp_serve_classical_shaded(raw_p, 4095.0, 1, 1, one, blk, out_p, 0, mat(coef), gains_p, k, GH, GW, n, H, w, 0, 0,
                                               F._stream())

    overflow = [256, 256, 256, 0] + list(good[4:])
    for name, call in (('risp_raw_shade', shade), ('risp_serve_classical_shaded', classical)):
        refused = {'null input': (dict(raw_p=None), b'null'), 'null out': (dict(out_p=None), b'null'),
                   'null gains': (dict(gains_p=None), b'null'), 'k 1': (dict(k=1), b'cell_log2 1'), 'k 9': (dict(k=9), b'cell_log2 9'),
                   'GH one too small': (dict(GH=gh - 1), ('a %d x %d map' % (gh - 1, gw)).encode())}
        if call is shade:
            refused['bits 14'] = (dict(bits=14), b'bits 14')
            refused['out 2-byte aligned'] = (dict(out_p=C.c_void_p(u16.data_ptr() + 2)), b'aligned')
        else:
            refused['odd H'] = (dict(H=5, GH=LS.map_shape(5, w, k)[0]), b'H=5')
            refused['out 1-byte aligned'] = (dict(out_p=C.c_void_p(out.data_ptr() + 1)), b'aligned')
            refused['a matrix row overflows'] = (dict(coef=overflow), b'cy')
        for what, (kw, word) in refused.items():
            assert call(**kw) != 0, '%s: %s was accepted' % (name, what)
            err = lib.risp_last_error()
            assert name.encode() in err and word in err, (name, what, err)
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item() and (u16.cpu() == 0x5A5A).all().item(), 'a refused call wrote to its output'
    # the same arguments without the fault are accepted and write the image alone
    assert shade() == 0
    torch.cuda.synchronize()
    assert (u16[n * h * w:].cpu() == 0x5A5A).all().item() and not (u16[:n * h * w].cpu() == 0x5A5A).all().item()
    for coef, size in ((None, n * h * w * 3), (good, n * (h + h // 2) * w)):
        out.fill_(0x5A)
        assert classical(coef=coef) == 0
        torch.cuda.synchronize()
        assert not (out[:size] == 0x5A).all().item() and (out[size:] == 0x5A).all().item()
