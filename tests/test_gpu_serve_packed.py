"""GPU: MIPI-packed RAW10 / RAW12 into the serving path - the unpack launch (risp_raw_unpack, both forms), the fused packed loads
of the one-launch kernels (risp_serve_packed, risp_serve_classical_packed) and ``serve(raw_format=...)`` on every route.

Unpacking is an integer function of the bytes and everything behind the sample is unchanged, so every comparison is
``torch.equal``: the unpack launch against tests/raw_packed_reference.py (numpy), every serving call against the same call on
the frames that reference unpacks.  Nothing here has a tolerance.

Shapes.  A thread owns a 2 x 4 patch - one RAW10 group or two RAW12 groups per row - and a workgroup a 64 x 32 pixel tile:
(4,4) is one group per row, left and right border pairs fall inside the thread's own group; (4,8) and (6,12) have border and
interior patches; (34,68) crosses the tile both ways; (2,4) is the smallest frame risp_serve_packed takes (no bilateral).
Layouts: N 1 and 3 (the image offset n * H * stride); the stride minimal, minimal + 3 (odd: rows unaligned) and rounded up to
64; the base aligned and one byte into a larger allocation whose other bytes are 0xFF, so that a read outside the payload
cannot hide as zeros - with the padding of a row random.  Frames: full range (white 2^bits - 1) and samples 0 .. 15 with white
15, which tests/test_raw_packed_reference_cpu.py shows to tell a mishandled low-bits byte apart in the served bytes."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import raw_packed_reference as PR
from raw_placement import _place

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4), (4, 8), (6, 12), (34, 68)]
BITS = {'raw10': 10, 'raw12': 12}
PHASES = ['rggb', 'grbg', 'gbrg', 'bggr']


def _strides(w, bits):
    used = w * bits // 8
    return [used, used + 3, (used + 63) // 64 * 64]


def _layouts(w, bits):
    """(n, stride, offset): every stride with every offset, N alternating - and both N for the unaligned minimal stride"""
    out = [(n, s, o) for k, (s, o) in enumerate(itertools.product(_strides(w, bits), (0, 1))) for n in ((1, 3)[(k // 2 + k) % 2],)]
    return out + [(1, _strides(w, bits)[0], 1)]


def _frames(kind, n, h, w, bits, seed):
    """(frames, white level)"""
    if kind == 'low':
        return PR.low_bit_frame(n, h, w, seed), 15
    return PR.full_range_frame(n, h, w, bits, seed), (1 << bits) - 1


def _case(kind, n, h, w, bits, stride, offset, seed):
    """(packed device view, the uint16 device frames the reference unpacks from its bytes, white level)"""
    x, white = _frames(kind, n, h, w, bits, seed)
    data = PR.pack(x, bits, stride, None)
    ref = PR.unpack(data, bits, w)
    assert np.array_equal(ref, x)
    return _place(data, offset), torch.from_numpy(ref).cuda(), white


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


# ---------------------------------------------------------------- 1. the unpack launch
@pytest.mark.parametrize('h,w', SHAPES + [(1, 4), (3, 20), (2, 64)], ids=lambda v: str(v))
@pytest.mark.parametrize('fmt', list(BITS))
def test_raw_unpack_equals_the_reference_in_both_forms(fmt, h, w):
    """(3,20) and (34,68) end a row with a chunk shorter than the 16 pixels of a thread, (2,64) has full chunks only; an
    aligned base with a stride that is a multiple of 4 takes the dword form, everything else the byte form"""
    import reconfigisp_amd.functional as F
    bits = BITS[fmt]
    for n, stride, offset in _layouts(w, bits):
        for kind in ('full', 'low'):
            packed, want, _ = _case(kind, n, h, w, bits, stride, offset, seed=h + w + stride)
            got, calls = _counted(lambda: F.raw_unpack(packed, bits, w))
            assert calls == {'risp_raw_unpack': 1}
            assert got.dtype == torch.uint16 and tuple(got.shape) == (n, h, w)
            assert torch.equal(got.cpu(), want.cpu()), '%s %dx%dx%d stride %d offset %d %s' % (fmt, n, h, w, stride, offset, kind)
    # the default width is all a minimal row holds; a single (H,stride) frame; out= is honoured and nothing beside it written
    packed, want, _ = _case('full', 2, h, w, bits, w * bits // 8, 0, seed=5)
    assert torch.equal(F.raw_unpack(packed, bits).cpu(), want.cpu())
    assert torch.equal(F.raw_unpack(packed[1], bits, w).cpu(), want[1].cpu())
    big = torch.full((2 * h * w + 8,), 0xA5A5, dtype=torch.uint16).cuda()
    out = big[4:4 + 2 * h * w].view(2, h, w)
    assert F.raw_unpack(packed, bits, w, out=out) is out
    assert torch.equal(out.cpu(), want.cpu()) and (big[:4].cpu() == 0xA5A5).all() and (big[4 + 2 * h * w:].cpu() == 0xA5A5).all()
    with pytest.raises(ValueError):
        F.raw_unpack(packed, bits, w, out=big[1:1 + 2 * h * w].view(2, h, w))       # 2-byte aligned only


# ---------------------------------------------------------------- 2. - 4. the fused loads, entry point against entry point
def _sensor_cases(bits):
    """(frame kind, black level): the full-range frame with both black levels, the low-bit frame (white 15) without one"""
    return [('full', 0), ('full', 64), ('low', 0)]


@pytest.mark.parametrize('h,w', SHAPES + [(2, 4)], ids=lambda v: str(v))
@pytest.mark.parametrize('fmt', list(BITS))
def test_serve_packed_equals_serve_u8_on_the_unpacked_frames(fmt, h, w):
    import reconfigisp_amd.functional as F
    import test_gpu_serve_cfa as CF
    bits = BITS[fmt]
    layouts = _layouts(w, bits)
    k = 0
    for kind, black in _sensor_cases(bits):
        for phase in PHASES:
            for form in range(3):                           # no bilateral, max_window 3 with mixed windows, max_window 1
                if form and h == 2:
                    continue
                for tail in CF._tails():                    # without and with WbQuadratic
                    n, stride, offset = layouts[k % len(layouts)]
                    k += 1
                    packed, dev, white = _case(kind, n, h, w, bits, stride, offset, seed=k)
                    pars = CF._chain_params(n, 100 + k)
                    params = [pars[op] for op in tail]
                    bil = CF._stage_forms(n)[form]
                    reverse = bool(k & 1)
                    want = F.serve_u8(dev, float(white - black), tail, params, bil, reverse, black_level=black, cfa=phase)
                    got, calls = _counted(lambda: F.serve_packed(packed, bits, w, float(white - black), tail, params, bil,
                                                                 reverse, black_level=black, cfa=phase))
                    assert calls == {'risp_serve_packed': 1}
                    assert torch.equal(got, want), '%s %dx%dx%d stride %d offset %d %s black %d %s form %d: %d bytes differ' % (
                        fmt, n, h, w, stride, offset, kind, black, phase, form, (got != want).sum().item())
    assert k >= 2 * len(layouts), 'every layout was served'
    assert h * w < 64 or len(torch.unique(got)) > 4, 'a flat image would prove nothing'


@pytest.mark.parametrize('h,w', SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize('fmt', list(BITS))
def test_serve_classical_packed_equals_serve_classical_u8_on_the_unpacked_frames(fmt, h, w):
    import reconfigisp_amd.functional as F
    import test_gpu_serve_classical as SC
    bits = BITS[fmt]
    layouts = _layouts(w, bits)
    WB, GA, FI, WQ = F.OP_WB_MANUAL, F.OP_GAMMA, F.OP_TONE_FILMIC, F.OP_WB_QUADRATIC
    k = 0
    for kind, black in _sensor_cases(bits):
        for phase in PHASES:
            for demosaic in SC.KINDS:
                for ops in ([WB, FI, GA], [WQ, FI]):
                    n, stride, offset = layouts[k % len(layouts)]
                    k += 1
                    packed, dev, white = _case(kind, n, h, w, bits, stride, offset, seed=k)
                    pars = SC._params(n, 200 + k, k % 3)
                    params = [pars[op] for op in ops]
                    reverse = bool(k & 1)
                    want = F.serve_classical_u8(dev, float(white - black), demosaic, ops, params, reverse, black_level=black, cfa=phase)
                    got, calls = _counted(lambda: F.serve_classical_packed(packed, bits, w, float(white - black), demosaic, ops,
                                                                           params, reverse, black_level=black, cfa=phase))
                    assert calls == {'risp_serve_classical_packed': 1}
                    assert torch.equal(got, want), '%s %dx%dx%d stride %d offset %d %s black %d %s %s: %d bytes differ' % (
                        fmt, n, h, w, stride, offset, kind, black, phase, demosaic, (got != want).sum().item())
    assert k >= 2 * len(layouts)


@pytest.mark.parametrize('h,w', [(4, 4), (6, 12), (34, 68)], ids=lambda v: str(v))
@pytest.mark.parametrize('fmt', list(BITS))
def test_both_entry_points_store_nv12(fmt, h, w):
    import reconfigisp_amd.functional as F
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    bits = BITS[fmt]
    layouts = _layouts(w, bits)
    matrices = list(F.NV12_MATRIX)
    for k, (phase, black) in enumerate(itertools.product(PHASES, (0, 64))):
        n, stride, offset = layouts[k % len(layouts)]
        packed, dev, white = _case('full', n, h, w, bits, stride, offset, seed=300 + k)
        matrix, div = matrices[k % 4], float(white - black)
        pars = SC._params(n, 300 + k, k % 3)
        for form in (0, 1):
            tail = CF._tails()[form]
            params = [pars[op] for op in tail]
            bil = CF._stage_forms(n)[1 if form else 0]
            want = F.serve_nv12(dev, div, tail, params, bil, matrix, black_level=black, cfa=phase)
            got = F.serve_packed(packed, bits, w, div, tail, params, bil, matrix=matrix, black_level=black, cfa=phase)
            assert tuple(got.shape) == (n, h + h // 2, w) and torch.equal(got, want), (fmt, h, w, phase, black, form)
        for demosaic in SC.KINDS:
            ops = [F.OP_WB_MANUAL, F.OP_TONE_FILMIC, F.OP_GAMMA]
            params = [pars[op] for op in ops]
            want = F.serve_classical_nv12(dev, div, demosaic, ops, params, matrix, black_level=black, cfa=phase)
            got = F.serve_classical_packed(packed, bits, w, div, demosaic, ops, params, matrix=matrix, black_level=black, cfa=phase)
            assert tuple(got.shape) == (n, h + h // 2, w) and torch.equal(got, want), (fmt, h, w, phase, black, demosaic)
    with pytest.raises(ValueError, match='reverse_channels'):
        F.serve_packed(packed, bits, w, div, [], [], reverse_channels=True, matrix='bt601_full')


# ---------------------------------------------------------------- 5. serve(raw_format=...) on every route
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
@pytest.mark.parametrize('fmt', list(BITS))
def test_serve_takes_packed_frames_on_every_route(fmt, what):
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    bits = BITS[fmt]
    n, h, w = 2, 34, 68
    net, kw, route = _route_case(what)
    stride = _strides(w, bits)[1]
    packed, dev, white = _case('full', n, h, w, bits, stride, 1, seed=400 + bits)
    sensor = dict(black_level=64, cfa='grbg')
    want = net.serve(dev, float(white), **sensor, **kw).clone()
    assert net.last_serve_route == route and net.last_serve_load is None
    _, plain_calls = _counted(lambda: net.serve(dev, float(white), **sensor, **kw))
    got, calls = _counted(lambda: net.serve(packed, float(white), raw_format=fmt, raw_width=w, **sensor, **kw))
    load = PF.serve_load(route, fmt)
    assert net.last_serve_route == route and net.last_serve_load == load
    assert load == ('pass' if what not in ('fused', 'classical') else load)
    if load == 'pass':
        assert calls == dict(plain_calls, risp_raw_unpack=1), (calls, plain_calls)
    else:
        assert calls == {'risp_serve_packed' if route == 'fused' else 'risp_serve_classical_packed': 1}, calls
    assert torch.equal(got, want), '%s %s: %d bytes differ' % (fmt, what, (got != want).sum().item())
    assert len(torch.unique(got)) > 8
    # NV12 out of packed in, on the same route
    want12 = net.serve(dev, float(white), out_format='nv12', yuv_matrix='bt709_full', **sensor, **kw).clone()
    got12 = net.serve(packed, float(white), out_format='nv12', yuv_matrix='bt709_full', raw_format=fmt, raw_width=w, **sensor, **kw)
    assert net.last_serve_route == route and net.last_serve_load == load and torch.equal(got12, want12)
    # 7. out= given: the same bytes, and a warm call allocates nothing
    buf = torch.empty_like(want)
    net.serve(packed, float(white), out=buf, raw_format=fmt, raw_width=w, **sensor, **kw)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert net.serve(packed, float(white), out=buf, raw_format=fmt, raw_width=w, **sensor, **kw) is buf
    if what != 'composed':                                 # (the composed route allocates its fp32 planes, packed or not)
        assert torch.cuda.memory_allocated() == before
    assert torch.equal(buf, want)
    # 9. the explicit default is the call without the keyword
    assert torch.equal(net.serve(dev, float(white), raw_format='u16', **sensor, **kw), want) and net.last_serve_load is None


def test_the_default_width_and_the_model_wrapper():
    import test_gpu_serve_frame as SF
    model = SF._model('classical')
    n, h, w = 1, 6, 12
    packed, dev, white = _case('full', n, h, w, 12, 18, 0, seed=9)
    want = model.serve(dev, float(white))
    assert torch.equal(model.serve(packed, float(white), raw_format='raw12'), want) and model.netG.last_serve_load is not None


# ---------------------------------------------------------------- 6. full frames in tiles
@pytest.mark.parametrize('fmt', list(BITS))
def test_serve_frame_unpacks_once_in_front_of_the_tiles(fmt):
    import test_gpu_serve_frame as SF
    bits = BITS[fmt]
    model = SF._model('classical')
    net = model.netG
    h, w = 64, 96
    packed, dev, white = _case('full', 1, h, w, bits, _strides(w, bits)[1], 1, seed=6)
    kw = dict(tile_batch=4, black_level=64, cfa='gbrg')
    want = net.serve_frame(dev, float(white), 48, 32, **kw).clone()
    assert net.last_serve_route == 'tiled' and net.last_serve_load is None
    got, calls = _counted(lambda: net.serve_frame(packed, float(white), 48, 32, raw_format=fmt, raw_width=w, **kw))
    assert net.last_serve_route == 'tiled' and net.last_serve_load == 'pass' and calls.get('risp_raw_unpack') == 1, calls
    assert tuple(got.shape) == (1, h, w, 3) and torch.equal(got, want)
    one = model.serve_frame(packed[0], float(white), 48, 32, raw_format=fmt, raw_width=w, **kw)        # (H,stride)
    assert tuple(one.shape) == (h, w, 3) and torch.equal(one, want[0])
    assert torch.equal(net.serve_frame(dev, float(white), 48, 32, raw_format='u16', **kw), want)


# ---------------------------------------------------------------- 8. a captured graph
@pytest.mark.parametrize('route', ['fused', 'classical'])
@pytest.mark.parametrize('fmt', list(BITS))
def test_a_packed_fused_call_replays_from_a_graph(fmt, route):
    """both one-launch routes, so that a launch with the packed load is captured whatever ``serve_load`` answers for one of them"""
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    bits = BITS[fmt]
    n, h, w = 3, 34, 68
    net = CF._pipeline(CF.HEADLINE if route == 'fused' else SC.ARCHS[0])
    stride = _strides(w, bits)[0]
    a, dev_a, white = _case('full', n, h, w, bits, stride, 0, seed=1)
    b, dev_b, _ = _case('full', n, h, w, bits, stride, 0, seed=2)
    eager_a, eager_b = net.serve(dev_a, float(white)).clone(), net.serve(dev_b, float(white)).clone()
    assert not torch.equal(eager_a, eager_b)
    slot, buf = a.clone(), torch.zeros((n, h, w, 3), device='cuda', dtype=torch.uint8)
    net.serve(slot, float(white), out=buf, raw_format=fmt, raw_width=w)       # fills the caches
    assert net.last_serve_route == route and torch.equal(buf, eager_a)
    buf.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.serve(slot, float(white), out=buf, raw_format=fmt, raw_width=w)
    slot.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager_b)


# ---------------------------------------------------------------- 10. refusals through the C ABI
def test_refusals_through_the_c_abi_leave_the_output_alone():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    lib = L.load()
    n, h, w, bits = 2, 4, 8, 10
    stride = w * bits // 8
    packed, _, _ = _case('full', n, h, w, bits, stride, 0, seed=5)
    u16 = torch.full((n * h * w + 8,), 0x5A5A, dtype=torch.uint16).cuda()
    out = torch.full((n * (h + h // 2) * w * 3 + 16,), 0x5A, device='cuda', dtype=torch.uint8)
    gam = torch.full((n, 1), 0.5).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    good = F.NV12_MATRIX['bt601_full']
    mat = lambda coef: (C.c_int * 12)(*coef) if coef is not None else None
    one, blk = (C.c_int * 1)(F.OP_GAMMA), L.ptr_array([gam.data_ptr()])

    def unpack(raw_p=p(packed), out_p=p(u16), bits=bits, W=w, stride=stride, N=n, H=h, coef=None):
        return lib.risp_raw_unpack(raw_p, out_p, bits, N, H, W, stride, F._stream())

    def fused(raw_p=p(packed), out_p=p(out), bits=bits, W=w, stride=stride, N=n, H=h, coef=None):
        return lib.risp_serve_packed(raw_p, bits, stride, 1023.0, None, None, None, 0, 1, one, blk, out_p, 0, mat(coef), N, H, W, 0, 0,
                                     F._stream())

    def classical(raw_p=p(packed), out_p=p(out), bits=bits, W=w, stride=stride, N=n, H=h, coef=None):
        return lib.risp_serve_classical_packed(raw_p, bits, stride, 1023.0, 1, 1, one, blk, out_p, 0, mat(coef), N, H, W, 0, 0,
                                               F._stream())

    overflow = [256, 256, 256, 0] + list(good[4:])
    for name, call in (('risp_raw_unpack', unpack), ('risp_serve_packed', fused), ('risp_serve_classical_packed', classical)):
        refused = {'bits 8': (dict(bits=8), b'8'), 'bits 14': (dict(bits=14), b'14'), 'W 6': (dict(W=6), b'6'),
                   'W 0': (dict(W=0), b'0'), 'stride one too small': (dict(stride=stride - 1), str(stride - 1).encode()),
                   'raw12 in rows of raw10': (dict(bits=12), b'12'), 'null input': (dict(raw_p=None), b'null'),
                   'null out': (dict(out_p=None), b'null'), 'N 0': (dict(N=0), b'N=0')}
        if call is unpack:
            refused['out 2-byte aligned'] = (dict(out_p=C.c_void_p(u16.data_ptr() + 2)), b'aligned')
        else:
            refused['odd H'] = (dict(H=3), b'H=3')
            refused['a matrix row overflows'] = (dict(coef=overflow), b'cy')
            refused['coefficient 257'] = (dict(coef=[257, 0, 0, 0] + list(good[4:])), b'257')
        for what, (kw, word) in refused.items():
            assert call(**kw) != 0, '%s: %s was accepted' % (name, what)
            err = lib.risp_last_error()
            assert name.encode() in err and word in err, (name, what, err)
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item() and (u16.cpu() == 0x5A5A).all().item(), 'a refused call wrote to its output'
    # the same arguments without the fault are accepted and write the image alone
    assert unpack() == 0
    torch.cuda.synchronize()
    assert (u16[n * h * w:].cpu() == 0x5A5A).all().item() and not (u16[:n * h * w].cpu() == 0x5A5A).all().item()
    for call, size in ((fused, n * h * w * 3), (classical, n * h * w * 3)):
        for coef, size in ((None, n * h * w * 3), (good, n * (h + h // 2) * w)):
            out.fill_(0x5A)
            assert call(coef=coef) == 0
            torch.cuda.synchronize()
            assert not (out[:size] == 0x5A).all().item() and (out[size:] == 0x5A).all().item()
