"""``serve(warp=)`` / ``serve_frame(warp=)``: byte for byte
``nv12?(bgr8_resize?(bgr8_warp(serve(.. without warp, the resize keywords and out_format ..), warp), ..))`` on every kind of
route, with the launches of the call without the keyword and exactly one ``risp_bgr8_warp`` more; the numpy references
(tests/warp_reference.py, resize_reference.py, nv12_reference.py) say what those bytes are."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv12_reference as NR  # noqa: E402
import resize_reference as RR  # noqa: E402
import warp_reference as WR  # noqa: E402

pytestmark = pytest.mark.gpu

WHITE = 1023
H, W = 32, 48
SIZE, CELL = (28, 40), 8            # the warped image: even, so that NV12 can follow; not the sensor's size
OUT = (18, 26)                      # out_size behind the warp


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


def _warp(kernel, h=H, w=W, size=SIZE, kind='rot_radial'):
    mesh = WR.make_mesh(kind, (h, w), size, CELL.bit_length() - 1, seed=7)
    return (torch.from_numpy(mesh).cuda(), CELL, size, kernel), mesh


def _ref(bgr, mesh, size, kernel, out_size=None, window=None, resample='triangle', matrix=None):
    """the contract's right-hand side from the references, on a packed device image, as a device tensor"""
    out = WR.warp(bgr.cpu().numpy(), mesh, CELL.bit_length() - 1, size, kernel)
    if out_size is not None or window is not None:
        out = RR.resize(out, out_size, window, resample)
    if matrix is not None:
        out = NR.nv12(out, NR.TABLE[matrix], 'bgr')
    return torch.from_numpy(out).cuda()


def _route_case(what):
    """(net, frames, keywords of serve(), the route they take), built as tests/test_gpu_serve_resize.py builds them"""
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    import test_gpu_serve_denoise as D
    n = 2
    if what == 'fused':
        return CF._pipeline('Demosaic_01_sRGB_07_11_01_14'), CF._u16(CF._raw(n, H, W, WHITE, seed=40)), {}, 'fused'
    if what == 'classical':
        return CF._pipeline(SC.ARCHS[1]), CF._u16(CF._raw(n, H, W, WHITE, seed=46)), {}, 'classical'
    if what == 'denoise':
        return CF._pipeline('Bayer_02_Demosaic_02_sRGB_07_01'), D._frames(n, H, W, seed=42), dict(fast_denoise=True), 'denoise'
    return CF._pipeline('Demosaic_02_sRGB_13', 'IspUniversal'), D._frames(n, H, W, seed=45), {}, 'composed'


@pytest.mark.parametrize('what', ['fused', 'classical', 'denoise', 'composed'])
def test_serve_warps_behind_every_kind_of_route(what):
    import reconfigisp_amd.functional as F
    net, dev, kw, route = _route_case(what)
    n = dev.shape[0]
    sensor = dict(black_level=64, cfa='grbg')
    bgr = net.serve(dev, float(WHITE), **sensor, **kw).clone()
    assert net.last_serve_route == route and net.last_serve_warp is None
    _, plain_calls = _counted(lambda: net.serve(dev, float(WHITE), **sensor, **kw))
    _, none_calls = _counted(lambda: net.serve(dev, float(WHITE), warp=None, **sensor, **kw))
    assert none_calls == plain_calls
    for kernel in WR.KERNELS:
        warp, mesh = _warp(kernel)
        got, calls = _counted(lambda: net.serve(dev, float(WHITE), warp=warp, **sensor, **kw))
        assert net.last_serve_route == route and net.last_serve_warp == 'pass' and net.last_serve_store is None
        assert net.last_serve_resize is None
        assert calls == dict(plain_calls, risp_bgr8_warp=1), (calls, plain_calls)
        assert tuple(got.shape) == (n,) + SIZE + (3,)
        assert torch.equal(got, F.bgr8_warp(bgr, warp)) and torch.equal(got, _ref(bgr, mesh, SIZE, kernel))
    assert len(torch.unique(got)) > 8, 'a flat image would prove nothing'
    # NV12 behind the warp: the routes that own a fused NV12 store serve BGR, the conversion launch follows the warp
    warp, mesh = _warp('bicubic')
    got, calls = _counted(lambda: net.serve(dev, float(WHITE), warp=warp, out_format='nv12', yuv_matrix='bt709_full', **sensor, **kw))
    assert net.last_serve_route == route and net.last_serve_warp == 'pass' and net.last_serve_store == 'pass'
    assert calls == dict(plain_calls, risp_bgr8_warp=1, risp_bgr8_to_nv12=1), (calls, plain_calls)
    assert tuple(got.shape) == (n, SIZE[0] * 3 // 2, SIZE[1])
    assert torch.equal(got, _ref(bgr, mesh, SIZE, 'bicubic', matrix='bt709_full'))
    assert torch.equal(got, F.bgr8_to_nv12(F.bgr8_warp(bgr, warp), 'bt709_full'))
    # out_size behind the warp, BGR and NV12: the window lies in the warped image
    win = (2, 3, 24, 34)
    got, calls = _counted(lambda: net.serve(dev, float(WHITE), warp=warp, out_size=OUT, out_window=win, resample='bicubic', **sensor, **kw))
    assert net.last_serve_warp == 'pass' and net.last_serve_resize == 'pass' and net.last_serve_store is None
    assert calls == dict(plain_calls, risp_bgr8_warp=1, risp_bgr8_resize=1), (calls, plain_calls)
    assert tuple(got.shape) == (n,) + OUT + (3,)
    assert torch.equal(got, _ref(bgr, mesh, SIZE, 'bicubic', OUT, win, 'bicubic'))
    assert torch.equal(got, F.bgr8_resize(F.bgr8_warp(bgr, warp), OUT, win, 'bicubic'))
    got = net.serve(dev, float(WHITE), warp=warp, out_size=OUT, out_format='nv12', **sensor, **kw)
    assert net.last_serve_warp == 'pass' and net.last_serve_resize == 'pass' and net.last_serve_store in ('resize', 'pass')
    assert torch.equal(got, _ref(bgr, mesh, SIZE, 'bicubic', OUT, None, 'triangle', 'bt601_full'))
    # a warp whose output has the sensor's size, then the call without the keyword: neither sees the other's image
    same, smesh = _warp('bilinear', size=(H, W))
    assert torch.equal(net.serve(dev, float(WHITE), warp=same, out_size=(H, W), **sensor, **kw), _ref(bgr, smesh, (H, W), 'bilinear'))
    assert torch.equal(net.serve(dev, float(WHITE), warp=same, out_format='nv12', **sensor, **kw),
                       _ref(bgr, smesh, (H, W), 'bilinear', matrix='bt601_full'))
    assert torch.equal(net.serve(dev, float(WHITE), **sensor, **kw), bgr) and net.last_serve_warp is None


def test_serve_with_another_phase_reversed_channels_packed_frames_shading_defects_and_statistics():
    import raw_packed_reference as PR
    import reconfigisp_amd.functional as F
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    import test_gpu_serve_defect as GD
    net = CF._pipeline(SC.ARCHS[0])
    x = PR.full_range_frame(2, H, W, 10, seed=71)
    dev = torch.from_numpy(x).cuda()
    packed = GD._place_packed(x, 10, W * 10 // 8 + 3, 1)
    _, shading = GD._gains(H, W, 8, seed=72)
    warp, mesh = _warp('bicubic')
    cases = [dict(black_level=64, cfa='gbrg'), dict(reverse_channels=True), dict(black_level=16, cfa='bggr', reverse_channels=True),
             dict(lens_shading=shading, defect_correction=(16, 32, None), black_level=64)]
    for kw in cases:
        bgr = net.serve(dev, float(WHITE), **kw).clone()
        got = net.serve(dev, float(WHITE), warp=warp, **kw)
        assert torch.equal(got, F.bgr8_warp(bgr, warp)) and torch.equal(got, _ref(bgr, mesh, SIZE, 'bicubic')), kw
        assert net.last_serve_warp == 'pass'
    # RAW10 in: the fused packed load of the classical route stays, the warp launch follows
    bgr = net.serve(dev, float(WHITE), black_level=64).clone()
    got, calls = _counted(lambda: net.serve(packed, float(WHITE), black_level=64, raw_format='raw10', raw_width=W, warp=warp))
    _, plain = _counted(lambda: net.serve(packed, float(WHITE), black_level=64, raw_format='raw10', raw_width=W))
    assert calls == dict(plain, risp_bgr8_warp=1) and net.last_serve_load == 'fused'
    assert torch.equal(got, _ref(bgr, mesh, SIZE, 'bicubic'))
    # statistics describe the sensor frame: the zones and histograms of the call without warp
    a, b = (F.raw_statistics(2, H, W, zone=(8, 8), bins=64, hist_shift=4, lo=64, hi=900) for _ in range(2))
    plain_img, plain_calls = _counted(lambda: net.serve(dev, float(WHITE), black_level=64, statistics=a))
    got, calls = _counted(lambda: net.serve(dev, float(WHITE), black_level=64, statistics=b, warp=warp))
    assert calls == dict(plain_calls, risp_bgr8_warp=1) and net.last_serve_stats == 'pass' and net.last_serve_warp == 'pass'
    assert torch.equal(a.zones, b.zones) and torch.equal(a.hist, b.hist) and int(a.hist.sum()) == 2 * H * W
    assert torch.equal(got, _ref(plain_img, mesh, SIZE, 'bicubic'))
    assert torch.equal(net.serve(dev, float(WHITE), black_level=64), bgr) and net.last_serve_warp is None


def _refused(fn, what):
    with pytest.raises(ValueError, match=what):
        fn()


def test_serve_refuses_before_anything_is_launched():
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    net = CF._pipeline(SC.ARCHS[0])
    dev = CF._u16(CF._raw(2, H, W, WHITE, seed=5))
    warp, _ = _warp('bilinear')
    mesh = warp[0]
    good = torch.empty((2,) + SIZE + (3,), dtype=torch.uint8, device='cuda')
    for kw, what in ((dict(warp=(mesh, 12, SIZE, 'bilinear')), 'cell 12'), (dict(warp=(mesh, CELL, SIZE, 'box')), "kernel 'box'"),
                     (dict(warp=(mesh, CELL, (28, 41), 'bilinear')), r'\(5,7,2\)'),
                     (dict(warp=(mesh.cpu(), CELL, SIZE, 'bilinear')), 'lives on'),
                     (dict(warp=(mesh.float(), CELL, SIZE, 'bilinear')), 'int32'),
                     (dict(warp=(mesh[:4], CELL, (27, 40), 'bilinear'), out_format='nv12'), 'even'),
                     (dict(warp=warp, out=good[:, :, :39]), 'out must be'), (dict(warp=warp, out=good[:1]), 'out must be'),
                     (dict(warp=warp, out_format='nv12', reverse_channels=True), 'reverse_channels'),
                     (dict(warp=warp, out_format='nv12', yuv_matrix='bt2020'), 'matrix'),
                     (dict(warp=warp, out_window=(0, 0, 29, 40)), 'out_window'),
                     (dict(warp=warp, out_size=OUT, out=good), 'out must be')):
        _, calls = _counted(lambda: _refused(lambda: net.serve(dev, float(WHITE), **kw), what))
        assert calls == {}, (kw, calls)


def test_serve_frame_single_and_batched():
    import reconfigisp_amd.functional as F
    import test_gpu_serve_frame as SF
    model = SF._model('classical')
    net = model.netG
    g = torch.Generator().manual_seed(9)
    h, w, size = 48, 64, (40, 52)
    dev = torch.randint(0, WHITE + 1, (2, h, w), generator=g, dtype=torch.int32).to(torch.uint16).cuda()
    kw = dict(tile_batch=5, black_level=64, cfa='gbrg')
    warp, mesh = _warp('bicubic', h, w, size)
    bgr = net.serve_frame(dev, float(WHITE), 32, 16, **kw).clone()
    assert net.last_serve_route == 'tiled' and net.last_serve_warp is None
    _, plain = _counted(lambda: net.serve_frame(dev, float(WHITE), 32, 16, **kw))
    got, calls = _counted(lambda: net.serve_frame(dev, float(WHITE), 32, 16, warp=warp, **kw))
    assert net.last_serve_route == 'tiled' and net.last_serve_warp == 'pass' and net.last_serve_store is None
    assert calls == dict(plain, risp_bgr8_warp=1), (calls, plain)
    assert tuple(got.shape) == (2,) + size + (3,) and torch.equal(got, _ref(bgr, mesh, size, 'bicubic'))
    # a single (H,W) frame gives (WH,WW,3); the IspModel passes the keyword through; reversed channels; out=
    one = model.serve_frame(dev[1], float(WHITE), 32, 16, warp=warp, **kw)
    assert tuple(one.shape) == size + (3,) and torch.equal(one, got[1])
    rev = net.serve_frame(dev[1], float(WHITE), 32, 16, reverse_channels=True, warp=warp, **kw)
    assert torch.equal(rev, one.flip(-1))
    buf = torch.empty_like(got)
    assert net.serve_frame(dev, float(WHITE), 32, 16, out=buf, warp=warp, **kw) is buf and torch.equal(buf, got)
    nv, calls = _counted(lambda: net.serve_frame(dev, float(WHITE), 32, 16, out_format='nv12', yuv_matrix='bt601_video', warp=warp,
                                                 out_size=OUT, **kw))
    assert net.last_serve_warp == 'pass' and net.last_serve_resize == 'pass'
    assert calls['risp_bgr8_warp'] == 1 and calls['risp_bgr8_resize'] == 1
    assert torch.equal(nv, _ref(bgr, mesh, size, 'bicubic', OUT, None, 'triangle', 'bt601_video'))
    assert torch.equal(model.serve(dev, float(WHITE), black_level=64, warp=warp),
                       F.bgr8_warp(model.serve(dev, float(WHITE), black_level=64), warp))
    _, calls = _counted(lambda: _refused(lambda: net.serve_frame(dev, float(WHITE), 32, 16, warp=(warp[0], 16, size, 'bicubic'), **kw),
                                         r'\(4,5,2\)'))
    assert calls == {}
    assert torch.equal(net.serve_frame(dev, float(WHITE), 32, 16, **kw), bgr) and net.last_serve_warp is None


def test_a_warm_call_is_captured_in_a_graph_and_replayed_on_new_frames():
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    net = CF._pipeline(SC.ARCHS[0])
    xa, xb = (CF._u16(CF._raw(2, H, W, WHITE, seed=s)) for s in (11, 12))
    plain = dict(black_level=64, cfa='grbg')
    warp, mesh = _warp('bicubic')
    kw = dict(warp=warp, out_size=OUT, resample='bicubic', out_format='nv12', **plain)
    eager = [_ref(net.serve(x, float(WHITE), **plain), mesh, SIZE, 'bicubic', OUT, None, 'bicubic', 'bt601_full') for x in (xa, xb)]
    assert not torch.equal(eager[0], eager[1])
    before_plain = net.serve(xa, float(WHITE), **plain).clone()
    slot = xa.clone()
    buf = torch.zeros((2, OUT[0] * 3 // 2, OUT[1]), dtype=torch.uint8, device='cuda')
    net.serve(slot, float(WHITE), out=buf, **kw)            # fills the caches: the tables, the three images
    assert net.last_serve_warp == 'pass' and torch.equal(buf, eager[0])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    net.serve(slot, float(WHITE), out=buf, **kw)
    assert torch.cuda.memory_allocated() == before, 'a warm call allocated'
    buf.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.serve(slot, float(WHITE), out=buf, **kw)
    slot.copy_(xb)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager[1])
    assert torch.equal(net.serve(xa, float(WHITE), **plain), before_plain) and net.last_serve_warp is None
