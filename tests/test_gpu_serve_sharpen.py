"""``serve(sharpen=)`` / ``serve_frame(sharpen=)``: byte for byte
``nv12?(bgr8_sharpen(bgr8_resize?(bgr8_warp?(serve(.. without these keywords ..)))))`` on every kind of route, with the launches
of the call without the keyword and exactly one ``risp_bgr8_sharpen`` more; the numpy references (tests/sharpen_reference.py,
warp_reference.py, resize_reference.py, nv12_reference.py) say what those bytes are."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv12_reference as NR  # noqa: E402
import resize_reference as RR  # noqa: E402
import sharpen_reference as SR  # noqa: E402
import warp_reference as WR  # noqa: E402

pytestmark = pytest.mark.gpu

WHITE = 1023
H, W = 32, 48
SIZE, CELL = (28, 40), 8            # the warped image: even, so that NV12 can follow; not the sensor's size
OUT = (18, 26)                      # out_size
WIN = (2, 3, 24, 34)                # out_window: inside the warped image and the sensor's
SHARP = (640, 2, 48, 2)
SHARP1 = (1024, 0, 255, 1)


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


def _warp(kernel='bilinear', h=H, w=W, size=SIZE):
    mesh = WR.make_mesh('rot_radial', (h, w), size, CELL.bit_length() - 1, seed=7)
    return (torch.from_numpy(mesh).cuda(), CELL, size, kernel), mesh


def _ref(bgr, sharpen, channels='bgr', warp=None, out_size=None, window=None, resample='triangle', matrix=None):
    """the contract's right-hand side from the references, on a packed device image, as a device tensor"""
    out = bgr.cpu().numpy()
    if warp is not None:
        mesh, size, kernel = warp
        out = WR.warp(out, mesh, CELL.bit_length() - 1, size, kernel)
    if out_size is not None or window is not None:
        out = RR.resize(out, out_size, window, resample)
    out = SR.sharpen(out, sharpen, channels)
    if matrix is not None:
        out = NR.nv12(out, NR.TABLE[matrix], 'bgr')
    return torch.from_numpy(out).cuda()


def _route_case(what):
    import test_gpu_serve_warp as SW
    return SW._route_case(what)


@pytest.mark.parametrize('what', ['fused', 'classical', 'denoise', 'composed'])
def test_serve_sharpens_behind_every_kind_of_route(what):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    net, dev, kw, route = _route_case(what)
    n = dev.shape[0]
    sensor = dict(black_level=64, cfa='grbg')
    store = 'sharpen' if PF.sharpen_store('nv12') == 'fused' else 'pass'
    after = {} if store == 'sharpen' else dict(risp_bgr8_to_nv12=1)
    bgr = net.serve(dev, float(WHITE), **sensor, **kw).clone()
    assert net.last_serve_route == route and net.last_serve_sharpen is None
    _, plain_calls = _counted(lambda: net.serve(dev, float(WHITE), **sensor, **kw))
    none, none_calls = _counted(lambda: net.serve(dev, float(WHITE), sharpen=None, **sensor, **kw))
    assert none_calls == plain_calls and torch.equal(none, bgr) and net.last_serve_sharpen is None
    for sharpen in (SHARP, SHARP1):
        got, calls = _counted(lambda: net.serve(dev, float(WHITE), sharpen=sharpen, **sensor, **kw))
        assert net.last_serve_route == route and net.last_serve_sharpen == 'pass' and net.last_serve_store is None
        assert net.last_serve_resize is None and net.last_serve_warp is None
        assert calls == dict(plain_calls, risp_bgr8_sharpen=1), (calls, plain_calls)
        assert tuple(got.shape) == (n, H, W, 3)
        assert torch.equal(got, F.bgr8_sharpen(bgr, sharpen)) and torch.equal(got, _ref(bgr, sharpen))
        assert (got != bgr).float().mean() > 0.05, 'an image that passes unchanged would prove nothing'
    # NV12: the routes that own a fused NV12 store serve BGR
    got, calls = _counted(lambda: net.serve(dev, float(WHITE), sharpen=SHARP, out_format='nv12', yuv_matrix='bt709_full', **sensor, **kw))
    assert net.last_serve_route == route and net.last_serve_sharpen == 'pass' and net.last_serve_store == store
    assert calls == dict(plain_calls, risp_bgr8_sharpen=1, **after), (calls, plain_calls)
    assert tuple(got.shape) == (n, H * 3 // 2, W)
    assert torch.equal(got, _ref(bgr, SHARP, matrix='bt709_full'))
    assert torch.equal(got, F.bgr8_to_nv12(F.bgr8_sharpen(bgr, SHARP), 'bt709_full'))
    # behind the warp, behind the resize, behind both - BGR and NV12
    warp, mesh = _warp('bicubic')
    wref = (mesh, SIZE, 'bicubic')
    for extra, more, ref_kw, shape in (
            (dict(warp=warp), dict(risp_bgr8_warp=1), dict(warp=wref), SIZE),
            (dict(out_size=OUT, out_window=WIN, resample='bicubic'), dict(risp_bgr8_resize=1),
             dict(out_size=OUT, window=WIN, resample='bicubic'), OUT),
            (dict(warp=warp, out_size=OUT, out_window=WIN), dict(risp_bgr8_warp=1, risp_bgr8_resize=1),
             dict(warp=wref, out_size=OUT, window=WIN), OUT)):
        got, calls = _counted(lambda: net.serve(dev, float(WHITE), sharpen=SHARP, **extra, **sensor, **kw))
        assert net.last_serve_route == route and net.last_serve_sharpen == 'pass' and net.last_serve_store is None
        assert net.last_serve_warp == ('pass' if 'warp' in extra else None)
        assert net.last_serve_resize == ('pass' if 'out_size' in extra else None)
        assert calls == dict(plain_calls, risp_bgr8_sharpen=1, **more), (extra.keys(), calls, plain_calls)
        assert tuple(got.shape) == (n,) + shape + (3,) and torch.equal(got, _ref(bgr, SHARP, **ref_kw)), extra.keys()
        got, calls = _counted(lambda: net.serve(dev, float(WHITE), sharpen=SHARP, out_format='nv12', **extra, **sensor, **kw))
        assert net.last_serve_sharpen == 'pass' and net.last_serve_store == store
        assert calls == dict(plain_calls, risp_bgr8_sharpen=1, **more, **after), (extra.keys(), calls, plain_calls)
        assert tuple(got.shape) == (n, shape[0] * 3 // 2, shape[1])
        assert torch.equal(got, _ref(bgr, SHARP, matrix='bt601_full', **ref_kw)), extra.keys()
    # the calls without the keyword see none of its images, at coinciding shapes too
    same = _warp('bilinear', size=(H, W))
    assert torch.equal(net.serve(dev, float(WHITE), sharpen=SHARP, warp=same[0], **sensor, **kw),
                       _ref(bgr, SHARP, warp=(same[1], (H, W), 'bilinear')))
    assert torch.equal(net.serve(dev, float(WHITE), warp=same[0], **sensor, **kw), F.bgr8_warp(bgr, same[0]))
    assert torch.equal(net.serve(dev, float(WHITE), out_format='nv12', **sensor, **kw), F.bgr8_to_nv12(bgr))
    assert torch.equal(net.serve(dev, float(WHITE), **sensor, **kw), bgr) and net.last_serve_sharpen is None


def test_serve_with_reversed_channels_another_phase_packed_frames_shading_defects_and_statistics():
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
    cases = [dict(black_level=64, cfa='gbrg'), dict(reverse_channels=True), dict(black_level=16, cfa='bggr', reverse_channels=True),
             dict(lens_shading=shading, defect_correction=(16, 32, None), black_level=64)]
    for kw in cases:
        served = net.serve(dev, float(WHITE), **kw).clone()
        channels = 'rgb' if kw.get('reverse_channels') else 'bgr'
        got = net.serve(dev, float(WHITE), sharpen=SHARP, **kw)
        assert torch.equal(got, _ref(served, SHARP, channels)), kw
        assert torch.equal(got, F.bgr8_sharpen(served, SHARP, channels=channels)) and net.last_serve_sharpen == 'pass'
        if channels == 'rgb':       # the launch was told the order: the reversed image is the sharpened BGR image reversed
            assert torch.equal(got.flip(-1), _ref(served.flip(-1).contiguous(), SHARP, 'bgr'))
            assert not torch.equal(got, _ref(served, SHARP, 'bgr'))
    # RAW10 in: the fused packed load of the classical route stays, the sharpen launch follows
    bgr = net.serve(dev, float(WHITE), black_level=64).clone()
    got, calls = _counted(lambda: net.serve(packed, float(WHITE), black_level=64, raw_format='raw10', raw_width=W, sharpen=SHARP))
    _, plain = _counted(lambda: net.serve(packed, float(WHITE), black_level=64, raw_format='raw10', raw_width=W))
    assert calls == dict(plain, risp_bgr8_sharpen=1) and net.last_serve_load == 'fused'
    assert torch.equal(got, _ref(bgr, SHARP))
    # statistics describe the sensor frame: the numbers of the call without the keyword
    a, b = (F.raw_statistics(2, H, W, zone=(8, 8), bins=64, hist_shift=4, lo=64, hi=900) for _ in range(2))
    plain_img, plain_calls = _counted(lambda: net.serve(dev, float(WHITE), black_level=64, statistics=a))
    got, calls = _counted(lambda: net.serve(dev, float(WHITE), black_level=64, statistics=b, sharpen=SHARP))
    assert calls == dict(plain_calls, risp_bgr8_sharpen=1) and net.last_serve_stats == 'pass' and net.last_serve_sharpen == 'pass'
    assert torch.equal(a.zones, b.zones) and torch.equal(a.hist, b.hist) and int(a.hist.sum()) == 2 * H * W
    assert torch.equal(got, _ref(plain_img, SHARP))
    assert torch.equal(net.serve(dev, float(WHITE), black_level=64), bgr) and net.last_serve_sharpen is None


def test_serve_over_three_frames_of_a_temporal_filter():
    import reconfigisp_amd.functional as F
    import temporal_reference as TR
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    net = CF._pipeline(SC.ARCHS[0])
    seq = TR.sequence((2, H, W), seed=31, steps=3)
    a, b = F.temporal_state(2, H, W), F.temporal_state(2, H, W)
    net.serve(torch.from_numpy(seq[0]).cuda(), float(WHITE), black_level=64)       # (the stage parameters are made once)
    for frame in seq:
        dev = torch.from_numpy(frame).cuda()
        plain, plain_calls = _counted(lambda: net.serve(dev, float(WHITE), black_level=64, temporal_denoise=(a,) + TR.PARAMS[0]))
        plain = plain.clone()
        got, calls = _counted(lambda: net.serve(dev, float(WHITE), black_level=64, temporal_denoise=(b,) + TR.PARAMS[0], sharpen=SHARP))
        assert calls == dict(plain_calls, risp_bgr8_sharpen=1) and net.last_serve_temporal == 'pass'
        assert torch.equal(got, _ref(plain, SHARP)) and torch.equal(a.frames, b.frames)


def _refused(fn, what):
    with pytest.raises(ValueError, match=what):
        fn()


def test_serve_refuses_before_anything_is_launched():
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    net = CF._pipeline(SC.ARCHS[0])
    dev = CF._u16(CF._raw(2, H, W, WHITE, seed=5))
    good = torch.empty((2, H, W, 3), dtype=torch.uint8, device='cuda')
    for kw, what in ((dict(sharpen=(640, 2, 48)), 'amount, threshold, limit, radius'), (dict(sharpen=(4096, 2, 48, 2)), 'amount'),
                     (dict(sharpen=(640, 2, 48, 3)), 'radius'), (dict(sharpen=(640, 2.0, 48, 2)), 'threshold'),
                     (dict(sharpen=(640, 2, True, 2)), 'limit'),
                     (dict(sharpen=SHARP, out_size=(17, 26), out_format='nv12'), 'even'),
                     (dict(sharpen=SHARP, out=good[:, :, :47]), 'out must be'), (dict(sharpen=SHARP, out=good[:1]), 'out must be'),
                     (dict(sharpen=SHARP, out=good, out_format='nv12'), 'out must be'),
                     (dict(sharpen=SHARP, out=good, out_size=OUT), 'out must be'),
                     (dict(sharpen=SHARP, out_format='nv12', reverse_channels=True), 'reverse_channels'),
                     (dict(sharpen=SHARP, out_format='nv12', yuv_matrix='bt2020'), 'matrix'),
                     (dict(sharpen=SHARP, out_window=(0, 0, 33, 40)), 'out_window')):
        _, calls = _counted(lambda: _refused(lambda: net.serve(dev, float(WHITE), **kw), what))
        assert calls == {}, (kw, calls)


def test_serve_frame_single_and_batched():
    import test_gpu_serve_frame as SF
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    model = SF._model('classical')
    net = model.netG
    g = torch.Generator().manual_seed(9)
    h, w, size = 48, 64, (40, 52)
    dev = torch.randint(0, WHITE + 1, (2, h, w), generator=g, dtype=torch.int32).to(torch.uint16).cuda()
    kw = dict(tile_batch=5, black_level=64, cfa='gbrg')
    store = 'sharpen' if PF.sharpen_store('nv12') == 'fused' else 'pass'
    bgr = net.serve_frame(dev, float(WHITE), 32, 16, **kw).clone()
    assert net.last_serve_route == 'tiled' and net.last_serve_sharpen is None
    _, plain = _counted(lambda: net.serve_frame(dev, float(WHITE), 32, 16, **kw))
    got, calls = _counted(lambda: net.serve_frame(dev, float(WHITE), 32, 16, sharpen=SHARP, **kw))
    assert net.last_serve_route == 'tiled' and net.last_serve_sharpen == 'pass' and net.last_serve_store is None
    assert calls == dict(plain, risp_bgr8_sharpen=1), (calls, plain)
    assert tuple(got.shape) == (2, h, w, 3) and torch.equal(got, _ref(bgr, SHARP))
    # a single (H,W) frame gives (H,W,3); the IspModel passes the keyword through; reversed channels; out=
    one = model.serve_frame(dev[1], float(WHITE), 32, 16, sharpen=SHARP, **kw)
    assert tuple(one.shape) == (h, w, 3) and torch.equal(one, got[1])
    rev = net.serve_frame(dev[1], float(WHITE), 32, 16, reverse_channels=True, sharpen=SHARP, **kw)
    assert torch.equal(rev, one.flip(-1))
    buf = torch.empty_like(got)
    assert net.serve_frame(dev, float(WHITE), 32, 16, out=buf, sharpen=SHARP, **kw) is buf and torch.equal(buf, got)
    warp, mesh = _warp('bicubic', h, w, size)
    nv, calls = _counted(lambda: net.serve_frame(dev, float(WHITE), 32, 16, out_format='nv12', yuv_matrix='bt601_video', warp=warp,
                                                 out_size=OUT, sharpen=SHARP1, **kw))
    assert net.last_serve_warp == 'pass' and net.last_serve_resize == 'pass' and net.last_serve_sharpen == 'pass'
    assert net.last_serve_store == store
    assert calls['risp_bgr8_warp'] == 1 and calls['risp_bgr8_resize'] == 1 and calls['risp_bgr8_sharpen'] == 1
    assert torch.equal(nv, _ref(bgr, SHARP1, warp=(mesh, size, 'bicubic'), out_size=OUT, matrix='bt601_video'))
    nv = net.serve_frame(dev[0], float(WHITE), 32, 16, out_format='nv12', sharpen=SHARP, **kw)
    assert tuple(nv.shape) == (h * 3 // 2, w) and torch.equal(nv, _ref(bgr[:1], SHARP, matrix='bt601_full')[0])
    assert torch.equal(model.serve(dev, float(WHITE), black_level=64, sharpen=SHARP),
                       _ref(model.serve(dev, float(WHITE), black_level=64).clone(), SHARP))
    _, calls = _counted(lambda: _refused(lambda: net.serve_frame(dev, float(WHITE), 32, 16, sharpen=(640, 2, 48, 0), **kw), 'radius'))
    assert calls == {}
    assert torch.equal(net.serve_frame(dev, float(WHITE), 32, 16, **kw), bgr) and net.last_serve_sharpen is None


def test_a_warm_call_is_captured_in_a_graph_and_replayed_on_new_frames():
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    net = CF._pipeline(SC.ARCHS[0])
    xa, xb = (CF._u16(CF._raw(2, H, W, WHITE, seed=s)) for s in (11, 12))
    plain = dict(black_level=64, cfa='grbg')
    kw = dict(sharpen=SHARP, out_size=OUT, resample='bicubic', out_format='nv12', **plain)
    eager = [_ref(net.serve(x, float(WHITE), **plain), SHARP, out_size=OUT, resample='bicubic', matrix='bt601_full') for x in (xa, xb)]
    assert not torch.equal(eager[0], eager[1])
    before_plain = net.serve(xa, float(WHITE), **plain).clone()
    slot = xa.clone()
    buf = torch.zeros((2, OUT[0] * 3 // 2, OUT[1]), dtype=torch.uint8, device='cuda')
    net.serve(slot, float(WHITE), out=buf, **kw)            # fills the caches: the tables, the images
    assert net.last_serve_sharpen == 'pass' and torch.equal(buf, eager[0])
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
    # packed BGR out too, straight behind the route
    kw = dict(sharpen=SHARP1, **plain)
    eager = [_ref(net.serve(x, float(WHITE), **plain), SHARP1) for x in (xa, xb)]
    out = torch.zeros((2, H, W, 3), dtype=torch.uint8, device='cuda')
    slot.copy_(xa)
    net.serve(slot, float(WHITE), out=out, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.serve(slot, float(WHITE), out=out, **kw)
    slot.copy_(xb)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[1])
    assert torch.equal(net.serve(xa, float(WHITE), **plain), before_plain) and net.last_serve_sharpen is None
