"""GPU: YUV 4:2:0 (NV12) out of the serving path - the conversion launch (risp_bgr8_to_nv12), the fused NV12 stores of the
one-launch kernels (risp_serve_nv12, risp_serve_classical_nv12) and ``serve(out_format='nv12')`` on every route.

The NV12 bytes are an integer function of the 8-bit codes the BGR route stores, so every comparison is ``torch.equal`` against
tests/nv12_reference.py (numpy int64) applied to the bytes the same object returns without the keyword; nothing here has a
tolerance.

Shapes.  The conversion launch: (2,2), (2,6) and (6,10) have W % 4 != 0 and take the scalar form (one quad per thread);
(4,4), (32,64) and (34,68) take the vector form (a 2 x 4 patch per thread), and a 4-aligned shape read through a view one
byte off takes the scalar form again.  The fused kernels' workgroup owns a 64 x 32 pixel tile: 4 x 4 and 2 x 4 are one
patch or one row of patches, 6 x 12 and 10 x 12 have interior patches, 34 x 68 crosses the tile both ways."""
import ctypes as C

import pytest
import torch

import nv12_reference as NR
from bgr8_placement import _at_odd_address, _guards_intact

pytestmark = pytest.mark.gpu

WHITE = 1023
PRESETS = list(NR.TABLE)


def _ref(bgr, matrix='bt601_full', channels='bgr'):
    """the reference on the bytes of a packed (N,H,W,3) device image, as a device tensor"""
    coef = NR.TABLE[matrix] if isinstance(matrix, str) else matrix
    return torch.from_numpy(NR.nv12(bgr.cpu().numpy(), coef, channels)).cuda()


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


# ---------------------------------------------------------------- 1. the conversion launch
def _images(n, h, w, seed):
    """random bytes, all 0, all 255, and the six primaries and secondaries cycling pixel by pixel (so that quads mix them)"""
    g = torch.Generator().manual_seed(seed)
    palette = torch.tensor([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255]], dtype=torch.uint8)
    idx = (torch.arange(w)[None, :] + 2 * torch.arange(h)[:, None] + torch.arange(n)[:, None, None]) % 6
    return {'random': torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8),
            'zeros': torch.zeros((n, h, w, 3), dtype=torch.uint8), 'ones': torch.full((n, h, w, 3), 255, dtype=torch.uint8),
            'palette': palette[idx]}


@pytest.mark.parametrize('n,h,w', [(1, 2, 2), (2, 2, 6), (3, 6, 10), (2, 4, 4), (1, 32, 64), (2, 34, 68)], ids=lambda v: str(v))
def test_bgr8_to_nv12_equals_the_reference(n, h, w):
    import reconfigisp_amd.functional as F
    for what, img in _images(n, h, w, seed=7 * h + w).items():
        dev = img.cuda()
        for matrix in PRESETS:
            for channels in ('bgr', 'rgb'):
                want = torch.from_numpy(NR.nv12(img.numpy(), NR.TABLE[matrix], channels)).cuda()
                got = F.bgr8_to_nv12(dev, matrix, channels)
                assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h + h // 2, w)
                assert torch.equal(got, want), '%dx%dx%d %s %s %s: %d bytes differ' % (n, h, w, what, matrix, channels,
                                                                                      (got != want).sum().item())
    # twelve integers in place of a name, and a single (H,W,3) image
    dev = _images(n, h, w, seed=1)['random'].cuda()
    coef = [256, 0, 0, 255, 0, 256, 0, 0, 0, 0, -256, 65535]
    assert torch.equal(F.bgr8_to_nv12(dev, coef), _ref(dev, coef))
    assert torch.equal(F.bgr8_to_nv12(dev[0]), _ref(dev[:1])[0])


def test_bgr8_to_nv12_through_views_one_byte_off():
    """a 4-aligned shape whose input, then output, starts at an odd address: the scalar form, and nothing outside is written"""
    import reconfigisp_amd.functional as F
    n, h, w = 2, 34, 68
    img = _images(n, h, w, seed=5)['random']
    want = torch.from_numpy(NR.nv12(img.numpy(), NR.TABLE['bt709_video']))
    view, _ = _at_odd_address(img, 1, 7, 0)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    got, calls = _counted(lambda: F.bgr8_to_nv12(view, 'bt709_video'))
    assert calls == {'risp_bgr8_to_nv12': 1} and torch.equal(got.cpu(), want)
    out, obig = _at_odd_address(tuple(want.shape), 3, 5)
    assert out.data_ptr() % 4 == 3
    assert F.bgr8_to_nv12(img.cuda(), 'bt709_video', out=out) is out
    assert torch.equal(out.cpu(), want) and _guards_intact(obig, out)


# ---------------------------------------------------------------- 2. the fused stores through the pipelines' serve()
def _sensor_cases():
    import test_gpu_serve_cfa as CF
    return [(black, phase) for black in CF.BLACKS for phase in CF.PHASES]


def _check_fused(net, n, h, w, route, entry, seed):
    import test_gpu_serve_cfa as CF
    dev = CF._u16(CF._raw(n, h, w, WHITE, seed=seed))
    for k, (black, phase) in enumerate(_sensor_cases()):
        matrix = PRESETS[k % 4]
        bgr = net.serve(dev, float(WHITE), black_level=black, cfa=phase)
        assert net.last_serve_route == route and net.last_serve_store is None
        got, calls = _counted(lambda: net.serve(dev, float(WHITE), black_level=black, cfa=phase, out_format='nv12', yuv_matrix=matrix))
        assert net.last_serve_route == route and net.last_serve_store == 'fused'
        assert calls == {entry: 1}, calls
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h + h // 2, w)
        want = _ref(bgr, matrix)
        assert torch.equal(got, want), '%dx%dx%d %s black %d %s: %d bytes differ' % (n, h, w, phase, black, matrix,
                                                                                    (got != want).sum().item())
    assert h * w < 64 or len(torch.unique(got)) > 8, 'a flat image would prove nothing'


def _classical_archs():
    import test_gpu_serve_classical as SC
    return SC.ARCHS


@pytest.mark.parametrize('n,h,w', [(2, 4, 4), (1, 6, 12), (3, 34, 68)], ids=lambda v: str(v))
@pytest.mark.parametrize('k', range(4))
def test_classical_route_stores_nv12_in_its_one_launch(k, n, h, w):
    import test_gpu_serve_cfa as CF
    net = CF._pipeline(_classical_archs()[k])
    _check_fused(net, n, h, w, 'classical', 'risp_serve_classical_nv12', seed=3 * h + n + k)


@pytest.mark.parametrize('arch,n,h,w', [('Demosaic_01_sRGB_07_11_01_14', 1, 10, 12), ('Demosaic_01_sRGB_07_11_01_14', 3, 34, 68),
                                        ('Demosaic_01_sRGB_11_01_14', 2, 2, 4)], ids=lambda v: str(v))
def test_fused_route_stores_nv12_in_its_one_launch(arch, n, h, w):
    import test_gpu_serve_cfa as CF
    net = CF._pipeline(arch)
    _check_fused(net, n, h, w, 'fused', 'risp_serve_nv12', seed=5 * h + n)


# ---------------------------------------------------------------- 3. every other route: BGR scratch, then the conversion launch
def _pass_case(what):
    """(net, frames, keywords of serve(), the route they take)"""
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_cond as GC
    import test_gpu_serve_denoise as D
    n, h, w = 2, 34, 68
    if what == 'scene':
        return CF._pipeline('Demosaic_02_sRGB_05_01'), D._frames(n, h, w, seed=41), dict(fast_scene=True), 'scene'
    if what == 'denoise':
        return CF._pipeline('Bayer_02_Demosaic_02_sRGB_07_01'), D._frames(n, h, w, seed=42), dict(fast_denoise=True), 'denoise'
    if what == 'denoise_scene':
        return CF._pipeline('Demosaic_02_sRGB_05_07_01'), D._frames(n, h, w, seed=43), dict(fast_denoise_scene=True), 'denoise_scene'
    if what == 'cond':
        return GC._net('Demosaic_01_sRGB_18_01', h * w), GC._u16(GC._head_frames(n, h, w, seed=44)), dict(fast_cond=True), 'cond'
    # a CNN pipeline: the demosaic proxy network, then WbQuadratic
    return CF._pipeline('Demosaic_02_sRGB_13', 'IspUniversal'), D._frames(n, h, w, seed=45), {}, 'composed'


@pytest.mark.parametrize('what', ['scene', 'denoise', 'denoise_scene', 'cond', 'composed'])
def test_pass_store_routes(what):
    net, dev, kw, route = _pass_case(what)
    n, h, w = dev.shape
    sensor = dict(black_level=64, cfa='grbg')
    bgr = net.serve(dev, float(WHITE), **sensor, **kw).clone()
    assert net.last_serve_route == route and net.last_serve_store is None
    _, plain_calls = _counted(lambda: net.serve(dev, float(WHITE), **sensor, **kw))
    got, calls = _counted(lambda: net.serve(dev, float(WHITE), out_format='nv12', yuv_matrix='bt709_full', **sensor, **kw))
    assert net.last_serve_route == route and net.last_serve_store == 'pass'
    assert calls == dict(plain_calls, risp_bgr8_to_nv12=1), (calls, plain_calls)
    assert tuple(got.shape) == (n, h + h // 2, w) and torch.equal(got, _ref(bgr, 'bt709_full'))
    assert len(torch.unique(got)) > 8
    # the call without the keyword still gives its bytes, and a warm call with out= allocates nothing
    assert torch.equal(net.serve(dev, float(WHITE), **sensor, **kw), bgr) and net.last_serve_store is None
    buf = torch.empty_like(got)
    net.serve(dev, float(WHITE), out=buf, out_format='nv12', **sensor, **kw)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert net.serve(dev, float(WHITE), out=buf, out_format='nv12', **sensor, **kw) is buf
    if what != 'composed':                                 # (the composed route allocates its fp32 planes with or without NV12)
        assert torch.cuda.memory_allocated() == before
    assert torch.equal(buf, _ref(bgr))


def test_serve_frame_converts_each_frame():
    import test_gpu_serve_frame as SF
    model = SF._model('classical')
    net = model.netG
    dev = SF._u16(SF._raw(2, seed=6))
    kw = dict(tile_batch=5, black_level=64, cfa='gbrg')
    bgr = net.serve_frame(dev, float(WHITE), SF.SIZE, SF.STRIDE, **kw).clone()
    assert net.last_serve_route == 'tiled' and net.last_serve_store is None
    got, calls = _counted(lambda: net.serve_frame(dev, float(WHITE), SF.SIZE, SF.STRIDE, out_format='nv12', yuv_matrix='bt601_video', **kw))
    assert net.last_serve_route == 'tiled' and net.last_serve_store == 'pass'
    assert calls.get('risp_tile_blend_u8') == 2 and calls.get('risp_bgr8_to_nv12') == 2, calls
    assert tuple(got.shape) == (2, SF.H + SF.H // 2, SF.W) and torch.equal(got, _ref(bgr, 'bt601_video'))
    # a single (H,W) frame gives (3H/2,W); the IspModel passes the keywords through
    one = model.serve_frame(dev[1], float(WHITE), SF.SIZE, SF.STRIDE, out_format='nv12', yuv_matrix='bt601_video', **kw)
    assert tuple(one.shape) == (SF.H + SF.H // 2, SF.W) and torch.equal(one, got[1])
    buf = torch.empty_like(one)
    assert net.serve_frame(dev[1], float(WHITE), SF.SIZE, SF.STRIDE, out=buf, out_format='nv12', **kw) is buf
    assert torch.equal(buf, _ref(bgr[1:])[0])
    with pytest.raises(ValueError):
        net.serve_frame(dev[1], float(WHITE), SF.SIZE, SF.STRIDE, reverse_channels=True, out_format='nv12', **kw)
    with pytest.raises(ValueError):
        net.serve_frame(dev[1], float(WHITE), SF.SIZE, SF.STRIDE, out_format='i420', **kw)


# ---------------------------------------------------------------- 4. out=, refusals
@pytest.mark.parametrize('arch', ['Demosaic_03_sRGB_11_04_01', 'Demosaic_01_sRGB_07_11_01_14'])
def test_out_is_honoured_and_a_warm_call_allocates_nothing(arch):
    import test_gpu_serve_cfa as CF
    net = CF._pipeline(arch)
    n, h, w = 3, 34, 68
    dev = CF._u16(CF._raw(n, h, w, WHITE, seed=90))
    want = _ref(net.serve(dev, 1023.0, black_level=64, cfa='bggr'), 'bt601_video')
    kept = net.intermediate_results
    big = torch.full((n * (h + h // 2) * w + 64,), 0xA5, device='cuda', dtype=torch.uint8)
    buf = big[12:12 + n * (h + h // 2) * w].view(n, h + h // 2, w)        # 4-byte aligned, neither 8 nor 16
    net.serve(dev, 1023.0, out=buf, black_level=64, cfa='bggr', out_format='nv12', yuv_matrix='bt601_video')
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert net.serve(dev, 1023.0, out=buf, black_level=64, cfa='bggr', out_format='nv12', yuv_matrix='bt601_video') is buf
    assert torch.cuda.memory_allocated() == before
    assert net.last_serve_store == 'fused' and torch.equal(buf, want)
    assert (big[:12] == 0xA5).all().item() and (big[12 + buf.numel():] == 0xA5).all().item()
    assert net.intermediate_results is kept, 'serve() touched intermediate_results'
    with pytest.raises(ValueError):
        net.serve(dev, 1023.0, out=torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8), out_format='nv12')


def test_python_refusals():
    import reconfigisp_amd.functional as F
    import test_gpu_serve_cfa as CF
    net = CF._pipeline('Demosaic_02_sRGB_11_01_14')
    dev = CF._u16(CF._raw(2, 34, 68, WHITE, seed=3))
    with pytest.raises(ValueError, match='reverse_channels'):
        net.serve(dev, 1023.0, reverse_channels=True, out_format='nv12')
    with pytest.raises(ValueError, match='out_format'):
        net.serve(dev, 1023.0, out_format='yuv420')
    with pytest.raises(ValueError, match='matrix'):
        net.serve(dev, 1023.0, out_format='nv12', yuv_matrix='bt2020')
    with pytest.raises(ValueError, match='matrix'):
        net.serve(dev, 1023.0, out_format='nv12', yuv_matrix=[256, 256, 256, 0] + [0] * 8)
    for odd in (dev[:, :33], dev[:, :, :67]):              # odd H, odd W
        with pytest.raises(ValueError, match='even'):
            net.serve(odd, 1023.0, out_format='nv12')
    img = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device='cuda')
    for bad in (dict(img_u8=img[:, :3]), dict(img_u8=img[:, :, :3]), dict(img_u8=img.float()), dict(img_u8=img[..., :2]),
                dict(img_u8=img, matrix='bt2020'), dict(img_u8=img, channels='gbr'),
                dict(img_u8=img, out=torch.empty((1, 4, 4, 3), dtype=torch.uint8, device='cuda'))):
        with pytest.raises(ValueError):
            F.bgr8_to_nv12(**bad)
    with pytest.raises(RuntimeError):
        F.bgr8_to_nv12(img.cpu())
    raw = dev[:, :4, :8].contiguous()
    with pytest.raises(ValueError, match='matrix'):
        F.serve_nv12(raw, 1023.0, [], [], matrix='bt2020')
    with pytest.raises(ValueError, match='matrix'):
        F.serve_classical_nv12(raw, 1023.0, 'bilinear', [], [], matrix=[0] * 11)


def test_refusals_through_the_c_abi_leave_the_output_alone():
    import reconfigisp_amd.functional as F
    import test_gpu_serve_cfa as CF
    from reconfigisp_amd import lib as L
    lib = L.load()
    n, h, w = 2, 4, 8
    raw = CF._u16(CF._raw(n, h, w, WHITE, seed=5))
    img = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8).cuda()
    out = torch.full((n * (h + h // 2) * w + 16,), 0x5A, device='cuda', dtype=torch.uint8)
    gam = torch.full((n, 1), 0.5).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    good = NR.TABLE['bt601_full']
    mat = lambda coef: (C.c_int * 12)(*coef) if coef is not None else None
    one, blk = (C.c_int * 1)(F.OP_GAMMA), L.ptr_array([gam.data_ptr()])

    def convert(img_p=p(img), out_p=p(out), coef=good, H=h, W=w, N=n):
        return lib.risp_bgr8_to_nv12(img_p, out_p, mat(coef), 0, N, H, W, F._stream())

    def fused(raw_p=p(raw), out_p=p(out), coef=good, H=h, W=w, N=n):
        return lib.risp_serve_nv12(raw_p, 1023.0, None, None, None, 0, 1, one, blk, out_p, mat(coef), N, H, W, 0, 0, F._stream())

    def classical(raw_p=p(raw), out_p=p(out), coef=good, H=h, W=w, N=n):
        return lib.risp_serve_classical_nv12(raw_p, 1023.0, 1, 1, one, blk, out_p, mat(coef), N, H, W, 0, 0, F._stream())

    overflow = [256, 256, 256, 0] + list(good[4:])
    negative = list(good[:8]) + [127, -106, -21, 0]
    for name, call, first in (('risp_bgr8_to_nv12', convert, 'img_p'), ('risp_serve_nv12', fused, 'raw_p'),
                              ('risp_serve_classical_nv12', classical, 'raw_p')):
        refused = {'null input': {first: None}, 'null out': dict(out_p=None), 'null matrix': dict(coef=None), 'odd H': dict(H=h - 1),
                   'odd W': dict(W=w - 1), 'N 0': dict(N=0), 'a row overflows': dict(coef=overflow),
                   'a row goes negative': dict(coef=negative), 'coefficient 257': dict(coef=[257, 0, 0, 0] + list(good[4:]))}
        if first == 'raw_p':
            refused['W % 4'] = dict(W=6)
        for what, kw in refused.items():
            assert call(**kw) != 0, '%s: %s was accepted' % (name, what)
            assert name.encode() in lib.risp_last_error(), (name, what, lib.risp_last_error())
        assert call(coef=overflow) != 0 and b'cy' in lib.risp_last_error()
        assert call(coef=negative) != 0 and b'cv' in lib.risp_last_error()
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item(), 'a refused call wrote to its output'
    # the same arguments without the fault are accepted (the conversion also with W % 4 != 0), and write the image alone
    size = n * (h + h // 2) * w
    for call in (convert, fused, classical):
        out.fill_(0x5A)
        assert call() == 0
        torch.cuda.synchronize()
        assert not (out[:size] == 0x5A).all().item() and (out[size:] == 0x5A).all().item()
    assert convert(W=6) == 0 and convert(H=2, W=2, N=1) == 0
    torch.cuda.synchronize()
    assert (out[size:] == 0x5A).all().item()
