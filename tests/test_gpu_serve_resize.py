"""GPU: a scaled, cropped output of the serving path - the resize launch (risp_bgr8_resize) against tests/resize_reference.py,
and ``serve`` / ``serve_frame`` with ``out_size`` / ``out_window`` on every route.

The output is an integer function of the packed bytes, so every comparison is ``torch.equal``; nothing here has a tolerance.

Shapes.  A workgroup owns RESIZE_TILE_W = 64 output columns x 16 output rows (8, 4, 2 where the source rows of 16 do not fit
the LDS budget).  The listed cases are single tiles with ragged edges, enlargements, reductions up to the 32-tap limit, one
output column, one output row, a window and a crop; ``TILED`` has three whole tiles and a ragged one on both axes, and its box
form reduces the rows 32:1, where 16 output rows would need 512 source rows and the launch takes 8."""
import ctypes as C

import numpy as np
import pytest
import torch

import nv12_reference as NR
import resize_reference as RR
from bgr8_placement import _at_odd_address, _guards_intact

pytestmark = pytest.mark.gpu

WHITE = 1023
MATRICES = ('bt601_full', 'bt709_video')
_IMAGES, _WANT = {}, {}


def _image(ci):
    """case ci's input on the host, made once"""
    if ci not in _IMAGES:
        _IMAGES[ci] = RR.make_image(*RR.CASES[ci][0], seed=100 + ci)
    return _IMAGES[ci]


def _want(ci, kernel):
    """the reference's bytes for case ci, computed once and shared"""
    if (ci, kernel) not in _WANT:
        _, size, win = RR.CASES[ci]
        out = RR.resize(_image(ci), size, win, kernel)
        out.setflags(write=False)
        _WANT[ci, kernel] = out
    return _WANT[ci, kernel]


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


def _ref(bgr, size, win, kernel, matrix=None, channels='bgr'):
    """the reference on a packed device image (N,H,W,3), as a device tensor"""
    out = RR.resize(bgr.cpu().numpy(), size, win, kernel)
    if matrix is not None:
        out = NR.nv12(out, NR.TABLE[matrix], channels)
    return torch.from_numpy(out).cuda()


# ---------------------------------------------------------------- 1. the launch
@pytest.mark.parametrize('kernel', RR.KERNELS)
@pytest.mark.parametrize('ci', range(len(RR.CASES)), ids=lambda ci: '%s->%s@%s' % RR.CASES[ci])
def test_bgr8_resize_equals_the_reference(ci, kernel):
    import reconfigisp_amd.functional as F
    shape, size, win = RR.CASES[ci]
    img, want = _image(ci), _want(ci, kernel)
    dev = torch.from_numpy(img).cuda()
    got, calls = _counted(lambda: F.bgr8_resize(dev, size, win, kernel))
    assert calls == {'risp_bgr8_resize': 1}
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want), '%d bytes differ' % (got.cpu().numpy() != want).sum()
    if ci == 3:
        assert torch.equal(got, dev), 'D == S is one tap of 16384: the input'
    if size is None:
        y0, x0, h, w = win
        assert torch.equal(got, dev[:, y0:y0 + h, x0:x0 + w]), 'a crop'
    # a single (H,W,3) image
    assert np.array_equal(F.bgr8_resize(dev[0], size, win, kernel).cpu().numpy(), want[0])
    if want.shape[1] % 2 == 0 and want.shape[2] % 2 == 0:
        for matrix in MATRICES:
            nv, calls = _counted(lambda: F.bgr8_resize(dev, size, win, kernel, nv12=matrix))
            assert calls == {'risp_bgr8_resize': 1}
            expect = NR.nv12(want, NR.TABLE[matrix])
            assert np.array_equal(nv.cpu().numpy(), expect), '%s: %d bytes differ' % (matrix, (nv.cpu().numpy() != expect).sum())
            assert torch.equal(F.bgr8_to_nv12(got, matrix), nv), 'the other form: resize to BGR, then the conversion launch'
    else:
        with pytest.raises(ValueError, match='even'):
            F.bgr8_resize(dev, size, win, kernel, nv12='bt601_full')


@pytest.mark.parametrize('kernel', RR.KERNELS)
def test_a_reduction_beyond_32_taps_is_refused(kernel):
    """(1,37,53) -> (19,1): 53 samples to one need 53 taps with every kernel"""
    import reconfigisp_amd.functional as F
    shape, size, win = RR.REFUSED_CASE
    dev = torch.zeros(shape + (3,), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='RESIZE_MAX_TAPS'):
        F.bgr8_resize(dev, size, win, kernel)


# three whole tiles and a ragged one on both axes: 214 = 3 * 64 + 22 columns; 58 = 3 * 16 + 10 rows, and with the box kernel
# 26 = 3 * 8 + 2 rows out of 832 - 32:1, where the span of 16 rows (512 source rows x 192 bytes) passes the LDS budget
TILED = {'box': ((1, 832, 40), (26, 214)), 'triangle': ((1, 100, 300), (58, 214)), 'bicubic': ((1, 100, 300), (58, 214))}


@pytest.mark.parametrize('kernel', RR.KERNELS)
def test_tiles_and_ragged_remainders_on_both_axes(kernel):
    import reconfigisp_amd.functional as F
    shape, size = TILED[kernel]
    rows, span = F.resize_tile_rows(shape[1], size[0], kernel)
    assert F.RESIZE_TILE_W == 64 and rows == (8 if kernel == 'box' else 16)
    assert size[1] > 3 * F.RESIZE_TILE_W and size[1] % F.RESIZE_TILE_W and size[0] > 3 * rows and size[0] % rows
    img = RR.make_image(*shape, seed=31)
    dev = torch.from_numpy(img).cuda()
    want = RR.resize(img, size, None, kernel)
    got = F.bgr8_resize(dev, size, None, kernel)
    assert np.array_equal(got.cpu().numpy(), want), '%d bytes differ' % (got.cpu().numpy() != want).sum()
    nv = F.bgr8_resize(dev, size, None, kernel, nv12='bt709_full')
    assert np.array_equal(nv.cpu().numpy(), NR.nv12(want, NR.TABLE['bt709_full']))


def test_images_and_out_at_odd_addresses_and_nothing_outside_is_written():
    import reconfigisp_amd.functional as F
    ci, kernel = 0, 'bicubic'
    (n, h, w), size, win = RR.CASES[ci]
    img, want = _image(ci), torch.from_numpy(_want(ci, kernel).copy())
    view, _ = _at_odd_address(img, 1, 7, 0)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    assert torch.equal(F.bgr8_resize(view, size, win, kernel).cpu(), want)
    for at in (1, 2, 3, 4):
        out, obig = _at_odd_address(tuple(want.shape), at, 16 - at, 0xAA)
        assert out.data_ptr() % 4 == at % 4
        for _ in range(2):                                  # made twice: the second call finds the first one's bytes
            assert F.bgr8_resize(view, size, win, kernel, out=out) is out
            assert torch.equal(out.cpu(), want)
        assert _guards_intact(obig, out, 0xAA)
    # NV12 out: 4-byte aligned, and refused otherwise
    expect = torch.from_numpy(NR.nv12(want.numpy(), NR.TABLE['bt601_full']))
    out, obig = _at_odd_address(tuple(expect.shape), 4, 12, 0xAA)
    for _ in range(2):
        assert F.bgr8_resize(view, size, win, kernel, nv12='bt601_full', out=out) is out
        assert torch.equal(out.cpu(), expect)
    assert _guards_intact(obig, out, 0xAA)
    with pytest.raises(ValueError, match='aligned'):
        F.bgr8_resize(view, size, win, kernel, nv12='bt601_full', out=obig[2:2 + expect.numel()].view(expect.shape))


def test_nv12_with_a_last_tile_of_two_columns():
    """9 x 70 -> 6 x 66: OW % 4 == 2 and OW > 64, so the last column tile is two columns wide, its patches hold one quad and the
    store takes the byte form.  (``TILED`` reaches a one-quad patch too - 214 columns - but with one image, one channel order and
    no guard bytes.)"""
    import reconfigisp_amd.functional as F
    size = (6, 66)
    assert size[1] % 4 == 2 and F.RESIZE_TILE_W < size[1] < F.RESIZE_TILE_W + 4
    dev = torch.from_numpy(RR.make_image(2, 9, 70, seed=77)).cuda()
    packed = F.bgr8_resize(dev, size, None, 'triangle')
    assert np.array_equal(packed.cpu().numpy(), RR.resize(dev.cpu().numpy(), size, None, 'triangle'))
    for channels in ('bgr', 'rgb'):
        want = F.bgr8_to_nv12(packed, 'bt601_full', channels)
        out, buf = _at_odd_address(tuple(want.shape), 4, 12, 0xAA)
        assert out.data_ptr() % 4 == 0
        assert F.bgr8_resize(dev, size, None, 'triangle', nv12='bt601_full', channels=channels, out=out) is out
        assert torch.equal(out, want), (channels, (out != want).sum().item())
        assert _guards_intact(buf, out, 0xAA), 'bytes outside out were written'


def test_rgb_against_bgr_for_nv12():
    import reconfigisp_amd.functional as F
    ci = 0
    _, size, win = RR.CASES[ci]
    dev = torch.from_numpy(_image(ci)).cuda()
    for kernel in RR.KERNELS:
        want = _want(ci, kernel)
        for channels in ('bgr', 'rgb'):
            got = F.bgr8_resize(dev, size, win, kernel, nv12='bt709_video', channels=channels)
            assert np.array_equal(got.cpu().numpy(), NR.nv12(want, NR.TABLE['bt709_video'], channels)), (kernel, channels)
        # the swapped image read in the other order is the same picture
        assert torch.equal(F.bgr8_resize(dev.flip(-1), size, win, kernel, nv12='bt709_video', channels='rgb'),
                           F.bgr8_resize(dev, size, win, kernel, nv12='bt709_video'))


def test_a_warm_call_uploads_and_allocates_nothing():
    import reconfigisp_amd.functional as F
    dev = torch.from_numpy(_image(0)).cuda()
    out = torch.empty((2, 10, 18, 3), dtype=torch.uint8, device='cuda')
    F.bgr8_resize(dev, (10, 18), None, 'triangle', out=out)
    torch.cuda.synchronize()
    tables, before = dict(F._RESIZE_TABLES), torch.cuda.memory_allocated()
    assert F.bgr8_resize(dev, (10, 18), None, 'triangle', out=out) is out
    assert torch.cuda.memory_allocated() == before
    assert F._RESIZE_TABLES.keys() == tables.keys() and all(F._RESIZE_TABLES[k] is v for k, v in tables.items())


def test_python_refusals():
    import reconfigisp_amd.functional as F
    dev = torch.from_numpy(_image(0)).cuda()
    for kw in (dict(out_size=(0, 18)), dict(out_size=(10, 18), out_window=(0, 0, 25, 40)), dict(out_size=(10, 18), resample='lanczos'),
               dict(out_size=(10, 1)), dict(out_size=(9, 18), nv12='bt601_full'), dict(out_size=(10, 18), nv12='bt2020'),
               dict(out_size=(10, 18), out=torch.empty((2, 10, 18), dtype=torch.uint8, device='cuda')),
               dict(out_size=(10, 18), out=torch.empty((2, 10, 18, 3), dtype=torch.int8, device='cuda')),
               dict(out_size=(24, 40), out=dev), dict(out_size=(10, 18), channels='gbr')):
        with pytest.raises(ValueError):
            F.bgr8_resize(dev, **kw)
    with pytest.raises(RuntimeError):
        F.bgr8_resize(dev.cpu(), (10, 18))
    shared = torch.zeros(2 * 24 * 40 * 3 + 2 * 10 * 18 * 3, dtype=torch.uint8, device='cuda')
    src = shared[:2 * 24 * 40 * 3].view(2, 24, 40, 3)
    with pytest.raises(ValueError, match='shares memory'):
        F.bgr8_resize(src, (10, 18), out=shared[100:100 + 2 * 10 * 18 * 3].view(2, 10, 18, 3))


def test_refusals_through_the_c_abi_leave_the_output_alone():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    lib = L.load()
    n, h, w, oh, ow = 2, 24, 40, 10, 18
    img = torch.from_numpy(_image(0)).cuda()
    out = torch.full((n * oh * ow * 3 + 16,), 0x5A, device='cuda', dtype=torch.uint8)
    xs, xw, tx, _ = F._resize_axis(w, ow, 'triangle', 0, img.device)
    ys, yw, ty, _ = F._resize_axis(h, oh, 'triangle', 0, img.device)
    rows, span = F.resize_tile_rows(h, oh, 'triangle')
    p = lambda t: C.c_void_p(t.data_ptr())
    good = NR.TABLE['bt601_full']
    mat = lambda coef: (C.c_int * 12)(*coef) if coef is not None else None

    def call(img_p=p(img), out_p=p(out), xs_p=p(xs), xw_p=p(xw), tx=tx, ys_p=p(ys), yw_p=p(yw), ty=ty, rows=rows, span=span, coef=None,
             N=n, H=h, W=w, OH=oh, OW=ow):
        return lib.risp_bgr8_resize(img_p, out_p, xs_p, xw_p, tx, ys_p, yw_p, ty, rows, span, mat(coef), 0, N, H, W, OH, OW, F._stream())

    refused = {'null img': dict(img_p=None), 'null out': dict(out_p=None), 'null xstart': dict(xs_p=None), 'null xweight': dict(xw_p=None),
               'null ystart': dict(ys_p=None), 'null yweight': dict(yw_p=None), 'N 0': dict(N=0), 'N 65536': dict(N=65536), 'H 0': dict(H=0),
               'OW 0': dict(OW=0), 'tx 0': dict(tx=0), 'tx 33': dict(tx=33), 'ty 33': dict(ty=33), 'ty > H': dict(ty=25, H=24),
               'rows 0': dict(rows=0), 'rows 65': dict(rows=65), 'span 0': dict(span=0), 'span beyond LDS': dict(span=400),
               'out on img': dict(out_p=C.c_void_p(img.data_ptr() + 64)), 'NV12 odd OH': dict(coef=good, OH=9),
               'NV12 odd OW': dict(coef=good, OW=17), 'NV12 odd rows': dict(coef=good, rows=3),
               'NV12 out not aligned': dict(coef=good, out_p=C.c_void_p(out.data_ptr() + 2)),
               'a matrix row overflows': dict(coef=[256, 256, 256, 0] + list(good[4:]))}
    for what, kw in refused.items():
        assert call(**kw) != 0, '%s was accepted' % what
        assert b'risp_bgr8_resize' in lib.risp_last_error(), (what, lib.risp_last_error())
    assert call(tx=33) != 0 and b'RISP_RESIZE_MAX_TAPS' in lib.risp_last_error() and b'8:1' in lib.risp_last_error()
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item() and torch.equal(img.cpu(), torch.from_numpy(_image(0))), 'a refused call wrote'
    # the same arguments without the fault are accepted and write the image alone; so is a span larger than needed
    for kw in ({}, dict(span=span + 7), dict(coef=good)):
        out.fill_(0x5A)
        assert call(**kw) == 0
        torch.cuda.synchronize()
        size = n * oh * ow * 3 if 'coef' not in kw else n * (oh + oh // 2) * ow
        assert not (out[:size] == 0x5A).all().item() and (out[size:] == 0x5A).all().item()
        if 'coef' not in kw:
            assert np.array_equal(out[:size].view(n, oh, ow, 3).cpu().numpy(), _want(0, 'triangle'))


def test_a_wrong_table_gives_the_bytes_of_the_clamped_table():
    """starts a few samples past every edge of a random image that lies in the middle of a larger allocation of other bytes:
    the kernel clamps every start into the image as it loads it and every index start + k again, so the bytes are those of
    the clamped table - a missing clamp would read the bytes around the image and show as a mismatch - and the launch writes
    its image alone"""
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    lib = L.load()
    n, h, w, oh, ow, pad = 1, 12, 16, 6, 8, 6
    rng = np.random.default_rng(17)
    host = rng.integers(0, 256, size=((h + 2 * pad) * w * 3,), dtype=np.uint8)
    big = torch.from_numpy(host).cuda()
    img = big[pad * w * 3:(pad + h) * w * 3].view(n, h, w, 3)
    src = host[pad * w * 3:(pad + h) * w * 3].reshape(h, w, 3).astype(np.int64)
    xs = np.array([-3, -1, 0, 5, 14, 15, 16, 18], dtype=np.int32)
    ys = np.array([-2, 0, 3, 10, 11, 13], dtype=np.int32)
    xw = np.tile(np.array([[4096, 12288]], dtype=np.int16), (ow, 1))
    yw = np.tile(np.array([[12288, 4096]], dtype=np.int16), (oh, 1))
    xi = np.clip(np.clip(xs, 0, w - 1)[:, None] + np.arange(2), 0, w - 1)              # (OW,2)
    yi = np.clip(np.clip(ys, 0, h - 1)[:, None] + np.arange(2), 0, h - 1)              # (OH,2)
    hor = np.clip(((src[:, xi, :] * xw.astype(np.int64)[None, :, :, None]).sum(axis=2) + 8192) >> 14, 0, 255)
    want = np.clip(((hor[yi] * yw.astype(np.int64)[:, :, None, None]).sum(axis=1) + 8192) >> 14, 0, 255).astype(np.uint8)
    # two output rows per tile: the spans of the clamped starts are 2, 10 + 2 - 3 = 9 and 2
    rows, span = 2, 9
    out = torch.full((n * oh * ow * 3 + 16,), 0x5A, device='cuda', dtype=torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())
    dev = [torch.from_numpy(a).cuda() for a in (xs, xw, ys, yw)]
    assert lib.risp_bgr8_resize(p(img), p(out), p(dev[0]), p(dev[1]), 2, p(dev[2]), p(dev[3]), 2, rows, span, None, 0, n, h, w, oh, ow,
                                F._stream()) == 0
    torch.cuda.synchronize()
    got = out[:n * oh * ow * 3].view(oh, ow, 3).cpu().numpy()
    assert np.array_equal(got, want), '%d bytes differ' % (got != want).sum()
    assert (out[n * oh * ow * 3:] == 0x5A).all().item() and np.array_equal(big.cpu().numpy(), host)


# ---------------------------------------------------------------- 2. serve() on every route
H, W = 16, 24               # the smallest geometry every route accepts
SIZE, SIZE_NV12 = (10, 18), (12, 20)


def _route_case(what):
    """(net, frames, keywords of serve(), the route they take), built as tests/test_gpu_serve_nv12.py builds them"""
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    import test_gpu_serve_cond as GC
    import test_gpu_serve_denoise as D
    n = 2
    if what == 'fused':
        return CF._pipeline('Demosaic_01_sRGB_07_11_01_14'), CF._u16(CF._raw(n, H, W, WHITE, seed=40)), {}, 'fused'
    if what == 'classical':
        return CF._pipeline(SC.ARCHS[1]), CF._u16(CF._raw(n, H, W, WHITE, seed=46)), {}, 'classical'
    if what == 'scene':
        return CF._pipeline('Demosaic_02_sRGB_05_01'), D._frames(n, H, W, seed=41), dict(fast_scene=True), 'scene'
    if what == 'denoise':
        return CF._pipeline('Bayer_02_Demosaic_02_sRGB_07_01'), D._frames(n, H, W, seed=42), dict(fast_denoise=True), 'denoise'
    if what == 'denoise_scene':
        return CF._pipeline('Demosaic_02_sRGB_05_07_01'), D._frames(n, H, W, seed=43), dict(fast_denoise_scene=True), 'denoise_scene'
    if what == 'cond':
        return GC._net('Demosaic_01_sRGB_18_01', H * W), GC._u16(GC._head_frames(n, H, W, seed=44)), dict(fast_cond=True), 'cond'
    return CF._pipeline('Demosaic_02_sRGB_13', 'IspUniversal'), D._frames(n, H, W, seed=45), {}, 'composed'


ROUTES = ['fused', 'classical', 'scene', 'denoise', 'denoise_scene', 'cond', 'composed']


@pytest.mark.parametrize('what', ROUTES)
def test_serve_resizes_behind_every_route(what, monkeypatch):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    net, dev, kw, route = _route_case(what)
    n = dev.shape[0]
    sensor = dict(black_level=64, cfa='grbg')
    win = (2, 3, 13, 19)
    bgr = net.serve(dev, float(WHITE), **sensor, **kw).clone()
    assert net.last_serve_route == route and net.last_serve_resize is None
    _, plain_calls = _counted(lambda: net.serve(dev, float(WHITE), **sensor, **kw))
    for kernel in RR.KERNELS:
        got, calls = _counted(lambda: net.serve(dev, float(WHITE), out_size=SIZE, out_window=win, resample=kernel, **sensor, **kw))
        assert net.last_serve_route == route and net.last_serve_resize == 'pass' and net.last_serve_store is None
        assert calls == dict(plain_calls, risp_bgr8_resize=1), (calls, plain_calls)
        assert tuple(got.shape) == (n,) + SIZE + (3,)
        assert torch.equal(got, F.bgr8_resize(bgr, SIZE, win, kernel)) and torch.equal(got, _ref(bgr, SIZE, win, kernel))
    assert len(torch.unique(got)) > 8, 'a flat image would prove nothing'
    # NV12: the resize launch stores it, or the conversion launch follows - both answers of resize_store
    for table, store, extra in ((frozenset({'nv12'}), 'resize', {}), (frozenset(), 'pass', dict(risp_bgr8_to_nv12=1))):
        monkeypatch.setattr(PF, '_RESIZE_NV12_FUSED', table)
        got, calls = _counted(lambda: net.serve(dev, float(WHITE), out_format='nv12', yuv_matrix='bt709_full', out_size=SIZE_NV12,
                                                resample='bicubic', **sensor, **kw))
        assert net.last_serve_route == route and net.last_serve_resize == 'pass' and net.last_serve_store == store
        assert calls == dict(plain_calls, risp_bgr8_resize=1, **extra), (calls, plain_calls)      # the BGR launches of the route
        assert tuple(got.shape) == (n, SIZE_NV12[0] * 3 // 2, SIZE_NV12[1])
        assert torch.equal(got, _ref(bgr, SIZE_NV12, None, 'bicubic', 'bt709_full'))
    # the call without the keywords before and after: byte-identical
    assert torch.equal(net.serve(dev, float(WHITE), **sensor, **kw), bgr) and net.last_serve_resize is None


def test_serve_with_another_phase_reversed_channels_packed_frames_shading_and_defects():
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
        bgr = net.serve(dev, float(WHITE), **kw).clone()
        got = net.serve(dev, float(WHITE), out_size=SIZE, resample='bicubic', **kw)
        assert torch.equal(got, F.bgr8_resize(bgr, SIZE, None, 'bicubic')) and torch.equal(got, _ref(bgr, SIZE, None, 'bicubic')), kw
        assert net.last_serve_resize == 'pass'
    # RAW10 in: the fused packed load of the classical route stays, the resize launch follows
    bgr = net.serve(dev, float(WHITE), black_level=64).clone()
    got, calls = _counted(lambda: net.serve(packed, float(WHITE), black_level=64, raw_format='raw10', raw_width=W, out_size=SIZE,
                                            out_window=(0, 4, 16, 20)))
    _, plain = _counted(lambda: net.serve(packed, float(WHITE), black_level=64, raw_format='raw10', raw_width=W))
    assert calls == dict(plain, risp_bgr8_resize=1) and net.last_serve_load == 'fused'
    assert torch.equal(got, _ref(bgr, SIZE, (0, 4, 16, 20), 'triangle'))
    assert torch.equal(net.serve(dev, float(WHITE), black_level=64), bgr) and net.last_serve_resize is None


def _refused(fn, what):
    with pytest.raises(ValueError, match=what):
        fn()


def test_serve_refuses_before_anything_is_launched():
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    net = CF._pipeline(SC.ARCHS[0])
    dev = CF._u16(CF._raw(2, H, W, WHITE, seed=5))
    good = torch.empty((2,) + SIZE + (3,), dtype=torch.uint8, device='cuda')
    for kw, what in ((dict(out_size=(0, 4)), 'out_size'), (dict(out_window=(0, 0, 17, 24)), 'out_window'),
                     (dict(out_size=SIZE, resample='lanczos'), 'resample'),
                     (dict(out_size=(11, 18), out_format='nv12'), 'even'), (dict(out_size=SIZE, out=good[:, :, :17]), 'out must be'),
                     (dict(out_size=SIZE, out=good[:1]), 'out must be'),
                     (dict(out_size=SIZE_NV12, out_format='nv12', reverse_channels=True), 'reverse_channels'),
                     (dict(out_size=SIZE_NV12, out_format='nv12', yuv_matrix='bt2020'), 'matrix')):
        _, calls = _counted(lambda: _refused(lambda: net.serve(dev, float(WHITE), **kw), what))
        assert calls == {}, (kw, calls)
    big = CF._u16(CF._raw(1, 80, 24, WHITE, seed=6))
    _, calls = _counted(lambda: _refused(lambda: net.serve(big, float(WHITE), out_size=(1, 24)), 'RESIZE_MAX_TAPS'))
    assert calls == {}


# ---------------------------------------------------------------- 3. serve_frame, a captured graph
def test_serve_frame_single_and_batched():
    import reconfigisp_amd.functional as F
    import test_gpu_serve_frame as SF
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    model = SF._model('classical')
    net = model.netG
    g = torch.Generator().manual_seed(9)
    dev = torch.randint(0, WHITE + 1, (2, 48, 64), generator=g, dtype=torch.int32).to(torch.uint16).cuda()
    kw = dict(tile_batch=5, black_level=64, cfa='gbrg')
    win, size = (4, 8, 40, 50), (18, 26)
    bgr = net.serve_frame(dev, float(WHITE), 32, 16, **kw).clone()
    assert net.last_serve_route == 'tiled' and net.last_serve_resize is None
    _, plain = _counted(lambda: net.serve_frame(dev, float(WHITE), 32, 16, **kw))
    got, calls = _counted(lambda: net.serve_frame(dev, float(WHITE), 32, 16, out_size=size, out_window=win, resample='bicubic', **kw))
    assert net.last_serve_route == 'tiled' and net.last_serve_resize == 'pass' and net.last_serve_store is None
    assert calls == dict(plain, risp_bgr8_resize=1), (calls, plain)
    assert tuple(got.shape) == (2,) + size + (3,) and torch.equal(got, _ref(bgr, size, win, 'bicubic'))
    # a single (H,W) frame gives (OH,OW,3); the IspModel passes the keywords through; reversed channels; out=
    one = model.serve_frame(dev[1], float(WHITE), 32, 16, out_size=size, out_window=win, resample='bicubic', **kw)
    assert tuple(one.shape) == size + (3,) and torch.equal(one, got[1])
    rev = net.serve_frame(dev[1], float(WHITE), 32, 16, reverse_channels=True, out_size=size, out_window=win, resample='bicubic', **kw)
    assert torch.equal(rev, one.flip(-1))
    buf = torch.empty_like(got)
    assert net.serve_frame(dev, float(WHITE), 32, 16, out=buf, out_size=size, out_window=win, resample='bicubic', **kw) is buf
    assert torch.equal(buf, got)
    nv = net.serve_frame(dev, float(WHITE), 32, 16, out_format='nv12', yuv_matrix='bt601_video', out_size=size, out_window=win, **kw)
    assert net.last_serve_store == ('resize' if PF.resize_store('nv12') == 'fused' else 'pass') and net.last_serve_resize == 'pass'
    assert torch.equal(nv, _ref(bgr, size, win, 'triangle', 'bt601_video'))
    assert torch.equal(model.serve(dev, float(WHITE), black_level=64, out_size=size), F.bgr8_resize(model.serve(dev, float(WHITE), black_level=64), size))
    _, calls = _counted(lambda: _refused(lambda: net.serve_frame(dev, float(WHITE), 32, 16, out_size=(17, 26), out_format='nv12', **kw),
                                         'even'))
    assert calls == {}
    assert torch.equal(net.serve_frame(dev, float(WHITE), 32, 16, **kw), bgr) and net.last_serve_resize is None


def test_a_warm_call_is_captured_in_a_graph_and_replayed_on_new_frames():
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as SC
    net = CF._pipeline(SC.ARCHS[0])
    xa, xb = (CF._u16(CF._raw(2, H, W, WHITE, seed=s)) for s in (11, 12))
    plain = dict(black_level=64, cfa='grbg')
    win = (0, 2, 16, 22)
    kw = dict(out_size=SIZE_NV12, out_window=win, resample='bicubic', out_format='nv12', **plain)
    eager = [_ref(net.serve(x, float(WHITE), **plain), SIZE_NV12, win, 'bicubic', 'bt601_full') for x in (xa, xb)]
    assert not torch.equal(eager[0], eager[1])
    before_plain = net.serve(xa, float(WHITE), **plain).clone()
    slot = xa.clone()
    buf = torch.zeros((2, SIZE_NV12[0] * 3 // 2, SIZE_NV12[1]), dtype=torch.uint8, device='cuda')
    net.serve(slot, float(WHITE), out=buf, **kw)            # fills the caches: the tables, the sensor-size image
    assert net.last_serve_resize == 'pass' and torch.equal(buf, eager[0])
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
    assert torch.equal(net.serve(xa, float(WHITE), **plain), before_plain) and net.last_serve_resize is None
