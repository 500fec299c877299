"""GPU: the serving path for the four Bayer phases and a sensor black level.

One definition, one oracle, no tolerance anywhere (every comparison is torch.equal on bytes or on fp32 bits):

    serve(raw, white, black_level=b, cfa=c) == unflip_c( serve_as_it_was( flip_c( max(raw - b, 0) ), white - b ) )

``max(raw - b, 0)`` is an exact uint16 frame and ``flip_c`` is torch.flip along x (GRBG), y (GBRG) or both (BGGR), so the
right-hand side is computed with the entry points tests/test_gpu_serve.py already holds to the fp32 route; the clamped and
mirrored frames are prepared on the host.  The kernels under test do no flip pass: they mirror their addresses.

Shapes (a thread owns a 2 x 4 patch, a workgroup a 64 x 32 pixel tile): 2 x 4 is one patch, 10 x 12 the smallest frame at
which a pipeline's bilateral joins the launch - every ring clamp within three patches -, 34 x 68 crosses the tile both
ways, and 32 x 64 with N = 8 is a grid of 8 tiles, which takes the XCD-aware order."""
import ctypes as C
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu

PHASES = ['rggb', 'grbg', 'gbrg', 'bggr']
BLACKS = [0, 64]
WHITE = 1023


def _dims(code):
    return [d for d, bit in ((-1, 1), (-2, 2)) if code & bit]


def _flip_hw(t, code, image=False):
    """mirror H and W of (.., H, W) - or of (N, H, W, C) with image=True - along x where code & 1 and y where code & 2"""
    dims = [d - 1 if image else d for d in _dims(code)]
    return torch.flip(t, dims) if dims else t


def _raw(n, h, w, white, seed):
    """(N,H,W) int32 on the host: samples up to 10 % above the white level, some below the black levels of this file; image 1
    all zero and image 2 constant where the batch has them"""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(0, int(white * 1.1) + 1, (n, h, w), generator=g, dtype=torch.int32)
    raw[0, 0, 0] = int(white * 1.1)                       # above the white level
    raw[0, 0, 1], raw[0, 1, 0], raw[0, -1, -1] = 5, 63, 64     # below and at the black level
    if n > 1:
        raw[1] = 0
    if n > 2:
        raw[2] = white // 3
    return raw


def _u16(raw_i32):
    return raw_i32.to(torch.uint16).cuda()


def _clamped_mirrored(raw_i32, black, code):
    """flip_c(max(raw - b, 0)) as a uint16 device frame"""
    return _u16(_flip_hw((raw_i32 - black).clamp_(min=0), code).contiguous())


def _chain_params(n, seed):
    import reconfigisp_amd.functional as F
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    return {F.OP_WB_MANUAL: (u(n, 3) * 5).cuda(), F.OP_GAMMA: (0.2 + 0.6 * u(n, 1)).cuda(),
            F.OP_GTM_MANUAL: torch.sort(u(n, 3), dim=1).values.cuda(), F.OP_WB_QUADRATIC: (0.45 + 0.1 * u(n, 30)).cuda(),
            F.OP_GAIN3: (0.5 + 1.5 * u(n, 3)).cuda()}


def _tails():
    import reconfigisp_amd.functional as F
    return [[F.OP_WB_MANUAL, F.OP_GAMMA, F.OP_GTM_MANUAL],                                    # the instance without WbQuadratic
            [F.OP_WB_QUADRATIC, F.OP_WB_MANUAL, F.OP_GAMMA, F.OP_GTM_MANUAL, F.OP_GAIN3]]     # and with it


SIGMAS = [0.05, 10.0, 100.0]


def _stage_forms(n):
    """the three stage forms of tests/test_gpu_serve.py: no bilateral; per-image windows (3, 1, 3, ..) under max_window 3;
    window 1"""
    sc = torch.tensor([SIGMAS[i % 3] for i in range(n)]).cuda()
    ss = torch.tensor([SIGMAS[(i + 1) % 3] for i in range(n)]).cuda()
    mixed = torch.tensor([(3, 1, 3, 1)[i % 4] for i in range(n)], dtype=torch.int32).cuda()
    ones = torch.ones(n, dtype=torch.int32).cuda()
    return [None, (mixed, sc, ss, 3), (ones, ss, sc, 1)]


# ---------------------------------------------------------------- 1. serve_u8 against the flip oracle
@pytest.mark.parametrize('n,h,w', [(1, 2, 4), (3, 2, 4), (1, 10, 12), (3, 10, 12), (1, 34, 68), (3, 34, 68), (8, 32, 64)],
                         ids=lambda v: str(v))
def test_serve_u8_equals_the_flip_oracle(n, h, w):
    import reconfigisp_amd.functional as F
    raw = _raw(n, h, w, WHITE, seed=3 * h + n)
    dev = _u16(raw)
    pars = _chain_params(n, 11 * n + h)
    forms = _stage_forms(n)
    for black in BLACKS:
        divisor = float(WHITE - black)
        for phase in PHASES:
            code = F.CFA[phase]
            mirrored = _clamped_mirrored(raw, black, code)
            for form in forms:
                for ops in _tails():
                    params = [pars[op] for op in ops]
                    for reverse in (False, True):
                        want = _flip_hw(F.serve_u8(mirrored, divisor, ops, params, form, reverse), code, image=True)
                        got = F.serve_u8(dev, divisor, ops, params, form, reverse, black_level=black, cfa=phase)
                        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, w, 3)
                        assert torch.equal(got, want), '%dx%dx%d %s black %d window %s ops %s reverse %s: %d bytes differ' % (
                            n, h, w, phase, black, form and form[3], ops, reverse, (got != want).sum().item())
                        if code == 0 and black == 0:       # the keywords' defaults are today's entry point, and its bytes
                            assert torch.equal(F.serve_u8(dev, divisor, ops, params, form, reverse), got)


def test_serve_u8_cfa_entry_point_with_zero_keywords_gives_serve_u8_bytes():
    """risp_serve_u8_cfa itself (the Python default goes to risp_serve_u8) with black 0 and cfa 0"""
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    n, h, w = 3, 34, 68
    dev = _u16(_raw(n, h, w, WHITE, seed=9))
    pars = _chain_params(n, 4)
    ops = _tails()[1]
    params = [pars[op] for op in ops]
    win, sc, ss, wmax = _stage_forms(n)[1]
    want = F.serve_u8(dev, 1023.0, ops, params, (win, sc, ss, wmax))
    out = torch.zeros_like(want)
    p = lambda t: C.c_void_p(t.data_ptr())
    L.call('risp_serve_u8_cfa', p(dev), 1023.0, p(win), p(sc), p(ss), wmax, len(ops), (C.c_int * len(ops))(*ops),
           L.ptr_array([t.data_ptr() for t in params]), p(out), 0, n, h, w, 0, 0, F._stream())
    assert torch.equal(out, want)


# ---------------------------------------------------------------- 2. raw_crops
@pytest.mark.parametrize('size', [(2, 2), (6, 10), (34, 68)], ids=lambda s: '%dx%d' % s)
def test_raw_crops_equals_flipped_crops_of_the_clamped_frames(size):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.data.gpu_input import raw_crops
    frames = _raw(3, 40, 76, WHITE, seed=size[0])
    dev = _u16(frames)
    sel = torch.tensor([[2, 4, 6], [0, 2, 8], [1, 6, 2], [2, 0, 0]], dtype=torch.int32)       # non-zero even offsets (and one at 0)
    for black in BLACKS:
        clamped = _u16((frames - black).clamp_(min=0))
        for phase in PHASES:
            code = F.CFA[phase]
            want = _flip_hw(raw_crops(clamped, sel, size, float(WHITE - black)), code)
            got = raw_crops(dev, sel, size, float(WHITE), black_level=black, cfa=phase)
            assert got.dtype == torch.float32 and tuple(got.shape) == (4, 1) + size
            assert torch.equal(got, want), '%s black %d: %d values differ' % (phase, black, (got != want).sum().item())
    assert torch.equal(raw_crops(dev, sel, size, float(WHITE), black_level=0, cfa='rggb'), raw_crops(dev, sel, size, float(WHITE)))


# ---------------------------------------------------------------- 3. quantise_u8(flip=)
@pytest.mark.parametrize('shape', [(1, 3, 1, 1), (3, 3, 5, 7), (2, 1, 6, 10), (1, 3, 34, 68)], ids=str)
def test_quantise_u8_flip_equals_flipped_quantise(shape):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.utils import util
    n, c, h, w = shape
    x = (torch.rand(shape, generator=torch.Generator().manual_seed(5 + h)) * 1.4 - 0.2).cuda()
    for reverse in (False, True):
        plain = F.quantise_u8(x, reverse)
        for flip in range(4):
            want = _flip_hw(plain, flip, image=True)
            got = F.quantise_u8(x, reverse, flip=flip)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, w, c)
            assert torch.equal(got, want), 'shape %s reverse %s flip %d' % (shape, reverse, flip)
            assert torch.equal(util.tensor2bgr_device(x, reverse, flip=flip), want)
            buf = torch.empty((n, h, w, c), device='cuda', dtype=torch.uint8)
            assert F.quantise_u8(x, reverse, out=buf, flip=flip) is buf and torch.equal(buf, want)


def test_quantise_u8_flip_unaligned_views():
    """input at an odd float and output at an odd byte (W % 4 == 0, so only the alignment keeps it from the vector form)"""
    import reconfigisp_amd.functional as F
    t = torch.rand(2 * 3 * 6 * 8 + 1, generator=torch.Generator().manual_seed(3)) * 1.4 - 0.2
    x = t.cuda()[1:].view(2, 3, 6, 8)
    plain = F.quantise_u8(x.clone(), True)
    for flip in range(1, 4):
        big = torch.full((2 * 6 * 8 * 3 + 8,), 0xA5, device='cuda', dtype=torch.uint8)
        out = big[3:3 + 2 * 6 * 8 * 3].view(2, 6, 8, 3)
        F.quantise_u8(x, True, out=out, flip=flip)
        assert torch.equal(out, _flip_hw(plain, flip, image=True)), flip
        assert (big[:3] == 0xA5).all().item() and (big[3 + out.numel():] == 0xA5).all().item()


# ---------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_output_alone():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    from reconfigisp_amd.codes.data.gpu_input import raw_crops
    lib = L.load()
    n, h, w = 2, 4, 8
    raw = _u16(_raw(n, h, w, WHITE, seed=5))
    out = torch.full((n * h * w * 3 + 16,), 0x5A, device='cuda', dtype=torch.uint8)
    gam = torch.full((n, 1), 0.5).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())

    def serve(black=0, cfa=0, H=h):
        return lib.risp_serve_u8_cfa(p(raw), 1023.0, None, None, None, 0, 1, (C.c_int * 1)(F.OP_GAMMA), L.ptr_array([gam.data_ptr()]),
                                     p(out), 0, n, H, w, black, cfa, F._stream())

    for kw, named in [(dict(cfa=4), b'4'), (dict(cfa=-1), b'-1'), (dict(cfa=7), b'7'), (dict(black=-1), b'-1'),
                      (dict(black=65536), b'65536'), (dict(H=3), b'3')]:
        assert serve(**kw) != 0, '%s was accepted' % kw
        msg = lib.risp_last_error()
        assert b'risp_serve_u8_cfa' in msg and named in msg, msg
    x = torch.rand(1, 3, 4, 4).cuda()
    fout = torch.full((1, 1, 3, 4), -7.0, device='cuda')
    sel = torch.zeros((1, 3), dtype=torch.int32).cuda()
    assert lib.risp_quantise_u8_flip(p(x), p(out), 1, 3, 4, 4, 0, 4, F._stream()) != 0 and b'4' in lib.risp_last_error()
    assert lib.risp_quantise_u8_flip(p(x), p(out), 1, 3, 4, 4, 0, -1, F._stream()) != 0
    assert lib.risp_quantise_u8_flip(p(x), p(out), 1, 2, 4, 4, 0, 1, F._stream()) != 0
    for args in [(3, 4, 1023.0, 0, 2), (4, 3, 1023.0, 0, 1), (4, 4, 1023.0, 0, 4), (4, 4, 1023.0, -1, 0), (4, 4, 1023.0, 65536, 0),
                 (4, 4, 0.0, 0, 1)]:
        ch, cw, div, black, cfa = args
        assert lib.risp_raw_crop_cfa(p(raw), p(fout), p(sel), 1, h, w, ch, cw, div, black, cfa, F._stream()) != 0, args
        assert b'risp_raw_crop_cfa' in lib.risp_last_error()
    # the Python layer refuses the same before it calls anything
    with pytest.raises(ValueError, match='rggb, grbg, gbrg, bggr'):
        F.serve_u8(raw, 1023.0, [], [], out=out[:n * h * w * 3].view(n, h, w, 3), cfa='rgbg')
    for bad in (-1, 65536, 1.5):
        with pytest.raises(ValueError, match='black_level'):
            F.serve_u8(raw, 1023.0, [], [], out=out[:n * h * w * 3].view(n, h, w, 3), black_level=bad)
    with pytest.raises(ValueError, match='flip'):
        F.quantise_u8(x, flip=4)
    with pytest.raises(ValueError, match='even'):
        raw_crops(raw, sel, (3, 4), 1023.0, cfa='gbrg')
    with pytest.raises(ValueError, match='black_level'):
        raw_crops(raw, sel, (4, 4), 1023.0, black_level=1023)
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item() and (fout == -7.0).all().item(), 'a refused call wrote to its output'
    # and the same arguments without the fault are accepted
    assert serve(black=65535, cfa=3) == 0 and serve() == 0
    torch.cuda.synchronize()
    assert not (out[:n * h * w * 3] == 0x5A).all().item() and (out[n * h * w * 3:] == 0x5A).all().item()


# ---------------------------------------------------------------- 5. the pipelines' serve()
HEADLINE = 'Demosaic_01_sRGB_07_11_01_14'            # bench.py ARCH_DENOISE, an OriginUniversal
COMPOSED = 'Demosaic_01_sRGB_07_05_11'               # gray-world behind the bilateral: a whole-image quantity first


def _pipeline(arch, which='OriginUniversal'):
    from reconfigisp_amd.codes.models import networks
    opt = {'network_G': {'which_model_G': which, 'architecture': arch, 'module_path': None,
                         'individual_module_paths': [None] * 8}}
    torch.manual_seed(10)
    return networks.define_G(opt).cuda().eval()


def _serve_oracle(net, raw_i32, white, black, code, reverse=False):
    return _flip_hw(net.serve(_clamped_mirrored(raw_i32, black, code), white - black, reverse_channels=reverse), code,
                    image=True).clone()


@pytest.mark.parametrize('phase', PHASES)
def test_pipeline_serve_headline_is_one_launch(phase):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    net = _pipeline(HEADLINE)
    raw = _raw(3, 34, 68, WHITE, seed=90)
    dev = _u16(raw)
    want = _serve_oracle(net, raw, 1023.0, 64, F.CFA[phase])
    want_rgb = _serve_oracle(net, raw, 1023.0, 64, F.CFA[phase], True)
    assert net.last_serve_route == 'fused'
    L.CALLS = {}
    try:
        got = net.serve(dev, 1023.0, black_level=64, cfa=phase)
        calls = dict(L.CALLS)
    finally:
        L.CALLS = None
    assert net.last_serve_route == 'fused' and calls == {'risp_serve_u8_cfa': 1}, calls
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 34, 68, 3)
    assert torch.equal(got, want)
    assert torch.equal(net.serve(dev, 1023.0, reverse_channels=True, black_level=64, cfa=phase), want_rgb)
    # with out= a warm call allocates nothing
    buf = torch.empty_like(got)
    net.serve(dev, 1023.0, out=buf, black_level=64, cfa=phase)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert net.serve(dev, 1023.0, out=buf, black_level=64, cfa=phase) is buf
    assert torch.cuda.memory_allocated() == before
    assert torch.equal(buf, want)


@pytest.mark.parametrize('phase', PHASES)
def test_pipeline_serve_composed_route(phase):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    net = _pipeline(COMPOSED)
    raw = _raw(3, 34, 68, WHITE, seed=91)
    dev = _u16(raw)
    want = _serve_oracle(net, raw, 1023.0, 64, F.CFA[phase])
    assert net.last_serve_route == 'composed'
    L.CALLS = {}
    try:
        got = net.serve(dev, 1023.0, black_level=64, cfa=phase)
        calls = dict(L.CALLS)
    finally:
        L.CALLS = None
    assert net.last_serve_route == 'composed'
    # the mirror rides on the two passes the route has anyway
    assert calls.get('risp_raw_crop_cfa') == 1 and 'risp_raw_crop' not in calls, calls
    if phase == 'rggb':
        assert calls.get('risp_quantise_u8') == 1 and 'risp_quantise_u8_flip' not in calls, calls
    else:
        assert calls.get('risp_quantise_u8_flip') == 1 and 'risp_quantise_u8' not in calls, calls
    assert torch.equal(got, want)


def test_pipeline_serve_refuses_a_mirrored_odd_axis_and_a_bad_black_level():
    net = _pipeline(COMPOSED)
    odd_h, odd_w = _u16(_raw(1, 33, 68, WHITE, seed=1)), _u16(_raw(1, 34, 67, WHITE, seed=2))
    buf = torch.full((1, 33, 68, 3), 0x5A, device='cuda', dtype=torch.uint8)
    for frame, phase in [(odd_h, 'gbrg'), (odd_h, 'bggr'), (odd_w, 'grbg'), (odd_w, 'bggr')]:
        with pytest.raises(ValueError, match='even'):
            net.serve(frame, 1023.0, cfa=phase, out=buf if frame is odd_h else None)
    for black in (-1, 1023, 2000, 0.5):
        with pytest.raises(ValueError, match='black_level'):
            net.serve(odd_h, 1023.0, black_level=black, out=buf)
    with pytest.raises(ValueError, match='rggb, grbg, gbrg, bggr'):
        net.serve(odd_h, 1023.0, cfa='xtrans', out=buf)
    torch.cuda.synchronize()
    assert (buf == 0x5A).all().item()
    # an odd axis that is not mirrored is no concern of the keywords: the call gets as far as it does without them (this
    # pipeline's nearest demosaic is what refuses an odd mosaic, today as before)
    for kw in (dict(), dict(black_level=64, cfa='grbg')):
        with pytest.raises(ValueError, match='RGGB mosaic with even H, W'):
            net.serve(odd_h, 1023.0, **kw)


def test_isp_model_serve_passes_the_keywords():
    from reconfigisp_amd.codes.models import create_model
    opt = OrderedDict(model='isp', gpu_ids=[0], dist=False, is_train=False,
                      network_G=dict(which_model_G='OriginUniversal', architecture=HEADLINE, module_path=None),
                      path=dict(pretrain_model_G=None, strict_load=True))
    model = create_model(opt)
    raw = _raw(1, 34, 68, WHITE, seed=4)
    want = _serve_oracle(model.netG, raw, 1023.0, 64, 3, True)
    got = model.serve(_u16(raw), 1023.0, reverse_channels=True, black_level=64, cfa='bggr')
    assert model.netG.last_serve_route == 'fused'
    assert torch.equal(got, want)
    assert not torch.equal(got, model.serve(_u16(raw), 1023.0, reverse_channels=True))
