"""GPU: the classical pipelines' serving path - uint16 sensor frames in, packed 8-bit images out, ONE launch for the
nearest, the bilinear and the Malvar-He-Cutler demosaic followed by element-wise stages and Crysis / Filmic tone curves.

The definition of the feature is "the bytes of the composed route", so every comparison is torch.equal and nothing here has
a tolerance.  The oracle is built by hand from the functions that route calls: ``raw_crops`` (black level and phase) ->
``chain_forward`` with the nearest demosaic or ``origin_demosaic`` -> per stage ``chain_forward`` or ``origin_tonemap``,
every stage output in fp32 -> ``quantise_u8`` (un-mirrored).

Shapes (a thread owns a 2 x 4 patch and reads mosaic rows py-2 .. py+3, columns px-2 .. px+5; a workgroup owns a 64 x 32
pixel tile): at 4 x 4 every tap outside the patch reflects, 4 x 8 has a left and a right border patch, 6 x 12 is the first
size with an interior patch in the Laplacian form, 34 x 68 crosses the tile both ways, and 8 x 32 x 64 is a grid of eight
tiles, which takes the XCD-aware order."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

WHITE = 1023
KINDS = ['nearest', 'bilinear', 'laplacian']
SHAPES = [(1, 4, 4), (3, 4, 4), (1, 4, 8), (3, 6, 12), (3, 34, 68), (8, 32, 64)]


def _op_lists():
    import reconfigisp_amd.functional as F
    WB, GA, GT, WQ, G3, CR, FI = (F.OP_WB_MANUAL, F.OP_GAMMA, F.OP_GTM_MANUAL, F.OP_WB_QUADRATIC, F.OP_GAIN3, F.OP_TONE_CRYSIS,
                                  F.OP_TONE_FILMIC)
    return [[], [CR], [WB, FI, GA], [WQ, WB, CR, GA, GT, FI, G3, GA], [F.OP_SKIP, FI, F.OP_SKIP]]


def _params(n, seed, shift):
    """per-image parameter blocks by op code.  The tone curves' draws go through their edges: lum_adapted 0 and 1; white_point
    0 and 0.005 (both below the 0.01 floor) and 1; exposure_bias 1 and 10 - image i of draw ``shift`` takes entry i + shift"""
    import reconfigisp_amd.functional as F
    import test_gpu_serve_cfa as CF
    pars = CF._chain_params(n, seed)
    g = torch.Generator().manual_seed(seed + 1)
    r = lambda: torch.rand(1, generator=g).item()
    pick = lambda vals: torch.tensor([vals[(i + shift) % len(vals)] for i in range(n)])
    lum = pick([0.0, 1.0, r(), r()])
    wp = pick([0.0, 0.005, 1.0, r()])
    bias = pick([1.0, 10.0, 1.0 + 9.0 * r(), 1.0 + 9.0 * r()])
    pars[F.OP_TONE_CRYSIS] = lum[:, None].contiguous().cuda()
    pars[F.OP_TONE_FILMIC] = torch.stack([wp, bias], dim=1).contiguous().cuda()
    pars[F.OP_SKIP] = None
    return pars


def _composed_fp32(dev, kind, ops, params, black, phase):
    """the composed route by hand, up to the last stage in fp32 (RGGB orientation)"""
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.data.gpu_input import raw_crops
    n, h, w = dev.shape
    sel = torch.tensor([[i, 0, 0] for i in range(n)], dtype=torch.int32)
    x = raw_crops(dev, sel, (h, w), float(WHITE), black, phase)
    if kind == 'nearest':
        x = F.chain_forward(x, [F.OP_DEMOSAIC_NEAREST], [None])[-1]
    else:
        x = F.origin_demosaic(x, kind, (255., 255.))
    for op, p in zip(ops, params):
        if op == F.OP_TONE_CRYSIS:
            x = F.origin_tonemap(x, 'crysisengine', {'lum_adapted': p[:, 0].contiguous()}, (255., 255.))
        elif op == F.OP_TONE_FILMIC:
            x = F.origin_tonemap(x, 'filmic', {'white_point': p[:, 0].contiguous(), 'exposure_bias': p[:, 1].contiguous()},
                                 (255., 255.))
        elif op != F.OP_SKIP:
            x = F.chain_forward(x, [op], [p])[-1]
    return x


# ---------------------------------------------------------------- 1. serve_classical_u8 against the composed route
@pytest.mark.parametrize('n,h,w', SHAPES, ids=lambda v: str(v))
def test_serve_classical_u8_equals_the_composed_route(n, h, w):
    import reconfigisp_amd.functional as F
    import test_gpu_serve_cfa as CF
    dev = CF._u16(CF._raw(n, h, w, WHITE, seed=3 * h + n))
    for shift in range(3 if n == 1 else 1):                # one image per draw: three draws reach every edge value
        pars = _params(n, 11 * n + h, shift)
        for black in CF.BLACKS:
            divisor = float(WHITE - black)
            for phase in CF.PHASES:
                code = F.CFA[phase]
                for kind in KINDS:
                    for ops in _op_lists():
                        params = [pars[op] for op in ops]
                        last = _composed_fp32(dev, kind, ops, params, black, phase)
                        for reverse in (False, True):
                            want = F.quantise_u8(last, reverse, None, code)
                            got = F.serve_classical_u8(dev, divisor, kind, ops, params, reverse, black_level=black, cfa=phase)
                            assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, w, 3)
                            assert torch.equal(got, want), '%dx%dx%d %s %s black %d ops %s reverse %s draw %d: %d bytes differ' % (
                                n, h, w, kind, phase, black, ops, reverse, shift, (got != want).sum().item())


def test_serve_classical_u8_nearest_gives_serve_u8_bytes():
    """without a tone curve the nearest form is risp_serve_u8[_cfa]'s pipeline: the same bytes from both entry points"""
    import reconfigisp_amd.functional as F
    import test_gpu_serve_cfa as CF
    n, h, w = 3, 34, 68
    dev = CF._u16(CF._raw(n, h, w, WHITE, seed=12))
    pars = CF._chain_params(n, 13)
    for ops in CF._tails():
        params = [pars[op] for op in ops]
        for black, phase in ((0, 'rggb'), (64, 'grbg')):
            want = F.serve_u8(dev, float(WHITE - black), ops, params, None, black_level=black, cfa=phase)
            assert torch.equal(F.serve_classical_u8(dev, float(WHITE - black), 'nearest', ops, params, black_level=black, cfa=phase), want)


def test_serve_classical_u8_writes_into_an_aligned_view():
    import reconfigisp_amd.functional as F
    import test_gpu_serve_cfa as CF
    n, h, w = 3, 34, 68
    dev = CF._u16(CF._raw(n, h, w, WHITE, seed=77))
    pars = _params(n, 78, 0)
    ops = [F.OP_WB_MANUAL, F.OP_TONE_FILMIC, F.OP_GAMMA]
    params = [pars[op] for op in ops]
    size = n * h * w * 3
    big = torch.full((size + 64,), 0xA5, device='cuda', dtype=torch.uint8)
    out = big[12:12 + size].view(n, h, w, 3)               # 4-byte aligned, neither 8 nor 16
    assert out.data_ptr() % 4 == 0 and out.data_ptr() % 8 != 0
    assert F.serve_classical_u8(dev, 1023.0, 'laplacian', ops, params, out=out) is out
    assert torch.equal(out, F.quantise_u8(_composed_fp32(dev, 'laplacian', ops, params, 0, 'rggb')))
    assert (big[:12] == 0xA5).all().item() and (big[12 + size:] == 0xA5).all().item()
    with pytest.raises(ValueError):
        F.serve_classical_u8(dev, 1023.0, 'laplacian', ops, params, out=big[13:13 + size].view(n, h, w, 3))
    with pytest.raises(ValueError, match='nearest, bilinear, laplacian'):
        F.serve_classical_u8(dev, 1023.0, 'malvar', ops, params)
    with pytest.raises(ValueError, match='black_level'):
        F.serve_classical_u8(dev, 1023.0, 'bilinear', ops, params, black_level=65536)
    with pytest.raises(ValueError, match='rggb, grbg, gbrg, bggr'):
        F.serve_classical_u8(dev, 1023.0, 'bilinear', ops, params, cfa='rgbg')


# ---------------------------------------------------------------- 2. refusals through the C ABI
def test_refusals_leave_the_output_alone():
    import reconfigisp_amd.functional as F
    import test_gpu_serve_cfa as CF
    from reconfigisp_amd import lib as L
    lib = L.load()
    n, h, w = 2, 4, 8
    raw = CF._u16(CF._raw(n, h, w, WHITE, seed=5))
    out = torch.full((n * h * w * 3 + 16,), 0x5A, device='cuda', dtype=torch.uint8)
    gam = torch.full((n, 1), 0.5).cuda()
    fil = torch.tensor([[0.5, 2.0]] * n).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(raw_p=p(raw), divisor=1023.0, demosaic=2, ops=(F.OP_GAMMA, F.OP_TONE_FILMIC), params=(gam.data_ptr(), fil.data_ptr()),
             out_p=p(out), N=n, H=h, W=w, black=0, cfa=0, n_ops=None):
        n_ops = len(ops) if n_ops is None else n_ops
        return lib.risp_serve_classical_u8(raw_p, divisor, demosaic, n_ops, (C.c_int * max(1, len(ops)))(*ops),
                                           L.ptr_array(list(params) or [None]), out_p, 0, N, H, W, black, cfa, F._stream())

    refused = {
        'demosaic 3': dict(demosaic=3), 'demosaic -1': dict(demosaic=-1),
        'op 9': dict(ops=(9,), params=(gam.data_ptr(),)), 'op -1': dict(ops=(-1,), params=(gam.data_ptr(),)),
        'demosaic in ops': dict(ops=(F.OP_DEMOSAIC_NEAREST,), params=(None,)),
        'missing parameter block': dict(ops=(F.OP_TONE_CRYSIS,), params=(None,)),
        'nine stages': dict(ops=(F.OP_GAMMA,) * 9, params=(gam.data_ptr(),) * 9), 'negative stage count': dict(n_ops=-1),
        'H 2': dict(H=2), 'H odd': dict(H=5), 'H 0': dict(H=0), 'W % 4': dict(W=6), 'W 2': dict(W=2), 'W 0': dict(W=0),
        'N 0': dict(N=0), 'N 65536': dict(N=65536),
        'raw at 2 bytes': dict(raw_p=C.c_void_p(raw.data_ptr() + 2)), 'raw at 4 bytes': dict(raw_p=C.c_void_p(raw.data_ptr() + 4)),
        'out at 1 byte': dict(out_p=C.c_void_p(out.data_ptr() + 1)), 'null raw': dict(raw_p=None), 'null out': dict(out_p=None),
        'divisor 0': dict(divisor=0.0), 'divisor nan': dict(divisor=float('nan')),
        'cfa 4': dict(cfa=4), 'cfa -1': dict(cfa=-1), 'black -1': dict(black=-1), 'black 65536': dict(black=65536),
    }
    for what, kw in refused.items():
        assert call(**kw) != 0, '%s was accepted' % what
        assert b'risp_serve_classical_u8' in lib.risp_last_error(), what
    # the tone codes belong to this entry point alone
    x = torch.rand(n, 3, h, w).cuda()
    y = torch.full((n, 3, h, w), -7.0, device='cuda')
    for op in (F.OP_TONE_CRYSIS, F.OP_TONE_FILMIC):
        one, blk = (C.c_int * 1)(op), L.ptr_array([fil.data_ptr()])
        assert lib.risp_serve_u8(p(raw), 1023.0, None, None, None, 0, 1, one, blk, p(out), 0, n, h, w, F._stream()) != 0
        assert b'risp_serve_u8' in lib.risp_last_error()
        assert lib.risp_serve_u8_cfa(p(raw), 1023.0, None, None, None, 0, 1, one, blk, p(out), 0, n, h, w, 0, 0, F._stream()) != 0
        assert lib.risp_chain_fwd(p(x), 1, one, blk, L.ptr_array([y.data_ptr()]), n, h, w, F._stream()) != 0
        assert b'risp_chain_fwd' in lib.risp_last_error()
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item() and (y == -7.0).all().item(), 'a refused call wrote to its output'
    # and the same arguments without the fault are accepted (every demosaic kind, black level and phase at their ends, no stage)
    assert call() == 0 and call(demosaic=0, black=65535, cfa=3) == 0 and call(demosaic=1, ops=(), params=()) == 0
    assert call(H=4, W=4, N=1) == 0
    torch.cuda.synchronize()
    assert not (out[:n * h * w * 3] == 0x5A).all().item() and (out[n * h * w * 3:] == 0x5A).all().item()


# ---------------------------------------------------------------- 3. the pipelines' serve()
ARCHS = ['Demosaic_02_sRGB_11_01_14',            # bilinear, WbManual, Gamma, GtmManual
         'Demosaic_03_sRGB_11_04_01',            # Malvar-He-Cutler, WbManual, Filmic, Gamma
         'Demosaic_03_sRGB_13_10_03_01',         # Malvar-He-Cutler, WbQuadratic, Skip, Crysis, Gamma
         'Demosaic_01_sRGB_03_01']               # nearest, Crysis, Gamma


def _composed(monkeypatch):
    """within the returned context serve() takes the composed route for every pipeline that is not 'fused'"""
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    ctx = monkeypatch.context()
    m = ctx.__enter__()
    m.setattr(PF, 'serve_route', lambda modules: 'composed')
    return ctx


@pytest.mark.parametrize('arch', ARCHS)
def test_pipeline_serve_classical_is_one_launch(arch, monkeypatch):
    import test_gpu_serve_cfa as CF
    from reconfigisp_amd import lib as L
    net = CF._pipeline(arch)
    raw = CF._raw(3, 34, 68, WHITE, seed=90)
    dev = CF._u16(raw)
    ctx = _composed(monkeypatch)
    try:                                                   # every reference first, on the composed route
        want = net.serve(dev, 1023.0).clone()
        assert net.last_serve_route == 'composed'
        want_rgb = net.serve(dev, 1023.0, reverse_channels=True).clone()
        want_bggr = CF._serve_oracle(net, raw, 1023.0, 64, 3)
        assert net.last_serve_route == 'composed'
    finally:
        ctx.__exit__(None, None, None)
    kept = net.intermediate_results
    L.CALLS = {}
    try:
        got = net.serve(dev, 1023.0)
        calls = dict(L.CALLS)
    finally:
        L.CALLS = None
    assert net.last_serve_route == 'classical' and calls == {'risp_serve_classical_u8': 1}, calls
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 34, 68, 3)
    assert torch.equal(got, want)
    assert torch.equal(net.serve(dev, 1023.0, reverse_channels=True), want_rgb)
    assert torch.equal(net.serve(dev, 1023.0, black_level=64, cfa='bggr'), want_bggr) and net.last_serve_route == 'classical'
    # with out= a warm call allocates nothing and leaves intermediate_results alone
    buf = torch.empty_like(got)
    net.serve(dev, 1023.0, out=buf, black_level=64, cfa='bggr')
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert net.serve(dev, 1023.0, out=buf, black_level=64, cfa='bggr') is buf
    assert torch.cuda.memory_allocated() == before
    assert torch.equal(buf, want_bggr)
    assert net.intermediate_results is kept, 'serve() touched intermediate_results'


def test_pipeline_serve_follows_the_filmic_parameter(monkeypatch):
    import test_gpu_serve_cfa as CF
    net = CF._pipeline('Demosaic_03_sRGB_11_04_01')
    dev = CF._u16(CF._raw(3, 34, 68, WHITE, seed=17))
    first = net.serve(dev, 1023.0).clone()
    assert net.last_serve_route == 'classical'
    name, = [k for k, _ in net.named_parameters() if 'filmic' in k]
    with torch.no_grad():
        getattr(net, name).copy_(torch.tensor([2.0, -1.5]))     # in place: the same storage, a new _version
    second = net.serve(dev, 1023.0).clone()
    assert net.last_serve_route == 'classical'
    assert not torch.equal(first, second), 'a changed Filmic parameter did not reach serve()'
    ctx = _composed(monkeypatch)
    try:
        want = net.serve(dev, 1023.0)
        assert net.last_serve_route == 'composed'
    finally:
        ctx.__exit__(None, None, None)
    assert torch.equal(second, want)


@pytest.mark.parametrize('arch,route,calls', [
    ('Demosaic_02_sRGB_07_01', 'composed', None),                              # a bilateral behind the bilinear demosaic
    ('Demosaic_02_sRGB_02_01', 'composed', None),                              # Reinhard: the log-average luminance first
    ('Demosaic_01_sRGB_07_11_01_14', 'fused', {'risp_serve_u8': 1}),           # the headline keeps its launch
], ids=lambda v: v if isinstance(v, str) and '_' in v else None)
def test_routes_that_do_not_move(arch, route, calls):
    import test_gpu_serve as S
    import test_gpu_serve_cfa as CF
    from reconfigisp_amd import lib as L
    net = CF._pipeline(arch)
    raw = CF._u16(CF._raw(3, 34, 68, WHITE, seed=len(arch)))
    want = S._forward_bytes(net, raw, 1023.0)
    L.CALLS = {}
    try:
        got = net.serve(raw, 1023.0)
        seen = dict(L.CALLS)
    finally:
        L.CALLS = None
    assert net.last_serve_route == route
    assert 'risp_serve_classical_u8' not in seen and (calls is None or seen == calls), seen
    assert torch.equal(got.cpu(), want)
