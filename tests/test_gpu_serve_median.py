"""GPU: the serving path of the classical pipelines that hold one median of a learned size above 3 - uint16 sensor frames in,
packed 8-bit images out, ONE launch (risp_serve_median_u8) for a nearest / bilinear / Malvar-He-Cutler demosaic, stages, a
K x K median (K = 5 .. 15) and more stages - and ``serve(fast_median=True)``, which reaches it.

The definition of the feature is "the bytes of the default call", so every comparison is torch.equal / np.array_equal and
nothing here has a tolerance.  The oracle of part 1 is the composed route built by hand from the functions that route calls
(test_gpu_serve_denoise._composed_fp32 with ``origin_denoise(x, 'median', {'size': K}, (255., 255.))`` as the median step);
part 2 is one known answer that passes through none of the project's median kernels.

Shapes (a workgroup owns a 64 x 32 pixel tile and stages it with a ring of K/2 rounded up to even rows and 4 or 8 columns of
packed codes in LDS; a thread owns a 2 x 4 patch): at the smallest legal image of a size every tap and every ring pixel
reflects, on both sides at once; 34 x 68 is ragged with last tiles of 2 rows / 4 columns, thinner than the ring; 70 x 136 is a
3 x 3 tile grid with an interior tile; 2 x 128 x 64 is a grid of eight tiles, which takes the XCD-aware order.  The frames of
test_gpu_serve_denoise._frames have flat regions (ties) and a constant image."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WHITE = 1023
SIZES = [5, 7, 9, 11, 13, 15]
KINDS = ['nearest', 'bilinear', 'laplacian']
SMALLEST = {5: (4, 4), 7: (4, 4), 9: (6, 8), 11: (6, 8), 13: (8, 8), 15: (8, 8)}
SHAPES = ['smallest', (2, 34, 68), (1, 70, 136), (2, 128, 64)]


def _shape(shape, k):
    return (3,) + SMALLEST[k] if shape == 'smallest' else shape


def _forms():
    import test_gpu_serve_denoise as D
    forms = D._forms()
    return [forms[0], forms[3]]                            # ([], []) and (front, back): WbManual, Filmic | Gamma, WbQuadratic


# ---------------------------------------------------------------- 1. serve_median_u8 against the composed route
@pytest.mark.parametrize('k', SIZES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda v: str(v))
def test_serve_median_u8_equals_the_composed_route(shape, k):
    import reconfigisp_amd.functional as F
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as CL
    import test_gpu_serve_denoise as D
    n, h, w = _shape(shape, k)
    dev = D._frames(n, h, w, seed=7 * h + n + k)
    pars = CL._params(n, 13 * n + h, 0)
    for black in CF.BLACKS:
        divisor = float(WHITE - black)
        for phase in CF.PHASES:
            code = F.CFA[phase]
            for kind in KINDS:
                for pre, post in _forms():
                    pre_p, post_p = [pars[op] for op in pre], [pars[op] for op in post]
                    x = CL._composed_fp32(dev, kind, pre, pre_p, black, phase)
                    x = F.origin_denoise(x, 'median', {'size': k}, (255., 255.))
                    last = D._stages(x, post, post_p)
                    for reverse in (False, True):
                        want = F.quantise_u8(last, reverse, None, code)
                        got = F.serve_median_u8(dev, divisor, kind, pre, pre_p, k, post, post_p, reverse, black_level=black,
                                                cfa=phase)
                        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, w, 3)
                        assert torch.equal(got, want), '%dx%dx%d size %d %s %s black %d pre %s post %s reverse %s: %d bytes differ' % (
                            n, h, w, k, kind, phase, black, pre, post, reverse, (got != want).sum().item())


# ---------------------------------------------------------------- 2. a known answer without the project's median kernels
def _numpy_nearest_median(raw, black, div, k):
    """nearest demosaic -> K x K median, no stages, float32 throughout: (N,H,W) integers -> (N,H,W,3) BGR bytes"""
    f32 = np.float32
    s = np.maximum(raw.astype(np.int64) - black, 0).astype(f32)
    v = (s / f32(div)).astype(f32) * f32(255)
    code = np.floor(np.clip(v, f32(0), f32(255)) + f32(0.5)).astype(f32)
    n, h, w = raw.shape
    quad = lambda a: np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)
    r, b = quad(code[:, 0::2, 0::2]), quad(code[:, 1::2, 1::2])
    g = np.empty_like(code)                                # a row takes the green sample of its own mosaic row
    g[:, 0::2] = np.repeat(code[:, 0::2, 1::2], 2, axis=2)
    g[:, 1::2] = np.repeat(code[:, 1::2, 0::2], 2, axis=2)
    img = np.stack([b, g, r], axis=1)                      # (N,3,H,W)
    rad = k // 2
    pad = np.pad(img, ((0, 0), (0, 0), (rad, rad), (rad, rad)), mode='reflect')
    win = np.lib.stride_tricks.sliding_window_view(pad, (k, k), axis=(2, 3)).reshape(n, 3, h, w, k * k)
    med = np.sort(win, axis=-1)[..., (k * k) // 2].astype(f32)
    out = ((med * (f32(1) / f32(255))).astype(f32) * f32(255)).astype(f32)
    return np.trunc(out).astype(np.uint8).transpose(0, 2, 3, 1)


@pytest.mark.parametrize('k', [5, 9, 15])
@pytest.mark.parametrize('n,h,w', [(3, 8, 8), (2, 34, 68)], ids=lambda v: str(v))
def test_nearest_median_known_answer(n, h, w, k):
    import reconfigisp_amd.functional as F
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_denoise as D
    dev = D._frames(n, h, w, seed=3 * k + h)
    raw = dev.cpu().numpy()
    for black in CF.BLACKS:
        want = _numpy_nearest_median(raw, black, WHITE - black, k)
        got = F.serve_median_u8(dev, float(WHITE - black), 'nearest', [], [], k, [], [], black_level=black).cpu().numpy()
        assert np.array_equal(got, want), 'size %d black %d: %d bytes differ' % (k, black, (got != want).sum())


# ---------------------------------------------------------------- 3. the pipelines' serve(fast_median=True)
ARCH = 'Bayer_02_Demosaic_03_sRGB_01_08_13'                # Skip, Malvar-He-Cutler, Gamma, median, WbQuadratic


def _logit_for(k):
    p = ((k - 3) // 2 + 0.5) / 7                           # the middle of the parameter range that gives size k
    return float(np.log(p / (1 - p)))


def _net(k):
    import test_gpu_serve_cfa as CF
    net = CF._pipeline(ARCH)
    name, = [key for key, _ in net.named_parameters() if 'median' in key]
    with torch.no_grad():
        getattr(net, name).fill_(_logit_for(k))
    return net


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


def test_pipeline_serve_median_is_one_launch():
    import raw_packed_reference as RP
    import test_gpu_serve_denoise as D
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    dev = D._frames(3, 34, 68, seed=90)
    packed = torch.from_numpy(RP.pack(dev.cpu().numpy(), 10)).cuda()
    for k in [3] + sorted(PF._MEDIAN_SIZES):
        entry = 'risp_serve_denoise_u8' if k == 3 else 'risp_serve_median_u8'
        net = _net(k)
        want = net.serve(dev, 1023.0).clone()
        assert net.last_serve_route == 'composed'
        want_bggr = net.serve(dev, 1023.0, black_level=64, cfa='bggr').clone()
        want_raw10 = net.serve(packed, 1023.0, raw_format='raw10').clone()
        want_nv12 = net.serve(dev, 1023.0, out_format='nv12').clone()
        assert net.last_serve_route == 'composed'
        kept = net.intermediate_results
        got, calls = _counted(lambda: net.serve(dev, 1023.0, fast_median=True))
        assert net.last_serve_route == 'denoise' and calls == {entry: 1}, (k, calls)
        assert torch.equal(got, want), k
        assert torch.equal(net.serve(dev, 1023.0, black_level=64, cfa='bggr', fast_median=True), want_bggr), k
        got, calls = _counted(lambda: net.serve(packed, 1023.0, raw_format='raw10', fast_median=True))
        assert net.last_serve_route == 'denoise' and net.last_serve_load == 'pass', k
        assert calls == {'risp_raw_unpack': 1, entry: 1}, (k, calls)
        assert torch.equal(got, want_raw10) and torch.equal(want_raw10, want), k
        got, calls = _counted(lambda: net.serve(dev, 1023.0, out_format='nv12', fast_median=True))
        assert net.last_serve_route == 'denoise' and net.last_serve_store == 'pass', k
        assert calls == {entry: 1, 'risp_bgr8_to_nv12': 1}, (k, calls)
        assert torch.equal(got, want_nv12), k
        # with out= a warm call allocates nothing and leaves intermediate_results alone
        buf = torch.empty_like(want)
        net.serve(dev, 1023.0, out=buf, black_level=64, cfa='bggr', fast_median=True)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        assert net.serve(dev, 1023.0, out=buf, black_level=64, cfa='bggr', fast_median=True) is buf
        assert torch.cuda.memory_allocated() == before
        assert torch.equal(buf, want_bggr), k
        assert net.intermediate_results is kept, 'serve() touched intermediate_results'
        # fast_denoise keeps its meaning, and the default call has not moved
        net.serve(dev, 1023.0, fast_denoise=True)
        assert net.last_serve_route == ('denoise' if k == 3 else 'composed')
        assert torch.equal(net.serve(dev, 1023.0), want) and net.last_serve_route == 'composed'


def test_pipeline_serve_median_follows_the_parameter():
    import test_gpu_serve_denoise as D
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    sizes = [3] + sorted(PF._MEDIAN_SIZES)
    net = _net(sizes[0])
    dev = D._frames(2, 34, 68, seed=17)
    first = net.serve(dev, 1023.0, fast_median=True).clone()
    name, = [key for key, _ in net.named_parameters() if 'median' in key]
    with torch.no_grad():
        getattr(net, name).fill_(_logit_for(sizes[-1] if len(sizes) > 1 else 17))    # in place: the same storage, a new _version
    second = net.serve(dev, 1023.0, fast_median=True).clone()
    assert net.last_serve_route == ('denoise' if len(sizes) > 1 else 'composed')
    assert not torch.equal(first, second), 'a changed size did not reach serve()'
    assert torch.equal(second, net.serve(dev, 1023.0)) and net.last_serve_route == 'composed'


def test_isp_model_serve_takes_the_keyword():
    from collections import OrderedDict
    import test_gpu_serve_denoise as D
    from reconfigisp_amd.codes.models import create_model
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    opt = OrderedDict(model='isp', gpu_ids=[0], dist=False, is_train=False,
                      network_G=dict(which_model_G='OriginUniversal', architecture=ARCH, module_path=None),
                      path=dict(pretrain_model_G=None, strict_load=True))
    model = create_model(opt)
    k = max(PF._MEDIAN_SIZES) if PF._MEDIAN_SIZES else 3
    name, = [key for key, _ in model.netG.named_parameters() if 'median' in key]
    with torch.no_grad():
        getattr(model.netG, name).fill_(_logit_for(k))
    dev = D._frames(1, 34, 68, seed=4)
    want = model.serve(dev, 1023.0, reverse_channels=True).clone()
    assert model.netG.last_serve_route == 'composed'
    got, calls = _counted(lambda: model.serve(dev, 1023.0, reverse_channels=True, fast_median=True))
    assert torch.equal(got, want) and model.netG.last_serve_route == 'denoise'
    assert calls == {'risp_serve_denoise_u8' if k == 3 else 'risp_serve_median_u8': 1}, calls


# ---------------------------------------------------------------- 4. fallbacks: the call runs as without the keyword
def _med(size, n=2):
    """an OriginNoiseMedian parameter block whose image 0 gives ``size``; image 1 alone would give 3"""
    p = ((size - 3) // 2 + 0.5) / 7 if size < 17 else 1.0
    return torch.tensor([[p]] + [[0.05]] * (n - 1)).cuda()


def _serve_lists(names, pars, dev, **kw):
    import test_gpu_serve_denoise as D
    out, calls = _counted(lambda: D._serve_lists(names, pars, dev, **kw))
    return out, calls


CASES = ['size 17', 'size 15 on 6 x 8', 'odd H', 'W % 4 = 2', 'a bilateral list', 'two denoisers', 'a size that is not listed']


@pytest.mark.parametrize('case', CASES)
def test_fallbacks_run_as_without_the_keyword(case, monkeypatch):
    import test_gpu_serve_denoise as D
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    n = 2
    gam = 0.2 + 0.6 * torch.rand(n, 1, generator=torch.Generator().manual_seed(len(case))).cuda()
    if case == 'size 15 on 6 x 8':
        # (the geometry rule is about the size, whatever the measurement listed)
        monkeypatch.setattr(PF, '_MEDIAN_SIZES', PF._MEDIAN_SIZES | {15})
    elif case == 'a size that is not listed' and PF._MEDIAN_SIZES >= set(SIZES):
        # every size is listed today: the rule is exercised with the table narrowed by one
        monkeypatch.setattr(PF, '_MEDIAN_SIZES', PF._MEDIAN_SIZES - {11})
    elif not PF._MEDIAN_SIZES:
        monkeypatch.setattr(PF, '_MEDIAN_SIZES', frozenset({9}))
    listed = sorted(PF._MEDIAN_SIZES)
    names = good_names = ('laplacian', 'gamma', 'median')
    pars = good = [None, gam, _med(listed[0])]
    shape = good_shape = (n, 34, 68)
    refusal = False                                        # whether the default call may refuse the frames
    if case == 'size 17':
        pars = [None, gam, _med(17)]
    elif case == 'size 15 on 6 x 8':                       # min(H, W) = 6 is not above the radius 7; 8 x 8 is
        pars = good = [None, gam, _med(15)]
        shape, good_shape, refusal = (n, 6, 8), (n, 8, 8), True
    elif case == 'odd H':                                  # a stencil demosaic takes no mosaic of odd height
        shape, refusal = (n, 7, 12), True
    elif case == 'W % 4 = 2':
        shape = (n, 12, 10)
    elif case == 'a bilateral list':
        names, pars = ('laplacian', 'gamma', 'bilateral'), [None, gam, torch.tensor([[0.5, 0.3, 0.7]] * n).cuda()]
    elif case == 'two denoisers':
        names, pars = ('laplacian', 'median', 'gamma', 'median'), [None, _med(listed[0]), gam, _med(listed[0])]
    else:
        pars = [None, gam, _med([k for k in SIZES if k not in listed][0])]
    dev = D._frames(*shape, seed=31)
    plain, _ = _serve_lists(names, pars, dev)
    fast, calls = _serve_lists(names, pars, dev, fast_median=True)
    assert D._same(plain, fast), (plain, fast)
    assert 'risp_serve_median_u8' not in calls and 'risp_serve_denoise_u8' not in calls, calls
    if refusal:
        assert plain[0] == 'raises' or plain[2] == 'composed', plain
    else:
        assert plain[0] == 'bytes' and plain[2] == 'composed', plain
    # the same list with only the one thing named mended does take the launch
    dev = D._frames(*good_shape, seed=31)
    ok, calls = _serve_lists(good_names, good, dev, fast_median=True)
    assert ok[0] == 'bytes' and ok[2] == 'denoise' and calls == {'risp_serve_median_u8': 1}, (ok, calls)
    assert D._same(_serve_lists(good_names, good, dev)[0], ok[:2] + ('composed',))


def test_a_proxy_list_runs_as_without_the_keyword():
    """IspUniversal builds the differentiable proxies of the same names - CNNs: its list keeps the composed route, and
    OriginUniversal's list of the same architecture takes the launch"""
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_denoise as D
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    dev = D._frames(2, 34, 68, seed=12)
    net = CF._pipeline(ARCH, which='IspUniversal')
    want = net.serve(dev, 1023.0).clone()
    assert net.last_serve_route == 'composed'
    got, calls = _counted(lambda: net.serve(dev, 1023.0, fast_median=True))
    assert net.last_serve_route == 'composed' and torch.equal(got, want)
    assert 'risp_serve_median_u8' not in calls and 'risp_serve_denoise_u8' not in calls, calls
    net = _net(max(PF._MEDIAN_SIZES) if PF._MEDIAN_SIZES else 3)
    net.serve(dev, 1023.0, fast_median=True)
    assert net.last_serve_route == 'denoise'


# ---------------------------------------------------------------- 5. refusals through the C ABI
def test_refusals_leave_the_output_alone():
    import reconfigisp_amd.functional as F
    import test_gpu_serve_denoise as D
    from reconfigisp_amd import lib as L
    lib = L.load()
    n, h, w = 2, 8, 8
    raw = D._frames(n, h, w, seed=5)
    out = torch.full((n * h * w * 3 + 16,), 0x5A, device='cuda', dtype=torch.uint8)
    gam = torch.full((n, 1), 0.5).cuda()
    fil = torch.tensor([[0.5, 2.0]] * n).cuda()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(raw_p=p(raw), divisor=1023.0, demosaic=2, pre=(F.OP_GAMMA,), pre_params=(gam.data_ptr(),), size=5,
             post=(F.OP_TONE_FILMIC,), post_params=(fil.data_ptr(),), out_p=p(out), N=n, H=h, W=w, black=0, cfa=0, n_pre=None,
             n_post=None):
        n_pre = len(pre) if n_pre is None else n_pre
        n_post = len(post) if n_post is None else n_post
        return lib.risp_serve_median_u8(raw_p, divisor, demosaic, n_pre, (C.c_int * max(1, len(pre)))(*pre),
                                        L.ptr_array(list(pre_params) or [None]), size, n_post,
                                        (C.c_int * max(1, len(post)))(*post), L.ptr_array(list(post_params) or [None]), out_p, 0,
                                        N, H, W, black, cfa, F._stream())

    g = gam.data_ptr()
    refused = {
        'size 3': (dict(size=3), b'size 3'), 'size 4': (dict(size=4), b'size 4'), 'size 17': (dict(size=17), b'size 17'),
        'size 6': (dict(size=6), b'size 6'), 'size -5': (dict(size=-5), b'size -5'),
        'H = size / 2': (dict(size=13, H=6), b'H=6'), 'H < size / 2': (dict(size=15, H=4), b'H=4'),
        'W = size / 2': (dict(size=9, W=4), b'W=4'), 'W < size / 2': (dict(size=15, W=4), b'W=4'),
        'H 2': (dict(H=2), b'H=2'), 'H odd': (dict(H=7), b'H=7'), 'H 0': (dict(H=0), b'H=0'), 'W % 4': (dict(W=6), b'W=6'),
        'W 2': (dict(W=2), b'W=2'), 'N 0': (dict(N=0), b'N=0'), 'N 65536': (dict(N=65536), b'N=65536'),
        'demosaic 3': (dict(demosaic=3), b'demosaic 3'), 'demosaic -1': (dict(demosaic=-1), b'demosaic -1'),
        'op 9 in front': (dict(pre=(9,)), b'op 9'), 'op -1 behind': (dict(post=(-1,)), b'op -1'),
        'demosaic in ops': (dict(pre=(F.OP_DEMOSAIC_NEAREST,), pre_params=(None,)), b'op %d' % F.OP_DEMOSAIC_NEAREST),
        'missing parameter block in front': (dict(pre_params=(None,)), b'stage 0 has no parameter block'),
        'missing parameter block behind': (dict(post_params=(None,)), b'stage 1 has no parameter block'),
        'nine stages': (dict(pre=(F.OP_GAMMA,) * 5, pre_params=(g,) * 5, post=(F.OP_GAMMA,) * 4, post_params=(g,) * 4), b'5 + 4'),
        'nine stages in front': (dict(pre=(F.OP_GAMMA,) * 9, pre_params=(g,) * 9, post=(), post_params=()), b'9 + 0'),
        'negative stage count': (dict(n_post=-1), b'-1'),
        'raw at 2 bytes': (dict(raw_p=C.c_void_p(raw.data_ptr() + 2)), b'8-byte'),
        'raw at 4 bytes': (dict(raw_p=C.c_void_p(raw.data_ptr() + 4)), b'8-byte'),
        'out at 1 byte': (dict(out_p=C.c_void_p(out.data_ptr() + 1)), b'4-byte'),
        'null raw': (dict(raw_p=None), b'null'), 'null out': (dict(out_p=None), b'null'),
        'divisor 0': (dict(divisor=0.0), b'divisor'), 'divisor nan': (dict(divisor=float('nan')), b'divisor'),
        'cfa 4': (dict(cfa=4), b'cfa 4'), 'black -1': (dict(black=-1), b'black_level -1'), 'black 65536': (dict(black=65536), b'65536'),
    }
    for what, (kw, named) in refused.items():
        assert call(**kw) != 0, '%s was accepted' % what
        msg = lib.risp_last_error()
        assert b'risp_serve_median_u8' in msg and named in msg, (what, msg)
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item(), 'a refused call wrote to its output'
    # the wrapper refuses the sizes on the host, and the 3 x 3 entry point keeps refusing the large ones
    with pytest.raises(ValueError, match='median size 3'):
        F.serve_median_u8(raw, 1023.0, 'bilinear', [], [], 3, [], [])
    with pytest.raises(ValueError, match='median size 17'):
        F.serve_median_u8(raw, 1023.0, 'bilinear', [], [], 17, [], [])
    with pytest.raises(RuntimeError, match='H=8'):
        F.serve_median_u8(raw[:, :, :4].contiguous(), 1023.0, 'bilinear', [], [], 9, [], [])
    # a good call returns 0 and writes only its own bytes: a 4-byte aligned view with guard bytes around it
    size = n * h * w * 3
    view = out[12:12 + size]
    assert view.data_ptr() % 4 == 0 and view.data_ptr() % 8 != 0
    assert call(out_p=p(view), size=15, black=65535 - 1, cfa=3, demosaic=0) == 0
    assert call(out_p=p(view)) == 0
    torch.cuda.synchronize()
    assert not (view == 0x5A).all().item() and (out[:12] == 0x5A).all().item() and (out[12 + size:] == 0x5A).all().item()
    want = F.serve_median_u8(raw, 1023.0, 'laplacian', [F.OP_GAMMA], [gam], 5, [F.OP_TONE_FILMIC], [fil])
    assert torch.equal(view.view(n, h, w, 3), want)
