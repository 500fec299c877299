"""GPU: the serving path of the classical pipelines that hold one classical denoiser - uint16 sensor frames in, packed 8-bit
images out, ONE launch (risp_serve_denoise_u8) for a nearest / bilinear / Malvar-He-Cutler demosaic, stages, a bilateral
(window 3), a median (3 x 3) or non-local means (block 3, search 3), and more stages.

The definition of the feature is "the bytes of the composed route", so every comparison is torch.equal and nothing here has
a tolerance.  The oracle is built by hand from the functions that route calls: ``raw_crops`` (black level and phase) ->
``chain_forward`` with the nearest demosaic or ``origin_demosaic`` -> per stage ``chain_forward`` or ``origin_tonemap`` ->
``origin_denoise`` -> stages -> ``quantise_u8`` (un-mirrored), every stage output in fp32.

Shapes (a workgroup owns a 64 x 32 pixel tile and stages it with a ring of 2 rows / 4 columns in LDS; a thread owns a
2 x 4 patch): at 4 x 4 every tap and every ring pixel reflects, on both sides at once; 6 x 12 has an interior patch;
34 x 68 is ragged in both axes and its rings cross the tile borders; 2 x 128 x 64 is a grid of eight tiles, which takes the
XCD-aware order.  Every batch has per-image sigmas / decay that differ, and frames with flat regions (median ties, a
normaliser near 1) beside random ones."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

WHITE = 1023
KINDS = ['nearest', 'bilinear', 'laplacian']
DENOISERS = ['bilateral', 'median', 'fastnlm']
SHAPES = [(3, 4, 4), (1, 6, 12), (2, 34, 68), (2, 128, 64)]


def _frames(n, h, w, seed):
    """(N,H,W) uint16 on the device: random samples below the white level; every odd image (and the only one of a batch of
    one) has its lower right part made of flat 2 x 4 blocks of few levels, and image 2 of a batch of three is constant"""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(0, WHITE, (n, h, w), generator=g, dtype=torch.int32)
    for i in range(n):
        if i % 2 == 1 or n == 1:
            bh, bw = (h // 2 + 1) // 2, (w // 2 + 3) // 4
            blocks = torch.randint(0, 4, (bh, bw), generator=g, dtype=torch.int32) * 300
            flat = blocks.repeat_interleave(2, 0).repeat_interleave(4, 1)[:h - h // 2, :w - w // 2]
            raw[i, h // 2:, w // 2:] = flat
    if n == 3:
        raw[2] = WHITE // 3
    return raw.to(torch.uint16).cuda()


def _denoise_args(name, n):
    """per-image values that differ across the batch, at both ends of the rules' range (p * 99 + 1)"""
    pick = lambda vals: torch.tensor([vals[i % len(vals)] for i in range(n)]).cuda()
    if name == 'bilateral':
        return (3, pick([1.0, 37.5, 100.0]), pick([100.0, 1.0, 12.25]))
    if name == 'median':
        return (3,)
    return (3, 3, pick([1.0, 20.0, 100.0]))


def _origin_params(name, args):
    if name == 'bilateral':
        return {'window_length': 3, 'sigma_color': args[1], 'sigma_space': args[2], 'max_window': 3}
    if name == 'median':
        return {'size': 3}
    return {'block_size': 3, 'search_block': 3, 'decay_factor': args[2], 'max_block': 3, 'max_search': 3}


def _stages(x, ops, params):
    import reconfigisp_amd.functional as F
    for op, p in zip(ops, params):
        if op == F.OP_TONE_CRYSIS:
            x = F.origin_tonemap(x, 'crysisengine', {'lum_adapted': p[:, 0].contiguous()}, (255., 255.))
        elif op == F.OP_TONE_FILMIC:
            x = F.origin_tonemap(x, 'filmic', {'white_point': p[:, 0].contiguous(), 'exposure_bias': p[:, 1].contiguous()}, (255., 255.))
        elif op != F.OP_SKIP:
            x = F.chain_forward(x, [op], [p])[-1]
    return x


def _composed_fp32(dev, kind, pre, pre_params, name, args, post, post_params, black, phase):
    """the composed route by hand, up to the last stage in fp32 (RGGB orientation)"""
    import reconfigisp_amd.functional as F
    import test_gpu_serve_classical as CL
    x = CL._composed_fp32(dev, kind, pre, pre_params, black, phase)
    x = F.origin_denoise(x, name, _origin_params(name, args), (255., 255.))
    return _stages(x, post, post_params)


def _forms():
    import reconfigisp_amd.functional as F
    front, back = [F.OP_WB_MANUAL, F.OP_TONE_FILMIC], [F.OP_GAMMA, F.OP_WB_QUADRATIC]
    return [([], []), (front, []), ([], back), (front, back)]


# ---------------------------------------------------------------- 1. serve_denoise_u8 against the composed route
@pytest.mark.parametrize('name', DENOISERS)
@pytest.mark.parametrize('n,h,w', SHAPES, ids=lambda v: str(v))
def test_serve_denoise_u8_equals_the_composed_route(n, h, w, name):
    import reconfigisp_amd.functional as F
    import test_gpu_serve_cfa as CF
    import test_gpu_serve_classical as CL
    dev = _frames(n, h, w, seed=7 * h + n)
    pars = CL._params(n, 13 * n + h, 0)
    args = _denoise_args(name, n)
    for black in CF.BLACKS:
        divisor = float(WHITE - black)
        for phase in CF.PHASES:
            code = F.CFA[phase]
            for kind in KINDS:
                for pre, post in _forms():
                    pre_p, post_p = [pars[op] for op in pre], [pars[op] for op in post]
                    last = _composed_fp32(dev, kind, pre, pre_p, name, args, post, post_p, black, phase)
                    for reverse in (False, True):
                        want = F.quantise_u8(last, reverse, None, code)
                        got = F.serve_denoise_u8(dev, divisor, kind, pre, pre_p, name, args, post, post_p, reverse,
                                                 black_level=black, cfa=phase)
                        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, w, 3)
                        assert torch.equal(got, want), '%dx%dx%d %s %s %s black %d pre %s post %s reverse %s: %d bytes differ' % (
                            n, h, w, kind, name, phase, black, pre, post, reverse, (got != want).sum().item())


def test_serve_denoise_u8_writes_into_an_aligned_view():
    import reconfigisp_amd.functional as F
    import test_gpu_serve_classical as CL
    n, h, w = 2, 34, 68
    dev = _frames(n, h, w, seed=77)
    pars = CL._params(n, 78, 0)
    pre, post = _forms()[3]
    pre_p, post_p = [pars[op] for op in pre], [pars[op] for op in post]
    args = _denoise_args('fastnlm', n)
    size = n * h * w * 3
    big = torch.full((size + 64,), 0xA5, device='cuda', dtype=torch.uint8)
    out = big[12:12 + size].view(n, h, w, 3)               # 4-byte aligned, neither 8 nor 16
    assert out.data_ptr() % 4 == 0 and out.data_ptr() % 8 != 0
    assert F.serve_denoise_u8(dev, 1023.0, 'laplacian', pre, pre_p, 'fastnlm', args, post, post_p, out=out) is out
    assert torch.equal(out, F.quantise_u8(_composed_fp32(dev, 'laplacian', pre, pre_p, 'fastnlm', args, post, post_p, 0, 'rggb')))
    assert (big[:12] == 0xA5).all().item() and (big[12 + size:] == 0xA5).all().item()
    with pytest.raises(ValueError):
        F.serve_denoise_u8(dev, 1023.0, 'laplacian', pre, pre_p, 'fastnlm', args, post, post_p, out=big[13:13 + size].view(n, h, w, 3))
    with pytest.raises(ValueError, match='bilateral, median, fastnlm'):
        F.serve_denoise_u8(dev, 1023.0, 'laplacian', pre, pre_p, 'bm3d', args, post, post_p)
    with pytest.raises(ValueError, match='nearest, bilinear, laplacian'):
        F.serve_denoise_u8(dev, 1023.0, 'malvar', pre, pre_p, 'fastnlm', args, post, post_p)
    with pytest.raises(ValueError, match='per-image'):
        F.serve_denoise_u8(dev, 1023.0, 'bilinear', pre, pre_p, 'fastnlm', (3, 3, args[2][:1]), post, post_p)
    with pytest.raises(RuntimeError, match='window 5'):    # the sizes are the entry point's rule
        F.serve_denoise_u8(dev, 1023.0, 'bilinear', pre, pre_p, 'bilateral', (5,) + _denoise_args('bilateral', n)[1:], post, post_p)


# ---------------------------------------------------------------- 2. the pipelines' serve(fast_denoise=True)
ARCHS = [('Bayer_02_Demosaic_02_sRGB_07_01', None),            # Skip, bilinear, bilateral, Gamma
         ('Bayer_02_Demosaic_03_sRGB_01_08_13', 'median'),     # Skip, Malvar-He-Cutler, Gamma, median, WbQuadratic
         ('Bayer_02_Demosaic_01_sRGB_11_09_04', None)]         # Skip, nearest, WbManual, non-local means, Filmic


def _net(arch, small):
    import test_gpu_serve_cfa as CF
    net = CF._pipeline(arch)
    if small:                                              # sigmoid(-2.5) = 0.076 < 1 / 7: a 3 x 3 median (the initial 0.5 gives 9 x 9)
        name, = [k for k, _ in net.named_parameters() if small in k]
        with torch.no_grad():
            getattr(net, name).fill_(-2.5)
    return net


@pytest.mark.parametrize('arch,small', ARCHS, ids=lambda v: v if isinstance(v, str) and '_' in v else None)
def test_pipeline_serve_denoise_is_one_launch(arch, small):
    from reconfigisp_amd import lib as L
    net = _net(arch, small)
    dev = _frames(3, 34, 68, seed=90)
    want = net.serve(dev, 1023.0).clone()
    assert net.last_serve_route == 'composed'
    want_rgb = net.serve(dev, 1023.0, reverse_channels=True).clone()
    want_bggr = net.serve(dev, 1023.0, black_level=64, cfa='bggr').clone()
    assert net.last_serve_route == 'composed'
    kept = net.intermediate_results
    L.CALLS = {}
    try:
        got = net.serve(dev, 1023.0, fast_denoise=True)
        calls = dict(L.CALLS)
    finally:
        L.CALLS = None
    assert net.last_serve_route == 'denoise' and calls == {'risp_serve_denoise_u8': 1}, calls
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 34, 68, 3)
    assert torch.equal(got, want)
    assert torch.equal(net.serve(dev, 1023.0, reverse_channels=True, fast_denoise=True), want_rgb)
    assert torch.equal(net.serve(dev, 1023.0, black_level=64, cfa='bggr', fast_denoise=True), want_bggr)
    assert net.last_serve_route == 'denoise'
    # with out= a warm call allocates nothing and leaves intermediate_results alone
    buf = torch.empty_like(got)
    net.serve(dev, 1023.0, out=buf, black_level=64, cfa='bggr', fast_denoise=True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert net.serve(dev, 1023.0, out=buf, black_level=64, cfa='bggr', fast_denoise=True) is buf
    assert torch.cuda.memory_allocated() == before
    assert torch.equal(buf, want_bggr)
    assert net.intermediate_results is kept, 'serve() touched intermediate_results'
    # the default call has not moved
    assert torch.equal(net.serve(dev, 1023.0), want) and net.last_serve_route == 'composed'


def test_pipeline_serve_denoise_is_capturable():
    net = _net(*ARCHS[2])
    a, b = _frames(3, 34, 68, seed=1), _frames(3, 34, 68, seed=2)
    eager_a, eager_b = net.serve(a, 1023.0).clone(), net.serve(b, 1023.0).clone()
    assert net.last_serve_route == 'composed' and not torch.equal(eager_a, eager_b)
    slot, buf = a.clone(), torch.zeros((3, 34, 68, 3), device='cuda', dtype=torch.uint8)
    net.serve(slot, 1023.0, out=buf, fast_denoise=True)    # fills the caches
    buf.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.serve(slot, 1023.0, out=buf, fast_denoise=True)
    assert net.last_serve_route == 'denoise'
    slot.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager_b)


def test_pipeline_serve_denoise_follows_the_parameters():
    net = _net(*ARCHS[0])
    dev = _frames(2, 34, 68, seed=17)
    first = net.serve(dev, 1023.0, fast_denoise=True).clone()
    assert net.last_serve_route == 'denoise'
    name, = [k for k, _ in net.named_parameters() if 'bilateral' in k]
    with torch.no_grad():
        getattr(net, name)[1] = -6.0                       # sigma_color 1.2, in place: the same storage, a new _version
    second = net.serve(dev, 1023.0, fast_denoise=True).clone()
    assert net.last_serve_route == 'denoise' and not torch.equal(first, second), 'a changed sigma did not reach serve()'
    assert torch.equal(second, net.serve(dev, 1023.0)) and net.last_serve_route == 'composed'


def test_isp_model_serve_takes_the_keyword():
    from collections import OrderedDict
    from reconfigisp_amd.codes.models import create_model
    opt = OrderedDict(model='isp', gpu_ids=[0], dist=False, is_train=False,
                      network_G=dict(which_model_G='OriginUniversal', architecture=ARCHS[0][0], module_path=None),
                      path=dict(pretrain_model_G=None, strict_load=True))
    model = create_model(opt)
    dev = _frames(1, 34, 68, seed=4)
    want = model.serve(dev, 1023.0, reverse_channels=True).clone()
    assert model.netG.last_serve_route == 'composed'
    assert torch.equal(model.serve(dev, 1023.0, reverse_channels=True, fast_denoise=True), want)
    assert model.netG.last_serve_route == 'denoise'


# ---------------------------------------------------------------- 3. fallbacks: the call runs as without the keyword
def _serve_lists(names, pars, dev, **kw):
    """('bytes', image, route) or ('raises', type, message) of pipeline_fusion.serve on a module list built by hand"""
    import test_serve_denoise_plan_cpu as P
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    mods = [m.cuda() for m in P.modules(*names)]
    try:
        with torch.no_grad():
            out, route = PF.serve(mods, pars, dev, 1023.0, **kw)
    except (ValueError, RuntimeError) as e:
        return 'raises', type(e), str(e)
    return 'bytes', out.clone(), route


def _same(a, b):
    return a[0] == b[0] and (torch.equal(a[1], b[1]) if a[0] == 'bytes' else a[1] is b[1]) and a[2] == b[2]


@pytest.mark.parametrize('case', ['bilateral window 17 in one image', 'median size 5', 'odd H', 'W % 4 = 2', 'a fused list'])
def test_fallbacks_run_as_without_the_keyword(case):
    n = 2
    u = lambda *s: torch.rand(*s, generator=torch.Generator().manual_seed(len(case))).cuda()
    gam = 0.2 + 0.6 * u(n, 1)
    shape, route = (n, 34, 68), 'composed'
    if case.startswith('bilateral'):
        names, pars = ('bilinear', 'bilateral', 'gamma'), [None, torch.tensor([[0.5, 0.3, 0.7], [1.0, 0.3, 0.7]]).cuda(), gam]
    elif case.startswith('median'):
        names, pars = ('laplacian', 'gamma', 'median'), [None, gam, torch.tensor([[0.2], [0.2]]).cuda()]
    elif case == 'odd H':
        names, pars, shape, route = ('bilinear', 'fastnlm', 'gamma'), [None, 0.9 * u(n, 3), gam], (n, 7, 12), None
    elif case == 'W % 4 = 2':
        names, pars, shape = ('nearest', 'gamma', 'fastnlm'), [None, gam, 0.9 * u(n, 3)], (n, 12, 10)
    else:
        names, pars, route = ('nearest', 'bilateral', 'gamma'), [None, 0.9 * u(n, 3), gam], 'fused'
    dev = _frames(*shape, seed=31)
    plain = _serve_lists(names, pars, dev)
    fast = _serve_lists(names, pars, dev, fast_denoise=True)
    assert _same(plain, fast), (plain, fast)
    if route is None:                                      # a stencil demosaic takes no mosaic of odd height: the same refusal either way
        assert plain[0] == 'raises' or plain[2] == 'composed'
    else:
        assert plain[0] == 'bytes' and plain[2] == route
    # the lists above are the route's but for the one thing named: without it the keyword does take the one launch
    if case != 'a fused list':
        good = list(pars)
        if case.startswith('bilateral'):
            good[1] = torch.tensor([[0.5, 0.3, 0.7], [0.9, 0.3, 0.7]]).cuda()
        elif case.startswith('median'):
            good[2] = torch.tensor([[0.1], [0.1]]).cuda()
        dev = _frames(n, 34, 68, seed=31)
        ok = _serve_lists(names, good, dev, fast_denoise=True)
        assert ok[0] == 'bytes' and ok[2] == 'denoise', ok
        assert _same(_serve_lists(names, good, dev), ok[:2] + ('composed',))


# ---------------------------------------------------------------- 4. refusals through the C ABI
def test_refusals_leave_the_output_alone():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    lib = L.load()
    n, h, w = 2, 4, 8
    raw = _frames(n, h, w, seed=5)
    out = torch.full((n * h * w * 3 + 16,), 0x5A, device='cuda', dtype=torch.uint8)
    gam = torch.full((n, 1), 0.5).cuda()
    fil = torch.tensor([[0.5, 2.0]] * n).cuda()
    sig = torch.tensor([10.0, 20.0]).cuda()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(raw_p=p(raw), divisor=1023.0, demosaic=2, pre=(F.OP_GAMMA,), pre_params=(gam.data_ptr(),), denoise=0, window=3, search=3,
             a=sig, b=sig, post=(F.OP_TONE_FILMIC,), post_params=(fil.data_ptr(),), out_p=p(out), N=n, H=h, W=w, black=0, cfa=0,
             n_pre=None, n_post=None):
        n_pre = len(pre) if n_pre is None else n_pre
        n_post = len(post) if n_post is None else n_post
        return lib.risp_serve_denoise_u8(raw_p, divisor, demosaic, n_pre, (C.c_int * max(1, len(pre)))(*pre),
                                         L.ptr_array(list(pre_params) or [None]), denoise, window, search, p(a), p(b), n_post,
                                         (C.c_int * max(1, len(post)))(*post), L.ptr_array(list(post_params) or [None]), out_p, 0,
                                         N, H, W, black, cfa, F._stream())

    g = gam.data_ptr()
    refused = {
        'demosaic 3': (dict(demosaic=3), b'demosaic 3'), 'demosaic -1': (dict(demosaic=-1), b'demosaic -1'),
        'denoiser 3': (dict(denoise=3), b'denoiser 3'), 'denoiser -1': (dict(denoise=-1), b'denoiser -1'),
        'op 9 in front': (dict(pre=(9,)), b'op 9'), 'op -1 behind': (dict(post=(-1,)), b'op -1'),
        'demosaic in ops': (dict(pre=(F.OP_DEMOSAIC_NEAREST,), pre_params=(None,)), b'op %d' % F.OP_DEMOSAIC_NEAREST),
        'missing parameter block in front': (dict(pre_params=(None,)), b'stage 0 has no parameter block'),
        'missing parameter block behind': (dict(post_params=(None,)), b'stage 1 has no parameter block'),
        'nine stages': (dict(pre=(F.OP_GAMMA,) * 5, pre_params=(g,) * 5, post=(F.OP_GAMMA,) * 4, post_params=(g,) * 4), b'5 + 4'),
        'nine stages in front': (dict(pre=(F.OP_GAMMA,) * 9, pre_params=(g,) * 9, post=(), post_params=()), b'9 + 0'),
        'negative stage count': (dict(n_post=-1), b'-1'),
        'H 2': (dict(H=2), b'H=2'), 'H odd': (dict(H=5), b'H=5'), 'H 0': (dict(H=0), b'H=0'), 'W % 4': (dict(W=6), b'W=6'),
        'W 2': (dict(W=2), b'W=2'), 'N 0': (dict(N=0), b'N=0'), 'N 65536': (dict(N=65536), b'N=65536'),
        'raw at 2 bytes': (dict(raw_p=C.c_void_p(raw.data_ptr() + 2)), b'8-byte'),
        'raw at 4 bytes': (dict(raw_p=C.c_void_p(raw.data_ptr() + 4)), b'8-byte'),
        'out at 1 byte': (dict(out_p=C.c_void_p(out.data_ptr() + 1)), b'4-byte'),
        'null raw': (dict(raw_p=None), b'null'), 'null out': (dict(out_p=None), b'null'),
        'divisor 0': (dict(divisor=0.0), b'divisor'), 'divisor nan': (dict(divisor=float('nan')), b'divisor'),
        'cfa 4': (dict(cfa=4), b'cfa 4'), 'black -1': (dict(black=-1), b'black_level -1'), 'black 65536': (dict(black=65536), b'65536'),
        'bilateral window 5': (dict(window=5), b'window 5'), 'bilateral window 1': (dict(window=1), b'window 1'),
        'bilateral without sigma_color': (dict(a=None), b'sigma'), 'bilateral without sigma_space': (dict(b=None), b'sigma'),
        'median size 5': (dict(denoise=1, window=5), b'size 5'), 'median size 9': (dict(denoise=1, window=9), b'size 9'),
        'nlm block 5': (dict(denoise=2, window=5), b'block 5'), 'nlm search 5': (dict(denoise=2, search=5), b'search 5'),
        'nlm without decay': (dict(denoise=2, a=None), b'decay'),
    }
    for what, (kw, named) in refused.items():
        assert call(**kw) != 0, '%s was accepted' % what
        msg = lib.risp_last_error()
        assert b'risp_serve_denoise_u8' in msg and named in msg, (what, msg)
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item(), 'a refused call wrote to its output'
    # and the same arguments without the fault are accepted (every denoiser; what a denoiser ignores may be anything)
    assert call() == 0 and call(denoise=1, window=3, search=0, a=None, b=None) == 0 and call(denoise=2, b=None, demosaic=0, black=65535, cfa=3) == 0
    assert call(demosaic=1, pre=(), pre_params=(), post=(), post_params=(), H=4, W=4, N=1) == 0
    torch.cuda.synchronize()
    assert not (out[:n * h * w * 3] == 0x5A).all().item() and (out[n * h * w * 3:] == 0x5A).all().item()
