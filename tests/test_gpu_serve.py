"""GPU: the serving path - uint16 RGGB frames in, packed 8-bit images out.

Every comparison is torch.equal on bytes; nothing here has a tolerance.  The references are the existing routes:
``util.tensor2bgr`` on the host for the conversion, and for the one launch ``raw_crops`` on whole frames, then
``chain_forward`` / ``BilateralChainPlan`` (every stage output in fp32), then ``tensor2bgr`` of the last stage, image by
image (the host function converts image 0 of a batch).

The one launch keeps the quad form's geometry: a thread owns a 2 x 4 pixel patch, a workgroup a 64 x 32 pixel tile, and a
tile count that is a multiple of 8 takes the XCD-aware order.  Shapes: one patch (2 x 4), 4 x 8, 6 x 12 and 34 x 68, which
crosses the tile in both directions - with N = 4 that is 16 tiles (remapped order), with N = 3 it is 12 (plain order)."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(2, 4), (4, 8), (6, 12), (34, 68)]
BATCHES = [1, 3, 4]
DEPTHS = [(1023, 1023.0), (16383, 16383.0)]          # (white level of the samples, divisor)


def _host_bytes(t, reverse):
    """tensor2bgr image by image -> (N,H,W,C) uint8 tensor; the RGB reference is the host array flipped"""
    from reconfigisp_amd.codes.utils import util
    imgs = [util.tensor2bgr(t[i:i + 1]) for i in range(t.shape[0])]
    imgs = [np.ascontiguousarray(im[..., ::-1]) if reverse else im for im in imgs]
    return torch.from_numpy(np.stack(imgs))


# ---------------------------------------------------------------- 1. quantise_u8 against tensor2bgr
def _quantise_values(shape, seed):
    n, c, h, w = shape
    count = n * c * h * w
    g = torch.Generator().manual_seed(seed)
    v = (torch.rand(count, generator=g) * 1.4 - 0.2).numpy()                     # uniform in [-0.2, 1.2]
    k = (np.arange(256, dtype=np.float32) / np.float32(255))
    special = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)),
                              np.array([0.0, 1.0, -0.0, 3.5e6, -3.5e6, 1e30, -1e30], np.float32)]).astype(np.float32)
    return v, special


@pytest.mark.parametrize('shape', [(1, 3, 1, 1), (3, 3, 5, 7), (2, 1, 6, 10), (1, 3, 34, 68)], ids=str)
def test_quantise_u8_equals_tensor2bgr(shape):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.utils import util
    n, c, h, w = shape
    count = n * c * h * w
    uniform, special = _quantise_values(shape, 5 + h)
    tensors = [torch.from_numpy(uniform.copy()).view(shape)]
    for start in range(0, special.size, count):            # every special value, in as many tensors as the shape needs
        chunk = special[start:start + count]
        t = uniform.copy()
        t[:chunk.size] = chunk
        tensors.append(torch.from_numpy(t[np.random.RandomState(7).permutation(count)]).view(shape))     # spread over the planes
    for t in tensors:
        x = t.cuda()
        for reverse in (False, True):
            got = F.quantise_u8(x, reverse_channels=reverse)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, w, c) and got.is_cuda
            assert torch.equal(got.cpu(), _host_bytes(t, reverse)), 'shape %s reverse %s' % (shape, reverse)
            assert torch.equal(util.tensor2bgr_device(x, reverse), got)
    # a (C,H,W) tensor is a batch of one; an out= buffer is filled in place
    x = tensors[0].cuda()
    assert torch.equal(util.tensor2bgr_device(x[0]), F.quantise_u8(x[:1]))
    buf = torch.empty((n, h, w, c), device='cuda', dtype=torch.uint8)
    assert F.quantise_u8(x, out=buf) is buf and torch.equal(buf.cpu(), _host_bytes(tensors[0], False))


def test_quantise_u8_unaligned_views():
    """input at an odd float and output at an odd byte: the one-byte-per-thread form, same bytes"""
    import reconfigisp_amd.functional as F
    t = torch.rand(2 * 3 * 6 * 8 + 1, generator=torch.Generator().manual_seed(3)) * 1.4 - 0.2
    x = t.cuda()[1:].view(2, 3, 6, 8)
    big = torch.full((2 * 6 * 8 * 3 + 8,), 0xA5, device='cuda', dtype=torch.uint8)
    out = big[3:3 + 2 * 6 * 8 * 3].view(2, 6, 8, 3)
    F.quantise_u8(x, True, out=out)
    assert torch.equal(out.cpu(), _host_bytes(t[1:].view(2, 3, 6, 8), True))
    assert (big[:3] == 0xA5).all().item() and (big[3 + out.numel():] == 0xA5).all().item()


# ---------------------------------------------------------------- 2. serve_u8 against the existing route
def _raw(n, h, w, white, seed):
    """(N,H,W) uint16: samples up to 10 % above the white level; image 1 all zero and image 2 constant where the batch has them"""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(0, int(white * 1.1) + 1, (n, h, w), generator=g, dtype=torch.int32)
    raw[0, 0, 0] = int(white * 1.1)                       # at least one sample above the white level
    if n > 1:
        raw[1] = 0
    if n > 2:
        raw[2] = white // 3
    return raw.to(torch.uint16)


def _chain_params(n, seed):
    import reconfigisp_amd.functional as F
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    return {F.OP_WB_MANUAL: (u(n, 3) * 5).cuda(), F.OP_GAMMA: (0.2 + 0.6 * u(n, 1)).cuda(),
            F.OP_GTM_MANUAL: torch.sort(u(n, 3), dim=1).values.cuda(), F.OP_WB_QUADRATIC: (0.45 + 0.1 * u(n, 30)).cuda(),
            F.OP_GAIN3: (0.5 + 1.5 * u(n, 3)).cuda(), F.OP_SKIP: None}


def _chains():
    import reconfigisp_amd.functional as F
    S, WB, GA, GT, WQ, G3 = F.OP_SKIP, F.OP_WB_MANUAL, F.OP_GAMMA, F.OP_GTM_MANUAL, F.OP_WB_QUADRATIC, F.OP_GAIN3
    return [[], [S], [WB], [GA], [GT], [WQ], [G3],
            [WB, GA, GT],                                  # the headline tail: the instance without WbQuadratic
            [WQ, WB, GA, GT, G3],                          # the five ops: the instance with it
            [GA, WB, GA, GT, G3, WB, GT, GA],              # eight stages with repeats
            [S, WB, S, GA, S]]                             # SKIP at the front, in the middle and at the end


SIGMAS = [0.05, 10.0, 100.0]


def _stage_forms(n):
    """None = no bilateral; else (window per image, sigma_color, sigma_space, max_window)"""
    sc = torch.tensor([SIGMAS[i % 3] for i in range(n)]).cuda()
    ss = torch.tensor([SIGMAS[(i + 1) % 3] for i in range(n)]).cuda()
    mixed = torch.tensor([(3, 1, 3, 1)[i % 4] for i in range(n)], dtype=torch.int32).cuda()
    ones = torch.ones(n, dtype=torch.int32).cuda()
    return [None, (mixed, sc, ss, 3), (ones, ss, sc, 1)]


def _existing_route(raw, divisor, bilateral, ops, params):
    """raw_crops on whole frames -> chain_forward / BilateralChainPlan -> the last stage in fp32"""
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.data.gpu_input import raw_crops
    n, h, w = raw.shape
    sel = torch.tensor([[i, 0, 0] for i in range(n)], dtype=torch.int32)
    x = raw_crops(raw, sel, (h, w), divisor)
    if bilateral is None:
        # (a launch takes RISP_MAX_CHAIN = 8 stages, the demosaic included: a longer chain continues in a second launch, as
        # fused_forward cuts it)
        x = F.chain_forward(x, [F.OP_DEMOSAIC_NEAREST] + ops[:7], [None] + params[:7])[-1]
        return F.chain_forward(x, ops[7:], params[7:])[-1] if ops[7:] else x
    win, sc, ss, wmax = bilateral
    return F.BilateralChainPlan(x, True, win, sc, ss, wmax, ops, params).launch()[-1]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_serve_u8_equals_existing_route(shape):
    import reconfigisp_amd.functional as F
    h, w = shape
    chains = _chains()
    for n in BATCHES:
        pars = _chain_params(n, 11 * n + h)
        forms = _stage_forms(n)
        for white, divisor in DEPTHS:
            raw = _raw(n, h, w, white, seed=white + n + w).cuda()
            for form in forms:
                for ops in chains:
                    params = [pars[op] for op in ops]
                    last = _existing_route(raw, divisor, form, ops, params)
                    for reverse in (False, True):
                        got = F.serve_u8(raw, divisor, ops, params, form, reverse)
                        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, w, 3)
                        want = _host_bytes(last, reverse)
                        assert torch.equal(got.cpu(), want), '%dx%dx%d white %d window %s ops %s reverse %s: %d bytes differ' % (
                            n, h, w, white, form and form[3], ops, reverse, (got.cpu() != want).sum().item())


def test_serve_u8_writes_into_an_aligned_view():
    import reconfigisp_amd.functional as F
    n, h, w = 3, 34, 68
    raw = _raw(n, h, w, 1023, seed=77).cuda()
    pars = _chain_params(n, 78)
    ops = [F.OP_WB_MANUAL, F.OP_GAMMA, F.OP_GTM_MANUAL]
    params = [pars[op] for op in ops]
    form = _stage_forms(n)[1]
    size = n * h * w * 3
    big = torch.full((size + 64,), 0xA5, device='cuda', dtype=torch.uint8)
    out = big[12:12 + size].view(n, h, w, 3)               # 4-byte aligned, neither 8 nor 16
    assert out.data_ptr() % 4 == 0 and out.data_ptr() % 8 != 0
    assert F.serve_u8(raw, 1023.0, ops, params, form, out=out) is out
    assert torch.equal(out.cpu(), _host_bytes(_existing_route(raw, 1023.0, form, ops, params), False))
    assert (big[:12] == 0xA5).all().item() and (big[12 + size:] == 0xA5).all().item()
    with pytest.raises(ValueError):
        F.serve_u8(raw, 1023.0, ops, params, form, out=big[13:13 + size].view(n, h, w, 3))


# ---------------------------------------------------------------- 3. refusals through the C ABI
def test_serve_u8_refusals_leave_the_output_alone():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    fn = L.load().risp_serve_u8
    n, h, w = 2, 4, 8
    raw = _raw(n, h, w, 1023, seed=5).cuda()
    out = torch.full((n * h * w * 3 + 16,), 0x5A, device='cuda', dtype=torch.uint8)
    win = torch.full((n,), 3, dtype=torch.int32).cuda()
    sig = torch.full((n,), 10.0).cuda()
    gam = torch.full((n, 1), 0.5).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(raw_p=p(raw), divisor=1023.0, bil=(p(win), p(sig), p(sig)), wmax=3, ops=(F.OP_GAMMA,), params=(gam.data_ptr(),),
             out_p=p(out), N=n, H=h, W=w, n_ops=None):
        n_ops = len(ops) if n_ops is None else n_ops
        return fn(raw_p, divisor, *bil, wmax, n_ops, (C.c_int * max(1, len(ops)))(*ops), L.ptr_array(list(params) or [None]),
                  out_p, 0, N, H, W, F._stream())

    none3 = (None, None, None)
    refused = {
        'max_window 2': dict(wmax=2), 'max_window 5': dict(wmax=5), 'max_window -1': dict(wmax=-1), 'max_window 17': dict(wmax=17),
        'divisor 0': dict(divisor=0.0), 'divisor < 0': dict(divisor=-1023.0), 'divisor nan': dict(divisor=float('nan')),
        'unknown op 7': dict(ops=(7,)), 'unknown op -1': dict(ops=(-1,)),
        'demosaic in ops': dict(ops=(F.OP_DEMOSAIC_NEAREST,)),
        'demosaic after a stage': dict(ops=(F.OP_GAMMA, F.OP_DEMOSAIC_NEAREST), params=(gam.data_ptr(), None)),
        'missing parameter block': dict(params=(None,)),
        'missing block after a skip': dict(ops=(F.OP_SKIP, F.OP_GAMMA), params=(None, None)),
        'nine stages': dict(ops=(F.OP_GAMMA,) * 9, params=(gam.data_ptr(),) * 9),
        'negative stage count': dict(n_ops=-1),
        'null raw': dict(raw_p=None), 'null out': dict(out_p=None),
        'bilateral without its arrays': dict(bil=none3),
        'H odd': dict(H=3), 'H 0': dict(H=0), 'W % 4': dict(W=6), 'W 2': dict(W=2), 'W 0': dict(W=0),
        'N 0': dict(N=0), 'N 65536': dict(N=65536), 'N < 0': dict(N=-1),
        'raw at 2 bytes': dict(raw_p=C.c_void_p(raw.data_ptr() + 2)), 'out at 1 byte': dict(out_p=C.c_void_p(out.data_ptr() + 1)),
    }
    for what, kw in refused.items():
        assert call(**kw) != 0, '%s was accepted' % what
        assert L.load().risp_last_error() != b'', what
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item(), 'a refused call wrote to the output'
    # and the same arguments without the fault are accepted (max_window 0 ignores the bilateral pointers; no stage at all)
    assert call() == 0 and call(wmax=0, bil=none3) == 0 and call(wmax=1, ops=(), params=()) == 0
    torch.cuda.synchronize()
    assert not (out[:n * h * w * 3] == 0x5A).all().item() and (out[n * h * w * 3:] == 0x5A).all().item()


def test_quantise_u8_refusals():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    fn = L.load().risp_quantise_u8
    x = torch.rand(1, 3, 4, 4).cuda()
    out = torch.full((64,), 0x5A, device='cuda', dtype=torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())
    for args in [(None, p(out), 1, 3, 4, 4), (p(x), None, 1, 3, 4, 4), (p(x), p(out), 0, 3, 4, 4), (p(x), p(out), 1, 2, 4, 4),
                 (p(x), p(out), 1, 4, 4, 4), (p(x), p(out), 1, 3, 0, 4), (p(x), p(out), 1, 3, 4, 0)]:
        assert fn(*args, 0, F._stream()) != 0, args[2:]
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item()
    with pytest.raises(ValueError):
        F.quantise_u8(torch.rand(1, 2, 4, 4).cuda())


# ---------------------------------------------------------------- 4. the pipelines' serve()
HEADLINE = 'Demosaic_01_sRGB_07_11_01_14'            # bench.py ARCH_DENOISE, an OriginUniversal


def _pipeline(arch, which='OriginUniversal'):
    from reconfigisp_amd.codes.models import networks
    opt = {'network_G': {'which_model_G': which, 'architecture': arch, 'module_path': None,
                         'individual_module_paths': [None] * 8}}
    torch.manual_seed(10)
    return networks.define_G(opt).cuda().eval()


def _forward_bytes(net, raw, white_level, reverse=False):
    """tensor2bgr(net(raw / white_level)) image by image.  The quotient is formed in fp32 on the host (numpy divides; a
    torch division of a device tensor by a Python scalar multiplies by the reciprocal, which is another number)."""
    x = torch.from_numpy(raw.cpu().numpy().astype(np.float32) / np.float32(white_level))[:, None].cuda()
    with torch.no_grad():
        y = net(x)
    return _host_bytes(y, reverse)


@pytest.mark.parametrize('n', [3, 4])
def test_pipeline_serve_headline_is_one_launch(n):
    from reconfigisp_amd import lib as L
    net = _pipeline(HEADLINE)
    raw = _raw(n, 34, 68, 1023, seed=90 + n).cuda()
    want, want_rgb = _forward_bytes(net, raw, 1023.0), _forward_bytes(net, raw, 1023.0, True)
    kept = net.intermediate_results                        # (a forward call binds a new list: both references come first)
    assert len(kept) == 5
    L.CALLS = {}
    try:
        got = net.serve(raw, 1023.0)
        calls = dict(L.CALLS)
    finally:
        L.CALLS = None
    assert net.last_serve_route == 'fused' and calls == {'risp_serve_u8': 1}, calls
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, 34, 68, 3)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(net.serve(raw, 1023.0, reverse_channels=True).cpu(), want_rgb)
    assert net.intermediate_results is kept and len(kept) == 5, 'serve() touched intermediate_results'


def test_pipeline_serve_follows_parameter_versions():
    net = _pipeline(HEADLINE)
    raw = _raw(3, 34, 68, 16383, seed=17).cuda()
    first = net.serve(raw, 16383.0).clone()
    assert torch.equal(first.cpu(), _forward_bytes(net, raw, 16383.0))
    with torch.no_grad():
        net.param_step4_gamma.fill_(1.0)                   # in place: the same storage, a new _version
    second = net.serve(raw, 16383.0).clone()
    assert not torch.equal(first, second), 'a changed gamma did not reach serve()'
    assert torch.equal(second.cpu(), _forward_bytes(net, raw, 16383.0))
    with torch.no_grad():
        net.param_step3_wbmanual.mul_(0.25)
        net.param_step2_bilateral[1] = -6.0                # sigma_color 1.2: the bilateral argument cache
    third = net.serve(raw, 16383.0)
    assert net.last_serve_route == 'fused' and not torch.equal(second, third)
    assert torch.equal(third.cpu(), _forward_bytes(net, raw, 16383.0))


def test_pipeline_serve_wide_bilateral_window_composes():
    """sigmoid(30) is 1 in fp32, and int(1) * 7 * 2 + 3 = 17: a learned window the one launch does not take"""
    net = _pipeline(HEADLINE)
    raw = _raw(2, 34, 68, 1023, seed=23).cuda()
    net.serve(raw, 1023.0)
    assert net.last_serve_route == 'fused'
    with torch.no_grad():
        net.param_step2_bilateral[0] = 30.0
    got = net.serve(raw, 1023.0)
    assert net.last_serve_route == 'composed'
    assert torch.equal(got.cpu(), _forward_bytes(net, raw, 1023.0))


@pytest.mark.parametrize('arch,which,route', [
    ('Demosaic_01_sRGB_05_01', 'OriginUniversal', 'composed'),                 # gray-world
    ('Demosaic_01_sRGB_07_05_11', 'OriginUniversal', 'composed'),              # gray-world behind the bilateral
    ('Demosaic_01_sRGB_08_01', 'OriginUniversal', 'composed'),                 # a 3 x 3 median
    ('Bayer_02_Demosaic_01_sRGB_11_01_14', 'IspUniversal', 'fused'),           # bench.py ARCH_HBM: element-wise only
    ('Demosaic_01_sRGB_13_10_01', 'IspUniversal', 'fused'),                    # WbQuadratic, a Skip in the middle
], ids=lambda v: v if isinstance(v, str) and '_' in v else None)
def test_pipeline_serve_routes(arch, which, route):
    net = _pipeline(arch, which)
    raw = _raw(3, 34, 68, 1023, seed=len(arch)).cuda()
    kept = net.intermediate_results
    buf = torch.empty((3, 34, 68, 3), device='cuda', dtype=torch.uint8)
    got = net.serve(raw, 1023.0, out=buf)
    assert got is buf and net.last_serve_route == route
    assert net.intermediate_results is kept
    assert torch.equal(got.cpu(), _forward_bytes(net, raw, 1023.0))


def test_isp_model_serve():
    from reconfigisp_amd.codes.models import create_model
    opt = OrderedDict(model='isp', gpu_ids=[0], dist=False, is_train=False,
                      network_G=dict(which_model_G='OriginUniversal', architecture=HEADLINE, module_path=None),
                      path=dict(pretrain_model_G=None, strict_load=True))
    model = create_model(opt)
    raw = _raw(1, 34, 68, 1023, seed=4).cuda()
    got = model.serve(raw, 1023.0, reverse_channels=True)
    assert model.netG.last_serve_route == 'fused'
    assert torch.equal(got.cpu(), _forward_bytes(model.netG, raw, 1023.0, True))


# ---------------------------------------------------------------- 5. graph capture
def test_serve_is_capturable():
    """one linear capture on a single stream: with out= given and the parameter blocks cached, serve() allocates nothing and
    never waits for the device"""
    net = _pipeline(HEADLINE)
    a, b = _raw(3, 34, 68, 1023, seed=1).cuda(), _raw(3, 34, 68, 1023, seed=2).cuda()
    eager_a, eager_b = net.serve(a, 1023.0).clone(), net.serve(b, 1023.0).clone()     # (also fills the caches)
    assert not torch.equal(eager_a, eager_b)
    slot, buf = a.clone(), torch.zeros((3, 34, 68, 3), device='cuda', dtype=torch.uint8)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.serve(slot, 1023.0, out=buf)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager_a)
    slot.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager_b)
