"""GPU: DemosaicNet (include/risp.h "DemosaicNet") against its float64 restatement (tests/demosaicnet_reference.py) with random
weights: the four kernels of risp_dmnet.hip on their own, the whole op on both convolution routes (RISP_CONV_ARITH), bit
repeatability (repeated calls, batch positions, step-level reuse, graph replay), and the op inside the plugin, OriginUniversal and
the super-net.  RISP_TEST_SEEDS widens the random cases."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import demosaicnet_reference as R
from reconfigisp_amd import convnets as CN
from reconfigisp_amd import demosaicnet as DN
from reconfigisp_amd import functional as F
from reconfigisp_amd import lib as L
from reconfigisp_amd.isp_kernels import demosaic as dm

pytestmark = pytest.mark.gpu
_SEEDS = int(os.environ.get('RISP_TEST_SEEDS', '8'))
KERNEL_SHAPES = [(4, 4), (48, 48), (256, 256), (36, 20), (520, 12)]       # (36, 20): W/2 = 10, not a multiple of 4; tall strip


@pytest.fixture
def unregister():
    yield
    dm.unregister_demosaicnet()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return F._stream()


def _rel(got, ref, keep=None):
    """max |got - ref| relative to the RMS of ref (over the pixels ``keep`` selects)"""
    got, ref = got.double().cpu(), ref.double()
    if keep is not None:
        got, ref = got[keep], ref[keep]
    return ((got - ref).abs().max() / ref.pow(2).mean().sqrt()).item()


def _draw(seed, n, h, w):
    g = torch.Generator().manual_seed(seed)
    fd = DN.fold(R.random_state_dict(seed))
    x = torch.rand(n, 1, h, w, generator=g, dtype=torch.float64)
    fa = torch.relu(torch.randn(n, 64, h // 2, w // 2, generator=g, dtype=torch.float64))
    fb = torch.relu(torch.randn(n, 64, h // 2, w // 2, generator=g, dtype=torch.float64))
    up = torch.randn(n, 3, h, w, generator=g, dtype=torch.float64)
    gy = torch.randn(n, 3, h, w, generator=g, dtype=torch.float64)
    add = torch.randn(n, 1, h, w, generator=g, dtype=torch.float64)
    # the kernels see fp32 values: the float64 reference starts from the same rounded numbers
    r32 = lambda t: t.float().double()
    return {k: r32(v) for k, v in fd.items()}, r32(x), r32(fa), r32(fb), r32(up), r32(gy), r32(add)


def _cuda(t):
    return t.float().contiguous().cuda()


@pytest.mark.parametrize('shape', KERNEL_SHAPES)
def test_tail_kernels_against_float64(shape):
    h, w = shape
    n = 2
    fd, _, fa, fb, _, gup, _ = _draw(11 + h, n, h, w)
    d = {k: _cuda(v) for k, v in fd.items()}
    fa_, fb_ = _cuda(fa), _cuda(fb)
    up = torch.empty(n, 3, h, w, device='cuda')
    L.call('risp_dmnet_tail_fwd', _p(fa_), _p(fb_), _p(d['rp.weight']), _p(d['rp.bias']), _p(d['up.weight']), _p(d['up.bias']),
           _p(up), n, h, w, _stream())
    fa.requires_grad_(True)
    fb.requires_grad_(True)
    ref = R.tail(fa, fb, fd)
    assert _rel(up, ref.detach()) <= 1e-5
    # backward: the gradients at conv15's pre-activations (the ReLU masks come from the saved post-ReLU halves)
    ga, gb = torch.empty_like(fa_), torch.empty_like(fb_)
    L.call('risp_dmnet_tail_bwd', _p(_cuda(gup)), _p(fa_), _p(fb_), _p(d['rp.weight']), _p(d['up.weight']), _p(ga), _p(gb),
           n, h, w, _stream())
    ra, rb = torch.autograd.grad(ref, (fa, fb), gup)
    ra, rb = ra * (fa > 0), rb * (fb > 0)
    assert _rel(ga, ra) <= 1e-5 and _rel(gb, rb) <= 1e-5


@pytest.mark.parametrize('shape', KERNEL_SHAPES)
def test_head_kernels_against_float64(shape):
    h, w = shape
    n = 2
    fd, x, _, _, up, gy, add = _draw(23 + w, n, h, w)
    d = {k: _cuda(v) for k, v in fd.items()}
    x_, up_ = _cuda(x), _cuda(up)
    y = torch.empty(n, 3, h, w, device='cuda')
    L.call('risp_dmnet_head_fwd', _p(x_), _p(up_), _p(d['post.weight']), _p(d['post.bias']), _p(d['out.weight']), _p(d['out.bias']),
           _p(y), n, h, w, _stream())
    x.requires_grad_(True)
    up.requires_grad_(True)
    ref = R.head(x, up, fd)
    assert _rel(y, ref.detach()) <= 1e-5
    g_up, g_x = torch.empty_like(up_), torch.empty_like(x_)
    g_x2 = torch.empty_like(x_)
    for out, a in ((g_x, None), (g_x2, _cuda(add))):
        L.call('risp_dmnet_head_bwd', _p(_cuda(gy)), _p(x_), _p(up_), _p(d['post.weight']), _p(d['post.bias']), _p(d['out.weight']),
               _p(a), _p(g_up), _p(out), n, h, w, _stream())
    rx, rup = torch.autograd.grad(ref, (x, up), gy)
    # a hidden pre-activation within fp32 rounding of 0 may take the other side of the ReLU: leave its 3x3 footprint out
    # (the kernel rows of tests/test_gpu_demosaicnet_space.py draw inputs without such a unit and compare every pixel)
    pre = torch.nn.functional.conv2d(torch.cat([R.masked_mosaic(x.detach()), up.detach()], 1), fd['post.weight'], fd['post.bias'],
                                     padding=1)
    near = (pre.abs() < 2e-6 * pre.abs().max()).any(dim=1, keepdim=True).double()
    keep = torch.nn.functional.max_pool2d(near, 3, 1, 1) == 0
    assert keep.double().mean() > 0.98
    assert _rel(g_up, rup, keep.expand_as(rup)) <= 1e-5
    assert _rel(g_x, rx, keep) <= 1e-5
    assert torch.equal(g_x2, _cuda(add) + g_x)                       # add + the direct term, in that order


def test_entry_points_refuse_bad_geometry():
    t = torch.zeros(64, device='cuda')
    lib = L.load()
    for (n, h, w) in ((1, 2, 8), (1, 8, 2), (1, 7, 8), (1, 8, 9), (0, 8, 8), (1, 1 << 15, 1 << 14)):
        assert lib.risp_dmnet_head_fwd(_p(t), _p(t), _p(t), _p(t), _p(t), _p(t), _p(t), n, h, w, _stream()) != 0
        assert lib.risp_dmnet_tail_fwd(_p(t), _p(t), _p(t), _p(t), _p(t), _p(t), _p(t), n, h, w, _stream()) != 0
        assert lib.risp_dmnet_tail_bwd(_p(t), _p(t), _p(t), _p(t), _p(t), _p(t), _p(t), n, h, w, _stream()) != 0
        assert lib.risp_dmnet_head_bwd(_p(t), _p(t), _p(t), _p(t), _p(t), _p(t), None, _p(t), _p(t), n, h, w, _stream()) != 0
    with pytest.raises(ValueError, match='even'):
        F.demosaicnet(torch.zeros(1, 1, 8, 10, device='cuda')[:, :, :, :9], DN.load_demosaicnet(R.random_state_dict(0)))


@pytest.mark.parametrize('arith', ['f16x2', 'f32'])
def test_op_against_float64_over_draws(arith, monkeypatch):
    """Output: conftest.ErrorBudget(factor=1.25) with the fp32 CPU restatement as ref32.  Input gradient against a random
    functional in the 2-norm, || g - g64 || / || g64 ||: through 17 ReLU layers a single draw is a coin toss on flipped masks (one
    flip is an O(1) error on its footprint: measured per draw 8e-7 .. 4e-3 for this build and 6e-7 .. 8e-3 for the fp32
    restatement on the same draws), so on the split-precision route the median over draws is held to 1.5 x the restatement's
    median, as test_gpu_fullsize.py does for Path-Restore."""
    from conftest import ErrorBudget
    monkeypatch.setattr(CN, 'CONV_ARITH', arith)
    torch.set_num_threads(max(8, torch.get_num_threads()))
    budget = ErrorBudget(factor=1.25)
    e_hips, e_refs = [], []
    for draw in range(max(5, _SEEDS // 4)):
        g = torch.Generator().manual_seed(500 + draw)
        sd = R.random_state_dict(900 + draw)
        x = torch.rand((2, 1, 96, 96), generator=g, dtype=torch.float64).float()
        net = DN.load_demosaicnet(sd)
        xg = x.cuda().requires_grad_(True)
        y = F.demosaicnet(xg, net)
        gy = torch.randn(tuple(y.shape), generator=g, dtype=torch.float64).float()
        gx, = torch.autograd.grad(y, xg, gy.cuda())
        refs = {}
        for dt in (torch.float32, torch.float64):
            xc = x.to(dt).requires_grad_(True)
            yc = R.reference(xc, {k: v.to(dt) for k, v in sd.items()})
            gc, = torch.autograd.grad(yc, xc, gy.to(dt))
            refs[dt] = (yc.detach(), gc)
        budget(y, refs[torch.float32][0], refs[torch.float64][0], 'output, draw %d' % draw, 'outputs')
        g64 = refs[torch.float64][1]
        e_hip = ((gx.double().cpu() - g64).norm() / g64.norm()).item()
        e_ref = ((refs[torch.float32][1].double() - g64).norm() / g64.norm()).item()
        e_hips.append(e_hip)
        e_refs.append(e_ref)
        assert e_hip < 1e-2, (draw, e_hip)                     # (a wrong backward kernel is an error of order 1)
    budget.finish()
    if arith == 'f16x2':
        assert np.median(e_hips) <= 1.5 * np.median(e_refs), (e_hips, e_refs)
    # (RISP_CONV_ARITH=f32: over 16 draws the median is 2.3 x the restatement's - its 3x3 layers run in F(4,3) Winograd form and
    # decide their ReLU ties differently, as test_gpu_fullsize.py records for Path-Restore; the sanity bound above is what holds there)


def _net(seed=0):
    return DN.load_demosaicnet(R.random_state_dict(seed))


def test_same_bits_repeated_and_across_batch_positions():
    net = _net(1)
    x = torch.rand(4, 1, 64, 96, device='cuda')
    perm = torch.tensor([2, 0, 3, 1], device='cuda')
    gy = torch.randn(4, 3, 64, 96, device='cuda')
    outs = []
    for xi, gi in ((x, gy), (x, gy), (x[perm], gy[perm])):
        xi = xi.clone().requires_grad_(True)
        y = F.demosaicnet(xi, net)
        gx, = torch.autograd.grad(y, xi, gi)
        outs.append((y.detach(), gx))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0][perm], outs[2][0]) and torch.equal(outs[0][1][perm], outs[2][1])
    with torch.no_grad():                                              # inference launches: per image, any batch
        a = F.demosaicnet(x, net)
        b = F.demosaicnet(x[perm], net)
        c = F.demosaicnet(x[1:2], net)
    assert torch.equal(a[perm], b) and torch.equal(a[1:2], c)


def test_same_bits_with_step_level_reuse():
    net = _net(2)
    x = torch.rand(2, 1, 48, 48, device='cuda')
    gy = torch.randn(2, 3, 48, 48, device='cuda')
    ref_x = x.clone().requires_grad_(True)
    y0 = F.demosaicnet(ref_x, net)
    g0, = torch.autograd.grad(y0, ref_x, gy)
    rec = {}
    calls = [0]
    real = CN.L.call

    def counting(name, *a):
        calls[0] += 1
        return real(name, *a)

    CN.L.call = counting
    try:
        for k in range(2):
            xi = x.clone().requires_grad_(True)
            before = calls[0]
            y = F.demosaicnet(xi, net, rec)
            if k == 1:
                assert calls[0] == before                                # served from the record: nothing launched
            g, = torch.autograd.grad(y, xi, gy)
            assert torch.equal(y, y0) and torch.equal(g, g0)
    finally:
        CN.L.call = real


def test_same_bits_eager_and_graph_replay():
    from reconfigisp_amd.graphs import GraphedQueue
    net = _net(3)

    class Wrap(torch.nn.Module):
        def forward(self, x):
            return F.demosaicnet(x, net)

    xs = [torch.rand(2, 1, 64, 64, device='cuda') for _ in range(2)]
    with torch.no_grad():
        eager = [F.demosaicnet(x, net) for x in xs]
    q = GraphedQueue(Wrap(), xs)
    outs = q()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        assert torch.equal(a, b)
    xn = torch.rand(2, 1, 64, 64, device='cuda')
    q.load(0, xn)
    outs = q()
    with torch.no_grad():
        assert torch.equal(outs[0], F.demosaicnet(xn, net))


def test_plugin_call_and_origin_universal(unregister):
    from reconfigisp_amd.codes.models.modules import tools_origin as T
    from reconfigisp_amd.codes.models.modules.origin_universal import OriginUniversal
    sd = R.random_state_dict(4)
    net = dm.load_demosaicnet(sd)
    x = torch.rand(2, 1, 48, 64)
    xc = x.cuda()
    with torch.no_grad():
        direct = F.demosaicnet(xc, net)
        plug = T.DemosaicNet()(xc)
    assert torch.equal(direct, plug)
    model = OriginUniversal(None, 'Bayer_02_Demosaic_04_sRGB_10').cuda().eval()      # skip, DemosaicNet, skip
    with torch.no_grad():
        y = model(xc)
    ref64 = R.reference(x.double(), sd)
    ref32 = R.reference(x, {k: v.float() for k, v in sd.items()})
    from conftest import ErrorBudget
    budget = ErrorBudget(factor=1.25)
    budget(y, ref32, ref64, 'OriginUniversal Bayer_02_Demosaic_04_sRGB_10')
    budget.finish()


def test_supernet_search_step_with_weights(unregister):
    """A super-net with DemosaicNet loaded: the op is no longer masked.  One DARTS search step runs; then one forward / backward
    where alpha_demosaic[3]'s gradient must match the softmax-mixture gradient p3 (G.o3 - sum_k p_k G.o_k) with o3 from the float64
    restatement (G = the gradient at the demosaic slot's output, o_k the slot's operator outputs)."""
    from reconfigisp_amd.codes.models import create_model
    from test_host_logic import darts_opt
    sd = R.random_state_dict(5)
    dm.load_demosaicnet(sd)
    opt = darts_opt(torch.device('cuda'), n_step=1)
    opt['train']['step_reuse'] = True
    torch.manual_seed(0)
    model = create_model(opt)
    g = torch.Generator().manual_seed(7)
    data = (torch.rand(2, 1, 48, 48, generator=g), torch.rand(2, 3, 48, 48, generator=g),
            torch.rand(2, 1, 48, 48, generator=g), torch.rand(2, 3, 48, 48, generator=g))
    model.feed_data(data)
    model.update_learning_rate(0, warmup_iter=-1)
    model.optimize_alphas()
    ga = model.netG.alpha_demosaic.grad
    assert ga is not None and torch.isfinite(ga).all() and ga[3].item() != 0.0
    model.optimize_parameters()

    net = model.netG
    net.zero_grad()
    xin = data[0].cuda()
    y = net(xin)
    slot_in, slot_out = net.middle_results[0], net.middle_results[1]
    slot_out.retain_grad()
    G = torch.randn(tuple(y.shape), generator=g).cuda()
    (y * G).sum().backward()
    Gs = slot_out.grad.double().cpu()
    mods = net.all_modules[1]
    with torch.no_grad():
        outs = [m(slot_in, None).double().cpu() for m in mods[:3]]
    outs.append(R.reference(slot_in.detach().double().cpu(), sd))
    p = torch.softmax(net.alpha_demosaic.detach().double().cpu(), 0)
    assert (p > 0.2 * p.max()).all()                                  # nothing pruned at these logits
    dots = torch.stack([(Gs * o).sum() for o in outs])
    want = p[3] * (dots[3] - (p * dots).sum())
    got = net.alpha_demosaic.grad[3].double().cpu()
    assert torch.isfinite(got) and got != 0
    assert abs(got - want) <= 1e-3 * abs(want) + 1e-6 * (p * dots.abs()).sum(), (got.item(), want.item())
