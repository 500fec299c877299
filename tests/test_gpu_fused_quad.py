"""GPU: the barrier-free quad form of the fused stencil segment (bilateral_chain_quad_kernel, risp_fused.hip) must give
the bits of the stage-by-stage path: nearest demosaic, bilateral (3 x 3 window), then the element-wise tail, each as
its own launch.  The shapes walk through border cases of the 2 x 4 patch and its ring of neighbour quads: one
quad row, two patch columns, tiles cut by the image edge, a tile count that is not a multiple of 8 (plain tile order
instead of the XCD-aware one), and the headline batch.  (One patch column - W = 4, both neighbour columns clamped - and
the rest of the argument space: tests/test_gpu_fused_segment.py.)"""
import pytest
import torch

import isp_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(64, 256, 256), (1, 2, 8), (3, 6, 8), (5, 48, 48), (7, 34, 136), (2, 512, 512)]


def _params(n, seed, quadratic=False):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    p = {'wb': (u(n, 3) * 5).cuda(), 'gamma': (0.2 + 0.6 * u(n, 1)).cuda(),
         'gtm': torch.sort(u(n, 3), dim=1).values.cuda(),
         'sc': (1 + 99 * u(n)).cuda(), 'ss': (1 + 99 * u(n)).cuda()}
    if quadratic:
        p['wbq'] = (0.45 + 0.1 * u(n, 30)).cuda()
    return p


def _both_paths(bay, window, p, quadratic=False):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    n = bay.shape[0]
    x = bay.cuda()
    win = window.to(torch.int32).cuda()
    first = (F.OP_WB_QUADRATIC, p['wbq'], F.wb_quadratic) if quadratic else (F.OP_WB_MANUAL, p['wb'], F.wb_manual)
    name = L.load().risp_bilateral_chain_kernel(1, 3, int(quadratic)).decode()
    assert name == 'bilateral_chain_quad_kernel<%s>' % ('true' if quadratic else 'false'), name
    plan = F.BilateralChainPlan(x, True, win, p['sc'], p['ss'], 3, [first[0], F.OP_GAMMA, F.OP_GTM_MANUAL],
                                [first[1], p['gamma'], p['gtm']])
    for o in plan.outs:
        o.fill_(float('nan'))                # every element of every stage must be written
    fused = [o.clone() for o in plan.launch()]
    with torch.no_grad():
        dem = F.demosaic_nearest(x)
        bil = F.origin_denoise(dem, 'bilateral', {'window_length': win, 'sigma_color': p['sc'], 'sigma_space': p['ss'],
                                                  'max_window': 3}, (255.0, 255.0))
        s0 = first[2](bil, first[1])
        s1 = F.gamma(s0, p['gamma'])
        s2 = F.gtm_manual(s1, p['gtm'])
    assert dem.shape == (n, 3) + tuple(bay.shape[2:])
    return fused, [dem, bil, s0, s1, s2]


def _assert_same_bits(fused, unfused, what):
    assert len(fused) == len(unfused) == 5
    for k, (a, b) in enumerate(zip(fused, unfused)):
        assert not torch.isnan(a).any().item(), '%s stage %d: elements left unwritten' % (what, k)
        assert torch.equal(a, b), '%s stage %d: %d elements differ, max %g' % (what, k, (a != b).sum().item(),
                                                                                (a - b).abs().max().item())


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_quad_form_equals_stage_by_stage(shape):
    n, h, w = shape
    bay, _ = O.synthetic_raw(n, max(h, 16), max(w, 16), seed=31 + n)
    bay = bay[:, :, :h, :w].contiguous()
    fused, unfused = _both_paths(bay, torch.full((n,), 3), _params(n, 100 + h))
    _assert_same_bits(fused, unfused, '%d x %d x %d' % shape)


def test_quad_form_windows_1_and_3_mixed():
    n, h, w = 6, 36, 72
    bay, _ = O.synthetic_raw(n, h, w, seed=41)
    window = torch.tensor([3, 1, 1, 3, 1, 3])
    fused, unfused = _both_paths(bay, window, _params(n, 7))
    _assert_same_bits(fused, unfused, 'windows 1 / 3')
    # window 1 is the 8-bit rounding of the demosaic output and nothing else
    dem, bil = fused[0], fused[1]
    for i in (1, 2, 4):
        assert torch.equal(bil[i], torch.floor(torch.clamp(dem[i] * 255.0, 0, 255) + 0.5) * (1.0 / 255.0))


def test_quad_form_with_wb_quadratic():
    n, h, w = 4, 48, 80
    bay, _ = O.synthetic_raw(n, h, w, seed=43)
    fused, unfused = _both_paths(bay, torch.full((n,), 3), _params(n, 9, quadratic=True), quadratic=True)
    _assert_same_bits(fused, unfused, 'WbQuadratic tail')
