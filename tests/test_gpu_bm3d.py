"""Classical BM3D (risp_origin_bm3d, reconfigisp_amd/csrc/risp_bm3d.hip) against its float64 OPSPEC
(tests/bm3d_reference.py), and the layers above it.

Bar of the Origin kernels (test_gpu_origin.py): no code more than 1 off, at most 0.2 % of the codes off; the
unquantised form (out_div < 0) >= 99.9 % of the samples within 1e-3 codes and all within 1 code.  A 3D coefficient
that sits on the hard threshold can be kept in one arithmetic and dropped in the other, and a value at .5 can round
either way; the group tables are integer work and must be identical.  Observed worst case over this file at
RISP_TEST_SEEDS=64 (73 code comparisons on one MI355X): no code more than 1 off, 9 comparisons with any code off at
all, the worst of them 0.025 % of its codes (a random case); the full-size and tall-strip cases under 0.005 %."""
import os

import numpy as np
import pytest
import torch

import bm3d_reference as B

pytestmark = pytest.mark.gpu

_FUZZ = int(os.environ.get('RISP_TEST_SEEDS', '8'))
# (n1, radius, cspace, wtransform) per image of a mixed batch: both block sizes, R in {1, 4, 9}, both colour spaces,
# both transforms
MIXED = [(8, 1, 0, 0), (4, 4, 1, 1), (8, 9, 1, 0), (4, 9, 0, 1), (8, 4, 0, 1), (4, 1, 1, 0)]
INIT = dict(cff=1.5, n1=8, cspace=0, wtransform=0, neighborhood=8)       # the reference's initial values


def image(n, h, w, seed, noise=12.0):
    """smooth structure (so that block distances spread) plus Gaussian noise, 0..255 with clipping"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    base = []
    for _ in range(n):
        f = torch.rand(3, 3, generator=g) * 0.3 + 0.05
        ph = torch.rand(3, generator=g) * 6.3
        base.append(torch.stack([128 + 90 * torch.sin(f[c, 0] * yy + f[c, 1] * xx + ph[c]) * torch.cos(f[c, 2] * xx)
                                 for c in range(3)]))
    x = torch.stack(base) + noise * torch.randn(n, 3, h, w, generator=g)
    return x.clamp(-10, 265)


def split(cfg):
    return [list(v) for v in zip(*cfg)]


def run(x, sigma, n1, radius, cspace, wtransform, scales=(1.0, 1.0), **kw):
    import reconfigisp_amd.functional as F
    return F.origin_bm3d(x.cuda(), torch.as_tensor(sigma, dtype=torch.float32), n1, cspace, wtransform, radius,
                         scales, **kw)


OBSERVED = []      # (what, largest code difference, fraction of codes off) of every comparison, for soak reports


def assert_codes(y, ref, what=''):
    d = (y.cpu().double() - ref.double()).abs()
    frac = (d > 0.5).double().mean().item()
    OBSERVED.append((what, d.max().item(), frac))
    assert d.max().item() <= 1.0 + 1e-6, '%s: a code %g off' % (what, d.max().item())
    assert frac <= 0.002, '%s: %.4f %% of the codes off' % (what, 100 * frac)


def assert_diag(y, ref, what=''):
    d = (y.cpu().double() - ref.double()).abs()
    assert d.max().item() <= 1.0, '%s: %g codes off' % (what, d.max().item())
    assert (d <= 1e-3).double().mean().item() >= 0.999, '%s: %.4f %% beyond 1e-3' % (what, 100 * (d > 1e-3).double().mean())


@pytest.mark.parametrize('shape', [(8, 8), (34, 50), (64, 48), (256, 256)])
def test_group_tables_equal_reference(shape):
    h, w = shape
    cfg = MIXED if min(h, w) >= 8 else [c for c in MIXED if c[0] == 4]
    n1, rad, cs, wt = split(cfg)
    x = image(len(cfg), h, w, seed=h * 1000 + w)
    _, groups = run(x, [4.0] * len(cfg), n1, rad, cs, wt, want_groups=True)
    ref = B.group_table(x, n1, rad)
    assert groups.shape == ref.shape
    assert torch.equal(groups.cpu(), ref)


@pytest.mark.parametrize('shape', [(34, 50), (64, 48)])
def test_mixed_batch_matches_reference(shape):
    h, w = shape
    n1, rad, cs, wt = split(MIXED)
    sigma = [2.55 * c for c in (1.5, 6.0, 12.0, 3.0, 9.0, 0.0)]       # the last image: sigma 0 returns the codes
    x = image(len(MIXED), h, w, seed=7 + h)
    y, _ = run(x, sigma, n1, rad, cs, wt)
    ref, _ = B.bm3d(x, sigma, n1, cs, wt, rad)
    assert_codes(y, ref, 'codes')
    assert torch.equal(y[-1].cpu(), torch.from_numpy(B.codes(x[-1:])[0]).float())
    yd, _ = run(x, sigma, n1, rad, cs, wt, scales=(1.0, -1.0))
    refd, _ = B.bm3d(x, sigma, n1, cs, wt, rad, out_div=-1.0)
    assert_diag(yd, refd, 'unquantised')


def test_full_size_initial_parameters():
    """256 x 256 at the reference's initial parameters (cff 1.5 -> sigma 3.825, n1 8, opponent, DCT, R 8), the same
    with n1 = 4, and a stronger sigma (cff 6) on the initial geometry"""
    x = image(2, 256, 256, seed=3, noise=10.0)
    for n1, cff in ((8, 1.5), (4, 1.5), (8, 6.0)):
        y, _ = run(x, 2.55 * cff, n1, 8, 0, 0)
        ref, _ = B.bm3d(x, 2.55 * cff, n1, 0, 0, 8)
        assert_codes(y, ref, 'n1=%d cff=%g' % (n1, cff))


@pytest.mark.parametrize('n1', [8, 4])
def test_tall_strip_beyond_32768_rows(n1):
    """member corners with y >= 32768 (the packed corner's top bit set) filter and aggregate like any other"""
    h, w = 32800, 12
    x = image(1, h, w, seed=21)
    y, groups = run(x, 2.55 * 3.0, n1, 2, 0, 0, want_groups=True)
    assert torch.isfinite(y).all()
    ref, table = B.bm3d(x, 2.55 * 3.0, n1, 0, 0, 2)
    assert torch.equal(groups.cpu(), table)
    assert (y[:, :, 32760:].cpu() - ref[:, :, 32760:]).abs().max().item() <= 1.0     # the rows past the sign bit
    assert_codes(y, ref, 'tall strip')


@pytest.mark.parametrize('seed', range(_FUZZ))
def test_random_cases(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 4))
    h, w = int(rng.integers(8, 41)), int(rng.integers(8, 41))
    n1 = [int(v) for v in rng.choice([4, 8], n)]
    rad = [int(v) for v in rng.integers(1, 10, n)]
    cs, wt = [int(v) for v in rng.integers(0, 2, n)], [int(v) for v in rng.integers(0, 2, n)]
    sigma = [float(v) for v in rng.uniform(0.5, 30.6, n)]
    x = image(n, h, w, seed=seed, noise=float(rng.uniform(2, 30)))
    y, groups = run(x, sigma, n1, rad, cs, wt, want_groups=True)
    ref, table = B.bm3d(x, sigma, n1, cs, wt, rad)
    assert torch.equal(groups.cpu(), table)
    assert_codes(y, ref, 'seed %d' % seed)


def test_determinism_batch_independence_and_chunks():
    import reconfigisp_amd.lib as L
    n1, rad, cs, wt = split(MIXED[:5])
    sigma = [10.0, 20.0, 5.0, 30.0, 15.0]
    x = image(5, 40, 36, seed=11)
    y1, g1 = run(x, sigma, n1, rad, cs, wt, want_groups=True)
    y2, g2 = run(x, sigma, n1, rad, cs, wt, want_groups=True)
    assert torch.equal(y1, y2) and torch.equal(g1, g2)
    for i in range(5):
        yi, gi = run(x[i:i + 1], sigma[i], n1[i], rad[i], cs[i], wt[i], want_groups=True)
        assert torch.equal(yi[0], y1[i]) and torch.equal(gi[0], g1[i])
    per = L.load().risp_origin_bm3d_scratch_bytes(1, 40, 36)
    yc, gc = run(x, sigma, n1, rad, cs, wt, scratch_bytes=2 * per, want_groups=True)     # chunks of 2, 2, 1
    assert torch.equal(yc, y1) and torch.equal(gc, g1)


def test_unit_scales_equal_plugin_convention():
    x = image(3, 32, 40, seed=5)
    n1, rad, cs, wt = split(MIXED[:3])
    y255, _ = run(x, [8.0, 16.0, 24.0], n1, rad, cs, wt)
    y01, _ = run((x / 255.).contiguous(), [8.0, 16.0, 24.0], n1, rad, cs, wt, scales=(255.0, 255.0))
    assert torch.equal(y01, y255 / 255.)


def test_refused_arguments():
    import reconfigisp_amd.lib as L
    x = image(1, 6, 16, seed=1)
    with pytest.raises(ValueError):
        run(x, 5.0, 8, 2, 0, 0)                             # H < n1
    x = image(1, 16, 16, seed=1)
    with pytest.raises(ValueError):
        run(x, 5.0, 5, 2, 0, 0)                             # n1 not in {4, 8}
    for r in (0, 10):
        with pytest.raises(ValueError):
            run(x, 5.0, 8, r, 0, 0)
    with pytest.raises(ValueError):
        run(image(1, 8, 65536, seed=1), 5.0, 4, 2, 0, 0)      # W beyond the packed corner's 16 bits
    per = L.load().risp_origin_bm3d_scratch_bytes(1, 16, 16)
    with pytest.raises(RuntimeError):
        run(x, 5.0, 8, 2, 0, 0, scratch_bytes=per - 256)    # scratch short of one image
    assert L.load().risp_origin_bm3d_scratch_bytes(1, 3, 16) == 0


def test_scratch_cache_release():
    import reconfigisp_amd.functional as F
    x = image(1, 16, 16, seed=2)
    y1, _ = run(x, 6.0, 8, 2, 0, 0)
    assert F._bm3d_scratch
    F.release_bm3d_scratch()
    assert not F._bm3d_scratch
    y2, _ = run(x, 6.0, 8, 2, 0, 0)
    assert torch.equal(y1, y2)


def test_spatial_noise_reduction_plugin():
    from reconfigisp_amd.isp_kernels.spatialnoisereduction import SpatialNoiseReduction
    x = image(2, 24, 32, seed=9)
    params = dict(cff=torch.tensor([1.5, 8.0]), n1=[8, 4], cspace=[0, 1], wtransform=[0, 1], neighborhood=[8, 3])
    out = SpatialNoiseReduction().run(x.permute(0, 2, 3, 1).cuda(), 'bm3d', params)
    ref, _ = B.bm3d(x, 2.55 * params['cff'], params['n1'], params['cspace'], params['wtransform'],
                    params['neighborhood'])
    assert out.shape == (2, 24, 32, 3)
    assert_codes(out.permute(0, 3, 1, 2), ref, 'plugin')


def test_origin_universal_classical_bm3d():
    from reconfigisp_amd.codes.models.modules.origin_universal import OriginUniversal
    from reconfigisp_amd.codes.models.modules.srcnn_res_arch import SRCNNRes
    from reconfigisp_amd.codes.models.modules.tools_origin import OriginNoiseBm3d
    arch = 'Bayer_02_Demosaic_02_sRGB_15'
    assert isinstance(OriginUniversal(None, arch).all_modules[-1], SRCNNRes)       # default: the proxy stays
    model = OriginUniversal(None, arch, classical_bm3d=True).cuda()
    assert isinstance(model.all_modules[-1], OriginNoiseBm3d)
    g = torch.Generator().manual_seed(4)
    raw = (torch.rand(2, 1, 48, 64, generator=g) * 0.6 + 0.2).cuda()
    with torch.no_grad():
        y = model(raw)
    bgr = model.intermediate_results[-2]
    # the initial parameters: sigmoid(PARAM_INIT) -> cff 1.5, n1 8, opponent, DCT, R 8
    ref, _ = B.bm3d(bgr.cpu(), 2.55 * 12 * torch.sigmoid(torch.tensor(-1.946)), 8, 0, 0, 8, in_scale=255., out_div=255.)
    assert_codes(y.cpu() * 255., ref * 255., 'OriginUniversal')


def test_darts_ft_bm3d_teacher():
    """proxy_ft_params.bm3d_teacher on the synthetic search options: the bm3d proxy learns from the classical BM3D,
    every other proxy draws the same random numbers and ends with the same weights as without the key"""
    import random
    from reconfigisp_amd.codes.models import create_model
    from reconfigisp_amd.codes.options import options as option
    here = os.path.dirname(os.path.abspath(__file__))
    yml = os.path.join(here, '..', 'reconfigisp_amd', 'codes', 'options', 'train', 'synthetic_search_ft.yml')

    def build(teacher):
        opt = option.parse(yml, is_train=True)
        opt['network_G']['n_step'] = 1
        opt['proxy_ft_params'].update(memory_size=2, ft_steps=2)
        if teacher:
            opt['proxy_ft_params']['bm3d_teacher'] = True
        random.seed(0)
        torch.manual_seed(0)
        model = create_model(opt)
        g = torch.Generator().manual_seed(1)
        data = (torch.rand(2, 1, 32, 32, generator=g), torch.rand(2, 3, 32, 32, generator=g),
                torch.rand(2, 1, 32, 32, generator=g), torch.rand(2, 3, 32, 32, generator=g))
        model.feed_data(data)
        model.optimize_parameters()
        return model

    plain, taught = build(False), build(True)
    assert [n for n, *_ in plain.ft_nets] == ['crysisengine', 'whiteworld', 'bilateral', 'median', 'fastnlm']
    assert [n for n, *_ in taught.ft_nets] == ['crysisengine', 'whiteworld', 'bilateral', 'median', 'fastnlm', 'bm3d']
    idx = [n for n, _ in taught.netG.proxy_ft_flag].index('bm3d')
    before = {k: v.clone() for k, v in taught.netG.all_modules[-1][idx].state_dict().items()}
    for m in (plain, taught):
        random.seed(5)
        torch.manual_seed(5)
        m.finetune_proxies()
    assert np.isfinite(taught.log_dict['ft_loss_bm3d'])
    after = taught.netG.all_modules[-1][idx].state_dict()
    assert any(not torch.equal(after[k], before[k]) for k in before)
    for k in plain.log_dict:
        if k.startswith('ft_loss_'):
            assert np.isfinite(taught.log_dict[k])
    for j, (name, _) in enumerate(plain.netG.proxy_ft_flag):
        if name == 'bm3d':
            continue
        a, b = plain.netG.all_modules[-1][j].state_dict(), taught.netG.all_modules[-1][j].state_dict()
        for k in a:
            assert torch.equal(a[k], b[k]), (name, k)
