"""GPU: SSIM on the HIP path (risp_ssim_fwd / risp_ssim_bwd) against the float64 reference of tests/ssim_reference.py on the
same inputs - value, quantised form, gradient, determinism, the criteria inside both models and the drivers' report.

Bars: |hip - f64| <= 1e-4 absolute on the value (BASELINE.json's parity bar; SSIM is of order 1) and no worse than the
fp32 torch restatement of the same formula by conftest.ErrorBudget; the gradient within 1e-4 of its largest magnitude."""
import os

import numpy as np
import pytest
import torch

import ssim_reference as R
from conftest import ErrorBudget
from test_host_logic import darts_opt, isp_opt, seed_darts

pytestmark = pytest.mark.gpu
CODES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'reconfigisp_amd', 'codes')

SHAPES = [(4, 3, 48, 48), (2, 1, 64, 80), (2, 3, 67, 53), (32, 1, 256, 256), (32, 3, 256, 256)]
IDS = ['x'.join(str(v) for v in s) for s in SHAPES]


def _check_value(got, x, y, dr, budget, what):
    truth = R.ssim(x.double(), y.double(), dr.double() if isinstance(dr, torch.Tensor) else dr)
    restated = R.ssim(x, y, dr)                              # the same text in fp32
    err = (got.double().cpu() - truth).abs().max().item()
    print('SSIM %-28s |hip - f64| = %.3e   |fp32 restatement - f64| = %.3e' % (what, err, (restated.double() - truth).abs().max().item()))
    assert err <= 1e-4, '%s: |hip - f64| = %.3e' % (what, err)
    budget(got, restated, truth, what=what, family='ssim')


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_value_matches_float64(shape):
    import reconfigisp_amd.functional as F
    x, y = R.smooth_pair(*shape, seed=sum(shape))
    budget = ErrorBudget()
    _check_value(F.ssim(x.cuda(), y.cuda()), x, y, 1.0, budget, 'smooth + noise')
    _check_value(F.ssim(x.cuda(), y.cuda(), 0.7), x, y, 0.7, budget, 'data range 0.7')
    budget.finish()


def test_identical_images_give_exactly_one():
    import reconfigisp_amd.functional as F
    x, _ = R.smooth_pair(3, 3, 67, 53, seed=2)
    got = F.ssim(x.cuda(), x.clone().cuda())
    assert torch.equal(got.cpu(), torch.ones(3))
    from reconfigisp_amd.codes.utils import util
    assert util.ssim_tensors(x[0].cuda(), x[0].clone().cuda()) == 1.0


def test_flat_bright_image_survives_the_cancellation():
    """0.9 +- 1e-3: E[xx] - E[x]^2 cancels seven digits; the plain fp32 restatement is 3.6e-6 off at data range 1 (measured:
    C2 = 9e-4 swamps a variance of ~3e-7 there), the kernel (sums about a per-tile pivot) has to stay inside 1e-4 and is
    expected well under the restatement.  Second row, data range 1e-2: C2 = 9e-8 is below the variance, so the variance
    terms decide the value and the cancellation is what is measured (the restatement is far off there; the kernel is held
    to the same 1e-4)."""
    import reconfigisp_amd.functional as F
    g = torch.Generator().manual_seed(11)
    y = (0.9 + 1e-3 * (2 * torch.rand(2, 3, 128, 160, generator=g) - 1)).float()
    x = (y + 3e-4 * torch.randn(2, 3, 128, 160, generator=g)).float()
    budget = ErrorBudget()
    _check_value(F.ssim(x.cuda(), y.cuda()), x, y, 1.0, budget, 'flat bright')
    _check_value(F.ssim(x.cuda(), y.cuda(), 1e-2), x, y, 1e-2, budget, 'flat bright, range 1e-2')
    budget.finish()


def test_per_image_data_ranges():
    import reconfigisp_amd.functional as F
    x, y = R.smooth_pair(4, 3, 64, 80, seed=4)
    dr = torch.tensor([1.0, 0.5, 0.25, 2.0])
    budget = ErrorBudget()
    got = F.ssim(x.cuda(), y.cuda(), dr.cuda())
    _check_value(got, x, y, dr, budget, 'per-image data ranges')
    budget.finish()
    for n in range(4):                                       # every image sees its own range
        assert torch.equal(got[n:n + 1], F.ssim(x[n:n + 1].cuda(), y[n:n + 1].cuda(), float(dr[n])))


@pytest.mark.parametrize('shape', [(2, 3, 48, 48), (1, 3, 67, 53), (1, 1, 64, 80)], ids=['48x48', '67x53', '64x80'])
def test_quantised_form_and_get_ssim(shape):
    from reconfigisp_amd.codes.utils import util
    from reconfigisp_amd.codes.utils import util_path_restore as U
    x, y = R.smooth_pair(*shape, seed=21)
    x = (x * 1.2 - 0.1)                                       # values outside [0, 1]: the clip is part of the arithmetic
    xq, yq = R.tensor2bgr_codes(x), R.tensor2bgr_codes(y)
    for n in range(shape[0]):
        assert np.array_equal(xq[n].transpose(1, 2, 0), util.tensor2bgr(x[n]))
    truth = R.ssim_numpy(xq, yq, 255.0)
    got = util.ssim_tensors(x.cuda(), y.cuda())
    got = np.atleast_1d(np.asarray(got, np.float64))
    print('SSIM quantised %s |hip - f64| = %.3e' % (shape, np.abs(got - truth).max()))
    assert np.abs(got - truth).max() <= 1e-4
    # get_ssim: NHWC arrays, the data range of the INPUT image, per image
    ranges = np.asarray([float(a.max()) - float(a.min()) for a in xq])
    truth_r = R.ssim_numpy(xq, yq, ranges)
    got_r = U.get_ssim(xq.transpose(0, 2, 3, 1), yq.transpose(0, 2, 3, 1))
    assert got_r.shape == (shape[0],) and np.abs(got_r - truth_r).max() <= 1e-4
    one = U.get_ssim(xq[0].transpose(1, 2, 0), yq[0].transpose(1, 2, 0))
    assert isinstance(one, float) and abs(one - truth_r[0]) <= 1e-4


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_gradient_matches_float64_autograd(shape):
    import reconfigisp_amd.functional as F
    x, y = R.smooth_pair(*shape, seed=7 + sum(shape))
    g = torch.Generator().manual_seed(3)
    gs = torch.randn(shape[0], generator=g) * 2 + 0.5         # non-uniform upstream
    dr = 0.8
    xd = x.double().requires_grad_(True)
    (R.ssim(xd, y.double(), dr) * gs.double()).sum().backward()
    xg = x.cuda().requires_grad_(True)
    (F.ssim(xg, y.cuda(), dr) * gs.cuda()).sum().backward()
    scale = xd.grad.abs().max().item()
    err = (xg.grad.double().cpu() - xd.grad).abs().max().item() / scale
    print('SSIM gradient %s: error / largest magnitude = %.3e (largest %.3e)' % (shape, err, scale))
    assert err <= 1e-4
    # ssim_loss = 1 - mean: the same kernel behind a uniform upstream
    xl = x.cuda().requires_grad_(True)
    loss = F.ssim_loss(xl, y.cuda(), dr)
    loss.backward()
    xd.grad = None
    ref = 1 - R.ssim(xd, y.double(), dr).mean()
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-4
    assert (xl.grad.double().cpu() - xd.grad).abs().max().item() <= 1e-4 * xd.grad.abs().max().item()


def test_target_gradient_is_refused():
    import reconfigisp_amd.functional as F
    x, y = R.smooth_pair(1, 3, 16, 16, seed=1)
    with pytest.raises(RuntimeError, match='target'):
        F.ssim(x.cuda(), y.cuda().requires_grad_(True))


def test_same_bits_on_every_run_and_stream():
    import reconfigisp_amd.functional as F
    x, y = R.smooth_pair(8, 3, 131, 97, seed=13)
    x, y = x.cuda(), y.cuda()
    gs = torch.linspace(-1, 2, 8).cuda()

    def run():
        xg = x.clone().requires_grad_(True)
        v = F.ssim(xg, y, 0.9)
        (v * gs).sum().backward()
        return v.detach().clone(), xg.grad.clone()
    v0, g0 = run()
    v1, g1 = run()
    assert torch.equal(v0, v1) and torch.equal(g0, g1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        v2, g2 = run()
    side.synchronize()
    assert torch.equal(v0, v2) and torch.equal(g0, g2)


# ---------------------------------------------------------------------------------------------- models
def _isp_step(crit, weight=None):
    from reconfigisp_amd.codes.models import create_model
    opt = isp_opt(torch.device('cuda'), 'OriginUniversal', 'Bayer_02_Demosaic_01_sRGB_11_01_13_14', crit)
    if weight is not None:
        opt['train']['ssim_weight'] = weight
    torch.manual_seed(1)
    model = create_model(opt)
    g = np.random.Generator(np.random.PCG64(5))
    img = torch.from_numpy(g.random((4, 1, 48, 48)).astype(np.float32)) * 0.6
    gt = torch.from_numpy(g.random((4, 3, 48, 48)).astype(np.float32))
    before = [p.detach().clone() for p in model.netG.parameters()]
    model.feed_data((img, gt))
    model.update_learning_rate(0, warmup_iter=-1)
    model.optimize_parameters()
    moved = max((p.detach() - b).abs().max().item() for p, b in zip(model.netG.parameters(), before) if p.numel())
    return float(model.log_dict['loss']), moved, model


@pytest.mark.filterwarnings('ignore:Detected call of')
def test_isp_model_trains_with_the_ssim_criteria():
    l2, _, plain = _isp_step('l2')
    assert plain._fused                                      # the element-wise pipeline with l2 takes the fused step ...
    mixed, moved, model = _isp_step('l2_ssim', 0.3)
    assert not model._fused                                  # ... and never with an SSIM criterion
    assert np.isfinite(mixed) and mixed != l2 and moved > 0
    zero, moved0, model0 = _isp_step('l2_ssim', 0.0)
    assert not model0._fused and moved0 > 0
    assert abs(zero - l2) <= 1e-6 * abs(l2), (zero, l2)
    alone, moved1, _ = _isp_step('ssim')
    assert np.isfinite(alone) and 0 < alone < 2 and moved1 > 0


def _darts_iteration(crit, weight=None):
    from reconfigisp_amd.codes.models import create_model
    opt = darts_opt(torch.device('cuda'), 3)
    opt['train']['pixel_criterion'] = crit
    if weight is not None:
        opt['train']['ssim_weight'] = weight
    torch.manual_seed(0)
    model = create_model(opt)
    seed_darts(model)
    g = np.random.Generator(np.random.PCG64(8))
    mk = lambda c: torch.from_numpy(g.random((4, c, 48, 48)).astype(np.float32))
    data = (mk(1) * 0.6, mk(3), mk(1) * 0.6, mk(3))
    before = [p.detach().clone() for p in model.netG.trainable_parameters if p.numel()]
    alphas = [a.detach().clone() for a in model.netG.alphas]
    model.feed_data(data)
    model.update_learning_rate(0, warmup_iter=-1)
    model.optimize_alphas()
    model.optimize_parameters()
    moved = max((p.detach() - b).abs().max().item()
                for p, b in zip([p for p in model.netG.trainable_parameters if p.numel()], before))
    moved_a = max((a.detach() - b).abs().max().item() for a, b in zip(model.netG.alphas, alphas))
    return float(model.log_dict['loss']), float(model.val_loss), moved, moved_a


@pytest.mark.filterwarnings('ignore:Detected call of')
def test_darts_model_searches_with_the_ssim_criteria():
    l2, v2, _, _ = _darts_iteration('l2')
    mixed, vm, moved, moved_a = _darts_iteration('l2_ssim', 0.3)
    assert np.isfinite(mixed) and np.isfinite(vm) and mixed != l2 and vm != v2
    assert moved > 0 and moved_a > 0
    zero, vz, _, _ = _darts_iteration('l2_ssim', 0.0)
    assert abs(zero - l2) <= 1e-6 * abs(l2) and abs(vz - v2) <= 1e-6 * abs(v2), (zero, l2, vz, v2)


# ---------------------------------------------------------------------------------------------- drivers
def test_test_driver_reports_ssim_on_request(tmp_path, monkeypatch, capsys):
    from reconfigisp_amd.codes import test as t1
    from reconfigisp_amd.codes.options import options as option
    real = option.parse
    report = [False]

    def parse(path, is_train=True):
        opt = real(path, is_train)
        opt['datasets']['test'].update(data_size=128, n_images=2)
        opt['path']['results_root'] = opt['path']['log'] = str(tmp_path / 'res')
        opt['test_seed'] = 3
        if report[0]:
            opt['report_ssim'] = True
        return opt
    monkeypatch.setattr(option, 'parse', parse)
    yml = os.path.join(CODES, 'options', 'test', 'synthetic_test.yml')
    t1.main(['--opt', yml])
    plain = capsys.readouterr().out
    report[0] = True
    t1.main(['--opt', yml])
    with_ssim = capsys.readouterr().out
    lines = lambda s, tag: [l for l in s.splitlines() if l.startswith(tag)]
    assert not lines(plain, 'SSIM')
    assert lines(plain, 'PSNR') == lines(with_ssim, 'PSNR') and len(lines(plain, 'PSNR')) == 2
    got = lines(with_ssim, 'SSIM')
    assert len(got) == 2 and got[0].startswith('SSIM in: min ') and got[1].startswith('SSIM out: min ')
    for l in got:
        vals = [float(p.split()[-1]) for p in l.split(': ', 1)[1].split(', ')]
        assert len(vals) == 4 and 0 < vals[0] <= vals[2] <= vals[1] <= 1          # min <= mean <= max
    # everything but the SSIM lines is what it was
    assert [l for l in with_ssim.splitlines() if not l.startswith('SSIM')] == plain.splitlines()


def test_full_frame_through_ssim_tensors():
    """3000 x 4000: the size of the frames test_split.py blends (that driver prints PSNR only; this is the call a user makes on its output)"""
    from reconfigisp_amd.codes.utils import util
    x, y = R.smooth_pair(1, 3, 3000, 4000, seed=31, noise=0.03)
    got = util.ssim_tensors(x[0].cuda(), y[0].cuda())
    truth = R.ssim_numpy(R.tensor2bgr_codes(x), R.tensor2bgr_codes(y), 255.0)[0]
    print('SSIM 3000 x 4000 quantised: hip %.7f f64 %.7f' % (got, truth))
    assert abs(got - truth) <= 1e-4
