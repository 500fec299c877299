"""SSIM without a GPU: the C ABI exports and binds the entry points, the float64 reference of tests/ssim_reference.py is the
measure it claims to be (equal to scikit-image's filter-then-crop route, 1 on identical images, symmetric), the criteria
are wired into both models, and bad inputs are rejected with a message."""
import ctypes

import numpy as np
import pytest
import torch

import ssim_reference as R


def test_library_exports_and_binds_the_ssim_entry_points():
    from reconfigisp_amd import lib
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in ('risp_ssim_fwd', 'risp_ssim_bwd', 'risp_ssim_scratch_floats'):
        assert hasattr(handle, name), 'libreconfigisp_hip.so does not export %s' % name
        assert name in lib.SIGNATURES, 'lib.SIGNATURES does not bind %s' % name
    loaded = lib.load()
    # one partial sum per workgroup and plane; nothing for shapes the entry points reject
    assert loaded.risp_ssim_scratch_floats(4, 3, 48, 48) >= 4 * 3
    assert loaded.risp_ssim_scratch_floats(1, 3, 3000, 4000) >= 3 * (2994 // 64) * (3994 // 64)
    assert loaded.risp_ssim_scratch_floats(1, 3, 6, 48) == 0


def test_entry_points_reject_bad_geometry_with_a_message():
    """argument checks run before any launch: no device is needed to see them"""
    import threading
    from reconfigisp_amd import lib
    loaded = lib.load()
    failures = []

    def body():                         # risp_last_error is per thread: the messages provoked here stay out of the main thread's
        try:
            _bad_geometry(loaded)
        except BaseException as e:      # noqa: BLE001 - handed to the main thread
            failures.append(e)
    t = threading.Thread(target=body)
    t.start()
    t.join()
    if failures:
        raise failures[0]
    assert loaded.risp_last_error() == b''


def _bad_geometry(loaded):
    one = ctypes.c_void_p(16)           # never dereferenced: the geometry is refused first
    for shape in ((1, 3, 6, 48), (1, 3, 48, 5), (0, 3, 48, 48), (70000, 1, 8, 8), (8, 4, 8192, 8192)):
        status = loaded.risp_ssim_fwd(one, one, None, 1.0, 0, one, one, 1 << 20, *shape, None)
        assert status == 1
        msg = loaded.risp_last_error().decode()
        assert 'risp_ssim_fwd' in msg and 'H=%d' % shape[2] in msg, msg
        assert loaded.risp_ssim_bwd(one, one, None, 1.0, one, one, *shape, None) == 1
        assert 'risp_ssim_bwd' in loaded.risp_last_error().decode()
    assert loaded.risp_ssim_fwd(one, one, None, 1.0, 0, one, one, 0, 1, 3, 48, 48, None) == 1
    assert 'scratch' in loaded.risp_last_error().decode()


@pytest.mark.parametrize('shape', [(3, 48, 48), (1, 64, 80), (3, 67, 53)])
def test_reference_equals_filter_then_crop(shape):
    c, h, w = shape
    x, y = R.smooth_pair(1, c, h, w, seed=h * w)
    x, y = x.double().numpy(), y.double().numpy()
    for dr in (1.0, 0.6):
        a = R.ssim_numpy(x, y, dr)[0]
        b = R.ssim_filter_crop(x[0], y[0], dr)
        assert abs(a - b) <= 1e-12, (a, b)
        assert 0.0 < a < 1.0


def test_reference_identity_symmetry_and_ranges():
    x, y = R.smooth_pair(3, 3, 40, 37, seed=5)
    x, y = x.double(), y.double()
    assert torch.equal(R.ssim(x, x), torch.ones(3, dtype=torch.float64))
    assert torch.equal(R.ssim(x, y, 0.8), R.ssim(y, x, 0.8))
    per_image = torch.tensor([1.0, 0.5, 0.25], dtype=torch.float64)
    both = R.ssim(x, y, per_image)
    for n in range(3):
        assert abs(both[n] - R.ssim(x[n:n + 1], y[n:n + 1], float(per_image[n]))[0]) <= 1e-15
    assert R.ssim(x[:1], y[:1], 1.0)[0] > R.ssim(x[:1], y[:1], 0.25)[0]         # smaller constants: the same noise costs more
    with pytest.raises(ValueError):
        R.ssim(x[:, :, :6], y[:, :, :6])


def test_reference_gradient_matches_finite_differences():
    """the gradient truth of the GPU test is autograd through the reference; here autograd is checked against central
    differences of the reference itself, so that truth is not circular"""
    x, y = R.smooth_pair(2, 2, 12, 11, seed=9)
    x, y = x.double().requires_grad_(True), y.double()
    gs = torch.tensor([0.7, -1.3], dtype=torch.float64)
    (R.ssim(x, y, 0.9) * gs).sum().backward()
    eps = 1e-6
    for n, c, i, j in [(0, 0, 0, 0), (0, 1, 5, 6), (1, 0, 11, 10), (1, 1, 3, 9), (0, 0, 6, 3)]:
        d = torch.zeros_like(x)
        d[n, c, i, j] = eps
        with torch.no_grad():
            fd = (((R.ssim(x + d, y, 0.9) - R.ssim(x - d, y, 0.9)) * gs).sum() / (2 * eps)).item()
        assert abs(fd - x.grad[n, c, i, j].item()) <= 1e-7 * max(1.0, abs(fd)), (fd, x.grad[n, c, i, j].item())


def test_criteria_accept_the_ssim_kinds():
    from reconfigisp_amd.codes.models.darts_model import PixelLoss, _criterion
    from reconfigisp_amd.codes.models.isp_model import pixel_criterion
    from reconfigisp_amd.codes.utils.util_loss import SsimLoss
    dev = torch.device('cpu')
    opt = {'ssim_weight': 0.25}
    for make in (lambda kind, o: _criterion(kind, o, dev), lambda kind, o: pixel_criterion(kind, dev, o)):
        plain = make('ssim', {})
        assert isinstance(plain, SsimLoss) and plain.pixel is None
        for kind in ('l1_ssim', 'l2_ssim'):
            cri = make(kind, opt)
            assert isinstance(cri, SsimLoss) and cri.weight == 0.25 and cri.pixel is not None
            with pytest.raises(KeyError, match='ssim_weight'):
                make(kind, {})
        with pytest.raises(NotImplementedError):
            make('l3_ssim', opt)
        with pytest.raises(NotImplementedError):
            make('cosine', opt)
    assert isinstance(_criterion('l1_ssim', opt, dev).pixel, PixelLoss) and _criterion('l1_ssim', opt, dev).pixel.kind == 'l1'
    assert isinstance(pixel_criterion('l2_ssim', dev, opt).pixel, torch.nn.MSELoss)
    for kind in ('ssim', 'l1_ssim', 'l2_ssim'):        # the models key other behaviour on these substrings
        assert 'local_global' not in kind and 'latency' not in kind


def test_ssim_criterion_has_no_fused_training_step():
    """FusedIspStep computes MSE / L1 inside its kernel: any SSIM criterion must leave it to the op-by-op path"""
    from reconfigisp_amd.codes.models.isp_model import pixel_criterion
    from reconfigisp_amd.train_step import FusedIspStep
    for kind in ('ssim', 'l1_ssim', 'l2_ssim'):
        cri = pixel_criterion(kind, torch.device('cpu'), {'ssim_weight': 0.5})
        assert FusedIspStep.build(object(), cri, object()) is None


def test_cpu_tensors_and_small_images_are_rejected():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.utils import util
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.ssim(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.ssim_loss(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        util.ssim_tensors(torch.rand(3, 16, 16), torch.rand(3, 16, 16))
    with pytest.raises((ValueError, RuntimeError), match='H=6 W=16'):
        F.ssim(torch.rand(1, 3, 6, 16), torch.rand(1, 3, 6, 16))
    with pytest.raises((ValueError, RuntimeError), match='shape'):
        F.ssim(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 17))


def test_get_ssim_keeps_the_reference_signature():
    import inspect
    from reconfigisp_amd.codes.utils import util_path_restore as U
    assert list(inspect.signature(U.get_ssim).parameters) == ['x', 'y']
    with pytest.raises(ValueError, match='Invalid data'):
        U.get_ssim(np.zeros((8, 8)), np.zeros((8, 8)))
    with pytest.raises(ValueError, match='data range 0'):      # refused before anything is sent to a device
        U.get_ssim(np.full((8, 8, 3), 7, np.uint8), np.zeros((8, 8, 3), np.uint8))
