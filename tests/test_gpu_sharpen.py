"""``functional.bgr8_sharpen`` (``risp_bgr8_sharpen``, one launch) against the numpy restatement of include/risp.h
(tests/sharpen_reference.py), byte for byte: both radii and channel orders at the sizes around the kernel's 64 x 16 tile, images
and outputs at odd byte addresses, bytes around ``out`` left alone, the extremes of every parameter, the NV12 store against
tests/nv12_reference.py of the reference's codes, and the refusals."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv12_reference as NR  # noqa: E402
from bgr8_placement import _at_odd_address, _guards_intact  # noqa: E402
import sharpen_reference as SR  # noqa: E402

pytestmark = pytest.mark.gpu

_WANT = {}


def _want(case):
    """the reference's bytes of a case, computed once"""
    if case['name'] not in _WANT:
        _WANT[case['name']] = SR.sharpen(SR.case_image(case), case['params'], case['channels'])
    return _WANT[case['name']]


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


@pytest.mark.parametrize('case', SR.CASES, ids=[c['name'] for c in SR.CASES])
def test_every_case_byte_for_byte(case):
    import reconfigisp_amd.functional as F
    img = SR.case_image(case)
    want = torch.from_numpy(_want(case)).cuda()
    dev = torch.from_numpy(img).cuda()
    got, calls = _counted(lambda: F.bgr8_sharpen(dev, case['params'], channels=case['channels']))
    assert calls == {'risp_bgr8_sharpen': 1}
    assert got.shape == dev.shape and torch.equal(got, want), '%d bytes differ' % (got != want).sum().item()
    assert torch.equal(dev, torch.from_numpy(img).cuda()), 'the input was written'
    # the same bits from a second call, and a single (H,W,3) image
    assert torch.equal(F.bgr8_sharpen(dev, case['params'], channels=case['channels']), got)
    assert torch.equal(F.bgr8_sharpen(dev[1], case['params'], channels=case['channels']), want[1])
    # img and out at odd byte addresses inside larger buffers whose other bytes must survive
    for off_in, off_out in ((1, 3), (3, 2), (2, 1)):
        src, _ = _at_odd_address(dev, off_in)
        out, buf = _at_odd_address(tuple(dev.shape), off_out)
        assert src.data_ptr() % 4 == off_in % 4 and out.data_ptr() % 4 == off_out % 4
        assert F.bgr8_sharpen(src, case['params'], channels=case['channels'], out=out) is out
        assert torch.equal(out, want), (off_in, off_out, (out != want).sum().item())
        assert _guards_intact(buf, out), 'bytes outside out were written'


@pytest.mark.parametrize('size', SR.NV12_SIZES, ids=['%dx%d' % s for s in SR.NV12_SIZES])
def test_the_nv12_store_is_the_conversion_of_the_sharpened_codes(size):
    import reconfigisp_amd.functional as F
    h, w = size
    case = dict(size=size, seed=700 + h)
    img = SR.case_image(case)
    dev = torch.from_numpy(img).cuda()
    for radius in SR.RADII:
        for matrix, channels in zip(SR.NV12_MATRICES, ('bgr', 'rgb')):
            params = (512, 3, 64, radius)
            codes = SR.sharpen(img, params, channels)
            want = torch.from_numpy(NR.nv12(codes, NR.TABLE[matrix], channels)).cuda()
            got, calls = _counted(lambda: F.bgr8_sharpen(dev, params, nv12=matrix, channels=channels))
            assert calls == {'risp_bgr8_sharpen': 1}
            assert tuple(got.shape) == (SR.N_IMAGES, h + h // 2, w) and torch.equal(got, want), (radius, matrix)
            assert torch.equal(got, F.bgr8_to_nv12(F.bgr8_sharpen(dev, params, channels=channels), matrix, channels))
            assert torch.equal(F.bgr8_sharpen(dev[2], params, nv12=NR.TABLE[matrix], channels=channels), want[2])
            # an NV12 image at an odd address (the byte stores), its surroundings left alone
            src, _ = _at_odd_address(dev, 1)
            out, buf = _at_odd_address(tuple(want.shape), 3)
            F.bgr8_sharpen(src, params, nv12=matrix, channels=channels, out=out)
            assert torch.equal(out, want)
            assert out.data_ptr() - buf.data_ptr() == 3 and _guards_intact(buf, out)


def test_refusals():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    dev = torch.zeros((2, 6, 8, 3), dtype=torch.uint8, device='cuda')
    params = (256, 4, 40, 2)
    with pytest.raises(RuntimeError, match='CUDA/HIP'):
        F.bgr8_sharpen(dev.cpu(), params)
    both = torch.zeros(2 * dev.numel(), dtype=torch.uint8, device='cuda')
    src = both[:dev.numel()].view(dev.shape)
    for start in (0, 1, dev.numel() - 1):
        _, calls = _counted(lambda: pytest.raises(ValueError, F.bgr8_sharpen, src, params,
                                                  out=both[start:start + dev.numel()].view(dev.shape)).match('shares memory'))
        assert calls == {}
    assert F.bgr8_sharpen(src, params, out=both[dev.numel():].view(dev.shape)) is not None      # adjacent is not overlapping
    for kw, what in ((dict(out=torch.zeros((2, 6, 8, 3), dtype=torch.uint8)), 'out must be'),
                     (dict(out=torch.zeros((2, 6, 9, 3), dtype=torch.uint8, device='cuda')), 'out must be'),
                     (dict(nv12='bt601_full', out=torch.zeros((2, 6, 8, 3), dtype=torch.uint8, device='cuda')), 'out must be'),
                     (dict(nv12='bt2020'), 'matrix')):
        with pytest.raises(ValueError, match=what):
            F.bgr8_sharpen(dev, params, **kw)
    with pytest.raises(ValueError, match='4:2:0'):
        F.bgr8_sharpen(dev[:, :5], params, nv12='bt601_full')
    # the C entry refuses what the wrapper would have: the library's error code, nothing launched
    out = torch.zeros_like(dev)
    p = lambda t: t.data_ptr()      # noqa: E731
    lib = L.load()
    for args in ((p(dev), p(out), None, 0, 3, 256, 4, 40, 2, 6, 8), (p(dev), p(out), None, 0, 2, 4096, 4, 40, 2, 6, 8),
                 (p(dev), p(out), None, 0, 2, 256, 256, 40, 2, 6, 8), (p(dev), p(out), None, 0, 2, 256, 4, -1, 2, 6, 8),
                 (p(dev), p(dev) + 5, None, 0, 2, 256, 4, 40, 2, 6, 8), (p(dev), None, None, 0, 2, 256, 4, 40, 2, 6, 8),
                 (p(dev), p(out), None, 0, 2, 256, 4, 40, 65536, 6, 8), (p(dev), p(out), None, 0, 2, 256, 4, 40, 2, 0, 8)):
        assert lib.risp_bgr8_sharpen(*args, None) != 0, args
    torch.cuda.synchronize()
    assert int(out.sum()) == 0
