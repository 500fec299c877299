"""CPU: the checks the output-stage wrappers of ``functional`` share (bgr8_to_nv12, bgr8_resize, bgr8_warp, bgr8_sharpen, and the
4:2:0 check and coefficient array of the serve_*_nv12 wrappers), each stated once there: what they accept, what they return, the
exact text of what they refuse, and the order in which each wrapper refuses.  Nothing here needs a device: a CPU tensor passes
every check in front of the one that asks for the device."""
import ctypes as C
import re

import pytest
import torch


def _refused(text):
    return pytest.raises(ValueError, match='^' + re.escape(text) + '$')


def _img(*shape, dtype=torch.uint8):
    return torch.zeros(shape, dtype=dtype)


WARP = (torch.zeros((2, 2, 2), dtype=torch.int32), 8, (6, 8), 'bilinear')      # a good warp of any image to 6 x 8


def test_the_image_check():
    import reconfigisp_amd.functional as F
    assert F._bgr8_images(_img(2, 6, 8, 3)) == (2, 6, 8, (2,))
    assert F._bgr8_images(_img(6, 8, 3)) == (1, 6, 8, ())
    assert F._bgr8_images(_img(5, 6, 8, 3)[::2, :, ::2]) == (3, 6, 4, (3,))        # any strides: made contiguous later
    text = 'expected (N,H,W,3) or (H,W,3) uint8 images, got %s %s'
    for bad in (_img(2, 6, 8, 3, dtype=torch.int8), _img(2, 6, 8, 3, dtype=torch.float32), _img(2, 6, 8, 4), _img(8, 3),
                _img(1, 2, 6, 8, 3)):
        with _refused(text % (bad.dtype, tuple(bad.shape))):
            F._bgr8_images(bad)
    for bad in (None, [[[0, 0, 0]]], 'img'):
        with _refused(text % (type(bad), ())):
            F._bgr8_images(bad)


def test_the_batch_asks_for_the_device_then_for_at_most_65535_images(monkeypatch):
    import reconfigisp_amd.functional as F
    img = _img(3, 6, 8, 3)[::2]
    with pytest.raises(RuntimeError, match='img must be a CUDA/HIP tensor'):
        F._bgr8_batch(img, 65536)                               # the device first
    monkeypatch.setattr(F, '_need_gpu', lambda t, what='tensor': None)
    got = F._bgr8_batch(img, 65535)
    assert got.is_contiguous() and torch.equal(got, img) and F._bgr8_batch(got, 2) is got
    with _refused('65536 images in one call: at most 65535'):
        F._bgr8_batch(img, 65536)


def test_the_channels_check():
    import reconfigisp_amd.functional as F
    assert F._channels('bgr') == 0 and F._channels('rgb') == 1 and type(F._channels('rgb')) is int
    for bad in ('gbr', 'RGB', None, 0, ('bgr',)):
        with _refused("channels %r: 'bgr' or 'rgb'" % (bad,)):
            F._channels(bad)


def test_the_420_check():
    import reconfigisp_amd.functional as F
    for h, w in ((2, 2), (4, 68), (0, 4)):
        assert F._check_420(h, w) is None
    assert F._check_420(2, 2, least=2) is None
    for h, w in ((3, 4), (4, 5), (1, 1)):
        with _refused('a %d x %d image has no 4:2:0 form: H and W must be even' % (h, w)):
            F._check_420(h, w)
    with _refused('a 0 x 4 image has no 4:2:0 form: H and W must be even'):
        F._check_420(0, 4, least=2)
    # the same check in the words of the callers that name other sizes
    with _refused('a 9 x 18 output has no 4:2:0 form: OH and OW must be even'):
        F.resize_check((9, 18), None, 'triangle', 24, 40, nv12=True)
    assert F.resize_check((9, 18), None, 'triangle', 24, 40) == ((9, 18), (0, 0, 24, 40))
    with _refused('a 6 x 7 warp output has no 4:2:0 form: WH and WW must be even'):
        F.warp_check(WARP[:2] + ((6, 7), 'bilinear'), 12, 16, nv12=True)
    with _refused('reverse_channels has no meaning with a yuv matrix: the conversion knows the channel order'):
        F._packed_out('bt601_full', True, None, 1, 3, 4, torch.device('cpu'))
    with _refused('a 3 x 4 image has no 4:2:0 form: H and W must be even'):
        F._packed_out('bt601_full', False, None, 1, 3, 4, torch.device('cpu'))


def test_the_coefficient_array():
    import reconfigisp_amd.functional as F
    assert F._coef12(None) is None
    coef = F.nv12_matrix('bt709_video')
    arr = F._coef12(coef)
    assert isinstance(arr, C.c_int * 12) and tuple(arr) == coef
    arr, out = F._packed_out('bt709_video', False, None, 2, 4, 8, torch.device('cpu'))
    assert tuple(arr) == coef and tuple(out.shape) == (2, 6, 8) and out.dtype == torch.uint8
    assert F._packed_out(None, True, None, 2, 4, 8, torch.device('cpu'))[0] is None


def test_the_output_kept_apart_from_the_images():
    import reconfigisp_amd.functional as F
    big, cpu = torch.zeros(400, dtype=torch.uint8), torch.device('cpu')
    img = big[100:100 + 96].view(2, 4, 4, 3)
    new = F._u8_out(None, (2, 2, 2, 3), cpu, 1, img, 'rows')
    assert new.dtype == torch.uint8 and tuple(new.shape) == (2, 2, 2, 3) and new.device == cpu
    for start in (100 - 24, 196):                               # ends where the images begin, begins where they end
        out = big[start:start + 24].view(2, 2, 2, 3)
        assert F._u8_out(out, (2, 2, 2, 3), cpu, 1, img, 'rows') is out
    for what in ('rows', 'pixels'):
        for start in (100 - 23, 100, 150, 195):                 # one byte shared is shared
            out = big[start:start + 24].view(2, 2, 2, 3)
            with _refused('out shares memory with the images: a tile reads %s other tiles would have overwritten' % what):
                F._u8_out(out, (2, 2, 2, 3), cpu, 1, img, what)
            assert F._u8_out(out, (2, 2, 2, 3), cpu, 1) is out      # nothing to keep apart from
    # what _u8_out refuses is refused first, in its words
    assert big.data_ptr() % 4 == 0
    for bad, align in ((big[101:125].view(2, 2, 2, 3), 4), (big[100:124].view(2, 2, 6), 1), (big[100:124].view(torch.int8).view(2, 2, 2, 3), 1),
                       (big[100:148:2].view(2, 2, 2, 3), 1), (torch.zeros((2, 2, 2, 3), dtype=torch.uint8, device='meta'), 1)):
        with _refused('out must be a contiguous uint8 (2, 2, 2, 3) tensor on cpu, %d-byte aligned; got %s %s'
                      % (align, bad.dtype, tuple(bad.shape))):
            F._u8_out(bad, (2, 2, 2, 3), cpu, align, img, 'rows')


def test_bgr8_to_nv12_asks_for_the_device_first():
    import reconfigisp_amd.functional as F
    for img, kw in ((_img(2, 5, 8, 3, dtype=torch.float32), dict(channels='gbr')), (_img(2, 6, 8, 3), dict(matrix='bt2020')), (None, {})):
        with pytest.raises(RuntimeError, match='img must be a CUDA/HIP tensor'):
            F.bgr8_to_nv12(img, **kw)


def test_bgr8_resize_refuses_in_its_order():
    import reconfigisp_amd.functional as F
    good = _img(2, 24, 40, 3)
    with pytest.raises(ValueError, match='^expected '):          # wrong dtype and bad channels
        F.bgr8_resize(good.float(), (10, 18), channels='gbr')
    with pytest.raises(ValueError, match='^channels '):          # bad channels and an unknown matrix
        F.bgr8_resize(good, (10, 18), channels='gbr', nv12='bt2020')
    with pytest.raises(ValueError, match='^unknown yuv matrix'):    # an unknown matrix and an unknown kernel
        F.bgr8_resize(good, (10, 18), nv12='bt2020', resample='lanczos')
    with pytest.raises(ValueError, match='^channels '):          # bad channels and an odd size
        F.bgr8_resize(good, (9, 18), channels='gbr', nv12='bt601_full')
    with pytest.raises(ValueError, match='has no 4:2:0 form'):   # an odd size, on the host
        F.bgr8_resize(good, (9, 18), nv12='bt601_full')
    with pytest.raises(RuntimeError, match='img must be a CUDA/HIP tensor'):      # every argument right: the device is asked for last
        F.bgr8_resize(good, (10, 18), nv12='bt601_full', out=torch.zeros(3))


def test_bgr8_sharpen_refuses_in_its_order():
    import reconfigisp_amd.functional as F
    good, params = _img(2, 5, 8, 3), (256, 4, 40, 2)
    with pytest.raises(ValueError, match='^expected '):
        F.bgr8_sharpen(good[..., :2], params, channels='gbr')
    with pytest.raises(ValueError, match='^channels '):          # bad channels and an odd size
        F.bgr8_sharpen(good, params, nv12='bt601_full', channels='gbr')
    with pytest.raises(ValueError, match='^a yuv matrix is'):    # a bad matrix and a bad sharpening
        F.bgr8_sharpen(good, (256, 4, 40, 3), nv12=(1, 2, 3))
    with pytest.raises(ValueError, match='^sharpen radius 3'):   # a bad sharpening and an odd size
        F.bgr8_sharpen(good, (256, 4, 40, 3), nv12='bt601_full')
    with pytest.raises(ValueError, match='^sharpening into NV12 with H = 5'):
        F.bgr8_sharpen(good, params, nv12='bt601_full')
    with pytest.raises(RuntimeError, match='img must be a CUDA/HIP tensor'):
        F.bgr8_sharpen(good, params, out=torch.zeros(3))


def test_bgr8_warp_refuses_in_its_order():
    import reconfigisp_amd.functional as F
    good = _img(2, 12, 16, 3)
    with pytest.raises(ValueError, match='^expected '):          # wrong rank and no warp
        F.bgr8_warp(good[0, 0], None, stage='both')
    with pytest.raises(ValueError, match='^a warp is '):         # no warp and a bad stage
        F.bgr8_warp(good, None, stage='both')
    with pytest.raises(ValueError, match='^warp stage '):        # a bad stage, on the host
        F.bgr8_warp(good, WARP, stage='both')
    for stage in (None, 0, 'lds'):
        with pytest.raises(RuntimeError, match='img must be a CUDA/HIP tensor'):
            F.bgr8_warp(good, WARP, stage=stage, out=torch.zeros(3))
