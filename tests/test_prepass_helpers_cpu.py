"""CPU: the checks the sensor pre-pass wrappers of ``functional`` share (raw_unpack, raw_shade, raw_defect, raw_temporal,
raw_stats), each stated once there: what they accept, what they return and the exact text of what they refuse.  Nothing here needs
a device; the frames themselves are checked on the GPU (a CPU tensor is refused before anything else is looked at, as before)."""
import re

import numpy as np
import pytest
import torch


def _refused(text):
    return pytest.raises(ValueError, match='^' + re.escape(text) + '$')


def test_the_black_level_check():
    import reconfigisp_amd.functional as F
    for good, want in ((0, 0), (65535, 65535), (64.0, 64), (np.int64(256), 256)):
        got = F._black_level(good)
        assert got == want and type(got) is int
    for bad in (-1, 65536, 1.5, -0.5):
        with _refused('black_level %r: an integer in 0 .. 65535' % (bad,)):
            F._black_level(bad)
        with _refused('black_level %r: an integer in 0 .. 65535' % (bad,)):
            F._sensor(bad, 'rggb')
    assert F._sensor(64.0, 'BGGR') == (64, 3)
    with pytest.raises(ValueError, match='unknown cfa'):       # the phase is looked at first
        F._sensor(-1, 'rgbg')


def test_the_shading_cell_check():
    import reconfigisp_amd.functional as F
    for k in range(2, 9):
        assert F._shading_cell(1 << k) == k
    good = torch.zeros((4, 6, 4), dtype=torch.uint16)
    for bad in (3, 2, 512, 0, -4, 16.0, True, None, '16'):
        text = 'lens shading cell %r: a power of two from 4 to 256' % (bad,)
        with _refused(text):
            F._shading_cell(bad)
        with _refused(text):
            F.shading_check((good, bad), 34, 68)
        with _refused(text):
            F.shading_map(np.ones((2, 2)), 34, 68, bad)
    assert tuple(F.shading_map(np.ones((2, 2)), 34, 68, 16).shape) == (4, 6, 4)


def test_the_same_device_check():
    import reconfigisp_amd.functional as F
    t = torch.zeros(4)
    for device in (None, torch.device('cpu'), 'cpu'):
        F._on_frames_device(t, device, 'the defect map lives')
    for device in (torch.device('meta'), 'meta'):
        with _refused('the defect map lives on cpu, the frames on meta'):
            F._on_frames_device(t, device, 'the defect map lives')
    with _refused('lens shading gains live on cpu, the frames on meta'):
        F._on_frames_device(t, torch.device('meta'), 'lens shading gains live')
    st = F.RawStatistics(1, 8, 16, zone=(4, 8), bins=16, device='cpu')
    with _refused('statistics.zones lives on cpu, the frames on meta'):
        F.stats_check(st, 1, 8, 16, torch.device('meta'))


def test_the_uint16_output():
    import reconfigisp_amd.functional as F
    cpu = torch.device('cpu')
    new = F._u16_out(None, (2, 4, 8), cpu)
    assert new.dtype == torch.uint16 and tuple(new.shape) == (2, 4, 8) and new.device == cpu and new.is_contiguous()
    big = torch.zeros(2 * 4 * 8 + 8, dtype=torch.uint16)
    assert big.data_ptr() % 8 == 0
    out = big[4:4 + 64].view(2, 4, 8)
    assert F._u16_out(out, (2, 4, 8), cpu) is out
    for bad in (big[1:1 + 64].view(2, 4, 8),                   # 2-byte aligned only
                out.view(torch.int16), out[:, :, ::2], out.view(4, 2, 8), torch.zeros((2, 4, 8), dtype=torch.uint16, device='meta')):
        with _refused('out must be a contiguous uint16 (2, 4, 8) tensor on cpu, 8-byte aligned; got %s %s'
                      % (bad.dtype, tuple(bad.shape))):
            F._u16_out(bad, (2, 4, 8), cpu)
    # memory shared with what the launch reads: the frames in their own element size, any one of the pairs
    frames, state = big[8:8 + 64].view(2, 4, 8), torch.zeros((2, 4, 8), dtype=torch.uint16)
    packed = big.view(torch.uint8)[2 * 68 - 1:2 * 68 + 9]       # begins at the last byte of out
    text = 'out shares memory with %s: the %s reads neighbours other threads would have overwritten'
    with _refused(text % ('the frames', 'correction')):
        F._u16_out(out, (2, 4, 8), cpu, ((frames, 'the frames'),), 'correction')
    with _refused(text % ('the frames', 'correction')):
        F._u16_out(out, (2, 4, 8), cpu, ((packed, 'the frames'),), 'correction')
    with _refused(text % ('the temporal state', 'filter')):
        F._u16_out(out, (2, 4, 8), cpu, ((state, 'the frames'), (frames, 'the temporal state')), 'filter')
    apart = big.view(torch.uint8)[2 * 68:]                      # begins where out ends
    assert F._u16_out(out, (2, 4, 8), cpu, ((state, 'the frames'), (apart, 'the temporal state')), 'filter') is out


def test_the_frames_are_asked_for_their_device_first():
    """a CPU tensor is refused for being there, whatever else is wrong with it: no wrapper reads a shape before that"""
    import reconfigisp_amd.functional as F
    wrong = torch.zeros((2, 3), dtype=torch.float32)
    for bits, kw, what in ((16, {}, 'frames'), (10, {}, 'frames'), (12, dict(u16=False), 'packed')):
        with pytest.raises(RuntimeError, match='%s must be a CUDA/HIP tensor' % what):
            F._raw_frames(wrong, bits, None, what, **kw)
    for call in (lambda: F.raw_unpack(wrong, 10), lambda: F.raw_shade(wrong, None), lambda: F.raw_defect(wrong, None),
                 lambda: F.raw_temporal(wrong, None), lambda: F.raw_stats(wrong, None)):
        with pytest.raises(RuntimeError, match='must be a CUDA/HIP tensor'):
            call()
