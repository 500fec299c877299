"""MIPI-packed RAW10 / RAW12, no GPU: the byte vectors of include/risp.h, that tests/raw_packed_reference.py inverts itself and
ignores padding, that the frames tests/test_gpu_serve_packed.py serves tell the definition from three wrong ones in the served
bytes (tests/serve_reference.py, float64), ``pipeline_fusion.serve_load`` over every route and format, and the refusals of
``serve(raw_format=...)`` that need no device."""
import numpy as np
import pytest
import torch

import raw_packed_reference as PR
import reconfigisp_amd.functional as F
import serve_reference as SR
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF

VECTORS = {10: ([0x3FF, 0x000, 0x155, 0x2AA], [0xFF, 0x00, 0x55, 0xAA, 0x93]),
           12: ([0xABC, 0x123, 0xABC, 0x123], [0xAB, 0x12, 0x3C, 0xAB, 0x12, 0x3C])}


@pytest.mark.parametrize('bits', [10, 12])
def test_the_byte_vectors_of_the_header(bits):
    pixels, data = VECTORS[bits]
    assert PR.pack(np.array([pixels]), bits).tolist() == [data]
    assert PR.unpack(np.array([data], dtype=np.uint8), bits, 4).tolist() == [pixels]


def test_the_package_table():
    assert F.RAW_FORMAT == {'u16': 0, 'raw10': 10, 'raw12': 12}
    assert [F.raw_format_bits(k) for k in ('u16', 'raw10', 'raw12')] == [0, 10, 12]
    with pytest.raises(ValueError, match='raw14'):
        F.raw_format_bits('raw14')


@pytest.mark.parametrize('bits', [10, 12])
@pytest.mark.parametrize('w', [4, 8, 12])
def test_round_trip_and_padding(bits, w):
    x = PR.full_range_frame(2, 3, w, bits, seed=bits + w)
    used = w * bits // 8
    for stride in (used, used + 3):
        want = None
        for pad in (0x00, 0xFF, None):
            data = PR.pack(x, bits, stride, pad)
            assert data.dtype == np.uint8 and data.shape == (2, 3, stride)
            assert np.array_equal(PR.unpack(data, bits, w), x)
            assert want is None or np.array_equal(data[..., :used], want), 'the padding changed the payload'
            want = data[..., :used]
        if stride > used:
            assert (PR.pack(x, bits, stride, 0xFF)[..., used:] == 0xFF).all()
            assert not np.array_equal(PR.pack(x, bits, stride, None), PR.pack(x, bits, stride, 0))


def _served(frame, white, demosaic):
    return SR.serve(frame, float(white), 0, 'rggb', demosaic, None, [], []).bytes


@pytest.mark.parametrize('demosaic', ['nearest', 'bilinear'])
@pytest.mark.parametrize('bits', [10, 12])
def test_the_low_bit_frame_shows_a_mishandled_low_byte(bits, demosaic):
    """the condition that lets the GPU test see a kernel that drops or permutes the low bits"""
    h, w = 6, 12
    x = PR.low_bit_frame(1, h, w, seed=20 + bits)
    assert x.max() == 15 and len(np.unique(x)) == 16
    data = PR.pack(x, bits)
    if bits == 12:
        assert (data.reshape(1, h, w // 2, 3)[..., :2] == 0).all(), 'every high byte is 0'
    right = _served(PR.unpack(data, bits, w), 15, demosaic)
    assert np.array_equal(right, _served(x, 15, demosaic))
    for wrong in (PR.unpack_drop_low, PR.unpack_swapped_low):
        assert (_served(wrong(data, bits, w), 15, demosaic) != right).any(), wrong.__name__


@pytest.mark.parametrize('demosaic', ['nearest', 'bilinear'])
@pytest.mark.parametrize('bits', [10, 12])
def test_the_full_range_frame_shows_a_neighbours_high_byte(bits, demosaic):
    h, w = 6, 12
    white = (1 << bits) - 1
    x = PR.full_range_frame(1, h, w, bits, seed=30 + bits)
    assert x.max() == white and x.min() == 0
    data = PR.pack(x, bits)
    right = _served(PR.unpack(data, bits, w), white, demosaic)
    assert (_served(PR.unpack_neighbour_high(data, bits, w), white, demosaic) != right).any()


def test_serve_load_over_every_route_and_format():
    assert PF.SERVE_ROUTES == ('fused', 'classical', 'scene', 'denoise', 'denoise_scene', 'cond', 'composed', 'tiled')
    for route in PF.SERVE_ROUTES:
        assert PF.serve_load(route, 'u16') is None
        for fmt in ('raw10', 'raw12'):
            load = PF.serve_load(route, fmt)
            if route in ('fused', 'classical'):
                # the measurement decides (profiles/serve_packed.txt): the table is the only source
                assert load == ('fused' if (route, fmt) in PF._FUSED_LOAD else 'pass')
            else:
                assert load == 'pass', (route, fmt)
    assert PF._FUSED_LOAD <= {(r, f) for r in ('fused', 'classical') for f in ('raw10', 'raw12')}
    with pytest.raises(ValueError, match='raw8'):
        PF.serve_load('fused', 'raw8')
    with pytest.raises(ValueError, match='direct'):
        PF.serve_load('direct', 'raw10')


def test_serve_load_is_what_the_measurement_shows():
    """the rule: a route keeps its fused load for a format only where profiles/serve_packed.txt has it beat the unpack launch
    followed by the uint16 call by more than the spread on the 3000 x 4000 frame"""
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'serve_packed.txt')
    lines = open(path).read().splitlines()
    pairs = lambda text: {tuple(k.strip().split('/')) for k in text.split(',') if '/' in k}
    won = [ln.split('for:')[1] for ln in lines if 'beats unpack + uint16 by more than the spread for:' in ln]
    lost = [ln.split('for:')[1] for ln in lines if 'and does not for:' in ln]
    assert len(won) == 1 and len(lost) == 1
    assert pairs(won[0]) | pairs(lost[0]) == {(r, f) for r in ('fused', 'classical') for f in ('raw10', 'raw12')}
    assert PF._FUSED_LOAD == pairs(won[0])


def test_packed_width():
    assert F.packed_width(10, 20) == 16 and F.packed_width(12, 24) == 16 and F.packed_width(10, 64, 48) == 48
    assert F.packed_width(10, 23, 16) == 16 and F.packed_width(12, 6) == 4
    for bits, stride, width, names in ((10, 19, 16, '16'), (12, 23, 16, '16'), (10, 20, 6, '6'), (10, 20, 0, '0'),
                                       (10, 23, None, '18'), (12, 3, None, '2'), (8, 16, 16, '8')):
        with pytest.raises(ValueError, match=names):
            F.packed_width(bits, stride, width)


def test_the_keywords_exist_on_every_entry():
    import inspect
    from reconfigisp_amd.codes.models.isp_model import IspModel
    from reconfigisp_amd.codes.models.modules.isp_universal import IspUniversal
    from reconfigisp_amd.codes.models.modules.origin_universal import OriginUniversal
    for cls in (PF, IspUniversal, OriginUniversal, IspModel):
        for fn in (cls.serve, cls.serve_frame):
            par = inspect.signature(fn).parameters
            assert par['raw_format'].default == 'u16' and par['raw_format'].kind is inspect.Parameter.KEYWORD_ONLY, fn
            assert par['raw_width'].default is None and par['raw_width'].kind is inspect.Parameter.KEYWORD_ONLY, fn


@pytest.mark.parametrize('entry', ['serve', 'serve_frame'])
def test_host_side_refusals_come_before_the_device(entry):
    """host tensors throughout: each refusal is raised, and names the value, before anything asks for a device"""
    def call(raw, **kw):
        if entry == 'serve':
            return PF.serve([], [], raw, 1023.0, **kw)
        return PF.serve_frame([], [], raw, 1023.0, 32, 24, **kw)

    good = torch.zeros((2, 4, 20), dtype=torch.uint8)
    with pytest.raises(ValueError, match='raw14'):
        call(good, raw_format='raw14')
    with pytest.raises(ValueError, match='uint16'):
        call(torch.zeros((2, 4, 20), dtype=torch.uint16), raw_format='raw10')
    with pytest.raises(ValueError, match='float32'):
        call(good.float(), raw_format='raw12')
    with pytest.raises(ValueError, match='raw10'):
        call(good[0, 0], raw_format='raw10')                # one dimension
    with pytest.raises(ValueError, match='6'):
        call(good, raw_format='raw10', raw_width=6)
    with pytest.raises(ValueError, match='20'):
        call(good, raw_format='raw10', raw_width=20)        # 25 bytes per row, the rows have 20
    with pytest.raises(ValueError, match='13'):
        call(good, raw_format='raw12')                      # rows of 20 bytes hold 13 samples: the width has to be given
    with pytest.raises(ValueError, match='3 rows'):
        call(good[:, :3], raw_format='raw10')
    # what is left needs the device: the well-formed call gets as far as asking for it
    with pytest.raises(RuntimeError, match='GPU-only'):
        call(good, raw_format='raw10', raw_width=16)
    with pytest.raises(RuntimeError, match='GPU-only'):
        F.raw_unpack(good, 10)
    with pytest.raises(RuntimeError, match='GPU-only'):
        F.serve_packed(good, 10, None, 1023.0, [], [])
    with pytest.raises(RuntimeError, match='GPU-only'):
        F.serve_classical_packed(good, 12, 12, 4095.0, 'bilinear', [], [])
