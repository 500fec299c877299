"""The serving path's definition of a Bayer phase and a black level, pinned without a GPU (numpy and the oracle only).

phase by mirror: a GRBG / GBRG / BGGR mosaic with even H and W is an RGGB mosaic mirrored along x / y / both, so
``serve(raw, cfa=c) == unflip_c(serve_rggb(flip_c(raw)))``.  For the nearest demosaic this must be the natural per-phase
index map - R and B replicated over their own quad, G from the pixel's own row - and that is what is checked here, on
mosaics laid out from a random RGB image.  tests/test_gpu_serve_cfa.py holds the kernels to the same definition byte for
byte."""
import numpy as np
import pytest
import torch

import isp_oracle as O

# phase -> the colour (0 R, 1 G, 2 B) at (row parity, column parity) of the mosaic
SITES = {'rggb': ((0, 1), (1, 2)), 'grbg': ((1, 0), (2, 1)), 'gbrg': ((1, 2), (0, 1)), 'bggr': ((2, 1), (1, 0))}
SIZES = [(2, 2), (4, 6), (6, 4), (10, 12)]


def _mosaic(rgb, phase):
    """(3,H,W) RGB image -> (H,W) mosaic of that phase"""
    h, w = rgb.shape[1:]
    out = np.empty((h, w), rgb.dtype)
    for py in range(2):
        for px in range(2):
            out[py::2, px::2] = rgb[SITES[phase][py][px], py::2, px::2]
    return out


def _flip(a, code):
    """mirror the last two axes: bit 0 along x, bit 1 along y (its own inverse)"""
    if code & 1:
        a = a[..., ::-1]
    if code & 2:
        a = a[..., ::-1, :]
    return np.ascontiguousarray(a)


def _natural_map(mosaic, phase):
    """the per-phase nearest demosaic written out pixel by pixel -> (3,H,W) in the oracle's B, G, R order: every pixel takes
    the R and the B site of its own quad and the green sample of its own row in that quad"""
    h, w = mosaic.shape
    out = np.empty((3, h, w), mosaic.dtype)
    for y in range(h):
        for x in range(w):
            qy, qx = y - y % 2, x - x % 2
            site = {}
            for dy in range(2):
                for dx in range(2):
                    c = SITES[phase][dy][dx]
                    if c == 1:
                        site[('g', dy)] = mosaic[qy + dy, qx + dx]
                    else:
                        site[c] = mosaic[qy + dy, qx + dx]
            out[0, y, x], out[1, y, x], out[2, y, x] = site[2], site[('g', y % 2)], site[0]
    return out


@pytest.mark.parametrize('phase', list(SITES))
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_mirror_is_the_natural_map_of_the_phase(phase, size):
    import reconfigisp_amd.functional as F
    code = F.CFA[phase]
    rgb = np.random.RandomState(17 + code + size[1]).rand(3, *size).astype(np.float32)
    mosaic = _mosaic(rgb, phase)
    # a mirrored mosaic of this phase is laid out as RGGB
    assert np.array_equal(_flip(mosaic, code), _mosaic(_flip(rgb, code), 'rggb'))
    got = O.demosaic_nearest(torch.from_numpy(_flip(mosaic, code))[None, None])[0].numpy()
    got = _flip(got, code)
    want = _natural_map(mosaic, phase)
    assert np.array_equal(got[2], want[2]), 'R is not the own quad\'s R site'
    assert np.array_equal(got[0], want[0]), 'B is not the own quad\'s B site'
    assert np.array_equal(got[1], want[1]), 'G is not the green sample of the pixel\'s own row'
    # and the sites themselves come through untouched: every sample of the mosaic is its pixel's value of its own colour
    for py in range(2):
        for px in range(2):
            c = SITES[phase][py][px]
            assert np.array_equal(got[2 - c, py::2, px::2], rgb[c, py::2, px::2])
    if phase == 'rggb':                                    # phase 0 is the oracle's own map, no mirror at all
        assert np.array_equal(want, O.demosaic_nearest(torch.from_numpy(mosaic)[None, None])[0].numpy())


def test_cfa_table_and_unknown_name():
    import reconfigisp_amd.functional as F
    assert F.CFA == {'rggb': 0, 'grbg': 1, 'gbrg': 2, 'bggr': 3}
    for name, code in F.CFA.items():                       # cfa = flip_x | flip_y << 1
        assert F.cfa_code(name) == code == (name in ('grbg', 'bggr')) | (name in ('gbrg', 'bggr')) << 1
        assert F.cfa_code(name.upper()) == code
    for bad in ('rgbg', '', 'bayer', None, 1):
        with pytest.raises(ValueError) as e:
            F.cfa_code(bad)
        assert all(name in str(e.value) for name in F.CFA), str(e.value)


def test_mirrored_axis_must_be_even():
    """a mirrored odd axis is no RGGB mosaic; with cfa 'rggb' odd sizes stay allowed (the check every serving call makes)"""
    import reconfigisp_amd.functional as F
    F._check_mirror(0, 3, 5)                               # RGGB: odd sizes stay allowed
    F._check_mirror(1, 3, 4), F._check_mirror(2, 4, 3), F._check_mirror(3, 4, 4)
    for flip, h, w in [(1, 4, 3), (2, 3, 4), (3, 3, 4), (3, 4, 3)]:
        with pytest.raises(ValueError, match='even'):
            F._check_mirror(flip, h, w)


@pytest.mark.parametrize('black,white', [(0, 1023), (64, 1023), (512, 16383), (1023, 16383), (65535 - 1, 65535)])
def test_black_level_integer_form_is_the_oracle_expression(black, white):
    """the kernels' input expression (float)(s > b ? s - b : 0) / (white - b) - an integer subtraction, one conversion and one
    fp32 division - against max(raw - b, 0) / (white - b) formed from the clamped uint16 frame the GPU oracle is fed"""
    s = np.unique(np.clip(np.concatenate([np.arange(0, 8), np.arange(black - 4, black + 5), np.arange(white - 4, white + 5),
                                          [65535, 65534, 40000], np.random.RandomState(black).randint(0, 65536, 4096)]), 0, 65535))
    s = s.astype(np.uint16)
    assert (s < black).any() or black == 0
    assert (s == black).any() and (s > white).any() or white == 65535
    div = np.float32(white - black)
    clamped = np.maximum(s.astype(np.int64) - black, 0)
    assert clamped.max() <= 65535 and np.array_equal(clamped.astype(np.uint16), clamped), 'max(raw - b, 0) is not an exact uint16'
    oracle = clamped.astype(np.uint16).astype(np.float32) / div          # what serve-as-it-is computes on the clamped frame
    si = s.astype(np.int32)
    integer_form = np.where(si > black, si - black, 0).astype(np.float32) / div
    assert np.array_equal(oracle, integer_form)
    assert np.all(integer_form[s <= black] == 0) and np.all(integer_form[s == white] == 1) and np.all(integer_form[s > white] > 1)
