"""The NV12 format definition on the CPU: the preset table, the acceptance rule, what the presets do to greys, their distance
from the float64 BT.601 / BT.709 matrices, the byte layout, and that the yardstick (tests/nv12_reference.py) tells the
plausible wrong definitions from the right one.  No GPU needed."""
import numpy as np
import pytest

import nv12_reference as NR
import reconfigisp_amd.functional as F

PRESETS = ['bt601_full', 'bt601_video', 'bt709_full', 'bt709_video']


def _lattice():
    """every (R, G, B) with codes 0, 5, .., 255, as one (1, 2, 2 * 52^3, 3) BGR image of uniform quads"""
    c = np.arange(0, 256, 5, dtype=np.uint8)
    r, g, b = [v.ravel() for v in np.meshgrid(c, c, c, indexing='ij')]
    row = np.repeat(np.stack([b, g, r], axis=1), 2, axis=0)           # each colour twice along x
    return np.stack([row, row])[None], r.astype(np.float64), g.astype(np.float64), b.astype(np.float64)


def _float_yuv(name, r, g, b):
    """the float64 matrix of the standard at the preset's range, unrounded"""
    kr, kb = (0.299, 0.114) if name.startswith('bt601') else (0.2126, 0.0722)
    y = kr * r + (1.0 - kr - kb) * g + kb * b
    u, v = (b - y) / (2.0 * (1.0 - kb)), (r - y) / (2.0 * (1.0 - kr))
    if name.endswith('video'):
        return 16.0 + y * 219.0 / 255.0, 128.0 + u * 224.0 / 255.0, 128.0 + v * 224.0 / 255.0
    return y, 128.0 + u, 128.0 + v


def test_the_package_table_is_the_reference_table():
    assert sorted(F.NV12_MATRIX) == sorted(NR.TABLE) == sorted(PRESETS)
    for name in PRESETS:
        assert tuple(F.NV12_MATRIX[name]) == tuple(NR.TABLE[name]), name
        assert tuple(F.nv12_matrix(name)) == tuple(NR.TABLE[name])
        assert tuple(F.nv12_matrix(list(NR.TABLE[name]))) == tuple(NR.TABLE[name])


def test_every_preset_passes_the_acceptance_rule_and_bad_matrices_do_not():
    for name in PRESETS:
        assert NR.accepted(NR.TABLE[name]), name
    good = list(NR.TABLE['bt601_full'])
    bad = {'overflow': [256, 256, 256, 0] + good[4:], 'negative': good[:4] + [-43, -84, 127, 0] + good[8:],
           'coefficient': [257, 0, 0, 0] + good[4:], 'offset': good[:8] + [0, 0, 0, 65536], 'eleven': good[:11]}
    for what, coef in bad.items():
        assert not NR.accepted(coef), what
        with pytest.raises(ValueError):
            F.nv12_matrix(coef)
    assert NR.accepted([256, 0, 0, 255] * 3) and tuple(F.nv12_matrix([256, 0, 0, 255] * 3)) == (256, 0, 0, 255) * 3
    for junk in ('bt2020', None, 7, [0.5] * 12, ['a'] * 12):
        with pytest.raises(ValueError):
            F.nv12_matrix(junk)


@pytest.mark.parametrize('name', PRESETS)
def test_greys(name):
    v = np.arange(256, dtype=np.uint8)
    img = np.repeat(np.repeat(v[None, None, :, None], 2, axis=1), 2, axis=2).repeat(3, axis=3)      # (1,2,512,3): quads of one grey
    out = NR.nv12(img, NR.TABLE[name])
    assert (out[0, 2] == 128).all(), 'a grey has U = V = 128'
    if name.endswith('full'):
        assert (out[0, 0, 0::2] == v).all() and (out[0, 1, 1::2] == v).all(), 'full range maps grey v to Y = v'
    else:
        assert out[0, 0, 0] == 16 and out[0, 0, -1] == 235


@pytest.mark.parametrize('name', PRESETS)
def test_presets_against_the_float64_matrices(name):
    img, r, g, b = _lattice()
    out = NR.nv12(img, NR.TABLE[name])
    y, u, v = out[0, 0, 0::2].astype(np.float64), out[0, 2, 0::2].astype(np.float64), out[0, 2, 1::2].astype(np.float64)
    fy, fu, fv = _float_yuv(name, r, g, b)
    dev = [np.abs(y - fy).max(), np.abs(u - fu).max(), np.abs(v - fv).max()]
    print('%s: largest deviation from float64 Y %.3f U %.3f V %.3f' % (name, *dev))
    assert max(dev) <= 2.0, dev
    lo, hi = ((0, 1, 1), (255, 255, 255)) if name.endswith('full') else ((16, 16, 16), (235, 240, 240))
    assert (y.min(), u.min(), v.min()) == lo and (y.max(), u.max(), v.max()) == hi


def _wrong(img, coef, what):
    r, g, b = NR.planes(img)
    y = NR.dot(coef[0:4], r, g, b)
    rm, gm, bm = NR.quad_mean(r), NR.quad_mean(g), NR.quad_mean(b)
    if what == 'uv swapped':
        return NR.pack(y, NR.dot(coef[8:12], rm, gm, bm), NR.dot(coef[4:8], rm, gm, bm))
    if what == 'mean of converted':
        return NR.pack(y, NR.quad_mean(NR.dot(coef[4:8], r, g, b)), NR.quad_mean(NR.dot(coef[8:12], r, g, b)))
    if what == 'truncated mean':
        rm, gm, bm = [(c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2]) >> 2 for c in (r, g, b)]
    if what == 'top left':
        rm, gm, bm = r[:, 0::2, 0::2], g[:, 0::2, 0::2], b[:, 0::2, 0::2]
    return NR.pack(y, NR.dot(coef[4:8], rm, gm, bm), NR.dot(coef[8:12], rm, gm, bm))


@pytest.mark.parametrize('what', ['uv swapped', 'mean of converted', 'truncated mean', 'top left'])
def test_wrong_definitions_differ_from_the_reference(what):
    img = np.random.RandomState(12).randint(0, 256, (2, 8, 12, 3)).astype(np.uint8)
    for name in PRESETS:
        coef = NR.TABLE[name]
        want, got = NR.nv12(img, coef), _wrong(img, coef, what)
        assert np.array_equal(want[:, :8], got[:, :8]) and not np.array_equal(want[:, 8:], got[:, 8:]), (what, name)


def test_layout_of_a_4_x_4_image():
    """bt601_full, by hand.  Quads: white | red over black | one red-and-a-little-green pixel beside a little green.
    white: Y (256*255 + 128) >> 8 = 255, U = V = 32896 >> 8 = 128.  red: Y (77*255 + 128) >> 8 = 77, U (32896 - 43*255) >> 8 = 85,
    V (127*255 + 32896) >> 8 = 255.  black: Y 0, U = V = 128.  The last quad has R codes 255, 0, 0, 0 -> Rm (255 + 2) >> 2 = 64
    (63 truncated) and G codes 1, 1, 0, 0 -> Gm (2 + 2) >> 2 = 1 (0 truncated): Y (77*255 + 150 + 128) >> 8 = 77 and
    (150 + 128) >> 8 = 1, U (32896 - 43*64 - 84) >> 8 = 117, V (127*64 - 106 + 32896) >> 8 = 159."""
    W_, R_, K_ = (255, 255, 255), (0, 0, 255), (0, 0, 0)          # B, G, R
    img = np.array([[[W_, W_, R_, R_],
                     [W_, W_, R_, R_],
                     [K_, K_, (0, 1, 255), (0, 1, 0)],
                     [K_, K_, K_, K_]]], dtype=np.uint8)
    want = np.array([[[255, 255, 77, 77],
                      [255, 255, 77, 77],
                      [0, 0, 77, 1],
                      [0, 0, 0, 0],
                      [128, 128, 85, 255],
                      [128, 128, 117, 159]]], dtype=np.uint8)
    got = NR.nv12(img, NR.TABLE['bt601_full'])
    assert got.shape == (1, 6, 4) and got.dtype == np.uint8 and np.array_equal(got, want), got
    assert np.array_equal(NR.nv12(img[..., ::-1].copy(), NR.TABLE['bt601_full'], channels='rgb'), want)
