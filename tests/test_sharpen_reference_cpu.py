"""Output sharpening without a GPU: the definition (tests/sharpen_reference.py) against vectors worked by hand, its identities and
its arithmetic bound, what each deliberate mistake of the reference changes on the GPU tests' own inputs, that those inputs meet
everything the definition provides for, and the plumbing - host refusals, keywords, header, verdict table."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sharpen_reference as SR  # noqa: E402
from serve_verdicts import read_verdict  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gray(values):
    v = np.asarray(values, dtype=np.uint8)
    return np.repeat(v[..., None], 3, axis=-1)


def _spot():
    """7 x 7, gray 100 with one pixel of 200 in the middle: L is the gray value, (256 v + 128) >> 8 = v"""
    img = np.full((7, 7), 100, dtype=np.uint8)
    img[3, 3] = 200
    return _gray(img)


# ---------------------------------------------------------------- vectors worked by hand
@pytest.mark.parametrize('radius', SR.RADII)
def test_a_flat_image_is_unchanged(radius):
    img = np.full((5, 6, 3), 0, dtype=np.uint8)
    img[...] = (10, 200, 77)
    assert np.array_equal(SR.sharpen(img, (4095, 0, 255, radius)), img)


def test_a_single_bright_pixel_radius_2():
    """S = 256 * 100 + 100 w with w the pixel's weight under the spot: 36, 24, 16, 6, 4, 1.  amount 128 (0.5).
    centre: D = 51200 - 29200 = 22000, E = (22000 * 128 + 32768) >> 16 = 43 -> 243
    w = 24: D = -2400, E = (307200 + 32768) >> 16 = 5 -> 95      w = 16: D = -1600, E = (204800 + 32768) >> 16 = 3 -> 97
    w = 6:  D = -600,  E = (76800 + 32768) >> 16 = 1 -> 99       w = 4: D = -400, E = (51200 + 32768) >> 16 = 1 -> 99
    w = 1:  D = -100,  E = (12800 + 32768) >> 16 = 0 -> 100      outside the window: 100"""
    got = SR.sharpen(_spot(), (128, 0, 255, 2))
    assert (got[..., 0] == got[..., 1]).all() and (got[..., 1] == got[..., 2]).all()
    g = got[..., 0].astype(int)
    assert g[3, 3] == 243 and g[3, 2] == 95 and g[2, 3] == 95 and g[2, 2] == 97 and g[3, 1] == 99 and g[2, 1] == 99
    assert g[1, 1] == 100 and g[3, 0] == 100 and g[0, 0] == 100
    assert np.array_equal(g, g.T) and np.array_equal(g, g[::-1, ::-1])


def test_a_single_bright_pixel_radius_1():
    """weights 16 * ([1 2 1] (x) [1 2 1]): 64, 32, 16.  centre: D = 51200 - 32000 = 19200, E = (2457600 + 32768) >> 16 = 38 -> 238
    w = 32: D = -3200, E = (409600 + 32768) >> 16 = 6 -> 94     w = 16: D = -1600, E = 3 -> 97     two away: 100"""
    g = SR.sharpen(_spot(), (128, 0, 255, 1))[..., 0].astype(int)
    assert g[3, 3] == 238 and g[3, 2] == 94 and g[4, 3] == 94 and g[2, 2] == 97 and g[4, 4] == 97
    assert g[3, 1] == 100 and g[1, 3] == 100 and g[1, 1] == 100


def test_a_step_at_a_border_shows_the_replication():
    """1 x 3, gray 100 100 200, radius 1, amount 256: every row of the window is the one row, so S = 16 * 4 * (l + 2 c + r).
    x = 0: 100 + 200 + 100 = 400, S = 25600, D = 0 -> 100         x = 1: 100 + 200 + 200 = 500, S = 32000, D = -6400, E = 25 -> 75
    x = 2: 100 + 400 + 200 (its own value again) = 700, S = 44800, D = 6400 -> 225; a reflected border takes 100 there: D = 12800 -> 250"""
    img = _gray([[100, 100, 200]])
    assert SR.sharpen(img, (256, 0, 255, 1))[0, :, 1].tolist() == [100, 75, 225]
    assert SR.sharpen(img, (256, 0, 255, 1), variant='reflected_border')[0, :, 1].tolist() == [100, 75, 250]
    # the same image as a column, and at radius 2: l2 + 4 l1 + 6 c + 4 r1 + r2 with clamped indices
    # x = 2: 100 + 400 + 1200 + 800 + 200 = 2700, S = 16 * 2700 = 43200, D = 8000, E = (2048000 + 32768) >> 16 = 31 -> 231
    assert SR.sharpen(img.transpose(1, 0, 2), (256, 0, 255, 1))[:, 0, 1].tolist() == [100, 75, 225]
    assert SR.sharpen(img, (256, 0, 255, 2))[0, 2, 1] == 231


def test_amount_4095_on_a_checkerboard_clamps_at_both_ends():
    """64 / 192 squares of one pixel, radius 1, inside: L = 192 has four 64s at weight 2 -> D = 256 * 192 - 16 * (8 * 192 + 8 * 64)
    = 16384, E = (16384 * 4095 + 32768) >> 16 = 1024 -> limit 255 -> 192 + 255 clamps to 255; the 64s go to 64 - 255 -> 0"""
    y, x = np.mgrid[0:6, 0:8]
    board = np.where((y + x) % 2 == 1, 192, 64).astype(np.uint8)
    got = SR.sharpen(_gray(board), (4095, 0, 255, 1))
    assert np.array_equal(got, _gray(np.where(board == 192, 255, 0).astype(np.uint8)))
    ev = SR.events(_gray(board), (4095, 0, 255, 1))
    assert ev['clamped_at_0'] == 3 * 24 and ev['clamped_at_255'] == 3 * 24 and ev['limited'] == 48


def test_a_threshold_that_cores_everything():
    """the spot's largest |D| is 22000: 256 * 86 = 22016 cores all of it; 256 * 85 = 21760 leaves A = 240 at the centre alone,
    E = (240 * 4095 + 32768) >> 16 = 15"""
    assert np.array_equal(SR.sharpen(_spot(), (4095, 86, 255, 2)), _spot())
    got = SR.sharpen(_spot(), (4095, 85, 255, 2))
    want = _spot()
    want[3, 3] = 215
    assert np.array_equal(got, want)
    # hard coring would let the whole 22000 through: E = min((22000 * 4095 + 32768) >> 16, 255) = 255 -> clamped
    assert SR.sharpen(_spot(), (4095, 85, 255, 2), variant='hard_coring')[3, 3, 0] == 255


def test_limit_1():
    g = SR.sharpen(_spot(), (128, 0, 1, 2))[..., 0].astype(int)
    assert g[3, 3] == 201 and g[3, 2] == 99 and g[2, 2] == 99 and g[3, 1] == 99 and g[2, 1] == 99 and g[1, 1] == 100
    assert int((g != 100).sum()) == 21                  # the 5 x 5 window without its four corners


def test_luma_weights_and_channel_order():
    px = np.array([[[10, 20, 30]]], dtype=np.uint8)
    assert SR.luma(px, 'bgr')[0, 0] == (77 * 30 + 150 * 20 + 29 * 10 + 128) >> 8 == 22
    assert SR.luma(px, 'rgb')[0, 0] == (77 * 10 + 150 * 20 + 29 * 30 + 128) >> 8 == 18
    assert SR.luma(np.array([[[255, 255, 255]]], dtype=np.uint8))[0, 0] == 255
    # the same step goes to all three channels: differences between channels survive until one clips
    img = _spot()
    img[..., 0] = np.minimum(img[..., 0].astype(int) + 20, 255).astype(np.uint8)
    got = SR.sharpen(img, (64, 0, 255, 2)).astype(int)
    inside = (got > 0).all(axis=-1) & (got < 255).all(axis=-1)
    assert inside.all() and ((got[..., 0] - got[..., 1]) == 20).all() and (got[..., 1] == got[..., 2]).all()


# ---------------------------------------------------------------- identities and the bound
@pytest.mark.parametrize('radius', SR.RADII)
def test_amount_0_and_limit_0_pass_the_image(radius):
    img = np.random.RandomState(3).randint(0, 256, size=(2, 9, 11, 3)).astype(np.uint8)
    assert np.array_equal(SR.sharpen(img, (0, 0, 255, radius)), img)
    assert np.array_equal(SR.sharpen(img, (4095, 0, 0, radius)), img)
    assert not np.array_equal(SR.sharpen(img, (4095, 0, 1, radius)), img)


def test_the_arithmetic_bound():
    assert SR.MAX_DETAIL == 256 * 255 == 65280 and SR.MAX_AMOUNT == 4095
    assert SR.MAX_DETAIL * SR.MAX_AMOUNT + 32768 < 2 ** 32
    for radius in SR.RADII:
        t = np.array(SR.TAPS[radius])
        assert int(np.outer(t, t).sum()) * SR.SCALE[radius] == 256
        # the extremes of D: a white pixel in black and the reverse
        img = np.zeros((5, 5, 3), dtype=np.uint8)
        img[2, 2] = 255
        L = SR.luma(img)
        D = 256 * L - SR.blur(L, radius)
        assert 0 < D.max() <= SR.MAX_DETAIL and (D[2, 2] == 65280 - 255 * int(t[radius]) ** 2 * SR.SCALE[radius])
    assert (77 + 150 + 29) == 256 and (256 * 255 + 128) >> 8 == 255


# ---------------------------------------------------------------- the shared cases
def _outputs(variant=None):
    return [SR.sharpen(SR.case_image(c), c['params'], c['channels'], variant) for c in SR.CASES]


_RIGHT = _outputs()


def test_the_case_table_covers_what_the_gpu_test_promises():
    assert {c['size'] for c in SR.CASES} == set(SR.SIZES) and len(SR.CASES) == 4 * len(SR.SIZES) + 10
    for size in SR.SIZES:
        assert {(c['params'][3], c['channels']) for c in SR.CASES if c['size'] == size} >= {(r, o) for r in SR.RADII for o in ('bgr', 'rgb')}
    p = [c['params'][:3] for c in SR.CASES]
    assert any(a == 4095 for a, _, _ in p) and {0, 255} <= {t for _, t, _ in p} and {0, 255} <= {l for _, _, l in p}
    assert len({c['name'] for c in SR.CASES}) == len(SR.CASES)


@pytest.mark.parametrize('name', SR.VARIANTS)
def test_every_wrong_variant_changes_a_byte_on_the_cases(name):
    wrong = _outputs(name)
    differing = [c['name'] for c, a, b in zip(SR.CASES, _RIGHT, wrong) if not np.array_equal(a, b)]
    assert differing, name
    if name == 'rb_not_swapped':
        assert all('rgb' in d for d in differing)


@pytest.mark.parametrize('event', SR.EVENTS)
def test_every_event_occurs_in_a_case(event):
    assert any(SR.events(SR.case_image(c), c['params'], c['channels'])[event] > 0 for c in SR.CASES), event


def test_a_kernel_that_copies_cannot_pass():
    for c, got in zip(SR.CASES, _RIGHT):
        img = SR.case_image(c)
        if c['identity']:
            assert np.array_equal(got, img), c['name']
        else:
            assert (got != img).mean() >= 0.25, (c['name'], (got != img).mean())


# ---------------------------------------------------------------- the plumbing
def test_sharpen_check_names_what_is_wrong():
    import reconfigisp_amd.functional as F
    assert F.SHARPEN_RADII == (1, 2)
    assert F.sharpen_check((256, 4, 40, 2)) == (256, 4, 40, 2)
    assert F.sharpen_check([0, 0, 0, 1], True, 4, 6) == (0, 0, 0, 1)
    assert F.sharpen_check((4095, 255, 255, 1), False, 1, 1) == (4095, 255, 255, 1)
    assert all(type(v) is int for v in F.sharpen_check((256, 4, 40, 2)))
    for bad in ((256, 4, 40), (256, 4, 40, 2, 1), 256, None, 'abcd'[:3]):
        with pytest.raises(ValueError, match=r'\(amount, threshold, limit, radius\)'):
            F.sharpen_check(bad)
    for bad, what in (((True, 4, 40, 2), 'amount'), ((256, False, 40, 2), 'threshold'), ((256, 4, True, 2), 'limit'),
                      ((256, 4, 40, True), 'radius')):
        with pytest.raises(ValueError, match=what + '.*bool'):
            F.sharpen_check(bad)
    for bad, what in (((256.0, 4, 40, 2), 'amount'), ((256, 4.5, 40, 2), 'threshold'), ((256, 4, '40', 2), 'limit'),
                      ((256, 4, 40, 2.0), 'radius'), ((None, 4, 40, 2), 'amount')):
        with pytest.raises(ValueError, match=what + '.*integer'):
            F.sharpen_check(bad)
    for bad, what in (((4096, 4, 40, 2), 'amount.*4095'), ((-1, 4, 40, 2), 'amount'), ((256, 256, 40, 2), 'threshold.*255'),
                      ((256, -1, 40, 2), 'threshold'), ((256, 4, 256, 2), 'limit.*255'), ((256, 4, -1, 2), 'limit')):
        with pytest.raises(ValueError, match=what):
            F.sharpen_check(bad)
    for radius in (0, 3, -1):
        with pytest.raises(ValueError, match='radius.*one of'):
            F.sharpen_check((256, 4, 40, radius))
    for h, w in ((3, 4), (4, 3)):
        with pytest.raises(ValueError, match='4:2:0.*even'):
            F.sharpen_check((256, 4, 40, 2), True, h, w)
        assert F.sharpen_check((256, 4, 40, 2), False, h, w) == (256, 4, 40, 2)
    with pytest.raises(ValueError, match='2\\^24'):
        F.sharpen_check((256, 4, 40, 2), False, 0, 4)


def test_host_refusals_come_before_the_device():
    """on tensors of the host: what is wrong with the call is named before the missing device is"""
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    img = torch.zeros((2, 5, 6, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match='uint8 images'):
        F.bgr8_sharpen(img.float(), (256, 4, 40, 2))
    with pytest.raises(ValueError, match='channels'):
        F.bgr8_sharpen(img, (256, 4, 40, 2), channels='yuv')
    with pytest.raises(ValueError, match='radius'):
        F.bgr8_sharpen(img, (256, 4, 40, 5))
    with pytest.raises(ValueError, match='4:2:0'):
        F.bgr8_sharpen(img, (256, 4, 40, 2), nv12='bt601_full')
    with pytest.raises(RuntimeError, match='CUDA/HIP'):
        F.bgr8_sharpen(img, (256, 4, 40, 2))
    raw = torch.zeros((2, 8, 12), dtype=torch.uint16)
    with pytest.raises(ValueError, match='amount'):
        PF.output_plan(raw, 'u16', None, (3,), (5000, 0, 0, 1), None, None, None, 'triangle', 'bgr8', 'bt601_full', False, None)
    with pytest.raises(ValueError, match='4:2:0'):
        PF.output_plan(raw, 'u16', None, (3,), (256, 4, 40, 2), None, (5, 6), None, 'triangle', 'nv12', 'bt601_full', False, None)
    with pytest.raises(ValueError, match='reverse_channels'):
        PF.output_plan(raw, 'u16', None, (3,), (256, 4, 40, 2), None, None, None, 'triangle', 'nv12', 'bt601_full', True, None)
    with pytest.raises(ValueError, match='out must be'):
        PF.output_plan(raw, 'u16', None, (3,), (256, 4, 40, 2), None, None, None, 'triangle', 'bgr8', 'bt601_full', False,
                       torch.zeros((2, 8, 12), dtype=torch.uint8))
    steps, coef, final, store = PF.output_plan(raw, 'u16', None, (3,), (256, 4, 40, 2), None, (4, 6), None, 'triangle', 'nv12',
                                               'bt709_full', False, None)
    assert [name for name, _, _ in steps] == ['resize', 'sharpen']              # no warp step
    assert steps[0][1][0] == (4, 6) and steps[1][1] == (256, 4, 40, 2) and len(coef) == 12 and final == (4, 6)
    assert PF.output_plan(raw, 'u16', None, (3,), None, None, None, None, 'triangle', 'bgr8', 'bt601_full', False, None) is None


def _serve_functions():
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    from reconfigisp_amd.codes.models.isp_model import IspModel
    from reconfigisp_amd.codes.models.modules.isp_universal import IspUniversal
    from reconfigisp_amd.codes.models.modules.origin_universal import OriginUniversal
    return [(PF.serve, 'serve'), (PF.serve_frame, 'serve_frame')] + [
        (getattr(cls, name), name) for cls in (IspUniversal, OriginUniversal, IspModel) for name in ('serve', 'serve_frame')]


def test_the_keyword_on_all_eight_functions():
    fns = _serve_functions()
    assert len(fns) == 8
    for fn, name in fns:
        pars = inspect.signature(fn).parameters
        names = list(pars)
        p = pars['sharpen']
        assert p.default is None and 'sharpen' in fn.__doc__, fn
        at = names.index('sharpen')
        if name == 'serve':
            assert p.kind is inspect.Parameter.KEYWORD_ONLY, fn
            assert pars[names[at - 1]].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and names[at - 1] == 'fast_cond', fn
            assert names[at + 1] == 'out_format', fn
        else:
            assert p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, fn
            assert names[at - 1] == 'yuv_matrix' and names[at + 1] == 'out_size', fn
            assert pars['out_size'].kind is inspect.Parameter.KEYWORD_ONLY, fn


def test_the_entry_point_is_declared():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    header = open(os.path.join(ROOT, 'include', 'risp.h')).read()
    assert re.search(r'^int risp_bgr8_sharpen\(', header, flags=re.M)
    assert 'risp_bgr8_sharpen' in L.SIGNATURES and len(L.SIGNATURES['risp_bgr8_sharpen'][1]) == 12
    decl = header[header.index('\nint risp_bgr8_sharpen('):]
    assert decl[:decl.index(';')].count(',') == 11
    for name, value in (('RISP_SHARPEN_TILE_W', 64), ('RISP_SHARPEN_TILE_H', F.SHARPEN_TILE_H),
                        ('RISP_SHARPEN_MAX_AMOUNT', F.SHARPEN_MAX_AMOUNT)):
        assert re.search(r'^#define %s %d$' % (name, value), header, flags=re.M), name
    assert '(77 R + 150 G + 29 B + 128) >> 8' in header and '65280 * 4095 + 32768 < 2^32' in header


def test_sharpen_store_is_a_pure_table_and_the_table_is_the_measured_verdict():
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    assert isinstance(PF._SHARPEN_NV12_FUSED, frozenset) and PF._SHARPEN_NV12_FUSED <= {'nv12'}
    assert PF.sharpen_store('bgr8') is None
    assert PF.sharpen_store('nv12') == ('fused' if 'nv12' in PF._SHARPEN_NV12_FUSED else 'pass')
    assert PF.sharpen_store('nv12') == PF.sharpen_store('nv12')
    for bad in ('yuv', None, 0):
        with pytest.raises(ValueError, match='out_format'):
            PF.sharpen_store(bad)
    assert read_verdict('serve_sharpen.txt', '_SHARPEN_NV12_FUSED') == PF._SHARPEN_NV12_FUSED
