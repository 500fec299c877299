"""The scaled, cropped output without a GPU: the tap tables against hand-worked values and against the numpy restatement
(tests/resize_reference.py), the properties the definition promises, what each deliberate mistake of the reference would change
on the GPU tests' own inputs, Pillow beside it, and the plumbing - keywords, verdict table, header, host refusals."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_reference as RR  # noqa: E402
from serve_verdicts import read_verdict  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = ((4000, 1920), (4000, 640), (4000, 500), (3000, 1080))


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------- the tables
def test_hand_worked_tables():
    """worked on paper from the definition; the reference and the product both give them"""
    import reconfigisp_amd.functional as F
    for taps in (RR.taps, F.resample_taps):
        start, weight = taps(8, 4, 'box')
        assert start.tolist() == [0, 2, 4, 6] and weight.tolist() == [[8192, 8192]] * 4
        for kernel in RR.KERNELS:
            start, weight = taps(7, 7, kernel, 3)
            assert start.tolist() == list(range(3, 10)) and weight.tolist() == [[16384]] * 7
        # triangle 4 -> 8: scale 0.5, support 1; c = 0.25, 0.75, ...: f(0.25) = 0.75 and f(0.75) = 0.25 alternate, and the two
        # outputs at the ends see one sample only
        start, weight = taps(4, 8, 'triangle')
        assert start.tolist() == [0, 0, 0, 1, 1, 2, 2, 2]
        assert weight.tolist() == [[16384, 0], [12288, 4096], [4096, 12288], [12288, 4096], [4096, 12288], [12288, 4096],
                                   [4096, 12288], [0, 16384]]
        # bicubic 4 -> 2: scale 2, support 4, c = 1: x = -0.25, 0.25, 0.75, 1.25 -> f = 0.8671875, 0.8671875, 0.2265625,
        # -0.0703125, sum 1.890625 -> 7515.04, 7515.04, 1963.4, -609.3 -> rounded they sum to 16384, no residue
        start, weight = taps(4, 2, 'bicubic')
        assert start.tolist() == [0, 0] and weight.tolist() == [[7515, 7515, 1963, -609], [-609, 1963, 7515, 7515]]


def test_resample_taps_equals_the_reference_over_a_grid():
    """every S, D in 1 .. 40, three kernels, offsets 0 and 5; a geometry whose support window passes 32 samples is refused"""
    import reconfigisp_amd.functional as F
    for kernel in RR.KERNELS:
        for S in range(1, 41):
            for D in range(1, 41):
                if RR.longest_window(S, D, kernel) > 32:
                    with pytest.raises(ValueError, match='RESIZE_MAX_TAPS'):
                        F.resample_taps(S, D, kernel)
                    continue
                for o in (0, 5):
                    got = F.resample_taps(S, D, kernel, o)
                    assert got[0].dtype == np.int32 and got[1].dtype == np.int16
                    assert _same(got, RR.taps(S, D, kernel, o)), (kernel, S, D, o)


@pytest.mark.parametrize('kernel', RR.KERNELS)
def test_resample_taps_equals_the_reference_at_sensor_sizes(kernel):
    import reconfigisp_amd.functional as F
    for S, D in BIG:
        for o in (0, 5):
            assert _same(F.resample_taps(S, D, kernel, o), RR.taps(S, D, kernel, o)), (S, D, o)


def test_rows_sum_to_16384_starts_never_decrease_and_stay_in_the_window():
    """starts never decrease with box and triangle and on every reduction.  A bicubic ENLARGEMENT is the one exception the
    definition itself makes: an output that falls exactly on a sample has exact zeros at |x| = 1 and 2, trimming moves its start
    one past its neighbour's (7 -> 33 at output 16), and the next start steps back by that one"""
    import reconfigisp_amd.functional as F
    geos = [(S, D) for S in (1, 2, 3, 7, 16, 31, 40) for D in (1, 2, 5, 16, 33, 40)] + list(BIG)
    for kernel in RR.KERNELS:
        for S, D in geos:
            if RR.longest_window(S, D, kernel) > 32:
                continue
            for o in (0, 5):
                start, weight = F.resample_taps(S, D, kernel, o)
                T = weight.shape[1]
                assert (weight.astype(np.int64).sum(axis=1) == 16384).all(), (kernel, S, D)
                assert start.min() >= o and start.max() + T <= o + S and T <= S, (kernel, S, D)
                assert (np.diff(start) >= (-1 if kernel == 'bicubic' and D > S else 0)).all(), (kernel, S, D)


def test_tap_counts_and_the_limit():
    import reconfigisp_amd.functional as F
    want = {'box': (3, 7, 8), 'triangle': (5, 13, 16), 'bicubic': (9, 25, 32)}
    for kernel in RR.KERNELS:
        assert tuple(F.resample_taps(4000, D, kernel)[1].shape[1] for D in (1920, 640, 500)) == want[kernel]
    with pytest.raises(ValueError, match='8:1'):
        F.resample_taps(4000, 499, 'bicubic')
    with pytest.raises(ValueError, match='RESIZE_MAX_TAPS'):
        F.resize_check((1080, 499), None, 'bicubic', 3000, 4000)
    assert F.RESIZE_MAX_TAPS == 32
    shape, size, win = RR.REFUSED_CASE
    for kernel in RR.KERNELS:
        with pytest.raises(ValueError, match='RESIZE_MAX_TAPS'):
            F.resize_check(size, win, kernel, shape[1], shape[2])


def test_tile_rows_follow_the_span():
    """the first row count whose span fits the LDS budget: 16 rows wherever the reduction is moderate, fewer at 32:1"""
    import reconfigisp_amd.functional as F
    assert F.resize_tile_rows(2250, 1080, 'triangle', 375)[0] == 16
    rows, span = F.resize_tile_rows(832, 26, 'box')
    assert (rows, span) == (8, 256)
    start = RR.taps(832, 26, 'box')[0]
    assert span == start[7] + 32 - start[0] and start[15] + 32 - start[0] == 512
    assert 512 * F.RESIZE_TILE_W * 3 > F.RESIZE_LDS_BYTES > 256 * F.RESIZE_TILE_W * 3 + 6400


def test_host_tables_are_bounded_and_a_moving_window_adds_its_offset():
    """the host keeps the last RESIZE_HOST_CACHE tables and tile plans; a window that moves reuses the table of its size"""
    import reconfigisp_amd.functional as F
    base = F.resample_taps(40, 18, 'bicubic')
    built = len(F._RESAMPLE_BASE)
    for o in range(F.RESIZE_HOST_CACHE + 40):
        start, weight = F.resample_taps(40, 18, 'bicubic', o)
        assert weight is base[1] and np.array_equal(start, base[0] + o) and start.dtype == np.int32
        F.resize_tile_rows(40, 18, 'bicubic', o)
    assert len(F._RESAMPLE_BASE) == built, 'a moved window built its table again'
    assert len(F._RESAMPLE_TAPS) <= F.RESIZE_HOST_CACHE and len(F._RESIZE_TILES) <= F.RESIZE_HOST_CACHE
    assert _same(F.resample_taps(40, 18, 'bicubic', 0), RR.taps(40, 18, 'bicubic', 0)), 'an evicted table comes back the same'


def test_more_row_tiles_than_a_grid_holds_are_refused_on_the_host(monkeypatch):
    import reconfigisp_amd.functional as F
    monkeypatch.setattr(F, 'resize_tile_rows', lambda *a: (2, 3))
    assert F.resize_check((131070, 4), None, 'box', 4, 4) == ((131070, 4), (0, 0, 4, 4))
    with pytest.raises(ValueError, match='row tiles'):
        F.resize_check((131072, 4), None, 'box', 4, 4)


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize('kernel', RR.KERNELS)
def test_a_flat_image_maps_to_itself(kernel):
    for value in (0, 1, 127, 254, 255):
        img = np.full((1, 24, 40, 3), value, dtype=np.uint8)
        for size in ((10, 18), (36, 52), (24, 40), (3, 5)):
            assert (RR.resize(img, size, None, kernel) == value).all(), (value, size)


@pytest.mark.parametrize('kernel', RR.KERNELS)
def test_a_window_equals_slicing_first(kernel):
    img = RR.make_image(2, 24, 40, 7)
    for win in ((3, 5, 17, 29), (0, 0, 24, 40), (23, 39, 1, 1), (0, 11, 24, 8)):
        y0, x0, h, w = win
        cut = np.ascontiguousarray(img[:, y0:y0 + h, x0:x0 + w])
        for size in ((10, 18), (h, w), (31, 7)):
            assert np.array_equal(RR.resize(img, size, win, kernel), RR.resize(cut, size, None, kernel)), (win, size)
        assert np.array_equal(RR.resize(img, None, win, kernel), cut)


@pytest.mark.parametrize('variant', RR.VARIANTS)
def test_each_wrong_variant_would_be_seen(variant):
    """on the GPU tests' own inputs each deliberate mistake changes at least 5 % of the bytes of at least one listed case"""
    worst = 0.0
    for ci, (shape, size, win) in enumerate(RR.CASES):
        img = RR.make_image(*shape, seed=100 + ci)
        for kernel in RR.KERNELS:
            worst = max(worst, float((RR.resize(img, size, win, kernel) != RR.resize(img, size, win, kernel, variant)).mean()))
    print(variant, 'changes up to %.1f %% of the bytes' % (100 * worst))
    assert worst >= 0.05


def test_within_one_code_of_pillow():
    """Pillow's 22-bit weights against Q14 rows renormalised to 16384: within 1 code, at most 3 % of the bytes differ"""
    Image = pytest.importorskip('PIL.Image')
    modes = {'box': Image.BOX, 'triangle': Image.BILINEAR, 'bicubic': Image.BICUBIC}
    for (h, w), (oh, ow) in (((24, 40), (10, 18)), ((24, 40), (36, 52)), ((30, 44), (8, 12)), ((64, 64), (8, 8))):
        img = RR.make_image(1, h, w, 3)
        for kernel, mode in modes.items():
            ours = RR.resize(img, (oh, ow), None, kernel)[0].astype(np.int64)
            theirs = np.asarray(Image.fromarray(img[0]).resize((ow, oh), mode)).astype(np.int64)
            diff = np.abs(ours - theirs)
            print((h, w), (oh, ow), kernel, 'max', diff.max(), 'differing %.2f %%' % (100 * (diff > 0).mean()))
            assert diff.max() <= 1 and (diff > 0).mean() <= 0.03


# ---------------------------------------------------------------- plumbing
def _serve_functions():
    from reconfigisp_amd.codes.models.isp_model import IspModel
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    from reconfigisp_amd.codes.models.modules.isp_universal import IspUniversal
    from reconfigisp_amd.codes.models.modules.origin_universal import OriginUniversal
    return [(PF.serve, 'serve'), (PF.serve_frame, 'serve_frame')] + [
        (getattr(cls, name), name) for cls in (IspUniversal, OriginUniversal, IspModel) for name in ('serve', 'serve_frame')]


def test_the_keywords_on_all_eight_functions():
    fns = _serve_functions()
    assert len(fns) == 8
    for fn, name in fns:
        pars = inspect.signature(fn).parameters
        names = list(pars)
        for key, default in (('out_size', None), ('out_window', None), ('resample', 'triangle')):
            p = pars[key]
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == default, (fn, key)
            assert key in fn.__doc__, (fn, key)
        at = names.index('out_size')
        assert names[at:at + 3] == ['out_size', 'out_window', 'resample'], fn
        if name == 'serve':
            assert names[at - 1] == 'yuv_matrix' and names[at + 3] == 'raw_format', fn
            assert names[-5:] == ['raw_width', 'lens_shading', 'defect_correction', 'fast_median', 'fast_denoise_scene'], fn
        else:
            assert pars[names[at - 1]].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and names[at + 3] == 'raw_format', fn
            assert names[-3:] == ['raw_width', 'defect_correction', 'lens_shading'], fn


def test_resize_store_is_a_pure_table_and_the_table_is_the_measured_verdict():
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    assert isinstance(PF._RESIZE_NV12_FUSED, frozenset) and PF._RESIZE_NV12_FUSED <= {'nv12'}
    assert PF.resize_store('bgr8') is None
    assert PF.resize_store('nv12') == ('fused' if 'nv12' in PF._RESIZE_NV12_FUSED else 'pass')
    with pytest.raises(ValueError, match='out_format'):
        PF.resize_store('i420')
    assert read_verdict('serve_resize.txt', '_RESIZE_NV12_FUSED') == PF._RESIZE_NV12_FUSED


def test_the_entry_point_is_declared():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    header = open(os.path.join(ROOT, 'include', 'risp.h')).read()
    assert re.search(r'^int risp_bgr8_resize\(', header, flags=re.M)
    assert 'risp_bgr8_resize' in L.SIGNATURES and len(L.SIGNATURES['risp_bgr8_resize'][1]) == 18
    decl = header[header.index('\nint risp_bgr8_resize('):]
    assert decl[:decl.index(';')].count(',') == 17
    for name, value in (('RISP_RESIZE_MAX_TAPS', F.RESIZE_MAX_TAPS), ('RISP_RESIZE_TILE_W', F.RESIZE_TILE_W),
                        ('RISP_RESIZE_LDS_BYTES', F.RESIZE_LDS_BYTES)):
        assert re.search(r'^#define %s %d$' % (name, value), header, flags=re.M), name
    assert F.RESAMPLE == ('box', 'triangle', 'bicubic')


def test_host_refusals_come_before_the_device():
    """on CPU tensors: whatever is wrong is named before the device is asked for, and a right call is refused for being there"""
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    H, W = 24, 40
    assert F.resize_check(None, None, 'box', H, W) == ((H, W), (0, 0, H, W))
    assert F.resize_check((10, 18), (3, 5, 17, 29), 'bicubic', H, W) == ((10, 18), (3, 5, 17, 29))
    assert F.resize_check([np.int64(10), 18], None, 'triangle', H, W, True) == ((10, 18), (0, 0, H, W))
    for size in ((0, 4), (4,), (4, 4, 4), (4.0, 4), (True, 4), 'ab', 7, (-1, 4)):
        with pytest.raises(ValueError, match='out_size'):
            F.resize_check(size, None, 'triangle', H, W)
    for win in ((0, 0, 25, 40), (0, 1, 24, 40), (-1, 0, 4, 4), (0, 0, 0, 4), (0, 0, 4), (0, 0, 4.0, 4), 5, (20, 0, 5, 4)):
        with pytest.raises(ValueError, match='out_window'):
            F.resize_check(None, win, 'triangle', H, W)
    for kernel in ('lanczos', 'bilinear', None, 1):
        with pytest.raises(ValueError, match='resample'):
            F.resize_check((4, 4), None, kernel, H, W)
    for size in ((9, 18), (10, 17)):
        with pytest.raises(ValueError, match='even'):
            F.resize_check(size, None, 'triangle', H, W, True)
    with pytest.raises(ValueError, match='RESIZE_MAX_TAPS'):
        F.resize_check((4, 1), None, 'triangle', H, W)              # 40 -> 1
    img = torch.zeros((2, H, W, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match='uint8'):
        F.bgr8_resize(img.float(), (10, 18))
    with pytest.raises(ValueError, match='uint8'):
        F.bgr8_resize(img[..., :2], (10, 18))
    with pytest.raises(ValueError, match='channels'):
        F.bgr8_resize(img, (10, 18), channels='gbr')
    with pytest.raises(ValueError, match='yuv matrix'):
        F.bgr8_resize(img, (10, 18), nv12='bt2020')
    with pytest.raises(ValueError, match='out_window'):
        F.bgr8_resize(img, (10, 18), (0, 0, 25, 40))
    with pytest.raises(ValueError, match='even'):
        F.bgr8_resize(img, (9, 18), nv12='bt601_full')
    with pytest.raises(RuntimeError, match='img'):
        F.bgr8_resize(img, (10, 18))                                # all is right but the device
    # serve and serve_frame check before they launch: CPU frames never reach a kernel, and what is wrong with the keywords is named
    raw = torch.zeros((1, H, W), dtype=torch.uint16)
    for kw, what in ((dict(out_size=(0, 4)), 'out_size'), (dict(out_window=(0, 0, 25, 40)), 'out_window'),
                     (dict(out_size=(4, 4), resample='lanczos'), 'resample'), (dict(out_size=(4, 1)), 'RESIZE_MAX_TAPS'),
                     (dict(out_size=(9, 18), out_format='nv12'), 'even'),
                     (dict(out_size=(10, 18), out=torch.zeros((1, 10, 17, 3), dtype=torch.uint8)), 'out must be')):
        with pytest.raises(ValueError, match=what):
            PF.serve_frame([], [], raw, 1023.0, 16, 8, **kw)
        with pytest.raises(ValueError, match=what):
            PF.serve_frame([], [], raw[0], 1023.0, 16, 8, **kw)
    for call in (lambda: PF.serve([], [], raw, 1023.0, out_size=(10, 18)),
                 lambda: PF.serve_frame([], [], raw, 1023.0, 16, 8, out_size=(10, 18))):
        with pytest.raises((RuntimeError, ValueError)):
            call()
