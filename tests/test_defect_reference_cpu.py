"""No GPU: the defective-pixel definition of include/risp.h as tests/defect_reference.py restates it - hand-worked vectors, the
sums that 16-bit lanes get wrong, the wrong variants that the GPU test's frames tell apart -, the host helpers
``functional.defect_map`` and ``functional.defect_check``, and the plumbing: signatures, ``defect_shade`` and its table against the
verdict line of profiles/serve_defect.txt."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import defect_reference as DR
from serve_verdicts import read_verdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flat():
    return np.full((6, 8), 100, dtype=np.uint16)


def _only(got, frame, y, x, value):
    """``got`` is ``frame`` but for ``value`` at (y, x)"""
    want = frame.copy()
    want[y, x] = value
    return np.array_equal(got, want)


# ---------------------------------------------------------------- the definition by hand
def test_hand_worked_vectors():
    # an interior hot pixel: H 100, 120 (20)  V 90, 97 (7)  D 100, 110 (10)  A 100, 130 (30); mx = 130, 1000 > 130 + 16;
    # V wins: (90 + 97 + 1) >> 1 = 94 (93 without the + 1).  No neighbour of it is corrected: 1000 only raises their maximum
    f = _flat()
    f[2, 4], f[2, 6], f[0, 4], f[4, 4], f[4, 6], f[4, 2] = 1000, 120, 90, 97, 110, 130
    assert _only(DR.dpc_ref(f, 16, 0, None), f, 2, 4, 94)
    assert DR.dpc_ref(f, 16, 0, None, 'trunc')[2, 4] == 93
    assert np.array_equal(DR.dpc_ref(f, 870, 0, None), f)               # 1000 > 130 + 870 does not hold
    assert _only(DR.dpc_ref(f, 869, 0, None), f, 2, 4, 94)
    # a dead pixel: H 100, 103 (3)  V 80, 82 (2)  D 100, 120 (20)  A 100, 115 (15); mn = 80, T(80) = 16 + (80 * 64 >> 8) = 36,
    # 0 + 36 < 80; V wins: (80 + 82 + 1) >> 1 = 81
    f = _flat()
    f[3, 3], f[3, 5], f[1, 3], f[5, 3], f[5, 5], f[5, 1] = 0, 103, 80, 82, 120, 115
    assert _only(DR.dpc_ref(f, 16, 64, None), f, 3, 3, 81)
    assert np.array_equal(DR.dpc_ref(f, 16, 64, None, 'hotonly'), f)
    f[3, 3] = 44                                                        # 44 + 36 < 80 does not hold; 43 + 36 does
    assert np.array_equal(DR.dpc_ref(f, 16, 64, None), f)
    f[3, 3] = 43
    assert _only(DR.dpc_ref(f, 16, 64, None), f, 3, 3, 81)
    # a listed pixel that is neither: the first frame with 105 in place of 1000, no dynamic test
    f = _flat()
    f[2, 4], f[2, 6], f[0, 4], f[4, 4], f[4, 6], f[4, 2] = 105, 120, 90, 97, 110, 130
    assert np.array_equal(DR.dpc_ref(f, 16, 0, None), f)
    assert _only(DR.dpc_ref(f, None, 0, DR.map_ref([(2, 4)], 6, 8)), f, 2, 4, 94)
    assert _only(DR.dpc_ref(f, 16, 0, DR.map_ref([(2, 4)], 6, 8)), f, 2, 4, 94)
    # the corner: -2 reflects onto 2, so H is S(0,2) twice, V S(2,0) twice, D and A S(2,2) twice - four ties at 0, H wins
    f = _flat()
    f[0, 0], f[0, 2], f[2, 0], f[2, 2] = 500, 60, 70, 80
    assert _only(DR.dpc_ref(f, 16, 0, None), f, 0, 0, 60)
    assert DR.dpc_ref(f, 16, 0, None, 'clamp')[0, 0] == 500             # the edge replicated: the pixel is its own neighbour
    assert DR.dpc_ref(f, 16, 0, None, 'vfirst')[0, 0] == 70 and DR.dpc_ref(f, 16, 0, None, 'lasttie')[0, 0] == 80
    # the last corner likewise: 2 (n-1) - i
    f = _flat()
    f[5, 7], f[5, 5], f[3, 7], f[3, 5] = 500, 61, 71, 81
    assert _only(DR.dpc_ref(f, 16, 0, None), f, 5, 7, 61)
    # a tie of H and V, both 10 apart: H wins, (100 + 110 + 1) >> 1 = 105; V would give 95
    f = _flat()
    f[2, 6], f[0, 4], f[0, 2], f[4, 6], f[0, 6], f[4, 2] = 110, 90, 50, 150, 50, 150
    m = DR.map_ref([(2, 4)], 6, 8)
    assert _only(DR.dpc_ref(f, None, 0, m), f, 2, 4, 105)
    assert DR.dpc_ref(f, None, 0, m, 'vfirst')[2, 4] == 95 and DR.dpc_ref(f, None, 0, m, 'lasttie')[2, 4] == 95
    # a tie of D and A, both 4 apart, H and V 50 apart: D wins, (100 + 104 + 1) >> 1 = 102; A would give (98 + 102 + 1) >> 1 = 100
    f = _flat()
    f[2, 6], f[4, 4], f[4, 6], f[0, 6], f[4, 2] = 150, 150, 104, 98, 102
    assert _only(DR.dpc_ref(f, None, 0, m), f, 2, 4, 102)
    assert DR.dpc_ref(f, None, 0, m, 'afirst')[2, 4] == 100 and DR.dpc_ref(f, None, 0, m, 'lasttie')[2, 4] == 100


def test_a_constant_frame_passes_for_every_parameter():
    for value in (0, 7, 1023, 65535):
        f = np.full((2, 6, 12), value, dtype=np.uint16)
        for thr, slope in DR.PARAMS + [(None, 0)]:
            for bitmap in (None, DR.random_bitmap(6, 12, 1)):
                if thr is None and bitmap is None:
                    continue
                assert np.array_equal(DR.dpc_ref(f, thr, slope, bitmap), f), (value, thr, slope)


def test_the_largest_threshold_corrects_nothing_and_16_bit_sums_do():
    for h, w in DR.SHAPES:
        f = DR.frame_set('full', h, w)
        assert f.max() == 65535 and f.min() == 0
        assert np.array_equal(DR.dpc_ref(f, 65535, 255, None), f), (h, w)
        assert not np.array_equal(DR.dpc_ref(f, 65535, 255, None, 'wrap16'), f), (h, w)


# ---------------------------------------------------------------- the GPU test's inputs tell every wrong variant apart
def _differs(kind, h, w, thr, slope, variant):
    f = DR.frame_set(kind, h, w)
    return int((DR.dpc_ref(f, thr, slope, None) != DR.dpc_ref(f, thr, slope, None, variant)).sum())


def test_every_variant_differs_on_the_gpu_tests_inputs():
    """what each input set is there for, asserted so that a later change of inputs cannot quietly lose one"""
    for h, w in DR.SHAPES:
        # full-range and 10-bit frames at (0,0) and (16,32) correct a good part of the pixels (8.3 .. 24.4 % with these seeds) ...
        for kind in ('full', 'ten'):
            for thr, slope in ((0, 0), (16, 32)):
                f = DR.frame_set(kind, h, w)
                share = (DR.dpc_ref(f, thr, slope, None) != f).mean()
                assert 0.08 <= share <= 0.25, (kind, h, w, thr, slope, share)
                # ... and separate these at every shape
                for variant in ('clamp', 'dist1', 'vfirst', 'lasttie', 'hotonly'):
                    assert _differs(kind, h, w, thr, slope, variant), (variant, kind, h, w, thr, slope)
            assert _differs(kind, h, w, 0, 0, 'ge'), (kind, h, w)
        # the slope on p needs slope > 0
        assert any(_differs(kind, h, w, 0, 255, 'slope_p') for kind in DR.KINDS), (h, w)
        # without the + 1: at H <= 4 the reflected V pair is one sample twice, so the winning sum is even
        for kind in DR.KINDS:
            if h <= 4:
                assert not _differs(kind, h, w, 0, 0, 'trunc'), (kind, h, w)
        if h > 4:
            assert _differs('full', h, w, 0, 0, 'trunc') and _differs('ten', h, w, 0, 0, 'trunc'), (h, w)
        # sums in uint16
        assert _differs('full', h, w, 16, 32, 'wrap16') and _differs('full', h, w, 65535, 255, 'wrap16'), (h, w)
    assert _differs('full', 34, 68, 16, 32, 'slope_p') and _differs('ten', 34, 68, 16, 32, 'slope_p')
    # A before D: a tie of D and A below H and V needs few codes and many pixels
    assert 10 <= _differs('low', 34, 68, 0, 0, 'afirst') <= 30
    # neighbours from corrected output (a raster loop in python: the small shape)
    assert _differs('ten', 6, 12, 16, 32, 'recursive') and _differs('full', 6, 12, 0, 0, 'recursive')
    # and the map: a mirrored map is another map
    for h, w in DR.SHAPES:
        m = DR.random_bitmap(h, w, seed=h + w)
        listed = DR.listed_ref(m, h, w)
        assert listed[0, 0] and listed[h - 1, w - 1] and not np.array_equal(listed, listed[:, ::-1])
        assert w <= 32 or (listed[0, 31] and listed[0, 32])
        f = DR.frame_set('ten', h, w)
        assert not np.array_equal(DR.dpc_ref(f, None, 0, m), f)


# ---------------------------------------------------------------- functional.defect_map
def test_defect_map_builds_the_bitmap():
    import reconfigisp_amd.functional as F
    m = F.defect_map([(0, 0), (0, 31), (1, 32), (2, 67)], 3, 68)
    assert m.dtype == torch.int32 and tuple(m.shape) == (3, 3) and m.is_contiguous() and not m.is_cuda
    assert m.tolist() == [[1 - (1 << 31), 0, 0], [0, 1, 0], [0, 0, 8]]   # bit 0 and bit 31 (the sign bit); the last column: bit 3 of word 2
    assert np.array_equal(m.numpy(), DR.map_ref([(0, 0), (0, 31), (1, 32), (2, 67)], 3, 68))
    assert F.defect_map([(1, 31)], 3, 32).tolist() == [[0], [-(1 << 31)], [0]]
    coords = np.argwhere(DR.listed_ref(DR.random_bitmap(34, 68, 3), 34, 68))
    for given in (coords, coords.tolist(), torch.from_numpy(coords), (tuple(c) for c in coords.tolist())):
        assert np.array_equal(F.defect_map(given, 34, 68).numpy(), DR.map_ref(coords.tolist(), 34, 68))
    assert np.array_equal(F.defect_map(np.concatenate([coords, coords]), 34, 68).numpy(), DR.map_ref(coords.tolist(), 34, 68))
    for empty in ([], np.zeros((0, 2), dtype=np.int64)):
        z = F.defect_map(empty, 5, 40)
        assert tuple(z.shape) == (5, 2) and z.dtype == torch.int32 and not z.any()


def test_defect_map_refusals():
    import reconfigisp_amd.functional as F
    for bad in ([(3, 0)], [(0, 8)], [(-1, 0)], [(0, -1)]):
        with pytest.raises(ValueError, match='outside'):
            F.defect_map(bad, 3, 8)
    for bad in ([(0.0, 1.0)], np.array([[0.5, 1]]), [(True, False)]):
        with pytest.raises(ValueError, match='integers'):
            F.defect_map(bad, 3, 8)
    for bad in ([(0, 1, 2)], np.zeros((2, 3), dtype=np.int64), [1, 2]):
        with pytest.raises(ValueError, match=r'\(K,2\)'):
            F.defect_map(bad, 3, 8)
    with pytest.raises(ValueError, match='frame size'):
        F.defect_map([], 0, 8)


# ---------------------------------------------------------------- functional.defect_check
def test_host_refusals_come_before_the_device():
    """on CPU tensors: whatever is wrong is named before the device is asked for, and a right map on the CPU is refused for
    being there"""
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    h, w = 34, 68
    good = torch.zeros((h, 3), dtype=torch.int32)
    assert F.defect_check((16, 32, None), h, w) == (16, 32, None)
    assert F.defect_check((np.int64(0), np.uint8(255), None), h, w) == (0, 255, None)
    for dc in (None, 16, (16, 32), (16, 32, None, None)):
        with pytest.raises(ValueError, match='threshold, slope, defects'):
            F.defect_check(dc, h, w)
    for thr in (-1, 65536, 16.0, True, '16'):
        with pytest.raises(ValueError, match='threshold'):
            F.defect_check((thr, 0, good), h, w)
    for slope in (-1, 256, 1.0, False, None):
        with pytest.raises(ValueError, match='slope'):
            F.defect_check((16, slope, good), h, w)
    with pytest.raises(ValueError, match='neither'):
        F.defect_check((None, 0, None), h, w)
    with pytest.raises(ValueError, match='int32'):
        F.defect_check((16, 0, good.to(torch.int64)), h, w)
    with pytest.raises(ValueError, match='int32'):
        F.defect_check((16, 0, good.numpy()), h, w)
    for bad in (torch.zeros((h, 2), dtype=torch.int32), torch.zeros((h - 1, 3), dtype=torch.int32),
                torch.zeros((3, h), dtype=torch.int32).t(), torch.zeros((h, 6), dtype=torch.int32)[:, ::2]):
        with pytest.raises(ValueError, match=r'\(34,3\)'):
            F.defect_check((16, 0, bad), h, w)
    for hh, ww in ((2, 8), (4, 6), (4, 0)):
        with pytest.raises(ValueError, match='H >= 3'):
            F.defect_check((16, 0, None), hh, ww)
    with pytest.raises(RuntimeError, match='defect map'):
        F.defect_check((None, 0, good), h, w)                # a CPU tensor
    # serve, serve_frame and raw_defect check before they launch: CPU frames never reach a kernel
    raw = torch.zeros((1, h, w), dtype=torch.uint16)
    for call in (lambda: PF.serve([], [], raw, 1023.0, defect_correction=(16, 0, None)),
                 lambda: PF.serve_frame([], [], raw, 1023.0, 32, 16, defect_correction=(16, 256, None)),
                 lambda: F.raw_defect(raw, (16, 0, None))):
        with pytest.raises((RuntimeError, ValueError)):
            call()
    with pytest.raises(ValueError, match='slope'):
        PF.serve_frame([], [], raw, 1023.0, 32, 16, defect_correction=(16, 256, None))


# ---------------------------------------------------------------- plumbing
def _serve_functions():
    from reconfigisp_amd.codes.models.isp_model import IspModel
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    from reconfigisp_amd.codes.models.modules.isp_universal import IspUniversal
    from reconfigisp_amd.codes.models.modules.origin_universal import OriginUniversal
    return [(PF.serve, 'serve'), (PF.serve_frame, 'serve_frame')] + [
        (getattr(cls, name), name) for cls in (IspUniversal, OriginUniversal, IspModel) for name in ('serve', 'serve_frame')]


def test_defect_correction_is_keyword_only_with_default_none_on_all_eight_functions():
    fns = _serve_functions()
    assert len(fns) == 8
    for fn, name in fns:
        pars = inspect.signature(fn).parameters
        p = pars['defect_correction']
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn
        assert 'defect_correction' in fn.__doc__, fn
        names = list(pars)
        at = names.index('defect_correction')
        if name == 'serve':
            assert names[at - 2:] == ['raw_width', 'lens_shading', 'defect_correction', 'fast_median', 'fast_denoise_scene'], fn
        else:
            assert names[at - 1:] == ['raw_width', 'defect_correction', 'lens_shading'], fn


def test_defect_shade_is_a_pure_table_and_the_table_is_the_measured_verdict():
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    assert isinstance(PF._DEFECT_SHADE_FUSED, frozenset) and PF._DEFECT_SHADE_FUSED <= {'u16', 'raw10', 'raw12'}
    for fmt in ('u16', 'raw10', 'raw12'):
        assert PF.defect_shade(fmt) == ('fused' if fmt in PF._DEFECT_SHADE_FUSED else 'pass')
    with pytest.raises(ValueError, match='raw_format'):
        PF.defect_shade('raw14')
    assert read_verdict('serve_defect.txt', '_DEFECT_SHADE_FUSED') == PF._DEFECT_SHADE_FUSED


def test_the_entry_point_is_declared():
    from reconfigisp_amd import lib as L
    header = open(os.path.join(ROOT, 'include', 'risp.h')).read()
    assert re.search(r'^int risp_raw_defect\(', header, flags=re.M)
    assert 'risp_raw_defect' in L.SIGNATURES and len(L.SIGNATURES['risp_raw_defect'][1]) == 16
    decl = header[header.index('\nint risp_raw_defect('):]
    assert decl[:decl.index(';')].count(',') == 15
