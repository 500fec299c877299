"""CPU: the temporal noise reduction's definition (tests/temporal_reference.py) on hand-worked vectors and at the unsigned extremes,
the host-side refusals of ``functional.temporal_check`` and of the priming rule, the keyword's place on all eight serving
functions, and the conditions the inputs of tests/test_gpu_temporal.py must meet: they tell every wrong variant of the definition
apart, and each regime of the share k holds a good part of their pixels."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import temporal_reference as TR
from conftest import ROOT


# ---------------------------------------------------------------- the definition by hand
def test_flat_frames_by_hand():
    c, p = np.full((3, 4), 100), np.full((3, 4), 60)
    # A = 25 * 40 = 1000, B = 1500.  lo = 25 * 30 = 750, e = 250, k = 64 + (250 * 16 >> 8) = 79
    assert (TR.gains(c, p, 64, 30, 0, 16) == 79).all()
    # (60 * 177 + 100 * 79 + 128) >> 8 = 18648 >> 8 = 72
    assert (TR.tnr_ref(c, p, 64, 30, 0, 16) == 72).all()
    # black 10: Bs = 1500 - 250 = 1250, lo = 750 + (1250 * 128 >> 8) = 750 + 625 = 1375 > 1000: e = 0, k = 64
    assert (TR.gains(c, p, 64, 30, 128, 16, 10) == 64).all()
    # (60 * 192 + 100 * 64 + 128) >> 8 = 18048 >> 8 = 70
    assert (TR.tnr_ref(c, p, 64, 30, 128, 16, 10) == 70).all()
    # without the pedestal Bs = 1500: lo = 750 + 750 = 1500, the same k here - and with slope 64, lo = 750 + 312 = 1062 against
    # 750 + 375 = 1125: both above 1000.  Black 40: Bs = 500, lo = 750 + 125 = 875, e = 125, k = 64 + 7 = 71
    assert (TR.gains(c, p, 64, 30, 64, 16, 40) == 71).all()
    # the sign of A does not matter
    assert (TR.gains(p, c, 64, 30, 0, 16) == 79).all()
    # (100 * 177 + 60 * 79 + 128) >> 8 = 22568 >> 8 = 88
    assert (TR.tnr_ref(p, np.full((3, 4), 100), 64, 30, 0, 16) == 88).all()


def test_one_spike_by_hand_shows_the_reflection():
    """a spike of 1000 at (0,0) over an empty state: A = 1000 times the number of times the window holds (0,0).  Rows of pixel row
    0: 2 1 0 1 2, of row 1: 1 0 1 2 1, of row 2: 0 1 2 1 0 - row 0 once, once, twice; columns of pixel column 0: 2 1 0 1 2, 1:
    1 0 1 2 3, 2: 0 1 2 3 2, 3: 1 2 3 2 1 - column 0 once, once, once, never"""
    c, p = np.zeros((3, 4), dtype=np.int64), np.zeros((3, 4), dtype=np.int64)
    c[0, 0] = 1000
    # threshold 0, ramp 64: k = min(A * 64 >> 8, 256) = min(A / 4, 256)
    assert TR.gains(c, p, 0, 0, 0, 64).tolist() == [[250, 250, 250, 0], [250, 250, 250, 0], [256, 256, 256, 0]]
    out = TR.tnr_ref(c, p, 0, 0, 0, 64)
    assert out[0, 0] == (1000 * 250 + 128) >> 8 == 977 and out.sum() == 977
    # the repeated edge would hold row 0 three times from pixel row 0: A = 3000 there and k = 256
    assert TR.tnr_ref(c, p, 0, 0, 0, 64, variant='clamp')[0, 0] == 1000
    # a 3 x 3 window never reaches (0,0) from column 2 or row 2
    k3 = TR.tnr_ref(np.full((3, 4), 500) + c, p, 0, 0, 0, 1, variant='win3')
    assert k3.shape == (3, 4)


def test_the_unsigned_extremes():
    for cv, pv, params, black, k, value in TR.EXTREMES:
        for shape in ((3, 4), (6, 8)):
            c, p = np.full(shape, cv), np.full(shape, pv)
            assert (TR.gains(c, p, *params, black) == k).all(), (cv, pv, params, black)
            out = TR.tnr_ref(c, p, *params, black)          # asserts every intermediate against 2^32
            assert out.dtype == np.uint16 and (out == value).all(), (cv, pv, params, black, out[0, 0])
    # k = 255 for ramp 1 on a sum of 65535 * 25: the clamp of e comes in front of the multiply
    assert (TR.gains(np.full((3, 4), 65535), np.zeros((3, 4)), 0, 0, 0, 1) == 255).all()
    assert (TR.tnr_ref(np.full((3, 4), 65535), np.zeros((3, 4)), 0, 0, 0, 1, variant='shiftfirst') == 65535).all()


def test_strength_256_is_the_identity_and_strength_0_freezes():
    seq = TR.sequence((2, 6, 8), seed=5)
    for params in ((256, 0, 0, 0), (256, 65535, 255, 65535), (256, 40, 10, 24)):
        assert np.array_equal(TR.tnr_ref(seq[1], seq[0], *params, 64), seq[1])
    assert np.array_equal(TR.tnr_ref(seq[1], seq[0], 0, 65535, 255, 65535, 0), seq[0])
    outs, state = TR.run_ref(seq, 0, 65535, 0, 0)
    assert all(np.array_equal(o, seq[0]) for o in outs) and np.array_equal(state, seq[0])
    outs, state = TR.run_ref(seq, 256, 0, 0, 0)
    assert all(np.array_equal(o, s) for o, s in zip(outs, seq)) and np.array_equal(state, seq[-1])


def test_the_recursion_primes_and_advances():
    seq = TR.sequence((1, 6, 8), seed=6)
    outs, state = TR.run_ref(seq, 64, 40, 0, 24, 64)
    assert np.array_equal(outs[0], seq[0])
    prev = seq[0]
    for frame, out in zip(seq[1:], outs[1:]):
        assert np.array_equal(out, TR.tnr_ref(frame, prev, 64, 40, 0, 24, 64))
        prev = out
    assert np.array_equal(state, outs[-1])
    # continued from a given state
    more, state2 = TR.run_ref(seq[3:], 64, 40, 0, 24, 64, state=outs[2])
    assert np.array_equal(more[0], outs[3]) and np.array_equal(state2, state)


# ---------------------------------------------------------------- the inputs of the GPU tests
def _first_steps():
    """[(shape, params, cur, state)]: the first filtered step of every case of tests/test_gpu_temporal.py - two independent
    uniform 10-bit frame stacks"""
    return [(shape, params) + tuple(TR.sequence(shape)[1::-1]) for shape in TR.SHAPES for params in TR.PARAMS]


def test_each_regime_holds_a_tenth_of_the_pixels_of_each_case():
    for shape, params, cur, state in _first_steps():
        k = TR.gains(cur, state, *params, TR.BLACK)
        share = [(k == params[0]).mean(), ((k > params[0]) & (k < 256)).mean(), (k == 256).mean()]
        assert min(share) >= 0.10, (shape, params, share)


def test_the_gpu_inputs_tell_every_wrong_variant_apart():
    told = dict.fromkeys(TR.VARIANTS, 0)
    for shape in TR.SHAPES:
        seq = TR.sequence(shape)
        for params in TR.PARAMS:
            want, _ = TR.run_ref(seq, *params, TR.BLACK)
            for variant in TR.VARIANTS:
                if variant == 'inplace' and shape[1] * shape[2] > 100:
                    continue                                # (a Python loop per pixel)
                got, _ = TR.run_ref(seq, *params, TR.BLACK, variant=variant)
                told[variant] += any(not np.array_equal(a, b) for a, b in zip(got, want))
    for cv, pv, params, black, _, value in TR.EXTREMES:
        c, p = np.full((3, 4), cv), np.full((3, 4), pv)
        for variant in TR.VARIANTS:
            if variant != 'frozen':
                told[variant] += bool((TR.tnr_ref(c, p, *params, black, variant=variant) != value).any())
    assert all(told.values()), told
    # the border, the window, the rounding and the recursion show in every random case; the pedestal where the slope is on
    assert told['clamp'] >= 8 and told['win3'] >= 8 and told['noround'] >= 8 and told['frozen'] >= 8 and told['nopedestal'] >= 4


# ---------------------------------------------------------------- functional.temporal_check
def test_host_refusals_come_before_the_device():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    n, h, w = 2, 6, 8
    st = F.temporal_state(n, h, w, device='cpu')
    assert tuple(st.frames.shape) == (n, h, w) and st.frames.dtype == torch.uint16 and st.frames.is_contiguous()
    assert st.frames.data_ptr() % 8 == 0 and st.primed is False and not st.frames.any()
    st.primed = True
    st.reset()
    assert st.primed is False
    for bad in ((0, h, w), (n, 2, w), (n, h, 6), (n, h, 0), (1.5, h, w), (True, h, w)):
        with pytest.raises(ValueError, match='temporal state'):
            F.temporal_state(*bad, device='cpu')
    for td in (None, st, (st, 64, 40, 0), (st, 64, 40, 0, 24, 1)):
        with pytest.raises(ValueError, match='state, strength, threshold, slope, ramp'):
            F.temporal_check(td, n, h, w)
    for state in (None, st.frames, (n, h, w)):
        with pytest.raises(ValueError, match='TemporalState'):
            F.temporal_check((state, 64, 40, 0, 24), n, h, w)
    for v in (-1, 257, 64.0, True, '64', None):
        with pytest.raises(ValueError, match='strength'):
            F.temporal_check((st, v, 40, 0, 24), n, h, w)
    for v in (-1, 65536, 40.0, False, None):
        with pytest.raises(ValueError, match='threshold'):
            F.temporal_check((st, 64, v, 0, 24), n, h, w)
    for v in (-1, 256, 1.0, True, None):
        with pytest.raises(ValueError, match='slope'):
            F.temporal_check((st, 64, 40, v, 24), n, h, w)
    for v in (-1, 65536, 24.0, True, None):
        with pytest.raises(ValueError, match='ramp'):
            F.temporal_check((st, 64, 40, 0, v), n, h, w)
    for hh, ww in ((2, 8), (6, 6), (6, 0)):
        with pytest.raises(ValueError, match='H >= 3'):
            F.temporal_check((st, 64, 40, 0, 24), n, hh, ww)
    # a state of another shape, dtype or layout
    for nn, hh, ww in ((1, h, w), (n, h + 1, w), (n, h, w + 4)):
        with pytest.raises(ValueError, match=r'\(%d,%d,%d\)' % (nn, hh, ww)):
            F.temporal_check((st, 64, 40, 0, 24), nn, hh, ww)
    for frames in (torch.zeros((n, h, w), dtype=torch.int16), torch.zeros((n, w, h), dtype=torch.uint16).transpose(1, 2),
                   torch.zeros((n, h, w)).numpy()):
        other = F.temporal_state(n, h, w, device='cpu')
        other.frames = frames
        with pytest.raises(ValueError, match='contiguous'):
            F.temporal_check((other, 64, 40, 0, 24), n, h, w)
    # everything right but the device: a CPU state is refused for being there
    with pytest.raises(RuntimeError, match='temporal state'):
        F.temporal_check((st, np.int64(64), np.uint16(40), 0, 24), n, h, w)
    # serve, serve_frame and raw_temporal check before they launch: CPU frames never reach a kernel
    raw = torch.zeros((n, h, w), dtype=torch.uint16)
    for call in (lambda: PF.serve([], [], raw, 1023.0, temporal_denoise=(st, 64, 40, 0, 24)),
                 lambda: PF.serve_frame([], [], raw, 1023.0, 4, 2, temporal_denoise=(st, 64, 40, 0, 24)),
                 lambda: F.raw_temporal(raw, (st, 64, 40, 0, 24))):
        with pytest.raises((RuntimeError, ValueError)):
            call()
    with pytest.raises(ValueError, match='ramp'):
        PF.serve_frame([], [], raw, 1023.0, 4, 2, temporal_denoise=(st, 64, 40, 0, 65536))
    with pytest.raises(ValueError, match='strength'):
        PF.temporal_plan(raw, 'u16', None, (3,), (st, 300, 40, 0, 24))
    with pytest.raises(ValueError, match=r'\(1,6,8\)'):
        PF.temporal_plan(raw[0], 'u16', None, (2, 3), (st, 64, 40, 0, 24))      # an (H,W) frame wants a state of one image
    assert PF.temporal_plan(raw, 'u16', None, (3,), None) is None


def test_the_priming_rule():
    import reconfigisp_amd.functional as F
    st = F.temporal_state(1, 3, 4, device='cpu')
    assert F._temporal_prime(st, False) == 1
    with pytest.raises(RuntimeError, match='not primed.*capturing'):
        F._temporal_prime(st, True)
    st.primed = True
    assert F._temporal_prime(st, False) == 0 and F._temporal_prime(st, True) == 0
    st.reset()
    assert F._temporal_prime(st, False) == 1


# ---------------------------------------------------------------- plumbing
def _serve_functions():
    from reconfigisp_amd.codes.models.isp_model import IspModel
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    from reconfigisp_amd.codes.models.modules.isp_universal import IspUniversal
    from reconfigisp_amd.codes.models.modules.origin_universal import OriginUniversal
    return [(PF.serve, 'serve'), (PF.serve_frame, 'serve_frame')] + [
        (getattr(cls, name), name) for cls in (IspUniversal, OriginUniversal, IspModel) for name in ('serve', 'serve_frame')]


def test_temporal_denoise_is_keyword_only_with_default_none_on_all_eight_functions():
    fns = _serve_functions()
    assert len(fns) == 8
    for fn, name in fns:
        pars = inspect.signature(fn).parameters
        p = pars['temporal_denoise']
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn
        assert 'temporal_denoise' in fn.__doc__, fn
        names = list(pars)
        at = names.index('temporal_denoise')
        assert names[at - 1] == 'raw_format' and names[at + 1] == 'statistics', fn
        if name == 'serve':
            assert names[-1] == 'fast_denoise_scene', fn


def test_the_entry_point_is_declared():
    from reconfigisp_amd import lib as L
    header = open(os.path.join(ROOT, 'include', 'risp.h')).read()
    assert re.search(r'^int risp_raw_temporal\(', header, flags=re.M)
    assert 'risp_raw_temporal' in L.SIGNATURES and len(L.SIGNATURES['risp_raw_temporal'][1]) == 13
    decl = header[header.index('\nint risp_raw_temporal('):]
    assert decl[:decl.index(';')].count(',') == 12
    import ctypes
    assert hasattr(ctypes.CDLL(L.LIB_PATH), 'risp_raw_temporal')
