"""GPU: the temporal noise reduction's launch (risp_raw_temporal through ``functional.raw_temporal``) against
tests/temporal_reference.py.  The filter is an integer function of the current frame and the state (include/risp.h), so every
comparison is ``torch.equal`` / ``np.array_equal``, on the returned frames AND on ``state.frames``: nothing here has a tolerance.

The inputs are those of tests/temporal_reference.py (``SHAPES``, ``PARAMS``, ``sequence``, ``EXTREMES``);
tests/test_temporal_reference_cpu.py asserts that they tell every wrong variant of the definition apart and that each regime of
the share k holds a tenth of the pixels of each case.  Shapes: (1,3,4) - the smallest legal frame, every neighbour a reflection,
one thread; (2,6,8); (3,37,260) - a thread walks 8 rows, 37 % 8 = 5 leaves a short last strip, 65 column groups put a strip change
inside a wave; (1,16,1028) - 257 column groups pass a workgroup.  The output and the state lie between bands of sentinels
(tests/guarded.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import temporal_reference as TR
from guarded import Guarded
from raw_placement import _place16

pytestmark = pytest.mark.gpu


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


def _guarded_u16(shape):
    """(the guard, a contiguous 16-byte aligned uint16 view of ``shape`` between its bands)"""
    g = Guarded(int(np.prod(shape)) // 2)
    return g, g.t.view(torch.uint16).view(shape)


def _state(shape):
    """(the guard, a TemporalState whose frames lie between sentinel bands)"""
    import reconfigisp_amd.functional as F
    g, frames = _guarded_u16(shape)
    st = F.temporal_state(*shape)
    st.frames = frames
    return g, st


_REF = {}


def _ref(shape, params):
    """the reference recursion of a case, computed once: (the sequence, its filtered frames)"""
    key = (shape, params)
    if key not in _REF:
        seq = TR.sequence(shape)
        _REF[key] = (seq, TR.run_ref(seq, *params, TR.BLACK)[0])
    return _REF[key]


# ---------------------------------------------------------------- 1. the recursion: priming, then four frames
@pytest.mark.parametrize('params', TR.PARAMS, ids=lambda v: '-'.join(map(str, v)))
@pytest.mark.parametrize('shape', TR.SHAPES, ids=lambda v: 'x'.join(map(str, v)))
def test_raw_temporal_equals_the_reference_over_a_sequence(shape, params):
    import reconfigisp_amd.functional as F
    seq, want = _ref(shape, params)
    gs, st = _state(shape)
    go, out = _guarded_u16(shape)
    td = (st,) + params
    for step, (frame, ref) in enumerate(zip(seq, want)):
        dev = torch.from_numpy(frame).cuda()
        assert st.primed is (step > 0)
        got, calls = _counted(lambda: F.raw_temporal(dev, td, TR.BLACK, out=out))
        assert got is out and calls == {'risp_raw_temporal': 1} and st.primed is True
        assert np.array_equal(out.cpu().numpy(), ref), 'step %d: %d samples differ' % (step, (out.cpu().numpy() != ref).sum())
        assert torch.equal(st.frames, out), 'step %d: the state is not the filtered frame' % step
        assert torch.equal(dev.cpu(), torch.from_numpy(frame))
        assert gs.bands_intact() and go.bands_intact()
    assert not np.array_equal(want[1], seq[1]) and not np.array_equal(want[1], want[0])
    # without out= the frames are allocated; an (H,W) frame over a state of one image
    if shape[0] == 1:
        st2 = F.temporal_state(*shape)
        for frame, ref in zip(seq[:3], want[:3]):
            got = F.raw_temporal(torch.from_numpy(frame[0]).cuda(), (st2,) + params, TR.BLACK)
            assert tuple(got.shape) == shape[1:] and np.array_equal(got.cpu().numpy(), ref[0])
            assert np.array_equal(st2.frames.cpu().numpy(), ref)
        # reset: the next frame primes again
        st2.reset()
        assert torch.equal(F.raw_temporal(torch.from_numpy(seq[3]).cuda(), (st2,) + params, TR.BLACK).cpu(), torch.from_numpy(seq[3]))


# ---------------------------------------------------------------- 2. frames that are only 2-byte aligned: the narrow loads
@pytest.mark.parametrize('shape', [TR.SHAPES[0], TR.SHAPES[2]], ids=lambda v: 'x'.join(map(str, v)))
def test_a_frame_stack_at_a_2_byte_aligned_address(shape):
    import reconfigisp_amd.functional as F
    params = TR.PARAMS[1]
    seq, want = _ref(shape, params)
    for at in (1, 3):
        gs, st = _state(shape)
        for frame, ref in zip(seq[:3], want[:3]):
            dev = _place16(frame, at)
            assert dev.data_ptr() % 8 == 2 * at
            got = F.raw_temporal(dev, (st,) + params, TR.BLACK)
            assert np.array_equal(got.cpu().numpy(), ref) and np.array_equal(st.frames.cpu().numpy(), ref)
        assert gs.bands_intact()


# ---------------------------------------------------------------- 3. the unsigned extremes, strength 0 and 256
def test_the_extreme_frames():
    import reconfigisp_amd.functional as F
    shape = (1, 6, 8)
    for cv, pv, params, black, _, value in TR.EXTREMES:
        gs, st = _state(shape)
        st.frames.fill_(pv)
        st.primed = True
        got = F.raw_temporal(torch.full(shape, cv, dtype=torch.uint16).cuda(), (st,) + params, black)
        assert (got.cpu().numpy() == value).all(), (cv, pv, params, black, got.flatten()[:4].tolist())
        assert torch.equal(st.frames, got) and gs.bands_intact()
    # full-range random frames under the largest parameters
    rng = np.random.default_rng(3)
    c, p = (rng.integers(0, 65536, (2, 9, 12)).astype(np.uint16) for _ in range(2))
    for params, black in (((0, 0, 255, 65535), 0), ((255, 65535, 255, 65535), 65535), ((1, 1, 255, 1), 1000)):
        gs, st = _state(c.shape)
        st.frames.copy_(torch.from_numpy(p))
        st.primed = True
        got = F.raw_temporal(torch.from_numpy(c).cuda(), (st,) + params, black)
        assert np.array_equal(got.cpu().numpy(), TR.tnr_ref(c, p, *params, black)), (params, black)


def test_strength_256_passes_the_frames_and_strength_0_freezes():
    import reconfigisp_amd.functional as F
    shape = TR.SHAPES[1]
    seq = [torch.from_numpy(f).cuda() for f in TR.sequence(shape)]
    st = F.temporal_state(*shape)
    for frame in seq:
        assert torch.equal(F.raw_temporal(frame, (st, 256, 40, 10, 24), TR.BLACK), frame) and torch.equal(st.frames, frame)
    st = F.temporal_state(*shape)
    for frame in seq:
        assert torch.equal(F.raw_temporal(frame, (st, 0, 65535, 0, 0), TR.BLACK), seq[0]) and torch.equal(st.frames, seq[0])


def test_the_same_bits_twice():
    import reconfigisp_amd.functional as F
    shape, params = TR.SHAPES[2], TR.PARAMS[0]
    seq, want = _ref(shape, params)
    cur, prev = torch.from_numpy(seq[2]).cuda(), torch.from_numpy(want[1]).cuda()
    runs = []
    for _ in range(2):
        st = F.temporal_state(*shape)
        st.frames.copy_(prev)
        st.primed = True
        runs.append(F.raw_temporal(cur, (st,) + params, TR.BLACK).clone())
        assert torch.equal(st.frames, runs[-1])
    assert torch.equal(runs[0], runs[1]) and np.array_equal(runs[0].cpu().numpy(), want[2])


# ---------------------------------------------------------------- 4. refusals
def test_refusals():
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    shape, params = (2, 6, 8), TR.PARAMS[0]
    seq = TR.sequence(shape)
    dev = torch.from_numpy(seq[0]).cuda()
    st = F.temporal_state(*shape)
    td = (st,) + params
    keep = st.frames.clone()
    # out aliasing the frames or the state, wholly or in part
    both = torch.zeros((3,) + shape[1:], dtype=torch.uint16).cuda()
    with pytest.raises(ValueError, match='shares memory with the frames'):
        F.raw_temporal(both[:2], td, out=both[1:])
    with pytest.raises(ValueError, match='shares memory with the frames'):
        F.raw_temporal(dev, td, out=dev)
    with pytest.raises(ValueError, match='shares memory with the temporal state'):
        F.raw_temporal(dev, td, out=st.frames)
    with pytest.raises(ValueError, match='aligned'):
        F.raw_temporal(dev, td, out=torch.zeros(dev.numel() + 4, dtype=torch.uint16).cuda()[1:1 + dev.numel()].view(shape))
    # a CPU tensor; a state of another shape; packed frames
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.raw_temporal(dev.cpu(), td)
    with pytest.raises(ValueError, match=r'\(2,6,8\)'):
        F.raw_temporal(dev, (F.temporal_state(2, 6, 12),) + params)
    with pytest.raises(ValueError, match=r'\(1,6,8\)'):
        F.raw_temporal(dev[0], td)
    with pytest.raises(ValueError, match='uint16'):
        F.raw_temporal(torch.zeros((2, 6, 10), dtype=torch.uint8).cuda(), td)
    with pytest.raises(ValueError, match='black_level'):
        F.raw_temporal(dev, td, black_level=65536)
    assert st.primed is False and torch.equal(st.frames, keep)
    # the C ABI refuses an aliasing out itself, before anything is issued
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    scratch = torch.full(shape, 0x5A5A, dtype=torch.uint16).cuda()
    for cur, state, out in ((dev, st.frames, dev), (dev, scratch, scratch), (both[:2], st.frames, both[1:])):
        assert lib.risp_raw_temporal(p(cur), p(state), p(out), 0, 64, 40, 0, 24, 64, *shape, F._stream()) != 0
        err = lib.risp_last_error()
        assert b'risp_raw_temporal' in err and b'overlaps' in err, err
    for bad, word in ((dict(strength=257), b'strength 257'), (dict(threshold=65536), b'threshold 65536'),
                      (dict(slope=256), b'slope 256'), (dict(ramp=-1), b'ramp -1'), (dict(h=2), b'H=2'), (dict(w=6), b'W 6')):
        a = dict(strength=64, threshold=40, slope=0, ramp=24, h=shape[1], w=shape[2])
        a.update(bad)
        assert lib.risp_raw_temporal(p(dev), p(st.frames), p(scratch), 0, a['strength'], a['threshold'], a['slope'], a['ramp'], 64,
                                     shape[0], a['h'], a['w'], F._stream()) != 0
        assert word in lib.risp_last_error(), (bad, lib.risp_last_error())
    torch.cuda.synchronize()
    assert (scratch.cpu() == 0x5A5A).all().item() and torch.equal(st.frames, keep), 'a refused call wrote'


def test_an_unprimed_state_under_capture_is_refused():
    import reconfigisp_amd.functional as F
    shape, params = (2, 6, 8), TR.PARAMS[0]
    seq, want = _ref(shape, params)
    slot = torch.from_numpy(seq[0]).cuda()
    st = F.temporal_state(*shape)
    out, marker = torch.zeros(shape, dtype=torch.uint16).cuda(), torch.zeros(4, device='cuda')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match='not primed'):
        with torch.cuda.graph(graph):
            marker.fill_(1.0)
            F.raw_temporal(slot, (st,) + params, TR.BLACK, out=out)
    torch.cuda.synchronize()
    assert st.primed is False and not st.frames.cpu().any().item()
    # primed by one eager call, the same call captures, and each replay advances the state
    F.raw_temporal(slot, (st,) + params, TR.BLACK, out=out)
    assert st.primed and torch.equal(out, slot)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        F.raw_temporal(slot, (st,) + params, TR.BLACK, out=out)
    for frame, ref in zip(seq[1:], want[1:]):
        slot.copy_(torch.from_numpy(frame))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(st.frames.cpu().numpy(), ref)
