"""GPU: ``serve(temporal_denoise=...)`` / ``serve_frame`` - the temporal noise reduction in front of every route.

The contract (pipeline_fusion.serve): a call with the keyword returns, byte for byte, the same call without it on the frames
tests/temporal_reference.py filters from what today's pre-pass (defect correction, lens shading, the unpack) hands over, and
afterwards the caller's ``state.frames`` are those filtered frames.  Every comparison is ``torch.equal``; every case runs a
sequence - the priming frame and frames behind it - so that a state that is not advanced, or advanced twice, shows."""
import numpy as np
import pytest
import torch

import defect_reference as DR
import lens_shading_reference as LS
import raw_packed_reference as PR
import stats_reference as SR
import temporal_reference as TR

pytestmark = pytest.mark.gpu

N, H, W, BLACK, WHITE = 2, 16, 32, 64, 1023.0
PARAMS = TR.PARAMS[0]
STEPS = 3


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


def _route_case(what):
    import test_gpu_serve_shade as SH
    return SH._route_case(what)


def _sequence(seed, shape=(N, H, W), steps=STEPS):
    return TR.sequence(shape, seed=seed, steps=steps)


def _run(serve, srcs, filtered, st, params, ref_kw, kw, extra_calls=(), check=None):
    """``serve(frames, **kw)`` with the keyword over the device frames ``srcs`` against ``serve(ref, **ref_kw)`` on the
    reference's ``filtered`` frames: the same bytes, the state advanced to the filtered frames, the launches of the plain call
    plus ``extra_calls`` and one risp_raw_temporal.  Returns the images"""
    td = (st,) + params
    images = []
    for step, (src, ref) in enumerate(zip(srcs, filtered)):
        dev_ref = torch.from_numpy(ref).cuda()
        if dev_ref.dim() == 3 and srcs[0].dim() == 2:
            dev_ref = dev_ref[0]
        want = serve(dev_ref, **ref_kw).clone()
        _, plain_calls = _counted(lambda: serve(dev_ref, **ref_kw))
        got, calls = _counted(lambda: serve(src, temporal_denoise=td, **kw))
        expect = dict(plain_calls, risp_raw_temporal=1)
        for name in extra_calls:
            expect[name] = expect.get(name, 0) + 1
        assert calls == expect, (step, calls, plain_calls)
        assert torch.equal(got, want), 'step %d: %d bytes differ' % (step, (got != want).sum().item())
        assert st.primed and np.array_equal(st.frames.cpu().numpy(), ref), 'step %d: the state is not the filtered frames' % step
        if check is not None:
            check(step, ref)
        images.append(want)
    assert not torch.equal(images[0], images[1])
    return images


# ---------------------------------------------------------------- 1. every kind of route, another cfa
@pytest.mark.parametrize('what', ['fused', 'classical', 'composed', 'denoise'])
def test_serve_filters_in_front_of_every_route(what):
    import reconfigisp_amd.functional as F
    net, kw, route = _route_case(what)
    seq = _sequence(seed=11)
    filtered, _ = TR.run_ref(seq, *PARAMS, BLACK)
    assert not np.array_equal(filtered[1], seq[1])
    srcs = [torch.from_numpy(f).cuda() for f in seq]
    for cfa in ('rggb', 'gbrg'):
        st = F.temporal_state(N, H, W)
        sensor = dict(white_level=WHITE, black_level=BLACK, cfa=cfa, **kw)

        def check(step, ref):
            assert net.last_serve_route == route and net.last_serve_temporal == 'pass' and net.last_serve_load is None
        _run(net.serve, srcs, filtered, st, PARAMS, sensor, sensor, check=check)
    # None passed explicitly is the call without the keyword: today's bytes, today's calls, the state left alone
    keep = st.frames.clone()
    plain, today = _counted(lambda: net.serve(srcs[0], WHITE, black_level=BLACK, **kw))
    plain = plain.clone()
    none, none_calls = _counted(lambda: net.serve(srcs[0], WHITE, black_level=BLACK, temporal_denoise=None, **kw))
    assert torch.equal(none, plain) and none_calls == today and 'risp_raw_temporal' not in none_calls
    assert net.last_serve_temporal is None and torch.equal(st.frames, keep)
    # out= given and a primed state: a warm call allocates nothing
    buf = torch.empty_like(plain)
    net.serve(srcs[1], WHITE, out=buf, black_level=BLACK, temporal_denoise=(st,) + PARAMS, **kw)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert net.serve(srcs[2], WHITE, out=buf, black_level=BLACK, temporal_denoise=(st,) + PARAMS, **kw) is buf
    if what != 'composed':                                  # (the composed route allocates its fp32 planes either way)
        assert torch.cuda.memory_allocated() == before


# ---------------------------------------------------------------- 2. RAW10 in: unpacked first, no fused packed load
@pytest.mark.parametrize('what', ['classical', 'fused'])
def test_serve_filters_packed_frames_behind_the_unpack(what):
    import reconfigisp_amd.functional as F
    net, kw, route = _route_case(what)
    seq = _sequence(seed=12)
    filtered, _ = TR.run_ref(seq, *PARAMS, BLACK)
    srcs = []
    for f in seq:
        data = PR.pack(f, 10, W * 10 // 8 + 3, None)
        big = torch.full((data.size + 16,), 0xFF, dtype=torch.uint8, device='cuda')
        pk = big[1:1 + data.size].view(data.shape)
        pk.copy_(torch.from_numpy(data))
        srcs.append(pk)
    st = F.temporal_state(N, H, W)
    sensor = dict(white_level=WHITE, black_level=BLACK, cfa='grbg', **kw)

    def check(step, ref):
        assert net.last_serve_route == route and net.last_serve_temporal == 'pass' and net.last_serve_load == 'pass'
    _run(net.serve, srcs, filtered, st, PARAMS, sensor, dict(sensor, raw_format='raw10', raw_width=W),
         extra_calls=('risp_raw_unpack',), check=check)


# ---------------------------------------------------------------- 3. behind defect correction, lens shading, and both
@pytest.mark.parametrize('pre', ['defect', 'shade', 'both'])
@pytest.mark.parametrize('what', ['classical', 'fused'])
def test_serve_filters_behind_the_pre_passes(what, pre):
    import test_gpu_serve_shade as SH
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    net, kw, route = _route_case(what)
    cell = 8
    seq = _sequence(seed=13)
    gains = LS.random_map(H, W, 3, seed=14, lo=3500, hi=4700)
    shading = (SH._place_map(gains), cell)
    handed = seq
    serve_kw, extra = {}, []
    if pre in ('defect', 'both'):
        handed = [DR.dpc_ref(f, 16, 32, None) for f in handed]
        serve_kw['defect_correction'] = (16, 32, None)
        extra.append('risp_raw_defect')
    white, black = WHITE, BLACK
    if pre in ('shade', 'both'):
        handed = [LS.shade_ref(f, BLACK, gains, 3) for f in handed]
        serve_kw['lens_shading'] = shading
        if pre == 'shade' or PF.defect_shade('u16') == 'pass':
            extra.append('risp_raw_shade')
        white, black = WHITE - BLACK, 0                     # behind a shading the samples have black level 0
    assert any(not np.array_equal(a, b) for a, b in zip(handed, seq))
    filtered, _ = TR.run_ref(handed, *PARAMS, black)
    st = F.temporal_state(N, H, W)
    srcs = [torch.from_numpy(f).cuda() for f in seq]

    def check(step, ref):
        assert net.last_serve_route == route and net.last_serve_temporal == 'pass'
        assert net.last_serve_shade == (None if pre == 'defect' else 'pass')
        assert (net.last_serve_defect is None) == (pre == 'shade')
    _run(net.serve, srcs, filtered, st, PARAMS, dict(white_level=white, black_level=black, cfa='grbg', **kw),
         dict(white_level=WHITE, black_level=BLACK, cfa='grbg', **serve_kw, **kw), extra_calls=extra, check=check)


# ---------------------------------------------------------------- 4. statistics read the filtered frames
def test_statistics_are_those_of_the_filtered_frames():
    import reconfigisp_amd.functional as F
    net, kw, route = _route_case('classical')
    zone, bins, shift, lo, hi = (4, 8), 16, 6, BLACK, 900
    seq = _sequence(seed=15)
    filtered, _ = TR.run_ref(seq, *PARAMS, BLACK)
    st = F.temporal_state(N, H, W)
    stats = F.raw_statistics(N, H, W, zone=zone, bins=bins, hist_shift=shift, lo=lo, hi=hi)
    sensor = dict(white_level=WHITE, black_level=BLACK, cfa='grbg')

    def check(step, ref):
        zones, hist = SR.stats_ref(ref, BLACK, zone, bins, shift, lo, hi)
        assert np.array_equal(stats.zones.cpu().numpy(), zones) and np.array_equal(stats.hist.cpu().numpy(), hist), step
        assert net.last_serve_stats == 'pass' and net.last_serve_temporal == 'pass'
    srcs = [torch.from_numpy(f).cuda() for f in seq]
    _run(net.serve, srcs, filtered, st, PARAMS, sensor, dict(sensor, statistics=stats), extra_calls=('risp_raw_stats',), check=check)
    zones_plain, _ = SR.stats_ref(seq[-1], BLACK, zone, bins, shift, lo, hi)
    assert not np.array_equal(stats.zones.cpu().numpy(), zones_plain)


# ---------------------------------------------------------------- 5. NV12 out, a resized output
@pytest.mark.parametrize('what', ['classical', 'composed'])
def test_nv12_and_a_resized_output(what):
    import reconfigisp_amd.functional as F
    net, kw, route = _route_case(what)
    seq = _sequence(seed=16)
    filtered, _ = TR.run_ref(seq, *PARAMS, BLACK)
    srcs = [torch.from_numpy(f).cuda() for f in seq]
    for out_kw in (dict(out_format='nv12', yuv_matrix='bt709_full'), dict(out_size=(8, 16), resample='bicubic'),
                   dict(out_format='nv12', out_size=(8, 16), out_window=(2, 4, 12, 24))):
        st = F.temporal_state(N, H, W)
        sensor = dict(white_level=WHITE, black_level=BLACK, cfa='grbg', **out_kw, **kw)
        images = _run(net.serve, srcs, filtered, st, PARAMS, sensor, sensor)
        assert net.last_serve_route == route
        assert tuple(images[0].shape) == ((N, 12, 16) if 'out_size' in out_kw and 'out_format' in out_kw else
                                          (N, H + H // 2, W) if 'out_format' in out_kw else (N, 8, 16, 3))


# ---------------------------------------------------------------- 6. full frames in tiles
@pytest.mark.parametrize('single', [False, True], ids=['stack', 'frame'])
def test_serve_frame_filters_once_in_front_of_the_tiles(single):
    import test_gpu_serve_frame as SF
    import reconfigisp_amd.functional as F
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    model = SF._model('classical')
    net = model.netG
    n, h, w = (1 if single else 2), 34, 68
    size, stride = (20, 40), (14, 28)                       # a 2 x 2 tile geometry
    assert PF.frame_geometry(h, w, size, stride, 'gbrg', 'cuda')[0].shape[0] == 4
    seq = _sequence(seed=17, shape=(n, h, w))
    filtered, _ = TR.run_ref(seq, *PARAMS, BLACK)
    srcs = [torch.from_numpy(f[0] if single else f).cuda() for f in seq]
    st = F.temporal_state(n, h, w)
    kw = dict(white_level=WHITE, patch_size=size, patch_stride=stride, tile_batch=3, cfa='gbrg', black_level=BLACK)

    def check(step, ref):
        assert net.last_serve_route == 'tiled' and net.last_serve_temporal == 'pass'
    images = _run(model.serve_frame, srcs, filtered, st, PARAMS, kw, kw, check=check)
    assert tuple(images[0].shape) == ((h, w, 3) if single else (n, h, w, 3))
    net.serve_frame(srcs[0], **kw)
    assert net.last_serve_temporal is None
    # a state for another number of images is refused before anything is launched
    with pytest.raises(ValueError, match=r'\(%d,34,68\)' % n):
        net.serve_frame(srcs[0], temporal_denoise=(F.temporal_state(n + 1, h, w),) + PARAMS, **kw)


def test_the_model_wrapper_passes_the_keyword_on():
    import test_gpu_serve_frame as SF
    import reconfigisp_amd.functional as F
    model = SF._model('classical')
    seq = _sequence(seed=18)
    filtered, _ = TR.run_ref(seq, *PARAMS, BLACK)
    st = F.temporal_state(N, H, W)
    sensor = dict(white_level=WHITE, black_level=BLACK)
    _run(model.serve, [torch.from_numpy(f).cuda() for f in seq], filtered, st, PARAMS, sensor, sensor)
    assert model.netG.last_serve_temporal == 'pass'


# ---------------------------------------------------------------- 7. refusals come before anything is launched
def test_refusals_leave_the_state_alone():
    import reconfigisp_amd.functional as F
    net, kw, route = _route_case('classical')
    src = torch.from_numpy(_sequence(seed=19)[0]).cuda()
    st = F.temporal_state(N, H, W)
    for td, word in (((st, 257, 40, 0, 24), 'strength'), ((st, 64, 40, 0), 'state, strength'),
                     ((F.temporal_state(N, H, W + 4), 64, 40, 0, 24), r'\(2,16,32\)'), ((st.frames, 64, 40, 0, 24), 'TemporalState')):
        _, calls = _counted(lambda: pytest.raises(ValueError, net.serve, src, WHITE, black_level=BLACK, temporal_denoise=td).match(word))
        assert calls == {}, (td[1:], calls)
    assert st.primed is False and not st.frames.cpu().any().item()


# ---------------------------------------------------------------- 8. a captured graph advances the state on every replay
@pytest.mark.parametrize('what', ['fused', 'classical'])
def test_a_graph_captured_once_replays_the_recursion(what):
    import reconfigisp_amd.functional as F
    net, kw, route = _route_case(what)
    seq = _sequence(seed=20, steps=5)
    filtered, _ = TR.run_ref(seq, *PARAMS, BLACK)
    sensor = dict(black_level=BLACK, cfa='grbg', **kw)
    eager = [net.serve(torch.from_numpy(f).cuda(), WHITE, **sensor).clone() for f in filtered]
    st = F.temporal_state(N, H, W)
    td = (st,) + PARAMS
    slot, buf = torch.from_numpy(seq[0]).cuda(), torch.zeros((N, H, W, 3), device='cuda', dtype=torch.uint8)
    # an unprimed state is refused while the stream is capturing, before anything is captured
    net.serve(slot, WHITE, out=buf, **sensor)               # fills the caches of the plain call
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match='not primed'):
        with torch.cuda.graph(graph):
            buf.zero_()
            net.serve(slot, WHITE, out=buf, temporal_denoise=td, **sensor)
    torch.cuda.synchronize()
    assert st.primed is False
    # primed with one eager call, warmed with a second
    net.serve(slot, WHITE, out=buf, temporal_denoise=td, **sensor)
    assert net.last_serve_route == route and torch.equal(buf, eager[0]) and st.primed
    slot.copy_(torch.from_numpy(seq[1]))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    net.serve(slot, WHITE, out=buf, temporal_denoise=td, **sensor)
    assert torch.cuda.memory_allocated() == before
    assert torch.equal(buf, eager[1]) and np.array_equal(st.frames.cpu().numpy(), filtered[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.serve(slot, WHITE, out=buf, temporal_denoise=td, **sensor)
    assert np.array_equal(st.frames.cpu().numpy(), filtered[1]), 'capturing ran nothing'
    for step in (2, 3, 4):
        slot.copy_(torch.from_numpy(seq[step]))
        buf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf, eager[step]), step
        assert np.array_equal(st.frames.cpu().numpy(), filtered[step]), 'replay %d did not advance the state' % step
