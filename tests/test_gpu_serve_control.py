"""GPU: the closed 3A loop through the serving path - ``serve(.., lens_shading=ctl.shading, statistics=st)`` followed by
``ctl.update(st)`` over the twelve frames of the scene of tests/control_reference.py, at N = 1 and N = 2, 48 x 64.

Everything is integers up to the image, so every comparison is ``torch.equal`` / ``array_equal``: state and ``.gains`` behind
every frame against ``control_reference.loop_ref`` (lens_shading_reference, stats_reference and solve_ref chained in numpy), and
the image of frame t against the same call with ``lens_shading=(the reference's map of frame t, cell)`` and no controller.
tests/test_control_reference_cpu.py shows on the reference alone that the loop settles on these scenes."""
import functools

import numpy as np
import pytest
import torch

import control_reference as CR
import raw_packed_reference as PR

pytestmark = pytest.mark.gpu

H, W = CR.SCENE_SHAPE
BLACK, WHITE, CELL = CR.SCENE_BLACK, float(CR.SCENE_WHITE), 1 << CR.SCENE_CELL_LOG2
PHASES = ('rggb', 'grbg', 'gbrg', 'bggr')


def _base_map():
    """a lens shading from ``functional.shading_map``: a vignette of 1.0 .. 1.3, a little different per plane"""
    import reconfigisp_amd.functional as F
    yy, xx = np.mgrid[0:H, 0:W]
    r2 = ((yy - H / 2) / H) ** 2 + ((xx - W / 2) / W) ** 2
    return F.shading_map(np.stack([1.0 + (0.5 + 0.05 * p) * r2 for p in range(4)]), H, W, CELL)


@functools.lru_cache(maxsize=None)
def _scene(n, cfa, seed, with_base):
    """(frames, the reference's loop over them, the base map or None) - computed once, shared, never written"""
    frames = CR.scene(n, cfa, seed)
    base = _base_map().numpy() if with_base else None
    return frames, CR.loop_ref(frames, BLACK, CR.spec_tuple(), CR.SCENE_STATS, CR.SCENE_CELL_LOG2, cfa, base=base), base


def _new(n, cfa, base):
    import reconfigisp_amd.functional as F
    zone, bins, shift, lo, hi = CR.SCENE_STATS
    st = F.raw_statistics(n, H, W, zone=zone, bins=bins, hist_shift=shift, lo=lo, hi=hi)
    ctl = F.gain_control(st, cell=CELL, base=None if base is None else torch.from_numpy(base).cuda(), cfa=PHASES[cfa])
    return st, ctl


def _assert_loop_state(ctl, want, t):
    _, state, gains = want
    got = ctl.state.cpu().numpy()
    assert np.array_equal(got, state), 'frame %d: state %s, reference %s' % (t, got.tolist(), state.tolist())
    assert np.array_equal(ctl.gains.cpu().numpy(), gains), 'frame %d: the map differs' % t


def _run_loop(call, n, cfa, seed, with_base=False, source=lambda x: torch.from_numpy(x).cuda()):
    """``call(src, **sensor)`` over the scene with the controller behind it: state and map behind every frame equal the
    reference's, the image equals the same call with the reference's map of that frame"""
    frames, want, base = _scene(n, cfa, seed, with_base)
    st, ctl = _new(n, cfa, base)
    sensor = dict(black_level=BLACK, cfa=PHASES[cfa])
    images = []
    for t, x in enumerate(frames):
        src = source(x)
        used = torch.from_numpy(want[t][0]).cuda()
        expect = call(src, lens_shading=(used, CELL), **sensor).clone()
        got = call(src, lens_shading=ctl.shading, statistics=st, **sensor)
        assert torch.equal(got, expect), 'frame %d: %d image bytes differ' % (t, (got != expect).sum().item())
        assert ctl.update(st) is ctl
        _assert_loop_state(ctl, want[t], t)
        images.append(expect)
    assert not torch.equal(images[0], images[-1]) and len(torch.unique(images[-1])) > 8
    assert want[-1][1][3] == len(frames) and want[-1][1][0] > 4096                 # twelve updates; the dark scene was lifted
    return images


def _route(what):
    import test_gpu_serve_shade as SH
    return SH._route_case(what)


# ---------------------------------------------------------------- 1. serve + update, eager
@pytest.mark.parametrize('n,cfa,seed', [(1, 0, 0), (2, 0, 1)], ids=['N1', 'N2'])
@pytest.mark.parametrize('what', ['classical', 'composed'])
def test_the_loop_through_serve_equals_the_reference(what, n, cfa, seed):
    net, kw, route = _route(what)
    _run_loop(lambda src, **sensor: net.serve(src, WHITE, **sensor, **kw), n, cfa, seed)
    assert net.last_serve_route == route and net.last_serve_stats == 'pass' and net.last_serve_shade == 'pass'


def test_with_a_base_map_from_shading_map():
    net, kw, _ = _route('classical')
    base = _base_map()
    nodes = base.to(torch.int32).view(-1, 4)
    assert base.dtype == torch.uint16 and int(nodes.max()) > 4096 + 400 and len(torch.unique(nodes, dim=0)) > 4
    _run_loop(lambda src, **sensor: net.serve(src, WHITE, **sensor), 2, 0, 1, with_base=True)


def test_with_cfa_gbrg():
    net, kw, _ = _route('classical')
    _run_loop(lambda src, **sensor: net.serve(src, WHITE, **sensor), 1, 2, 2)
    _, want, _ = _scene(1, 2, 2, False)
    assert want[-1][1][10] > want[-1][1][8] == want[-1][1][11]                  # gbrg: red is plane 2, planes 0 and 3 are green


def test_raw10_in():
    net, kw, _ = _route('classical')
    stride = W * 10 // 8 + 3

    def packed(x):
        data = PR.pack(x, 10, stride, None)
        big = torch.full((data.size + 16,), 0xFF, dtype=torch.uint8, device='cuda')
        pk = big[1:1 + data.size].view(data.shape)
        pk.copy_(torch.from_numpy(data))
        return pk

    _run_loop(lambda src, **sensor: net.serve(src, WHITE, raw_format='raw10', raw_width=W, **sensor), 2, 1, 3, source=packed)


def test_serve_frame_closes_the_loop_too():
    import test_gpu_serve_frame as SF
    model = SF._model('classical')
    _run_loop(lambda src, **sensor: model.serve_frame(src, WHITE, (24, 32), (16, 24), tile_batch=3, **sensor), 1, 0, 0)
    assert model.netG.last_serve_route == 'tiled' and model.netG.last_serve_stats == 'pass'


# ---------------------------------------------------------------- 2. serve + update in one captured graph
@pytest.mark.parametrize('n,cfa,seed', [(1, 0, 0), (2, 0, 1)], ids=['N1', 'N2'])
def test_a_captured_graph_of_serve_and_update_replays_the_loop(n, cfa, seed):
    """Capturing refuses a host wait and an allocation outside the graph's pool would not be replayed, so the capture itself shows
    that the pair waits for nothing; the replays show that state, scratch and map carry over from one replay to the next."""
    net, kw, _ = _route('classical')
    frames, want, _ = _scene(n, cfa, seed, False)
    eager = _run_loop(lambda src, **sensor: net.serve(src, WHITE, **sensor), n, cfa, seed)
    st, ctl = _new(n, cfa, None)
    sensor = dict(black_level=BLACK, cfa=PHASES[cfa])
    slot, buf = torch.from_numpy(frames[0]).cuda(), torch.zeros((n, H, W, 3), device='cuda', dtype=torch.uint8)
    net.serve(slot, WHITE, out=buf, lens_shading=ctl.shading, statistics=st, **sensor)      # one eager call fills the caches
    ctl.update(st)
    _assert_loop_state(ctl, want[0], 0)
    ctl.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.serve(slot, WHITE, out=buf, lens_shading=ctl.shading, statistics=st, **sensor)
        before = torch.cuda.memory_allocated()              # (serve keeps its shaded frames per stream: the capture's stream is new)
        ctl.update(st)
        after = torch.cuda.memory_allocated()
    assert after == before, 'the captured update allocated'
    ctl.reset()                                             # (capturing runs nothing; start the loop where the reference starts)
    for t, x in enumerate(frames):
        slot.copy_(torch.from_numpy(x))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf, eager[t]), 'replay %d: %d image bytes differ' % (t, (buf != eager[t]).sum().item())
        _assert_loop_state(ctl, want[t], t)
    assert not ctl._scratch.any().item()
