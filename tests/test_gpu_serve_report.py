"""What ``serve`` / ``serve_frame`` report about themselves (``last_serve_*``) is what their launches imply: eight settings of
the sensor side against the sixteen combinations of warp? x resize? x sharpen? x 'bgr8' / 'nv12', on a classical-route and a
composed-route pipeline.  The launches are counted (``lib.CALLS``), the mapping launches -> report is the table ``_implied``
below, and the bytes are ``F.bgr8_to_nv12?(F.bgr8_sharpen?(F.bgr8_resize?(F.bgr8_warp?(plain))))`` of the same call's image
without the output keywords."""
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raw_packed_reference as PR  # noqa: E402
import temporal_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu

WHITE, BLACK = 1023, 64
N, H, W = 2, 32, 48
OUT = (18, 26)
SHARP = (640, 2, 48, 2)
OUTPUTS = list(itertools.product((False, True), (False, True), (False, True), ('bgr8', 'nv12')))   # warp, resize, sharpen, format
INPUTS = ('plain', 'raw10', 'shading', 'defects', 'defects_shading', 'temporal', 'statistics', 'raw10_shading_statistics')
STAGE = {'warp': 'risp_bgr8_warp', 'resize': 'risp_bgr8_resize', 'sharpen': 'risp_bgr8_sharpen'}


def _counted(fn):
    from reconfigisp_amd import lib as L
    L.CALLS = {}
    try:
        out = fn()
        return out, dict(L.CALLS)
    finally:
        L.CALLS = None


def _implied(calls, kw, route):
    """the report the launches of a call with the keywords ``kw`` imply"""
    ran = lambda name: calls.get(name, 0)
    decoded = ran('risp_raw_unpack') + ran('risp_raw_shade') + ran('risp_raw_defect')
    shading, defects = 'lens_shading' in kw, 'defect_correction' in kw
    want = {'route': route,
            'load': None if 'raw_format' not in kw else ('pass' if decoded else 'fused'),
            'shade': None if not shading else ('pass' if ran('risp_raw_shade') + ran('risp_raw_defect') else 'fused'),
            'defect': None if not defects else ('fused' if shading and not ran('risp_raw_shade') else 'pass'),
            'temporal': 'pass' if ran('risp_raw_temporal') else None,
            'stats': 'pass' if ran('risp_raw_stats') else None}
    for key, launch in STAGE.items():
        assert ran(launch) in (0, 1)
        want[key] = 'pass' if ran(launch) else None
    if kw.get('out_format', 'bgr8') == 'bgr8':
        want['store'] = None
    elif ran('risp_bgr8_to_nv12'):
        want['store'] = 'pass'
    else:                                                   # the last launch stored NV12 itself: a stage's, else the route's
        want['store'] = 'sharpen' if want['sharpen'] else ('resize' if want['resize'] else 'fused')
    assert (want['temporal'] is None) == ('temporal_denoise' not in kw) and (want['stats'] is None) == ('statistics' not in kw)
    assert (want['warp'] is None) == ('warp' not in kw) and (want['sharpen'] is None) == ('sharpen' not in kw)
    assert (want['resize'] is None) == ('out_size' not in kw) and (not defects or ran('risp_raw_defect') == 1)
    return want


def _reported(net):
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    return {key: getattr(net, 'last_serve_' + key) for key in PF.SERVE_REPORT}


def _output(warp, out):
    use_warp, use_resize, use_sharpen, fmt = out
    kw = {}
    if use_warp:
        kw['warp'] = warp
    if use_resize:
        kw['out_size'] = OUT
    if use_sharpen:
        kw['sharpen'] = SHARP
    if fmt != 'bgr8':
        kw['out_format'] = fmt
    return kw


def _composed(plain, kw):
    import reconfigisp_amd.functional as F
    img = plain
    if 'warp' in kw:
        img = F.bgr8_warp(img, kw['warp'])
    if 'out_size' in kw:
        img = F.bgr8_resize(img, kw['out_size'])
    if 'sharpen' in kw:
        img = F.bgr8_sharpen(img, kw['sharpen'])
    return F.bgr8_to_nv12(img) if 'out_format' in kw else img


def _check(call, plain, plain_calls, sensor, warp, route, net, fused_store):
    """the sixteen output combinations of one sensor setting: ``call(**keywords)`` serves, ``plain`` is its image without them"""
    for out in OUTPUTS:
        kw = _output(warp, out)
        got, calls = _counted(lambda: call(**kw))
        assert _reported(net) == _implied(calls, dict(sensor, **kw), route), (out, calls)
        stages = {STAGE[key]: 1 for key in STAGE if {'warp': 'warp', 'resize': 'out_size', 'sharpen': 'sharpen'}[key] in kw}
        if stages:          # the route serves BGR as in the plain call, the stages follow, and a conversion where none stores NV12
            rest = {k: v for k, v in calls.items() if k != 'risp_bgr8_to_nv12'}
            assert rest == dict(plain_calls, **stages), (out, calls, plain_calls)
        elif kw:            # NV12 alone: the route's launch stores it where it owns such a store, else conversions follow
            assert sum(calls.values()) - calls.get('risp_bgr8_to_nv12', 0) == sum(plain_calls.values()), (calls, plain_calls)
            assert (net.last_serve_store == 'fused') == fused_store
        else:
            assert calls == plain_calls
        assert torch.equal(got, _composed(plain, kw)), out
    assert len(torch.unique(got)) > 8, 'a flat image would prove nothing'


@pytest.mark.parametrize('setting', INPUTS)
@pytest.mark.parametrize('what', ['classical', 'composed'])
def test_serve_reports_what_its_launches_imply(what, setting):
    import reconfigisp_amd.functional as F
    import test_gpu_serve_defect as GD
    import test_gpu_serve_warp as SW
    net, _, extra, route = SW._route_case(what)
    x = PR.full_range_frame(N, H, W, 10, seed=91)
    dev = torch.from_numpy(x).cuda()
    frames, sensor = dev, dict(black_level=BLACK, **extra)
    if 'raw10' in setting:
        frames = GD._place_packed(x, 10, W * 10 // 8 + 3, 1)
        sensor.update(raw_format='raw10', raw_width=W)
    if 'shading' in setting:
        sensor['lens_shading'] = GD._gains(H, W, 8, seed=92)[1]
    if 'defects' in setting:
        sensor['defect_correction'] = (16, 32, None)
    if 'statistics' in setting:
        sensor['statistics'] = F.raw_statistics(N, H, W, zone=(8, 8), bins=64, hist_shift=4, lo=64, hi=900)
    state = None
    if setting == 'temporal':
        # one primed state, put back in front of every call: each call filters the same frames over the same history
        state = F.temporal_state(N, H, W)
        sensor['temporal_denoise'] = (state,) + TR.PARAMS[0]
        net.serve(torch.from_numpy(TR.sequence((N, H, W), seed=93, steps=1)[0]).cuda(), float(WHITE), **sensor)
        history = state.frames.clone()

    def call(**kw):
        if state is not None:
            state.frames.copy_(history)
        return net.serve(frames, float(WHITE), **sensor, **kw)
    call()                                                  # (the stage parameters and the cached buffers are made once)
    plain, plain_calls = _counted(call)
    plain = plain.clone()
    assert net.last_serve_route == route
    warp = SW._warp('bilinear')[0]
    _check(call, plain, plain_calls, sensor, warp, route, net, route == 'classical')
    if 'statistics' in setting:
        assert int(sensor['statistics'].hist.sum()) == N * H * W


def test_serve_frame_reports_what_its_launches_imply():
    import test_gpu_serve_frame as SF
    import test_gpu_serve_sharpen as SS
    net = SF._model('classical').netG
    g = torch.Generator().manual_seed(9)
    h, w = 48, 64
    dev = torch.randint(0, WHITE + 1, (N, h, w), generator=g, dtype=torch.int32).to(torch.uint16).cuda()
    sensor = dict(black_level=BLACK, cfa='gbrg')

    def call(**kw):
        return net.serve_frame(dev, float(WHITE), 32, 16, tile_batch=5, **sensor, **kw)
    call()
    plain, plain_calls = _counted(call)
    plain = plain.clone()
    warp = SS._warp('bilinear', h, w)[0]
    _check(call, plain, plain_calls, sensor, warp, 'tiled', net, False)
