#!/usr/bin/env python3
"""GPU box: DemosaicNet (random He-scale weights: the cost does not depend on their values) against PathRestore14lBayer on the same
mosaic, in the same process, in alternating runs.  Cases: batch 32 x 256 x 256 (inference, and forward + backward to the mosaic),
the shipped search geometry 4 x 48 x 48 (both), one 4000 x 3000 frame (inference).  Whole calls are timed with HIP events (median
of REPS alternating pairs); the share of the four risp_dmnet launches comes from a torch.profiler kernel trace of the same calls
(forward: a training forward without backward; backward: forward + backward minus that forward).
python tools/bench_demosaicnet.py   (not under rocprofv3: its tracer and torch.profiler collide)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import torch

import demosaicnet_reference as R
import reconfigisp_amd.functional as F
from reconfigisp_amd import demosaicnet as DN
from reconfigisp_amd.codes.models.modules.tools_proxy import PathRestore14lBayer

REPS = 10
NET = DN.load_demosaicnet(R.random_state_dict(0))
torch.manual_seed(0)
PATH = PathRestore14lBayer(0, None).cuda()
NEW_FWD, NEW_BWD = ('dmnet_tail_fwd', 'dmnet_head_fwd'), ('dmnet_tail_bwd', 'dmnet_head_bwd')


def call(which, x, mode):
    op = (lambda t: F.demosaicnet(t, NET)) if which == 'dmnet' else (lambda t: PATH(t, None))
    if mode == 'infer':
        with torch.no_grad():
            return op(x)
    xg = x.detach().requires_grad_(True)
    y = op(xg)
    if mode == 'fwd':
        return y
    gx, = torch.autograd.grad(y, xg, torch.ones_like(y))
    return gx


def timed(which, x, mode):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call(which, x, mode)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_ms(x, mode):
    """(total, risp_dmnet forward launches, risp_dmnet backward launches, {launch: ms}) in ms per call from a kernel trace"""
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for _ in range(REPS):
            call('dmnet', x, mode)
        torch.cuda.synchronize()
    tot = fwd = bwd = 0.0
    each = {}
    for ev in prof.key_averages():
        us = getattr(ev, 'device_time_total', None)
        if us is None:
            us = ev.cuda_time_total
        if ev.device_type != torch.autograd.DeviceType.CUDA and us == 0:
            continue
        if any(k in ev.key for k in ('Memcpy', 'Memset')) or ev.key.startswith('aten::') or ev.key.startswith('autograd::'):
            continue
        ms = us / REPS / 1e3
        tot += ms
        fwd += ms if any(k in ev.key for k in NEW_FWD) else 0.0
        bwd += ms if any(k in ev.key for k in NEW_BWD) else 0.0
        for k in NEW_FWD + NEW_BWD:
            if k in ev.key:
                each[k] = each.get(k, 0.0) + ms
    return tot, fwd, bwd, each


def split(each):
    return ', '.join('%s %.3f' % (k, v) for k, v in sorted(each.items()))


def case(n, h, w, modes):
    x = torch.rand(n, 1, h, w, generator=torch.Generator().manual_seed(1)).cuda()
    print('\n%d x %d x %d mosaic' % (n, h, w))
    for mode in modes:
        for _ in range(2):
            call('dmnet', x, mode)
            call('path', x, mode)
        torch.cuda.synchronize()
        td, tp = [], []
        for _ in range(REPS):                                  # alternating runs
            td.append(timed('dmnet', x, mode))
            tp.append(timed('path', x, mode))
        md, mp = sorted(td)[REPS // 2], sorted(tp)[REPS // 2]
        print('  %-8s DemosaicNet %9.3f ms   PathRestore14lBayer %9.3f ms   ratio %.2f' % (
            {'infer': 'infer', 'fwdbwd': 'fwd+bwd'}[mode], md, mp, md / mp))
        if mode == 'infer':
            tot, fwd, _, each = kernel_ms(x, 'infer')
            print('           kernels %.3f ms, the two new forward launches %.3f ms = %.1f %% of the forward (%s)' % (
                tot, fwd, 100 * fwd / tot, split(each)))
        else:
            tf, ff, _, _ = kernel_ms(x, 'fwd')
            tt, _, bb, each = kernel_ms(x, 'fwdbwd')
            print('           training forward kernels %.3f ms, new launches %.3f ms = %.1f %%; backward kernels %.3f ms, new '
                  'launches %.3f ms = %.1f %%\n           (%s)' % (tf, ff, 100 * ff / tf, tt - tf, bb, 100 * bb / (tt - tf), split(each)))


print('DemosaicNet vs PathRestore14lBayer, RISP_CONV_ARITH=%s; HIP events, median of %d alternating runs; shares from torch.profiler'
      % (os.environ.get('RISP_CONV_ARITH', 'f16x2'), REPS))
case(32, 256, 256, ('infer', 'fwdbwd'))
case(4, 48, 48, ('infer', 'fwdbwd'))
case(1, 4000, 3000, ('infer',))
