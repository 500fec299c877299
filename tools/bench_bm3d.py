#!/usr/bin/env python3
"""GPU box: the classical BM3D (risp_origin_bm3d) at batch 32 x 256 x 256, the reference's initial parameters
(cff 1.5 -> sigma 3.825, cspace 0, DCT, R 8) for n1 = 8 and n1 = 4, one stream.  The whole call is timed with events;
the times of the launch families (prep / match / filter step 1 / aggregate step 1 / filter step 2 / aggregate step 2)
come from a torch.profiler kernel trace of the same calls, not from events.  Bytes per family are ALGORITHMIC, counted
from the group table of the call (the member slots K.block of 3 x n1^2 floats per member, written by a filter pass and
read by the aggregation after it, the member blocks a filter gathers, the planes each launch streams) - no hardware
counter measured them; a gathered block re-read from cache counts again, so for the filters they are an upper
estimate of the HBM traffic.  '% of 8 TB/s' divides those bytes by the family's time.
python tools/bench_bm3d.py [N H W]   (not under rocprofv3: its tracer and torch.profiler collide - a kernel trace is a run of its own)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reconfigisp_amd.functional as F
import reconfigisp_amd.lib as L

n, h, w = (int(v) for v in (sys.argv[1:4] + ['32', '256', '256'][len(sys.argv) - 1:]))
PEAK = 8e12
REPS = 10
g = torch.Generator().manual_seed(0)
x = ((torch.rand(n, 3, h, w, generator=g) * 200 + 25) + torch.randn(n, 3, h, w, generator=g) * 4).cuda()
FAMILIES = [('prep', 'bm3d_prep'), ('match', 'bm3d_match'), ('filter step 1', 'bm3d_filter_kernel<1>'),
            ('aggregate step 1', 'bm3d_aggregate_kernel<1>'), ('filter step 2', 'bm3d_filter_kernel<2>'),
            ('aggregate step 2', 'bm3d_aggregate_kernel<2>')]


def grid_n(m, n1):
    return (m - n1 + 2) // 3 + 1


def family_bytes(n1):
    refs = grid_n(h, n1) * grid_n(w, n1)
    plane = 4 * h * w
    groups = F.origin_bm3d(x, 2.55 * 1.5, n1, 0, 0, 8, want_groups=True)[1]
    members = int(groups[:, :, 0].sum())              # N2 summed over every group of the batch
    slots = 4 * members * 3 * n1 * n1                  # member slots of the batch
    return {'prep': n * plane * (3 + 1 + 3),           # read BGR, write S and the colour planes
            'match': n * (plane + refs * 17 * 4),      # S (the windows come from cache) + the group table
            'filter step 1': slots + slots,            # the member blocks gathered from Z, the slots written
            'aggregate step 1': slots + n * 3 * plane,
            'filter step 2': 2 * slots + slots,        # Z and the basic estimate gathered, the slots written
            'aggregate step 2': slots + n * 3 * plane}, slots, members / (n * refs)


def run(n1):
    return F.origin_bm3d(x, 2.55 * 1.5, n1, 0, 0, 8)[0]


print('risp_origin_bm3d  N=%d H=%d W=%d  sigma 3.825, opponent, DCT, R 8; scratch %.1f MB per image' % (
    n, h, w, L.load().risp_origin_bm3d_scratch_bytes(1, h, w) / 1e6))
for n1 in (8, 4):
    for _ in range(3):
        run(n1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        run(n1)
    e1.record()
    e1.synchronize()
    total = e0.elapsed_time(e1) / REPS
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for _ in range(REPS):
            run(n1)
        torch.cuda.synchronize()
    times = {}
    for ev in prof.key_averages():
        for fam, key in FAMILIES:
            if key in ev.key:
                dev_us = getattr(ev, 'device_time_total', None)
                if dev_us is None:
                    dev_us = ev.cuda_time_total
                times[fam] = times.get(fam, 0.0) + dev_us / REPS / 1e3
    nbytes, slot_bytes, mean_n2 = family_bytes(n1)
    print('\nn1 = %d: %.3f ms per call (events, %d calls); mean N2 %.2f, member slots %.2f GB per pass' % (
        n1, total, REPS, mean_n2, slot_bytes / 1e9))
    print('  %-18s %9s %10s %9s   (ms: torch.profiler; GB: algorithmic, from the group table)' % (
        'family', 'ms', 'GB', 'of 8TB/s'))
    for fam, _ in FAMILIES:
        t = times.get(fam)
        if t is None:
            print('  %-18s %9s %10.3f %9s' % (fam, 'n/a', nbytes[fam] / 1e9, ''))
        else:
            print('  %-18s %9.3f %10.3f %8.1f%%' % (fam, t, nbytes[fam] / 1e9, 100 * nbytes[fam] / (t * 1e-3) / PEAK))
    if times:
        print('  %-18s %9.3f' % ('sum of kernels', sum(times.values())))
