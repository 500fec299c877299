#!/usr/bin/env python3
"""GPU box: a sensor pre-pass alone in several builds of the library, in interleaved rounds in one process - how many rows a thread
of risp_raw_defect walks (ROWS, the register ring's reuse against the number of threads), the parent commit's kernels beside the
tree's, and any other variant of a kernel given as a build.

    for R in 4 16; do make -C reconfigisp_amd/csrc OUT=/tmp/rows$R/libreconfigisp_hip.so OBJDIR=/tmp/rows$R EXTRA=-DRISP_DEFECT_ROWS=$R; done
    python tools/bench_serve_defect_rows.py rows4=/tmp/rows4/libreconfigisp_hip.so rows16=/tmp/rows16/libreconfigisp_hip.so [--out FILE]
    python tools/bench_serve_defect_rows.py --call all --formats u16,u16+2,raw10,raw12 parent=/tmp/parent/libreconfigisp_hip.so

Leg `tree` is the in-tree library; every NAME=PATH adds a leg with that build's entry point bound to the same signature.  --call:
defect (the default), shade, temporal, stats or all, each through its functional.raw_* wrapper, host side included: frames, sizes
and parameters as in leg (a) of tools/bench_serve_defect.py / _shade / _temporal / _stats, on resident frames, 64 x 256 x 256 and
3000 x 4000, 7 rounds after one that is not kept.  --formats: u16, raw10, raw12, and u16+2 for uint16 frames one word into their
allocation (2-byte aligned only: the single-sample loads); temporal takes the uint16 ones.  All builds read and fill the same
buffers, and their results are compared first.  Per row and build the rule of tools/serve_bench.py says whether that build beats
the tree."""
import numpy as np
import torch

import serve_bench as SB
import reconfigisp_amd.functional as F
from bench_serve_defect import BLACK, CELL, LISTED, SLOPE, THRESHOLD, WHITE
from bench_serve_stats import BINS, HI, LO, SHIFT
from bench_serve_temporal import PARAMS

CALLS = ('defect', 'shade', 'temporal', 'stats')
FORMATS = {'u16': 16, 'u16+2': 16, 'raw10': 10, 'raw12': 12}
ZONES = {256: (32, 32), 3000: (200, 200)}           # by frame height, as tools/bench_serve_stats.py


def prepare(call, raw, bits, shape, seed):
    """(reset(), leg(): one call of the wrapper, the tensors it fills).  Every build fills the same tensors: where a buffer lies
    moves a call by more than the builds differ (2 us of 33 between two processes), so no build gets buffers of its own"""
    n, h, w = shape
    if call == 'stats':
        st = F.raw_statistics(n, h, w, zone=ZONES[h], bins=BINS, hist_shift=SHIFT, lo=LO, hi=HI)
        return (lambda: None), (lambda: F.raw_stats(raw, st, BLACK, bits, w)), (st.zones, st.hist)
    out = torch.zeros(shape, device='cuda', dtype=torch.uint16)
    if call == 'defect':
        rng = np.random.default_rng(seed)
        coords = np.stack([rng.integers(0, h, int(h * w * LISTED)), rng.integers(0, w, int(h * w * LISTED))], axis=1)
        dc = (THRESHOLD, SLOPE, F.defect_map(coords, h, w).cuda())
        return (lambda: None), (lambda: F.raw_defect(raw, dc, bits, w, out=out)), (out,)
    if call == 'shade':
        shading = (F.shading_map(SB.vignette(h, w), h, w, CELL).cuda(), CELL)
        return (lambda: None), (lambda: F.raw_shade(raw, shading, BLACK, bits, w, out=out)), (out,)
    # temporal: one state that every call advances; reset() puts it back to its start
    start = (SB.frames_int(n, h, w, seed + 1, int(WHITE) - BLACK) + BLACK).to(torch.uint16).cuda()
    td = (F.temporal_state(n, h, w),) + PARAMS
    td[0].primed = True
    return (lambda: td[0].frames.copy_(start)), (lambda: F.raw_temporal(raw, td, BLACK, out=out)), (out, td[0].frames)


def main():
    ap = SB.parser(300, 7)
    ap.add_argument('builds', nargs='*', help='NAME=PATH of another build of libreconfigisp_hip.so')
    ap.add_argument('--call', default='defect', choices=CALLS + ('all',))
    ap.add_argument('--formats', default='u16,raw10', help='of ' + ', '.join(FORMATS))
    args = ap.parse_args()
    calls = {c: 'risp_raw_' + c for c in (CALLS if args.call == 'all' else (args.call,))}
    builds = SB.load_builds(args.builds, calls.values())
    emit = SB.Report(args.out)
    emit('tools/bench_serve_defect_rows.py --call %s --formats %s %s   (%s)' % (
        args.call, args.formats, ' '.join(n for n in builds if n != 'tree'), torch.cuda.get_device_name(0)))
    beaten = []
    for call, entry in calls.items():
        for fmt in args.formats.split(','):
            bits = FORMATS[fmt]
            if call == 'temporal' and bits != 16:
                continue
            for (n, h, w), seed, reps in (((64, 256, 256), 10, args.reps), ((1, 3000, 4000), 20, max(20, args.reps // 3))):
                x = SB.frames_int(n, h, w, seed, int(WHITE) - BLACK) + BLACK
                raw = (x.to(torch.uint16) if bits == 16 else SB.pack(x, bits)).cuda()
                if fmt == 'u16+2':
                    big = torch.zeros(raw.numel() + 4, device='cuda', dtype=torch.uint16)
                    big[1:1 + raw.numel()].copy_(raw.view(-1))
                    raw = big[1:1 + raw.numel()].view(n, h, w)
                    assert raw.data_ptr() % 8 == 2
                reset, leg, filled = prepare(call, raw, bits, (n, h, w), seed)
                won = SB.compare_builds(emit, '%s, %s, %d x %d x %d' % (call, fmt, n, h, w), builds, entry, leg, filled, reps,
                                        args.rounds, reset)
                beaten += ['%s %s %dx%dx%d by %s' % (call, fmt, n, h, w, name) for name in won]
    emit(SB.beaten_line(beaten))
    emit.write()


if __name__ == '__main__':
    main()
