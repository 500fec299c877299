#!/usr/bin/env python3
"""GPU box: risp_raw_defect alone in several builds of the library, in interleaved rounds in one process - how many rows a thread
walks (ROWS, the register ring's reuse against the number of threads) and any other variant of the kernel given as a build.

    for R in 4 16; do make -C reconfigisp_amd/csrc OUT=/tmp/rows$R/libreconfigisp_hip.so OBJDIR=/tmp/rows$R EXTRA=-DRISP_DEFECT_ROWS=$R; done
    python tools/bench_serve_defect_rows.py rows4=/tmp/rows4/libreconfigisp_hip.so rows16=/tmp/rows16/libreconfigisp_hip.so [--out FILE]

Leg `tree` is the in-tree library; every NAME=PATH adds a leg with that build's risp_raw_defect bound to the same signature.  Frames,
sizes, parameters and timing as in tools/bench_serve_defect.py leg (a): functional.raw_defect(raw, (32, 16, map), out=) on resident
u16 and raw10 frames, 64 x 256 x 256 and 3000 x 4000, 7 rounds after one that is not kept; the outputs of all builds are compared
first."""
import numpy as np
import torch

import serve_bench as SB
import reconfigisp_amd.functional as F
from reconfigisp_amd import lib as L
from bench_serve_defect import BLACK, LISTED, SLOPE, THRESHOLD, WHITE

CALL = 'risp_raw_defect'


def main():
    ap = SB.parser(300, 7)
    ap.add_argument('builds', nargs='*', help='NAME=PATH of another build of libreconfigisp_hip.so')
    args = ap.parse_args()
    own = getattr(L.load(), CALL)
    fns = {'tree': own}
    for item in args.builds:
        name, path = item.split('=', 1)
        fns[name] = getattr(SB.load_parent(path, [CALL]), CALL)
    emit = SB.Report(args.out)
    emit('tools/bench_serve_defect_rows.py %s   (%s)' % (' '.join(n for n in fns if n != 'tree'), torch.cuda.get_device_name(0)))
    for fmt, bits in (('u16', 16), ('raw10', 10)):
        for (n, h, w), seed, reps in (((64, 256, 256), 10, args.reps), ((1, 3000, 4000), 20, max(20, args.reps // 3))):
            x = SB.frames_int(n, h, w, seed, int(WHITE) - BLACK) + BLACK
            raw = (x.to(torch.uint16) if fmt == 'u16' else SB.pack(x, bits)).cuda()
            rng = np.random.default_rng(seed)
            coords = np.stack([rng.integers(0, h, int(h * w * LISTED)), rng.integers(0, w, int(h * w * LISTED))], axis=1)
            dc = (THRESHOLD, SLOPE, F.defect_map(coords, h, w).cuda())
            outs = {k: torch.zeros((n, h, w), device='cuda', dtype=torch.uint16) for k in fns}

            def timed_build(leg, reps):                     # a leg is (a build's risp_raw_defect, the output it fills)
                build, out = leg
                L._FN[CALL] = build
                return SB.timed(lambda: F.raw_defect(raw, dc, bits, w, out=out), reps)

            try:
                res = SB.rounds_of({name: (fn, outs[name]) for name, fn in fns.items()}, reps, args.rounds, True, timed_build)
            finally:
                L._FN[CALL] = own
            torch.cuda.synchronize()
            assert all(torch.equal(o, outs['tree']) for o in outs.values()), 'the builds disagree'
            emit(' %s, %d x %d x %d, %d calls per round; us per call' % (fmt, n, h, w, reps))
            for name, v in res.items():
                emit('  %-10s median %.1f us  min %.1f  spread %.1f   rounds %s' % (
                    name, SB.median(v), min(v), SB.spread(v), ' '.join('%.1f' % t for t in v)))
    emit.write()


if __name__ == '__main__':
    main()
