#!/usr/bin/env python3
"""GPU box: risp_raw_defect alone in several builds of the library, in interleaved rounds in one process - how many rows a thread
walks (ROWS, the register ring's reuse against the number of threads) and any other variant of the kernel given as a build.

    for R in 4 16; do make -C reconfigisp_amd/csrc OUT=/tmp/rows$R/libreconfigisp_hip.so OBJDIR=/tmp/rows$R EXTRA=-DRISP_DEFECT_ROWS=$R; done
    python tools/bench_serve_defect_rows.py rows4=/tmp/rows4/libreconfigisp_hip.so rows16=/tmp/rows16/libreconfigisp_hip.so [--out FILE]

Leg `tree` is the in-tree library; every NAME=PATH adds a leg with that build's risp_raw_defect bound to the same signature.  Frames,
sizes, parameters and timing as in tools/bench_serve_defect.py leg (a): functional.raw_defect(raw, (32, 16, map), out=) on resident
u16 and raw10 frames, 64 x 256 x 256 and 3000 x 4000, 7 rounds after one that is not kept; the outputs of all builds are compared
first."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import reconfigisp_amd.functional as F  # noqa: E402
from reconfigisp_amd import lib as L  # noqa: E402
from bench_serve_defect import BLACK, LISTED, SLOPE, THRESHOLD, WHITE  # noqa: E402
from bench_serve_packed import frames_int, pack, timed  # noqa: E402

CALL = 'risp_raw_defect'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('builds', nargs='*', help='NAME=PATH of another build of libreconfigisp_hip.so')
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    own = getattr(L.load(), CALL)
    fns = {'tree': own}
    for item in args.builds:
        name, path = item.split('=', 1)
        fn = getattr(C.CDLL(os.path.abspath(path)), CALL)
        fn.restype, fn.argtypes = L.SIGNATURES[CALL]
        fns[name] = fn
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit('tools/bench_serve_defect_rows.py %s   (%s)' % (' '.join(n for n in fns if n != 'tree'), torch.cuda.get_device_name(0)))
    for fmt, bits in (('u16', 16), ('raw10', 10)):
        for (n, h, w), seed, reps in (((64, 256, 256), 10, args.reps), ((1, 3000, 4000), 20, max(20, args.reps // 3))):
            x = frames_int(n, h, w, seed, int(WHITE) - BLACK) + BLACK
            raw = (x.to(torch.uint16) if fmt == 'u16' else pack(x, bits)).cuda()
            rng = np.random.default_rng(seed)
            coords = np.stack([rng.integers(0, h, int(h * w * LISTED)), rng.integers(0, w, int(h * w * LISTED))], axis=1)
            dc = (THRESHOLD, SLOPE, F.defect_map(coords, h, w).cuda())
            outs = {k: torch.zeros((n, h, w), device='cuda', dtype=torch.uint16) for k in fns}
            res = {k: [] for k in fns}
            try:
                for r in range(args.rounds + 1):
                    for name, fn in fns.items():
                        L._FN[CALL] = fn
                        t = timed(lambda: F.raw_defect(raw, dc, bits, w, out=outs[name]), reps)
                        if r:
                            res[name].append(t)
            finally:
                L._FN[CALL] = own
            torch.cuda.synchronize()
            assert all(torch.equal(o, outs['tree']) for o in outs.values()), 'the builds disagree'
            emit(' %s, %d x %d x %d, %d calls per round; us per call' % (fmt, n, h, w, reps))
            for name, v in res.items():
                emit('  %-10s median %.1f us  min %.1f  spread %.1f   rounds %s' % (
                    name, sorted(v)[len(v) // 2], min(v), max(v) - min(v), ' '.join('%.1f' % t for t in v)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
