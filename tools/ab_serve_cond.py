#!/usr/bin/env python3
"""GPU box: the histogram launch of the conditional route (risp_serve_cond_hist: its memset and its kernel) alone, for one
build of the library - the committed one, or an ablation build with another shard count or another number of private LDS
histograms per workgroup:

    make -C reconfigisp_amd/csrc OUT=/tmp/ab/s8.so OBJDIR=/tmp/ab/s8 EXTRA="-DRISP_COND_AB_SHARDS=8"
    make -C reconfigisp_amd/csrc OUT=/tmp/ab/c16.so OBJDIR=/tmp/ab/c16 EXTRA="-DRISP_COND_AB_COPIES=16"
    RISP_HIP_LIBRARY=/tmp/ab/s8.so python tools/ab_serve_cond.py --label "8 shards, 64 copies"

One process per build (run them one after the other on one box and compare the medians; the spread between the rounds of one
build is the noise).  Nearest demosaic, no prefix, 4 and 8 bins, 64 x 256 x 256 and 1 x 3000 x 4000; the C ABI is called
directly with a counts buffer large enough for 64 shards, so the Python side's shard count does not enter.  The counts of
every build are checked against each other through their total (the pixels inside [0,1] x 3)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import reconfigisp_amd.functional as F  # noqa: E402
from reconfigisp_amd import lib as L  # noqa: E402
from reconfigisp_amd.codes.data.synthetic_raw import make_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--label', default='committed build')
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    lib = L.load()
    print('tools/ab_serve_cond.py  %s  (%s)' % (args.label, L.LIB_PATH), flush=True)
    for n, h, w in ((64, 256, 256), (1, 3000, 4000)):
        bay = make_batch(n, h, w, seed=10)[0][:, 0]
        raw = (bay * 1023.0).round().clamp(0, 1023).to(torch.int32).to(torch.uint16).cuda()
        for bins in (4, 8):
            counts = torch.empty((n, 64, 3 * bins), device='cuda', dtype=torch.int32)
            ops, blocks = (C.c_int * 1)(0), L.ptr_array([None])

            def call():
                return lib.risp_serve_cond_hist(C.c_void_p(raw.data_ptr()), 1023.0, 0, 0, ops, blocks, bins, C.c_void_p(counts.data_ptr()),
                                                n, h, w, 0, 0, F._stream())

            counts.zero_()
            assert call() == 0, lib.risp_last_error()
            torch.cuda.synchronize()
            total = counts.sum().item()
            rounds = []
            for _ in range(args.rounds):
                for _ in range(3):
                    call()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    call()
                e1.record()
                e1.synchronize()
                rounds.append(e0.elapsed_time(e1) / args.reps * 1e3)
            print('  %d x %d x %d, %d bins: median %.1f us  min %.1f  spread %.1f   (counted %d of %d values)' % (
                n, h, w, bins, sorted(rounds)[len(rounds) // 2], min(rounds), max(rounds) - min(rounds), total, 3 * n * h * w), flush=True)


if __name__ == '__main__':
    main()
