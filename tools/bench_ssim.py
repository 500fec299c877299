#!/usr/bin/env python3
"""GPU box: F.ssim (risp_ssim_fwd / risp_ssim_bwd) beside (a) the same quantity composed from torch ops - the avg_pool2d form of
tests/ssim_reference.py on the same fp32 tensors, what a user has without the kernels - and (b) F.pixel_loss on the same tensors,
which reads the same two planes once (and writes one gradient plane): the byte floor.  Forward (no autograd) and forward + backward
to x, at 32 x 3 x 256 x 256, 4 x 3 x 48 x 48 and 1 x 3 x 3000 x 4000.  HIP events around blocks of calls, the three variants
alternating block by block in one process, CALLS calls per variant after warm-up; per-call time = median over the blocks.
Algorithmic bytes: 8 per pixel and channel forward (read x, y), 20 forward + backward (8 + read x, y, write gx) - the HBM share is
those bytes over the call's time against the 8.0 TB/s peak of MI355X_MICROARCH (6.29 TB/s is what a float4 copy reaches).
python tools/bench_ssim.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import torch

import reconfigisp_amd.functional as F
import ssim_reference as R

CALLS, BLOCKS = 200, 10
HBM_PEAK = 8.0e12


def variants(x, y):
    def fwd(op):
        def run():
            with torch.no_grad():
                return op(x, y)
        return run

    def fwdbwd(op):
        def run():
            xg = x.detach().requires_grad_(True)
            gx, = torch.autograd.grad(op(xg, y), xg)
            return gx
        return run
    hip = lambda a, b: F.ssim(a, b).mean()
    one = torch.ones(1, device=x.device)                      # the data range on the device, made once: no copy inside the timed calls
    composed = lambda a, b: R.ssim(a, b, one).mean()
    pixel = lambda a, b: F.pixel_loss(a, b, 'l2')
    return {'fwd': [fwd(hip), fwd(composed), fwd(pixel)], 'fwd+bwd': [fwdbwd(hip), fwdbwd(composed), fwdbwd(pixel)]}


def block_ms(run, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def case(n, c, h, w):
    x, y = R.smooth_pair(n, c, h, w, seed=1)
    x, y = x.cuda(), y.cuda()
    px = n * c * h * w
    print('\n%d x %d x %d x %d' % (n, c, h, w))
    for mode, runs in variants(x, y).items():
        for run in runs:                                       # warm-up: code objects, allocator
            for _ in range(5):
                run()
        torch.cuda.synchronize()
        per = CALLS // BLOCKS
        t = [[], [], []]
        for _ in range(BLOCKS):                                # alternating blocks
            for k, run in enumerate(runs):
                t[k].append(block_ms(run, per))
        hip, comp, pix = (sorted(v)[BLOCKS // 2] for v in t)
        nbytes = px * (8 if mode == 'fwd' else 20)
        print('  %-8s F.ssim %9.4f ms (min %.4f)   torch ops %9.4f ms (min %.4f)   F.pixel_loss %9.4f ms   '
              'torch / hip %.2f   hip / pixel_loss %.2f   %.1f MB algorithmic -> %.3f TB/s = %.1f %% of HBM peak' % (
                  mode, hip, min(t[0]), comp, min(t[1]), pix, comp / hip, hip / pix, nbytes / 1e6, nbytes / (hip * 1e-3) / 1e12,
                  100 * nbytes / (hip * 1e-3) / HBM_PEAK))
        assert hip < comp, 'F.ssim is not faster than the torch composition'


print('F.ssim vs the torch composition vs F.pixel_loss; HIP events, %d calls per variant in %d alternating blocks, median block' % (
    CALLS, BLOCKS))
case(32, 3, 256, 256)
case(4, 3, 48, 48)
case(1, 3, 3000, 4000)
