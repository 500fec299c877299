#!/usr/bin/env python3
"""GPU box: the serving path against the route it replaces, on resident uint16 frames, in interleaved rounds in one process.

    python tools/bench_serve.py [--out profiles/serve_u8.txt] [--reps 2000] [--rounds 7]

Headline pipeline (nearest demosaic, 3 x 3 bilateral, WbManual, Gamma, GtmManual), 64 x 256 x 256 and one 3000 x 4000 frame:
  fp32 launch   risp_bilateral_chain_fwd alone on fp32 mosaics that are already there (every stage output in fp32)
  route         risp_raw_crop -> risp_bilateral_chain_fwd -> risp_quantise_u8: uint16 in, bytes out, three launches
  serve_u8      risp_serve_u8: uint16 in, bytes out, one launch
Each round times every candidate once (REPS launches between two events, rotating over 4 resident inputs at the batch size);
per candidate: the rounds, median, minimum and spread - the spread between the rounds of ONE candidate is the noise a
difference between two candidates has to clear.  The bytes of route and serve_u8 are compared first.  Last, tensor2bgr on
the host for the frame (what the drivers do today)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import reconfigisp_amd.functional as F  # noqa: E402
from reconfigisp_amd import lib as L  # noqa: E402
from reconfigisp_amd.codes.data.synthetic_raw import make_batch  # noqa: E402
from reconfigisp_amd.codes.utils import util  # noqa: E402

HBM_PEAK = 8.0e12
WHITE = 1023.0
OPS = [F.OP_WB_MANUAL, F.OP_GAMMA, F.OP_GTM_MANUAL]


def frames_u16(n, h, w, seed):
    bay = make_batch(n, h, w, seed=seed)[0][:, 0]
    return (bay * WHITE).round().clamp(0, WHITE).to(torch.int32).to(torch.uint16).cuda()


class Candidates:
    """the three candidates on one resident input, every buffer allocated and every argument marshalled beforehand"""

    def __init__(self, raw):
        n, h, w = raw.shape
        self.raw, self.shape = raw, (n, h, w)
        sig = lambda v: torch.sigmoid(torch.tensor(v)).repeat(n, 1).cuda()
        self.params = [sig([-1.38] * 3) * 5, sig([0.]), sig([-1.099, 0., 1.099])]
        self.sc, self.ss = torch.full((n,), 50.5).cuda(), torch.full((n,), 50.5).cuda()
        self.win = torch.full((n,), 3, dtype=torch.int32).cuda()
        self.sel = torch.tensor([[i, 0, 0] for i in range(n)], dtype=torch.int32).cuda()
        self.x = torch.empty((n, 1, h, w), device='cuda')
        self.plan = F.BilateralChainPlan(self.x, True, self.win, self.sc, self.ss, 3, OPS, self.params)
        self.out_route = torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8)
        self.out_serve = torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8)
        p = lambda t: C.c_void_p(t.data_ptr())
        self.crop_args = (p(raw), p(self.x), p(self.sel), n, h, w, h, w, WHITE, None)
        self.quant_args = (p(self.plan.outs[-1]), p(self.out_route), n, 3, h, w, 0, None)
        self.serve_args = (p(raw), WHITE, p(self.win), p(self.sc), p(self.ss), 3, len(OPS), (C.c_int * len(OPS))(*OPS),
                           L.ptr_array([t.data_ptr() for t in self.params]), p(self.out_serve), 0, n, h, w, None)
        L.call('risp_raw_crop', *self.crop_args)          # the fp32 mosaic the 'fp32 launch' candidate reads

    def fp32_launch(self):
        L.call('risp_bilateral_chain_fwd', *self.plan._args, None)

    def route(self):
        L.call('risp_raw_crop', *self.crop_args)
        L.call('risp_bilateral_chain_fwd', *self.plan._args, None)
        L.call('risp_quantise_u8', *self.quant_args)

    def serve(self):
        L.call('risp_serve_u8', *self.serve_args)


def measure(sets, reps, rounds, emit):
    names = ['fp32_launch', 'route', 'serve']
    for c in sets:                                        # same bytes first
        c.route(), c.serve()
        torch.cuda.synchronize()
        assert torch.equal(c.out_route, c.out_serve), 'serve_u8 and the route disagree'
    res = {k: [] for k in names}
    for _ in range(rounds):
        for name in names:
            fns = [getattr(c, name) for c in sets]
            for k in range(4):
                fns[k % len(fns)]()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for k in range(reps):
                fns[k % len(fns)]()
            e1.record()
            e1.synchronize()
            res[name].append(e0.elapsed_time(e1) / reps * 1e3)
    n, h, w = sets[0].shape
    pix = n * h * w
    for name in names:
        v = res[name]
        med = sorted(v)[len(v) // 2]
        emit('  %-12s rounds %s' % (name, ' '.join('%.2f' % t for t in v)))
        emit('  %-12s median %.2f us  min %.2f  spread %.2f' % (name, med, min(v), max(v) - min(v)))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    bps = 5.0 * pix / (med['serve'] * 1e-6)
    emit('  serve_u8 moves 5 B/pixel: %.3f TB/s = %.1f %% of the %.1f TB/s HBM peak; fp32 launch (64 B/pixel): %.2f TB/s' % (
        bps / 1e12, 100 * bps / HBM_PEAK, HBM_PEAK / 1e12, 64.0 * pix / (med['fp32_launch'] * 1e-6) / 1e12))
    emit('  serve_u8 / fp32 launch = %.3f   serve_u8 / route = %.3f   (%.0f MPix/s)' % (
        med['serve'] / med['fp32_launch'], med['serve'] / med['route'], pix / med['serve']))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--reps', type=int, default=2000)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit('tools/bench_serve.py --reps %d --rounds %d   (%s)' % (args.reps, args.rounds, torch.cuda.get_device_name(0)))
    emit('64 x 256 x 256, %d launches per round, rotating over 4 resident inputs; us per call' % args.reps)
    measure([Candidates(frames_u16(64, 256, 256, 10 + k)) for k in range(4)], args.reps, args.rounds, emit)
    frame_reps = max(20, args.reps // 10)
    emit('1 x 3000 x 4000, %d launches per round; us per call' % frame_reps)
    frame = Candidates(frames_u16(1, 3000, 4000, 20))
    measure([frame], frame_reps, args.rounds, emit)
    last = frame.plan.outs[-1]
    torch.cuda.synchronize()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        host = util.tensor2bgr(last)
        t.append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(torch.from_numpy(host), frame.out_route[0].cpu())
    emit('  tensor2bgr on the host (device fp32 -> numpy bytes), 3 calls: %s ms' % ' '.join('%.1f' % v for v in t))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
