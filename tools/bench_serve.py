#!/usr/bin/env python3
"""GPU box: the serving path against the route it replaces, on resident uint16 frames, in interleaved rounds in one process.

    python tools/bench_serve.py [--out profiles/serve_u8.txt] [--reps 2000] [--rounds 7] [--parent-lib PATH]

Headline pipeline (nearest demosaic, 3 x 3 bilateral, WbManual, Gamma, GtmManual), 64 x 256 x 256 and one 3000 x 4000 frame:
  fp32 launch   risp_bilateral_chain_fwd alone on fp32 mosaics that are already there (every stage output in fp32)
  route         risp_raw_crop -> risp_bilateral_chain_fwd -> risp_quantise_u8: uint16 in, bytes out, three launches
  serve_u8      risp_serve_u8: uint16 in, bytes out, one launch
  serve_<phase> risp_serve_u8_cfa for rggb / grbg / gbrg / bggr at black level 0, serve_b512 the same for rggb at black
                level 512: the phases and the pedestal beside the RGGB entry point they extend
  workaround    what a GRBG.. sensor with a pedestal cost before: torch.flip + subtract-and-clamp on the frame (as int16:
                the samples are below 2^15), risp_serve_u8, torch.flip on the image - bytes compared with serve_bggr's
  serve_parent  with --parent-lib: risp_serve_u8 of a second build of the library (the parent commit's), in the same rounds
Each round times every candidate once (REPS launches between two events, rotating over 4 resident inputs at the batch size);
per candidate: the rounds, median, minimum and spread - the spread between the rounds of ONE candidate is the noise a
difference between two candidates has to clear.  The bytes of route and serve_u8 are compared first.  Last, tensor2bgr on
the host for the frame (what the drivers do today)."""
import ctypes as C
import functools
import time

import torch

import serve_bench as SB
import reconfigisp_amd.functional as F
from reconfigisp_amd import lib as L
from reconfigisp_amd.codes.utils import util

WHITE = 1023.0
OPS = [F.OP_WB_MANUAL, F.OP_GAMMA, F.OP_GTM_MANUAL]


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
        self.out_cfa = torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8)
        self.cfa_args = self.serve_args[:9] + (p(self.out_cfa),) + self.serve_args[10:14]
        self.raw_i16 = raw.view(torch.int16)
        L.call('risp_raw_crop', *self.crop_args)          # the fp32 mosaic the 'fp32 launch' candidate reads

    def fp32_launch(self):
        L.call('risp_bilateral_chain_fwd', *self.plan._args, None)

    def route(self):
        L.call('risp_raw_crop', *self.crop_args)
        L.call('risp_bilateral_chain_fwd', *self.plan._args, None)
        L.call('risp_quantise_u8', *self.quant_args)

    def serve(self):
        L.call('risp_serve_u8', *self.serve_args)

    def serve_parent(self):
        status = PARENT.risp_serve_u8(*self.serve_args)
        assert status == 0, status

    def cfa(self, black, code):
        L.call('risp_serve_u8_cfa', *self.cfa_args, black, code, None)

    def serve_rggb(self):
        self.cfa(0, 0)

    def serve_grbg(self):
        self.cfa(0, 1)

    def serve_gbrg(self):
        self.cfa(0, 2)

    def serve_bggr(self):
        self.cfa(0, 3)

    def serve_b512(self):
        self.cfa(512, 0)

    def workaround(self, black=0):
        """a BGGR frame through the RGGB entry point: mirror both ways, take the pedestal off, serve, mirror back"""
        x = torch.flip(self.raw_i16, (1, 2))
        x = (x - black).clamp_(min=0).view(torch.uint16)
        n, h, w = self.shape
        args = (C.c_void_p(x.data_ptr()),) + self.serve_args[1:]
        L.call('risp_serve_u8', *args)
        self.out_work = torch.flip(self.out_serve, (1, 2))


PARENT = None           # --parent-lib: a second build of the library, bound with the same signatures
CFA_NAMES = ['serve_rggb', 'serve_grbg', 'serve_gbrg', 'serve_bggr', 'serve_b512', 'workaround']


def timed_rotating(fns, reps):
    """serve_bench.timed over the resident inputs in turn: the index stays inside the window, as the recorded rounds had it"""
    for k in range(4):
        fns[k % len(fns)]()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for k in range(reps):
        fns[k % len(fns)]()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def measure(sets, reps, rounds, emit):
    names = ['fp32_launch', 'route', 'serve'] + (['serve_parent'] if PARENT is not None else []) + CFA_NAMES
    for c in sets:                                        # same bytes first
        c.route(), c.serve()
        torch.cuda.synchronize()
        assert torch.equal(c.out_route, c.out_serve), 'serve_u8 and the route disagree'
        c.serve_rggb()
        assert torch.equal(c.out_cfa, c.out_serve), 'serve_u8_cfa (rggb, black 0) and serve_u8 disagree'
        c.serve_bggr(), c.workaround()
        assert torch.equal(c.out_cfa, c.out_work), 'serve_u8_cfa (bggr) and the flip workaround disagree'
        if PARENT is not None:
            c.out_serve.zero_()
            c.serve_parent()
            assert torch.equal(c.out_route, c.out_serve), 'the parent build and the route disagree'
    res = SB.rounds_of({name: [getattr(c, name) for c in sets] for name in names}, reps, rounds, False, timed_rotating)
    n, h, w = sets[0].shape
    pix = n * h * w
    for name, v in res.items():
        for line in SB.leg_lines(name, v, 12, '%.2f'):
            emit(line)
    med = {k: SB.median(v) for k, v in res.items()}
    emit('  serve_u8 moves 5 B/pixel: %s; fp32 launch (64 B/pixel): %.2f TB/s' % (
        SB.hbm_share(5.0 * pix, med['serve']), 64.0 * pix / (med['fp32_launch'] * 1e-6) / 1e12))
    emit('  serve_u8 / fp32 launch = %.3f   serve_u8 / route = %.3f   (%.0f MPix/s)' % (
        med['serve'] / med['fp32_launch'], med['serve'] / med['route'], pix / med['serve']))
    emit('  against serve_u8: ' + '  '.join('%s %.3f' % (k[6:] if k.startswith('serve_') else k, med[k] / med['serve'])
                                            for k in names[3:]))
    emit('  serve_bggr / workaround = %.3f' % (med['serve_bggr'] / med['workaround']))
    return res


COMPOSED_ARCH = 'Demosaic_01_sRGB_07_11_01_14'      # as an IspUniversal its bilateral is the proxy CNN: serve() composes


def measure_composed(reps, rounds, emit):
    """net.serve() on the composed route (risp_raw_crop[_cfa] -> fused_forward with a CNN stage -> risp_quantise_u8[_flip]), host
    side included, with and without a phase and a black level"""
    net = SB.pipeline(COMPOSED_ARCH, 'IspUniversal')
    raw = SB.frames_u16(8, 256, 256, 30, WHITE)
    buf = torch.empty((8, 256, 256, 3), device='cuda', dtype=torch.uint8)
    legs = {'rggb_b0': dict(), 'bggr_b64': dict(black_level=64, cfa='bggr')}
    for kw in legs.values():
        net.serve(raw, WHITE, out=buf, **kw)
        assert net.last_serve_route == 'composed'
    # a partial, not a closure: the window holds the call of net.serve and nothing around it, as the recorded rounds had it
    res = SB.rounds_of({name: functools.partial(net.serve, raw, WHITE, out=buf, **kw) for name, kw in legs.items()}, reps, rounds, False)
    for name, v in res.items():
        for line in SB.leg_lines(name, v, 12):
            emit(line)
    emit('  bggr_b64 / rggb_b0 = %.3f' % (SB.median(res['bggr_b64']) / SB.median(res['rggb_b0'])))


def main():
    global PARENT
    ap = SB.parser(2000, 7)
    ap.add_argument('--parent-lib', default=None, help='a second build of libreconfigisp_hip.so (the parent commit\'s): its '
                    'risp_serve_u8 is timed in the same rounds')
    args = ap.parse_args()
    if args.parent_lib:
        PARENT = SB.load_parent(args.parent_lib, ['risp_serve_u8'])
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    emit('64 x 256 x 256, %d launches per round, rotating over 4 resident inputs; us per call' % args.reps)
    measure([Candidates(SB.frames_u16(64, 256, 256, 10 + k, WHITE)) for k in range(4)], args.reps, args.rounds, emit)
    frame_reps = max(20, args.reps // 10)
    emit('1 x 3000 x 4000, %d launches per round; us per call' % frame_reps)
    frame = Candidates(SB.frames_u16(1, 3000, 4000, 20, WHITE))
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
    emit('composed route, IspUniversal %s (proxy CNN bilateral), 8 x 256 x 256, net.serve(out=) %d calls per round; us per call'
         % (COMPOSED_ARCH, frame_reps))
    measure_composed(frame_reps, args.rounds, emit)
    emit.write()


if __name__ == '__main__':
    main()
