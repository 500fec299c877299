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


def load_parent(path):
    global PARENT
    PARENT = C.CDLL(os.path.abspath(path))
    res, args = L.SIGNATURES['risp_serve_u8']
    PARENT.risp_serve_u8.restype, PARENT.risp_serve_u8.argtypes = res, args


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
    emit('  against serve_u8: ' + '  '.join('%s %.3f' % (k[6:] if k.startswith('serve_') else k, med[k] / med['serve'])
                                            for k in names[3:]))
    emit('  serve_bggr / workaround = %.3f' % (med['serve_bggr'] / med['workaround']))
    return res


COMPOSED_ARCH = 'Demosaic_01_sRGB_07_11_01_14'      # as an IspUniversal its bilateral is the proxy CNN: serve() composes


def measure_composed(reps, rounds, emit):
    """net.serve() on the composed route (risp_raw_crop[_cfa] -> fused_forward with a CNN stage -> risp_quantise_u8[_flip]), host
    side included, with and without a phase and a black level"""
    from reconfigisp_amd.codes.models import networks
    opt = {'network_G': {'which_model_G': 'IspUniversal', 'architecture': COMPOSED_ARCH, 'module_path': None,
                         'individual_module_paths': [None] * 8}}
    torch.manual_seed(10)
    net = networks.define_G(opt).cuda().eval()
    raw = frames_u16(8, 256, 256, 30)
    buf = torch.empty((8, 256, 256, 3), device='cuda', dtype=torch.uint8)
    legs = {'rggb_b0': dict(), 'bggr_b64': dict(black_level=64, cfa='bggr')}
    res = {k: [] for k in legs}
    for _ in range(rounds):
        for name, kw in legs.items():
            for k in range(3):
                net.serve(raw, WHITE, out=buf, **kw)
            assert net.last_serve_route == 'composed'
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for k in range(reps):
                net.serve(raw, WHITE, out=buf, **kw)
            e1.record()
            e1.synchronize()
            res[name].append(e0.elapsed_time(e1) / reps * 1e3)
    for name, v in res.items():
        emit('  %-12s rounds %s' % (name, ' '.join('%.1f' % t for t in v)))
        emit('  %-12s median %.1f us  min %.1f  spread %.1f' % (name, sorted(v)[len(v) // 2], min(v), max(v) - min(v)))
    emit('  bggr_b64 / rggb_b0 = %.3f' % (sorted(res['bggr_b64'])[rounds // 2] / sorted(res['rggb_b0'])[rounds // 2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--reps', type=int, default=2000)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--parent-lib', default=None, help='a second build of libreconfigisp_hip.so (the parent commit\'s): its '
                    'risp_serve_u8 is timed in the same rounds')
    args = ap.parse_args()
    if args.parent_lib:
        load_parent(args.parent_lib)
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
    emit('composed route, IspUniversal %s (proxy CNN bilateral), 8 x 256 x 256, net.serve(out=) %d calls per round; us per call'
         % (COMPOSED_ARCH, frame_reps))
    measure_composed(frame_reps, args.rounds, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
