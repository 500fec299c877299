#!/usr/bin/env python3
"""GPU box: temporal noise reduction in the serving path - what the launch and its state copy cost beside the streaming pre-pass
it follows, what the feature costs a served call, and the same filter composed from torch ops; on resident frames, in interleaved
rounds in one process.

    python tools/bench_serve_temporal.py [--out profiles/serve_temporal.txt] [--reps 300] [--rounds 7] [--nocopy-lib PATH]

Pipeline (OriginUniversal, route 'classical'): Demosaic_02_sRGB_11_01_14 (bilinear, WbManual, Gamma, GtmManual); 64 x 256 x 256 and
one 3000 x 4000 frame of 10-bit samples, black level 64, white level 1023; (strength, threshold, slope, ramp) = (64, 40, 10, 24);
the state holds another frame of the same statistics when the timing starts and follows the recursion from there.  A shading of
cell 64 with gains 1 .. 2 rising to the corners for the yardstick.  Legs, host side included (what a caller pays), timed between
two device events:
  (a) temporal    functional.raw_temporal(raw, td, out=) alone: the launch (6 bytes per pixel) and the copy of the state (4)
      launch      risp_raw_temporal of a build without the copy (make EXTRA=-DRISP_TEMPORAL_NO_COPY OUT=... OBJDIR=..., given as
                  --nocopy-lib): the launch alone; 'not measured' without the option
      shade       functional.raw_shade(raw, out=) alone, the streaming yardstick: 4 bytes per pixel
  (b) serve_tnr   net.serve(raw, out=, temporal_denoise=): what a user pays with the feature
      serve       the same call without the keyword
  (c) torch       the same filter composed from torch ops on int32 tensors (reflected index_select, 10 shifted adds per sum), state
                  update included; its output is compared with the launch's first
Each round times every leg once (REPS calls, after 3 warm ones), after one round that is not kept; per leg: the rounds, median,
minimum and spread - the spread between the rounds of ONE leg is the noise a difference between two legs has to clear.  Bytes are
algorithmic counts, the rate is those bytes over the median time."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import reconfigisp_amd.functional as F  # noqa: E402
from reconfigisp_amd import lib as L  # noqa: E402
from bench_serve_packed import frames_int, pipeline, timed  # noqa: E402
from bench_serve_shade import vignette  # noqa: E402

HBM_PEAK = 8.0e12
ARCH = 'Demosaic_02_sRGB_11_01_14'
WHITE, BLACK, CELL = 1023.0, 64, 64
PARAMS = (64, 40, 10, 24)


def reflect_index(n, device):
    i = torch.arange(-2, n + 2, device=device)
    return torch.where(i < 0, -i, torch.where(i >= n, 2 * (n - 1) - i, i))


def torch_temporal(cur, state, iy, ix, params, black):
    """the definition of include/risp.h from torch ops: (N,H,W) uint16 -> (N,H,W) uint16"""
    strength, threshold, slope, ramp = params
    h, w = cur.shape[-2:]
    c, p = cur.to(torch.int32), state.to(torch.int32)

    def box(v):
        v = v.index_select(-2, iy).index_select(-1, ix)
        v = v[..., :, 0:w] + v[..., :, 1:w + 1] + v[..., :, 2:w + 2] + v[..., :, 3:w + 3] + v[..., :, 4:w + 4]
        return v[..., 0:h, :] + v[..., 1:h + 1, :] + v[..., 2:h + 2, :] + v[..., 3:h + 3, :] + v[..., 4:h + 4, :]

    a, b = box(c - p), box(p)
    lo = 25 * threshold + (((b - 25 * black).clamp_(min=0) * slope) >> 8)
    e = (a.abs_() - lo).clamp_(0, 65535)
    k = (strength + ((e.to(torch.int64) * ramp) >> 8)).clamp_(max=256).to(torch.int32)
    return ((p * (256 - k) + c * k + 128) >> 8).to(torch.uint16)


def measure(net, shape, seed, reps, rounds, nocopy, emit):
    n, h, w = shape
    pix = n * h * w
    raw = (frames_int(n, h, w, seed, int(WHITE) - BLACK) + BLACK).to(torch.uint16).cuda()
    start = (frames_int(n, h, w, seed + 1, int(WHITE) - BLACK) + BLACK).to(torch.uint16).cuda()
    shading = (F.shading_map(vignette(h, w), h, w, CELL).cuda(), CELL)
    states = {k: F.temporal_state(n, h, w) for k in ('temporal', 'launch', 'serve', 'torch')}
    for st in states.values():
        st.frames.copy_(start)
        st.primed = True
    u16, u16_l, u16_s = (torch.empty((n, h, w), device='cuda', dtype=torch.uint16) for _ in range(3))
    out_t, out_s = (torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8) for _ in range(2))
    iy, ix = reflect_index(h, raw.device), reflect_index(w, raw.device)
    bpp = {'temporal': 10.0, 'launch': 6.0, 'shade': 4.0, 'serve_tnr': 15.0, 'serve': 5.0, 'torch': 10.0}

    def leg_temporal():
        F.raw_temporal(raw, (states['temporal'],) + PARAMS, BLACK, out=u16)

    def leg_launch():
        status = nocopy.risp_raw_temporal(F._p(raw), F._p(states['launch'].frames), F._p(u16_l), 0, *PARAMS, BLACK, n, h, w, F._stream())
        assert status == 0

    def leg_shade():
        F.raw_shade(raw, shading, BLACK, 16, w, out=u16_s)

    def leg_serve_tnr():
        net.serve(raw, WHITE, out=out_t, black_level=BLACK, temporal_denoise=(states['serve'],) + PARAMS)

    def leg_serve():
        net.serve(raw, WHITE, out=out_s, black_level=BLACK)

    def leg_torch():
        st = states['torch']
        st.frames.copy_(torch_temporal(raw, st.frames, iy, ix, PARAMS, BLACK))

    # the first step of every form gives the same frames
    leg_temporal(), leg_torch(), leg_serve_tnr(), leg_serve()
    assert net.last_serve_route == 'classical'
    torch.cuda.synchronize()
    assert torch.equal(states['temporal'].frames, states['torch'].frames), 'the torch composition and the launch disagree'
    assert torch.equal(states['temporal'].frames, states['serve'].frames) and torch.equal(u16, states['temporal'].frames)
    moved = (u16.to(torch.int32) != raw.to(torch.int32)).float().mean().item()
    legs = {'temporal': leg_temporal, 'shade': leg_shade, 'serve_tnr': leg_serve_tnr, 'serve': leg_serve, 'torch': leg_torch}
    if nocopy is not None:
        leg_launch()
        torch.cuda.synchronize()
        assert torch.equal(u16_l, u16) and torch.equal(states['launch'].frames, start), 'the build without the copy copied'
        legs['launch'] = leg_launch
    res = {k: [] for k in legs}
    for r in range(rounds + 1):                             # round 0 brings the clocks up and is not kept
        for name, fn in legs.items():
            t = timed(fn, reps if name != 'torch' else max(5, reps // 10))
            if r:
                res[name].append(t)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    emit(' %s, %d x %d x %d, %d calls per round (torch: a tenth); us per call; the first filtered frame differs from its input in '
         '%.1f %% of the samples' % (ARCH, n, h, w, reps, 100 * moved))
    for name, v in res.items():
        emit('  %-10s rounds %s' % (name, ' '.join('%.1f' % t for t in v)))
        rate = bpp[name] * pix / (med[name] * 1e-6)
        emit('  %-10s median %.1f us  min %.1f  spread %.1f   %.0f B/pixel: %.3f TB/s = %.1f %% of the %.1f TB/s HBM peak' % (
            name, med[name], min(v), spread[name], bpp[name], rate / 1e12, 100 * rate / HBM_PEAK, HBM_PEAK / 1e12))
    if 'launch' in med:
        emit('  (a) temporal / shade = %.2f   launch / shade = %.2f   the copy costs temporal - launch = %.1f us' % (
            med['temporal'] / med['shade'], med['launch'] / med['shade'], med['temporal'] - med['launch']))
    else:
        emit('  (a) temporal / shade = %.2f   launch: not measured (no --nocopy-lib)' % (med['temporal'] / med['shade']))
    emit('  (b) serve_tnr - serve = %.1f us: serve_tnr / serve = %.3f   (%.0f MPix/s with the filter)' % (
        med['serve_tnr'] - med['serve'], med['serve_tnr'] / med['serve'], pix / med['serve_tnr']))
    emit('  (c) torch / temporal = %.1f' % (med['torch'] / med['temporal']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--reps', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--nocopy-lib', default=None, help='a build of the library with -DRISP_TEMPORAL_NO_COPY: times the launch alone')
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    nocopy = None
    if args.nocopy_lib:
        nocopy = C.CDLL(os.path.abspath(args.nocopy_lib))
        nocopy.risp_raw_temporal.restype, nocopy.risp_raw_temporal.argtypes = L.SIGNATURES['risp_raw_temporal']
    emit('tools/bench_serve_temporal.py --reps %d --rounds %d%s   (%s)' % (
        args.reps, args.rounds, ' --nocopy-lib' if nocopy is not None else '', torch.cuda.get_device_name(0)))
    emit('(a) temporal / launch / shade: risp_raw_temporal with and without its state copy beside risp_raw_shade   (b) serve_tnr / '
         'serve: net.serve(raw, out=) with and without temporal_denoise   (c) torch: the filter from torch ops; host side included')
    net = pipeline(ARCH)
    for shape, seed, reps in (((64, 256, 256), 10, args.reps), ((1, 3000, 4000), 20, max(20, args.reps // 3))):
        measure(net, shape, seed, reps, args.rounds, nocopy, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
