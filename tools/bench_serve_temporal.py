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
import torch

import serve_bench as SB
import reconfigisp_amd.functional as F

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
    raw = (SB.frames_int(n, h, w, seed, int(WHITE) - BLACK) + BLACK).to(torch.uint16).cuda()
    start = (SB.frames_int(n, h, w, seed + 1, int(WHITE) - BLACK) + BLACK).to(torch.uint16).cuda()
    shading = (F.shading_map(SB.vignette(h, w), h, w, CELL).cuda(), CELL)
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
    res = SB.rounds_of(legs, {name: max(5, reps // 10) if name == 'torch' else reps for name in legs}, rounds, True)
    med = {k: SB.median(v) for k, v in res.items()}
    emit(' %s, %d x %d x %d, %d calls per round (torch: a tenth); us per call; the first filtered frame differs from its input in '
         '%.1f %% of the samples' % (ARCH, n, h, w, reps, 100 * moved))
    for name, v in res.items():
        rounds_line, stats_line = SB.leg_lines(name, v, 10)
        emit(rounds_line)
        emit(stats_line + '   %.0f B/pixel: %s' % (bpp[name], SB.hbm_share(bpp[name] * pix, med[name])))
    if 'launch' in med:
        emit('  (a) temporal / shade = %.2f   launch / shade = %.2f   the copy costs temporal - launch = %.1f us' % (
            med['temporal'] / med['shade'], med['launch'] / med['shade'], med['temporal'] - med['launch']))
    else:
        emit('  (a) temporal / shade = %.2f   launch: not measured (no --nocopy-lib)' % (med['temporal'] / med['shade']))
    emit('  (b) serve_tnr - serve = %.1f us: serve_tnr / serve = %.3f   (%.0f MPix/s with the filter)' % (
        med['serve_tnr'] - med['serve'], med['serve_tnr'] / med['serve'], pix / med['serve_tnr']))
    emit('  (c) torch / temporal = %.1f' % (med['torch'] / med['temporal']))


def main():
    ap = SB.parser(300, 7)
    ap.add_argument('--nocopy-lib', default=None, help='a build of the library with -DRISP_TEMPORAL_NO_COPY: times the launch alone')
    args = ap.parse_args()
    emit = SB.Report(args.out)
    nocopy = SB.load_parent(args.nocopy_lib, ['risp_raw_temporal']) if args.nocopy_lib else None
    emit(SB.header(__file__, args, ' --nocopy-lib' if nocopy is not None else ''))
    emit('(a) temporal / launch / shade: risp_raw_temporal with and without its state copy beside risp_raw_shade   (b) serve_tnr / '
         'serve: net.serve(raw, out=) with and without temporal_denoise   (c) torch: the filter from torch ops; host side included')
    net = SB.pipeline(ARCH)
    for shape, seed, reps in (((64, 256, 256), 10, args.reps), ((1, 3000, 4000), 20, max(20, args.reps // 3))):
        measure(net, shape, seed, reps, args.rounds, nocopy, emit)
    emit.write()


if __name__ == '__main__':
    main()
