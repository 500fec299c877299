#!/usr/bin/env python3
"""GPU box: MIPI-packed RAW10 / RAW12 into the serving path - the fused packed load of the one-launch kernels against the unpack
launch followed by the uint16 call, on resident frames, in interleaved rounds in one process.

    python tools/bench_serve_packed.py [--out profiles/serve_packed.txt] [--reps 300] [--rounds 7]

Pipelines (OriginUniversal): the headline Demosaic_01_sRGB_07_11_01_14 (nearest, bilateral, WbManual, Gamma, GtmManual:
risp_serve_u8 / risp_serve_packed) and Demosaic_02_sRGB_11_01_14 (bilinear, WbManual, Gamma, GtmManual: risp_serve_classical_u8
/ risp_serve_classical_packed); 64 x 256 x 256 and one 3000 x 4000 frame; RAW10 and RAW12 (rows of W * bits / 8 bytes, white
level 2^bits - 1) with BGR out, and RAW10 with NV12 out on the 3000 x 4000 frame.  Legs, host side included (what a caller
pays), timed between two device events:
  u16        (a) net.serve(raw_u16, out=buf): the uint16 call as before, one launch
  unpack_u16 (b) raw_unpack(packed, out=raw_u16) followed by (a): two launches, bits / 8 + 2 + 2 bytes per pixel in
  packed     (c) net.serve(packed, out=buf, raw_format=...): one launch, bits / 8 bytes per pixel in - with the fused load
             forced on, whatever pipeline_fusion.serve_load answers: this measurement is what that table is made from
  unpack     the unpack launch alone (bits / 8 + 2 bytes per pixel)
Each round times every leg once (REPS calls, after 3 warm ones); per leg: the rounds, median, minimum and spread - the spread
between the rounds of ONE leg is the noise a difference between two legs has to clear.  The bytes of (a), (b) and (c) are
compared first.  Verdict per case: (c) beats (b) when median(b) - median(c) exceeds the larger of the two spreads; a route keeps
its fused load for a format when that holds on the 3000 x 4000 frame.  (c) / (a) is reported, not judged.  Bytes are
algorithmic counts, the share of HBM peak is those bytes over the median time."""
import torch

import serve_bench as SB
import reconfigisp_amd.functional as F
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF

ARCHS = [('Demosaic_01_sRGB_07_11_01_14', 'fused'), ('Demosaic_02_sRGB_11_01_14', 'classical')]
ALL_FUSED = frozenset((route, fmt) for route in ('fused', 'classical') for fmt in ('raw10', 'raw12'))


def measure(arch, route, shape, seed, fmt, out_format, reps, rounds, emit):
    n, h, w = shape
    bits = F.RAW_FORMAT[fmt]
    white = float((1 << bits) - 1)
    pix = n * h * w
    x = SB.frames_int(n, h, w, seed, white)
    raw, packed = x.to(torch.uint16).cuda(), SB.pack(x, bits).cuda()
    assert torch.equal(F.raw_unpack(packed, bits, w).cpu(), raw.cpu()), 'the unpack launch and the host packer disagree'
    net = SB.pipeline(arch)
    nv12 = out_format == 'nv12'
    oshape = (n, h + h // 2, w) if nv12 else (n, h, w, 3)
    out_a, out_b, out_c = (torch.empty(oshape, device='cuda', dtype=torch.uint8) for _ in range(3))
    u16 = torch.empty((n, h, w), device='cuda', dtype=torch.uint16)
    obpp = 1.5 if nv12 else 3.0
    bpp = {'u16': 2 + obpp, 'unpack_u16': bits / 8 + 2 + 2 + obpp, 'packed': bits / 8 + obpp, 'unpack': bits / 8 + 2}

    def leg_u16():
        net.serve(raw, white, out=out_a, out_format=out_format)

    def leg_unpack_u16():
        F.raw_unpack(packed, bits, w, out=u16)
        net.serve(u16, white, out=out_b, out_format=out_format)

    def leg_packed():
        net.serve(packed, white, out=out_c, out_format=out_format, raw_format=fmt, raw_width=w)

    def leg_unpack():
        F.raw_unpack(packed, bits, w, out=u16)

    legs = {'u16': leg_u16, 'unpack_u16': leg_unpack_u16, 'packed': leg_packed, 'unpack': leg_unpack}
    leg_u16(), leg_unpack_u16(), leg_packed()
    assert net.last_serve_route == route and net.last_serve_load == 'fused'
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b) and torch.equal(out_a, out_c), 'the legs disagree'
    res = SB.rounds_of(legs, reps, rounds, False)
    med = {k: SB.median(v) for k, v in res.items()}
    emit(' %s (%s), %d x %d x %d, %s in, %s out, %d calls per round; us per call' % (arch, route, n, h, w, fmt, out_format, reps))
    for name, v in res.items():
        rounds_line, stats_line = SB.leg_lines(name, v, 10)
        emit(rounds_line)
        emit(stats_line + '   %.2f B/pixel: %s' % (bpp[name], SB.hbm_share(bpp[name] * pix, med[name])))
    gain, noise = SB.margin(res['packed'], res['unpack_u16'])
    won = SB.beats(res['packed'], res['unpack_u16'])
    emit('  (b) - (c) = %.1f us against a spread of %.1f us: the fused load %s   (c) / (b) = %.3f   (c) / (a) = %.3f   (%.0f MPix/s)' % (
        gain, noise, 'BEATS the unpack launch' if won else 'does NOT beat the unpack launch', med['packed'] / med['unpack_u16'],
        med['packed'] / med['u16'], pix / med['packed']))
    return won


def main():
    args = SB.parser(300, 7).parse_args()
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    emit('(a) u16: net.serve(raw_u16, out=)   (b) unpack_u16: raw_unpack(packed, out=) + (a)   (c) packed: net.serve(packed, out=, '
         'raw_format=) with the fused load   unpack: raw_unpack(out=) alone; host side included')
    table = PF._FUSED_LOAD
    PF._FUSED_LOAD = ALL_FUSED          # leg (c) measures the fused load, whatever the table says today
    batch, frame = (64, 256, 256), (1, 3000, 4000)
    verdict = {}
    try:
        for arch, route in ARCHS:
            for fmt in ('raw10', 'raw12'):
                for shape, seed, reps in ((batch, 10, args.reps), (frame, 20, max(20, args.reps // 3))):
                    won = measure(arch, route, shape, seed, fmt, 'bgr8', reps, args.rounds, emit)
                    if shape == frame:
                        verdict[(route, fmt)] = won
            measure(arch, route, frame, 20, 'raw10', 'nv12', max(20, args.reps // 3), args.rounds, emit)
    finally:
        PF._FUSED_LOAD = table
    emit('on the 3000 x 4000 frame, BGR out, the fused load beats unpack + uint16 by more than the spread for: %s' % (
        ', '.join('%s/%s' % k for k, v in sorted(verdict.items()) if v) or 'no route'))
    emit('                                                                      and does not for: %s' % (
        ', '.join('%s/%s' % k for k, v in sorted(verdict.items()) if not v) or 'no route'))
    emit('pipeline_fusion.serve_load answers \'fused\' for: %s' % (', '.join('%s/%s' % k for k in sorted(table)) or 'no route'))
    emit.write()


if __name__ == '__main__':
    main()
