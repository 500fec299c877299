#!/usr/bin/env python3
"""GPU box: YUV 4:2:0 (NV12) out of the serving path - the fused NV12 store of the one-launch kernels against the BGR launch
followed by the conversion launch, on resident uint16 frames, in interleaved rounds in one process.

    python tools/bench_serve_nv12.py [--out profiles/serve_nv12.txt] [--reps 300] [--rounds 7]

Pipelines (OriginUniversal): the headline Demosaic_01_sRGB_07_11_01_14 (nearest, bilateral, WbManual, Gamma, GtmManual:
risp_serve_u8 / risp_serve_nv12) and Demosaic_02_sRGB_11_01_14 (bilinear, WbManual, Gamma, GtmManual: risp_serve_classical_u8
/ risp_serve_classical_nv12); 64 x 256 x 256 and one 3000 x 4000 frame.  Legs, host side included (what a caller pays),
timed between two device events:
  bgr        (a) net.serve(raw, out=buf): packed BGR as before, one launch
  bgr_pass   (b) (a) followed by bgr8_to_nv12(buf, out=yuv): two launches, 2 + 3 + 3 + 1.5 bytes per pixel
  nv12       (c) net.serve(raw, out=yuv, out_format='nv12'): one launch, 2 + 1.5 bytes per pixel
  pass       the conversion launch alone on the resident BGR image (3 + 1.5 bytes per pixel)
  bgr_bggr, nv12_bggr   (a) and (c) for a BGGR sensor with black level 512 (the mirrored-address instantiations), as context
Each round times every leg once (REPS calls, after 3 warm ones); per leg: the rounds, median, minimum and spread - the spread
between the rounds of ONE leg is the noise a difference between two legs has to clear.  The bytes of (b) and (c) are compared
first.  Verdict per case: (c) beats (b) when median(b) - median(c) exceeds the larger of the two spreads; (c) / (a) is
reported.  Bytes are algorithmic counts, the share of HBM peak is those bytes over the median time."""
import torch

import serve_bench as SB
import reconfigisp_amd.functional as F

WHITE = 1023.0
ARCHS = [('Demosaic_01_sRGB_07_11_01_14', 'fused'), ('Demosaic_02_sRGB_11_01_14', 'classical')]
BPP = {'bgr': 5.0, 'bgr_pass': 9.5, 'nv12': 3.5, 'pass': 4.5, 'bgr_bggr': 5.0, 'nv12_bggr': 3.5}


def measure(arch, route, raw, reps, rounds, emit):
    n, h, w = raw.shape
    pix = n * h * w
    net = SB.pipeline(arch)
    bgr = torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8)
    yuv_b, yuv_c = (torch.empty((n, h + h // 2, w), device='cuda', dtype=torch.uint8) for _ in range(2))

    def leg_bgr():
        net.serve(raw, WHITE, out=bgr)

    def leg_bgr_pass():
        net.serve(raw, WHITE, out=bgr)
        F.bgr8_to_nv12(bgr, out=yuv_b)

    def leg_nv12():
        net.serve(raw, WHITE, out=yuv_c, out_format='nv12')

    def leg_pass():
        F.bgr8_to_nv12(bgr, out=yuv_b)

    def leg_bgr_bggr():
        net.serve(raw, WHITE, out=bgr, black_level=512, cfa='bggr')

    def leg_nv12_bggr():
        net.serve(raw, WHITE, out=yuv_c, out_format='nv12', black_level=512, cfa='bggr')

    legs = {'bgr': leg_bgr, 'bgr_pass': leg_bgr_pass, 'nv12': leg_nv12, 'pass': leg_pass, 'bgr_bggr': leg_bgr_bggr,
            'nv12_bggr': leg_nv12_bggr}
    leg_bgr_pass(), leg_nv12()
    assert net.last_serve_route == route and net.last_serve_store == 'fused'
    torch.cuda.synchronize()
    assert torch.equal(yuv_b, yuv_c), 'the fused NV12 store and the conversion launch disagree'
    res = SB.rounds_of(legs, reps, rounds, False)
    med = {k: SB.median(v) for k, v in res.items()}
    emit(' %s (%s), %d x %d x %d, %d calls per round; us per call' % (arch, route, n, h, w, reps))
    for name, v in res.items():
        rounds_line, stats_line = SB.leg_lines(name, v, 9)
        emit(rounds_line)
        emit(stats_line + '   %.1f B/pixel: %s' % (BPP[name], SB.hbm_share(BPP[name] * pix, med[name])))
    gain, noise = SB.margin(res['nv12'], res['bgr_pass'])
    won = SB.beats(res['nv12'], res['bgr_pass'])
    emit('  (b) - (c) = %.1f us against a spread of %.1f us: the fused store %s   (c) / (b) = %.3f   (c) / (a) = %.3f   '
         'nv12_bggr / bgr_bggr = %.3f   (%.0f MPix/s)' % (
             gain, noise, 'BEATS the conversion launch' if won else 'does NOT beat the conversion launch', med['nv12'] / med['bgr_pass'],
             med['nv12'] / med['bgr'], med['nv12_bggr'] / med['bgr_bggr'], pix / med['nv12']))
    return won


def main():
    args = SB.parser(300, 7).parse_args()
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    emit('(a) bgr: net.serve(raw, out=)   (b) bgr_pass: (a) + bgr8_to_nv12(out=)   (c) nv12: net.serve(raw, out=, out_format=nv12)   '
         'pass: bgr8_to_nv12(out=) alone; matrix bt601_full, host side included')
    batch, frame = SB.frames_u16(64, 256, 256, 10, WHITE), SB.frames_u16(1, 3000, 4000, 20, WHITE)
    wins = []
    for arch, route in ARCHS:
        for raw, reps in ((batch, args.reps), (frame, max(20, args.reps // 3))):
            wins.append(measure(arch, route, raw, reps, args.rounds, emit))
    emit('the fused NV12 store beats BGR + conversion by more than the spread in %d of %d cases' % (sum(wins), len(wins)))
    emit.write()


if __name__ == '__main__':
    main()
