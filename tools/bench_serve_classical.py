#!/usr/bin/env python3
"""GPU box: the classical pipelines' one launch against the composed route it replaces, on resident uint16 frames, in
interleaved rounds in one process.

    python tools/bench_serve_classical.py [--out profiles/serve_classical.txt] [--reps 300] [--rounds 7]

Pipelines (OriginUniversal): Demosaic_02_sRGB_11_01_14 (bilinear, WbManual, Gamma, GtmManual) and Demosaic_03_sRGB_11_04_01
(Malvar-He-Cutler, WbManual, Filmic, Gamma); 64 x 256 x 256 and one 3000 x 4000 frame.  Legs, each net.serve(raw, out=buf)
with the host side included (what a caller pays), timed between two device events:
  classical       risp_serve_classical_u8, RGGB, black level 0
  classical_bggr  the same launch for a BGGR sensor with black level 512
  composed        the route serve() took before: risp_raw_crop -> risp_origin_demosaic -> a chain launch per element-wise
                  run -> two launches per tone curve -> risp_quantise_u8 (serve_route answering 'composed')
  serve_u8        risp_serve_u8 on the nearest headline pipeline (Demosaic_01_sRGB_07_11_01_14), as context
Each round times every leg once (REPS calls, after 3 warm ones); per leg: the rounds, median, minimum and spread - the spread
between the rounds of ONE leg is the noise a difference between two legs has to clear.  The bytes of classical and composed
are compared first.  Bytes moved are algorithmic counts from the module list (fp32 planes written and read back by the
composed route; 2 read + 3 written by the one launch), the share of HBM peak is those bytes over the median time."""
import torch

import serve_bench as SB
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
from reconfigisp_amd.codes.models.modules import tools_origin as T

WHITE = 1023.0
ARCHS = ['Demosaic_02_sRGB_11_01_14', 'Demosaic_03_sRGB_11_04_01']
HEADLINE = 'Demosaic_01_sRGB_07_11_01_14'


def composed_bytes_per_pixel(modules):
    """what the composed route moves per pixel: the crop (2 + 4), the demosaic (4 + 12), an element-wise run of k stages in
    one launch (12 + 12 k), a tone curve (12 + 12), the conversion (12 + 3)"""
    total, run = 6 + 16 + 15, 0
    for m in modules[1:]:
        if type(m) is T.Skip:
            continue
        if type(m) in PF._TONE_OP:
            total, run = total + (12 + 12 * run if run else 0) + 24, 0
        else:
            run += 1
    return total + (12 + 12 * run if run else 0)


def measure(arch, head, raw, reps, rounds, emit):
    n, h, w = raw.shape
    pix = n * h * w
    net = SB.pipeline(arch)
    buf = {k: torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8) for k in ('classical', 'classical_bggr', 'composed', 'serve_u8')}
    route = PF.serve_route

    def classical():
        net.serve(raw, WHITE, out=buf['classical'])

    def classical_bggr():
        net.serve(raw, WHITE, out=buf['classical_bggr'], black_level=512, cfa='bggr')

    def composed():
        PF.serve_route = lambda modules: 'composed'
        try:
            net.serve(raw, WHITE, out=buf['composed'])
        finally:
            PF.serve_route = route

    def serve_u8():
        head.serve(raw, WHITE, out=buf['serve_u8'])

    legs = {'classical': classical, 'classical_bggr': classical_bggr, 'composed': composed, 'serve_u8': serve_u8}
    classical(), composed(), serve_u8()
    assert net.last_serve_route == 'composed' and head.last_serve_route == 'fused'
    classical()
    assert net.last_serve_route == 'classical'
    torch.cuda.synchronize()
    assert torch.equal(buf['classical'], buf['composed']), 'the one launch and the composed route disagree'
    res = SB.rounds_of(legs, reps, rounds, False)
    med = {k: SB.median(v) for k, v in res.items()}
    bpp = {'classical': 5, 'classical_bggr': 5, 'composed': composed_bytes_per_pixel(net.all_modules), 'serve_u8': 5}
    emit(' %s, %d x %d x %d, %d calls per round; us per call' % (arch, n, h, w, reps))
    for name, v in res.items():
        rounds_line, stats_line = SB.leg_lines(name, v, 14)
        emit(rounds_line)
        emit(stats_line + '   %d B/pixel: %s' % (bpp[name], SB.hbm_share(bpp[name] * pix, med[name])))
    emit('  classical / composed = %.3f   classical_bggr / classical = %.3f   classical / serve_u8 = %.3f   (%.0f MPix/s)' % (
        med['classical'] / med['composed'], med['classical_bggr'] / med['classical'], med['classical'] / med['serve_u8'],
        pix / med['classical']))
    return med


def main():
    args = SB.parser(300, 7).parse_args()
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    emit('net.serve(raw, out=buf), host side included; serve_u8: %s' % HEADLINE)
    head = SB.pipeline(HEADLINE)
    batch, frame = SB.frames_u16(64, 256, 256, 10, WHITE), SB.frames_u16(1, 3000, 4000, 20, WHITE)
    wins = []
    for arch in ARCHS:
        for raw, reps in ((batch, args.reps), (frame, max(20, args.reps // 3))):
            med = measure(arch, head, raw, reps, args.rounds, emit)
            wins.append(med['classical'] < med['composed'])
    emit('the one launch beats the composed route in %d of %d cases' % (sum(wins), len(wins)))
    emit.write()


if __name__ == '__main__':
    main()
