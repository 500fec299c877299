#!/usr/bin/env python3
"""GPU box: the conditional route (serve(fast_cond=True): per head risp_serve_cond_hist + risp_serve_cond_finish, then
risp_serve_classical_u8) against the composed route of the same pipeline - the default call, unchanged code - on resident
uint16 frames, in interleaved rounds in one process.

    python tools/bench_serve_cond.py [--out profiles/serve_cond.txt] [--reps 50] [--rounds 7]

Pipelines (IspUniversal with conditional_modules; the nearest demosaic, the heads, GtmManual):
  one head     Demosaic_01_sRGB_16_14         ConditionalGamma
  two heads    Demosaic_01_sRGB_17_16_14      ConditionalWbManual, ConditionalGamma
  three heads  Demosaic_01_sRGB_17_18_16_14   ConditionalWbManual, ConditionalWbQuadratic, ConditionalGamma
with 4 and 8 histogram bins per channel (first layer 12 / 24 wide, one hidden layer of 8); 64 x 256 x 256 and one 3000 x 4000
frame.  Legs, each net.serve(raw, out=buf) with the host side included (what a caller pays), timed between two device events:
  cond        2 S + 1 launches and S memsets for S heads; the mosaic read S + 1 times, 3 bytes per pixel written
  composed    risp_raw_crop -> chain -> per head risp_histc, risp_cond_fc_fwd, the scale, a chain -> risp_quantise_u8, every
              stage output an fp32 plane
Each round times every leg once (REPS calls, after 3 warm ones); per leg: the rounds, median, minimum and spread - the spread
between the rounds of ONE leg is the noise a difference between two legs has to clear.  A configuration keeps its place in
cond_plan when the composed median exceeds the cond median by more than the larger of the two spreads.  The bytes of the two
legs are compared first.  Bytes moved are algorithmic counts from the module list."""
import torch

import serve_bench as SB
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF

WHITE = 1023.0
ARCHS = [(1, 'Demosaic_01_sRGB_16_14'), (2, 'Demosaic_01_sRGB_17_16_14'), (3, 'Demosaic_01_sRGB_17_18_16_14')]
BINS = [4, 8]


def bytes_per_pixel(modules):
    """(cond, composed) per pixel.  cond: the mosaic once per head and once to serve, 3 bytes out.  composed: the crop (2 + 4),
    an element-wise run of k stages in one launch (read 4 or 12, write 12 k; the nearest demosaic counts as a stage of the first
    run), per head the histogram's read of the three planes (12), the conversion (12 + 3)"""
    _, stages, heads = PF.cond_plan(modules)
    cond = 2 * (sum(heads) + 1) + 3
    total, run, src = 6 + 15, 1, 4
    for is_head in heads:
        if is_head:
            total, run, src = total + src + 12 * run + 12, 0, 12
        run += 1
    return cond, total + src + 12 * run


def measure(arch, bins, raw, reps, rounds, emit):
    n, h, w = raw.shape
    pix = n * h * w
    ch = [3 * bins, 8]
    net = SB.pipeline(arch, 'IspUniversal', conditional_modules={'gamma_in_channels': ch, 'wb_manual_in_channels': ch,
                                                                  'wb_quadratic_in_channels': ch})
    buf = {k: torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8) for k in ('cond', 'composed')}

    def cond():
        net.serve(raw, WHITE, out=buf['cond'], fast_cond=True)

    def composed():
        net.serve(raw, WHITE, out=buf['composed'])

    legs = {'cond': cond, 'composed': composed}
    composed()
    assert net.last_serve_route == 'composed'
    cond()
    assert net.last_serve_route == 'cond'
    torch.cuda.synchronize()
    assert torch.equal(buf['cond'], buf['composed']), 'the conditional route and the composed route disagree'
    res = SB.rounds_of(legs, reps, rounds, False)
    med = {k: SB.median(v) for k, v in res.items()}
    bpp = dict(zip(('cond', 'composed'), bytes_per_pixel(net.all_modules)))
    emit(' %s, %d bins, %d x %d x %d, %d calls per round; us per call' % (arch, bins, n, h, w, reps))
    for name, v in res.items():
        rounds_line, stats_line = SB.leg_lines(name, v, 9)
        emit(rounds_line)
        emit(stats_line + '   %d B/pixel: %.3f TB/s' % (bpp[name], bpp[name] * pix / (med[name] * 1e-6) / 1e12))
    keeps = SB.beats(res['cond'], res['composed'])
    emit('  cond / composed = %.3f   (%.0f MPix/s against %.0f)   %s' % (
        med['cond'] / med['composed'], pix / med['cond'], pix / med['composed'],
        'beats the composed route by more than the larger spread' if keeps else 'does NOT clear the larger spread'))
    return keeps


def main():
    args = SB.parser(50, 7).parse_args()
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    emit('net.serve(raw, out=buf[, fast_cond=True]), host side included')
    batch, frame = SB.frames_u16(64, 256, 256, 10, WHITE), SB.frames_u16(1, 3000, 4000, 20, WHITE)
    wins = {}
    for heads, arch in ARCHS:
        for bins in BINS:
            for raw, reps in ((batch, args.reps), (frame, max(10, args.reps // 2))):
                wins.setdefault(heads, []).append(measure(arch, bins, raw, reps, args.rounds, emit))
    for heads, w in wins.items():
        emit('%d head%s: the conditional route clears the rule in %d of %d cases' % (heads, '' if heads == 1 else 's', sum(w), len(w)))
    emit.write()


if __name__ == '__main__':
    main()
