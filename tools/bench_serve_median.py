#!/usr/bin/env python3
"""GPU box: a median pipeline's one launch at every learned size (serve(fast_median=True), risp_serve_median_u8) against the
default call of the same pipeline - the composed route, unchanged code - on resident uint16 frames, in interleaved rounds in
one process.  pipeline_fusion._MEDIAN_SIZES is filled from the file this writes.

    python tools/bench_serve_median.py [--out profiles/serve_median.txt] [--reps 100] [--rounds 7]

Pipelines (OriginUniversal): Demosaic_0D_sRGB_11_08_01 - a bilinear (D = 2) or Malvar-He-Cutler (D = 3) demosaic, WbManual,
the median with its parameter set for K = 5, 7, .. 15, Gamma: one stage on each side; 64 x 256 x 256 and one 3000 x 4000 frame.
Legs, each net.serve(raw, out=buf) with the host side included (what a caller pays), timed between two device events:
  route       risp_serve_median_u8, one launch (every size is sent to it here, whatever _MEDIAN_SIZES holds)
  default     risp_raw_crop -> risp_origin_demosaic -> chain -> risp_origin_median -> chain -> risp_quantise_u8, every stage
              output an fp32 plane
  median      risp_origin_median alone on an fp32 image of the same shape: route minus this is what is left of everything
              else in the fused launch; a negative difference says the fused median phase runs slower than the stand-alone one
Each round times every leg once (REPS calls, after 3 warm ones); per leg: the rounds, median, minimum and spread - the spread
between the rounds of ONE leg is the noise a difference between two legs has to clear.  The bytes of route and default are
compared first.  The rule for _MEDIAN_SIZES: a size is listed only where the route beats the default call by more than the
larger spread of the two legs in all four rows of that size (both demosaics, both frame sizes)."""
import torch

import serve_bench as SB
import reconfigisp_amd.functional as F
from reconfigisp_amd import lib as L
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF

WHITE = 1023.0
DEMOSAICS = [('bilinear', 2), ('laplacian', 3)]
SIZES = [5, 7, 9, 11, 13, 15]


def measure(dem, kind, k, raw, planes, reps, rounds, emit):
    n, h, w = raw.shape
    arch = 'Demosaic_%02d_sRGB_11_08_01' % kind
    p = ((k - 3) // 2 + 0.5) / 7                           # the middle of the parameter range that gives size k
    net = SB.pipeline(arch, median=float(torch.logit(torch.tensor(p))))
    buf = {name: torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8) for name in ('route', 'default')}
    x, y = planes

    def route():
        net.serve(raw, WHITE, out=buf['route'], fast_median=True)

    def default():
        net.serve(raw, WHITE, out=buf['default'])

    def median():
        L.call('risp_origin_median', F._p(x), F._p(y), k, n, h, w, 255.0, 255.0, F._stream())

    legs = {'route': route, 'default': default, 'median': median}
    default()
    assert net.last_serve_route == 'composed'
    L.CALLS = {}
    route()
    calls, L.CALLS = L.CALLS, None
    assert net.last_serve_route == 'denoise' and calls == {'risp_serve_median_u8': 1}, calls
    torch.cuda.synchronize()
    assert torch.equal(buf['route'], buf['default']), 'the one launch and the default call disagree'
    res = SB.rounds_of(legs, reps, rounds, False)
    med = {name: SB.median(v) for name, v in res.items()}
    spread = {name: SB.spread(v) for name, v in res.items()}
    emit(' %s, median %d x %d, %d x %d x %d, %d calls per round; us per call' % (arch, k, k, n, h, w, reps))
    for name, v in res.items():
        emit(SB.leg_lines(name, v, 8)[0])
    won = SB.beats(res['route'], res['default'])
    emit('  K=%-2d %-9s %dx%dx%d  route %.1f +- %.1f us  default %.1f +- %.1f us  median alone %.1f +- %.1f us  '
         'route / default = %.3f  route - median alone = %.1f us  %s' % (
             k, dem, n, h, w, med['route'], spread['route'], med['default'], spread['default'], med['median'], spread['median'],
             med['route'] / med['default'], med['route'] - med['median'], 'wins' if won else 'does not win'))
    return won


def main():
    args = SB.parser(100, 7).parse_args()
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    emit('net.serve(raw, out=buf[, fast_median=True]), host side included; (+- is the spread between the rounds of a leg)')
    PF._MEDIAN_SIZES = frozenset(SIZES)                    # the measurement decides the table: every size takes the launch here
    sets = []
    for shape, seed, reps in (((64, 256, 256), 10, args.reps), ((1, 3000, 4000), 20, max(5, args.reps // 3))):
        raw = SB.frames_u16(*shape, seed, WHITE)
        x = torch.rand((shape[0], 3) + shape[1:], device='cuda')
        sets.append((raw, (x, torch.empty_like(x)), reps))
    wins = {k: [] for k in SIZES}
    for k in SIZES:
        for dem, kind in DEMOSAICS:
            for raw, planes, reps in sets:
                wins[k].append(measure(dem, kind, k, raw, planes, reps, args.rounds, emit))
    won = [k for k in SIZES if all(wins[k])]
    lost = [k for k in SIZES if not all(wins[k])]
    emit('fast_median=True beats the default call by more than the spread at both sizes for: %s' % (', '.join(map(str, won)) or '-'))
    emit('and does not for: %s' % (', '.join(map(str, lost)) or '-'))
    emit.write()


if __name__ == '__main__':
    main()
