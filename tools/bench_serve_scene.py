#!/usr/bin/env python3
"""GPU box: the scene route (serve(fast_scene=True): statistics, finish and serving launches per scene stage) against the
composed route of the same pipeline, on resident uint16 frames, in interleaved rounds in one process.

    python tools/bench_serve_scene.py [--out profiles/serve_scene.txt] [--reps 300] [--rounds 7]

Pipelines (OriginUniversal): Demosaic_02_sRGB_05_01 (bilinear, gray-world, Gamma) and Demosaic_03_sRGB_06_02
(Malvar-He-Cutler, white-world, Reinhard); 64 x 256 x 256 and one 3000 x 4000 frame.  Legs, each net.serve(raw, out=buf) with
the host side included (what a caller pays), timed between two device events:
  scene      fast_scene=True: 2 S + 1 launches for S scene stages, the mosaic read S + 1 times, no fp32 plane
  composed   the default call: risp_raw_crop -> risp_origin_demosaic -> chain / statistics / prepare / apply launches ->
             risp_quantise_u8
Each round times every leg once (REPS calls, after 3 warm ones); per leg: the rounds, median, minimum and spread - the spread
between the rounds of ONE leg is the noise a difference between two legs has to clear.  The bytes of the two legs are compared
first and the number that differ is printed (gray-world and Reinhard sum in another order: rounding ties may differ by one)."""
import torch

import serve_bench as SB
from bench_serve_classical import WHITE

ARCHS = [('Demosaic_02_sRGB_05_01', 1), ('Demosaic_03_sRGB_06_02', 2)]


def measure(arch, scenes, raw, reps, rounds, emit):
    n, h, w = raw.shape
    net = SB.pipeline(arch)
    buf = {k: torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8) for k in ('scene', 'composed')}
    legs = {'scene': lambda: net.serve(raw, WHITE, out=buf['scene'], fast_scene=True),
            'composed': lambda: net.serve(raw, WHITE, out=buf['composed'])}
    legs['composed']()
    assert net.last_serve_route == 'composed'
    legs['scene']()
    assert net.last_serve_route == 'scene'
    torch.cuda.synchronize()
    d = (buf['scene'].int() - buf['composed'].int()).abs()
    assert d.max().item() <= 1, 'the scene route and the composed route differ by more than a rounding tie'
    res = SB.rounds_of(legs, reps, rounds, False)
    med = {k: SB.median(v) for k, v in res.items()}
    emit(' %s (%d scene stage%s), %d x %d x %d, %d calls per round; us per call; %d of %d bytes differ by one' % (
        arch, scenes, 's' * (scenes > 1), n, h, w, reps, int((d != 0).sum().item()), d.numel()))
    for name, v in res.items():
        for line in SB.leg_lines(name, v, 9):
            emit(line)
    emit('  scene / composed = %.3f   (%.0f MPix/s)' % (med['scene'] / med['composed'], n * h * w / med['scene']))
    return med


def main():
    args = SB.parser(300, 7).parse_args()
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    emit('net.serve(raw, out=buf), host side included')
    batch, frame = SB.frames_u16(64, 256, 256, 10, WHITE), SB.frames_u16(1, 3000, 4000, 20, WHITE)
    wins = []
    for arch, scenes in ARCHS:
        for raw, reps in ((batch, args.reps), (frame, max(20, args.reps // 3))):
            med = measure(arch, scenes, raw, reps, args.rounds, emit)
            wins.append(med['scene'] < med['composed'])
    emit('the scene route beats the composed route in %d of %d cases' % (sum(wins), len(wins)))
    emit.write()


if __name__ == '__main__':
    main()
