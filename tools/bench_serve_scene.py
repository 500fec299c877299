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
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch  # noqa: E402

from bench_serve_classical import WHITE, frames_u16, pipeline, timed  # noqa: E402

ARCHS = [('Demosaic_02_sRGB_05_01', 1), ('Demosaic_03_sRGB_06_02', 2)]


def measure(arch, scenes, raw, reps, rounds, emit):
    n, h, w = raw.shape
    net = pipeline(arch)
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
    res = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            res[name].append(timed(fn, reps))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    emit(' %s (%d scene stage%s), %d x %d x %d, %d calls per round; us per call; %d of %d bytes differ by one' % (
        arch, scenes, 's' * (scenes > 1), n, h, w, reps, int((d != 0).sum().item()), d.numel()))
    for name, v in res.items():
        emit('  %-9s rounds %s' % (name, ' '.join('%.1f' % t for t in v)))
        emit('  %-9s median %.1f us  min %.1f  spread %.1f' % (name, med[name], min(v), max(v) - min(v)))
    emit('  scene / composed = %.3f   (%.0f MPix/s)' % (med['scene'] / med['composed'], n * h * w / med['scene']))
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--reps', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit('tools/bench_serve_scene.py --reps %d --rounds %d   (%s)' % (args.reps, args.rounds, torch.cuda.get_device_name(0)))
    emit('net.serve(raw, out=buf), host side included')
    batch, frame = frames_u16(64, 256, 256, 10), frames_u16(1, 3000, 4000, 20)
    wins = []
    for arch, scenes in ARCHS:
        for raw, reps in ((batch, args.reps), (frame, max(20, args.reps // 3))):
            med = measure(arch, scenes, raw, reps, args.rounds, emit)
            wins.append(med['scene'] < med['composed'])
    emit('the scene route beats the composed route in %d of %d cases' % (sum(wins), len(wins)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
