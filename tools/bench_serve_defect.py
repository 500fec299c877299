#!/usr/bin/env python3
"""GPU box: defective-pixel correction in the serving path - what the launch costs beside the two streaming pre-passes it joins,
one launch against two in front of a lens shading, and what the feature costs a served call; on resident frames, in interleaved
rounds in one process.

    python tools/bench_serve_defect.py [--out profiles/serve_defect.txt] [--reps 300] [--rounds 7]

Pipeline (OriginUniversal, route 'classical'): Demosaic_02_sRGB_11_01_14 (bilinear, WbManual, Gamma, GtmManual); 64 x 256 x 256 and
one 3000 x 4000 frame; formats u16 / raw10 / raw12 holding the same 10-bit samples, black level 64, white level 1023; threshold 32,
slope 16, a map with 0.05 % of the pixels listed; a shading of cell 64 with gains 1 .. 2 rising to the corners.  Legs, host side
included (what a caller pays), timed between two device events:
  (a) defect      functional.raw_defect(raw, (32, 16, None), out=) alone: bits / 8 + 2 bytes per pixel
      defect_map  the same with the map: + 1 / 8 byte per pixel
      unpack      functional.raw_unpack(raw, out=) alone (packed formats)
      shade       functional.raw_shade(raw, out=) alone, from the same format
  (b) fused       net.serve(raw, out=, defect_correction=, lens_shading=) with the format in _DEFECT_SHADE_FUSED: one risp_raw_defect
                  with the gains, then risp_serve_classical_u8
      pass        the same call with the table empty: risp_raw_defect, risp_raw_shade, then risp_serve_classical_u8
  (c) serve_dc    net.serve(raw, out=, defect_correction=): what a user pays with the feature
      serve       the same call without the keyword (packed formats: the fused packed load of the classical launch)
Each round times every leg once (REPS calls, after 3 warm ones), after one round that is not kept - the first leg of the first
round otherwise pays for the clocks coming up -; per leg: the rounds, median, minimum and spread - the spread between the rounds of
ONE leg is the noise a difference between two legs has to clear.  The bytes of fused and pass are compared first.  Row verdict:
fused beats pass when median(pass) - median(fused) exceeds the larger of the two spreads; a format enters
pipeline_fusion._DEFECT_SHADE_FUSED only if that holds at both sizes, and the line `verdict: _DEFECT_SHADE_FUSED = ...` says which
(tests/test_defect_reference_cpu.py compares it with the table).  Bytes are algorithmic counts, the rate is those bytes over the
median time."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import reconfigisp_amd.functional as F  # noqa: E402
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF  # noqa: E402
from bench_serve_packed import frames_int, pack, pipeline, timed  # noqa: E402
from bench_serve_shade import vignette  # noqa: E402

HBM_PEAK = 8.0e12
ARCH = 'Demosaic_02_sRGB_11_01_14'
FORMATS = ['u16', 'raw10', 'raw12']
WHITE, BLACK, CELL = 1023.0, 64, 64
THRESHOLD, SLOPE, LISTED = 32, 16, 0.0005


def measure(net, shape, seed, fmt, reps, rounds, emit):
    n, h, w = shape
    pix = n * h * w
    bits = F.RAW_FORMAT[fmt] or 16
    x = frames_int(n, h, w, seed, int(WHITE) - BLACK) + BLACK
    raw = (x.to(torch.uint16) if fmt == 'u16' else pack(x, bits)).cuda()
    fkw = {} if fmt == 'u16' else dict(raw_format=fmt, raw_width=w)
    rng = np.random.default_rng(seed)
    coords = np.stack([rng.integers(0, h, int(h * w * LISTED)), rng.integers(0, w, int(h * w * LISTED))], axis=1)
    bitmap = F.defect_map(coords, h, w).cuda()
    dyn, dc = (THRESHOLD, SLOPE, None), (THRESHOLD, SLOPE, bitmap)
    shading = (F.shading_map(vignette(h, w), h, w, CELL).cuda(), CELL)
    out_f, out_p, out_d, out_s = (torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8) for _ in range(4))
    u16 = torch.empty((n, h, w), device='cuda', dtype=torch.uint16)
    io = bits / 8 + 2.0
    bpp = {'defect': io, 'defect_map': io + 0.125, 'unpack': io, 'shade': io, 'fused': io + 0.125 + 2 + 3, 'pass': io + 0.125 + 4 + 2 + 3,
           'serve_dc': io + 0.125 + 2 + 3, 'serve': bits / 8 + 3.0}

    def leg_defect():
        F.raw_defect(raw, dyn, bits, w, out=u16)

    def leg_defect_map():
        F.raw_defect(raw, dc, bits, w, out=u16)

    def leg_unpack():
        F.raw_unpack(raw, bits, w, out=u16)

    def leg_shade():
        F.raw_shade(raw, shading, BLACK, bits, w, out=u16)

    def leg_fused():
        PF._DEFECT_SHADE_FUSED = frozenset({fmt})
        net.serve(raw, WHITE, out=out_f, black_level=BLACK, defect_correction=dc, lens_shading=shading, **fkw)

    def leg_pass():
        PF._DEFECT_SHADE_FUSED = frozenset()
        net.serve(raw, WHITE, out=out_p, black_level=BLACK, defect_correction=dc, lens_shading=shading, **fkw)

    def leg_serve_dc():
        net.serve(raw, WHITE, out=out_d, black_level=BLACK, defect_correction=dc, **fkw)

    def leg_serve():
        net.serve(raw, WHITE, out=out_s, black_level=BLACK, **fkw)

    legs = {'defect': leg_defect, 'defect_map': leg_defect_map, 'shade': leg_shade, 'fused': leg_fused, 'pass': leg_pass,
            'serve_dc': leg_serve_dc, 'serve': leg_serve}
    if fmt != 'u16':
        legs['unpack'] = leg_unpack
    leg_fused()
    assert net.last_serve_route == 'classical' and net.last_serve_defect == 'fused'
    leg_pass()
    assert net.last_serve_route == 'classical' and net.last_serve_defect == 'pass'
    leg_serve_dc(), leg_serve()
    torch.cuda.synchronize()
    assert torch.equal(out_f, out_p), 'one launch and two disagree'
    assert len(torch.unique(out_f)) > 32
    changed = (out_d != out_s).any(dim=-1).float().mean().item()
    res = {k: [] for k in legs}
    for r in range(rounds + 1):                             # round 0 brings the clocks up and is not kept
        for name, fn in legs.items():
            t = timed(fn, reps)
            if r:
                res[name].append(t)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    emit(' %s, %s, %d x %d x %d, %d calls per round; us per call; the correction changes %.2f %% of the served pixels' % (
        fmt, ARCH, n, h, w, reps, 100 * changed))
    for name, v in res.items():
        emit('  %-10s rounds %s' % (name, ' '.join('%.1f' % t for t in v)))
        rate = bpp[name] * pix / (med[name] * 1e-6)
        emit('  %-10s median %.1f us  min %.1f  spread %.1f   %.3f B/pixel: %.3f TB/s = %.1f %% of the %.1f TB/s HBM peak' % (
            name, med[name], min(v), spread[name], bpp[name], rate / 1e12, 100 * rate / HBM_PEAK, HBM_PEAK / 1e12))
    emit('  (a) defect / shade = %.2f   defect_map / defect = %.2f%s' % (
        med['defect'] / med['shade'], med['defect_map'] / med['defect'],
        '   defect / unpack = %.2f' % (med['defect'] / med['unpack']) if 'unpack' in med else ''))
    gain, noise = med['pass'] - med['fused'], max(spread['pass'], spread['fused'])
    won = gain > noise
    emit('  (b) pass - fused = %.1f us against a spread of %.1f us: one launch %s   fused / pass = %.3f' % (
        gain, noise, 'BEATS two' if won else 'does NOT beat two', med['fused'] / med['pass']))
    emit('  (c) serve_dc - serve = %.1f us: serve_dc / serve = %.3f   (%.0f MPix/s with the correction)' % (
        med['serve_dc'] - med['serve'], med['serve_dc'] / med['serve'], pix / med['serve_dc']))
    return won


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

    emit('tools/bench_serve_defect.py --reps %d --rounds %d   (%s)' % (args.reps, args.rounds, torch.cuda.get_device_name(0)))
    emit('(a) defect / defect_map / unpack / shade: the pre-pass launches alone   (b) fused / pass: net.serve(raw, out=, '
         'defect_correction=, lens_shading=) with one pre-pass launch or two   (c) serve_dc / serve: net.serve(raw, out=) with and '
         'without defect_correction; host side included')
    table = PF._DEFECT_SHADE_FUSED
    batch, frame = (64, 256, 256), (1, 3000, 4000)
    net = pipeline(ARCH)
    rows = {}
    try:
        for fmt in FORMATS:
            rows[fmt] = [measure(net, shape, seed, fmt, reps, args.rounds, emit)
                         for shape, seed, reps in ((batch, 10, args.reps), (frame, 20, max(20, args.reps // 3)))]
    finally:
        PF._DEFECT_SHADE_FUSED = table
    for fmt in FORMATS:
        emit('%s: one launch beats two by more than the spread in %d of %d rows' % (fmt, sum(rows[fmt]), len(rows[fmt])))
    emit('verdict: _DEFECT_SHADE_FUSED = %s' % (' '.join(f for f in FORMATS if all(rows[f])) or 'none'))
    emit('pipeline_fusion.defect_shade answers \'fused\' for: %s' % (', '.join(sorted(table)) or 'no format'))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
