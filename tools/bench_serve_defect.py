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
import numpy as np
import torch

import serve_bench as SB
import reconfigisp_amd.functional as F
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF

ARCH = 'Demosaic_02_sRGB_11_01_14'
FORMATS = ['u16', 'raw10', 'raw12']
WHITE, BLACK, CELL = 1023.0, 64, 64
THRESHOLD, SLOPE, LISTED = 32, 16, 0.0005


def measure(net, shape, seed, fmt, reps, rounds, emit):
    n, h, w = shape
    pix = n * h * w
    bits = F.RAW_FORMAT[fmt] or 16
    x = SB.frames_int(n, h, w, seed, int(WHITE) - BLACK) + BLACK
    raw = (x.to(torch.uint16) if fmt == 'u16' else SB.pack(x, bits)).cuda()
    fkw = {} if fmt == 'u16' else dict(raw_format=fmt, raw_width=w)
    rng = np.random.default_rng(seed)
    coords = np.stack([rng.integers(0, h, int(h * w * LISTED)), rng.integers(0, w, int(h * w * LISTED))], axis=1)
    bitmap = F.defect_map(coords, h, w).cuda()
    dyn, dc = (THRESHOLD, SLOPE, None), (THRESHOLD, SLOPE, bitmap)
    shading = (F.shading_map(SB.vignette(h, w), h, w, CELL).cuda(), CELL)
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
    res = SB.rounds_of(legs, reps, rounds, True)
    med = {k: SB.median(v) for k, v in res.items()}
    emit(' %s, %s, %d x %d x %d, %d calls per round; us per call; the correction changes %.2f %% of the served pixels' % (
        fmt, ARCH, n, h, w, reps, 100 * changed))
    for name, v in res.items():
        rounds_line, stats_line = SB.leg_lines(name, v, 10)
        emit(rounds_line)
        emit(stats_line + '   %.3f B/pixel: %s' % (bpp[name], SB.hbm_share(bpp[name] * pix, med[name])))
    emit('  (a) defect / shade = %.2f   defect_map / defect = %.2f%s' % (
        med['defect'] / med['shade'], med['defect_map'] / med['defect'],
        '   defect / unpack = %.2f' % (med['defect'] / med['unpack']) if 'unpack' in med else ''))
    gain, noise = SB.margin(res['fused'], res['pass'])
    won = SB.beats(res['fused'], res['pass'])
    emit('  (b) pass - fused = %.1f us against a spread of %.1f us: one launch %s   fused / pass = %.3f' % (
        gain, noise, 'BEATS two' if won else 'does NOT beat two', med['fused'] / med['pass']))
    emit('  (c) serve_dc - serve = %.1f us: serve_dc / serve = %.3f   (%.0f MPix/s with the correction)' % (
        med['serve_dc'] - med['serve'], med['serve_dc'] / med['serve'], pix / med['serve_dc']))
    return won


def main():
    args = SB.parser(300, 7).parse_args()
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    emit('(a) defect / defect_map / unpack / shade: the pre-pass launches alone   (b) fused / pass: net.serve(raw, out=, '
         'defect_correction=, lens_shading=) with one pre-pass launch or two   (c) serve_dc / serve: net.serve(raw, out=) with and '
         'without defect_correction; host side included')
    table = PF._DEFECT_SHADE_FUSED
    batch, frame = (64, 256, 256), (1, 3000, 4000)
    net = SB.pipeline(ARCH)
    rows = {}
    try:
        for fmt in FORMATS:
            rows[fmt] = [measure(net, shape, seed, fmt, reps, args.rounds, emit)
                         for shape, seed, reps in ((batch, 10, args.reps), (frame, 20, max(20, args.reps // 3)))]
    finally:
        PF._DEFECT_SHADE_FUSED = table
    for fmt in FORMATS:
        emit('%s: one launch beats two by more than the spread in %d of %d rows' % (fmt, sum(rows[fmt]), len(rows[fmt])))
    emit(SB.verdict_line('_DEFECT_SHADE_FUSED', [f for f in FORMATS if all(rows[f])]))
    emit('pipeline_fusion.defect_shade answers \'fused\' for: %s' % (', '.join(sorted(table)) or 'no format'))
    emit.write()


if __name__ == '__main__':
    main()
