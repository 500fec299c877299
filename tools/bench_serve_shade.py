#!/usr/bin/env python3
"""GPU box: lens-shading correction in the serving path - the fused shading load of the classical one-launch kernel against the
shade launch followed by the uint16 call, on resident frames, in interleaved rounds in one process.

    make -C reconfigisp_amd/csrc OUT=/tmp/parent/libreconfigisp_hip.so OBJDIR=/tmp/parent      (in a checkout of the parent commit)
    python tools/bench_serve_shade.py --parent-lib /tmp/parent/libreconfigisp_hip.so [--out profiles/serve_shade.txt]
    python tools/bench_serve_shade.py [--reps 300] [--rounds 7]                                 (without the parent leg)

Pipelines (OriginUniversal, route 'classical'): Demosaic_02_sRGB_11_01_14 (bilinear, WbManual, Gamma, GtmManual) and
Demosaic_03_sRGB_11_04_01 (Malvar-He-Cutler, WbManual, Filmic, Gamma); 64 x 256 x 256 and one 3000 x 4000 frame; 12-bit samples in
uint16, black level 64, white level 4095, a map of cell 64 with gains 1 .. 2 rising to the corners.  Legs, host side included
(what a caller pays), timed between two device events:
  fused      net.serve(raw, out=, lens_shading=) with ('classical', 'u16') in _FUSED_SHADE: risp_serve_classical_shaded, one launch
  pass       the same call with the table empty: risp_raw_shade into the cached frames, then risp_serve_classical_u8 - two launches
  u16        net.serve(shaded, white - black, out=): the uint16 call alone, this build
  u16_parent the same call with risp_serve_classical_u8 of --parent-lib (the parent commit's build of the library)
  shade      functional.raw_shade(raw, out=) alone (2 bytes read and 2 written per pixel)
Each round times every leg once (REPS calls, after 3 warm ones), after one round that is not kept - the first leg of the first
round otherwise pays for the clocks coming up, by 3 to 9 us here -; per leg: the rounds, median, minimum and spread - the spread
between the rounds of ONE leg is the noise a difference between two legs has to clear.  The bytes of fused, pass and u16 are
compared first.  Row verdict: fused beats pass when median(pass) - median(fused) exceeds the larger of the two spreads;
('classical', 'u16') enters pipeline_fusion._FUSED_SHADE only if that holds in all four rows, and the line `verdict: _FUSED_SHADE = ...`
says which (tests/test_lens_shading_reference_cpu.py compares it with the table).  u16 against u16_parent shows whether the
existing instantiations saw the new template parameter: their difference has to lie within the spreads.  Bytes are algorithmic
counts, the share of HBM peak is those bytes over the median time."""
import torch

import serve_bench as SB
import reconfigisp_amd.functional as F
from reconfigisp_amd import lib as L
from reconfigisp_amd.codes.data.synthetic_raw import make_batch
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF

ARCHS = ['Demosaic_02_sRGB_11_01_14', 'Demosaic_03_sRGB_11_04_01']
ENTRY = ('classical', 'u16')
WHITE, BLACK, CELL = 4095.0, 64, 64
CALL = 'risp_serve_classical_u8'
PARENT = None           # --parent-lib: risp_serve_classical_u8 of a second build of the library, bound with the same signature


def measure(arch, shape, seed, reps, rounds, emit):
    n, h, w = shape
    pix = n * h * w
    bay = make_batch(n, h, w, seed=seed)[0][:, 0]
    raw = (bay * (WHITE - BLACK) + BLACK).round().clamp(0, WHITE).to(torch.int32).to(torch.uint16).cuda()
    shading = (F.shading_map(SB.vignette(h, w), h, w, CELL).cuda(), CELL)
    net = SB.pipeline(arch)
    out_f, out_p, out_u = (torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8) for _ in range(3))
    shaded = torch.empty((n, h, w), device='cuda', dtype=torch.uint16)
    bpp = {'fused': 2 + 3.0, 'pass': 2 + 2 + 2 + 3.0, 'u16': 2 + 3.0, 'u16_parent': 2 + 3.0, 'shade': 2 + 2.0}

    def leg_fused():
        PF._FUSED_SHADE = frozenset({ENTRY})
        net.serve(raw, WHITE, out=out_f, black_level=BLACK, lens_shading=shading)

    def leg_pass():
        PF._FUSED_SHADE = frozenset()
        net.serve(raw, WHITE, out=out_p, black_level=BLACK, lens_shading=shading)

    def leg_u16():
        net.serve(shaded, WHITE - BLACK, out=out_u)

    def leg_shade():
        F.raw_shade(raw, shading, BLACK, out=shaded)

    own = getattr(L.load(), CALL)
    legs = {'fused': (leg_fused, own), 'pass': (leg_pass, own), 'u16': (leg_u16, own), 'shade': (leg_shade, own)}
    if PARENT is not None:
        legs['u16_parent'] = (leg_u16, PARENT)

    def timed_bound(leg, reps):                             # a leg is (call, the build whose kernel is bound while it is timed)
        fn, kernel = leg
        L._FN[CALL] = kernel
        try:
            return SB.timed(fn, reps)
        finally:
            L._FN[CALL] = own

    leg_shade(), leg_fused()
    assert net.last_serve_route == 'classical' and net.last_serve_shade == 'fused'
    leg_pass()
    assert net.last_serve_route == 'classical' and net.last_serve_shade == 'pass'
    leg_u16()
    torch.cuda.synchronize()
    assert torch.equal(out_f, out_p) and torch.equal(out_f, out_u), 'the legs disagree'
    assert len(torch.unique(out_f)) > 32
    res = SB.rounds_of(legs, reps, rounds, True, timed_bound)
    if PARENT is not None:
        out_u.zero_()
        L._FN[CALL] = PARENT
        try:
            leg_u16()
        finally:
            L._FN[CALL] = own
        torch.cuda.synchronize()
        assert torch.equal(out_u, out_f), 'the parent build and this one disagree'
    med = {k: SB.median(v) for k, v in res.items()}
    emit(' %s, %d x %d x %d, cell %d, %d calls per round; us per call' % (arch, n, h, w, CELL, reps))
    for name, v in res.items():
        rounds_line, stats_line = SB.leg_lines(name, v, 10)
        emit(rounds_line)
        emit(stats_line + '   %.2f B/pixel: %s' % (bpp[name], SB.hbm_share(bpp[name] * pix, med[name])))
    gain, noise = SB.margin(res['fused'], res['pass'])
    won = SB.beats(res['fused'], res['pass'])
    emit('  pass - fused = %.1f us against a spread of %.1f us: the fused shading load %s   fused / pass = %.3f   fused / u16 = %.3f   '
         '(%.0f MPix/s)' % (gain, noise, 'BEATS the shade launch' if won else 'does NOT beat the shade launch',
                            med['fused'] / med['pass'], med['fused'] / med['u16'], pix / med['fused']))
    if PARENT is not None:
        diff, noise = SB.margin(res['u16_parent'], res['u16'])
        emit('  u16 - u16_parent = %.1f us against a spread of %.1f us: the existing instantiation is %s' % (
            diff, noise, 'within the noise of the parent build\'s' if abs(diff) <= noise else 'NOT within the noise of the parent build\'s'))
    return won


def main():
    global PARENT
    ap = SB.parser(300, 7)
    ap.add_argument('--parent-lib', default=None, help='a second build of libreconfigisp_hip.so (the parent commit\'s): its '
                    'risp_serve_classical_u8 is timed in the same rounds as leg u16_parent')
    args = ap.parse_args()
    if args.parent_lib:
        PARENT = getattr(SB.load_parent(args.parent_lib, [CALL]), CALL)
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args, ' --parent-lib <the parent commit\'s build>' if args.parent_lib else ''))
    emit('fused: net.serve(raw, out=, lens_shading=) with the fused shading load   pass: the same call, risp_raw_shade first   '
         'u16: net.serve(shaded, out=)   u16_parent: u16 with the parent build\'s kernel   shade: raw_shade(out=) alone; host side included')
    table = PF._FUSED_SHADE
    batch, frame = (64, 256, 256), (1, 3000, 4000)
    rows = []
    try:
        for arch in ARCHS:
            for shape, seed, reps in ((batch, 10, args.reps), (frame, 20, max(20, args.reps // 3))):
                rows.append(measure(arch, shape, seed, reps, args.rounds, emit))
    finally:
        PF._FUSED_SHADE = table
    emit('the fused shading load beats shade launch + uint16 call by more than the spread in %d of %d rows' % (sum(rows), len(rows)))
    emit(SB.verdict_line('_FUSED_SHADE', ['/'.join(ENTRY)] if all(rows) else []))
    emit('pipeline_fusion.serve_shade answers \'fused\' for: %s' % (', '.join('%s/%s' % k for k in sorted(table)) or 'no route'))
    emit.write()


if __name__ == '__main__':
    main()
