#!/usr/bin/env python3
"""GPU box: the denoiser pipelines' one launch (serve(fast_denoise=True), risp_serve_denoise_u8) against the composed route
of the same pipeline - the default call, unchanged code - on resident uint16 frames, in interleaved rounds in one process.

    python tools/bench_serve_denoise.py [--out profiles/serve_denoise.txt] [--reps 100] [--rounds 7]

Pipelines (OriginUniversal): Demosaic_0D_sRGB_11_NN_01_14 - a bilinear (D = 2) or Malvar-He-Cutler (D = 3) demosaic,
WbManual, the bilateral (NN = 07), the median (08, its parameter set for the 3 x 3 window) or non-local means (09), Gamma,
GtmManual; 64 x 256 x 256 and one 3000 x 4000 frame.  Legs, each net.serve(raw, out=buf) with the host side included (what a
caller pays), timed between two device events:
  denoise     risp_serve_denoise_u8, one launch
  composed    risp_raw_crop -> risp_origin_demosaic -> chain -> the denoiser (the bilateral with its element-wise tail in
              risp_bilateral_chain_fwd) -> chain -> risp_quantise_u8, every stage output an fp32 plane
Each round times every leg once (REPS calls, after 3 warm ones); per leg: the rounds, median, minimum and spread - the spread
between the rounds of ONE leg is the noise a difference between two legs has to clear.  The bytes of the two legs are compared
first.  Bytes moved are algorithmic counts from the module list (fp32 planes written and read back by the composed route;
2 read + 3 written by the one launch)."""
import torch

import serve_bench as SB
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
from reconfigisp_amd.codes.models.modules import tools_origin as T

WHITE = 1023.0
DEMOSAICS = [('bilinear', 2), ('malvar', 3)]
DENOISERS = [('bilateral', 7), ('median', 8), ('fastnlm', 9)]


def composed_bytes_per_pixel(modules):
    """what the composed route moves per pixel: the crop (2 + 4), the demosaic (4 + 12), an element-wise run of k stages in
    one launch (12 + 12 k), a median / non-local means (12 + 12), a bilateral with the k stages behind it in its launch
    (12 + 12 (1 + k)), the conversion (12 + 3)"""
    total, run, bilateral = 6 + 16 + 15, 0, False
    flush = lambda: (12 + 12 * (run + bilateral)) if run or bilateral else 0
    for m in modules[1:]:
        if type(m) is T.Skip:
            continue
        if type(m) in PF._DENOISER:
            total, run, bilateral = total + flush(), 0, type(m) is T.OriginNoiseBilateral
            if not bilateral:
                total += 24
        else:
            run += 1
    return total + flush()


def measure(arch, raw, reps, rounds, emit):
    n, h, w = raw.shape
    pix = n * h * w
    net = SB.pipeline(arch, median=SB.MEDIAN_3X3)
    buf = {k: torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8) for k in ('denoise', 'composed')}

    def denoise():
        net.serve(raw, WHITE, out=buf['denoise'], fast_denoise=True)

    def composed():
        net.serve(raw, WHITE, out=buf['composed'])

    legs = {'denoise': denoise, 'composed': composed}
    composed()
    assert net.last_serve_route == 'composed'
    denoise()
    assert net.last_serve_route == 'denoise'
    torch.cuda.synchronize()
    assert torch.equal(buf['denoise'], buf['composed']), 'the one launch and the composed route disagree'
    res = SB.rounds_of(legs, reps, rounds, False)
    med = {k: SB.median(v) for k, v in res.items()}
    bpp = {'denoise': 5, 'composed': composed_bytes_per_pixel(net.all_modules)}
    emit(' %s, %d x %d x %d, %d calls per round; us per call' % (arch, n, h, w, reps))
    for name, v in res.items():
        rounds_line, stats_line = SB.leg_lines(name, v, 9)
        emit(rounds_line)
        emit(stats_line + '   %d B/pixel: %.3f TB/s' % (bpp[name], bpp[name] * pix / (med[name] * 1e-6) / 1e12))
    emit('  denoise / composed = %.3f   (%.0f MPix/s against %.0f)' % (
        med['denoise'] / med['composed'], pix / med['denoise'], pix / med['composed']))
    return med


def main():
    args = SB.parser(100, 7).parse_args()
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    emit('net.serve(raw, out=buf[, fast_denoise=True]), host side included')
    batch, frame = SB.frames_u16(64, 256, 256, 10, WHITE), SB.frames_u16(1, 3000, 4000, 20, WHITE)
    wins = {}
    for den, code in DENOISERS:
        for dem, kind in DEMOSAICS:
            arch = 'Demosaic_%02d_sRGB_11_%02d_01_14' % (kind, code)
            for raw, reps in ((batch, args.reps), (frame, max(10, args.reps // 3))):
                med = measure(arch, raw, reps, args.rounds, emit)
                wins.setdefault(den, []).append(med['denoise'] < med['composed'])
    for den, w in wins.items():
        emit('%s: the one launch beats the composed route in %d of %d cases' % (den, sum(w), len(w)))
    emit.write()


if __name__ == '__main__':
    main()
