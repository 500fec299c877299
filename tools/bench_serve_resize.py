#!/usr/bin/env python3
"""GPU box: a scaled, cropped output of the serving path - what the resize launch costs, whether its fused NV12 store beats
resize-to-BGR plus the conversion launch, and what a served call pays and saves; on resident frames, in interleaved rounds in one
process.

    python tools/bench_serve_resize.py [--out profiles/serve_resize.txt] [--reps 300] [--rounds 7]

Pipeline (OriginUniversal, route 'classical'): Demosaic_02_sRGB_11_01_14 (bilinear, WbManual, Gamma, GtmManual), black level 64,
white level 1023.  Sizes: one 3000 x 4000 frame whose window (375, 0, 2250, 4000) - the 16:9 part - goes to 1080 x 1920, and
64 x 256 x 256 frames to 128 x 128.  The launch legs run on the packed image the pipeline serves for those frames.  Legs, host
side included (what a caller pays), timed between two device events:
  (a) bgr_K / nv12_K   functional.bgr8_resize(img, size, window, K, out=) alone, K = box, triangle, bicubic, packed BGR out and NV12
                       out: the window's 3 bytes per pixel read once, 3 or 1.5 bytes per output pixel written once
  (b) fused_K          functional.bgr8_resize(img, ..., K, nv12=, out=): the resize launch stores NV12
      pass_K           functional.bgr8_to_nv12(functional.bgr8_resize(img, ..., K, out=bgr), out=): two launches; K = triangle, bicubic
  (c) serve_rs         net.serve(raw, out=, out_size=, out_window=): what a user pays with the feature (triangle)
      serve            the same call without the keywords, (N,H,W,3) out
      serve_torch      serve, then torch.nn.functional.interpolate(mode='bilinear', antialias=True) of the window with its two
                       conversions (to float planes and back to packed bytes): time only, its bytes differ
Each round times every leg once (REPS calls, after 3 warm ones), after one round that is not kept; per leg: the rounds, median,
minimum and spread - the spread between the rounds of ONE leg is the noise a difference between two legs has to clear.  The bytes
of fused and pass are compared first.  Row verdict: fused beats pass when median(pass) - median(fused) exceeds the larger of the
two spreads; 'nv12' enters pipeline_fusion._RESIZE_NV12_FUSED only if that holds in all four rows, and the line
`verdict: _RESIZE_NV12_FUSED = ...` says so (tests/test_resize_reference_cpu.py compares it with the table).  Bytes are
algorithmic counts, the rate is those bytes over the median time."""
import torch

import serve_bench as SB
import reconfigisp_amd.functional as F
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF

ARCH = 'Demosaic_02_sRGB_11_01_14'
WHITE, BLACK = 1023.0, 64
MATRIX = 'bt709_video'
VERDICT_KERNELS = ('triangle', 'bicubic')


def measure(net, shape, size, window, seed, reps, rounds, emit):
    n, h, w = shape
    oh, ow = size
    y0, x0, wh, ww = window if window is not None else (0, 0, h, w)
    raw = (SB.frames_int(n, h, w, seed, int(WHITE) - BLACK) + BLACK).to(torch.uint16).cuda()
    img = net.serve(raw, WHITE, black_level=BLACK).clone()
    assert net.last_serve_route == 'classical'
    u8 = lambda *s: torch.empty(s, device='cuda', dtype=torch.uint8)
    out_b, out_n, out_n2, out_rs, out_full = u8(n, oh, ow, 3), u8(n, oh * 3 // 2, ow), u8(n, oh * 3 // 2, ow), u8(n, oh, ow, 3), u8(n, h, w, 3)
    read = n * wh * ww * 3.0
    nbytes = {}
    legs = {}
    for k in F.RESAMPLE:
        legs['bgr_' + k] = lambda k=k: F.bgr8_resize(img, size, window, k, out=out_b)
        legs['nv12_' + k] = lambda k=k: F.bgr8_resize(img, size, window, k, nv12=MATRIX, out=out_n)
        nbytes['bgr_' + k], nbytes['nv12_' + k] = read + n * oh * ow * 3.0, read + n * oh * ow * 1.5
    for k in VERDICT_KERNELS:
        legs['fused_' + k] = lambda k=k: F.bgr8_resize(img, size, window, k, nv12=MATRIX, out=out_n)
        legs['pass_' + k] = lambda k=k: F.bgr8_to_nv12(F.bgr8_resize(img, size, window, k, out=out_b), MATRIX, out=out_n2)
        nbytes['fused_' + k], nbytes['pass_' + k] = read + n * oh * ow * 1.5, read + n * oh * ow * (3.0 + 3.0 + 1.5)

    def leg_serve_rs():
        net.serve(raw, WHITE, out=out_rs, black_level=BLACK, out_size=size, out_window=window)

    def leg_serve():
        net.serve(raw, WHITE, out=out_full, black_level=BLACK)

    def leg_serve_torch():
        full = net.serve(raw, WHITE, out=out_full, black_level=BLACK)
        planes = full[:, y0:y0 + wh, x0:x0 + ww].permute(0, 3, 1, 2).float()
        small = torch.nn.functional.interpolate(planes, size=size, mode='bilinear', antialias=True)
        return small.round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    legs.update(serve_rs=leg_serve_rs, serve=leg_serve, serve_torch=leg_serve_torch)
    nbytes.update(serve_rs=n * h * w * (2.0 + 3.0) + read + n * oh * ow * 3.0, serve=n * h * w * (2.0 + 3.0), serve_torch=None)
    for k in VERDICT_KERNELS:
        legs['fused_' + k](), legs['pass_' + k]()
        torch.cuda.synchronize()
        assert torch.equal(out_n, out_n2), 'the fused store and the two launches disagree (%s)' % k
    leg_serve_rs()
    assert net.last_serve_resize == 'pass' and torch.equal(out_rs, F.bgr8_resize(img, size, window, 'triangle'))
    theirs = leg_serve_torch()
    diff = (theirs.int() - out_rs.int()).abs()
    assert len(torch.unique(out_rs)) > 32
    res = SB.rounds_of(legs, reps, rounds, True)
    med = {k: SB.median(v) for k, v in res.items()}
    emit(' %s, %d x %d x %d, window %s -> %d x %d, %d calls per round; us per call; tile rows %d, span %d; torch differs from '
         'serve_rs in %.1f %% of the bytes, by at most %d' % (ARCH, n, h, w, (y0, x0, wh, ww), oh, ow, reps,
                                                              *F.resize_tile_rows(wh, oh, 'triangle', y0),
                                                              100 * (diff > 0).float().mean().item(), diff.max().item()))
    for name, v in res.items():
        rounds_line, line = SB.leg_lines(name, v, 14)
        emit(rounds_line)
        if nbytes[name] is not None:
            line += '   %.1f MB: %s' % (nbytes[name] / 1e6, SB.hbm_share(nbytes[name], med[name]))
        emit(line)
    won = []
    for k in VERDICT_KERNELS:
        gain, noise = SB.margin(res['fused_' + k], res['pass_' + k])
        won.append(SB.beats(res['fused_' + k], res['pass_' + k]))
        emit('  (b) %-8s pass - fused = %.1f us against a spread of %.1f us: the fused store %s   fused / pass = %.3f' % (
            k, gain, noise, 'BEATS two launches' if won[-1] else 'does NOT beat two launches', med['fused_' + k] / med['pass_' + k]))
    emit('  (c) serve_rs - serve = %.1f us: serve_rs / serve = %.3f;  serve_torch - serve = %.1f us: serve_rs / serve_torch = %.3f   '
         '(%.0f MPix/s of sensor with the resize)' % (med['serve_rs'] - med['serve'], med['serve_rs'] / med['serve'],
                                                       med['serve_torch'] - med['serve'], med['serve_rs'] / med['serve_torch'],
                                                       n * h * w / med['serve_rs']))
    return won


def main():
    args = SB.parser(300, 7).parse_args()
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    emit('(a) bgr_K / nv12_K: the resize launch alone   (b) fused_K / pass_K: NV12 from the resize launch or from resize-to-BGR plus '
         'risp_bgr8_to_nv12   (c) serve_rs / serve / serve_torch: net.serve(raw, out=) with out_size, without, and followed by '
         'torch.nn.functional.interpolate; host side included')
    net = SB.pipeline(ARCH)
    rows = []
    rows += measure(net, (1, 3000, 4000), (1080, 1920), (375, 0, 2250, 4000), 20, max(20, args.reps // 3), args.rounds, emit)
    rows += measure(net, (64, 256, 256), (128, 128), None, 10, args.reps, args.rounds, emit)
    emit('the fused NV12 store beats two launches by more than the spread in %d of %d rows' % (sum(rows), len(rows)))
    emit(SB.verdict_line('_RESIZE_NV12_FUSED', ['nv12'] if all(rows) else []))
    emit("pipeline_fusion.resize_store('nv12') answers %r" % PF.resize_store('nv12'))
    emit.write()


if __name__ == '__main__':
    main()
