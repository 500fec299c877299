#!/usr/bin/env python3
"""GPU box: output sharpening on the serving path - what the sharpen launch costs, whether its fused NV12 store beats
sharpen-to-BGR plus the conversion launch, and what a served call pays and saves; on resident frames, in interleaved rounds in one
process.

    python tools/bench_serve_sharpen.py [--out profiles/serve_sharpen.txt] [--reps 300] [--rounds 7]

Pipeline (OriginUniversal, route 'classical'): Demosaic_02_sRGB_11_01_14 (bilinear, WbManual, Gamma, GtmManual), black level 64,
white level 1023.  Sizes: 64 x 256 x 256 frames, one 3000 x 4000 frame, and that frame's window (375, 0, 2250, 4000) scaled to
1080 x 1920 (``out_size``) with the sharpening behind the scaler.  The launch legs run on the packed image the pipeline serves
(and resizes) for those frames.  sharpen = (384, 2, 48, radius).  Legs, host side included (what a caller pays), timed between
two device events:
  (a) bgr_rR / nv12_rR  functional.bgr8_sharpen(img, (.., R), out=) alone, R = 1, 2, packed BGR out and NV12 out: 3 bytes per
                        pixel read once, 3 or 1.5 written once
      resize            functional.bgr8_resize(img, out=) to the image's own size (one tap of 16384): the sister launch, same bytes
  (b) fused_rR          functional.bgr8_sharpen(img, .., nv12=, out=): the sharpen launch stores NV12
      pass_rR           functional.bgr8_to_nv12(functional.bgr8_sharpen(img, .., out=bgr), out=): two launches
  (c) serve_sh          net.serve(raw, out=, sharpen=[, out_size=, out_window=]): what a user pays with the feature (radius 2)
      serve             the same call without the keyword
      serve_torch       serve, then the same filter composed from torch ops on the served image with its two conversions (to
                        float planes and back to packed bytes): time only
Each round times every leg once (REPS calls, after 3 warm ones), after one round that is not kept; per leg: the rounds, median,
minimum and spread - the spread between the rounds of ONE leg is the noise a difference between two legs has to clear.  The bytes
of fused and pass are compared first.  Row verdict: fused beats pass when median(pass) - median(fused) exceeds the larger of the
two spreads; 'nv12' enters pipeline_fusion._SHARPEN_NV12_FUSED only if that holds in every row, and the line
`verdict: _SHARPEN_NV12_FUSED = ...` says so (tests/test_sharpen_reference_cpu.py compares it with the table).  Bytes are
algorithmic counts (6 per pixel for BGR out, 4.5 for NV12), the rate is those bytes over the median time.  No counters are read."""
import torch

import serve_bench as SB
import reconfigisp_amd.functional as F
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF

ARCH = 'Demosaic_02_sRGB_11_01_14'
WHITE, BLACK = 1023.0, 64
MATRIX = 'bt709_video'
AMOUNT, THRESHOLD, LIMIT = 384, 2, 48


def torch_sharpen(img, sharpen):
    """the same filter from torch ops: packed bytes -> float planes -> luma, binomial blur (replicate pad), coring, gain, limit
    -> packed bytes"""
    amount, threshold, limit, radius = sharpen
    x = img.permute(0, 3, 1, 2).float()
    luma = torch.floor((29.0 * x[:, 0:1] + 150.0 * x[:, 1:2] + 77.0 * x[:, 2:3] + 128.0) / 256.0)
    taps = torch.tensor([1.0, 2.0, 1.0] if radius == 1 else [1.0, 4.0, 6.0, 4.0, 1.0], device=img.device)
    k = torch.outer(taps, taps)
    k = (k * (256.0 / k.sum()))[None, None]
    blur = torch.nn.functional.conv2d(torch.nn.functional.pad(luma, (radius,) * 4, mode='replicate'), k)
    d = 256.0 * luma - blur
    e = torch.clamp(torch.floor((torch.clamp(d.abs() - 256.0 * threshold, min=0.0) * amount + 32768.0) / 65536.0), max=float(limit))
    return (x + torch.sign(d) * e).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def measure(net, shape, resize, seed, reps, rounds, emit):
    n, h, w = shape
    raw = (SB.frames_int(n, h, w, seed, int(WHITE) - BLACK) + BLACK).to(torch.uint16).cuda()
    rkw = {} if resize is None else dict(out_size=resize[0], out_window=resize[1])
    img = net.serve(raw, WHITE, black_level=BLACK, **rkw).clone()
    assert net.last_serve_route == 'classical'
    ih, iw = img.shape[1:3]
    u8 = lambda *s: torch.empty(s, device='cuda', dtype=torch.uint8)        # noqa: E731
    out_b, out_b2, out_n, out_n2, out_sv = u8(n, ih, iw, 3), u8(n, ih, iw, 3), u8(n, ih * 3 // 2, iw), u8(n, ih * 3 // 2, iw), u8(n, ih, iw, 3)
    pix = float(n * ih * iw)
    sharp = {r: (AMOUNT, THRESHOLD, LIMIT, r) for r in F.SHARPEN_RADII}
    legs, nbytes = {}, {}
    for r in F.SHARPEN_RADII:
        legs['bgr_r%d' % r] = lambda r=r: F.bgr8_sharpen(img, sharp[r], out=out_b)
        legs['nv12_r%d' % r] = lambda r=r: F.bgr8_sharpen(img, sharp[r], nv12=MATRIX, out=out_n)
        nbytes['bgr_r%d' % r], nbytes['nv12_r%d' % r] = 6.0 * pix, 4.5 * pix
    legs['resize'] = lambda: F.bgr8_resize(img, (ih, iw), None, 'triangle', out=out_b2)
    nbytes['resize'] = 6.0 * pix
    for r in F.SHARPEN_RADII:
        legs['fused_r%d' % r] = lambda r=r: F.bgr8_sharpen(img, sharp[r], nv12=MATRIX, out=out_n)
        legs['pass_r%d' % r] = lambda r=r: F.bgr8_to_nv12(F.bgr8_sharpen(img, sharp[r], out=out_b), MATRIX, out=out_n2)
        nbytes['fused_r%d' % r], nbytes['pass_r%d' % r] = 4.5 * pix, (6.0 + 4.5) * pix

    def leg_serve_sh():
        net.serve(raw, WHITE, out=out_sv, black_level=BLACK, sharpen=sharp[2], **rkw)

    def leg_serve():
        net.serve(raw, WHITE, out=out_b2, black_level=BLACK, **rkw)

    def leg_serve_torch():
        return torch_sharpen(net.serve(raw, WHITE, out=out_b2, black_level=BLACK, **rkw), sharp[2])

    legs.update(serve_sh=leg_serve_sh, serve=leg_serve, serve_torch=leg_serve_torch)
    nbytes.update(serve_sh=None, serve=None, serve_torch=None)
    for r in F.SHARPEN_RADII:
        legs['fused_r%d' % r](), legs['pass_r%d' % r]()
        torch.cuda.synchronize()
        assert torch.equal(out_n, out_n2), 'the fused store and the two launches disagree (radius %d)' % r
    leg_serve_sh()
    assert net.last_serve_sharpen == 'pass' and torch.equal(out_sv, F.bgr8_sharpen(img, sharp[2]))
    theirs = leg_serve_torch()
    diff = (theirs.int() - out_sv.int()).abs()
    changed = (out_sv != img).float().mean().item()
    assert len(torch.unique(out_sv)) > 32 and changed > 0.05
    res = SB.rounds_of(legs, reps, rounds, True)
    med = {k: SB.median(v) for k, v in res.items()}
    emit(' %s, %d x %d x %d%s, sharpened image %d x %d, %d calls per round; us per call; the sharpening changes %.1f %% of the bytes; '
         'torch differs from serve_sh in %.2f %% of the bytes, by at most %d'
         % (ARCH, n, h, w, '' if resize is None else ', window %s -> %d x %d' % (resize[1], resize[0][0], resize[0][1]), ih, iw, reps,
            100 * changed, 100 * (diff > 0).float().mean().item(), diff.max().item()))
    for name, v in res.items():
        rounds_line, line = SB.leg_lines(name, v, 12)
        emit(rounds_line)
        if nbytes[name] is not None:
            line += '   %.1f MB: %s' % (nbytes[name] / 1e6, SB.hbm_share(nbytes[name], med[name]))
        emit(line)
    won = []
    for r in F.SHARPEN_RADII:
        f, p = 'fused_r%d' % r, 'pass_r%d' % r
        gain, noise = SB.margin(res[f], res[p])
        won.append(SB.beats(res[f], res[p]))
        emit('  (b) radius %d  pass - fused = %.1f us against a spread of %.1f us: the fused store %s   fused / pass = %.3f' % (
            r, gain, noise, 'BEATS two launches' if won[-1] else 'does NOT beat two launches', med[f] / med[p]))
    emit('  (a) bgr_r2 / resize = %.3f   bgr_r1 / resize = %.3f' % (med['bgr_r2'] / med['resize'], med['bgr_r1'] / med['resize']))
    emit('  (c) serve_sh - serve = %.1f us: serve_sh / serve = %.3f;  serve_torch - serve = %.1f us: (serve_torch - serve) / '
         '(serve_sh - serve) = %.1f   (%.0f MPix/s of sensor with the sharpening)' % (
             med['serve_sh'] - med['serve'], med['serve_sh'] / med['serve'], med['serve_torch'] - med['serve'],
             (med['serve_torch'] - med['serve']) / (med['serve_sh'] - med['serve']), n * h * w / med['serve_sh']))
    return won


def main():
    args = SB.parser(300, 7).parse_args()
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    emit('(a) bgr_rR / nv12_rR: the sharpen launch alone, resize: risp_bgr8_resize at the same size   (b) fused_rR / pass_rR: NV12 from '
         'the sharpen launch or from sharpen-to-BGR plus risp_bgr8_to_nv12   (c) serve_sh / serve / serve_torch: net.serve(raw, out=) '
         'with sharpen, without, and followed by the same filter from torch ops; host side included; no counters were read')
    net = SB.pipeline(ARCH)
    rows = []
    rows += measure(net, (64, 256, 256), None, 10, args.reps, args.rounds, emit)
    rows += measure(net, (1, 3000, 4000), None, 20, max(20, args.reps // 3), args.rounds, emit)
    rows += measure(net, (1, 3000, 4000), ((1080, 1920), (375, 0, 2250, 4000)), 20, max(20, args.reps // 3), args.rounds, emit)
    emit('the fused NV12 store beats two launches by more than the spread in %d of %d rows' % (sum(rows), len(rows)))
    emit(SB.verdict_line('_SHARPEN_NV12_FUSED', ['nv12'] if all(rows) else []))
    emit("pipeline_fusion.sharpen_store('nv12') answers %r" % PF.sharpen_store('nv12'))
    emit.write()


if __name__ == '__main__':
    main()
