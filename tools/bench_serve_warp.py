#!/usr/bin/env python3
"""GPU box: a geometry-corrected output of the serving path - what the mesh-warp launch costs, whether staging a tile's source
box in LDS (stage 1) beats sampling global memory (stage 0), and what a served call pays and saves; on resident frames, in
interleaved rounds in one process.

    python tools/bench_serve_warp.py [--out profiles/serve_warp.txt] [--reps 300] [--rounds 7]

Pipeline (OriginUniversal, route 'classical'): Demosaic_02_sRGB_11_01_14 (bilinear, WbManual, Gamma, GtmManual), black level 64,
white level 1023.  Sizes: one 3000 x 4000 frame and 64 x 256 x 256 frames, warped to their own size with cells of 64 pixels.
Meshes: the identity, a rotation by 2 degrees about the middle, a radial correction (k1 = -0.12, zoom 0.94).  The launch legs run
on the packed image the pipeline serves for those frames.  Legs, host side included (what a caller pays), timed between two
device events:
  (a) K_M_s0 / K_M_s1   functional.bgr8_warp(img, (mesh M, 64, size, K), out=, stage=0 / 1), K = bilinear, bicubic: 3 bytes per
                        pixel read once and 3 written once
      resize_K          functional.bgr8_resize(img, size, None, K, out=) at the same sizes (one tap per axis for triangle, the
                        bicubic taps of an output that falls on its sample): the scaler's launch beside the warp's
  (b) serve_warp        net.serve(raw, out=, warp=) with the rotation, bilinear: what a user pays with the feature
      serve             the same call without the keyword
      serve_grid        serve, then torch.nn.functional.grid_sample(mode='bilinear', padding_mode='border', align_corners=True)
                        on a per-pixel grid kept on the device, with its two conversions (to float planes and back to packed
                        bytes): time only, its bytes differ
Each round times every leg once (REPS calls, after 3 warm ones), after one round that is not kept; per leg: the rounds, median,
minimum and spread - the spread between the rounds of ONE leg is the noise a difference between two legs has to clear.  The bytes
of stage 0 and stage 1 are compared first.  Row verdict: stage 1 beats stage 0 when median(s0) - median(s1) exceeds the larger of
the two spreads; a kernel enters pipeline_fusion._WARP_STAGED only if that holds in all of its six rows (two sizes x three
meshes), and the line `verdict: _WARP_STAGED = ...` says so (tests/test_warp_reference_cpu.py compares it with the table).  Bytes
are algorithmic counts, the rate is those bytes over the median time.  With RISP_HIP_LIBRARY set the rows are those of that build
(profiles/serve_warp_lds.txt: a build whose stage = 1 launch asks for 16 KB of LDS, make EXTRA=-DRISP_WARP_AB_LDS=16384)."""
import math
import os

import torch

import serve_bench as SB
import reconfigisp_amd.functional as F
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF

ARCH = 'Demosaic_02_sRGB_11_01_14'
WHITE, BLACK = 1023.0, 64
CELL = 64
MESHES = ('identity', 'rotate2', 'radial')


def meshes(h, w):
    a, cy, cx = math.radians(2.0), (h - 1) / 2.0, (w - 1) / 2.0
    c, s = math.cos(a), math.sin(a)
    # output (x, y, 1) -> source (x, y): a rotation about the middle
    rot = [[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0.0, 0.0, 1.0]]
    return {'identity': F.warp_homography([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], (h, w), CELL).cuda(),
            'rotate2': F.warp_homography(rot, (h, w), CELL).cuda(),
            'radial': F.warp_radial(h, w, (h, w), CELL, -0.12, zoom=0.94).cuda()}


def measure(net, shape, seed, reps, rounds, emit):
    n, h, w = shape
    raw = (SB.frames_int(n, h, w, seed, int(WHITE) - BLACK) + BLACK).to(torch.uint16).cuda()
    img = net.serve(raw, WHITE, black_level=BLACK).clone()
    assert net.last_serve_route == 'classical'
    u8 = lambda *s: torch.empty(s, device='cuda', dtype=torch.uint8)
    out_a, out_b, out_s, out_full = u8(n, h, w, 3), u8(n, h, w, 3), u8(n, h, w, 3), u8(n, h, w, 3)
    mesh = meshes(h, w)
    both = 2.0 * n * h * w * 3
    legs, nbytes = {}, {}
    for k in F.WARP_KERNELS:
        for m in MESHES:
            for stage in (0, 1):
                name = '%s_%s_s%d' % (k, m, stage)
                legs[name] = lambda k=k, m=m, stage=stage: F.bgr8_warp(img, (mesh[m], CELL, (h, w), k), out=out_a, stage=stage)
                nbytes[name] = both
    for k in ('triangle', 'bicubic'):
        legs['resize_' + k] = lambda k=k: F.bgr8_resize(img, (h, w), None, k, out=out_b)
        nbytes['resize_' + k] = both
    serve_warp = (mesh['rotate2'], CELL, (h, w), 'bilinear')
    # the grid of grid_sample from the same map, per pixel, normalised to -1 .. 1 (align_corners=True)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    a, cy, cx = math.radians(2.0), (h - 1) / 2.0, (w - 1) / 2.0
    sx = cx + math.cos(a) * (xs - cx) - math.sin(a) * (ys - cy)
    sy = cy + math.sin(a) * (xs - cx) + math.cos(a) * (ys - cy)
    grid = torch.stack([sx / (w - 1) * 2 - 1, sy / (h - 1) * 2 - 1], dim=-1)[None].expand(n, h, w, 2).contiguous().cuda()

    def leg_serve_warp():
        net.serve(raw, WHITE, out=out_s, black_level=BLACK, warp=serve_warp)

    def leg_serve():
        net.serve(raw, WHITE, out=out_full, black_level=BLACK)

    def leg_serve_grid():
        full = net.serve(raw, WHITE, out=out_full, black_level=BLACK)
        planes = torch.nn.functional.grid_sample(full.permute(0, 3, 1, 2).float(), grid, mode='bilinear', padding_mode='border',
                                                 align_corners=True)
        return planes.round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    legs.update(serve_warp=leg_serve_warp, serve=leg_serve, serve_grid=leg_serve_grid)
    nbytes.update(serve_warp=n * h * w * (2.0 + 3.0) + both, serve=n * h * w * (2.0 + 3.0), serve_grid=None)
    for k in F.WARP_KERNELS:
        for m in MESHES:
            legs['%s_%s_s0' % (k, m)]()
            first = out_a.clone()
            legs['%s_%s_s1' % (k, m)]()
            torch.cuda.synchronize()
            assert torch.equal(first, out_a), 'stage 0 and stage 1 disagree (%s, %s)' % (k, m)
            if m == 'identity':
                assert torch.equal(out_a, img), 'the identity mesh does not return the image (%s)' % k
    leg_serve_warp()
    assert net.last_serve_warp == 'pass' and torch.equal(out_s, F.bgr8_warp(img, serve_warp))
    theirs = leg_serve_grid()
    diff = (theirs.int() - out_s.int()).abs()
    assert len(torch.unique(out_s)) > 32
    res = SB.rounds_of(legs, reps, rounds, True)
    med = {k: SB.median(v) for k, v in res.items()}
    emit(' %s, %d x %d x %d -> the same size, cell %d, %d calls per round; us per call; grid_sample differs from serve_warp in '
         '%.1f %% of the bytes, by at most %d' % (ARCH, n, h, w, CELL, reps, 100 * (diff > 0).float().mean().item(), diff.max().item()))
    for name, v in res.items():
        rounds_line, line = SB.leg_lines(name, v, 22)
        emit(rounds_line)
        if nbytes[name] is not None:
            line += '   %.1f MB: %s' % (nbytes[name] / 1e6, SB.hbm_share(nbytes[name], med[name]))
        emit(line)
    won = {k: [] for k in F.WARP_KERNELS}
    for k in F.WARP_KERNELS:
        for m in MESHES:
            s0, s1 = '%s_%s_s0' % (k, m), '%s_%s_s1' % (k, m)
            gain, noise = SB.margin(res[s1], res[s0])
            won[k].append(SB.beats(res[s1], res[s0]))
            emit('  (a) %-8s %-8s s0 - s1 = %.1f us against a spread of %.1f us: staging %s   s1 / s0 = %.3f;  against resize_%s: '
                 's0 %.2f x, s1 %.2f x' % (k, m, gain, noise, 'BEATS the gather' if won[k][-1] else 'does NOT beat the gather',
                                           med[s1] / med[s0], 'triangle' if k == 'bilinear' else 'bicubic',
                                           med[s0] / med['resize_' + ('triangle' if k == 'bilinear' else 'bicubic')],
                                           med[s1] / med['resize_' + ('triangle' if k == 'bilinear' else 'bicubic')]))
    emit('  (b) serve_warp - serve = %.1f us: serve_warp / serve = %.3f;  serve_grid - serve = %.1f us: serve_warp / serve_grid = %.3f   '
         '(%.0f MPix/s of sensor with the warp)' % (med['serve_warp'] - med['serve'], med['serve_warp'] / med['serve'],
                                                    med['serve_grid'] - med['serve'], med['serve_warp'] / med['serve_grid'],
                                                    n * h * w / med['serve_warp']))
    return won


def main():
    args = SB.parser(300, 7).parse_args()
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    if os.environ.get('RISP_HIP_LIBRARY'):                  # an ablation build (make EXTRA=-DRISP_WARP_AB_LDS=..): its rows, not the library's
        emit('RISP_HIP_LIBRARY=%s %s' % (os.environ['RISP_HIP_LIBRARY'], os.environ.get('RISP_BENCH_NOTE', '')))
    emit('(a) K_M_s0 / K_M_s1: the warp launch alone, sampling global memory or the staged box; resize_K: the resize launch at the '
         'same sizes   (b) serve_warp / serve / serve_grid: net.serve(raw, out=) with warp, without, and followed by '
         'torch.nn.functional.grid_sample; host side included')
    net = SB.pipeline(ARCH)
    rows = {k: [] for k in F.WARP_KERNELS}
    for shape, seed, reps in (((1, 3000, 4000), 20, max(20, args.reps // 3)), ((64, 256, 256), 10, args.reps)):
        for k, v in measure(net, shape, seed, reps, args.rounds, emit).items():
            rows[k] += v
    for k in F.WARP_KERNELS:
        emit('%s: staging beats the gather by more than the spread in %d of %d rows' % (k, sum(rows[k]), len(rows[k])))
    emit(SB.verdict_line('_WARP_STAGED', [k for k in F.WARP_KERNELS if all(rows[k])]))
    emit('pipeline_fusion.warp_stage answers %s' % ', '.join('%s: %r' % (k, PF.warp_stage(k)) for k in F.WARP_KERNELS))
    emit.write()


if __name__ == '__main__':
    main()
