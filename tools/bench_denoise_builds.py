#!/usr/bin/env python3
"""GPU box: the tile launches alone - serve_denoise_u8, serve_denoise_scene_u8, serve_denoise_stats, serve_median_u8 - in several
builds of the library, in interleaved rounds in one process: the parent commit's kernels beside the tree's, or any variant given
as a build.

    make -C reconfigisp_amd/csrc OUT=/tmp/parent/libreconfigisp_hip.so OBJDIR=/tmp/parent      (in a checkout of the parent)
    python tools/bench_denoise_builds.py parent=/tmp/parent/libreconfigisp_hip.so [--out FILE]

Leg `tree` is the in-tree library; every NAME=PATH adds a leg with that build's entry point bound to the same signature.  Each
call goes through its functional wrapper, host side included, with the arguments net.serve itself passes to it (recorded from one
call of the route) for the pipelines of tools/bench_serve_denoise.py, _denoise_scene.py and _median.py with the bilinear demosaic:

  serve_denoise_u8         Demosaic_02_sRGB_11_NN_01_14, NN the bilateral (07), the median (08, 3 x 3) and non-local means (09)
  serve_denoise_scene_u8   Demosaic_02_sRGB_05_NN_06_01: gray-world's gain in front of the denoiser, white-world's behind it
  serve_denoise_stats      the statistics launch of that white-world stage, with SCENE_MEAN3 and with SCENE_MAX3
  serve_median_u8          Demosaic_02_sRGB_11_08_01 at K = 5, 9, 15

on 64 x 256 x 256 and 1 x 3000 x 4000 resident uint16 frames.  All builds read and fill the same buffers, and their results are
compared before anything is timed; 7 rounds after one that is not kept.  Per row and build the rule of tools/serve_bench.py says
whether that build beats the tree."""
import torch

import serve_bench as SB
import reconfigisp_amd.functional as F
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
from bench_serve_denoise import DENOISERS, WHITE

MEDIAN_K = (5, 9, 15)
ENTRY = {'serve_denoise_u8': 'risp_serve_denoise_u8', 'serve_denoise_scene_u8': 'risp_serve_denoise_scene_u8',
         'serve_denoise_stats': 'risp_serve_denoise_stats', 'serve_median_u8': 'risp_serve_median_u8'}


def recorded(net, raw, **keyword):
    """{wrapper: its positional arguments} for the wrappers of ENTRY that one net.serve(raw, **keyword) calls (the last call of
    each; a list is copied as it was at the call)"""
    calls, saved = {}, {name: getattr(F, name) for name in ENTRY}

    def recorder(name):
        def call(*args):
            calls[name] = [list(a) if isinstance(a, list) else a for a in args]
            return saved[name](*args)
        return call

    try:
        for name in ENTRY:
            setattr(F, name, recorder(name))
        net.serve(raw, WHITE, **keyword)
    finally:
        for name, fn in saved.items():
            setattr(F, name, fn)
    torch.cuda.synchronize()
    return calls


def legs(raw):
    """(row, wrapper, leg, out) for every measured call on ``raw``"""
    n, h, w = raw.shape
    out = torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8)
    partials = torch.empty((n, F.serve_scene_groups(h, w), 4), device='cuda', dtype=torch.float32)

    def image(name, args):                                      # (.., reverse_channels, out, black_level, cfa)
        args = args[:10] + [out] + args[11:]
        return lambda: getattr(F, name)(*args)

    for den, code in DENOISERS:
        net = SB.pipeline('Demosaic_02_sRGB_11_%02d_01_14' % code, median=SB.MEDIAN_3X3)
        yield 'serve_denoise_u8 %s' % den, 'serve_denoise_u8', image('serve_denoise_u8', recorded(net, raw, fast_denoise=True)['serve_denoise_u8']), out
    for den, code in DENOISERS:
        net = SB.pipeline('Demosaic_02_sRGB_05_%02d_06_01' % code, median=SB.MEDIAN_3X3)
        calls = recorded(net, raw, fast_denoise_scene=True)
        args = calls['serve_denoise_scene_u8']
        assert F.OP_GAIN3_Q8 in args[7], args[7]
        yield 'serve_denoise_scene_u8 %s' % den, 'serve_denoise_scene_u8', image('serve_denoise_scene_u8', args), out
        args = calls['serve_denoise_stats']                     # (.., post_ops, post_params, stat, partials, black_level, cfa)
        for stat, which in ((F.SCENE_MEAN3, 'mean'), (F.SCENE_MAX3, 'max')):
            yield ('serve_denoise_stats %s %s' % (den, which), 'serve_denoise_stats',
                   lambda a=args[:9] + [stat, partials] + args[11:]: F.serve_denoise_stats(*a), partials)
    for k in MEDIAN_K:
        p = ((k - 3) // 2 + 0.5) / 7                            # the middle of the parameter range that gives size k
        net = SB.pipeline('Demosaic_02_sRGB_11_08_01', median=float(torch.logit(torch.tensor(p))))
        args = recorded(net, raw, fast_median=True)['serve_median_u8']      # (.., size, post_ops, post_params, reverse_channels, out, ..)
        assert args[5] == k, args[5]
        args = args[:9] + [out] + args[10:]
        yield 'serve_median_u8 K = %d' % k, 'serve_median_u8', lambda a=args: F.serve_median_u8(*a), out


def main():
    ap = SB.parser(100, 7)
    ap.add_argument('builds', nargs='*', help='NAME=PATH of another build of libreconfigisp_hip.so')
    args = ap.parse_args()
    builds = SB.load_builds(args.builds, tuple(ENTRY.values()))
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args, ' ' + ' '.join(n for n in builds if n != 'tree')))
    PF._DENOISE_SCENE_SLOWER = frozenset()                     # every denoiser takes the denoise + scene route here
    PF._MEDIAN_SIZES = frozenset(F.MEDIAN_SIZES)
    beaten = []
    for (n, h, w), seed, reps in (((64, 256, 256), 10, args.reps), ((1, 3000, 4000), 20, max(10, args.reps // 3))):
        raw = SB.frames_u16(n, h, w, seed, WHITE)
        for row, wrapper, leg, out in legs(raw):
            row = '%s, %d x %d x %d' % (row, n, h, w)
            beaten += ['%s by %s' % (row, name) for name in SB.compare_builds(emit, row, builds, ENTRY[wrapper], leg, (out,), reps, args.rounds)]
    emit(SB.beaten_line(beaten))
    emit.write()


if __name__ == '__main__':
    main()
