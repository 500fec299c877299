#!/usr/bin/env python3
"""GPU box: the four output-stage calls alone - bgr8_resize, bgr8_sharpen, bgr8_warp, bgr8_to_nv12 - in several builds of the
library, in interleaved rounds in one process: the parent commit's kernels beside the tree's, or any variant given as a build.

    make -C reconfigisp_amd/csrc OUT=/tmp/parent/libreconfigisp_hip.so OBJDIR=/tmp/parent      (in a checkout of the parent)
    python tools/bench_output_builds.py parent=/tmp/parent/libreconfigisp_hip.so [--out FILE]

Leg `tree` is the in-tree library; every NAME=PATH adds a leg with that build's entry point bound to the same signature.  Each
call goes through its functional wrapper, host side included, with the parameters of leg (a) of tools/bench_serve_resize.py /
_sharpen / _warp (the rotation mesh, both kernels, both stages) / _nv12 on the image the classical route serves: 64 x 256 x 256
and 1 x 3000 x 4000, packed out and NV12 out where the call has it, all buffers 4-byte aligned (`aligned`) and the images and a
packed out one byte into their allocations (`+1`; an NV12 out stays aligned).  One more row: bgr8_resize into NV12 with
OW % 4 == 2, where the store of a patch takes its narrow form.  All builds read and fill the same buffers, and their results are
compared before anything is timed; 7 rounds after one that is not kept.  Per row and build the rule of tools/serve_bench.py says
whether that build beats the tree."""
import torch

import serve_bench as SB
import reconfigisp_amd.functional as F
from bench_serve_resize import ARCH, BLACK, MATRIX, WHITE
from bench_serve_sharpen import AMOUNT, LIMIT, THRESHOLD
from bench_serve_warp import CELL, meshes

# per frame height: (out_size, out_window) of tools/bench_serve_resize.py
RESIZE = {3000: ((1080, 1920), (375, 0, 2250, 4000)), 256: ((128, 128), None)}


def placed(shape, off, src=None):
    """a contiguous uint8 device view ``off`` bytes into its allocation, holding ``src`` when given"""
    count = int(torch.Size(shape).numel())
    view = torch.zeros(count + 4, device='cuda', dtype=torch.uint8)[off:off + count].view(shape)
    assert view.data_ptr() % 4 == off
    return view if src is None else view.copy_(src)


def legs(img, off, narrow=False):
    """(row, entry, leg, out) for every measured call on ``img``; ``narrow``: the one row of the narrow NV12 store instead"""
    n, h, w = img.shape[:3]
    size, window = RESIZE[h]
    if narrow:
        size = (size[0], size[1] + 2)
        out = placed((n, size[0] * 3 // 2, size[1]), 0)
        yield 'resize to OW = 2 mod 4 -> nv12', 'risp_bgr8_resize', lambda: F.bgr8_resize(img, size, window, 'triangle', nv12=MATRIX, out=out), out
        return
    bgr, nv = (lambda oh, ow: placed((n, oh, ow, 3), off)), (lambda oh, ow: placed((n, oh * 3 // 2, ow), 0))
    out_b, out_n = bgr(*size), nv(*size)
    yield 'resize -> bgr', 'risp_bgr8_resize', lambda: F.bgr8_resize(img, size, window, 'triangle', out=out_b), out_b
    yield 'resize -> nv12', 'risp_bgr8_resize', lambda: F.bgr8_resize(img, size, window, 'triangle', nv12=MATRIX, out=out_n), out_n
    out_s, out_sn = bgr(h, w), nv(h, w)
    for r in F.SHARPEN_RADII:
        sharp = (AMOUNT, THRESHOLD, LIMIT, r)
        yield 'sharpen r%d -> bgr' % r, 'risp_bgr8_sharpen', lambda sharp=sharp: F.bgr8_sharpen(img, sharp, out=out_s), out_s
        yield ('sharpen r%d -> nv12' % r, 'risp_bgr8_sharpen', lambda sharp=sharp: F.bgr8_sharpen(img, sharp, nv12=MATRIX, out=out_sn),
               out_sn)
    mesh = meshes(h, w)['rotate2']
    for k in F.WARP_KERNELS:
        for stage in (0, 1):
            yield ('warp %s s%d -> bgr' % (k, stage), 'risp_bgr8_warp',
                   lambda k=k, stage=stage: F.bgr8_warp(img, (mesh, CELL, (h, w), k), out=out_s, stage=stage), out_s)
    yield 'to_nv12', 'risp_bgr8_to_nv12', lambda: F.bgr8_to_nv12(img, MATRIX, out=out_sn), out_sn


def main():
    ap = SB.parser(300, 7)
    ap.add_argument('builds', nargs='*', help='NAME=PATH of another build of libreconfigisp_hip.so')
    args = ap.parse_args()
    builds = SB.load_builds(args.builds, ('risp_bgr8_resize', 'risp_bgr8_sharpen', 'risp_bgr8_warp', 'risp_bgr8_to_nv12'))
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args, ' ' + ' '.join(n for n in builds if n != 'tree')))
    net = SB.pipeline(ARCH)
    beaten = []
    for (n, h, w), seed, reps in (((64, 256, 256), 10, args.reps), ((1, 3000, 4000), 20, max(20, args.reps // 3))):
        raw = (SB.frames_int(n, h, w, seed, int(WHITE) - BLACK) + BLACK).to(torch.uint16).cuda()
        served = net.serve(raw, WHITE, black_level=BLACK)
        for off, narrow in ((0, False), (1, False)) + (((0, True),) if h == 256 else ()):
            img = placed(served.shape, off, served)
            for row, entry, leg, out in legs(img, off, narrow):
                row = '%s, %s, %d x %d x %d' % (row, '+1' if off else 'aligned', n, h, w)
                beaten += ['%s by %s' % (row, name) for name in SB.compare_builds(emit, row, builds, entry, leg, (out,), reps, args.rounds)]
    emit(SB.beaten_line(beaten))
    emit.write()


if __name__ == '__main__':
    main()
