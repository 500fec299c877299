#!/usr/bin/env python3
"""GPU box: a full sensor frame through a tiled pipeline, uint16 mosaic in, packed 8-bit image out - the serving route
(serve_frame: raw_crops on the mosaic -> the forward on tile slices -> risp_tile_blend_u8) against the same result from the
pieces that existed before it, in interleaved rounds in one process.

    python tools/bench_serve_frame.py [--out profiles/serve_frame.txt] [--rounds 7] [--reps 10]

The pipeline is BASELINE config 5: IspUniversal Bayer_01_Demosaic_02_sRGB_13 (Path-Restore, the demosaic proxy, WbQuadratic)
on one 3000 x 4000 frame, tiles 512 / 480 (63 of them), 21 tiles per forward.  Legs, host side included (what a caller pays),
timed between two device events (leg c ends on the host, so its second event follows the host conversion):
  a  serve_frame    net.serve_frame(raw, out=buf)
  b  composed       whole-frame raw_crops -> gather_tiles -> the same forward -> blend_tiles -> quantise_u8(out=buf)
  c  test_split     run_frame on the resident fp32 frame raw / white, then test_split.py's host conversion (D2H of the
                    (3,H,W) fp32 blend, numpy clip / x 255 / truncate)
Each round times every leg once (REPS calls after 2 warm ones; leg c a third of them); per leg: the rounds, median, minimum and
spread - the spread between the rounds of ONE leg is the noise a difference between two legs has to clear.  The bytes of the
three legs are compared first.

The blend step alone, on a random stack of the same geometry: risp_tile_blend_u8 against risp_tile_blend + risp_quantise_u8
into a preallocated fp32 frame, the same way.  Bytes are algorithmic counts from the shapes (the forward is the same in every
leg and is left out)."""
import contextlib
import io
from collections import OrderedDict

import numpy as np
import torch

import serve_bench as SB
import reconfigisp_amd.functional as F
from reconfigisp_amd import lib as L
from reconfigisp_amd.codes.data.gpu_input import raw_crops
from reconfigisp_amd.codes.models import create_model
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
from reconfigisp_amd.codes.test_split import run_frame
from reconfigisp_amd.codes.utils.util_path_restore import blend_tiles, gather_tiles, tile_grid

WHITE = 1023.0
ARCH = 'Bayer_01_Demosaic_02_sRGB_13'
H, W = 3000, 4000
SIZE, STRIDE, TILE_BATCH = (512, 512), (480, 480), 21


def model():
    opt = OrderedDict(model='isp', gpu_ids=[0], dist=False, is_train=False,
                      network_G=dict(which_model_G='IspUniversal', architecture=ARCH, individual_module_paths=[None] * 3,
                                     module_path=None),
                      path=dict(pretrain_model_G=None, strict_load=True))
    torch.manual_seed(10)
    m = create_model(opt)
    m.netG.cuda().eval()
    return m


def rounds_of(legs, reps, rounds):
    """two warm calls per leg and round, as the recorded profile was measured"""
    return SB.rounds_of(legs, reps, rounds, False, lambda fn, n: SB.timed(fn, n, warm=2))


def report(res, bytes_moved, emit, rate):
    """``rate``: the legs are nothing but those bytes (the blend step alone), so bytes over time is a rate worth printing"""
    med = {}
    for name, v in res.items():
        med[name] = SB.median(v)
        rounds_line, stats_line = SB.leg_lines(name, v, 13, '%.0f')
        emit(rounds_line)
        emit(stats_line + '   %.0f MB %s' % (
            bytes_moved[name] / 1e6,
            ': %.2f TB/s' % (bytes_moved[name] / (med[name] * 1e-6) / 1e12) if rate else 'at its two ends (the forward not counted)'))
    return med


def main():
    args = SB.parser(10, 7).parse_args()
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    m = model()
    net = m.netG
    raw = SB.frames_u16(1, H, W, 20, WHITE)[0]                                                    # (H,W) uint16
    frame32 = torch.from_numpy(raw.cpu().to(torch.int32).numpy().astype(np.float32) / np.float32(WHITE))[None, None].cuda()
    pos = tile_grid(H, W, SIZE, STRIDE)
    pos_dev = torch.from_numpy(pos).cuda()
    count = len(pos)
    sel0 = torch.zeros((1, 3), device='cuda', dtype=torch.int32)
    buf = {k: torch.empty((H, W, 3), device='cuda', dtype=torch.uint8) for k in 'ab'}
    host = {}

    def serve_frame():
        net.serve_frame(raw, WHITE, SIZE, STRIDE, TILE_BATCH, out=buf['a'])

    def composed():
        with torch.no_grad():
            frame = raw_crops(raw[None], sel0, (H, W), WHITE)
            tiles = gather_tiles(frame[0], pos, SIZE)
            stack = torch.empty((count, 3) + SIZE, device='cuda', dtype=torch.float32)
            pars = net._stage_params(min(TILE_BATCH, count))
            for at in range(0, count, TILE_BATCH):
                chunk, dest = tiles[at:at + TILE_BATCH], stack[at:at + TILE_BATCH]
                y, _ = PF.fused_forward(net.all_modules, [p[:chunk.shape[0]] if p is not None and p.dim() == 2 else p for p in pars],
                                        chunk, dest)
                if y.data_ptr() != dest.data_ptr():
                    dest.copy_(y)
            F.quantise_u8(blend_tiles(stack, pos, (H, W), STRIDE)[None], out=buf['b'][None])

    def test_split():
        merged = run_frame(m, frame32, SIZE, STRIDE, TILE_BATCH)
        host['c'] = (np.clip(merged[0].permute(1, 2, 0).cpu().numpy(), 0, 1) * 255.).astype(np.uint8)

    def test_split_quiet():                                 # run_frame prints the tile count on every call
        with contextlib.redirect_stdout(io.StringIO()):
            test_split()

    legs = OrderedDict([('a serve_frame', serve_frame), ('b composed', composed), ('c test_split', test_split_quiet)])
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    assert net.last_serve_route == 'tiled'
    assert torch.equal(buf['a'], buf['b']), 'serve_frame and the composed route disagree'
    assert np.array_equal(buf['a'].cpu().numpy(), host['c']), 'serve_frame and run_frame + host conversion disagree'
    emit('%s, %d x %d, tiles %d / %d (%d), %d per forward: the bytes of the three legs agree (%d distinct values)' % (
        ARCH, H, W, SIZE[0], STRIDE[0], count, TILE_BATCH, len(torch.unique(buf['a']))))

    px, tile_px = H * W, count * SIZE[0] * SIZE[1]
    back_u8 = tile_px * 12 + px * 3                          # the stack read, the image written
    back_two = tile_px * 12 + px * 12 + px * 12 + px * 3     # ... the fp32 frame written and read between
    ends = {'a serve_frame': tile_px * 2 + tile_px * 4 + back_u8,
            'b composed': px * 2 + px * 4 + tile_px * 4 + tile_px * 4 + back_two,
            'c test_split': tile_px * 4 + tile_px * 4 + tile_px * 12 + px * 12 + px * 12}      # gather, blend, D2H
    reps = {'a serve_frame': args.reps, 'b composed': args.reps, 'c test_split': max(2, args.reps // 3)}
    emit(' whole frame, %d calls per round (c: %d); us per call' % (args.reps, reps['c test_split']))
    med = report(rounds_of(legs, reps, args.rounds), ends, emit, False)
    emit('  a / b = %.3f   a / c = %.3f' % (med['a serve_frame'] / med['b composed'], med['a serve_frame'] / med['c test_split']))

    g = torch.Generator().manual_seed(5)
    stack = torch.rand((count, 3) + SIZE, generator=g).cuda()
    frame = torch.empty((3, H, W), device='cuda', dtype=torch.float32)
    eh, ew = (SIZE[0] - STRIDE[0]) // 2, (SIZE[1] - STRIDE[1]) // 2

    def blend_u8():
        F.tile_blend_u8(stack, pos_dev, (H, W), STRIDE, out=buf['a'])

    def blend_then_quantise():
        L.call('risp_tile_blend', F._p(stack), F._p(frame), F._p(pos_dev), count, 3, H, W, SIZE[0], SIZE[1], eh, ew, F._stream())
        L.call('risp_quantise_u8', F._p(frame), F._p(buf['b']), 1, 3, H, W, 0, F._stream())

    blend_u8()
    blend_then_quantise()
    torch.cuda.synchronize()
    assert torch.equal(buf['a'], buf['b']), 'risp_tile_blend_u8 and risp_tile_blend + risp_quantise_u8 disagree'
    steps = OrderedDict([('blend_u8', blend_u8), ('blend+quant', blend_then_quantise)])
    emit(' the blend step alone, random (%d,3,%d,%d) stack, %d calls per round; us per call' % (count, SIZE[0], SIZE[1], 5 * args.reps))
    med = report(rounds_of(steps, {k: 5 * args.reps for k in steps}, args.rounds), {'blend_u8': back_u8, 'blend+quant': back_two}, emit, True)
    emit('  blend_u8 / blend+quant = %.3f' % (med['blend_u8'] / med['blend+quant']))
    emit.write()


if __name__ == '__main__':
    main()
