#!/usr/bin/env python3
"""GPU box: the 3A statistics of the sensor frame - what the launch costs beside the project's streaming yardstick for these
inputs, what the keyword costs a served call, and what the same numbers cost composed from torch ops; on resident frames, in
interleaved rounds in one process.

    python tools/bench_serve_stats.py [--out profiles/serve_stats.txt] [--reps 300] [--rounds 7] [--variant NAME=LIB.so ...]

Pipeline (OriginUniversal, route 'classical'): Demosaic_02_sRGB_11_01_14 (bilinear, WbManual, Gamma, GtmManual); 64 x 256 x 256
with zones of 32 x 32 and one 3000 x 4000 frame with zones of 200 x 200; formats u16 / raw10 / raw12 holding the same 10-bit
samples, black level 64, white level 1023; 256 bins of four codes, lo 16, hi 900.  Legs, host side included (what a caller pays),
timed between two device events:
  stats      functional.raw_stats(raw, st, 64): the memset and the launch, bits / 8 bytes per pixel read once
  direct     risp_raw_stats of the in-tree library through ctypes, without functional.raw_stats's checks (only with --variant)
  NAME       the same ctypes call into another build of the library (--variant: builds with make EXTRA=-DRISP_STATS_MAX_TH=.. /
             -DRISP_STATS_MIN_TILES=.. / -DRISP_STATS_MAX_COPIES=.. for the accumulation forms), same arguments, same rounds; a
             build is judged against `direct`, the same host path
  shade      functional.raw_shade(raw, out=) alone from the same format: bits / 8 read and 2 written per pixel
  serve_st   net.serve(raw, out=, statistics=st): what a user pays with the keyword
  serve      the same call without it
  torch      the same statistics composed from torch ops on the unpacked uint16 frames (already unpacked: the unpacking is not
             timed); its result is compared with the launch's first
With --variant a third input, 4 x 3000 x 4000 (3008 tiles of 64 rows), is timed for the launch legs alone.
Each round times every leg once (REPS calls, the torch leg REPS / 10, after 3 warm ones), after one round that is not kept; per
leg: the rounds, median, minimum and spread.  Bytes are algorithmic counts, the rate is those bytes over the median time."""
import torch

import serve_bench as SB
import reconfigisp_amd.functional as F
from reconfigisp_amd import lib as L

ARCH = 'Demosaic_02_sRGB_11_01_14'
FORMATS = ['u16', 'raw10', 'raw12']
WHITE, BLACK, CELL = 1023.0, 64, 64
BINS, SHIFT, LO, HI = 256, 2, 16, 900


def torch_stats(x, zone):
    """(zones (N,ZH,ZW,4,3) int64, hist (N,4,BINS) int32) of (N,H,W) uint16 frames whose size the zones divide"""
    n, h, w = x.shape
    zh, zw = zone[0] // 2, zone[1] // 2
    s = (x.to(torch.int32) - BLACK).clamp_(min=0)
    zones, hist = [], []
    for c in range(4):
        p = s[:, c >> 1::2, c & 1::2]
        inside = (p >= LO) & (p <= HI)
        focus = torch.zeros_like(p)
        focus[:, :, 1:-1] = (2 * p[:, :, 1:-1] - p[:, :, :-2] - p[:, :, 2:]).abs()
        per = [t.view(n, h // 2 // zh, zh, w // 2 // zw, zw).sum(dim=(2, 4), dtype=torch.int64) for t in (p * inside, inside, focus)]
        zones.append(torch.stack(per, dim=-1))
        key = (p >> SHIFT).clamp_(max=BINS - 1).view(n, -1) + BINS * torch.arange(n, device=x.device, dtype=torch.int32)[:, None]
        hist.append(torch.bincount(key.view(-1), minlength=n * BINS).view(n, BINS).to(torch.int32))
    return torch.stack(zones, dim=3), torch.stack(hist, dim=1)


def measure(net, shape, zone, seed, fmt, reps, rounds, variants, emit, launch_only=False):
    n, h, w = shape
    pix = n * h * w
    bits = F.RAW_FORMAT[fmt] or 16
    x = SB.frames_int(n, h, w, seed, int(WHITE) - BLACK) + BLACK
    x16 = x.to(torch.uint16).cuda()
    raw = x16 if fmt == 'u16' else SB.pack(x, bits).cuda()
    fkw = {} if fmt == 'u16' else dict(raw_format=fmt, raw_width=w)
    shading = (F.shading_map(SB.vignette(h, w), h, w, CELL).cuda(), CELL)
    st = F.raw_statistics(n, h, w, zone=zone, bins=BINS, hist_shift=SHIFT, lo=LO, hi=HI)
    others = {name: F.raw_statistics(n, h, w, zone=zone, bins=BINS, hist_shift=SHIFT, lo=LO, hi=HI) for name in variants}
    out_a, out_b = (torch.empty((1 if launch_only else n, h, w, 3), device='cuda', dtype=torch.uint8) for _ in range(2))
    u16 = torch.empty((n, h, w), device='cuda', dtype=torch.uint16)
    stride = raw.shape[-1] * raw.element_size()
    bpp = {'stats': bits / 8, 'shade': bits / 8 + 2.0, 'serve_st': 2 * bits / 8 + 3.0, 'serve': bits / 8 + 3.0, 'torch': 2.0}

    def leg_stats():
        F.raw_stats(raw, st, BLACK, bits, w)

    def leg_variant(name):
        fn, o = variants[name], others[name]

        def leg():
            assert fn(F._p(raw), bits, stride, BLACK, F._p(o.zones), F._p(o.hist), zone[0], zone[1], BINS, SHIFT, LO, HI, n, h, w,
                      F._stream()) == 0
        return leg

    def leg_shade():
        F.raw_shade(raw, shading, BLACK, bits, w, out=u16)

    def leg_serve_st():
        net.serve(raw, WHITE, out=out_a, black_level=BLACK, statistics=st, **fkw)

    def leg_serve():
        net.serve(raw, WHITE, out=out_b, black_level=BLACK, **fkw)

    def leg_torch():
        torch_stats(x16, zone)

    legs = {'stats': leg_stats}
    for name in variants:
        legs[name] = leg_variant(name)
        bpp[name] = bits / 8
    if not launch_only:
        legs.update(shade=leg_shade, serve_st=leg_serve_st, serve=leg_serve, torch=leg_torch)
    leg_stats()
    if not launch_only:
        leg_serve_st(), leg_serve()
        assert net.last_serve_route == 'classical'
    for name in variants:
        legs[name]()
    tz, th = torch_stats(x16, zone)
    torch.cuda.synchronize()
    assert launch_only or torch.equal(out_a, out_b), 'the keyword changed the image'
    assert torch.equal(tz, st.zones) and torch.equal(th, st.hist), 'torch and the launch disagree'
    for name, o in others.items():
        assert torch.equal(o.zones, st.zones) and torch.equal(o.hist, st.hist), 'build %s disagrees' % name
    res = SB.rounds_of(legs, {name: max(3, reps // 10) if name == 'torch' else reps for name in legs}, rounds, True)
    med = {k: SB.median(v) for k, v in res.items()}
    emit(' %s, %s, %d x %d x %d, zones of %d x %d, %d calls per round; us per call' % (fmt, ARCH, n, h, w, zone[0], zone[1], reps))
    for name, v in res.items():
        rounds_line, stats_line = SB.leg_lines(name, v, 9)
        emit(rounds_line)
        emit(stats_line + '   %.3f B/pixel: %s' % (bpp[name], SB.hbm_share(bpp[name] * pix, med[name])))
    if not launch_only:
        emit('  stats / shade = %.2f   serve_st - serve = %.1f us (serve_st / serve = %.3f)   torch / stats = %.1f' % (
            med['stats'] / med['shade'], med['serve_st'] - med['serve'], med['serve_st'] / med['serve'], med['torch'] / med['stats']))
    won = {name: SB.beats(res['direct'], res[name]) for name in variants if name != 'direct'}
    for name in won:
        gain, noise = SB.margin(res['direct'], res[name])
        emit('  %s - direct = %+.1f us against a spread of %.1f us: the in-tree form %s' % (
            name, gain, noise, 'WINS' if won[name] else ('LOSES' if SB.beats(res[name], res['direct']) else 'is level')))
    return won


def main():
    ap = SB.parser(300, 7)
    ap.add_argument('--variant', action='append', default=[], metavar='NAME=LIB.so',
                    help='another build of the library whose risp_raw_stats is timed in the same rounds')
    args = ap.parse_args()
    emit = SB.Report(args.out)
    variants = {'direct': L.load().risp_raw_stats} if args.variant else {}
    for spec in args.variant:
        name, path = spec.split('=', 1)
        variants[name] = SB.load_parent(path, ['risp_raw_stats']).risp_raw_stats
    emit(SB.header(__file__, args, ''.join(' --variant %s=..' % v for v in variants if v != 'direct')))
    emit('stats: functional.raw_stats alone (memset and launch)   shade: functional.raw_shade alone   serve_st / serve: '
         'net.serve(raw, out=) with and without statistics=   torch: the same statistics from torch ops on the unpacked frames; '
         'host side included')
    net = SB.pipeline(ARCH)
    wins = {name: [] for name in variants if name != 'direct'}
    for fmt in FORMATS:
        for shape, zone, seed, reps in (((64, 256, 256), (32, 32), 10, args.reps), ((1, 3000, 4000), (200, 200), 20, max(20, args.reps // 3))):
            row = measure(net, shape, zone, seed, fmt, reps, args.rounds, variants, emit)
            for name, won in row.items():
                wins[name].append(won)
        if variants:
            # four frames, 3008 tiles of 64 rows: several rounds of workgroups per compute unit
            row = measure(net, (4, 3000, 4000), (200, 200), 30, fmt, max(20, args.reps // 6), args.rounds, variants, emit, True)
            for name, won in row.items():
                wins[name].append(won)
    for name, rows in wins.items():
        emit('%s: the in-tree form wins beyond the spread in %d of %d rows' % (name, sum(rows), len(rows)))
    emit.write()


if __name__ == '__main__':
    main()
