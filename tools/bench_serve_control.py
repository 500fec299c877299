#!/usr/bin/env python3
"""GPU box: the device-side auto white balance / auto exposure - what the two launches of an update cost, what they add to a
served call, and what the loop costs a user who solves on the host; on resident frames, in interleaved rounds in one process.

    python tools/bench_serve_control.py [--out profiles/serve_control.txt] [--reps 300] [--rounds 7]

Pipeline (OriginUniversal, route 'classical'): Demosaic_02_sRGB_11_01_14 (bilinear, WbManual, Gamma, GtmManual); 64 x 256 x 256
with zones of 32 x 32 and one 3000 x 4000 frame with zones of 200 x 200; uint16 frames of 10-bit samples, black level 64, white
level 1023; 256 bins of four codes, lo 16, hi 900; a gain map of cell 64 over a vignette from functional.shading_map; the
controller's default settings.  Legs, host side included (what a caller pays), timed between two device events:
  update     ctl.update(st) alone: risp_control_solve and risp_gain_map on statistics that are already there
  serve_ctl  net.serve(raw, out=, lens_shading=ctl.shading, statistics=st) and ctl.update(st) behind it: the closed loop
  serve      the same serving call without the update
  host       the loop a user has without the controller: the same serving call, st.zones.cpu() and st.hist.cpu(), the solve and
             the map of tests/control_reference.py in numpy on the host, and the upload of the map
Each round times every leg once (REPS calls, the host leg REPS / 10, after 3 warm ones), after one round that is not kept; per
leg: the rounds, median, minimum and spread.  Before anything is timed one update is compared with the reference.  No time is
fixed in advance and there is no pass mark: the file records the numbers."""
import os
import sys

import numpy as np
import torch

import serve_bench as SB
sys.path.insert(0, os.path.join(SB.ROOT, 'tests'))
import control_reference as CR  # noqa: E402
import reconfigisp_amd.functional as F  # noqa: E402

ARCH = 'Demosaic_02_sRGB_11_01_14'
WHITE, BLACK, CELL = 1023.0, 64, 64
BINS, SHIFT, LO, HI = 256, 2, 16, 900


def measure(net, shape, zone, seed, reps, rounds, emit):
    n, h, w = shape
    raw = SB.frames_u16(n, h, w, seed, int(WHITE))
    base = F.shading_map(SB.vignette(h, w), h, w, CELL)
    st = F.raw_statistics(n, h, w, zone=zone, bins=BINS, hist_shift=SHIFT, lo=LO, hi=HI)
    ctl = F.gain_control(st, cell=CELL, base=base.cuda())
    host_gains = torch.empty_like(ctl.gains)                # the map of the host loop, and its state on the host
    host = {'state': CR.new_state()}
    out_a, out_b, out_c = (torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8) for _ in range(3))
    spec, geometry, base_np = CR.spec_tuple(), (h, w, zone[0], zone[1], SHIFT, 0), base.numpy()
    sensor = dict(black_level=BLACK)

    def leg_update():
        ctl.update(st)

    def leg_serve_ctl():
        net.serve(raw, WHITE, out=out_a, lens_shading=ctl.shading, statistics=st, **sensor)
        ctl.update(st)

    def leg_serve():
        net.serve(raw, WHITE, out=out_b, lens_shading=ctl.shading, statistics=st, **sensor)

    def leg_host():
        net.serve(raw, WHITE, out=out_c, lens_shading=(host_gains, CELL), statistics=st, **sensor)
        host['state'] = CR.solve_ref(st.zones.cpu().numpy(), st.hist.cpu().numpy(), host['state'], spec, geometry)
        host_gains.copy_(torch.from_numpy(CR.gain_map_ref(base_np, host['state'])))

    # one step of both loops from the same start: the same state, the same map
    host_gains.copy_(ctl.gains)
    leg_serve_ctl(), leg_host()
    torch.cuda.synchronize()
    assert net.last_serve_route == 'classical' and torch.equal(out_a, out_c)
    assert np.array_equal(ctl.state.cpu().numpy(), host['state']) and torch.equal(ctl.gains, host_gains), 'launches and reference disagree'
    legs = dict(update=leg_update, serve_ctl=leg_serve_ctl, serve=leg_serve, host=leg_host)
    res = SB.rounds_of(legs, {name: max(3, reps // 10) if name == 'host' else reps for name in legs}, rounds, True)
    med = {k: SB.median(v) for k, v in res.items()}
    zones = n * st.grid[0] * st.grid[1]
    emit(' %s, %d x %d x %d, zones of %d x %d (%d zones, %d workgroups), %d bins, map of %d x %d nodes, %d calls per round; us per call'
         % (ARCH, n, h, w, zone[0], zone[1], zones, min(1024, -(-zones // 256)), BINS, ctl.gains.shape[0], ctl.gains.shape[1], reps))
    for name, v in res.items():
        rounds_line, stats_line = SB.leg_lines(name, v, 9)
        emit(rounds_line)
        emit(stats_line)
    gain, noise = SB.margin(res['serve'], res['serve_ctl'])
    emit('  serve_ctl - serve = %.1f us against a spread of %.1f us (serve_ctl / serve = %.3f)   host / serve_ctl = %.1f' % (
        gain, noise, med['serve_ctl'] / med['serve'], med['host'] / med['serve_ctl']))
    emit('  state behind the rounds: %s' % ctl.state.cpu().tolist()[:12])


def main():
    args = SB.parser(300, 7).parse_args()
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    emit('update: ctl.update(st) alone (two launches)   serve_ctl / serve: net.serve(raw, out=, lens_shading=, statistics=) with and '
         'without the update behind it   host: the same call, the statistics read back, solved in numpy, the map uploaded; host side '
         'included')
    net = SB.pipeline(ARCH)
    for shape, zone, seed, reps in (((64, 256, 256), (32, 32), 10, args.reps), ((1, 3000, 4000), (200, 200), 20, max(20, args.reps // 3))):
        measure(net, shape, zone, seed, reps, args.rounds, emit)
    emit.write()


if __name__ == '__main__':
    main()
