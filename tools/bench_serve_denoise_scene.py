#!/usr/bin/env python3
"""GPU box: the denoise + scene route (serve(fast_denoise_scene=True): per scene stage a statistics and a finish launch, then
risp_serve_denoise_scene_u8) against the composed route of the same pipeline - the default call, unchanged code - on
resident uint16 frames, in interleaved rounds in one process.  The plain scene route (serve(fast_scene=True)), whose speed had
not been measured, runs in the same way at the end.

    python tools/bench_serve_denoise_scene.py [--out profiles/serve_denoise_scene.txt] [--reps 100] [--rounds 7]

Pipelines (OriginUniversal, bilinear demosaic): each of the bilateral (07), the median (08, its parameter set for the 3 x 3
window) and non-local means (09) with gray-world in front (Demosaic_02_sRGB_05_NN_01_03: the headline pipeline with an
automatic white balance), gray-world behind (.._NN_05_01_03) and one scene stage each side (.._05_NN_06_01: gray-world,
denoiser, white-world, Gamma); scene-only lists Demosaic_02_sRGB_05_01_03 (gray-world), _06_01_03 (white-world),
_05_01_06 (both) and _01_02 (Reinhard); 64 x 256 x 256 and one 3000 x 4000 frame.  Legs, each net.serve(raw, out=buf) with
the host side included (what a caller pays), timed between two device events:
  fast        2 S + 1 launches for S scene stages, no fp32 plane
  composed    risp_raw_crop -> risp_origin_demosaic -> risp_channel_stats / gains / chain -> the denoiser -> ... ->
              risp_quantise_u8, every stage output an fp32 plane
Each round times every leg once (REPS calls, after 3 warm ones); per leg: the rounds, median, minimum and spread - the spread
between the rounds of ONE leg is the noise a difference between two legs has to clear.

The keep / drop rule: a (denoiser, scene position) combination stays in pipeline_fusion.denoise_scene_plan only if the fast
leg's median beats the composed leg's at BOTH sizes by more than the larger spread of the two legs.  The last lines name the
combinations that do not; pipeline_fusion._DENOISE_SCENE_SLOWER holds them."""
import torch

import serve_bench as SB
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF

WHITE = 1023.0
DENOISERS = [('bilateral', 7), ('median', 8), ('fastnlm', 9)]
POSITIONS = [('front', 'Demosaic_02_sRGB_05_%02d_01_03'), ('behind', 'Demosaic_02_sRGB_%02d_05_01_03'), ('both', 'Demosaic_02_sRGB_05_%02d_06_01')]
SCENE_ONLY = [('gray-world', 'Demosaic_02_sRGB_05_01_03'), ('white-world', 'Demosaic_02_sRGB_06_01_03'),
              ('gray-world + white-world', 'Demosaic_02_sRGB_05_01_06'), ('Reinhard', 'Demosaic_02_sRGB_01_02')]


def measure(arch, keyword, route, raw, reps, rounds, emit):
    """whether the fast leg clears the rule at this size"""
    n, h, w = raw.shape
    pix = n * h * w
    net = SB.pipeline(arch, median=SB.MEDIAN_3X3)
    buf = {k: torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8) for k in ('fast', 'composed')}

    def fast():
        net.serve(raw, WHITE, out=buf['fast'], **{keyword: True})

    def composed():
        net.serve(raw, WHITE, out=buf['composed'])

    legs = {'fast': fast, 'composed': composed}
    composed()
    assert net.last_serve_route == 'composed'
    fast()
    assert net.last_serve_route == route, net.last_serve_route
    torch.cuda.synchronize()
    differ = (buf['fast'] != buf['composed']).float().mean().item()
    worst = (buf['fast'].int() - buf['composed'].int()).abs().max().item()
    res = SB.rounds_of(legs, reps, rounds, False)
    med = {k: SB.median(v) for k, v in res.items()}
    emit(' %s, %d x %d x %d, %d calls per round; us per call; %.2e of the bytes differ from the default call (by at most %d)' % (
        arch, n, h, w, reps, differ, worst))
    for name, v in res.items():
        rounds_line, stats_line = SB.leg_lines(name, v, 9)
        emit(rounds_line)
        emit(stats_line + '   %.0f MPix/s' % (pix / med[name]))
    gain, noise = SB.margin(res['fast'], res['composed'])
    keep = SB.beats(res['fast'], res['composed'])
    emit('  fast / composed = %.3f   composed - fast = %.1f us against a spread of %.1f: %s' % (
        med['fast'] / med['composed'], gain, noise, 'clears the rule' if keep else 'DOES NOT clear the rule'))
    return keep


def main():
    args = SB.parser(100, 7).parse_args()
    emit = SB.Report(args.out)
    emit(SB.header(__file__, args))
    emit('net.serve(raw, out=buf[, fast_denoise_scene=True | fast_scene=True]), host side included')
    PF._DENOISE_SCENE_SLOWER = frozenset()                 # measure every combination, whatever the plan drops today
    sizes = [(SB.frames_u16(64, 256, 256, 10, WHITE), args.reps), (SB.frames_u16(1, 3000, 4000, 20, WHITE), max(10, args.reps // 3))]
    verdict = {}
    emit('denoise + scene route (fast_denoise_scene=True)')
    for den, code in DENOISERS:
        for where, pattern in POSITIONS:
            verdict[(den, where)] = all([measure(pattern % code, 'fast_denoise_scene', 'denoise_scene', raw, reps, args.rounds, emit)
                                         for raw, reps in sizes])
    emit('scene route (fast_scene=True)')
    scene = {what: all([measure(arch, 'fast_scene', 'scene', raw, reps, args.rounds, emit) for raw, reps in sizes])
             for what, arch in SCENE_ONLY}
    for (den, where), keep in verdict.items():
        emit('%-9s scene stage %-6s: %s' % (den, where, 'stays in denoise_scene_plan' if keep else 'DROPPED from denoise_scene_plan'))
    for what, keep in scene.items():
        emit('scene route, %s: %s' % (what, 'faster than the default call at both sizes' if keep else 'NOT faster at both sizes'))
    emit.write()


if __name__ == '__main__':
    main()
