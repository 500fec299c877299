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
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from reconfigisp_amd.codes.data.synthetic_raw import make_batch  # noqa: E402
from reconfigisp_amd.codes.models import networks  # noqa: E402
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF  # noqa: E402

WHITE = 1023.0
DENOISERS = [('bilateral', 7), ('median', 8), ('fastnlm', 9)]
POSITIONS = [('front', 'Demosaic_02_sRGB_05_%02d_01_03'), ('behind', 'Demosaic_02_sRGB_%02d_05_01_03'), ('both', 'Demosaic_02_sRGB_05_%02d_06_01')]
SCENE_ONLY = [('gray-world', 'Demosaic_02_sRGB_05_01_03'), ('white-world', 'Demosaic_02_sRGB_06_01_03'),
              ('gray-world + white-world', 'Demosaic_02_sRGB_05_01_06'), ('Reinhard', 'Demosaic_02_sRGB_01_02')]


def frames_u16(n, h, w, seed):
    bay = make_batch(n, h, w, seed=seed)[0][:, 0]
    return (bay * WHITE).round().clamp(0, WHITE).to(torch.int32).to(torch.uint16).cuda()


def pipeline(arch):
    opt = {'network_G': {'which_model_G': 'OriginUniversal', 'architecture': arch, 'module_path': None,
                         'individual_module_paths': [None] * 8}}
    torch.manual_seed(10)
    net = networks.define_G(opt).cuda().eval()
    for name, par in net.named_parameters():
        if 'median' in name:                               # sigmoid(-2.5) < 1 / 7: the 3 x 3 window (the initial value gives 9 x 9)
            with torch.no_grad():
                par.fill_(-2.5)
    return net


def timed(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def measure(arch, keyword, route, raw, reps, rounds, emit):
    """(median, spread) per leg, and whether the fast leg clears the rule at this size"""
    n, h, w = raw.shape
    pix = n * h * w
    net = pipeline(arch)
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
    res = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            res[name].append(timed(fn, reps))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    emit(' %s, %d x %d x %d, %d calls per round; us per call; %.2e of the bytes differ from the default call (by at most %d)' % (
        arch, n, h, w, reps, differ, worst))
    for name, v in res.items():
        emit('  %-9s rounds %s' % (name, ' '.join('%.1f' % t for t in v)))
        emit('  %-9s median %.1f us  min %.1f  spread %.1f   %.0f MPix/s' % (name, med[name], min(v), spread[name], pix / med[name]))
    gain, noise = med['composed'] - med['fast'], max(spread.values())
    keep = gain > noise
    emit('  fast / composed = %.3f   composed - fast = %.1f us against a spread of %.1f: %s' % (
        med['fast'] / med['composed'], gain, noise, 'clears the rule' if keep else 'DOES NOT clear the rule'))
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit('tools/bench_serve_denoise_scene.py --reps %d --rounds %d   (%s)' % (args.reps, args.rounds, torch.cuda.get_device_name(0)))
    emit('net.serve(raw, out=buf[, fast_denoise_scene=True | fast_scene=True]), host side included')
    PF._DENOISE_SCENE_SLOWER = frozenset()                 # measure every combination, whatever the plan drops today
    sizes = [(frames_u16(64, 256, 256, 10), args.reps), (frames_u16(1, 3000, 4000, 20), max(10, args.reps // 3))]
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
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
