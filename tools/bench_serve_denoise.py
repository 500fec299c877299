#!/usr/bin/env python3
"""GPU box: the denoiser pipelines' one launch (serve(fast_denoise=True), risp_serve_denoise_u8) against the composed route
of the same pipeline - the default call, unchanged code - on resident uint16 frames, in interleaved rounds in one process.

    python tools/bench_serve_denoise.py [--out profiles/serve_denoise.txt] [--reps 100] [--rounds 7]

Pipelines (OriginUniversal): Demosaic_0D_sRGB_11_NN_01_14 - a bilinear (D = 2) or Malvar-He-Cutler (D = 3) demosaic,
WbManual, the bilateral (NN = 07), the median (08, its parameter set for the 3 x 3 window) or non-local means (09), Gamma,
GtmManual; 64 x 256 x 256 and one 3000 x 4000 frame.  Legs, each net.serve(raw, out=buf) with the host side included (what a
caller pays), timed between two device events:
  denoise     risp_serve_denoise_u8, one launch
  composed    risp_raw_crop -> risp_origin_demosaic -> chain -> the denoiser (the bilateral with its element-wise tail in
              risp_bilateral_chain_fwd) -> chain -> risp_quantise_u8, every stage output an fp32 plane
Each round times every leg once (REPS calls, after 3 warm ones); per leg: the rounds, median, minimum and spread - the spread
between the rounds of ONE leg is the noise a difference between two legs has to clear.  The bytes of the two legs are compared
first.  Bytes moved are algorithmic counts from the module list (fp32 planes written and read back by the composed route;
2 read + 3 written by the one launch)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from reconfigisp_amd.codes.data.synthetic_raw import make_batch  # noqa: E402
from reconfigisp_amd.codes.models import networks  # noqa: E402
from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF  # noqa: E402
from reconfigisp_amd.codes.models.modules import tools_origin as T  # noqa: E402

WHITE = 1023.0
DEMOSAICS = [('bilinear', 2), ('malvar', 3)]
DENOISERS = [('bilateral', 7), ('median', 8), ('fastnlm', 9)]


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


def composed_bytes_per_pixel(modules):
    """what the composed route moves per pixel: the crop (2 + 4), the demosaic (4 + 12), an element-wise run of k stages in
    one launch (12 + 12 k), a median / non-local means (12 + 12), a bilateral with the k stages behind it in its launch
    (12 + 12 (1 + k)), the conversion (12 + 3)"""
    total, run, bilateral = 6 + 16 + 15, 0, False
    flush = lambda: (12 + 12 * (run + bilateral)) if run or bilateral else 0
    for m in modules[1:]:
        if type(m) is T.Skip:
            continue
        if type(m) in PF._DENOISER:
            total, run, bilateral = total + flush(), 0, type(m) is T.OriginNoiseBilateral
            if not bilateral:
                total += 24
        else:
            run += 1
    return total + flush()


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


def measure(arch, raw, reps, rounds, emit):
    n, h, w = raw.shape
    pix = n * h * w
    net = pipeline(arch)
    buf = {k: torch.empty((n, h, w, 3), device='cuda', dtype=torch.uint8) for k in ('denoise', 'composed')}

    def denoise():
        net.serve(raw, WHITE, out=buf['denoise'], fast_denoise=True)

    def composed():
        net.serve(raw, WHITE, out=buf['composed'])

    legs = {'denoise': denoise, 'composed': composed}
    composed()
    assert net.last_serve_route == 'composed'
    denoise()
    assert net.last_serve_route == 'denoise'
    torch.cuda.synchronize()
    assert torch.equal(buf['denoise'], buf['composed']), 'the one launch and the composed route disagree'
    res = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            res[name].append(timed(fn, reps))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    bpp = {'denoise': 5, 'composed': composed_bytes_per_pixel(net.all_modules)}
    emit(' %s, %d x %d x %d, %d calls per round; us per call' % (arch, n, h, w, reps))
    for name, v in res.items():
        emit('  %-9s rounds %s' % (name, ' '.join('%.1f' % t for t in v)))
        emit('  %-9s median %.1f us  min %.1f  spread %.1f   %d B/pixel: %.3f TB/s' % (
            name, med[name], min(v), max(v) - min(v), bpp[name], bpp[name] * pix / (med[name] * 1e-6) / 1e12))
    emit('  denoise / composed = %.3f   (%.0f MPix/s against %.0f)' % (
        med['denoise'] / med['composed'], pix / med['denoise'], pix / med['composed']))
    return med


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

    emit('tools/bench_serve_denoise.py --reps %d --rounds %d   (%s)' % (args.reps, args.rounds, torch.cuda.get_device_name(0)))
    emit('net.serve(raw, out=buf[, fast_denoise=True]), host side included')
    batch, frame = frames_u16(64, 256, 256, 10), frames_u16(1, 3000, 4000, 20)
    wins = {}
    for den, code in DENOISERS:
        for dem, kind in DEMOSAICS:
            arch = 'Demosaic_%02d_sRGB_11_%02d_01_14' % (kind, code)
            for raw, reps in ((batch, args.reps), (frame, max(10, args.reps // 3))):
                med = measure(arch, raw, reps, args.rounds, emit)
                wins.setdefault(den, []).append(med['denoise'] < med['composed'])
    for den, w in wins.items():
        emit('%s: the one launch beats the composed route in %d of %d cases' % (den, sum(w), len(w)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
