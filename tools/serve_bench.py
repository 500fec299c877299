"""What the tools/bench_serve*.py scripts share: how a leg is timed, how rounds are run, the statistics and the rule that turn
rounds into a verdict, the verdict line the CPU tests read back, the report frame and the resident inputs.  A script states its
legs and the report lines that are its own; tools/README.md ("The serving benchmarks") has the protocol and the rule in words.

Importing this module puts the repository root on sys.path, so a script imports it first and the package after it.  The
statistics, the rule, the round runner and the verdict line are plain Python and need no GPU (tests/test_serve_bench_cpu.py)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12
MEDIAN_3X3 = -2.5           # pipeline(median=): sigmoid(-2.5) < 1 / 7, the 3 x 3 window


# ---- timing: one leg, then every leg once per round

def timed(fn, reps, warm=3):
    """us per call of ``fn``: ``warm`` calls, then ``reps`` calls between two device events.  Nothing else belongs between the
    events: the legs include their host side and some are 25 us long"""
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def rounds_of(legs, reps, rounds, warm_round, timed=timed):
    """{leg: [us per round]}: every leg of ``legs`` once per round, in dict order, so that drift reaches all legs alike.  ``reps``
    is a number or {leg: number}.  ``warm_round`` runs one more round in front and drops it (the first leg of the first round
    otherwise pays for the clocks coming up); every script passes what its recorded profile was measured with.  ``timed(leg,
    reps)`` is the clock: a script whose legs are not plain callables, or a test, passes its own"""
    res = {name: [] for name in legs}
    for r in range(-1 if warm_round else 0, rounds):
        for name, leg in legs.items():
            t = timed(leg, reps[name] if isinstance(reps, dict) else reps)
            if r >= 0:
                res[name].append(t)
    return res


# ---- statistics and the rule

def median(v):
    """the upper median"""
    return sorted(v)[len(v) // 2]


def spread(v):
    """between the rounds of ONE leg: the noise that a difference between two legs has to clear"""
    return max(v) - min(v)


def margin(fast, slow):
    """(gain, noise) of two lists of rounds, the two numbers a report prints beside the outcome of the rule"""
    return median(slow) - median(fast), max(spread(fast), spread(slow))


def beats(fast, slow):
    """the rule behind every measured table of pipeline_fusion: ``fast`` beats ``slow`` when the medians differ by more than the
    larger of the two spreads, median(slow) - median(fast) > max(spread(fast), spread(slow)); a table entry asks for that in
    every measured row"""
    gain, noise = margin(fast, slow)
    return gain > noise


def verdict_line(name, members):
    """the line that carries a table into a CPU test (tests/serve_verdicts.py reads it back); ``members`` in the order given"""
    return 'verdict: %s = %s' % (name, ' '.join(members) or 'none')


# ---- the report frame

def parser(reps, rounds):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--reps', type=int, default=reps)
    ap.add_argument('--rounds', type=int, default=rounds)
    return ap


class Report:
    """``emit = Report(args.out)``: ``emit(line)`` prints, flushes and keeps the line, ``emit.write()`` writes --out"""

    def __init__(self, out):
        self.out, self.lines = out, []

    def __call__(self, s):
        print(s, flush=True)
        self.lines.append(s)

    def write(self):
        if self.out:
            os.makedirs(os.path.dirname(os.path.abspath(self.out)), exist_ok=True)
            with open(self.out, 'w') as f:
                f.write('\n'.join(self.lines) + '\n')


def header(script, args, extra=''):
    return 'tools/%s --reps %d --rounds %d%s   (%s)' % (os.path.basename(script), args.reps, args.rounds, extra,
                                                       torch.cuda.get_device_name(0))


def leg_lines(name, v, width, fmt='%.1f'):
    """the two lines of a leg, `<leg> rounds ..` and `<leg> median .. us  min ..  spread ..`; the caller appends its own tail"""
    head = '  %-*s ' % (width, name)
    return (head + 'rounds ' + ' '.join(fmt % t for t in v),
            head + 'median %s us  min %s  spread %s' % tuple(fmt % t for t in (median(v), min(v), spread(v))))


def hbm_share(nbytes, us):
    """``nbytes`` moved in ``us``, as a rate and as a share of the HBM peak"""
    rate = nbytes / (us * 1e-6)
    return '%.3f TB/s = %.1f %% of the %.1f TB/s HBM peak' % (rate / 1e12, 100 * rate / HBM_PEAK, HBM_PEAK / 1e12)


# ---- inputs

def frames_int(n, h, w, seed, white):
    """(N,H,W) int32 samples 0 .. white on the host"""
    from reconfigisp_amd.codes.data.synthetic_raw import make_batch
    bay = make_batch(n, h, w, seed=seed)[0][:, 0]
    return (bay * white).round().clamp(0, white).to(torch.int32)


def frames_u16(n, h, w, seed, white):
    return frames_int(n, h, w, seed, white).to(torch.uint16).cuda()


def pack(x, bits):
    """(N,H,W) int32 samples below 2^bits -> (N,H,W * bits / 8) uint8 on the host (include/risp.h has the layout)"""
    n, h, w = x.shape
    if bits == 10:
        g = x.view(n, h, w // 4, 4)
        low = (g[..., 0] & 3) | (g[..., 1] & 3) << 2 | (g[..., 2] & 3) << 4 | (g[..., 3] & 3) << 6
        grp = torch.cat([g >> 2, low[..., None]], dim=-1)
    else:
        g = x.view(n, h, w // 2, 2)
        grp = torch.cat([g >> 4, ((g[..., 0] & 15) | (g[..., 1] & 15) << 4)[..., None]], dim=-1)
    return grp.to(torch.uint8).reshape(n, h, w * bits // 8).contiguous()


def vignette(h, w):
    """a (4,33,33) gain image: 1 at the centre, up to 2 in the corners, a little colour shading between the planes"""
    y, x = np.meshgrid(np.linspace(-1, 1, 33), np.linspace(-1, 1, 33), indexing='ij')
    r2 = (y * y + x * x) / 2
    return np.stack([1 + (0.85 + 0.05 * c) * r2 for c in range(4)])


def pipeline(arch, model='OriginUniversal', median=None, **network_g):
    """the network of ``arch`` as the scripts build it (seed 10, no checkpoint).  ``median``: the value every parameter of a
    median stage is set to - its window size is learned, and the initial value gives 9 x 9.  ``network_g``: further entries of
    the network options (the conditional heads' widths)"""
    from reconfigisp_amd.codes.models import networks
    opt = {'network_G': dict(which_model_G=model, architecture=arch, module_path=None, individual_module_paths=[None] * 8,
                             **network_g)}
    torch.manual_seed(10)
    net = networks.define_G(opt).cuda().eval()
    if median is not None:
        for name, par in net.named_parameters():
            if 'median' in name:
                with torch.no_grad():
                    par.fill_(median)
    return net


def load_parent(path, names):
    """another build of the library (the parent commit's, an ablation) with ``names`` bound to the in-tree signatures"""
    from reconfigisp_amd import lib as L
    other = C.CDLL(os.path.abspath(path))
    for name in names:
        fn = getattr(other, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return other


# ---- one entry point in several builds of the library (tools/bench_serve_defect_rows.py, tools/bench_output_builds.py)

def load_builds(items, entries):
    """{'tree': {entry: function}, NAME: {entry: function}, ..}: the in-tree library first, then every ``NAME=PATH`` of ``items``"""
    from reconfigisp_amd import lib as L
    builds = {'tree': {e: getattr(L.load(), e) for e in entries}}
    for item in items:
        name, path = item.split('=', 1)
        other = load_parent(path, list(entries))
        builds[name] = {e: getattr(other, e) for e in entries}
    return builds


def compare_builds(emit, row, builds, entry, leg, filled, reps, rounds, reset=lambda: None, timed=timed):
    """One row of a build comparison -> the names of the builds that beat the tree in it.  ``leg()`` is one call of a wrapper that
    ends in ``entry`` and fills the tensors ``filled``; every build fills the same tensors (where a buffer lies moves a call by
    more than builds differ).  First one call per build from the same start (``reset()``), and the results must be equal; then
    ``rounds`` interleaved rounds after one that is dropped; then a line per build with the outcome of ``beats`` against the tree."""
    from reconfigisp_amd import lib as L

    def timed_build(name, reps):                                # a leg of rounds_of is a build's name
        L._FN[entry] = builds[name][entry]
        return timed(leg, reps)

    try:
        first = {}
        for name in builds:
            reset()
            L._FN[entry] = builds[name][entry]
            leg()
            first[name] = [t.clone() for t in filled]
        assert all(torch.equal(a, b) for o in first.values() for a, b in zip(o, first['tree'])), 'the builds disagree: ' + row
        res = rounds_of({name: name for name in builds}, reps, rounds, True, timed_build)
    finally:
        L._FN[entry] = builds['tree'][entry]
    emit(' %s, %d calls per round; us per call' % (row, reps))
    beaten = []
    for name, v in res.items():
        tail = ''
        if name != 'tree':
            gain, noise = margin(v, res['tree'])
            won = beats(v, res['tree'])
            tail = '   tree - %s = %+.1f us against a spread of %.1f us: %s' % (
                name, gain, noise, 'BEATS the tree' if won else ('loses' if beats(res['tree'], v) else 'level'))
            if won:
                beaten.append(name)
        emit('  %-10s median %.1f us  min %.1f  spread %.1f   rounds %s%s' % (
            name, median(v), min(v), spread(v), ' '.join('%.1f' % t for t in v), tail))
    return beaten


def beaten_line(rows):
    """the closing line of a build comparison; ``rows``: '<row> by <build>' for every row in which a build beat the tree"""
    return 'rows in which another build beats the tree: %s' % ('; '.join(rows) or 'none')
