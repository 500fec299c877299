"""GPU: the fused stencil segment (risp_bilateral_chain_fwd, risp_fused.hip) over its whole argument space.

One entry point dispatches to three kernel families, each with and without WbQuadratic:

    quad   bilateral_chain_quad_kernel<WBQ>        mosaic input, max_window == 3, 16-byte aligned mosaic
    lds1   bilateral_chain_kernel<FB, 1, WBQ>      max_window == 3 from BGR, or from a mosaic that is only 8-byte aligned
    lds0   bilateral_chain_kernel<FB, 0, WBQ>      every other max_window (1, 5 .. 17), run-time radius

Every case of the table below (and of the seeded walk) is launched in every form its arguments can take, every stage
output pre-filled with NaN, and held to three statements:

  1. bits against the stage-by-stage path (F.demosaic_nearest, F.origin_denoise 'bilateral', then each op's own launch):
     torch.equal on every stage - the header's "same bits" claim, no tolerance;
  2. bits across forms where the same arguments run in two (aligned against 8-byte offset mosaic);
  3. the float64 restatement of tests/fused_segment_reference.py, stage by stage: the demosaic exactly; the bilateral in
     codes - no code off by more than 1, a code may differ ONLY where the restatement's unquantised value lies within
     TAU codes of a rounding boundary, and at most 2e-3 of the codes of a case may differ at all; every element-wise
     stage against the restatement started from the GPU's own previous stage (single-code flips must not cascade) at
     conftest.assert_close.

The tables, the input builders and the walk's generator are plain CPU code: tests/test_fused_segment_reference_cpu.py
imports them to check the coverage of the table and the tie budget of every input without a GPU.
"""
import os

import numpy as np
import pytest
import torch

import fused_segment_reference as R
import isp_oracle as O
from fused_segment_reference import OP_SKIP, OP_WB_MANUAL, OP_GAMMA, OP_GTM_MANUAL, OP_WB_QUADRATIC, OP_GAIN3

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------- the axes
SHAPES = {                       # (N, H, W); LDS tiles are 64 x 16 pixels, quad tiles 64 x 32
    '1x2x4': (1, 2, 4),          # one patch: xl and xr both clamped
    '1x2x8': (1, 2, 8),
    '2x4x4': (2, 4, 4),
    '3x6x12': (3, 6, 12),
    '1x34x132': (1, 34, 132),    # the last tile column cut in every form (4 valid columns), a third tile row of 2 rows
    '9x30x68': (9, 30, 68),      # 36 LDS tiles / 18 quad tiles: not a multiple of 8, plain tile order
    '8x64x256': (8, 64, 256),    # 128 LDS tiles / 64 quad tiles: XCD-aware tile order
    '2x300x4': (2, 300, 4),      # tall and narrow: one patch column, 19 LDS / 10 quad tile rows
    '64x256x256': (64, 256, 256),  # the headline batch: once, aligned mosaic only; restatement on the first and last image
    '1x10x12': (1, 10, 12),      # the smallest shape the guard H, W > max_window / 2 admits for window 17
    '1x12x16': (1, 12, 16),      # ... and one just above it
}
TAILS = {
    'empty': [],
    'skip': [OP_SKIP],
    'gain3': [OP_GAIN3],
    'wb-skip-gamma': [OP_WB_MANUAL, OP_SKIP, OP_GAMMA],
    'gamma-wbq': [OP_GAMMA, OP_WB_QUADRATIC],
    'gtm-gamma-gamma-wb': [OP_GTM_MANUAL, OP_GAMMA, OP_GAMMA, OP_WB_MANUAL],
    'full8': [OP_WB_MANUAL, OP_GAMMA, OP_GTM_MANUAL, OP_GAIN3, OP_SKIP, OP_WB_QUADRATIC, OP_GAMMA, OP_WB_MANUAL],
}
WINDOWS = {                      # name: (max_window, per-image windows, cycled over the batch)
    '1/mw1': (1, [1]),           # max_window 1: radius 0 through the run-time-radius form
    '1/mw3': (3, [1]),           # windows 1 under max_window 3: the radius-1 forms with an empty ring
    '3': (3, [3]),
    '1-3': (3, [3, 1, 1, 3]),
    '5': (5, [5]),
    '3-5-7': (7, [3, 5, 7]),
    '9': (9, [9]),
    '17': (17, [17]),
}
SAMPLES = ('synthetic', 'uniform', 'constant', 'step')
# (sigma_color, sigma_space); image i of a case takes SIGMAS[(start + i) % 6].  0.05 drives every off-centre weight whose
# exponent is not exactly 0 to 0.  (sigma 0 is outside the plugin's range: tools_origin.py maps [0,1] to [1,100].)
SIGMAS = [(1.0, 1.0), (100.0, 100.0), (1.0, 100.0), (100.0, 1.0), (0.05, 0.05), (0.05, 100.0)]

# ---------------------------------------------------------------------------------------------------- the sweep
# (shape, input, windows, tail, samples, first sigma pair).  A mosaic case runs twice, 16-byte aligned and as a view at
# an 8-byte offset: with max_window 3 that is the quad form and the lds1 form, otherwise lds0 both times.  Coverage
# (checked by test_fused_segment_reference_cpu.py::test_sweep_covers_every_pair): every tail and every shape with
# every family (the headline and the two window-17 shapes aside, which belong to one family), every window, sample
# family, sigma pair and input kind with every family that admits it.
CASES = [
    # --- mosaic, max_window 3: quad (aligned) + lds1 (offset)
    ('1x2x4', 'mosaic', '3', 'full8', 'synthetic', 0),
    ('1x2x8', 'mosaic', '1/mw3', 'empty', 'uniform', 1),
    ('2x4x4', 'mosaic', '1-3', 'skip', 'constant', 2),
    ('3x6x12', 'mosaic', '3', 'gain3', 'step', 3),
    ('1x34x132', 'mosaic', '3', 'wb-skip-gamma', 'uniform', 4),
    ('9x30x68', 'mosaic', '1-3', 'gamma-wbq', 'synthetic', 5),
    ('8x64x256', 'mosaic', '3', 'gtm-gamma-gamma-wb', 'synthetic', 0),
    ('2x300x4', 'mosaic', '3', 'full8', 'uniform', 2),
    ('64x256x256', 'mosaic', '3', 'wb-skip-gamma', 'synthetic', 0),
    # --- BGR, max_window 3: lds1
    ('3x6x12', 'bgr', '1-3', 'full8', 'uniform', 0),
    ('1x34x132', 'bgr', '3', 'gamma-wbq', 'synthetic', 3),
    ('8x64x256', 'bgr', '3', 'gain3', 'step', 1),
    ('1x2x4', 'bgr', '1/mw3', 'skip', 'constant', 5),
    # --- every other max_window: lds0
    ('1x2x4', 'mosaic', '1/mw1', 'gamma-wbq', 'uniform', 0),
    ('1x2x8', 'bgr', '1/mw1', 'full8', 'synthetic', 1),
    ('2x4x4', 'mosaic', '3-5-7', 'gain3', 'uniform', 2),
    ('3x6x12', 'mosaic', '3-5-7', 'wb-skip-gamma', 'synthetic', 3),
    ('1x34x132', 'mosaic', '5', 'empty', 'step', 4),
    ('9x30x68', 'bgr', '3-5-7', 'gtm-gamma-gamma-wb', 'uniform', 5),
    ('8x64x256', 'mosaic', '5', 'skip', 'synthetic', 0),
    ('2x300x4', 'bgr', '5', 'full8', 'constant', 1),
    ('1x10x12', 'mosaic', '17', 'full8', 'synthetic', 2),
    ('1x12x16', 'bgr', '17', 'gamma-wbq', 'uniform', 3),
    ('9x30x68', 'mosaic', '5', 'gain3', 'constant', 4),
    ('3x6x12', 'bgr', '9', 'wb-skip-gamma', 'uniform', 1),
]
# Arguments the guards refuse BEFORE any launch (risp_fused.hip RISP_CHECK_ARG lines, BilateralChainPlan's own check):
# (N, H, W), input, max_window, tail, the exception
REFUSED = [
    ((1, 2, 4), 'mosaic', 5, [], RuntimeError),                 # H = 2 is not > 5 / 2
    ((2, 4, 4), 'bgr', 9, [], RuntimeError),                    # H = W = 4 is not > 9 / 2
    ((1, 8, 12), 'mosaic', 17, [], RuntimeError),               # H = 8 is not > 17 / 2
    ((1, 10, 8), 'bgr', 17, [], RuntimeError),                  # W = 8 is not > 17 / 2
    ((1, 16, 16), 'mosaic', 4, [], RuntimeError),               # even window
    ((1, 16, 16), 'bgr', 19, [], RuntimeError),                 # beyond 17
    ((1, 3, 8), 'bgr', 3, [], ValueError),                      # odd H
    ((1, 4, 6), 'mosaic', 3, [], ValueError),                   # W % 4
    ((1, 16, 16), 'mosaic', 3, [OP_GAMMA] * 9, RuntimeError),   # RISP_MAX_CHAIN + 1 stages
    ((1, 16, 16), 'bgr', 3, [R.OP_DEMOSAIC_NEAREST], RuntimeError),   # the demosaic is not a tail op
]

# ---------------------------------------------------------------------------------------------------- the tie budget
# TAU[k]: how close, in codes, the restatement's unquantised value must be to a rounding boundary for a code of window k
# to be allowed to differ.  Not taken from the kernel: the oracle's bilateral (oracle/isp_oracle.py) was run in float32
# and in float64 on the CPU on every input of the sweep, the largest |v32 - v64| in codes recorded per window size
# (E32), and TAU = 2 x E32 - the factor of conftest.ErrorBudget: the HIP path may cost at most twice the reference's own
# fp32 arithmetic.  tests/test_fused_segment_reference_cpu.py re-measures E32 and checks that the float32 oracle itself
# passes the rule below with this TAU on every input.  Measured (all on 'uniform' inputs, whose samples reach 1.3 x 255):
#   window 1: 1.502e-5 (half an ulp of x * 255 above 256)   3: 8.812e-5   5: 1.359e-4   7: 1.538e-4   9: 1.989e-4
#   17: 1.462e-4   ->   TAU = 3.0e-5, 1.8e-4, 2.7e-4, 3.1e-4, 4.0e-4, 2.9e-4 codes
E32 = {1: 1.502e-5, 3: 8.812e-5, 5: 1.359e-4, 7: 1.538e-4, 9: 1.989e-4, 17: 1.462e-4}
TAU = {k: 2.0 * v for k, v in E32.items()}
TIE_CAP = 2e-3                   # the share of codes of one case that may differ (codes_close of test_gpu_origin.py)

_FUZZ = int(os.environ.get('RISP_TEST_SEEDS', '8'))               # soak runs: RISP_TEST_SEEDS=64


# ---------------------------------------------------------------------------------------------------- builders (CPU)
def family(from_bayer, max_window, aligned):
    if max_window // 2 != 1:
        return 'lds0'
    return 'quad' if from_bayer and aligned else 'lds1'


def forms(shape_name, kind, max_window):
    """[(family, aligned)] a case is launched in"""
    if kind == 'bgr':
        return [(family(False, max_window, True), True)]
    if shape_name == '64x256x256':
        return [(family(True, max_window, True), True)]
    return [(family(True, max_window, True), True), (family(True, max_window, False), False)]


def make_samples(kind, from_bayer, n, h, w, seed):
    """float32 segment input, (N,1,H,W) mosaic or (N,3,H,W) BGR"""
    c = 1 if from_bayer else 3
    if kind == 'synthetic':
        bay, gt = O.synthetic_raw(n, max(h, 16), max(w, 16), seed=seed)
        return (bay if from_bayer else gt)[:, :, :h, :w].contiguous()
    if kind == 'uniform':                    # clip on both sides of the 8-bit range
        rng = np.random.Generator(np.random.PCG64(seed))
        return torch.from_numpy(rng.uniform(-0.2, 1.3, size=(n, c, h, w)).astype(np.float32))
    # flat colours that are exact codes / 255: (B, G, R) of the two sides, per image
    rng = np.random.Generator(np.random.PCG64(seed))
    lo = rng.integers(0, 56, size=(n, 3))
    bgr = torch.empty(n, 3, h, w)
    for i in range(n):
        for ch in range(3):
            bgr[i, ch] = float(lo[i, ch]) / 255.0
            if kind == 'step':               # two flat halves, 200 codes apart (the cut on a quad boundary)
                if i % 2 and h >= 4:
                    bgr[i, ch, (h // 4) * 2:] = float(lo[i, ch] + 200) / 255.0
                else:
                    bgr[i, ch, :, (w // 4) * 2:] = float(lo[i, ch] + 200) / 255.0
    if not from_bayer:
        return bgr
    bay = torch.empty(n, 1, h, w)            # the mosaic whose nearest demosaic is that image
    bay[:, 0, 0::2, 0::2] = bgr[:, 2, 0::2, 0::2]
    bay[:, 0, 0::2, 1::2] = bgr[:, 1, 0::2, 1::2]
    bay[:, 0, 1::2, 0::2] = bgr[:, 1, 1::2, 0::2]
    bay[:, 0, 1::2, 1::2] = bgr[:, 0, 1::2, 1::2]
    return bay


def make_params(ops, n, rng, full):
    """per-stage (N,P) float32 blocks as the C ABI takes them.  ``full``: the walk's ranges - everything over [0,1] (gains
    x 5 / x 3), WbQuadratic in [0.3, 0.7] as test_random_pointwise_ops_forward_and_gradients (outside it the polynomial
    amplifies fp32 noise past the bar in the oracle itself); otherwise the ranges of test_pointwise_vs_oracle."""
    u = lambda k, a=0.0, b=1.0: torch.from_numpy(rng.uniform(a, b, size=(n, k)).astype(np.float32))
    out = []
    for op in ops:
        if op == OP_SKIP:
            out.append(None)
        elif op == OP_WB_MANUAL:
            out.append(u(3) * 5)
        elif op == OP_GAMMA:
            out.append(u(1) if full else u(1, 0.2, 0.9))
        elif op == OP_GTM_MANUAL:
            out.append(u(3))
        elif op == OP_WB_QUADRATIC:
            out.append(u(30, 0.3, 0.7) if full else u(30, 0.4, 0.6))
        elif op == OP_GAIN3:
            out.append(u(3) * 3)
        else:
            raise ValueError(op)
    return out


def sweep_case(index):
    """-> dict(x, from_bayer, window, sc, ss, max_window, ops, params, forms, what, ref_images)"""
    shape_name, kind, win_name, tail_name, samples, s0 = CASES[index]
    n, h, w = SHAPES[shape_name]
    mw, pattern = WINDOWS[win_name]
    from_bayer = kind == 'mosaic'
    sig = [SIGMAS[(s0 + i) % len(SIGMAS)] for i in range(n)]
    ops = list(TAILS[tail_name])
    return dict(x=make_samples(samples, from_bayer, n, h, w, seed=1000 + index), from_bayer=from_bayer,
                window=torch.tensor([pattern[i % len(pattern)] for i in range(n)], dtype=torch.int32),
                sc=torch.tensor([s[0] for s in sig]), ss=torch.tensor([s[1] for s in sig]), max_window=mw, ops=ops,
                params=make_params(ops, n, np.random.Generator(np.random.PCG64(2000 + index)), full=False),
                forms=forms(shape_name, kind, mw), what='%s %s win %s tail %s %s' % CASES[index][:5],
                ref_images=[0, n - 1] if shape_name == '64x256x256' else list(range(n)))


def near_tie_share(case):
    """share of the bilateral's codes whose unquantised float64 value lies within TAU of a rounding boundary"""
    idx = case['ref_images']
    _, raw = R.segment(case['x'][idx], case['from_bayer'], case['window'][idx], case['sc'][idx], case['ss'][idx], [], [])
    tau = torch.tensor([TAU[int(k)] for k in case['window'][idx]], dtype=torch.float64).view(-1, 1, 1, 1)
    return (R.tie_distance(raw) <= tau).double().mean().item()


def walk_case(seed):
    """One step of the seeded walk over the same axes: shapes up to 2 x 120 x 160, per-image windows from {1, 3, 5, 7, 9}
    (40 % of the steps from {1, 3}: the radius-1 forms), tails of 0 .. 8 stages, parameters over their full range.
    WbQuadratic is placed only where its input is bounded by 1 (after the bilateral, a clamping op or a gamma of such
    a value): the polynomial squares its input, and behind an unclipped gain of up to 5 its fp32 cancellation error
    passes the bar in the oracle itself.  An input that puts more than TIE_CAP of its codes within TAU of a rounding
    boundary is drawn again (a property of the input and the float64 restatement alone)."""
    rng = np.random.default_rng(4200 + seed)
    n, h, w = int(rng.integers(1, 3)), 2 * int(rng.integers(4, 61)), 4 * int(rng.integers(2, 41))
    from_bayer = bool(rng.random() < 0.6)
    pool = [1, 3] if rng.random() < 0.4 else [1, 3, 5, 7, 9]
    window = [int(k) for k in rng.choice(pool, size=n)]
    mw = max(window) if rng.random() < 0.7 else max(pool)
    sig = np.exp(rng.uniform(0.0, np.log(100.0), size=(2, n)))
    sig = np.where(rng.random((2, n)) < 0.15, 0.05, sig).astype(np.float32)
    ops, unit = [], True                      # unit: the running value is known to lie in [0, 1]
    for _ in range(int(rng.integers(0, 9))):
        op = int(rng.choice([OP_SKIP, OP_WB_MANUAL, OP_GAMMA, OP_GTM_MANUAL, OP_WB_QUADRATIC, OP_GAIN3]))
        if op == OP_WB_QUADRATIC and not unit:
            op = OP_GTM_MANUAL
        unit = unit if op in (OP_SKIP, OP_GAMMA) else op != OP_WB_MANUAL
        ops.append(op)
    params = make_params(ops, n, rng, full=True)
    samples = SAMPLES[int(rng.integers(0, 4))]
    case = dict(from_bayer=from_bayer, window=torch.tensor(window, dtype=torch.int32), sc=torch.from_numpy(sig[0]),
                ss=torch.from_numpy(sig[1]), max_window=mw, ops=ops, params=params,
                forms=forms('', 'mosaic' if from_bayer else 'bgr', mw), ref_images=list(range(n)),
                what='walk %d: %d x %d x %d %s win %s/%d %s tail %s' % (seed, n, h, w, 'mosaic' if from_bayer else 'bgr',
                                                                      window, mw, samples, ops))
    for attempt in range(8):
        case['x'] = make_samples(samples, from_bayer, n, h, w, seed=5000 + 8 * seed + attempt)
        if near_tie_share(case) <= TIE_CAP:
            return case
    raise AssertionError('%s: no input under the tie cap in 8 draws' % case['what'])


# ---------------------------------------------------------------------------------------------------- the checks (GPU)
COUNTS = {}                      # family -> [cases run, largest share of differing (tie-excused) codes]


def _offset_view(x):
    """the same data as a contiguous view 8 bytes into a fresh allocation"""
    buf = torch.empty(x.numel() + 4, device=x.device, dtype=torch.float32)
    v = buf[2:2 + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 8
    return v


def _unfused_op(F, L, op, x, p):
    if op == OP_WB_MANUAL:
        return F.wb_manual(x, p)
    if op == OP_GAMMA:
        return F.gamma(x, p)
    if op == OP_GTM_MANUAL:
        return F.gtm_manual(x, p)
    if op == OP_WB_QUADRATIC:
        return F.wb_quadratic(x, p)
    assert op == OP_GAIN3
    y = torch.empty_like(x)                  # the launch behind F.grayworld, with the gains handed in
    L.call('risp_gain3_fwd', F._p(x), F._p(p), F._p(y), x.shape[0], x.shape[2] * x.shape[3], F._stream())
    return y


def _kernel_name(fam, from_bayer, wbq):
    b = lambda v: 'true' if v else 'false'
    if fam == 'quad':
        return 'bilateral_chain_quad_kernel<%s>' % b(wbq)
    return 'bilateral_chain_kernel<%s,%d,%s>' % (b(from_bayer), 1 if fam == 'lds1' else 0, b(wbq))


def run_case(case, rtol):
    import reconfigisp_amd.functional as F
    from reconfigisp_amd import lib as L
    from conftest import assert_close
    what, fb, mw, ops = case['what'], case['from_bayer'], case['max_window'], case['ops']
    x = case['x'].cuda()
    assert x.data_ptr() % 16 == 0
    win, sc, ss = case['window'].cuda(), case['sc'].cuda(), case['ss'].cuda()
    params = [p.cuda() if p is not None else None for p in case['params']]
    wbq = OP_WB_QUADRATIC in ops
    failed = []                              # every statement is evaluated, so that a report shows WHICH of the three fail

    def check(ok, message, *args):
        if not ok:
            failed.append(message % args if args else message)

    # ---- the stage-by-stage path
    with torch.no_grad():
        unfused, cur = [], x
        if fb:
            cur = F.demosaic_nearest(x)
            unfused.append(cur)
        cur = F.origin_denoise(cur, 'bilateral', {'window_length': win, 'sigma_color': sc, 'sigma_space': ss,
                                                  'max_window': mw}, (255.0, 255.0))
        unfused.append(cur)
        for op, p in zip(ops, params):
            if op != OP_SKIP:
                cur = _unfused_op(F, L, op, cur, p)
            unfused.append(cur)

    # ---- every form the arguments can take
    results = []
    for fam, aligned in case['forms']:
        if aligned:
            name = L.load().risp_bilateral_chain_kernel(int(fb), mw, int(wbq)).decode()
            assert name == _kernel_name(fam, fb, wbq), '%s: %s launches %s' % (what, fam, name)
        plan = F.BilateralChainPlan(x if aligned else _offset_view(x), fb, win, sc, ss, mw, ops, params)
        assert len(plan.outs) == len(unfused) == (2 if fb else 1) + len(ops)
        for o in plan.outs:
            o.fill_(float('nan'))            # every element of every stage must be written
        outs = plan.launch()
        first = 2 if fb else 1
        for k, op in enumerate(ops):         # a SKIP stage aliases the stage in front of it
            assert (outs[first + k] is outs[first + k - 1]) == (op == OP_SKIP), '%s stage %d' % (what, first + k)
        fused = [o.clone() for o in outs]
        for k, (a, b) in enumerate(zip(fused, unfused)):
            tag = '%s [%s%s] stage %d' % (what, fam, '' if aligned else ', offset', k)
            check(not torch.isnan(a).any().item(), '[unwritten] %s: elements left unwritten', tag)
            check(torch.equal(a, b), '[1: stage-by-stage bits] %s: %d elements differ, max %g', tag, (a != b).sum().item(),
                  (a - b).abs().max().item())
        results.append((fam, aligned, fused))
    for fam, aligned, fused in results[1:]:   # bits across forms
        for k, (a, b) in enumerate(zip(results[0][2], fused)):
            check(torch.equal(a, b), '[2: bits across forms] %s stage %d: %s and %s differ', what, k, results[0][0], fam)

    # ---- the float64 restatement (the forms hold the same bits: one comparison serves all of them)
    idx = case['ref_images']
    fused = [t[idx].cpu() for t in results[0][2]]
    xs, wins = case['x'][idx], case['window'][idx]
    ref, raw = R.segment(xs, fb, wins, case['sc'][idx], case['ss'][idx], [], [])
    k = 0
    if fb:
        check(torch.equal(fused[0].double(), ref[0]), '[3: float64 restatement] %s: demosaic', what)
        k = 1
    got = fused[k].double() * 255.0
    codes = got.round()
    check((got - codes).abs().max().item() <= 1e-4 and codes.min() >= 0 and codes.max() <= 255,
          '[3: float64 restatement] %s: the bilateral stage does not hold codes / 255', what)
    d = (codes - R.code(raw)).abs()
    tau = torch.tensor([TAU[int(v)] for v in wins], dtype=torch.float64).view(-1, 1, 1, 1)
    dist = R.tie_distance(raw)
    differ = d > 0
    share = differ.double().mean().item()
    print('%s: %d of %d codes differ (share %.2e), largest tie distance among them %.3e, max code difference %d' % (
        what, int(differ.sum()), differ.numel(), share, dist[differ].max().item() if differ.any() else 0.0, int(d.max())))
    check(d.max().item() <= 1, '[3: float64 restatement] %s: a code differs by %d', what, int(d.max()))
    away = differ & (dist > tau)
    check(not away.any().item(), '[3: float64 restatement] %s: %d codes differ away from a rounding tie (tie distance up to '
          '%.3e codes, tau %s)', what, int(away.sum()), dist[away].max().item() if away.any() else 0.0,
          sorted(set(tau.flatten().tolist())))
    check(share <= TIE_CAP, '[3: float64 restatement] %s: %.4f%% of the codes differ', what, 100 * share)
    if case.get('samples_are_flat_codes'):
        check(torch.equal(codes, R.code(ref[k - 1] * 255.0 if fb else xs.double() * 255.0)),
              '[3: float64 restatement] %s: a flat image of exact codes changed', what)
    for j, (op, p) in enumerate(zip(ops, case['params'])):       # element-wise stages, from the GPU's own previous stage
        if op == OP_SKIP:
            continue
        want = R.elementwise(op, fused[k + j].double(), p[idx])
        try:
            assert_close(fused[k + j + 1], want, rtol=rtol[op], what='%s stage %d (%s)' % (what, k + j + 1, R.OP_NAMES[op]))
        except AssertionError as e:
            failed.append('[3: float64 restatement] %s' % e)
    for fam in set(f for f, _, _ in results):
        c = COUNTS.setdefault(fam, [0, 0.0])
        c[0] += 1
        c[1] = max(c[1], share)
    assert not failed, '%d checks failed:\n  %s' % (len(failed), '\n  '.join(failed))
    return results


# rtol of conftest.assert_close per element-wise op.  The sweep: the default 1e-4, and 2e-4 for WbQuadratic - its
# coefficients 10 p - 5 are formed in fp32 from the fp32 parameter (half an ulp of 10, 4.8e-7, on each of ten terms of
# magnitude up to 1), which the float64 restatement does not share.  The walk: 2e-4 for every op, the figure
# test_random_pointwise_ops_forward_and_gradients uses for all of them over the full parameter range.
RTOL_SWEEP = {OP_WB_MANUAL: 1e-4, OP_GAMMA: 1e-4, OP_GTM_MANUAL: 1e-4, OP_WB_QUADRATIC: 2e-4, OP_GAIN3: 1e-4}
RTOL_WALK = {op: 2e-4 for op in RTOL_SWEEP}


@pytest.mark.parametrize('index', range(len(CASES)), ids=lambda i: '-'.join(str(v) for v in CASES[i]).replace('/', '_'))
def test_sweep(index):
    case = sweep_case(index)
    case['samples_are_flat_codes'] = CASES[index][4] == 'constant'
    run_case(case, RTOL_SWEEP)
    print('cases per family so far [count, largest share of tie-excused codes]: %s' % COUNTS)


@pytest.mark.parametrize('seed', range(_FUZZ))
def test_random_walk(seed):
    run_case(walk_case(seed), RTOL_WALK)
    print('cases per family so far [count, largest share of tie-excused codes]: %s' % COUNTS)


@pytest.mark.parametrize('row', range(len(REFUSED)))
def test_refused_arguments_raise_before_any_launch(row):
    import reconfigisp_amd.functional as F
    (n, h, w), kind, mw, ops, exc = REFUSED[row]
    fb = kind == 'mosaic'
    x = torch.zeros(n, 1 if fb else 3, h, w).cuda()
    win = torch.full((n,), mw, dtype=torch.int32).cuda()
    sig = torch.full((n,), 10.0).cuda()
    par = [torch.full((n, R.PARAM_WIDTH.get(op, 0) or 1), 0.5).cuda() for op in ops]
    with pytest.raises(exc):
        F.BilateralChainPlan(x, fb, win, sig, sig, mw, ops, par).launch()


def test_mosaic_at_an_odd_float_offset_takes_the_single_float_form():
    """include/risp.h: the radius-1 forms read the mosaic in 8-byte (quad: 16-byte) vectors, so a mosaic with
    max_window 3 whose address is no multiple of 8 must not reach them: it runs in the run-time-radius form, which reads
    single floats, with the bits of the aligned call.  The same view under max_window 5 was never vectorised."""
    import reconfigisp_amd.functional as F
    index = [c[0] for c in CASES].index('9x30x68')             # windows 1 / 3, tail gamma -> WbQuadratic
    case = sweep_case(index)
    assert case['from_bayer'] and case['max_window'] == 3
    x = case['x'].cuda()
    buf = torch.zeros(x.numel() + 4, device='cuda')
    v = buf[1:1 + x.numel()].view(x.shape)
    v.copy_(x)
    assert x.data_ptr() % 16 == 0 and v.data_ptr() % 8 == 4 and v.is_contiguous()
    win, sc, ss = case['window'].cuda(), case['sc'].cuda(), case['ss'].cuda()
    params = [p.cuda() for p in case['params']]
    for mw in (3, 5):
        outs = []
        for src in (x, v):
            plan = F.BilateralChainPlan(src, True, win, sc, ss, mw, case['ops'], params)
            for o in plan.outs:
                o.fill_(float('nan'))
            outs.append([o.clone() for o in plan.launch()])
        for k, (a, b) in enumerate(zip(*outs)):
            assert not torch.isnan(b).any().item(), 'max_window %d stage %d: elements left unwritten' % (mw, k)
            assert torch.equal(a, b), 'max_window %d stage %d: %d elements differ' % (mw, k, (a != b).sum().item())
