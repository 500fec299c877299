"""GPU: the fused training step (risp_chain_train_step, risp_train.hip) through its C ABI, over its argument space.

The launch geometry is bx = min(32, ceil(H*W/2 / 4096)) workgroups per image, 16 pixel pairs per thread, a grid-stride
loop beyond that, N * bx partial rows added by train_finish_kernel and ``for (n = lane; n < N; n += 64)`` for the rewritten
parameter blocks; two kernel instantiations (with and without a WbQuadratic stage).  Every case of the table below (and of
the seeded walk) builds the descriptor itself, pre-fills y, grad, loss and the scratch rows with NaN and is held to

  1. float64: y, loss, every stage's grad, exp_avg, exp_avg_sq, the update raw' - raw and every row of the rewritten blocks
     against tests/train_step_reference.py in float64 started from the SAME state, by conftest.ErrorBudget as
     test_gpu_error_budget.py uses it (ref32 = the restatement in float32);
  2. multi-step: 12 consecutive steps with the learning rate halved at step 6, statement 1 at every step, each step's
     reference started from the GPU's own state before it;
  3. ties under L1: the GPU's own output copied into the target at 30 % of the positions - gradient exactly 0 there;
  4. determinism: two calls from one state give the same bits in every output; y == NULL changes no other output;
  5. refusals: every argument the entry point rejects returns non-zero, names the cause, writes nothing.

The table, the builders and the walk are plain CPU code: tests/test_train_step_reference_cpu.py imports them to check the
coverage of the table and the conditioning rule (the restatement's own fp32 result within COND of its float64 result on
every judged tensor of every case) without a GPU.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import isp_oracle as O
import train_step_reference as R
from train_step_reference import OP_WB_MANUAL as WB, OP_GAMMA as GA, OP_GTM_MANUAL as GT, OP_WB_QUADRATIC as WQ

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------- the axes
PIPES = {
    'g': [GA],
    'q': [WQ],                                       # WbQuadratic alone
    'wb-g': [WB, GA],
    'q-g': [WQ, GA],                                 # ... first
    'wb-g-gtm': [WB, GA, GT],
    'wb-g-q': [WB, GA, WQ],                          # ... last (the pipeline of the reference golden, case a)
    'g-q-gtm': [GA, WQ, GT],                         # ... in the middle
    'q-g-gtm': [WQ, GA, GT],
    'g-g-gtm-q': [GA, GA, GT, WQ],
    'wb-wb-g-gtm-gtm': [WB, WB, GA, GT, GT],
    'wb-g-gtm-wb-g-gtm': [WB, GA, GT, WB, GA, GT],
    'wb-g-q-gtm-g-gtm': [WB, GA, WQ, GT, GA, GT],
}
SAMPLES = ('synthetic', 'uniform', 'constant')
FAMILIES = ('outputs', 'losses', 'param grads', 'first moments', 'second moments', 'updates', 'blocks')
BETAS, EPS, LR = (0.9, 0.99), 1e-8, 1e-2             # Adam as IspModel builds it (test_host_logic.isp_opt)
COND = 2e-5                                          # the conditioning rule: |ref32 - ref64| of every judged tensor
BX_MAX, PAIRS_PER_BLOCK = 32, 256 * 16
CLAMPED_MAX = 0.8


def launch_geometry(h, w):
    """(bx, trips of the pixel loop of the busiest thread) as risp_chain_train_step forms them"""
    pairs = h * w // 2
    bx = max(1, min(BX_MAX, -(-pairs // PAIRS_PER_BLOCK)))
    return bx, -(-pairs // (bx * 256))


def geometry_class(n, h, w):
    bx, trips = launch_geometry(h, w)
    pairs = h * w // 2
    if n == 64 and (h, w) == (256, 256):
        return 'headline'
    if bx == 1:
        if pairs == PAIRS_PER_BLOCK // 2 and n <= 3:
            return 'bx1-full'                        # 64 x 64: every thread busy, half of its 16 trips
        return 'bx1-idle' if n <= 2 else 'batch'     # small planes: threads without a pixel; many images
    if bx < BX_MAX:
        return 'ragged' if pairs % PAIRS_PER_BLOCK else 'bx8'
    return {16: 'bx32', 32: 'stride2'}.get(trips, 'stride8' if trips >= 128 else 'stride')


# name: (shape, pipeline, input, loss, samples, state, lr, seed).  state 'fresh': zero moments, step 1; 'resumed': moments
# and a step number as a checkpoint holds them.  The seed draws the samples and the parameters; a case that misses the
# conditioning rule gets another seed (test_train_step_reference_cpu.py::test_conditioning_rule), never a wider bound.
CASES = {
    # --- bx == 1, threads without a pixel
    'idle-a': ((1, 2, 2), 'g', 'bgr', 'mse', 'uniform', 'fresh', LR, 0),
    'idle-b': ((1, 2, 2), 'q', 'mosaic', 'l1', 'synthetic', 'resumed', LR, 200),
    'idle-c': ((2, 8, 8), 'wb-g', 'mosaic', 'l1', 'constant', 'fresh', LR, 2),
    'idle-d': ((2, 8, 8), 'q-g', 'bgr', 'mse', 'uniform', 'fresh', LR, 3),
    # --- bx == 1, every thread busy
    'full-a': ((3, 64, 64), 'wb-g-gtm', 'mosaic', 'mse', 'synthetic', 'fresh', LR, 4),
    'full-b': ((1, 64, 64), 'g-q-gtm', 'bgr', 'l1', 'synthetic', 'resumed', LR, 202),
    # --- 1 < bx < 32 with a ragged last workgroup; W % 4 != 0
    'ragged-a': ((2, 64, 130), 'g-g-gtm-q', 'mosaic', 'mse', 'synthetic', 'fresh', LR, 6),
    'ragged-b': ((2, 66, 258), 'wb-wb-g-gtm-gtm', 'bgr', 'l1', 'uniform', 'resumed', LR, 60),
    'ragged-c': ((1, 66, 258), 'wb-g-q-gtm-g-gtm', 'mosaic', 'l1', 'synthetic', 'fresh', LR, 8),
    'ragged-d': ((3, 64, 130), 'wb-g-gtm-wb-g-gtm', 'bgr', 'mse', 'synthetic', 'fresh', LR, 9),
    # --- whole workgroups
    'bx8-a': ((2, 256, 256), 'wb-g', 'mosaic', 'l1', 'uniform', 'fresh', LR, 10),
    'bx8-b': ((2, 256, 256), 'wb-g-q', 'bgr', 'mse', 'synthetic', 'resumed', LR, 60),
    'bx32-a': ((1, 512, 512), 'wb-g-gtm', 'bgr', 'mse', 'synthetic', 'resumed', LR, 60),
    'bx32-b': ((2, 512, 512), 'q-g', 'mosaic', 'l1', 'synthetic', 'fresh', LR, 203),
    # --- the grid-stride loop: 2 and 8 times the 16 trips of a full launch
    'stride2-a': ((1, 512, 1024), 'g', 'mosaic', 'mse', 'synthetic', 'fresh', LR, 14),
    'stride2-b': ((1, 512, 1024), 'q', 'bgr', 'l1', 'synthetic', 'fresh', LR, 201),
    'stride8-a': ((1, 1024, 2048), 'wb-g-gtm', 'mosaic', 'l1', 'synthetic', 'fresh', LR, 16),
    'stride8-b': ((1, 1024, 2048), 'wb-g-q', 'bgr', 'mse', 'synthetic', 'fresh', LR, 17),
    # --- the row loop of the finish kernel and the block rewrite on both sides of 64 images
    'batch-3': ((3, 8, 8), 'wb-g-q', 'mosaic', 'mse', 'synthetic', 'fresh', LR, 204),
    'batch-64a': ((64, 4, 4), 'wb-g-gtm', 'bgr', 'l1', 'uniform', 'fresh', LR, 19),
    'batch-64b': ((64, 4, 6), 'q-g', 'mosaic', 'mse', 'synthetic', 'fresh', LR, 202),
    'batch-65a': ((65, 4, 6), 'wb-g-gtm-wb-g-gtm', 'mosaic', 'mse', 'uniform', 'resumed', LR, 65),
    'batch-65b': ((65, 4, 4), 'g-g-gtm-q', 'bgr', 'l1', 'synthetic', 'fresh', LR, 22),
    'batch-70a': ((70, 2, 2), 'g', 'mosaic', 'l1', 'uniform', 'fresh', LR, 23),
    'batch-70b': ((70, 16, 18), 'wb-g-q-gtm-g-gtm', 'bgr', 'mse', 'synthetic', 'fresh', LR, 64),
    'batch-200a': ((200, 4, 4), 'wb-wb-g-gtm-gtm', 'mosaic', 'mse', 'synthetic', 'fresh', LR, 25),
    'batch-200b': ((200, 2, 4), 'g-q-gtm', 'bgr', 'l1', 'uniform', 'resumed', LR, 26),
    'batch-70x2': ((70, 64, 130), 'wb-g', 'bgr', 'mse', 'synthetic', 'fresh', LR, 27),     # 140 rows: bx == 2 AND N > 64
    # --- the batch the README quotes, once per instantiation
    'headline-a': ((64, 256, 256), 'wb-g-gtm', 'mosaic', 'mse', 'synthetic', 'fresh', LR, 28),
    'headline-b': ((64, 256, 256), 'wb-g-q', 'mosaic', 'l1', 'synthetic', 'fresh', LR, 29),
    # --- a saturated sigmoid: raw = -12 / +12 on two knots of the tone curve, (1 - s) * s = 6e-6.  The moments are a
    # checkpoint's: from zero moments the first update is lr * g / (|g| + eps) with |g| ~ eps, which no fp32 run resolves.
    # lr = 0.1: half an ulp of a raw value of 12 is 4.8e-7, which an update has to exceed 5e4 times to be judged to COND
    'saturated': ((2, 16, 18), 'wb-g-gtm', 'mosaic', 'mse', 'synthetic', 'resumed', 10 * LR, 30),
}
SATURATED = {'saturated': (2, [-12.0, 0.0, 12.0])}   # case: (stage, its raw parameter)
# (case, steps): the learning rate is halved at step HALVE_AT (MultiStepLR, gamma 0.5)
MULTI = ['ragged-d', 'batch-3']
MULTI_STEPS, HALVE_AT = 12, 6
# ties under L1: the last stage does not clamp (gamma) / clamps only outside the curve (tone curve)
TIES = {'tie-gamma': ((2, 64, 130), 'wb-g', 'bgr', 'l1', 'synthetic', 'fresh', LR, 40),
        'tie-gtm': ((3, 16, 18), 'q-g-gtm', 'mosaic', 'l1', 'synthetic', 'fresh', LR, 42)}
TIE_SHARE = 0.3

# The walk is sized for the default of 8 seeds.  Larger RISP_TEST_SEEDS run, but this file and its CPU companion are no
# soak target: with N(0, 0.3) on the raw parameters about 1 seed in 6 has a first draw outside COND (5 of 32 measured),
# and test_train_step_reference_cpu.py::test_conditioning_rule_walk fails, as it must, above 1 in 8.
_FUZZ = int(os.environ.get('RISP_TEST_SEEDS', '8'))
WALK_DRAWS = 12                                                   # parameter / sample draws a walk seed may take


# ---------------------------------------------------------------------------------------------------- builders (CPU)
def make_samples(kind, from_bayer, n, h, w, seed):
    """-> img (N,1,H,W) mosaic or (N,3,H,W) BGR, gt (N,3,H,W), float32"""
    rng = np.random.Generator(np.random.PCG64(seed))
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    if kind == 'synthetic':
        bay, gt = O.synthetic_raw(n, max(h, 16), max(w, 16), seed=seed)
        bay, gt = bay[:, :, :h, :w].contiguous(), gt[:, :, :h, :w].contiguous()
        if from_bayer:
            return bay, gt
        _, other = O.synthetic_raw(n, max(h, 16), max(w, 16), seed=seed + 7919)
        return gt, (0.5 * gt + 0.5 * other[:, :, :h, :w]).contiguous()
    gt = f32(rng.random((n, 3, h, w)))
    if kind == 'uniform':                            # both gates of the first clamp
        return f32(rng.uniform(-0.1, 1.2, size=(n, 1 if from_bayer else 3, h, w))), gt
    assert kind == 'constant'                        # one flat colour per image, on the knots of the tone curve too
    col = f32(rng.choice([0.25, 0.5, 0.75, 0.3, 0.61], size=(n, 3)))
    bgr = col.view(n, 3, 1, 1).expand(n, 3, h, w).contiguous()
    if not from_bayer:
        return bgr, gt
    bay = torch.empty(n, 1, h, w)
    bay[:, 0, 0::2, 0::2] = bgr[:, 2, 0::2, 0::2]
    bay[:, 0, 0::2, 1::2] = bgr[:, 1, 0::2, 1::2]
    bay[:, 0, 1::2, 0::2] = bgr[:, 1, 1::2, 0::2]
    bay[:, 0, 1::2, 1::2] = bgr[:, 0, 1::2, 1::2]
    return bay, gt


def make_state(ops, kind, rng):
    """raw parameters N(0, 0.3) around the constructor's values (O.PARAM_INIT); the Adam state of a fresh optimiser or
    of a checkpoint -> dict(raw, exp_avg, exp_avg_sq, step) with step the number of the NEXT step"""
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    raw = [f32(np.asarray(O.PARAM_INIT[R.OP_NAMES[op]]) + 0.3 * rng.standard_normal(R.PARAM_WIDTH[op])) for op in ops]
    if kind == 'fresh':
        return dict(raw=raw, exp_avg=[torch.zeros_like(r) for r in raw], exp_avg_sq=[torch.zeros_like(r) for r in raw], step=1)
    assert kind == 'resumed'
    # a state Adam can be in: |exp_avg| around 1e-3, exp_avg_sq between its square and four times it
    m = [f32(1e-3 * np.exp(rng.uniform(-1, 1, size=r.numel())) * rng.choice([-1.0, 1.0], size=r.numel())) for r in raw]
    v = [f32(np.square(a.double().numpy()) * rng.uniform(1.0, 4.0, size=a.numel())) for a in m]
    return dict(raw=raw, exp_avg=m, exp_avg_sq=v, step=int(rng.integers(2, 40)))


def build_case(name, row, draw=0):
    (n, h, w), pipe, kind, loss, samples, state, lr, seed = row
    ops = list(PIPES[pipe]) if isinstance(pipe, str) else list(pipe)
    img, gt = make_samples(samples, kind == 'mosaic', n, h, w, seed=3000 + 16 * seed + draw)
    st = make_state(ops, state, np.random.Generator(np.random.PCG64(7000 + 16 * seed + draw)))
    if name in SATURATED:
        k, vals = SATURATED[name]
        st['raw'][k] = torch.tensor(vals, dtype=torch.float32)
    return dict(name=name, n=n, h=h, w=w, ops=ops, from_bayer=kind == 'mosaic', loss_kind=R.LOSS_MSE if loss == 'mse' else R.LOSS_L1,
                img=img, gt=gt, state=st, lr=lr, geometry=geometry_class(n, h, w), wbq=WQ in ops,
                what='%s [%s] %dx%dx%d %s %s %s %s %s' % (name, geometry_class(n, h, w), n, h, w, kind, pipe if isinstance(pipe, str)
                                                         else '-'.join(R.OP_NAMES[o] for o in ops), loss, samples, state))


def table_case(name):
    return build_case(name, CASES[name])


def tie_case(name):
    return build_case(name, TIES[name])


def tie_mask(case):
    g = torch.Generator().manual_seed(97)
    return torch.rand((case['n'], 3, case['h'], case['w']), generator=g) < TIE_SHARE


def lr_at(case, step_index):
    """the learning rate of the step_index-th step (0-based) of a MULTI run"""
    return case['lr'] * (0.5 if step_index + 1 >= HALVE_AT else 1.0)


def reference_pair(case, state, lr, zero_grad_at=None):
    """the restatement in float32 and float64 from ``state`` -> (ref32, ref64), each the 7-tuple of reference_step"""
    args = (case['ops'], case['from_bayer'], case['loss_kind'], case['img'], case['gt'], state['raw'], state['exp_avg'],
            state['exp_avg_sq'], state['step'], lr, BETAS, EPS)
    return (R.reference_step(*args, dtype=torch.float32, zero_grad_at=zero_grad_at),
            R.reference_step(*args, dtype=torch.float64, zero_grad_at=zero_grad_at))


def judged(state, out):
    """[(family, label, tensor)] of one step: ``out`` is a 7-tuple as reference_step returns it"""
    y, loss, grads, raw, m, v, blocks = out
    rows = [('outputs', 'y', y), ('losses', 'loss', loss.reshape(1))]
    for k in range(len(grads)):
        rows += [('param grads', 'grad %d' % k, grads[k]), ('first moments', 'exp_avg %d' % k, m[k]),
                 ('second moments', 'exp_avg_sq %d' % k, v[k]),
                 ('updates', 'update %d' % k, raw[k].double() - state['raw'][k].double()), ('blocks', 'blocks %d' % k, blocks[k])]
    return rows


def conditioning(case, state, lr, zero_grad_at=None, pair=None):
    """the largest |ref32 - ref64| / max|ref64| over the judged tensors of one step, and its label"""
    r32, r64 = pair or reference_pair(case, state, lr, zero_grad_at)
    worst = (0.0, '')
    for (_, label, a), (_, _, b) in zip(judged(state, r32), judged(state, r64)):
        scale = b.abs().max().item() or 1.0
        worst = max(worst, ((a.double() - b.double()).abs().max().item() / scale, label))
    return worst


def clamped_share(out):
    """the share of the outputs on a clamp (0 or 1): no gradient flows through those, and a case that is all clamp tests
    nothing behind its last clamping stage.  The table and the walk keep it under CLAMPED_MAX and every stage's gradient
    away from exactly 0 (checked on the float64 restatement; a case that misses is drawn again, as for COND)."""
    return ((out[0] <= 0) | (out[0] >= 1)).double().mean().item()


def alive(out):
    return clamped_share(out) <= CLAMPED_MAX and all(g.abs().max().item() > 0 for g in out[2])


def next_state(state, out):
    return dict(raw=[t.float() for t in out[3]], exp_avg=[t.float() for t in out[4]], exp_avg_sq=[t.float() for t in out[5]],
                step=state['step'] + 1)


def walk_case(seed):
    """One step of the seeded walk: N 1 .. 5, planes up to 96 x 160 (bx 1 .. 2), pipelines of 1 .. 6 stages with at most
    one WbQuadratic, both inputs, losses and states, every sample family.  The samples and parameters of a seed are drawn
    again (at most WALK_DRAWS times) until the restatement's own fp32 result lies within COND of its float64 result and the
    case is alive (clamped_share) - properties of the draw and the restatement alone; test_train_step_reference_cpu.py
    fails if a seed runs out of draws or more than 1 seed in 8 misses COND at all."""
    rng = np.random.default_rng(9100 + seed)
    n, h, w = int(rng.integers(1, 6)), 2 * int(rng.integers(1, 49)), 2 * int(rng.integers(1, 81))
    ops = [int(rng.choice([WB, GA, GT])) for _ in range(int(rng.integers(1, 7)))]
    if rng.random() < 0.5:
        ops[int(rng.integers(0, len(ops)))] = WQ
    row = ((n, h, w), ops, 'mosaic' if rng.random() < 0.5 else 'bgr', 'mse' if rng.random() < 0.5 else 'l1',
           SAMPLES[int(rng.integers(0, 3))], 'fresh' if rng.random() < 0.5 else 'resumed', LR, 100 + seed)
    worst, missed = None, 0
    for draw in range(WALK_DRAWS):
        case = build_case('walk-%d' % seed, row, draw)
        case['pair'] = reference_pair(case, case['state'], case['lr'])
        worst = conditioning(case, case['state'], case['lr'], pair=case['pair'])
        missed += worst[0] > COND
        if worst[0] <= COND and alive(case['pair'][1]):
            case['draws'], case['missed_cond'] = draw + 1, missed
            return case
    raise AssertionError('%s: no draw within the conditioning rule in %d (last: %.2e on %s)' % (case['what'], WALK_DRAWS, *worst))


# ---------------------------------------------------------------------------------------------------- the kernel (GPU)
NAN = float('nan')


class Runner:
    """Device buffers of one case and the descriptor over them, every field under the test's control."""

    def __init__(self, case):
        from reconfigisp_amd import lib as L
        self.L, self.case = L, case
        n, h, w = case['n'], case['h'], case['w']
        self.img, self.gt = case['img'].cuda().contiguous(), case['gt'].cuda().contiguous()
        self.y = torch.empty(n, 3, h, w, device='cuda')
        self.loss = torch.empty(1, device='cuda')
        self.scratch = torch.empty(L.load().risp_train_scratch_floats(n), device='cuda')
        widths = [R.PARAM_WIDTH[op] for op in case['ops']]
        new = lambda: [torch.empty(p, device='cuda') for p in widths]
        self.raw, self.m, self.v, self.grad = new(), new(), new(), new()
        self.blocks = [torch.empty(n, p, device='cuda') for p in widths]

    def load_state(self, state):
        """parameters and moments from a CPU state; the per-image blocks as FusedIspStep._make_plan builds them"""
        for k, op in enumerate(self.case['ops']):
            self.raw[k].copy_(state['raw'][k]), self.m[k].copy_(state['exp_avg'][k]), self.v[k].copy_(state['exp_avg_sq'][k])
            self.blocks[k].copy_(R.blocks_of(op, self.raw[k], self.case['n']))

    def state(self, step):
        cpu = lambda ts: [t.detach().cpu().clone() for t in ts]
        return dict(raw=cpu(self.raw), exp_avg=cpu(self.m), exp_avg_sq=cpu(self.v), step=step)

    def desc(self, step, lr, with_y=True):
        from reconfigisp_amd import functional as F
        c, d = self.case, self.L.TrainDesc()
        d.in_, d.gt, d.y = F._p(self.img), F._p(self.gt), F._p(self.y) if with_y else None
        d.from_bayer, d.n_ops, d.loss_kind = int(c['from_bayer']), len(c['ops']), c['loss_kind']
        for k, op in enumerate(c['ops']):
            d.ops[k] = op
            d.blocks[k], d.raw[k], d.grad[k] = self.blocks[k].data_ptr(), self.raw[k].data_ptr(), self.grad[k].data_ptr()
            d.exp_avg[k], d.exp_avg_sq[k] = self.m[k].data_ptr(), self.v[k].data_ptr()
        d.N, d.H, d.W = c['n'], c['h'], c['w']
        beta1, beta2 = BETAS                                     # the step-dependent fields as train_step.py forms them
        d.lr_step = lr / (1.0 - beta1 ** step)
        d.beta1, d.beta2, d.bias2_sqrt, d.eps = beta1, beta2, math.sqrt(1.0 - beta2 ** step), EPS
        d.one_minus_beta1, d.one_minus_beta2 = 1.0 - beta1, 1.0 - beta2
        d.loss, d.scratch = F._p(self.loss), F._p(self.scratch)
        return d

    def prefill(self):
        for t in [self.y, self.loss, self.scratch] + self.grad:
            t.fill_(NAN)

    def outputs_untouched(self):
        torch.cuda.synchronize()
        return all(torch.isnan(t).all().item() for t in [self.y, self.loss, self.scratch] + self.grad)

    def step(self, step, lr, with_y=True):
        """one call -> the 7-tuple of reference_step (CPU tensors), y None without an output buffer"""
        from reconfigisp_amd import functional as F
        self.prefill()
        d = self.desc(step, lr, with_y)
        self.L.call('risp_chain_train_step', C.byref(d), F._stream())
        torch.cuda.synchronize()
        cpu = lambda ts: [t.detach().cpu().clone() for t in ts]
        if not with_y:
            assert torch.isnan(self.y).all().item(), 'y == NULL: the output buffer of an earlier call was written'
        return (self.y.cpu().clone() if with_y else None, self.loss.cpu().clone()[0], cpu(self.grad), cpu(self.raw), cpu(self.m),
                cpu(self.v), cpu(self.blocks))


def _flat(out):
    y, loss, grads, raw, m, v, blocks = out
    named = [('loss', loss)] + ([('y', y)] if y is not None else [])
    for name, ts in (('grad', grads), ('raw', raw), ('exp_avg', m), ('exp_avg_sq', v), ('blocks', blocks)):
        named += [('%s %d' % (name, k), t) for k, t in enumerate(ts)]
    return named


def assert_same_bits(a, b, what, skip_y=False):
    fa, fb = dict(_flat(a)), dict(_flat(b))
    for key in fa:
        if key == 'y' and (skip_y or key not in fb):
            continue
        assert torch.equal(fa[key].view(torch.int32), fb[key].view(torch.int32)), '%s: %s differs in bits' % (what, key)


def judge(case, state, got, lr, zero_grad_at=None, pair=None, tag=''):
    """statement 1 for one step: ``got`` against the restatement started from ``state``"""
    from conftest import ErrorBudget
    what = case['what'].split(' ')[0] + ' ' + case['what'].split(' ')[1] + tag
    for label, t in _flat(got):
        assert torch.isfinite(t).all().item(), '%s: %s holds NaN / inf (elements left unwritten)' % (case['what'] + tag, label)
    blocks = got[6]
    for k, b in enumerate(blocks):                               # .repeat(N, 1): every image reads the same parameters
        assert torch.equal(b, b[:1].expand_as(b)), '%s: blocks of stage %d differ between images (rows %s)' % (
            case['what'] + tag, k, (b != b[:1]).any(dim=1).nonzero().flatten().tolist()[:8])
    r32, r64 = pair or reference_pair(case, state, lr, zero_grad_at)
    budget = ErrorBudget()
    for (family, label, a), (_, _, b), (_, _, c) in zip(judged(state, got), judged(state, r32), judged(state, r64)):
        budget(a, b, c, '%s %s' % (what, label), family)
    budget.finish()


def run_table_case(case):
    run = Runner(case)
    st = case['state']
    run.load_state(st)
    first = run.step(st['step'], case['lr'])
    judge(case, st, first, case['lr'], pair=case.get('pair'))
    run.load_state(st)                                           # statement 4: the same state again, then without y
    again = run.step(st['step'], case['lr'])
    assert_same_bits(first, again, case['what'] + ': second call')
    run.load_state(st)
    without = run.step(st['step'], case['lr'], with_y=False)
    assert_same_bits(first, without, case['what'] + ': y == NULL', skip_y=True)


@pytest.mark.parametrize('name', list(CASES))
def test_table(name):
    run_table_case(table_case(name))


@pytest.mark.parametrize('seed', range(_FUZZ))
def test_random_walk(seed):
    run_table_case(walk_case(seed))


@pytest.mark.parametrize('name', MULTI)
def test_twelve_steps_from_the_gpus_own_state(name):
    case = table_case(name)
    run = Runner(case)
    run.load_state(case['state'])                                # the blocks of later steps are the kernel's own
    step = case['state']['step']
    twin = Runner(case)                                          # statement 4 along the way
    twin.load_state(case['state'])
    for i in range(MULTI_STEPS):
        before = run.state(step)
        lr = lr_at(case, i)
        got = run.step(step, lr)
        judge(case, before, got, lr, tag=' step %d' % (i + 1))
        assert_same_bits(got, twin.step(step, lr), '%s step %d: a second run' % (case['what'], i + 1))
        step += 1
    assert lr_at(case, 0) == 2 * lr_at(case, MULTI_STEPS - 1)


@pytest.mark.parametrize('name', list(TIES))
def test_l1_ties_have_gradient_zero(name):
    case = tie_case(name)
    assert case['loss_kind'] == R.LOSS_L1 and case['ops'][-1] in (GA, GT)
    run, st = Runner(case), case['state']
    run.load_state(st)
    y = run.step(st['step'], case['lr'])[0]                      # the forward: its state is thrown away
    mask = tie_mask(case)
    case['gt'] = torch.where(mask, y, case['gt'])
    run = Runner(case)
    run.load_state(st)
    got = run.step(st['step'], case['lr'])
    assert torch.equal(got[0], y) and torch.equal(got[0][mask], case['gt'][mask])
    judge(case, st, got, case['lr'], zero_grad_at=mask)
    # what the statement is worth: a kernel that returned +- 1 / count at the ties would be this far off
    _, r64 = reference_pair(case, st, case['lr'], zero_grad_at=mask)
    _, off = reference_pair(case, st, case['lr'])
    moved = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(off[2], r64[2]))
    assert moved > 1e-2, 'the ties do not move the gradient (%g): the case cannot tell sign(0) = 0 from +-1' % moved


# ---------------------------------------------------------------------------------------------------- refusals
def _set(field, value):
    def edit(d, run):
        setattr(d, field, value)
    return edit


def _stage(field, k, value):
    def edit(d, run):
        getattr(d, field)[k] = value
    return edit


def _ops(ops):
    def edit(d, run):
        d.n_ops = len(ops)
        for k, op in enumerate(ops):
            d.ops[k] = op
            for field in ('blocks', 'raw', 'grad', 'exp_avg', 'exp_avg_sq'):      # every stage complete (and 30 wide): only the
                getattr(d, field)[k] = getattr(d, field)[1]                       # ops are wrong
    return edit


# name: (edit of a valid descriptor of 2 x 4 x 4, gamma -> WbQuadratic; what risp_last_error() must name).  The buffers
# stay those of the valid call, so a check that let one of these through would still run inside them - except the
# shapes, which are therefore only ever SMALLER than the buffers (N = 65536 gets buffers of its own).
REFUSED = {
    'null in': (_set('in_', None), 'null tensor'), 'null gt': (_set('gt', None), 'null tensor'),
    'null loss': (_set('loss', None), 'null tensor'), 'null scratch': (_set('scratch', None), 'null tensor'),
    'odd H': (_set('H', 3), 'H, W must be even'), 'odd W': (_set('W', 3), 'H, W must be even'),
    'N = 0': (_set('N', 0), 'bad shape'), 'N = 65536': (_set('N', 65536), 'bad shape'),
    'no stage': (_set('n_ops', 0), 'stages'), 'seven stages': (_set('n_ops', 7), 'stages'),
    'two WbQuadratic': (_ops([WQ, GA, WQ]), 'at most one WbQuadratic'),
    'op SKIP': (_ops([GA, R.OP_SKIP]), 'no fused training form'),
    'op DEMOSAIC_NEAREST': (_ops([R.OP_DEMOSAIC_NEAREST, GA]), 'no fused training form'),
    'op GAIN3': (_ops([GA, R.OP_GAIN3]), 'no fused training form'), 'op 99': (_ops([99]), 'no fused training form'),
    'loss kind 2': (_set('loss_kind', 2), 'loss kind'),
}
for _field in ('blocks', 'raw', 'grad', 'exp_avg', 'exp_avg_sq'):
    REFUSED['stage 1 without %s' % _field] = (_stage(_field, 1, None), 'stage 1 incomplete')


def _refusal_case(n=2):
    return build_case('refusal', ((n, 4, 4), [GA, WQ], 'bgr', 'mse', 'uniform', 'fresh', LR, 50))


@pytest.mark.parametrize('name', ['null descriptor'] + list(REFUSED))
def test_refused_arguments_return_before_any_launch(name):
    from reconfigisp_amd import functional as F
    case = _refusal_case()
    if name == 'N = 65536':                                      # buffers as large as the refused call would need
        case.update(n=65536, img=case['img'][:1].expand(65536, 3, 4, 4), gt=case['gt'][:1].expand(65536, 3, 4, 4))
    run = Runner(case)
    run.load_state(case['state'])
    before = run.state(1), [b.clone() for b in run.blocks]
    run.prefill()
    fn = run.L.load().risp_chain_train_step
    if name == 'null descriptor':
        status, needle = fn(None, F._stream()), 'null descriptor'
    else:
        edit, needle = REFUSED[name]
        d = run.desc(1, LR)
        d.N = 2                                                  # the shape of the valid call; the edit changes what it names
        edit(d, run)
        status = fn(C.byref(d), F._stream())
    message = run.L.load().risp_last_error().decode()
    assert status != 0, '%s was accepted' % name
    assert 'risp_chain_train_step' in message and needle in message, '%s: "%s" does not name the cause' % (name, message)
    assert run.outputs_untouched(), '%s: an output was written' % name
    after = run.state(1)
    for key in ('raw', 'exp_avg', 'exp_avg_sq'):
        assert all(torch.equal(a, b) for a, b in zip(before[0][key], after[key])), '%s: %s changed' % (name, key)
    assert all(torch.equal(a, b) for a, b in zip(before[1], run.blocks)), '%s: the blocks changed' % name
    # and the entry point is not left in a state that refuses a valid call
    run.load_state(case['state'])
    if case['n'] == 2:
        judge(case, case['state'], run.step(1, LR), LR)
