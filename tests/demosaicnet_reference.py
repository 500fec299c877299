"""DemosaicNet (include/risp.h "DemosaicNet") restated in float64 torch on the CPU, in the released layout of
the public ``demosaicnet`` package (BayerDemosaick, Gharbi et al. 2016), plus the folded form the HIP path runs and the four kernel
stages on their own.  Plain F.conv2d / F.conv_transpose2d; differentiate with autograd.  The second half is the referee of
tests/test_gpu_demosaicnet_space.py: the folded network with hooks for the ReLU decisions, the comparison of one case (``judge``),
the case table, its branches and expected entries, and the wrong variants the rule must tell apart.  No GPU import."""
import numpy as np
import torch
import torch.nn.functional as Fn

from reconfigisp_amd import demosaicnet as DN

# CFA channel (0 R, 1 G, 2 B) of the site with row parity a, column parity b
PATTERNS = {'rggb': ((0, 1), (1, 2)), 'grbg': ((1, 0), (2, 1))}


def random_state_dict(seed, bias=0.05):
    """Random weights in the released layout at He scale (std sqrt(2 / fan_in)) so that activations survive the 17 ReLU layers;
    biases N(0, bias^2).  float64."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in DN.LAYOUT:
        if key.endswith('.bias'):
            sd[key] = torch.randn(shape, generator=g, dtype=torch.float64) * bias
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            if key.startswith('upsampler'):
                fan_in = 4                              # grouped: 4 input channels per output channel, one tap each
            sd[key] = torch.randn(shape, generator=g, dtype=torch.float64) * np.sqrt(2.0 / fan_in)
    return sd


def masked_mosaic(x, cfa='rggb'):
    """(N,3,H,W): x at each channel's own CFA sites, 0 elsewhere (RGB).  ``cfa``: a name, or the ((c00, c01), (c10, c11)) pattern"""
    n, _, h, w = x.shape
    pat = PATTERNS[cfa] if isinstance(cfa, str) else cfa
    m = torch.zeros((n, 3, h, w), dtype=x.dtype)
    for a in range(2):
        for b in range(2):
            m[:, pat[a][b], a::2, b::2] = x[:, 0, a::2, b::2]
    return m


def forward_rgb(x, sd, cfa='rggb', trace=None):
    """The released network on the mosaic x (N,1,H,W): RGB (N,3,H,W).  ``trace``: a list that receives (name, tensor) per layer."""
    mp = 'main_processor.'
    m3 = masked_mosaic(x, cfa)
    f = Fn.conv2d(m3, sd[mp + 'pack_mosaic.weight'], sd[mp + 'pack_mosaic.bias'], stride=2)
    if trace is not None:
        trace.append(('pack_mosaic', f))
    for i in range(1, 16):
        f = torch.relu(Fn.conv2d(f, sd[mp + 'conv%d.weight' % i], sd[mp + 'conv%d.bias' % i], padding=1))
        if trace is not None:
            trace.append(('conv%d' % i, f))
    r = Fn.conv2d(f[:, :64] * f[:, 64:], sd['residual_predictor.weight'], sd['residual_predictor.bias'])
    up = Fn.conv_transpose2d(r, sd['upsampler.weight'], sd['upsampler.bias'], stride=2, groups=3)
    h = torch.relu(Fn.conv2d(torch.cat([m3, up], 1), sd['fullres_processor.post_conv.weight'],
                             sd['fullres_processor.post_conv.bias'], padding=1))
    y = Fn.conv2d(h, sd['fullres_processor.output.weight'], sd['fullres_processor.output.bias'])
    if trace is not None:
        trace += [('residual', r), ('upsampled', up), ('post_conv', h), ('output', y)]
    return y


def reference(x, sd, cfa='rggb'):
    """The op of include/risp.h: BGR (N,3,H,W).  ``cfa`` names the mosaic the weights were trained on when x is read as such"""
    return forward_rgb(x, sd, cfa).flip(1)


def case_planes(table, h, w):
    """RISP_EPI_CASEBIAS: (cout,3,3) table -> (1,cout,h,w) planes, case 0 first row / column, 1 interior, 2 last"""
    cy = torch.ones(h, dtype=torch.long)
    cy[0], cy[-1] = 0, 2
    cx = torch.ones(w, dtype=torch.long)
    cx[0], cx[-1] = 0, 2
    return table[:, cy][:, :, cx].unsqueeze(0)


def folded_first(x, fd):
    """conv1 o pack_mosaic in the folded form (pre-ReLU): 3x3 on the space-to-depth planes + conv1's bias + the case planes"""
    p = Fn.pixel_unshuffle(x, 2)
    return Fn.conv2d(p, fd['conv1.weight'], fd['conv1.bias'], padding=1) + case_planes(fd['conv1.case'], p.shape[2], p.shape[3])


def tail_of(prod, fd):
    """up (N,3,H,W) from the gated features filters * masks"""
    r = Fn.conv2d(prod, fd['rp.weight'][:, :, None, None], fd['rp.bias'])
    return Fn.conv_transpose2d(r, fd['up.weight'].reshape(12, 1, 2, 2), fd['up.bias'], stride=2, groups=3)


def tail(fa, fb, fd):
    """up (N,3,H,W) from the post-ReLU halves of conv15"""
    return tail_of(fa * fb, fd)


def head_pre(x, up, fd, cfa='rggb'):
    """the head's hidden pre-activation (N,64,H,W): 3x3 on [masked mosaic, up] (``cfa``: the site pattern, always 'rggb' for a fold)"""
    return Fn.conv2d(torch.cat([masked_mosaic(x, cfa), up], 1), fd['post.weight'], fd['post.bias'], padding=1)


def head(x, up, fd):
    """y (N,3,H,W), output order of fd (BGR after the fold), from the mosaic and up"""
    h = torch.relu(head_pre(x, up, fd))
    return Fn.conv2d(h, fd['out.weight'][:, :, None, None], fd['out.bias'])


def body(x, fd):
    """(filters, masks): the post-ReLU halves of conv15"""
    f = torch.relu(folded_first(x, fd))
    for i in range(2, 16):
        f = torch.relu(Fn.conv2d(f, fd['conv%d.weight' % i], fd['conv%d.bias' % i], padding=1))
    return f[:, :64], f[:, 64:]


def folded_forward(x, fd):
    """the folded network (demosaicnet.fold) as the HIP path computes it: BGR"""
    fa, fb = body(x, fd)
    return head(x, tail(fa, fb, fd), fd)


def as_dtype(fd, dtype):
    return {k: v.to(dtype) for k, v in fd.items()}


# ------------------------------------------------------------------------------------------------ the referee of the network-level test
# tests/test_gpu_demosaicnet_space.py.  The rule is net_reference's: the float64 referee differentiates the folded network with
# every ReLU written as ``pre * m``, m = the DEVICE'S OWN decision as a constant, and checks separately (forward, every saved
# activation, against plain float64) that those decisions are legitimate.  Nothing is blanked.  One decision the device does not
# save: the head's hidden ReLU, which risp_dmnet_head_bwd recomputes from (x, up).  The referee decides it in float64 from the
# device's saved ``up``; a unit within TAU_HEAD of zero is UNDECIDED and both of its values are legitimate (``judge`` enumerates).
RELUS = 16                                            # hooks: conv1 .. conv14, conv15 as ONE 128-channel ReLU (the device runs it as two
#                                                       64-channel launches, filters and masks: its 17 ReLUs), the head's hidden layer
BAR = 1e-4                                            # the parity bar of BASELINE.json
# the largest error of the fp32 CPU restatement of the head's hidden pre-activation (``head_pre_chain``: bias, then the 54 taps in
# index order, one rounded multiply and one rounded add each) against float64 on the same fp32 (x, up), relative to max|pre|, over
# all rows of CASES (``up`` = float64's own, rounded to fp32) and KERNEL_CASES: per row 1.6e-7 .. 4.47e-7
# (tests/test_demosaicnet_cpu.py re-measures it) ...
HEAD_PRE_FP32_ERR = 4.5e-7
# ... and 4 x that: the kernel adds bias, mosaic taps and up channels in its own order and contracts to FMA - the factor is the margin
TAU_HEAD = 4 * HEAD_PRE_FP32_ERR
MAX_UNDECIDED = 4                                     # per case on the device: more FAILS the case
MAX_UNDECIDED_CPU = 2                                 # per row with the CPU's own ``up`` (float64's, and the fp32 restatement's)
MAX_PIXELS = 6144                                     # N H W of a row that differentiates: 393k hidden units, 3 .. 24 per million within TAU_HEAD of zero

WRONG = ('mask of the neighbouring layer', 'mask shifted by one pixel', 'filt for mask in the tail backward',
         'g_mask without [mask > 0]', 'upsampler dy / dx transposed', 'interior case on the border', 'first and last case swapped',
         'a border tap dropped from a backward pass', 'direct mosaic term dropped', 'wrong CFA channel on one phase',
         'BGR flip missing', 'grbg mirror on the 3x3 kernels only')


class _Relus:
    """net_reference._Relus for this network: the ReLUs of one evaluation in execution order; records every pre-activation; plain
    ``relu`` without masks, ``pre * m`` with the k-th mask as a constant otherwise.  ``bmasks`` (the wrong variants only): the
    VALUE keeps masks[k], the gradient takes bmasks[k]."""

    def __init__(self, masks, pre, bmasks=None):
        self.masks, self.pre, self.bmasks, self.k = masks, pre if pre is not None else [], bmasks, 0

    def __call__(self, t):
        k, self.k = self.k, self.k + 1
        self.pre.append(t)
        if self.masks is None:
            return torch.relu(t)
        if k >= len(self.masks):
            raise ValueError('ReLU %d has no mask: %d were given' % (k, len(self.masks)))
        m = self.masks[k]
        if tuple(m.shape) != tuple(t.shape):
            raise ValueError('mask %d is %s, its pre-activation %s' % (k, tuple(m.shape), tuple(t.shape)))
        m = m.to(t.dtype)
        out = t * m
        if self.bmasks is not None and self.bmasks[k] is not None:
            out = out + (t - t.detach()) * (self.bmasks[k].to(t.dtype) - m)
        return out

    def done(self):
        if self.k != RELUS or (self.masks is not None and len(self.masks) != self.k):
            raise ValueError('DemosaicNet has %d ReLUs, %d ran and %s masks were given' % (
                RELUS, self.k, 'no' if self.masks is None else len(self.masks)))


def _grad_from(value, other):
    """``value`` forward, the gradient of ``other`` backward"""
    return value.detach() + (other - other.detach())


def network(x, fd, masks=None, pre=None, bmasks=None, wrong=None):
    """(y, up) of the folded network with hooks.  Without masks it is ``folded_forward`` operation for operation.  ``wrong``: one of
    the WRONG variants that live inside the graph (tests/test_demosaicnet_cpu.py: the rule must tell each of them apart)."""
    relu = _Relus(masks, pre, bmasks)
    if wrong == 'interior case on the border':
        fd = dict(fd, **{'conv1.case': fd['conv1.case'][:, 1:2, 1:2].expand(-1, 3, 3)})
    elif wrong == 'first and last case swapped':
        fd = dict(fd, **{'conv1.case': fd['conv1.case'].flip(1, 2)})
    elif wrong == 'upsampler dy / dx transposed':
        fd = dict(fd, **{'up.weight': fd['up.weight'].reshape(12, 2, 2).transpose(1, 2).reshape(12, 4)})
    elif wrong == 'BGR flip missing':
        fd = dict(fd, **{'out.weight': fd['out.weight'].flip(0), 'out.bias': fd['out.bias'].flip(0)})
    f = relu(folded_first(x, fd))
    for i in range(2, 16):
        w = fd['conv%d.weight' % i]
        t = Fn.conv2d(f, w, fd['conv%d.bias' % i], padding=1)
        if wrong == 'a border tap dropped from a backward pass' and i == 8:
            # the backward-data pass of conv8 at column 0 misses the tap that reads the gradient of column 1 (ky = 1, kx = 0)
            wt = torch.zeros_like(w)
            wt[:, :, 1, 0] = w[:, :, 1, 0]
            col0 = torch.zeros_like(f)
            col0[..., 0] = 1
            t = _grad_from(t, t - Fn.conv2d(f * col0, wt, None, padding=1))
        f = relu(t)
    fa, fb = f[:, :64], f[:, 64:]
    if wrong == 'filt for mask in the tail backward':      # g_filt = (W_rp^T g_r) * FILT * [filt > 0]
        up = tail_of(_grad_from(fa * fb, fa.detach() * fb + 0.5 * fa * fa), fd)
    else:
        up = tail(fa, fb, fd)
    xh = x.detach() if wrong == 'direct mosaic term dropped' else x
    cfa = ((0, 1), (1, 0)) if wrong == 'wrong CFA channel on one phase' else 'rggb'      # the B site reads as R
    h = relu(head_pre(xh, up, fd, cfa))
    y = Fn.conv2d(h, fd['out.weight'][:, :, None, None], fd['out.bias'])
    relu.done()
    return y, up


def evaluate(x, fd, gy=None, masks=None, dtype=torch.float64, bmasks=None, wrong=None):
    """One evaluation in ``dtype``: {'y', 'pre' (the 16 pre-activations in execution order), 'up', and with ``gy``: 'gx'}.  ``masks``:
    one bool tensor per ReLU (see ``_Relus``)."""
    x = x.detach().to(dtype).requires_grad_(gy is not None)
    pre = []
    y, up = network(x, as_dtype(fd, dtype), masks, pre, bmasks, wrong)
    out = {'y': y.detach(), 'pre': [p.detach() for p in pre], 'up': up.detach()}
    if gy is not None:
        out['gx'], = torch.autograd.grad(y, x, gy.detach().to(dtype))
    return out


def saved_masks(saved):
    """the device's decisions of ReLUs 1-16 from ``y.grad_fn.saved_tensors`` = [x, conv1 .. conv14, fa, fb, up]: saved > 0"""
    saved = [t.detach().cpu() for t in saved]
    if len(saved) != 18:
        raise ValueError('%d tensors saved, [x, conv1 .. conv14, fa, fb, up] are 18' % len(saved))
    return [t > 0 for t in saved[1:15]] + [torch.cat([saved[15], saved[16]], 1) > 0]


def head_decisions(x, up, fd):
    """(mask, undecided) of the head's hidden ReLU in float64 from the fp32 (x, up): pre > 0, and |pre| <= TAU_HEAD max|pre|"""
    pre = head_pre(x.detach().cpu().double(), up.detach().cpu().double(), as_dtype(fd, torch.float64))
    return pre > 0, pre.abs() <= TAU_HEAD * pre.abs().max()


def head_pre_chain(x, up, fd):
    """the fp32 yardstick of the head's hidden pre-activation: bias, then the 54 taps in index order, one rounded multiply and one
    rounded add each (no library convolution: the same bits on every machine)"""
    x, up, fd = x.float(), up.float(), as_dtype(fd, torch.float32)
    planes = Fn.pad(torch.cat([masked_mosaic(x), up], 1), (1, 1, 1, 1))
    n, _, h, w = x.shape
    acc = fd['post.bias'].reshape(1, 64, 1, 1).expand(n, 64, h, w).clone()
    for c in range(6):
        for ky in range(3):
            for kx in range(3):
                acc = acc + fd['post.weight'][:, c, ky, kx].reshape(1, 64, 1, 1) * planes[:, c:c + 1, ky:ky + h, kx:kx + w]
    return acc


def head_pre_error(x, up, fd):
    """max|head_pre_chain - float64| / max|float64| on the same fp32 (x, up)"""
    ref = head_pre(x.float().double(), up.float().double(), as_dtype(fd, torch.float64))
    return float((head_pre_chain(x, up, fd).double() - ref).abs().max() / ref.abs().max())


def rel_err(got, ref):
    """max|got - ref| / max|ref| in float64; an all-zero reference asks for exact zeros (net_reference.rel_err)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if tuple(got.shape) != tuple(ref.shape):
        raise AssertionError('shape %s against %s' % (tuple(got.shape), tuple(ref.shape)))
    d, s = float((got - ref).abs().max()), float(ref.abs().max())
    if d != d:
        return float('inf')
    return d / s if s > 0 else (0.0 if d == 0 else float('inf'))


def judge(x, fd, dev, gy=None, yardstick=False):
    """The comparison of one case.  ``dev``: the device's {'y', and for a gradient: 'saved' (the 18 saved tensors), 'gx'}.  Returns
    {'rows': [(tensor, device error, fp32 yardstick or None)], 'flips', 'undecided'}; every error is max|got - ref64| / max|ref64|.
      rule 1: y, every saved activation and up against the PLAIN float64 evaluation;
      rule 2: gx against float64 autograd with the device's decisions.  With k undecided head units the legitimate gradients are
              g0 + sum_u s_u d_u, s in {0,1}^k (d_u: two backward passes that differ in unit u's mask only); the error is the
              smallest over the 2^k.  More than MAX_UNDECIDED units: AssertionError."""
    plain = evaluate(x, fd)
    p32 = evaluate(x, fd, dtype=torch.float32) if yardstick else None
    rows = [('y', rel_err(dev['y'], plain['y']), rel_err(p32['y'], plain['y']) if yardstick else None)]
    out = {'rows': rows, 'flips': 0, 'undecided': 0}
    if 'saved' not in dev:
        return out
    saved = [t.detach().cpu() for t in dev['saved']]
    masks = saved_masks(saved)
    acts = saved[1:15] + [torch.cat([saved[15], saved[16]], 1)]
    for k, act in enumerate(acts):
        rows.append(('act%d' % (k + 1), rel_err(act, torch.relu(plain['pre'][k])),
                     rel_err(torch.relu(p32['pre'][k]), torch.relu(plain['pre'][k])) if yardstick else None))
    rows.append(('up', rel_err(saved[17], plain['up']), rel_err(p32['up'], plain['up']) if yardstick else None))
    hmask, und = head_decisions(x, saved[17], fd)
    units = und.nonzero()
    out['undecided'] = len(units)
    assert len(units) <= MAX_UNDECIDED, '%d head units within %.1e of zero: at most %d' % (len(units), TAU_HEAD, MAX_UNDECIDED)
    base = hmask & ~und
    out['flips'] = (sum(int((m != (p > 0)).sum()) for m, p in zip(masks, plain['pre']))
                    + int(((hmask != (plain['pre'][15] > 0)) & ~und).sum()))       # decisions that differ from float64's own
    if gy is None:
        return out

    def span(dtype):
        g0 = evaluate(x, fd, gy, masks + [base], dtype)['gx']
        ds = []
        for u in units:
            on = base.clone()
            on[tuple(u.tolist())] = True
            ds.append(evaluate(x, fd, gy, masks + [on], dtype)['gx'] - g0)
        return g0, ds

    g0, ds = span(torch.float64)
    best, best_s = None, 0
    for s in range(1 << len(ds)):
        e = rel_err(dev['gx'], g0 + sum(d for j, d in enumerate(ds) if s >> j & 1))
        if best is None or e < best:
            best, best_s = e, s
    e32 = None
    if yardstick:
        h0, hs = span(torch.float32)
        pick = lambda a, b: a + sum(d for j, d in enumerate(b) if best_s >> j & 1)
        e32 = rel_err(pick(h0, hs), pick(g0, ds))
    rows.append(('gx', best, e32))
    return out


# ------------------------------------------------------------------------------------------------ the case table
# form, N, (H, W) of the mosaic, cfa, arith, input (net_reference.make_input).  Forms: 'grad'; 'infer' (autograd off, forward only);
# 'reuse' (the ``record`` dict).  Sizes for the code, not the workload - a head tile is 32 x 32 pixels, its backward region carries
# a 2-pixel halo, the body sees H/2 x W/2: (4, 4) a 2 x 2 plane (every pixel a border case, no k3, no matrix kernel); (4, 8) the
# smallest plane with W % 4 == 0; (8, 12), (36, 20) plane W % 4 != 0; (32, 32) one head tile exactly; (34, 66) 17 x 33 planes, 2-pixel
# tile remainders both ways; (66, 34) a tall strip; (40, 72) ragged, plane W % 4 == 0; (64, 96) 2 x 3 whole tiles.
# ``seed``: rows whose default seed (``case_seed``) leaves more than MAX_UNDECIDED_CPU head units undecided on the CPU name the first later
# seed that does not - a property of the input alone (float64 and the fp32 CPU restatement; tests/test_demosaicnet_cpu.py)
def _c(form, hw, n=2, cfa='rggb', arith='f16x2', inp='smooth', seed=None):
    return dict(form=form, hw=hw, n=n, cfa=cfa, arith=arith, input=inp, seed=seed)


CASES = [
    _c('grad', (4, 4)),
    _c('grad', (4, 4), n=3, cfa='grbg', arith='f32', inp='quantised'),
    _c('grad', (4, 8), inp='quantised'),
    _c('grad', (4, 8), arith='f32'),
    _c('grad', (8, 12), inp='constant'),
    _c('grad', (8, 12), arith='f32', inp='quantised'),
    _c('grad', (36, 20), n=3),
    _c('grad', (36, 20), cfa='grbg', arith='f32', inp='quantised'),
    _c('grad', (32, 32), seed=8137),
    _c('grad', (32, 32), cfa='grbg', arith='f32', inp='constant'),
    _c('grad', (34, 66), inp='quantised', seed=8172),
    _c('grad', (34, 66), arith='f32', inp='constant', seed=8190),
    _c('grad', (66, 34), arith='f32', seed=8206),
    _c('grad', (66, 34), cfa='grbg', inp='quantised', seed=8224),
    _c('grad', (40, 72), cfa='grbg', seed=8243),
    _c('grad', (40, 72), arith='f32', inp='quantised', seed=8263),
    _c('grad', (64, 96), n=1, inp='quantised', seed=8273),
    _c('grad', (64, 96), n=1, arith='f32'),
    _c('infer', (4, 4), inp='quantised'),
    _c('infer', (8, 12), arith='f32'),
    _c('infer', (34, 66), n=3, cfa='grbg'),
    _c('infer', (66, 34), n=1, arith='f32', inp='quantised'),
    _c('infer', (40, 72), arith='f32', inp='constant'),
    _c('infer', (64, 96)),
    _c('reuse', (36, 20)),
    _c('reuse', (32, 32), arith='f32', inp='constant'),
    _c('reuse', (40, 72), cfa='grbg', inp='quantised', seed=8447),
]
# the four risp_dmnet_* launches on their own (tail forward / backward, head forward / backward without and with ``add``), at the
# same sizes; N = 1 from (34, 66) on keeps the head-backward rows redrawable (``kernel_inputs``)
KERNEL_CASES = [dict(form='kernel', hw=hw, n=n, cfa='rggb', arith='f16x2', input='random', seed=seed)
                for hw, n, seed in (((4, 4), 3, None), ((4, 8), 2, None), ((8, 12), 2, None), ((36, 20), 2, None), ((32, 32), 2, None),
                                    ((34, 66), 1, None), ((66, 34), 1, None), ((40, 72), 1, None),
                                    ((64, 96), 1, 9000))]       # (its default seed finds an undecided unit in all 8 draws)
REDRAWS = 8


def case_id(case):
    return '%s-%dx%dx%d-%s-%s-%s' % ((case['form'], case['n']) + tuple(case['hw']) + (case['cfa'], case['arith'], case['input']))


def case_seed(case):
    if case['seed'] is not None:
        return case['seed']
    return 3000 + 17 * (CASES.index(case) if case['form'] != 'kernel' else 100 + KERNEL_CASES.index(case))


def case_inputs(case):
    """(sd, fd, x, gy) of a table row: the released-layout weights (float64), their fold as the device holds it (rounded to fp32 once,
    here as float64), the fp32 mosaic and a standard-normal fp32 upstream gradient"""
    import net_reference as NR
    seed, n, (h, w) = case_seed(case), case['n'], case['hw']
    sd = random_state_dict(seed)
    fd = {k: v.float().double() for k, v in DN.fold(sd, case['cfa']).items()}
    return sd, fd, NR.make_input(case['input'], n, 1, h, w, seed), NR.make_gy((n, 3, h, w), seed + 1001)


def kernel_inputs(case):
    """{'fd', 'x', 'fa', 'fb', 'up', 'gy', 'gup', 'add', 'draws'} of a kernel row, float64 holding fp32 values.  (x, up) are drawn
    again with the next seed, REDRAWS times at most, until float64 alone finds no undecided hidden unit - a property of the input
    (tests/test_demosaicnet_cpu.py), so the head-backward row compares every pixel."""
    seed, n, (h, w) = case_seed(case), case['n'], case['hw']
    g = torch.Generator().manual_seed(seed)
    r32 = lambda t: t.float().double()
    rand = lambda f, *s: r32(f(s, generator=g, dtype=torch.float64))
    out = {'fd': {k: r32(v) for k, v in DN.fold(random_state_dict(seed)).items()}}
    out['fa'], out['fb'] = torch.relu(rand(torch.randn, n, 64, h // 2, w // 2)), torch.relu(rand(torch.randn, n, 64, h // 2, w // 2))
    for name, c in (('gup', 3), ('gy', 3), ('add', 1)):
        out[name] = rand(torch.randn, n, c, h, w)
    for draw in range(REDRAWS):
        g = torch.Generator().manual_seed(seed + 1 + draw)
        out['x'], out['up'], out['draws'] = rand(torch.rand, n, 1, h, w), rand(torch.randn, n, 3, h, w), draw + 1
        if not head_decisions(out['x'], out['up'], out['fd'])[1].any():
            return out
    raise AssertionError('%s: an undecided head unit in each of %d draws' % (case_id(case), REDRAWS))


def expected_entries(case):
    """the ``risp_conv2d*`` entry of conv1, of the 15 body launches (conv2 .. conv14 and conv15's two halves) and of the backward
    passes, from shape predicates alone (tests/test_demosaicnet_cpu.py holds it against ``convnets.route`` / ``route_small``):
    {'conv1', 'body', 'body_bwd', 'join_bwd', 'conv1_bwd'}"""
    h, w = case['hw'][0] // 2, case['hw'][1] // 2
    quad = w % 4 == 0
    conv1 = 'risp_conv2d_k3' if quad and h >= 2 and w >= 2 else 'risp_conv2d'
    body = ('risp_conv2d_f16x2' if case['arith'] == 'f16x2' else 'risp_conv2d_wino43') if quad else 'risp_conv2d'
    # backward: EPI_MASK, and EPI_ADD | EPI_MASK with a full-width residual (add_c = 64 = the launch's cout), stay within every
    # kernel's epilogues; conv1's backward-data is a SmallConv (64 -> 4 planes, PixelShuffle store): the vector kernel, whose entry
    # point splits the input channels by the grid (risp_conv2d_small or risp_conv2d_small_split)
    return {'conv1': conv1, 'body': body, 'body_bwd': body, 'join_bwd': body, 'conv1_bwd': 'risp_conv2d_small'}


def expected_calls(case, backward=False):
    """``lib.CALLS`` of one forward (or one backward) restricted to risp_conv2d* (the two vector entries under one name)"""
    e, calls = expected_entries(case), {}
    for name, k in ((('body_bwd', 13), ('join_bwd', 2), ('conv1_bwd', 1)) if backward else (('conv1', 1), ('body', 15))):
        calls[e[name]] = calls.get(e[name], 0) + k
    return calls


_plane_w = lambda c: c['hw'][1] // 2
_net = lambda c: c['form'] != 'kernel'
_grad = lambda c: c['form'] in ('grad', 'reuse')
# the branches the table must reach: name -> predicate on a row of CASES + KERNEL_CASES
BRANCHES = {
    'conv1 on risp_conv2d_k3': lambda c: _net(c) and expected_entries(c)['conv1'] == 'risp_conv2d_k3',
    'conv1 on risp_conv2d (plane W % 4 != 0)': lambda c: _net(c) and expected_entries(c)['conv1'] == 'risp_conv2d' and _plane_w(c) > 2,
    'conv1 on a 2 x 2 plane: every pixel a border case': lambda c: _net(c) and c['hw'] == (4, 4),
    'body on risp_conv2d_f16x2': lambda c: c['form'] == 'grad' and expected_entries(c)['body'] == 'risp_conv2d_f16x2',
    'body on risp_conv2d_wino43': lambda c: c['form'] == 'grad' and expected_entries(c)['body'] == 'risp_conv2d_wino43',
    'body on risp_conv2d, split precision asked': lambda c: c['form'] == 'grad' and expected_entries(c)['body'] == 'risp_conv2d' and c['arith'] == 'f16x2',
    'body on risp_conv2d, fp32 asked': lambda c: c['form'] == 'grad' and expected_entries(c)['body'] == 'risp_conv2d' and c['arith'] == 'f32',
    'conv15 joined backward (EPI_ADD | EPI_MASK) on a ragged plane, f16x2': lambda c: c['form'] == 'grad' and c['hw'] == (40, 72) and c['arith'] == 'f16x2',
    'conv15 joined backward on a ragged plane, wino43': lambda c: c['form'] == 'grad' and c['hw'] == (40, 72) and c['arith'] == 'f32',
    'conv15 joined backward on a ragged plane, direct': lambda c: c['form'] == 'grad' and c['hw'] in ((34, 66), (66, 34), (36, 20)),
    'conv1 backward-data (EPI_SHUFFLE2) on one 2 x 2 plane': lambda c: _grad(c) and c['hw'] == (4, 4),
    'conv1 backward-data, odd plane sizes': lambda c: _grad(c) and c['hw'] == (34, 66),
    'head tiles with a 2-pixel remainder': lambda c: c['hw'] in ((34, 66), (66, 34)),
    'one head tile exactly': lambda c: c['hw'] == (32, 32),
    'several whole head tiles': lambda c: c['hw'] == (64, 96),
    'a batch of 3': lambda c: c['form'] == 'grad' and c['n'] == 3,
    'grbg, gradient': lambda c: c['form'] == 'grad' and c['cfa'] == 'grbg',
    'grbg, inference': lambda c: c['form'] == 'infer' and c['cfa'] == 'grbg',
    'grbg, reuse': lambda c: c['form'] == 'reuse' and c['cfa'] == 'grbg',
    'inference, split precision': lambda c: c['form'] == 'infer' and c['arith'] == 'f16x2',
    'inference, fp32': lambda c: c['form'] == 'infer' and c['arith'] == 'f32',
    'inference, plane W % 4 != 0': lambda c: c['form'] == 'infer' and _plane_w(c) % 4 != 0,
    'reuse': lambda c: c['form'] == 'reuse',
    'quantised input': lambda c: c['form'] == 'grad' and c['input'] == 'quantised',
    'constant image': lambda c: c['form'] == 'grad' and c['input'] == 'constant',
    'add= in risp_dmnet_head_bwd, ragged tiles': lambda c: c['form'] == 'kernel' and c['hw'] in ((34, 66), (66, 34)),
    'add= in risp_dmnet_head_bwd, one 4 x 4 image': lambda c: c['form'] == 'kernel' and c['hw'] == (4, 4),
    'tail kernels, plane W % 4 != 0': lambda c: c['form'] == 'kernel' and _plane_w(c) % 4 != 0,
}


def wrong_device(case, name):
    """What a device with defect ``name`` (WRONG) would hand to ``judge`` on a 'grad' row, computed in float64: {'y', 'saved', 'gx'};
    None where the defect cannot show (the grbg variant on an rggb row)."""
    sd, fd, x, gy = case_inputs(case)
    inside = name
    bm = None
    if name == 'grbg mirror on the 3x3 kernels only':
        if case['cfa'] != 'grbg':
            return None
        half = {k: (v.flip(-1) if k.endswith('.weight') and v.shape[-1] == 3 else v) for k, v in sd.items()}
        fd, inside = {k: v.float().double() for k, v in DN.fold(half).items()}, None
    own = evaluate(x, fd, wrong=inside)
    masks = [p > 0 for p in own['pre']]
    if name == 'mask of the neighbouring layer':          # conv7's backward reads conv8's saved activation
        bm, inside = [None] * RELUS, None
        bm[6] = masks[7]
    elif name == 'mask shifted by one pixel':
        bm, inside = [None] * RELUS, None
        bm[9] = torch.roll(masks[9], 1, dims=3)
    elif name == 'g_mask without [mask > 0]':
        bm, inside = [None] * RELUS, None
        bm[14] = torch.cat([masks[14][:, :64], torch.ones_like(masks[14][:, 64:])], 1)
    ev = evaluate(x, fd, gy, masks, bmasks=bm, wrong=inside)
    acts = [torch.relu(p) for p in own['pre'][:15]]
    return {'y': own['y'], 'gx': ev['gx'], 'saved': [x] + acts[:14] + [acts[14][:, :64], acts[14][:, 64:], own['up']]}


if __name__ == '__main__':
    # the He-scale generator keeps the activations alive through the 17 ReLU layers: RMS per layer
    x = torch.rand(2, 1, 48, 48, dtype=torch.float64)
    tr = []
    forward_rgb(x, random_state_dict(0), trace=tr)
    for name, t in tr:
        print('%-12s rms %.4f  nonzero %.3f' % (name, t.pow(2).mean().sqrt().item(), (t != 0).double().mean().item()))
