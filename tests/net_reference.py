"""The referee of the network-level tests (tests/test_gpu_net_space.py): dtype-generic restatements of the four proxy families
with hooks for the ReLU decisions, the seeded inputs and the case table.  Plain CPU code, no GPU import.

Why hooks.  A dense input gradient of two implementations cannot be compared at random weights: a pre-activation within rounding of
zero is clipped by one and passed by the other, and everything behind that decision differs by O(1).  Given the decisions the
backward pass is linear.  So the float64 referee

  1. compares the forward (the output and every post-ReLU activation the device saved) with a plain float64 evaluation - which
     confines a flipped decision to pre-activations within the forward bar of zero;
  2. differentiates the same network with every ReLU written as ``pre * m``, m = (the device's saved activation of that very layer
     > 0) as a constant - a mask taken from the wrong layer, shifted or packed wrongly is an O(1) error, and nothing is blanked;
  3. holds the saved argmin / argmax of SRCNNRes' statistics to their contract exactly (``check_arg``) and scatters the min / max
     plane gradients at the device's indices (``torch.min`` on ties is not a specification).

With no masks and no indices given the restatements are oracle/isp_oracle.py's ``srcnn_res``, ``srcnn_demosaic``, ``path14l_bayer``
and ``path14l_bgr`` operation for operation (tests/test_net_reference_cpu.py holds them to ``torch.equal``)."""
import numpy as np
import torch
import torch.nn.functional as TF

import isp_oracle as O

BAR = 1e-4                                           # the parity bar of BASELINE.json, the cap of conftest.ErrorBudget
FAMILY_P = (2, 1, 2, 1, 3, 1, 3, 5)                  # the SRCNNRes family of an sRGB slot (tests/test_gpu_group.py)
PAIR_P = (1, 3)
KINDS = ('srcnn_res', 'srcnn_demosaic', 'path14l_bayer', 'path14l_bgr')
RELUS = {'srcnn_res': 2, 'srcnn_demosaic': 2, 'path14l_bayer': 13, 'path14l_bgr': 13}      # per network, in execution order


class _Relus:
    """the ReLUs of one evaluation in execution order: records every pre-activation; plain ``relu`` without masks, ``pre * m``
    with the k-th mask as a constant otherwise"""

    def __init__(self, masks, pre):
        self.masks, self.pre = masks, pre if pre is not None else []
        self.k = 0

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
        return t * m.to(t.dtype)

    def done(self, kind):
        if self.k != RELUS[kind] or (self.masks is not None and len(self.masks) != self.k):
            raise ValueError('%s has %d ReLUs, %d ran and %s masks were given' % (
                kind, RELUS[kind], self.k, 'no' if self.masks is None else len(self.masks)))


def srcnn_res(x, param_vec, wts, masks=None, arg=None, pre=None):
    """oracle ``srcnn_res``.  ``arg`` (N,3,2) = the flat (row-major) index of each plane's min and max: the two statistics are then
    read - and differentiated - at these pixels"""
    relu = _Relus(masks, pre)
    n, _, h, w = x.shape
    if arg is None:
        fmin = x.min(dim=3)[0].min(dim=2)[0]
    else:
        flat, idx = x.flatten(2), arg.to(torch.int64)
        fmin = flat.gather(2, idx[..., 0:1]).squeeze(2)
    fmean = x.mean(dim=3).mean(dim=2)
    if arg is None:
        fmax = x.max(dim=3)[0].max(dim=2)[0]
    else:
        fmax = flat.gather(2, idx[..., 1:2]).squeeze(2)
    feat = torch.cat([fmin, fmean, fmax, param_vec], dim=1)
    fin = torch.cat([x, feat[:, :, None, None].expand(-1, -1, h, w)], dim=1)
    t = relu(O._conv(fin, wts['srcnn.0.weight'], wts['srcnn.0.bias'], 4))
    t = relu(O._conv(t, wts['srcnn.2.weight'], wts['srcnn.2.bias'], 2))
    relu.done('srcnn_res')
    return x + O._conv(t, wts['srcnn.4.weight'], wts['srcnn.4.bias'], 2)


def srcnn_demosaic(x, wts, masks=None, pre=None):
    relu = _Relus(masks, pre)
    t = O.bayer_to_rggb(x)
    t = relu(O._conv(t, wts['srcnn.0.weight'], wts['srcnn.0.bias'], 4))
    t = relu(O._conv(t, wts['srcnn.2.weight'], wts['srcnn.2.bias'], 0))
    relu.done('srcnn_demosaic')
    return O.pixel_shuffle2(O._conv(t, wts['srcnn.4.weight'], wts['srcnn.4.bias'], 2))


def _path14l_body(t, wts, relu):
    """oracle ``_path14l_body``; the 13 ReLUs in execution order are r0, u0, r1, u1, ..., u5, r6 - the order in which
    ``convnets._Path14l`` saves its activations"""
    p = 'path_restore_14l.'
    t = O._conv(t, wts[p + '0.weight'], wts[p + '0.bias'], 1)
    for k in range(6):
        r = relu(t)
        u = relu(O._conv(r, wts[p + '1.%d.basic.1.weight' % k], wts[p + '1.%d.basic.1.bias' % k], 1))
        t = O._conv(u, wts[p + '1.%d.basic.3.weight' % k], wts[p + '1.%d.basic.3.bias' % k], 1) + r
    return O._conv(relu(t), wts[p + '3.weight'], wts[p + '3.bias'], 1)


def path14l_bayer(x, wts, masks=None, pre=None):
    relu = _Relus(masks, pre)
    y = O.pixel_shuffle2(_path14l_body(O.bayer_to_rggb(x), wts, relu))
    relu.done('path14l_bayer')
    return y


def path14l_bgr(x, wts, masks=None, pre=None):
    relu = _Relus(masks, pre)
    y = _path14l_body(x[:, [2, 1, 0]], wts, relu)[:, [2, 1, 0]]
    relu.done('path14l_bgr')
    return y


def forward(kind, x, pv, wts, masks=None, arg=None, pre=None):
    if kind == 'srcnn_res':
        return srcnn_res(x, pv if pv is not None else x.new_zeros((x.shape[0], 0)), wts, masks, arg, pre)
    if arg is not None:
        raise ValueError('%s has no statistics' % kind)
    return {'srcnn_demosaic': srcnn_demosaic, 'path14l_bayer': path14l_bayer, 'path14l_bgr': path14l_bgr}[kind](x, wts, masks, pre)


def evaluate(kind, x, pv, wts, gy=None, masks=None, arg=None, dtype=torch.float64, weight_grads=False):
    """One evaluation in ``dtype``: {'y', 'pre' (the pre-activations in execution order), and with ``gy``: 'gx', 'gpv' (None without
    parameters), 'gw' (name -> gradient, with ``weight_grads``)}.  ``masks``: one per ReLU (bool, or a saved post-ReLU activation's
    ``> 0``), see ``_Relus``."""
    want = gy is not None
    x = x.detach().to(dtype).requires_grad_(want)
    has_pv = pv is not None and pv.shape[1] > 0
    pv = pv.detach().to(dtype).requires_grad_(want) if has_pv else None
    w = {k: v.detach().to(dtype).requires_grad_(want and weight_grads) for k, v in wts.items()}
    pre = []
    y = forward(kind, x, pv, w, masks, arg, pre)
    out = {'y': y.detach(), 'pre': [p.detach() for p in pre]}
    if want:
        names = sorted(w) if weight_grads else []
        leaves = [x] + ([pv] if has_pv else []) + [w[k] for k in names]
        grads = list(torch.autograd.grad(y, leaves, gy.detach().to(dtype)))
        out['gx'] = grads.pop(0)
        out['gpv'] = grads.pop(0) if has_pv else None
        out['gw'] = dict(zip(names, grads))
    return out


def masks_of(saved):
    """the device's decisions: its saved post-ReLU activations, in execution order, as constants"""
    return [(t.detach().cpu() > 0) for t in saved]


def flips(masks, pre):
    """decisions that differ from the evaluation's own (``pre`` > 0)"""
    return sum(int((m != (p > 0)).sum()) for m, p in zip(masks, pre))


def rel_err(got, ref):
    """max|got - ref| / max|ref| in float64; an all-zero reference asks for exact zeros"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if tuple(got.shape) != tuple(ref.shape):
        raise AssertionError('shape %s against %s' % (tuple(got.shape), tuple(ref.shape)))
    if not ref.numel():
        return 0.0
    d, s = float((got - ref).abs().max()), float(ref.abs().max())
    if d != d:
        return float('inf')                          # a NaN anywhere
    return d / s if s > 0 else (0.0 if d == 0 else float('inf'))


def check_arg(x, arg):
    """The contract of the saved indices against ``x`` (N,C,H,W), exactly: the pixel at arg[..., 0] / arg[..., 1] IS the plane's min /
    max, it is the FIRST such pixel in row-major order (tests/test_gpu_pointwise.py::test_channel_stats_first_occurrence), and a
    constant plane gives 0 for both.  Returns a list of complaints (empty = fine)."""
    flat, idx = x.detach().cpu().flatten(2), arg.detach().cpu().to(torch.int64)
    bad = []
    if tuple(idx.shape) != tuple(flat.shape[:2]) + (2,):
        return ['arg is %s for %s planes' % (tuple(idx.shape), tuple(flat.shape[:2]))]
    if int(idx.min()) < 0 or int(idx.max()) >= flat.shape[2]:
        return ['an index outside the plane: %d .. %d of %d' % (int(idx.min()), int(idx.max()), flat.shape[2])]
    for j, (name, ext) in enumerate((('min', flat.min(dim=2)[0]), ('max', flat.max(dim=2)[0]))):
        at = flat.gather(2, idx[..., j:j + 1]).squeeze(2)
        if not torch.equal(at, ext):
            bad.append('x[arg%s] is not the plane\'s %s on %d planes' % (name, name, int((at != ext).sum())))
        first = (flat == ext[..., None]).to(torch.uint8).argmax(dim=2)          # argmax of a 0/1 tensor: the first 1
        if not torch.equal(idx[..., j], first):
            bad.append('arg%s is not the first occurrence on %d planes' % (name, int((idx[..., j] != first).sum())))
    const = flat.min(dim=2)[0] == flat.max(dim=2)[0]
    if bool(const.any()) and int(idx[const].abs().max()) != 0:
        bad.append('a constant plane with a non-zero index')
    return bad


def first_arg(x):
    """(N,C,2) the indices ``check_arg`` accepts"""
    flat = x.detach().flatten(2)
    return torch.stack([(flat == flat.min(dim=2)[0][..., None]).to(torch.uint8).argmax(dim=2),
                        (flat == flat.max(dim=2)[0][..., None]).to(torch.uint8).argmax(dim=2)], dim=2)


# ------------------------------------------------------------------------------------------------ seeded inputs
INPUTS = ('smooth', 'quantised', 'constant')


def make_input(which, n, c, h, w, seed):
    """(n,c,h,w) fp32 in [0,1].  'smooth': a smooth random scene plus noise (``O.synthetic_raw``-like).  'quantised': 8-bit codes
    k/255 with a saturated patch of exact 0.0 and one of exact 1.0 in every plane, neither at pixel 0 - min and max are tied at many
    pixels, as in real frames.  'constant': 'smooth' with image 0 of the batch one value everywhere."""
    rng = np.random.Generator(np.random.PCG64(seed))
    low = rng.random((n, c, h // 16 + 2, w // 16 + 2)).astype(np.float32)
    scene = TF.interpolate(torch.from_numpy(low), size=(h + 32, w + 32), mode='bilinear', align_corners=False)[:, :, 16:16 + h, 16:16 + w].numpy()
    x = np.clip(0.05 + 0.9 * scene + rng.standard_normal(scene.shape).astype(np.float32) * 0.02, 0.02, 0.98).astype(np.float32)
    if which == 'quantised':
        x = np.round(x * 255).astype(np.float32) / 255.
        ph, pw = max(2, h // 4), max(2, w // 4)
        x[:, :, h - ph:, w // 3:w // 3 + pw] = 0.0
        x[:, :, 1:1 + ph, w - pw:] = 1.0
    elif which == 'constant':
        x[0] = 0.5
    elif which != 'smooth':
        raise ValueError(which)
    return torch.from_numpy(x)


def make_pv(n, p, seed):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).random((n, p)).astype(np.float32)) if p else None


def make_gy(shape, seed):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(tuple(shape)).astype(np.float32))


def case_inputs(case):
    """(x, [pv per member], [wts per member], [gy per member]) of a table row, all fp32 on the CPU: weights at gain 1 (never
    kink-free), a standard-normal upstream gradient per member"""
    seed = 1000 + CASES.index(case)
    kind, n, (h, w) = case['kind'], case['n'], case['hw']
    cin = 3 if kind in ('srcnn_res', 'path14l_bgr') else 1
    x = make_input(case['input'], n, cin, h, w, seed)
    ps = case['P'] if kind == 'srcnn_res' else (0,) * case['members']
    wts = [O.make_weights(kind, seed + 11 * (j + 1), p) for j, p in enumerate(ps)]
    pvs = [make_pv(n, p, seed + 101 * (j + 1)) for j, p in enumerate(ps)]
    gys = [make_gy((n, 3 if kind != 'path14l_bayer' else 1, h, w), seed + 1001 * (j + 1)) for j in range(len(ps))]
    return x, pvs, wts, gys


# ------------------------------------------------------------------------------------------------ the case table
# kind, form, P per member (SRCNNRes), batch, (H, W) of the INPUT tensor (the mosaic for the Bayer networks), input, arithmetic.
# Forms: SRCNNRes 'plain' / 'folded' / 'folded-infer' / 'train' / 'group'; SRCNNDemosaic and Path-Restore 'grad' / 'infer' (autograd
# off, forward only), SRCNNDemosaic also 'group-grad' / 'group-infer' (two members), Path-Restore also 'reuse' (``module._risp_reuse``).
def _c(kind, form, hw, n=2, P=(0,), inp='smooth', arith='f16x2', members=None):
    return dict(kind=kind, form=form, hw=hw, n=n, P=tuple(P), input=inp, arith=arith, members=members or len(P))


CASES = [
    # ---- SRCNNRes, one member.  (7, 12): no fold; (8, 8), (8, 12): the fold boundary; (20, 36), (34, 30): ragged; (40, 72), (64, 96):
    #      several 16 x 32 tiles, one 64-row segment exactly; (9, 17): H W = 153, no multiple of 4
    _c('srcnn_res', 'plain', (7, 12), P=(1,)),
    _c('srcnn_res', 'plain', (7, 12), P=(0,), inp='quantised'),
    _c('srcnn_res', 'plain', (8, 12), P=(3,), inp='constant'),
    _c('srcnn_res', 'plain', (9, 17), P=(5,), inp='quantised'),
    _c('srcnn_res', 'plain', (34, 30), n=3, P=(0,)),
    _c('srcnn_res', 'plain', (64, 96), P=(5,), inp='quantised'),
    _c('srcnn_res', 'folded', (8, 8), P=(0,), inp='quantised'),
    _c('srcnn_res', 'folded', (8, 12), P=(1,), inp='constant'),
    _c('srcnn_res', 'folded', (20, 36), P=(3,)),
    _c('srcnn_res', 'folded', (34, 30), n=3, P=(5,), inp='quantised'),
    _c('srcnn_res', 'folded', (40, 72), P=(1,)),
    _c('srcnn_res', 'folded', (64, 96), P=(3,), inp='quantised'),
    _c('srcnn_res', 'folded', (9, 17), P=(1,), inp='constant'),
    _c('srcnn_res', 'folded', (9, 17), n=3, P=(0,), inp='quantised'),
    _c('srcnn_res', 'folded-infer', (8, 8), P=(1,)),
    _c('srcnn_res', 'folded-infer', (8, 12), P=(5,), inp='quantised'),
    _c('srcnn_res', 'folded-infer', (34, 30), n=3, P=(3,), inp='constant'),
    _c('srcnn_res', 'folded-infer', (40, 72), P=(0,), inp='quantised'),
    _c('srcnn_res', 'folded-infer', (64, 96), P=(1,)),
    _c('srcnn_res', 'folded-infer', (9, 17), P=(3,), inp='quantised'),
    _c('srcnn_res', 'train', (7, 12), P=(3,), inp='quantised'),
    _c('srcnn_res', 'train', (8, 8), P=(5,)),
    _c('srcnn_res', 'train', (20, 36), P=(0,), inp='constant'),
    _c('srcnn_res', 'train', (34, 30), n=3, P=(1,)),
    _c('srcnn_res', 'train', (40, 72), P=(5,), inp='quantised'),
    _c('srcnn_res', 'train', (64, 96), P=(0,)),
    _c('srcnn_res', 'train', (9, 17), P=(1,), inp='quantised'),
    # ---- SRCNNRes groups through F.srcnn_res_group: the family of an sRGB slot and a pair
    _c('srcnn_res', 'group', (8, 12), n=2, P=FAMILY_P, inp='quantised'),
    _c('srcnn_res', 'group', (24, 32), n=4, P=FAMILY_P),
    _c('srcnn_res', 'group', (40, 72), n=2, P=FAMILY_P, inp='constant'),
    _c('srcnn_res', 'group', (8, 12), n=4, P=PAIR_P),
    _c('srcnn_res', 'group', (24, 32), n=2, P=PAIR_P, inp='constant'),
    _c('srcnn_res', 'group', (40, 72), n=4, P=PAIR_P, inp='quantised'),
    # ---- SRCNNDemosaic: (18, 26) = 9 x 13 planes; (36, 20), (18, 26): W % 8 != 0, no group
    _c('srcnn_demosaic', 'grad', (8, 8), inp='quantised'),
    _c('srcnn_demosaic', 'grad', (16, 24)),
    _c('srcnn_demosaic', 'grad', (36, 20), n=3, inp='constant'),
    _c('srcnn_demosaic', 'grad', (18, 26), inp='quantised'),
    _c('srcnn_demosaic', 'grad', (80, 72)),
    _c('srcnn_demosaic', 'grad', (128, 64), inp='quantised'),
    _c('srcnn_demosaic', 'infer', (16, 24), inp='quantised'),
    _c('srcnn_demosaic', 'infer', (36, 20)),
    _c('srcnn_demosaic', 'infer', (18, 26), n=3),
    _c('srcnn_demosaic', 'infer', (128, 64), inp='constant'),
    _c('srcnn_demosaic', 'group-grad', (8, 8), members=2),
    _c('srcnn_demosaic', 'group-grad', (16, 24), n=3, members=2, inp='quantised'),
    _c('srcnn_demosaic', 'group-grad', (80, 72), members=2, inp='constant'),
    _c('srcnn_demosaic', 'group-grad', (128, 64), members=2),
    _c('srcnn_demosaic', 'group-infer', (16, 24), members=2),
    _c('srcnn_demosaic', 'group-infer', (80, 72), members=2, inp='quantised'),
    # ---- Path-Restore 14l, bgr
    _c('path14l_bgr', 'grad', (5, 7), arith='f16x2', inp='quantised'),
    _c('path14l_bgr', 'grad', (5, 7), arith='f32'),
    _c('path14l_bgr', 'grad', (16, 16), arith='f16x2'),
    _c('path14l_bgr', 'grad', (16, 16), arith='f32', inp='constant'),
    _c('path14l_bgr', 'grad', (33, 30), n=3, arith='f16x2'),
    _c('path14l_bgr', 'grad', (33, 30), arith='f32', inp='quantised'),
    _c('path14l_bgr', 'grad', (48, 80), arith='f16x2', inp='constant'),
    _c('path14l_bgr', 'grad', (48, 80), arith='f32'),
    _c('path14l_bgr', 'grad', (64, 96), arith='f16x2', inp='quantised'),
    _c('path14l_bgr', 'grad', (64, 96), arith='f32'),
    _c('path14l_bgr', 'infer', (5, 7), arith='f32'),
    _c('path14l_bgr', 'infer', (33, 30), arith='f16x2'),
    _c('path14l_bgr', 'infer', (64, 96), arith='f16x2'),
    _c('path14l_bgr', 'infer', (48, 80), arith='f32', inp='quantised'),
    _c('path14l_bgr', 'reuse', (16, 16), arith='f16x2', inp='quantised'),
    # ---- Path-Restore 14l, bayer
    _c('path14l_bayer', 'grad', (8, 8), arith='f16x2'),
    _c('path14l_bayer', 'grad', (8, 8), arith='f32', inp='quantised'),
    _c('path14l_bayer', 'grad', (18, 26), n=3, arith='f16x2', inp='quantised'),
    _c('path14l_bayer', 'grad', (18, 26), arith='f32'),
    _c('path14l_bayer', 'grad', (40, 72), arith='f16x2', inp='constant'),
    _c('path14l_bayer', 'grad', (40, 72), arith='f32'),
    _c('path14l_bayer', 'grad', (96, 64), arith='f16x2'),
    _c('path14l_bayer', 'grad', (96, 64), arith='f32', inp='quantised'),
    _c('path14l_bayer', 'infer', (8, 8), arith='f32'),
    _c('path14l_bayer', 'infer', (18, 26), arith='f16x2'),
    _c('path14l_bayer', 'infer', (96, 64), arith='f16x2', inp='quantised'),
    _c('path14l_bayer', 'reuse', (18, 26), arith='f32'),
    _c('path14l_bayer', 'reuse', (40, 72), arith='f16x2'),
]


def case_id(case):
    p = '-P' + '.'.join(map(str, case['P'])) if case['kind'] == 'srcnn_res' else ('-x%d' % case['members'] if case['members'] > 1 else '')
    return '%s-%s%s-%dx%dx%d-%s-%s' % ((case['kind'], case['form'], p, case['n']) + tuple(case['hw']) + (case['input'], case['arith']))


# ------------------------------------------------------------------------------------------------ the predicates, on shapes
def srcnn_fold_ok(h, w, k=9):
    """``convnets._srcnn_fold_ok`` restated (tests/test_net_reference_cpu.py holds the two together)"""
    return h >= k - 1 and k - 1 <= w <= 8192


def can_group(kind, members, h, w):
    """the shape conditions of ``functional.can_group`` for fp32 tensors from the allocator (16-byte aligned, on the device), no
    member under fine-tuning: at least two members, W % 4 == 0; SRCNNRes: the fold; SRCNNDemosaic: H even, W % 8 == 0"""
    if members < 2 or w % 4:
        return False
    return srcnn_fold_ok(h, w) if kind == 'srcnn_res' else (h % 2 == 0 and w % 8 == 0)


def pack_conditions(kind, P=0):
    """``build_srcnn_packs``' conditions on cout / k, from the layer shapes alone: {'fold', 'small_bwd', 'small'}"""
    spec = O.conv_shapes(kind, P)
    (_, _, cin0, _), (_, cout2, _, k2) = spec[0], spec[2]
    residual = kind == 'srcnn_res'
    return {'fold': residual and cout2 <= 4, 'small_bwd': not residual and cin0 == 4,
            'small': not residual and cout2 <= 12 and k2 in (3, 5)}


def expected_form(case):
    """the form the dispatch takes for a row's shapes - what the row must declare (a 'plain' row at a size that folds names the
    Function ``_SrcnnRes`` itself, which the test then applies directly: the dispatch never reaches it there)"""
    kind, form, (h, w) = case['kind'], case['form'], case['hw']
    if kind == 'srcnn_res':
        if form == 'train':
            return 'train'
        if form == 'group':
            return 'group' if can_group(kind, case['members'], h, w) else None
        fold = pack_conditions(kind, case['P'][0])['fold'] and srcnn_fold_ok(h, w)
        if form == 'plain':
            return 'plain'
        return form if fold else None
    if h % 2 or w % 2:
        return None if kind != 'path14l_bgr' else form
    if form.startswith('group'):
        return form if can_group(kind, case['members'], h, w) else None
    return form


def plain_by_dispatch(case):
    return case['kind'] == 'srcnn_res' and case['form'] == 'plain' and not srcnn_fold_ok(*case['hw'])


# the wiring branches of convnets.py's Functions that the table must reach: name -> predicate on a row
BRANCHES = {
    '_SrcnnRes by dispatch (no fold)': plain_by_dispatch,
    '_SrcnnRes applied at a size that folds': lambda c: c['kind'] == 'srcnn_res' and c['form'] == 'plain' and not plain_by_dispatch(c),
    '_SrcnnResFolded': lambda c: c['form'] == 'folded',
    '_SrcnnResFolded, inference': lambda c: c['form'] == 'folded-infer',
    '_SrcnnResTrain': lambda c: c['form'] == 'train',
    '_SrcnnResTrain without fold': lambda c: c['form'] == 'train' and not srcnn_fold_ok(*c['hw']),
    '_SrcnnResGroupFn, the family': lambda c: c['form'] == 'group' and c['P'] == FAMILY_P,
    '_SrcnnResGroupFn, a pair': lambda c: c['form'] == 'group' and len(c['P']) == 2,
    'SRCNNRes without parameters': lambda c: c['kind'] == 'srcnn_res' and c['P'] == (0,),
    'SRCNNRes statistics, scalar kernels (H W % 4 != 0) with a backward': lambda c: c['kind'] == 'srcnn_res' and (c['hw'][0] * c['hw'][1]) % 4 != 0 and c['form'] in ('plain', 'folded', 'train'),
    'SRCNNRes tied statistics': lambda c: c['kind'] == 'srcnn_res' and c['input'] == 'quantised' and c['form'] != 'folded-infer',
    'SRCNNRes constant image': lambda c: c['kind'] == 'srcnn_res' and c['input'] == 'constant' and c['form'] != 'folded-infer',
    '_SrcnnDemosaic': lambda c: c['kind'] == 'srcnn_demosaic' and c['form'] == 'grad',
    '_SrcnnDemosaic, inference': lambda c: c['kind'] == 'srcnn_demosaic' and c['form'] == 'infer',
    '_SrcnnDemosaic where no group may form': lambda c: c['kind'] == 'srcnn_demosaic' and c['form'] == 'grad' and not can_group('srcnn_demosaic', 2, *c['hw']),
    '_SrcnnDemosaicGroupFn': lambda c: c['form'] == 'group-grad',
    '_SrcnnDemosaicGroupFn, inference': lambda c: c['form'] == 'group-infer',
    '_Path14l bgr, split precision': lambda c: c['kind'] == 'path14l_bgr' and c['form'] == 'grad' and c['arith'] == 'f16x2',
    '_Path14l bgr, fp32': lambda c: c['kind'] == 'path14l_bgr' and c['form'] == 'grad' and c['arith'] == 'f32',
    '_Path14l bgr, W % 4 != 0': lambda c: c['kind'] == 'path14l_bgr' and c['form'] == 'grad' and c['hw'][1] % 4 != 0,
    '_Path14l bayer, split precision': lambda c: c['kind'] == 'path14l_bayer' and c['form'] == 'grad' and c['arith'] == 'f16x2',
    '_Path14l bayer, fp32': lambda c: c['kind'] == 'path14l_bayer' and c['form'] == 'grad' and c['arith'] == 'f32',
    '_Path14l bayer, plane W % 4 != 0': lambda c: c['kind'] == 'path14l_bayer' and c['form'] == 'grad' and (c['hw'][1] // 2) % 4 != 0,
    '_Path14l, inference': lambda c: c['kind'].startswith('path14l') and c['form'] == 'infer',
    '_Path14l, record reuse bgr': lambda c: c['kind'] == 'path14l_bgr' and c['form'] == 'reuse',
    '_Path14l, record reuse bayer': lambda c: c['kind'] == 'path14l_bayer' and c['form'] == 'reuse',
}
