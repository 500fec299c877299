"""Differentiable ISP operators on top of the C ABI (``include/risp.h``).

Every function here is a ``torch.autograd.Function`` whose forward AND backward are
hand-written HIP kernels in ``libreconfigisp_hip.so``; PyTorch only owns the device
buffers and the stream.  Tensors must live on the GPU - a CPU tensor raises, there is
no fallback.

``_IMPL`` is the dispatch seam: the host logic above (registry, super-net, DARTS
step) calls ``F.<op>`` which forwards to ``_IMPL``.  The product never rebinds it;
the CPU test-suite does (tests/conftest.py) so that the host logic can be exercised
without a GPU.
"""
import ctypes as C

import torch

from . import lib as L

OP_SKIP, OP_DEMOSAIC_NEAREST, OP_WB_MANUAL, OP_GAMMA, OP_GTM_MANUAL, OP_WB_QUADRATIC, OP_GAIN3 = range(7)
OP_TONE_CRYSIS, OP_TONE_FILMIC = 7, 8      # stages of serve_classical_u8 only: every other entry point refuses them


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream():
    """The current HIP stream of the current device as a void* (the raw-handle getter is ~10x cheaper than building
    a torch.cuda.Stream object, which matters for launches of ~50 us)."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_gpu(t, what='tensor'):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError('reconfigisp_amd: %s must be a CUDA/HIP tensor (got %s); the ops are GPU-only '
                           'and there is no CPU fallback' % (what, getattr(t, 'device', type(t))))


def _dev(t, what='tensor'):
    _need_gpu(t, what)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _grad_scratch(n, device):
    """workspace of the element-wise backward kernels (per-workgroup partial parameter gradients)"""
    return torch.empty(L.load().risp_param_grad_scratch_floats(n), device=device, dtype=torch.float32)


def _check_bgr(x):
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError('expected a (N,3,H,W) BGR tensor, got %s' % (tuple(x.shape),))
    if (x.shape[2] * x.shape[3]) % 4:
        raise ValueError('H*W must be a multiple of 4, got %s' % (tuple(x.shape),))


def _check_params(p, n, width, name):
    if p.dim() != 2 or p.shape[0] != n or p.shape[1] != width:
        raise ValueError('%s: params must be (N=%d,%d), got %s' % (name, n, width, tuple(p.shape)))


class _Pointwise(torch.autograd.Function):
    """y = op(x, p) for the planar BGR ops; p is the (N,P) per-image block."""

    @staticmethod
    def forward(ctx, x, p, name, width):
        x, p = _dev(x, 'img'), _dev(p, 'params')
        _check_bgr(x)
        _check_params(p, x.shape[0], width, name)
        y = torch.empty_like(x)
        n, hw = x.shape[0], x.shape[2] * x.shape[3]
        L.call('risp_%s_fwd' % name, _p(x), _p(p), _p(y), n, hw, _stream())
        ctx.save_for_backward(x, p)
        ctx.name = name
        return y

    @staticmethod
    def backward(ctx, gy):
        x, p = ctx.saved_tensors
        gy = _dev(gy, 'grad')
        gx, gp = torch.empty_like(x), torch.empty_like(p)
        n, hw = x.shape[0], x.shape[2] * x.shape[3]
        L.call('risp_%s_bwd' % ctx.name, _p(x), _p(p), _p(gy), _p(gx), _p(gp), _p(_grad_scratch(n, x.device)), n, hw, _stream())
        return gx, gp, None, None


class _DemosaicNearest(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _dev(x, 'img')
        if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] % 2 or x.shape[3] % 2:
            raise ValueError('expected a (N,1,H,W) RGGB mosaic with even H, W; got %s' % (tuple(x.shape),))
        n, _, h, w = x.shape
        y = torch.empty((n, 3, h, w), device=x.device, dtype=torch.float32)
        L.call('risp_demosaic_nearest_fwd', _p(x), _p(y), n, h, w, _stream())
        ctx.shape = (n, h, w)
        return y

    @staticmethod
    def backward(ctx, gy):
        n, h, w = ctx.shape
        gy = _dev(gy, 'grad')
        gx = torch.empty((n, 1, h, w), device=gy.device, dtype=torch.float32)
        L.call('risp_demosaic_nearest_bwd', _p(gy), _p(gx), n, h, w, _stream())
        return gx


def channel_stats(x, want_arg=True):
    """(N,C,H,W) -> stats (N,C,4) = {min,sum,max,0}, arg (N,C,2) int32 (first argmin/argmax)."""
    x = _dev(x)
    n, c, h, w = x.shape
    stats = torch.empty((n, c, 4), device=x.device, dtype=torch.float32)
    arg = torch.empty((n, c, 2), device=x.device, dtype=torch.int32) if want_arg else None
    ws = torch.empty(L.load().risp_channel_stats_scratch_floats(n * c, h * w), device=x.device, dtype=torch.float32)
    L.call('risp_channel_stats', _p(x), _p(stats), _p(arg), _p(ws), n * c, h * w, _stream())
    return stats, arg


def histc01(x, bins):
    """Per-(n,c) histogram of an (N,C,H,W) tensor with torch.histc(.., bins, 0, 1) semantics -> (N, C*bins)."""
    x = _dev(x.detach())
    n, c, h, w = x.shape
    hist = torch.empty((n, c * bins), device=x.device, dtype=torch.float32)
    L.call('risp_histc', _p(x), _p(hist), n * c, h * w, bins, _stream())
    return hist


class _CondFc(torch.autograd.Function):
    """sigmoid(MLP(hist) + flat[global]) of the conditional heads (tools_origin.py:109-163): risp_cond_fc_fwd /
    risp_cond_fc_bwd.  ``hist`` carries no gradient; the gradient of the flat parameter vector is fully written."""

    @staticmethod
    def forward(ctx, hist, flat, widths):
        hist, flat = _dev(hist.detach(), 'hist'), _dev(flat, 'params')
        n, nl = hist.shape[0], len(widths) - 1
        cw = (C.c_int * len(widths))(*widths)
        row = L.load().risp_cond_fc_row_floats(cw, nl)
        acts = torch.empty((n, row), device=hist.device, dtype=torch.float32)
        out = torch.empty((n, widths[-1]), device=hist.device, dtype=torch.float32)
        L.call('risp_cond_fc_fwd', _p(hist), _p(flat), cw, nl, _p(acts), _p(out), n, _stream())
        ctx.save_for_backward(flat, acts, out)
        ctx.widths = tuple(widths)
        return out

    @staticmethod
    def backward(ctx, gout):
        flat, acts, out = ctx.saved_tensors
        widths, nl = ctx.widths, len(ctx.widths) - 1
        cw = (C.c_int * len(widths))(*widths)
        gout = _dev(gout, 'grad')
        deltas = torch.empty_like(acts)
        dflat = torch.empty_like(flat)
        L.call('risp_cond_fc_bwd', _p(flat), cw, nl, _p(acts), _p(out), _p(gout), _p(deltas), _p(dflat), flat.numel(),
               acts.shape[0], _stream())
        return None, dflat, None


def _hip_conditional_fc(img, flat, widths):
    bins = widths[0] // 3
    return _CondFc.apply(histc01(img, bins), flat, tuple(int(v) for v in widths))


class _Grayworld(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _dev(x, 'img')
        _check_bgr(x)
        n, hw = x.shape[0], x.shape[2] * x.shape[3]
        stats, _ = channel_stats(x, want_arg=False)
        gains = torch.empty((n, 3), device=x.device, dtype=torch.float32)
        L.call('risp_grayworld_gains_fwd', _p(stats), _p(gains), n, hw, _stream())
        y = torch.empty_like(x)
        L.call('risp_gain3_fwd', _p(x), _p(gains), _p(y), n, hw, _stream())
        ctx.save_for_backward(x, stats, gains)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, stats, gains = ctx.saved_tensors
        gy = _dev(gy, 'grad')
        n, hw = x.shape[0], x.shape[2] * x.shape[3]
        gx, gk, gm = torch.empty_like(x), torch.empty_like(gains), torch.empty_like(gains)
        L.call('risp_gain3_bwd', _p(x), _p(gains), _p(gy), _p(gx), _p(gk), _p(_grad_scratch(n, x.device)), n, hw, _stream())
        L.call('risp_grayworld_gains_bwd', _p(stats), _p(gk), _p(gm), n, hw, _stream())
        L.call('risp_stats_bwd', _p(gx), None, _p(gm), None, None, n * 3, hw, _stream())
        return gx


def grayworld_gains(x):
    """(N,3) gray-world gains of an (N,3,H,W) image (inference helper for the fused chain)."""
    x = _dev(x, 'img')
    _check_bgr(x)
    n, hw = x.shape[0], x.shape[2] * x.shape[3]
    stats, _ = channel_stats(x, want_arg=False)
    gains = torch.empty((n, 3), device=x.device, dtype=torch.float32)
    L.call('risp_grayworld_gains_fwd', _p(stats), _p(gains), n, hw, _stream())
    return gains


class _Mix(torch.autograd.Function):
    """y = sum_k w[k] * o_k ; w is a 1-D tensor (gradient flows to it), o_k the op outputs."""

    @staticmethod
    def forward(ctx, w, w_host, stacks, *outs):
        outs = [_aligned16(_dev(o)) for o in outs]      # risp_mix_* refuse a view that sits off a 16-byte boundary: such a view is copied
        k = len(outs)
        ctx.stacks = stacks
        if w_host is None:                  # the caller usually has the values on the host already (no second D2H)
            w_host = w.detach().cpu().tolist()
        w_host = [float(v) for v in w_host]
        if len(w_host) != k or w.numel() != k:
            raise ValueError('mix: %d weights for %d operands' % (len(w_host), k))
        y = torch.empty_like(outs[0])
        L.call('risp_mix_fwd', L.ptr_array([o.data_ptr() for o in outs]), (C.c_float * k)(*w_host), k, _p(y),
               y.numel(), _stream())
        ctx.save_for_backward(*outs)
        ctx.w_host = w_host
        ctx.w_meta = (w.device, w.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        outs = ctx.saved_tensors
        gy = _aligned16(_dev(gy, 'grad'))
        k = len(outs)
        need = ctx.needs_input_grad[3:]
        gos = [None] * k
        for members in (ctx.stacks or ()):          # operands that feed ONE grouped launch: consecutive slices of one buffer
            if all(need[i] for i in members):
                buf = torch.empty((len(members),) + tuple(outs[members[0]].shape), device=gy.device, dtype=torch.float32)
                for j, i in enumerate(members):
                    gos[i] = buf[j]
        gos = [g if g is not None else (torch.empty_like(o) if nd else None) for g, o, nd in zip(gos, outs, need)]
        gw = torch.empty(k, device=gy.device, dtype=torch.float32)
        scratch = torch.empty(L.load().risp_mix_scratch_floats(), device=gy.device, dtype=torch.float32)
        L.call('risp_mix_bwd', L.ptr_array([o.data_ptr() for o in outs]), (C.c_float * k)(*ctx.w_host), k, _p(gy),
               L.ptr_array([g.data_ptr() if g is not None else None for g in gos]), _p(gw), _p(scratch), gy.numel(), _stream())
        return (gw.to(device=ctx.w_meta[0], dtype=ctx.w_meta[1]), None, None) + tuple(gos)


SLOT_KINDS = {'skip': OP_SKIP, 'wb_manual': OP_WB_MANUAL, 'gamma': OP_GAMMA, 'gtm_manual': OP_GTM_MANUAL,
              'wb_quadratic': OP_WB_QUADRATIC, 'grayworld': OP_GAIN3}
_SLOT_WIDTH = {OP_WB_MANUAL: 3, OP_GAMMA: 1, OP_GTM_MANUAL: 3, OP_WB_QUADRATIC: 30}


class _SlotMix(torch.autograd.Function):
    """y = sum_k w[k] o_k of one super-net slot with the element-wise operators evaluated on the fly (risp_slot_mix_fwd /
    _bwd): operand k is a materialised tensor (kinds[k] == L.SLOT_TENSOR) or op(x, block) for an element-wise kind.
    ``flat``: per operand the tensor / the (N,P) parameter block / nothing (skip, gray world)."""

    @staticmethod
    def forward(ctx, w, w_host, x, kinds, stacks, *flat):
        x = _dev(x, 'img')
        _check_bgr(x)
        n, hw = x.shape[0], x.shape[2] * x.shape[3]
        k = len(kinds)
        w_host = [float(v) for v in (w_host if w_host is not None else w.detach().cpu().tolist())]
        if len(w_host) != k or w.numel() != k or k > L.MIX_MAX:
            raise ValueError('slot_mix: %d weights for %d operands (at most %d)' % (len(w_host), k, L.MIX_MAX))
        d = L.SlotMixDesc()
        d.K, d.N, d.HW = k, n, hw
        keep, it, stats = [], iter(flat), None
        for i, kind in enumerate(kinds):
            d.kind[i], d.w[i], d.pmul[i] = kind, w_host[i], 1.0
            if kind == L.SLOT_TENSOR:
                t = _dev(next(it))
                if t.shape != x.shape:
                    raise ValueError('slot_mix: operand %d has shape %s, the slot input %s' % (i, tuple(t.shape), tuple(x.shape)))
            elif kind == OP_SKIP:
                t = None
            elif kind == OP_GAIN3:                   # gray world: gains from the statistics of x (no parameters)
                stats, _ = channel_stats(x, want_arg=False)
                t = torch.empty((n, 3), device=x.device, dtype=torch.float32)
                L.call('risp_grayworld_gains_fwd', _p(stats), _p(t), n, hw, _stream())
            else:
                t = _dev(next(it), 'params')
                _check_params(t, n, _SLOT_WIDTH[kind], 'slot operand %d' % i)
                if kind == OP_WB_MANUAL:
                    d.pmul[i] = 5.0                   # the wrapper's params * 5 (tools_origin.py:214)
            keep.append(t)
            d.ptr[i] = t.data_ptr() if t is not None else None
        y = torch.empty_like(x)
        d.x, d.y = x.data_ptr(), y.data_ptr()
        L.call('risp_slot_mix_fwd', C.byref(d), _stream())
        ctx.save_for_backward(x, stats, *[t for t in keep if t is not None])
        ctx.kinds, ctx.w_host, ctx.stacks, ctx.w_meta = tuple(kinds), w_host, stacks, (w.device, w.dtype)
        ctx.has = [t is not None for t in keep]
        return y

    @staticmethod
    def backward(ctx, gy):
        x, stats, *rest = ctx.saved_tensors
        kinds, k = ctx.kinds, len(ctx.kinds)
        gy = _dev(gy, 'grad')
        n, hw = x.shape[0], x.shape[2] * x.shape[3]
        it = iter(rest)
        keep = [next(it) if h else None for h in ctx.has]
        dev = dict(device=gy.device, dtype=torch.float32)
        d = L.SlotMixDesc()
        d.K, d.N, d.HW = k, n, hw
        d.x = x.data_ptr()
        # gradient buffers: tensor operands of one grouped launch share a stacked buffer (convnets._stack_grads)
        go = [None] * k
        for members in (ctx.stacks or ()):
            if all(kinds[i] == L.SLOT_TENSOR for i in members):
                buf = torch.empty((len(members),) + tuple(x.shape), **dev)
                for j, i in enumerate(members):
                    go[i] = buf[j]
        gp = [None] * k
        pointwise = False
        # only what the graph consumes is allocated and written (risp_slot_mix_bwd takes NULL for go[k] / gp[k]): 12 B/pixel per
        # tensor operand whose producer needs no gradient.  forward inputs: (w, w_host, x, kinds, stacks, *flat)
        need_flat, need_x = iter(ctx.needs_input_grad[5:]), ctx.needs_input_grad[2]
        for i, kind in enumerate(kinds):
            d.kind[i], d.w[i], d.pmul[i] = kind, ctx.w_host[i], 5.0 if kind == OP_WB_MANUAL else 1.0
            d.ptr[i] = keep[i].data_ptr() if keep[i] is not None else None
            if kind == L.SLOT_TENSOR:
                need = next(need_flat)
                if go[i] is None and need:
                    go[i] = torch.empty_like(x)
                d.go[i] = go[i].data_ptr() if go[i] is not None else None
            else:
                pointwise = True
                need = next(need_flat) if kind not in (OP_SKIP, OP_GAIN3) else need_x       # gray world: its gains lead back to x
                if kind != OP_SKIP and need:
                    gp[i] = torch.empty_like(keep[i])
                    d.gp[i] = gp[i].data_ptr()
        gx = torch.empty_like(x) if pointwise else None
        gw = torch.empty(k, **dev)
        scratch = torch.empty(L.load().risp_slot_mix_scratch_floats(n, hw), **dev)
        L.call('risp_slot_mix_bwd', C.byref(d), _p(gy), _p(gx), _p(gw), _p(scratch), _stream())
        for i, kind in enumerate(kinds):
            if kind == OP_GAIN3 and gp[i] is not None:        # gray world: the gains' gradient flows back through the channel means
                gm = torch.empty((n, 3), **dev)
                L.call('risp_grayworld_gains_bwd', _p(stats), _p(gp[i]), _p(gm), n, hw, _stream())
                L.call('risp_stats_bwd', _p(gx), None, _p(gm), None, None, n * 3, hw, _stream())
        grads = []
        for i, kind in enumerate(kinds):
            if kind == L.SLOT_TENSOR:
                grads.append(go[i])
            elif kind not in (OP_SKIP, OP_GAIN3):
                grads.append(gp[i])
        return (gw.to(device=ctx.w_meta[0], dtype=ctx.w_meta[1]), None, gx, None, None) + tuple(grads)


class _PruneSoftmax(torch.autograd.Function):
    """post = pruned, renormalised softmax(alpha) of one super-net slot (risp_prune_softmax_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, alpha, threshold, unavailable):
        a = _dev(alpha, 'alpha')
        k = a.numel()
        buf = torch.empty((3, k), device=a.device, dtype=torch.float32)          # probs | coef | post
        L.call('risp_prune_softmax_fwd', _p(a), _p(unavailable), float(threshold), k, _p(buf[0]), _p(buf[1]), _p(buf[2]),
               _stream())
        ctx.save_for_backward(buf)
        return buf[2]

    @staticmethod
    def backward(ctx, gpost):
        buf, = ctx.saved_tensors
        k = buf.shape[1]
        galpha = torch.empty(k, device=buf.device, dtype=torch.float32)
        L.call('risp_prune_softmax_bwd', _p(buf[0]), _p(buf[1]), _p(_dev(gpost, 'grad')), k, _p(galpha), _stream())
        return galpha, None, None


class _ParamBlocks(torch.autograd.Function):
    """blocks[k] = sigmoid(raw[k]).repeat(N, 1) for all parametrised ops of a slot in ONE launch each way."""

    @staticmethod
    def forward(ctx, n, *raws):
        raws = [_dev(r, 'params') for r in raws]
        d = L.ParamBlocksDesc()
        d.n_ops, d.N = len(raws), n
        flat = torch.empty(n * sum(r.numel() for r in raws), device=raws[0].device, dtype=torch.float32)
        blocks, at = [], 0
        for k, r in enumerate(raws):
            w = r.numel()
            blk = flat[at: at + n * w].view(n, w)
            at += n * w
            d.width[k], d.raw[k], d.block[k] = w, r.data_ptr(), blk.data_ptr()
            blocks.append(blk)
        L.call('risp_param_blocks_fwd', C.byref(d), _stream())
        ctx.save_for_backward(*raws)
        ctx.n = n
        return tuple(blocks)

    @staticmethod
    def backward(ctx, *gblocks):
        raws = ctx.saved_tensors
        d = L.ParamBlocksDesc()
        d.n_ops, d.N = len(raws), ctx.n
        keep, grads = [], []
        for k, (r, g) in enumerate(zip(raws, gblocks)):
            if g is not None and not (g.is_cuda and g.dtype == torch.float32 and g.dim() == 2 and g.stride(1) == 1
                                      and g.stride(0) >= g.shape[1]):
                g = _dev(g, 'grad')               # (a column range of a wider matrix is read in place: SRCNNRes' folded backward)
            keep.append(g)
            gr = torch.empty_like(r)
            grads.append(gr)
            d.width[k], d.raw[k], d.graw[k] = r.numel(), r.data_ptr(), gr.data_ptr()
            d.gblock[k] = g.data_ptr() if g is not None else None
            d.gstride[k] = g.stride(0) if g is not None else 0
        L.call('risp_param_blocks_bwd', C.byref(d), _stream())
        return (None,) + tuple(grads)


class _ZeroGrad(torch.autograd.Function):
    """y passes through untouched; the extra parameters join the graph with an all-zero gradient.

    Stands for the reference's 'dummy gradients' term ``zeros(x.shape) * par.sum()``
    (super_prune_fifteen_demos_four_bayer_two.py:198-201, needed by DDP) without a pass over y."""

    @staticmethod
    def forward(ctx, y, *pars):
        ctx.shapes = [(p.shape, p.dtype, p.device) for p in pars]
        return y.view_as(y)

    @staticmethod
    def backward(ctx, gy):
        return (gy,) + tuple(torch.zeros(s, dtype=d, device=dev) for s, d, dev in ctx.shapes)


def attach_zero_grad(y, pars):
    return _ZeroGrad.apply(y, *pars)


class ChainPlan:
    """A fused element-wise segment with its output buffers and marshalled arguments prepared once;
    ``launch()`` is a single C-ABI call (``risp_chain_fwd``).  ``outs[k]`` is stage k's output
    (SKIP stages alias their input)."""

    def __init__(self, x, ops, params, out_last=None):
        x = _dev(x, 'img')
        n, cin, h, w = x.shape
        if h % 2 or w % 2:
            raise ValueError('H and W must be even, got %s' % (tuple(x.shape),))
        if cin != (1 if ops[0] == OP_DEMOSAIC_NEAREST else 3):
            raise ValueError('chain input has %d channels' % cin)
        self.x, self.outs, cur = x, [], x
        count = sum(1 for op in ops if op != OP_SKIP)
        # ``out_last``: the caller's buffer for the segment's LAST computed stage (a contiguous fp32 (N,3,H,W) device tensor, 16-byte
        # aligned - test_split.run_frame hands a slice of the frame's tile stack); the other stages share ONE allocation
        if out_last is not None and (not count or tuple(out_last.shape) != (n, 3, h, w) or not out_last.is_contiguous()
                                     or out_last.dtype != torch.float32 or out_last.device != x.device or out_last.data_ptr() % 16):
            out_last = None
        own = count - (1 if out_last is not None else 0)
        bufs = iter(torch.empty((own, n, 3, h, w), device=x.device, dtype=torch.float32).unbind(0)) if own else iter(())
        left = count
        for op in ops:
            if op != OP_SKIP:
                left -= 1
                cur = out_last if (left == 0 and out_last is not None) else next(bufs)      # every stage output is a (N,3,H,W) view of ONE allocation
            self.outs.append(cur)
        self.params = [_dev(p) if p is not None else None for p in params]   # keep alive
        self._args = (_p(x), len(ops), (C.c_int * len(ops))(*ops),
                      L.ptr_array([p.data_ptr() if p is not None else None for p in self.params]),
                      L.ptr_array([o.data_ptr() if op != OP_SKIP else None for o, op in zip(self.outs, ops)]),
                      n, h, w)

    def launch(self):
        L.call('risp_chain_fwd', *self._args, _stream())
        return self.outs


def chain_forward(x, ops, params, out_last=None):
    """Fused element-wise segment: returns the list of stage outputs (SKIP aliases its input).

    Inference-only fast path (no autograd graph is recorded)."""
    return ChainPlan(x, ops, params, out_last).launch()


class BilateralChainPlan:
    """[nearest demosaic ->] bilateral -> element-wise chain as ONE launch (risp_bilateral_chain_fwd).
    ``outs`` lists the stage outputs in pipeline order: [demosaic,] bilateral, chain stages..."""

    def __init__(self, x, from_bayer, window, sigma_color, sigma_space, max_window, ops, params):
        x = _dev(x, 'img')
        n, cin, h, w = x.shape
        if cin != (1 if from_bayer else 3) or h % 2 or w % 4:
            raise ValueError('fused stencil segment: unsupported input %s' % (tuple(x.shape),))
        count = (2 if from_bayer else 1) + sum(1 for op in ops if op != OP_SKIP)
        bufs = iter(torch.empty((count, n, 3, h, w), device=x.device, dtype=torch.float32).unbind(0))
        new = lambda: next(bufs)              # every stage output is a (N,3,H,W) view of ONE allocation
        self.x = x
        self.dem = new() if from_bayer else None
        self.bil = new()
        self.outs = ([self.dem] if from_bayer else []) + [self.bil]
        cur, chain_outs = self.bil, []
        for op in ops:
            if op != OP_SKIP:
                cur = new()
            chain_outs.append(cur)
        self.outs += chain_outs
        if window.dtype != torch.int32 or not window.is_cuda:
            raise ValueError('window must be an int32 device tensor')
        self.keep = [window.contiguous(), _dev(sigma_color), _dev(sigma_space)] + \
                    [_dev(p) if p is not None else None for p in params]
        win, sc, ss = self.keep[:3]
        self._args = (_p(x), int(from_bayer), _p(self.dem), _p(self.bil), _p(win), _p(sc), _p(ss), int(max_window),
                      len(ops), (C.c_int * max(1, len(ops)))(*ops),
                      L.ptr_array([p.data_ptr() if p is not None else None for p in self.keep[3:]] or [None]),
                      L.ptr_array([o.data_ptr() if op != OP_SKIP else None for o, op in zip(chain_outs, ops)] or [None]),
                      n, h, w)

    def launch(self):
        L.call('risp_bilateral_chain_fwd', *self._args, _stream())
        return self.outs


def _u8_out(out, shape, device, align, apart=None, what=None):
    """the caller's byte buffer when it fits (uint8, contiguous, on the device, ``align``-byte aligned), else a new one.  ``apart``:
    uint8 images whose memory the caller's ``out`` must not share - a tile reads ``what`` ('rows', 'pixels') other tiles write"""
    if out is None:
        return torch.empty(shape, device=device, dtype=torch.uint8)
    if (out.dtype != torch.uint8 or out.device != device or tuple(out.shape) != tuple(shape) or not out.is_contiguous()
            or out.data_ptr() % align):
        raise ValueError('out must be a contiguous uint8 %s tensor on %s, %d-byte aligned; got %s %s'
                         % (tuple(shape), device, align, out.dtype, tuple(out.shape)))
    if apart is not None and out.data_ptr() < apart.data_ptr() + apart.numel() and apart.data_ptr() < out.data_ptr() + out.numel():
        raise ValueError('out shares memory with the images: a tile reads %s other tiles would have overwritten' % what)
    return out


def _u16_out(out, shape, device, apart=(), reader=None):
    """``_u8_out`` for the uint16 frames of a sensor pre-pass (8-byte aligned).  ``apart``: (tensor, what) pairs whose memory
    the caller's ``out`` must not share, because the ``reader`` reads neighbours that other threads write."""
    if out is None:
        return torch.empty(shape, device=device, dtype=torch.uint16)
    if out.dtype != torch.uint16 or out.device != device or tuple(out.shape) != shape or not out.is_contiguous() or out.data_ptr() % 8:
        raise ValueError('out must be a contiguous uint16 %s tensor on %s, 8-byte aligned; got %s %s'
                         % (shape, device, out.dtype, tuple(out.shape)))
    for t, what in apart:
        if out.data_ptr() < t.data_ptr() + t.numel() * t.element_size() and t.data_ptr() < out.data_ptr() + out.numel() * 2:
            raise ValueError('out shares memory with %s: the %s reads neighbours other threads would have overwritten' % (what, reader))
    return out


# Bayer phase of a sensor, by the mirror that makes its mosaic an RGGB one (RISP_CFA_*): bit 0 mirrors x, bit 1 mirrors y
CFA = {'rggb': 0, 'grbg': 1, 'gbrg': 2, 'bggr': 3}


def cfa_code(cfa):
    """'rggb' | 'grbg' | 'gbrg' | 'bggr' (any letter case) -> its RISP_CFA_* code"""
    code = CFA.get(cfa.lower()) if isinstance(cfa, str) else None
    if code is None:
        raise ValueError('unknown cfa %r: one of %s' % (cfa, ', '.join(CFA)))
    return code


def _check_mirror(flip, h, w):
    """a mirrored mosaic is RGGB only when the mirrored axis is even"""
    if (flip & 1 and w % 2) or (flip & 2 and h % 2):
        raise ValueError('a %d x %d mosaic mirrored along %s is not RGGB: the mirrored axis must be even'
                         % (h, w, 'x' if flip & 1 and w % 2 else 'y'))


# ---- what the serve_* wrappers share: each check stated once, in the order the wrappers apply them
DEMOSAIC = {'nearest': 0, 'bilinear': 1, 'laplacian': 2}      # RISP_DEMOSAIC_*


def _u16_frames(raw_u16):
    """contiguous (N,H,W) uint16 frames on the device -> (n, h, w)"""
    _need_gpu(raw_u16, 'raw')
    if raw_u16.dtype != torch.uint16 or raw_u16.dim() != 3 or not raw_u16.is_contiguous():
        raise ValueError('expected contiguous (N,H,W) uint16 frames, got %s %s' % (raw_u16.dtype, tuple(raw_u16.shape)))
    return tuple(raw_u16.shape)


def _check_counts(ops, params, post_ops=None, post_params=None):
    """one parameter block per stage, in one list or in the two around a stencil"""
    if post_ops is None:
        if len(ops) != len(params):
            raise ValueError('%d ops but %d parameter blocks' % (len(ops), len(params)))
    elif len(ops) != len(params) or len(post_ops) != len(post_params):
        raise ValueError('%d + %d ops but %d + %d parameter blocks' % (len(ops), len(post_ops), len(params), len(post_params)))


def _demosaic_code(demosaic):
    """a key of ``DEMOSAIC`` -> its RISP_DEMOSAIC_* code"""
    kind = DEMOSAIC.get(demosaic) if isinstance(demosaic, str) else None
    if kind is None:
        raise ValueError('unknown demosaic %r: one of %s' % (demosaic, ', '.join(DEMOSAIC)))
    return kind


def _black_level(black_level):
    """a sensor's black level -> the int"""
    if black_level != int(black_level) or not 0 <= black_level <= 65535:
        raise ValueError('black_level %r: an integer in 0 .. 65535' % (black_level,))
    return int(black_level)


def _sensor(black_level, cfa, h=None, w=None):
    """-> (black level as an int, RISP_CFA_* code); with ``h`` and ``w`` the mirror the phase asks for is checked against them"""
    code = cfa_code(cfa)
    black = _black_level(black_level)
    if h is not None:
        _check_mirror(code, h, w)
    return black, code


def _stage_args(ops, params):
    """-> (count, the ops as a C int array, the blocks as a C pointer array, the float32 device tensors to keep alive across the call)"""
    keep = [_dev(p) if p is not None else None for p in params]
    return (len(ops), (C.c_int * max(1, len(ops)))(*ops),
            L.ptr_array([p.data_ptr() if p is not None else None for p in keep] or [None]), keep)


def _bilateral_args(bilateral):
    """None or (window_i32, sigma_color, sigma_space, max_window) -> (the four C arguments, the tensors to keep alive)"""
    if bilateral is None:
        return (None, None, None, 0), []
    win, sc, ss, wmax = bilateral
    if win.dtype != torch.int32 or not win.is_cuda:
        raise ValueError('window must be an int32 device tensor')
    keep = [win.contiguous(), _dev(sc), _dev(ss)]
    return (_p(keep[0]), _p(keep[1]), _p(keep[2]), int(wmax)), keep


def quantise_u8(x, reverse_channels=False, out=None, flip=0):
    """``util.tensor2bgr`` on the device, batched: planar (N,C,H,W) in [0,1] -> packed (N,H,W,C) ``torch.uint8`` =
    clip(x * 255, 0, 255) truncated.  C is 1 or 3; ``reverse_channels`` stores RGB.  ``flip`` (bit 0: x, bit 1: y, the
    ``CFA`` codes) stores the mirrored image: output pixel (y, x) takes input (H-1-y, W-1-x) on the set axes
    (``risp_quantise_u8_flip``).  One launch (``risp_quantise_u8`` when ``flip`` is 0); with ``out`` given nothing is
    allocated and the host does not wait."""
    x = _dev(x, 'img')
    if x.dim() != 4 or x.shape[1] not in (1, 3):
        raise ValueError('expected a (N,1|3,H,W) tensor, got %s' % (tuple(x.shape),))
    if flip not in (0, 1, 2, 3):
        raise ValueError('flip %r: 0 .. 3 (bit 0 mirrors x, bit 1 mirrors y)' % (flip,))
    n, c, h, w = x.shape
    out = _u8_out(out, (n, h, w, c), x.device, 1)
    if flip:
        L.call('risp_quantise_u8_flip', _p(x), _p(out), n, c, h, w, int(bool(reverse_channels)), flip, _stream())
    else:
        L.call('risp_quantise_u8', _p(x), _p(out), n, c, h, w, int(bool(reverse_channels)), _stream())
    return out


def tile_blend_u8(patches, positions, full, stride, reverse_channels=False, out=None, flip=0):
    """``blend_tiles`` and ``quantise_u8`` in ONE launch (``risp_tile_blend_u8``): the tile stack ``patches`` (T,C,h,w), C 1 or
    3, with the (T,2) tile origins ``positions`` (y,x) -> the packed (H,W,C) ``torch.uint8`` image of the ``full`` = (H,W)
    frame.  The edges of the ramp mask are (size - stride) // 2, as ``blend_tiles`` derives them; ``reverse_channels`` and
    ``flip`` as in ``quantise_u8``.  Byte for byte ``quantise_u8(blend_tiles(patches, ...)[None], reverse_channels,
    flip=flip)[0]``; the fp32 frame is never written.  With ``out`` given nothing is allocated - apart from ``positions``
    when it is not yet an int32 device tensor - and the host does not wait."""
    patches = _dev(patches, 'patches')
    if patches.dim() != 4 or patches.shape[1] not in (1, 3):
        raise ValueError('expected a (T,1|3,h,w) tile stack, got %s' % (tuple(patches.shape),))
    if flip not in (0, 1, 2, 3):
        raise ValueError('flip %r: 0 .. 3 (bit 0 mirrors x, bit 1 mirrors y)' % (flip,))
    t, c, h, w = patches.shape
    if not (isinstance(positions, torch.Tensor) and positions.is_cuda and positions.dtype == torch.int32
            and positions.is_contiguous()):
        positions = torch.as_tensor(positions).to(device=patches.device, dtype=torch.int32).contiguous()
    if tuple(positions.shape) != (t, 2):
        raise ValueError('positions must be (T=%d,2), got %s' % (t, tuple(positions.shape)))
    eh, ew = (h - int(stride[0])) // 2, (w - int(stride[1])) // 2
    out = _u8_out(out, (int(full[0]), int(full[1]), c), patches.device, 1)
    L.call('risp_tile_blend_u8', _p(patches), _p(out), _p(positions), t, c, int(full[0]), int(full[1]), h, w, eh, ew,
           int(bool(reverse_channels)), flip, _stream())
    return out


def serve_u8(raw_u16, divisor, ops, params, bilateral=None, reverse_channels=False, out=None, black_level=0, cfa='rggb'):
    """A fixed pipeline as an ISP in ONE launch (``risp_serve_u8``): (N,H,W) ``torch.uint16`` RGGB frames on the device ->
    (N,H,W,3) ``torch.uint8``.  sample / divisor, nearest demosaic, the bilateral when ``bilateral = (window_i32,
    sigma_color, sigma_space, max_window)`` is given (max_window 1 or 3), the element-wise stages ``ops`` (OP_*) with their
    per-image blocks ``params`` (None for OP_SKIP), then ``quantise_u8``'s conversion; only the result is stored, and its
    bytes are those of the fp32 kernels followed by ``tensor2bgr``.  H even, W % 4 == 0.  With ``out`` given nothing is
    allocated and the host does not wait.

    ``black_level`` (an integer, 0 .. 65535) and ``cfa`` (a key of ``CFA``) describe a real sensor: the input expression
    becomes max(sample - black_level, 0) / divisor, the subtraction in integers (``divisor`` is then white level - black
    level), and a GRBG / GBRG / BGGR mosaic is read mirrored and its image stored un-mirrored - still one launch
    (``risp_serve_u8_cfa``) and byte for byte ``flip(serve_u8(flip(clamp(raw - black_level)), divisor, ...))``."""
    n, h, w = _u16_frames(raw_u16)
    _check_counts(ops, params)
    black, code = _sensor(black_level, cfa, h, w)
    out = _u8_out(out, (n, h, w, 3), raw_u16.device, 4)
    count, oparr, blocks, keep = _stage_args(ops, params)
    bil, keep_bil = _bilateral_args(bilateral)
    args = (_p(raw_u16), float(divisor), *bil, count, oparr, blocks, _p(out), int(bool(reverse_channels)), n, h, w)
    if code or black:
        L.call('risp_serve_u8_cfa', *args, black, code, _stream())
    else:
        L.call('risp_serve_u8', *args, _stream())
    return out


def serve_classical_u8(raw_u16, divisor, demosaic, ops, params, reverse_channels=False, out=None, black_level=0, cfa='rggb'):
    """A classical pipeline as an ISP in ONE launch (``risp_serve_classical_u8``): (N,H,W) ``torch.uint16`` frames on the
    device -> (N,H,W,3) ``torch.uint8``.  max(sample - black_level, 0) / divisor, the demosaic (a key of ``DEMOSAIC``:
    nearest, or the classical bilinear / Malvar-He-Cutler ``origin_demosaic`` with its 8-bit rounding), the stages ``ops``
    with their per-image blocks ``params`` (None for OP_SKIP) - the element-wise OP_* of ``serve_u8`` and the two tone curves
    OP_TONE_CRYSIS ((N,1): lum_adapted) and OP_TONE_FILMIC ((N,2): white_point, exposure_bias in 1 .. 10), which are
    ``origin_tonemap`` with scales (255, 255) - then ``quantise_u8``'s conversion.  Only the result is stored; its bytes
    are those of ``raw_crops`` -> ``origin_demosaic`` / ``chain_forward`` / ``origin_tonemap`` -> ``quantise_u8``.  No
    bilateral.  H even and >= 4, W % 4 == 0; ``black_level`` and ``cfa`` as in ``serve_u8``.  With ``out`` given nothing
    is allocated and the host does not wait."""
    n, h, w = _u16_frames(raw_u16)
    _check_counts(ops, params)
    kind = _demosaic_code(demosaic)
    black, code = _sensor(black_level, cfa, h, w)
    out = _u8_out(out, (n, h, w, 3), raw_u16.device, 4)
    count, oparr, blocks, keep = _stage_args(ops, params)
    L.call('risp_serve_classical_u8', _p(raw_u16), float(divisor), kind, count, oparr, blocks, _p(out),
           int(bool(reverse_channels)), n, h, w, black, code, _stream())
    return out


# YUV 4:2:0 (NV12) out: cy[4], cu[4], cv[4], each row kR, kG, kB, offset (include/risp.h states the format).  The offsets
# carry the rounding constant 128 and the plane offset (16 << 8, 128 << 8); the full-range chroma rows use 127, not 128, so
# that no sum leaves 0 .. 65535 and the kernels need no clamp
NV12_MATRIX = {
    'bt601_full': (77, 150, 29, 128, -43, -84, 127, 32896, 127, -106, -21, 32896),
    'bt601_video': (66, 129, 25, 4224, -38, -74, 112, 32896, 112, -94, -18, 32896),
    'bt709_full': (54, 183, 19, 128, -29, -98, 127, 32896, 127, -115, -12, 32896),
    'bt709_video': (47, 157, 16, 4224, -26, -86, 112, 32896, 112, -102, -10, 32896),
}


def nv12_matrix(matrix):
    """A key of ``NV12_MATRIX`` or twelve integers -> the twelve integers the NV12 entry points take.  A matrix is accepted
    when every sum stays in 0 .. 65535 for all codes: per row |k| <= 256, offset + 255 * (sum of positive k) <= 65535 and
    offset + 255 * (sum of negative k) >= 0."""
    if isinstance(matrix, str):
        coef = NV12_MATRIX.get(matrix)
        if coef is None:
            raise ValueError('unknown yuv matrix %r: one of %s, or twelve integers' % (matrix, ', '.join(NV12_MATRIX)))
        return coef
    try:
        coef = tuple(int(k) for k in matrix)
        exact = all(k == v for k, v in zip(coef, matrix))
    except (TypeError, ValueError):
        coef, exact = (), False
    if len(coef) != 12 or not exact:
        raise ValueError('a yuv matrix is a key of NV12_MATRIX or twelve integers, got %r' % (matrix,))
    for r, name in enumerate(('cy', 'cu', 'cv')):
        k = coef[4 * r:4 * r + 4]
        if (max(abs(v) for v in k[:3]) > 256 or k[3] + 255 * sum(v for v in k[:3] if v > 0) > 65535
                or k[3] + 255 * sum(v for v in k[:3] if v < 0) < 0):
            raise ValueError('yuv matrix row %s %s leaves 0 .. 65535 for some codes (or a coefficient is outside -256 .. 256)'
                             % (name, k))
    return coef


# ---- what the bgr8_* wrappers share: each check stated once; a wrapper keeps the order in which it applies them
def _bgr8_images(img_u8):
    """(N,H,W,3) or (H,W,3) uint8 images, on any device -> (n, h, w, the shape in front of H: (N,) or ())"""
    if not isinstance(img_u8, torch.Tensor) or img_u8.dtype != torch.uint8 or img_u8.dim() not in (3, 4) or img_u8.shape[-1] != 3:
        raise ValueError('expected (N,H,W,3) or (H,W,3) uint8 images, got %s %s'
                         % (getattr(img_u8, 'dtype', type(img_u8)), tuple(getattr(img_u8, 'shape', ()))))
    return img_u8.shape[0] if img_u8.dim() == 4 else 1, img_u8.shape[-3], img_u8.shape[-2], tuple(img_u8.shape[:-3])


def _bgr8_batch(img_u8, n):
    """the ``n`` images of one tiled launch: on the device, at most 65535 (the grid's z), contiguous - a copy where they are not"""
    _need_gpu(img_u8, 'img')
    if n > 65535:
        raise ValueError('%d images in one call: at most 65535' % n)
    return img_u8.contiguous()


def _channels(channels):
    """'bgr' | 'rgb' -> the ``rgb_in`` argument, 0 | 1"""
    if channels not in ('bgr', 'rgb'):
        raise ValueError("channels %r: 'bgr' or 'rgb'" % (channels,))
    return int(channels == 'rgb')


def _check_420(h, w, what='image', names='H and W', least=0):
    """4:2:0 has one chroma sample per 2 x 2 quad: both sizes even (and at least ``least``)"""
    if h % 2 or w % 2 or h < least or w < least:
        raise ValueError('a %d x %d %s has no 4:2:0 form: %s must be even' % (h, w, what, names))


def _coef12(coef):
    """the twelve integers of ``nv12_matrix`` as the C array of the entry points, None as None"""
    return None if coef is None else (C.c_int * 12)(*coef)


def bgr8_to_nv12(img_u8, matrix='bt601_full', channels='bgr', out=None):
    """Packed 8-bit images to YUV 4:2:0 in ONE launch (``risp_bgr8_to_nv12``): (N,H,W,3) or (H,W,3) ``torch.uint8`` on the
    device, ``channels`` 'bgr' or 'rgb', H and W even -> (N,3H/2,W) or (3H/2,W) ``torch.uint8``: H rows of Y, then H/2 rows
    of U V U V ..., chroma the matrix of the rounded mean of a 2 x 2 quad's codes (``nv12_matrix``; the integer definition
    is in include/risp.h).  With ``out`` given nothing is allocated and the host does not wait."""
    _need_gpu(img_u8, 'img')                            # (first here, and no limit on N: a grid-stride launch, not a tiled one)
    n, h, w, lead = _bgr8_images(img_u8)
    rgb = _channels(channels)
    coef = nv12_matrix(matrix)
    _check_420(h, w, least=2)
    img_u8 = img_u8.contiguous()
    out = _u8_out(out, lead + (h + h // 2, w), img_u8.device, 1)
    L.call('risp_bgr8_to_nv12', _p(img_u8), _p(out), _coef12(coef), rgb, n, h, w, _stream())
    return out


# ---- a scaled, cropped output (risp_resize.hip; include/risp.h has the definition to the bit)
RESAMPLE = ('box', 'triangle', 'bicubic')
RESIZE_MAX_TAPS = 32                    # RISP_RESIZE_MAX_TAPS
RESIZE_TILE_W = 64                      # RISP_RESIZE_TILE_W: output columns of a workgroup
RESIZE_TILE_ROWS = (16, 8, 4, 2)        # output rows of a workgroup: the first whose source-row span fits the LDS budget
RESIZE_LDS_BYTES = 65536                # RISP_RESIZE_LDS_BYTES
_RESAMPLE_RADIUS = {'box': 0.5, 'triangle': 1.0, 'bicubic': 2.0}
_RESAMPLE_LIMIT = {'box': '32:1', 'triangle': '16:1', 'bicubic': '8:1'}


def _resample_weight(kernel, x):
    """the three kernels on a float: comparisons and + - * only"""
    if kernel == 'box':
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if x < 0.0:
        x = -x
    if kernel == 'triangle':
        return 1.0 - x if x < 1.0 else 0.0
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


RESIZE_HOST_CACHE = 256                 # host tables and tile plans kept (least recently used beyond that)
_RESAMPLE_BASE, _RESAMPLE_TAPS = {}, {}


def _lru_get(cache, key):
    hit = cache.pop(key, None)
    if hit is not None:
        cache[key] = hit                        # a dict keeps insertion order: the most recently used key is last
    return hit


def _lru_put(cache, key, value):
    while len(cache) >= RESIZE_HOST_CACHE:
        cache.pop(next(iter(cache)))
    cache[key] = value
    return value


def resample_taps(S, D, kernel, offset=0):
    """The integer tap table of one axis, built on the host (no device is touched): a source window of ``S`` samples at
    ``offset`` in the image resampled to ``D`` samples with ``kernel`` (a name of ``RESAMPLE``) -> (start (D,) numpy int32,
    weight (D,T) numpy int16): output i is the Q14 sum of weight[i][k] * source[start[i] + k].  Every row sums to exactly
    16384, offset <= start and start + T <= offset + S, starts never decrease on a reduction, and only IEEE basic operations on float64 enter, so every machine
    builds the same integers (include/risp.h has the definition; tests/resize_reference.py restates it).  A geometry whose
    support window hi - lo passes ``RESIZE_MAX_TAPS`` samples for some output is refused (T <= 32 for everything served):
    reductions up to 32:1 (box), 16:1 (triangle), 8:1 (bicubic).  The offset enters by addition only: the table of (S, D, kernel)
    is built once, a moving window of one size costs an addition per position.  The last ``RESIZE_HOST_CACHE`` tables are kept;
    the arrays returned are read-only."""
    import numpy as np
    if kernel not in RESAMPLE:
        raise ValueError('unknown resample %r: one of %s' % (kernel, ', '.join(RESAMPLE)))
    S, D, offset = _small_int(S, 1, 1 << 24), _small_int(D, 1, 1 << 24), _small_int(offset, 0, 1 << 24)
    if S is None or D is None or offset is None:
        raise ValueError('resample_taps: a source length and an output length in 1 .. 2^24 and an offset >= 0')
    key = (S, D, kernel, offset)
    hit = _lru_get(_RESAMPLE_TAPS, key)
    if hit is not None:
        return hit
    base = _lru_get(_RESAMPLE_BASE, key[:3])
    if base is None:
        base = _lru_put(_RESAMPLE_BASE, key[:3], _resample_table(S, D, kernel))
    start = base[0] + np.int32(offset)
    start.setflags(write=False)
    return _lru_put(_RESAMPLE_TAPS, key, (start, base[1]))


def _resample_table(S, D, kernel):
    """``resample_taps`` at offset 0, built from the definition"""
    import math
    import numpy as np
    scale = S / D
    fs = max(scale, 1.0)
    support = _RESAMPLE_RADIUS[kernel] * fs
    los, rows = [], []
    for i in range(D):
        c = (i + 0.5) * scale
        lo, hi = max(int(c - support + 0.5), 0), min(int(c + support + 0.5), S)
        if hi - lo > RESIZE_MAX_TAPS:
            # judged on the support window, not on the trimmed row: whether an edge tap rounds to zero is an accident of the
            # quantisation, and a table is refused before it is built
            raise ValueError('resample %r from %d to %d samples: a support window of %d samples, at most RESIZE_MAX_TAPS = %d: '
                             'the largest served reduction is %s' % (kernel, S, D, hi - lo, RESIZE_MAX_TAPS, _RESAMPLE_LIMIT[kernel]))
        w = [_resample_weight(kernel, (k + lo - c + 0.5) / fs) for k in range(hi - lo)]
        s = 0.0
        for v in w:
            s += v
        if not s > 0.0:
            raise ValueError('resample %r from %d to %d samples: output %d has no weight' % (kernel, S, D, i))
        q = [int(math.floor(v / s * 16384 + 0.5)) for v in w]
        q[q.index(max(q))] += 16384 - sum(q)
        while q[0] == 0:
            q.pop(0)
            lo += 1
        while q[-1] == 0:
            q.pop()
        los.append(lo)
        rows.append(q)
    T = max(len(q) for q in rows)
    start, weight = np.zeros(D, dtype=np.int32), np.zeros((D, T), dtype=np.int16)
    for i, (lo, q) in enumerate(zip(los, rows)):
        at = min(lo, S - T)
        weight[i, lo - at:lo - at + len(q)] = q
        start[i] = at
    start.setflags(write=False)
    weight.setflags(write=False)
    return start, weight


def resize_check(out_size, out_window, resample, H, W, nv12=False):
    """The resize keywords for H x W images, checked on the host before anything is launched -> ((OH, OW), (y0, x0, h, w))
    normalised.  ``out_window=(y0, x0, h, w)`` lies inside the image (None: the whole image); ``out_size=(OH, OW)`` is at least
    1 x 1 (None: the window's size, a crop); ``resample`` is a name of ``RESAMPLE``; with ``nv12`` OH and OW are even; neither
    axis needs more than ``RESIZE_MAX_TAPS`` taps; the output has at most 65535 row tiles (``resize_tile_rows``)."""
    if resample not in RESAMPLE:
        raise ValueError('unknown resample %r: one of %s' % (resample, ', '.join(RESAMPLE)))
    H, W = int(H), int(W)
    if out_window is None:
        win = (0, 0, H, W)
    else:
        try:
            win = tuple(_small_int(v, 0, 1 << 24) for v in out_window)
        except TypeError:
            win = ()
        if len(win) != 4 or None in win:
            raise ValueError('out_window %r: (y0, x0, h, w) as integers' % (out_window,))
        if win[2] < 1 or win[3] < 1 or win[0] + win[2] > H or win[1] + win[3] > W:
            raise ValueError('out_window %r lies outside the %d x %d image (or is empty)' % (out_window, H, W))
    if out_size is None:
        size = win[2:]
    else:
        try:
            size = tuple(_small_int(v, 1, 1 << 24) for v in out_size)
        except TypeError:
            size = ()
        if len(size) != 2 or None in size:
            raise ValueError('out_size %r: (OH, OW) as integers >= 1' % (out_size,))
    if nv12:
        _check_420(size[0], size[1], 'output', 'OH and OW')
    resample_taps(win[2], size[0], resample, win[0])
    resample_taps(win[3], size[1], resample, win[1])
    rows = resize_tile_rows(win[2], size[0], resample, win[0])[0]
    if (size[0] + rows - 1) // rows > 65535:
        raise ValueError('out_size %r: %d output rows in tiles of %d are more than 65535 row tiles' % (out_size, size[0], rows))
    return size, win


_RESIZE_TABLES = {}


def release_resize_tables():
    """Drop the device tap tables of ``bgr8_resize`` (every device).  They are kept per (axis geometry with its offset, kernel,
    device) and never dropped otherwise - a captured graph holds their addresses, as it holds ``frame_geometry``'s origins -, so
    a caller that moves or zooms its window through many positions uploads two small tables (4 + 2 T bytes per output row or
    column) per new position and calls this between sessions; no graph captured before may be replayed after."""
    _RESIZE_TABLES.clear()


def _resize_axis(S, D, kernel, offset, device):
    """(start, weight) of ``resample_taps`` as device tensors with T and the host's start, kept per (axis geometry, kernel,
    device) until ``release_resize_tables``: a warm call uploads nothing"""
    key = (S, D, kernel, offset, device.type, device.index)
    hit = _RESIZE_TABLES.get(key)
    if hit is None:
        start, weight = resample_taps(S, D, kernel, offset)
        hit = _RESIZE_TABLES[key] = (torch.from_numpy(start.copy()).to(device), torch.from_numpy(weight.copy()).to(device),
                                     weight.shape[1], start)
    return hit


_RESIZE_TILES = {}


def resize_tile_rows(S, D, kernel, offset=0):
    """(tile rows, span) of the resize launch for the vertical axis ``resample_taps(S, D, kernel, offset)``: the first row count
    of ``RESIZE_TILE_ROWS`` whose largest source-row span over all tiles - the largest start of the tile's rows + T - their
    smallest - fits ``RESIZE_LDS_BYTES`` beside the table slices (the C side checks the same sum).  The last ``RESIZE_HOST_CACHE``
    answers are kept."""
    key = (int(S), int(D), kernel, int(offset))
    hit = _lru_get(_RESIZE_TILES, key)
    if hit is None:
        start, weight = resample_taps(S, D, kernel, offset)
        D, T = weight.shape
        for rows in RESIZE_TILE_ROWS:
            # (starts are not monotone everywhere - a bicubic enlargement trims the zero outer taps of an output that falls on a
            # sample -, so a tile's rows run from its smallest start to its largest plus T)
            span = max(int(start[i:i + rows].max()) + T - int(start[i:i + rows].min()) for i in range(0, D, rows))
            # (the horizontal table has at most RESIZE_MAX_TAPS taps too)
            if (span * RESIZE_TILE_W * 3 + (RESIZE_TILE_W + rows) * 4
                    + (RESIZE_TILE_W * RESIZE_MAX_TAPS + rows * T) * 2 <= RESIZE_LDS_BYTES):
                break
        else:
            raise ValueError('resample %r from %d to %d rows: %d source rows for %d output rows do not fit the launch'
                             % (kernel, S, D, span, rows))
        hit = _lru_put(_RESIZE_TILES, key, (rows, span))
    return hit


def bgr8_resize(img_u8, out_size=None, out_window=None, resample='triangle', nv12=None, channels='bgr', out=None):
    """Packed 8-bit images scaled and cropped in ONE launch (``risp_bgr8_resize``): (N,H,W,3) or (H,W,3) ``torch.uint8`` on the
    device -> (N,OH,OW,3) or (OH,OW,3), the window ``out_window=(y0, x0, h, w)`` of every image (default: all of it)
    resampled to ``out_size=(OH, OW)`` (default: the window's size - a crop, one tap of 16384) with ``resample`` 'box',
    'triangle' or 'bicubic': separable, antialiased on reduction, horizontal first, Q14 integer taps whose rows sum to 16384
    (``resample_taps``; include/risp.h fixes every bit).  With ``nv12`` (a matrix as ``nv12_matrix`` takes it) the same launch
    stores (N,3*OH/2,OW) YUV 4:2:0 instead, byte for byte ``bgr8_to_nv12`` of the packed result; ``channels`` 'bgr' or 'rgb'
    then names the order of the input (OH, OW even, ``out`` 4-byte aligned).  No alignment is asked of the images or of a
    packed ``out``; ``out`` must not share memory with the images.  The tap tables live on the device per (axis geometry,
    kernel, device) until ``release_resize_tables``: a warm call on contiguous images uploads nothing, with ``out`` given
    allocates nothing, and the host never waits; images that are not contiguous are copied first, which allocates."""
    n, h, w, lead = _bgr8_images(img_u8)
    rgb = _channels(channels)
    coef = None if nv12 is None else nv12_matrix(nv12)
    (oh, ow), (y0, x0, wh, ww) = resize_check(out_size, out_window, resample, h, w, coef is not None)
    img_u8 = _bgr8_batch(img_u8, n)
    shape = lead + ((oh, ow, 3) if coef is None else (oh + oh // 2, ow))
    out = _u8_out(out, shape, img_u8.device, 1 if coef is None else 4, img_u8, 'rows')
    xs, xw, tx, _ = _resize_axis(ww, ow, resample, x0, img_u8.device)
    ys, yw, ty, _ = _resize_axis(wh, oh, resample, y0, img_u8.device)
    rows, span = resize_tile_rows(wh, oh, resample, y0)
    L.call('risp_bgr8_resize', _p(img_u8), _p(out), _p(xs), _p(xw), tx, _p(ys), _p(yw), ty, rows, span, _coef12(coef), rgb,
           n, h, w, oh, ow, _stream())
    return out


# ---- a geometry-corrected output: the mesh warp (risp_warp.hip; include/risp.h has the definition to the bit)
WARP_KERNELS = ('bilinear', 'bicubic')
WARP_TILE_W = 64                        # RISP_WARP_TILE_W: output columns of a workgroup
WARP_TILE_H = 16                        # RISP_WARP_TILE_H: output rows of a workgroup
WARP_LDS_BYTES = 65536                  # RISP_WARP_LDS_BYTES: what a tile's staged source box may take, weights and tile included
_WARP_CELLS = (4, 8, 16, 32, 64, 128, 256)
_WARP_MAX = 1 << 23                     # sizes: a Q8 coordinate fits int32


def warp_cubic_table():
    """The Catmull-Rom weights of the 'bicubic' warp: (256,4) numpy int16, Q11, row f for the phase f / 256, from the integer
    formula of include/risp.h - every row sums to exactly 2048.  The kernel computes the same rows itself; this serves the
    reference's cross-check and the documents."""
    import numpy as np
    f = np.arange(256, dtype=np.int64)
    n = np.stack([-f ** 3 + 512 * f ** 2 - 65536 * f, 3 * f ** 3 - 1280 * f ** 2 + (1 << 25),
                  -3 * f ** 3 + 1024 * f ** 2 + 65536 * f, f ** 3 - 256 * f ** 2], axis=1)
    q = (n + 8192) >> 14
    q[np.arange(256), q.argmax(axis=1)] += 2048 - q.sum(axis=1)         # argmax: the first index of the largest
    return q.astype(np.int16)


def _warp_size(size, what='size'):
    try:
        wh, ww = (_small_int(v, 1, _WARP_MAX) for v in size)
    except (TypeError, ValueError):
        wh = ww = None
    if wh is None or ww is None:
        raise ValueError('warp %s %r: (WH, WW) as integers in 1 .. 2^23' % (what, size))
    return wh, ww


def _warp_cell(cell):
    if isinstance(cell, bool) or not isinstance(cell, int) or cell not in _WARP_CELLS:
        raise ValueError('warp cell %r: a power of two from 4 to 256' % (cell,))
    return cell.bit_length() - 1


def warp_check(warp, H, W, device=None, nv12=False):
    """A warp ``(mesh, cell, (WH, WW), kernel)`` for H x W images, checked on the host before anything is launched ->
    (mesh, k, (WH, WW), kernel) with cell = 1 << k.  ``cell``: a power of two from 4 to 256; WH, WW: integers >= 1 (at most
    2^23, as H and W; at most 65535 row tiles), even with ``nv12``; ``kernel``: a name of ``WARP_KERNELS``; ``mesh``: a
    contiguous (MH,MW,2) ``torch.int32`` tensor, 8-byte aligned, MH == (WH-1) // cell + 2 and MW == (WW-1) // cell + 2 exactly,
    on ``device`` when one is given - node (i,j) holds the Q8 source (y, x) of output pixel (i * cell, j * cell)
    (include/risp.h has the definition).  Every int32 value is legal, so the mesh is never read here and the host never waits."""
    try:
        mesh, cell, size, kernel = warp
    except (TypeError, ValueError):
        raise ValueError('a warp is (mesh, cell, (WH, WW), kernel): an (MH,MW,2) int32 tensor, the cell size in pixels, the output '
                         "size and 'bilinear' or 'bicubic'") from None
    k = _warp_cell(cell)
    wh, ww = _warp_size(size)
    if _small_int(H, 1, _WARP_MAX) is None or _small_int(W, 1, _WARP_MAX) is None:
        raise ValueError('warp of %r x %r images: H and W in 1 .. 2^23' % (H, W))
    if (wh + WARP_TILE_H - 1) // WARP_TILE_H > 65535:
        raise ValueError('warp size %r: %d output rows in tiles of %d are more than 65535 row tiles' % (size, wh, WARP_TILE_H))
    if nv12:
        _check_420(wh, ww, 'warp output', 'WH and WW')
    if kernel not in WARP_KERNELS:
        raise ValueError('unknown warp kernel %r: one of %s' % (kernel, ', '.join(WARP_KERNELS)))
    if not isinstance(mesh, torch.Tensor) or mesh.dtype != torch.int32:
        raise ValueError('a warp mesh must be an int32 tensor (Q8 coordinates), got %s' % (getattr(mesh, 'dtype', type(mesh)),))
    mh, mw = ((wh - 1) >> k) + 2, ((ww - 1) >> k) + 2
    if tuple(mesh.shape) != (mh, mw, 2) or not mesh.is_contiguous():
        raise ValueError('the warp mesh of a %d x %d output with cell %d must be contiguous (%d,%d,2): (WH-1) // cell + 2 by '
                         '(WW-1) // cell + 2 nodes of (y, x); got %s' % (wh, ww, cell, mh, mw, tuple(mesh.shape)))
    if device is not None and mesh.device != device:
        raise ValueError('the warp mesh lives on %s, the images on %s' % (mesh.device, device))
    if mesh.data_ptr() % 8:
        raise ValueError('the warp mesh must be 8-byte aligned')
    return mesh, k, (wh, ww), kernel


def bgr8_warp(img_u8, warp, out=None, stage=None):
    """Packed 8-bit images through a mesh warp in ONE launch (``risp_bgr8_warp``): (N,H,W,3) or (H,W,3) ``torch.uint8`` on the
    device -> (N,WH,WW,3) or (WH,WW,3), ``warp = (mesh, cell, (WH, WW), kernel)`` as ``warp_check`` takes it - the mesh on the
    images' device; one mesh serves every image.  Output pixel (y,x) takes the source coordinate interpolated bilinearly from
    the four nodes of its cell, clamped into the image (replicate border), and the 'bilinear' or 'bicubic' (Catmull-Rom, Q11)
    taps there: an integer function, include/risp.h fixes every bit.  ``stage``: 'lds' / 1 - a workgroup stages the source box
    of its tile in LDS where it fits - or 'gather' / 0 - every tile samples global memory -, the same bytes either way; None
    takes what ``pipeline_fusion.warp_stage(kernel)`` says.  No alignment is asked of the images or of ``out``; ``out`` must not
    share memory with the images.  With ``out`` given a call on contiguous images allocates nothing and the host never waits;
    images that are not contiguous are copied first, which allocates."""
    n, h, w, lead = _bgr8_images(img_u8)
    mesh, k, (wh, ww), kernel = warp_check(warp, h, w, img_u8.device)
    if stage is None:
        from .codes.models.modules.pipeline_fusion import warp_stage
        stage = warp_stage(kernel)
    if isinstance(stage, bool) or stage not in (0, 1, 'gather', 'lds'):
        raise ValueError("warp stage %r: 'lds' / 1, 'gather' / 0 or None" % (stage,))
    img_u8 = _bgr8_batch(img_u8, n)
    out = _u8_out(out, lead + (wh, ww, 3), img_u8.device, 1, img_u8, 'pixels')
    L.call('risp_bgr8_warp', _p(img_u8), _p(out), _p(mesh), k, mesh.shape[0], mesh.shape[1], WARP_KERNELS.index(kernel),
           int(stage in (1, 'lds')), n, h, w, wh, ww, _stream())
    return out


def warp_mesh(fn, size, cell):
    """Host builder of a warp mesh: ``fn(y, x) -> (sy, sx)`` gives the source pixel coordinates (floats; 0 is the centre of
    source pixel 0) of output pixel coordinates, and is called ONCE on the node coordinates - float64 numpy arrays of shapes
    (MH,1) and (1,MW) holding i * cell and j * cell, the row and column behind the last pixel included; what it returns is
    broadcast to (MH,MW).  -> the (MH,MW,2) ``torch.int32`` mesh of ``size = (WH, WW)`` on the host (move it to the device once):
    floor(v * 256 + 0.5), saturated to int32.  A value that is not a number is refused.  Where ``fn`` uses IEEE basic operations
    only, every machine builds the same integers."""
    import numpy as np
    k = _warp_cell(cell)
    wh, ww = _warp_size(size)
    mh, mw = ((wh - 1) >> k) + 2, ((ww - 1) >> k) + 2
    y = (np.arange(mh, dtype=np.float64) * cell)[:, None]
    x = (np.arange(mw, dtype=np.float64) * cell)[None, :]
    got = fn(y, x)
    try:
        sy, sx = got
    except (TypeError, ValueError):
        raise ValueError('warp_mesh: fn(y, x) must return (sy, sx), got %s' % (type(got).__name__,)) from None
    nodes = np.empty((mh, mw, 2), dtype=np.float64)
    try:
        nodes[..., 0] = np.asarray(sy, dtype=np.float64)
        nodes[..., 1] = np.asarray(sx, dtype=np.float64)
    except ValueError:
        raise ValueError('warp_mesh: fn returned shapes %s and %s, which do not broadcast to the (%d,%d) nodes'
                         % (np.shape(sy), np.shape(sx), mh, mw)) from None
    if np.isnan(nodes).any():
        raise ValueError('warp_mesh: fn returned values that are not numbers at %d nodes' % int(np.isnan(nodes).sum()))
    q = np.floor(nodes * 256.0 + 0.5)
    q = np.minimum(np.maximum(q, -2147483648.0), 2147483647.0)
    return torch.from_numpy(q.astype(np.int64).astype(np.int32))


def warp_homography(matrix3x3, size, cell):
    """Host builder: the mesh of a projective map.  ``matrix3x3`` takes an OUTPUT pixel to its SOURCE pixel,
    (sx * d, sy * d, d) = M (x, y, 1) - x first, as OpenCV's ``warpPerspective`` with WARP_INVERSE_MAP.  Identity, flips,
    90-degree turns, rotation, zoom, shift (affine maps: exact to within 1 Q8 unit per pixel) and keystone (interpolated
    bilinearly inside a cell: take smaller cells for a stronger one).  A node whose denominator d is not positive is refused.
    -> (MH,MW,2) ``torch.int32`` on the host, as ``warp_mesh``."""
    import numpy as np
    try:
        m = np.asarray(matrix3x3.detach().cpu().numpy() if isinstance(matrix3x3, torch.Tensor) else matrix3x3, dtype=np.float64)
    except (TypeError, ValueError):
        m = np.zeros(0)
    if m.shape != (3, 3) or not np.isfinite(m).all():
        raise ValueError('warp_homography: a finite 3 x 3 matrix, got %r' % (matrix3x3,))

    def fn(y, x):
        d = m[2, 0] * x + m[2, 1] * y + m[2, 2]
        if not (d > 0.0).all():
            raise ValueError('warp_homography: the denominator is %g at node %s: it must be positive at every node'
                             % (d.min(), tuple(int(v) for v in np.unravel_index(d.argmin(), d.shape))))
        return (m[1, 0] * x + m[1, 1] * y + m[1, 2]) / d, (m[0, 0] * x + m[0, 1] * y + m[0, 2]) / d
    return warp_mesh(fn, size, cell)


def warp_radial_source(H, W, size, k1, k2=0.0, centre=None, zoom=1.0):
    """``fn(y, x) -> (sy, sx)`` of ``warp_radial``: the Brown radial model on float64 arrays of output pixel coordinates."""
    wh, ww = _warp_size(size)
    if _small_int(H, 1, _WARP_MAX) is None or _small_int(W, 1, _WARP_MAX) is None:
        raise ValueError('warp_radial of %r x %r images: H and W in 1 .. 2^23' % (H, W))
    k1, k2, zoom = float(k1), float(k2), float(zoom)
    if not (k1 == k1 and k2 == k2 and zoom > 0.0 and abs(k1) < float('inf') and abs(k2) < float('inf') and zoom < float('inf')):
        raise ValueError('warp_radial: finite k1, k2 and a finite zoom > 0, got %r, %r, %r' % (k1, k2, zoom))
    try:
        cy, cx = ((H - 1) / 2.0, (W - 1) / 2.0) if centre is None else (float(centre[0]), float(centre[1]))
    except (TypeError, ValueError, IndexError):
        raise ValueError('warp_radial: centre %r: (cy, cx) in source pixels' % (centre,)) from None
    quarter = (float(H) * H + float(W) * W) / 4.0          # the square of half the source diagonal

    def fn(y, x):
        # the output frame mapped onto the source frame, pixel centres on pixel centres of the scaled grid
        dy, dx = (y + 0.5) * (H / wh) - 0.5 - cy, (x + 0.5) * (W / ww) - 0.5 - cx
        r2 = (dy * dy + dx * dx) / quarter
        s = zoom * (1.0 + k1 * r2 + k2 * (r2 * r2))
        return cy + dy * s, cx + dx * s
    return fn


def warp_radial(H, W, size, cell, k1, k2=0.0, centre=None, zoom=1.0):
    """Host builder: the mesh that corrects a radial lens distortion of H x W images (the Brown model, as DNG's
    ``WarpRectilinear`` without its tangential terms): source = centre + (p - centre) * zoom * (1 + k1 r^2 + k2 r^4), p the
    output pixel mapped onto the source frame ((y + 0.5) * H / WH - 0.5), r = |p - centre| over half the source diagonal,
    ``centre`` (cy, cx) in source pixels (default: the middle).  k1 < 0 corrects a pincushion, k1 > 0 a barrel distortion;
    ``zoom`` < 1 magnifies.  Only + - * / on float64 enter.  The model is interpolated bilinearly inside a cell: the error falls
    with the square of the cell (DESIGN.md 4.6 has figures).  -> (MH,MW,2) ``torch.int32`` on the host, as ``warp_mesh``."""
    return warp_mesh(warp_radial_source(H, W, size, k1, k2, centre, zoom), size, cell)


# ---- output sharpening: the luma edge enhancement (risp_sharpen.hip; include/risp.h has the definition to the bit)
SHARPEN_RADII = (1, 2)
SHARPEN_MAX_AMOUNT = 4095               # RISP_SHARPEN_MAX_AMOUNT: Q8, 256 is a gain of 1.0
SHARPEN_TILE_H = 16                     # RISP_SHARPEN_TILE_H: rows of a workgroup
_SHARPEN_MAX = 1 << 24                  # sizes


def sharpen_check(sharpen, nv12=False, H=None, W=None):
    """A sharpening ``(amount, threshold, limit, radius)``, checked on the host before anything is launched -> the four as
    ints.  ``amount``: 0 .. 4095, the Q8 gain on the detail (256 is 1.0); ``threshold``: 0 .. 255 codes of detail cored away
    (soft: subtracted); ``limit``: 0 .. 255, the largest step in codes; ``radius``: one of ``SHARPEN_RADII``, the binomial
    blur's (3 x 3 or 5 x 5).  Integers only - a bool or a float is refused.  With ``H`` / ``W`` given: 1 .. 2^24, at most
    65535 row tiles, and even with ``nv12``.  Nothing is read from the device and the host never waits."""
    try:
        amount, threshold, limit, radius = sharpen
    except (TypeError, ValueError):
        raise ValueError('a sharpening is (amount, threshold, limit, radius): four integers - the Q8 gain 0 .. 4095, the coring '
                         'threshold 0 .. 255, the limit 0 .. 255 and the radius 1 or 2; got %r' % (sharpen,)) from None
    for name, v, hi in (('amount', amount, SHARPEN_MAX_AMOUNT), ('threshold', threshold, 255), ('limit', limit, 255)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError('sharpen %s %r: an integer (not a bool, not a float) in 0 .. %d' % (name, v, hi))
        if not 0 <= v <= hi:
            raise ValueError('sharpen %s %r: outside 0 .. %d' % (name, v, hi))
    if isinstance(radius, bool) or not isinstance(radius, int):
        raise ValueError('sharpen radius %r: an integer (not a bool, not a float), one of %s' % (radius, SHARPEN_RADII))
    if radius not in SHARPEN_RADII:
        raise ValueError('sharpen radius %r: one of %s' % (radius, SHARPEN_RADII))
    for name, v in (('H', H), ('W', W)):
        if v is None:
            continue
        if _small_int(v, 1, _SHARPEN_MAX) is None:
            raise ValueError('sharpening of images with %s = %r: 1 .. 2^24' % (name, v))
        if nv12 and v % 2:
            raise ValueError('sharpening into NV12 with %s = %d: a frame with an odd size has no 4:2:0 form, H and W must be even'
                             % (name, v))
    if H is not None and (H + SHARPEN_TILE_H - 1) // SHARPEN_TILE_H > 65535:
        raise ValueError('sharpening of images with H = %d: more than 65535 row tiles of %d rows' % (H, SHARPEN_TILE_H))
    return amount, threshold, limit, radius


def bgr8_sharpen(img_u8, sharpen, nv12=None, channels='bgr', out=None):
    """Packed 8-bit images sharpened in ONE launch (``risp_bgr8_sharpen``): (N,H,W,3) or (H,W,3) ``torch.uint8`` on the device ->
    the same shape, ``sharpen = (amount, threshold, limit, radius)`` as ``sharpen_check`` takes it.  An unsharp mask of the 8-bit
    luma ``(77 R + 150 G + 29 B + 128) >> 8`` - ``channels`` 'bgr' or 'rgb' names the order - with a binomial blur of the radius
    (replicate border), the detail cored softly by ``threshold``, multiplied by ``amount`` / 256, bounded by ``limit`` and added
    to B, G and R alike, clamped: an integer function, include/risp.h fixes every bit.  With ``nv12`` (a matrix as
    ``nv12_matrix`` takes it) the same launch stores (N,3H/2,W) or (3H/2,W) YUV 4:2:0 of the sharpened codes instead, byte for
    byte ``bgr8_to_nv12`` of the packed result (H, W even).  No alignment is asked of the images or of ``out``; ``out`` must not
    share memory with the images.  With ``out`` given a call on contiguous images allocates nothing and the host never waits;
    images that are not contiguous are copied first, which allocates."""
    n, h, w, lead = _bgr8_images(img_u8)
    rgb = _channels(channels)
    coef = None if nv12 is None else nv12_matrix(nv12)
    amount, threshold, limit, radius = sharpen_check(sharpen, coef is not None, h, w)
    img_u8 = _bgr8_batch(img_u8, n)
    out = _u8_out(out, lead + ((h, w, 3) if coef is None else (h + h // 2, w)), img_u8.device, 1, img_u8, 'pixels')
    L.call('risp_bgr8_sharpen', _p(img_u8), _p(out), _coef12(coef), rgb, radius, amount, threshold, limit, n, h, w, _stream())
    return out


def serve_nv12(raw_u16, divisor, ops, params, bilateral=None, matrix='bt601_full', out=None, black_level=0, cfa='rggb'):
    """``serve_u8`` with the NV12 store (``risp_serve_nv12``, ONE launch): the same arguments with ``matrix``
    (``nv12_matrix``) in place of ``reverse_channels`` -> (N,3H/2,W) ``torch.uint8``, byte for byte
    ``bgr8_to_nv12(serve_u8(...), matrix)`` without the packed image ever being written.  H even, W % 4 == 0.  With ``out``
    given nothing is allocated and the host does not wait."""
    n, h, w = _u16_frames(raw_u16)
    _check_counts(ops, params)
    black, code = _sensor(black_level, cfa)             # (4:2:0 asks for even axes below: no mirror check)
    coef = nv12_matrix(matrix)
    _check_420(h, w)
    out = _u8_out(out, (n, h + h // 2, w), raw_u16.device, 4)
    count, oparr, blocks, keep = _stage_args(ops, params)
    bil, keep_bil = _bilateral_args(bilateral)
    L.call('risp_serve_nv12', _p(raw_u16), float(divisor), *bil, count, oparr, blocks, _p(out), _coef12(coef), n, h, w,
           black, code, _stream())
    return out


def serve_classical_nv12(raw_u16, divisor, demosaic, ops, params, matrix='bt601_full', out=None, black_level=0, cfa='rggb'):
    """``serve_classical_u8`` with the NV12 store (``risp_serve_classical_nv12``, ONE launch): the same arguments with
    ``matrix`` (``nv12_matrix``) in place of ``reverse_channels`` -> (N,3H/2,W) ``torch.uint8``, byte for byte
    ``bgr8_to_nv12(serve_classical_u8(...), matrix)``.  H even and >= 4, W % 4 == 0.  With ``out`` given nothing is allocated
    and the host does not wait."""
    n, h, w = _u16_frames(raw_u16)
    _check_counts(ops, params)
    kind = _demosaic_code(demosaic)
    black, code = _sensor(black_level, cfa)             # (4:2:0 asks for even axes below: no mirror check)
    coef = nv12_matrix(matrix)
    _check_420(h, w)
    out = _u8_out(out, (n, h + h // 2, w), raw_u16.device, 4)
    count, oparr, blocks, keep = _stage_args(ops, params)
    L.call('risp_serve_classical_nv12', _p(raw_u16), float(divisor), kind, count, oparr, blocks, _p(out), _coef12(coef), n, h, w,
           black, code, _stream())
    return out


# MIPI-packed sensor frames in: the sample width of ``raw_format`` (include/risp.h states the layout); 0: one sample per
# uint16 word
RAW_FORMAT = {'u16': 0, 'raw10': 10, 'raw12': 12}


def raw_format_bits(raw_format):
    """a key of ``RAW_FORMAT`` -> its sample width (0 for 'u16')"""
    bits = RAW_FORMAT.get(raw_format) if isinstance(raw_format, str) else None
    if bits is None:
        raise ValueError('unknown raw_format %r: one of %s' % (raw_format, ', '.join(RAW_FORMAT)))
    return bits


def packed_width(bits, stride, width=None):
    """The pixels per row of packed frames whose rows are ``stride`` bytes: ``width``, or with None all the row holds,
    ``stride * 8 // bits``.  A multiple of 4 (whole groups) that fits the row, else ValueError."""
    if bits not in (10, 12):
        raise ValueError('bits %r: 10 (RAW10) or 12 (RAW12)' % (bits,))
    if width is None:
        width = stride * 8 // bits
        if width < 4 or width % 4:
            raise ValueError('rows of %d bytes hold %d %d-bit samples, not a multiple of 4: pass the width' % (stride, width, bits))
        return width
    if width != int(width) or width < 4 or width % 4:
        raise ValueError('raw width %r: a multiple of 4, at least 4' % (width,))
    if width * bits // 8 > stride:
        raise ValueError('raw width %d needs %d bytes per row of %d-bit samples, the rows have %d' % (width, width * bits // 8, bits, stride))
    return int(width)


def _packed_frames(packed_u8, bits, width, what='raw'):
    """(N,H,stride) contiguous uint8 frames on the device -> (n, h, w, stride)"""
    _need_gpu(packed_u8, what)
    if packed_u8.dtype != torch.uint8 or packed_u8.dim() != 3 or not packed_u8.is_contiguous():
        raise ValueError('expected contiguous (N,H,stride) uint8 packed frames, got %s %s' % (packed_u8.dtype, tuple(packed_u8.shape)))
    n, h, stride = packed_u8.shape
    return n, h, packed_width(bits, stride, width), stride


def _raw_frames(frames, bits, width, what, u16=True):
    """The sensor frames of a pre-pass -> (n, h, w, stride, single): contiguous (N,H,W) uint16 with ``bits`` 16 (``u16`` False:
    the caller takes no such frames), else (N,H,stride) uint8 MIPI-packed RAW10 / RAW12 with ``width`` as in ``packed_width``;
    ``single``: the batch dimension is absent and n is 1."""
    _need_gpu(frames, what)
    single = frames.dim() == 2
    if u16 and bits == 16:
        if frames.dtype != torch.uint16 or frames.dim() not in (2, 3) or not frames.is_contiguous():
            raise ValueError('expected contiguous (N,H,W) or (H,W) uint16 frames, got %s %s' % (frames.dtype, tuple(frames.shape)))
        if width is not None and width != frames.shape[-1]:
            raise ValueError('width %r of uint16 frames %d wide' % (width, frames.shape[-1]))
        n, h, w = (1,) + tuple(frames.shape) if single else tuple(frames.shape)
        return n, h, w, 2 * w, single
    return _packed_frames(frames[None] if single else frames, bits, width, what) + (single,)


def raw_unpack(packed_u8, bits, width=None, out=None):
    """MIPI-packed RAW10 / RAW12 frames to one sample per word in ONE launch (``risp_raw_unpack``): (N,H,stride) or
    (H,stride) ``torch.uint8`` on the device, ``bits`` 10 or 12 -> (N,H,W) or (H,W) ``torch.uint16``.  RAW10 keeps four
    pixels in five bytes, RAW12 two in three (include/risp.h has the layout to the bit); ``width`` defaults to all the rows
    hold, ``stride * 8 // bits``, which must then be a multiple of 4, and the bytes of a row behind ``width * bits / 8`` are
    padding that is never read.  The frames may start at any byte.  With ``out`` (contiguous, 8-byte aligned) given nothing
    is allocated and the host does not wait."""
    n, h, w, stride, single = _raw_frames(packed_u8, bits, width, 'packed', u16=False)
    out = _u16_out(out, (h, w) if single else (n, h, w), packed_u8.device)
    L.call('risp_raw_unpack', _p(packed_u8), _p(out), bits, n, h, w, stride, _stream())
    return out


def _packed_out(matrix, reverse_channels, out, n, h, w, device):
    """the matrix argument and the output of a packed serving call: BGR (N,H,W,3) without a matrix, NV12 (N,3H/2,W) with one"""
    if matrix is None:
        return None, _u8_out(out, (n, h, w, 3), device, 4)
    if reverse_channels:
        raise ValueError('reverse_channels has no meaning with a yuv matrix: the conversion knows the channel order')
    _check_420(h, w)
    return _coef12(nv12_matrix(matrix)), _u8_out(out, (n, h + h // 2, w), device, 4)


def serve_packed(packed_u8, bits, width, divisor, ops, params, bilateral=None, reverse_channels=False, matrix=None, out=None,
                 black_level=0, cfa='rggb'):
    """``serve_u8`` / ``serve_nv12`` on MIPI-packed frames, still ONE launch (``risp_serve_packed``): (N,H,stride)
    ``torch.uint8`` RAW10 / RAW12 (``bits`` 10 / 12, ``width`` pixels per row or None for all the rows hold, as in
    ``raw_unpack``) -> (N,H,W,3) ``torch.uint8``, or with ``matrix`` (``nv12_matrix``) (N,3H/2,W) NV12.  The kernel decodes
    the groups where it loads them; byte for byte ``serve_u8(raw_unpack(packed_u8, bits, width), ...)`` /
    ``serve_nv12(...)`` without the uint16 frames ever being written.  The frames may start at any byte.  H even,
    W % 4 == 0.  With ``out`` given nothing is allocated and the host does not wait."""
    n, h, w, stride = _packed_frames(packed_u8, bits, width)
    _check_counts(ops, params)
    black, code = _sensor(black_level, cfa, h, w)
    coef, out = _packed_out(matrix, reverse_channels, out, n, h, w, packed_u8.device)
    count, oparr, blocks, keep = _stage_args(ops, params)
    bil, keep_bil = _bilateral_args(bilateral)
    L.call('risp_serve_packed', _p(packed_u8), bits, stride, float(divisor), *bil, count, oparr, blocks, _p(out),
           int(bool(reverse_channels)), coef, n, h, w, black, code, _stream())
    return out


def serve_classical_packed(packed_u8, bits, width, divisor, demosaic, ops, params, reverse_channels=False, matrix=None, out=None,
                           black_level=0, cfa='rggb'):
    """``serve_classical_u8`` / ``serve_classical_nv12`` on MIPI-packed frames, still ONE launch
    (``risp_serve_classical_packed``): ``packed_u8``, ``bits``, ``width`` and ``matrix`` as in ``serve_packed``, every other
    argument ``serve_classical_u8``'s; byte for byte that call on ``raw_unpack(packed_u8, bits, width)``.  H even and >= 4,
    W % 4 == 0.  With ``out`` given nothing is allocated and the host does not wait."""
    n, h, w, stride = _packed_frames(packed_u8, bits, width)
    _check_counts(ops, params)
    kind = _demosaic_code(demosaic)
    black, code = _sensor(black_level, cfa, h, w)
    coef, out = _packed_out(matrix, reverse_channels, out, n, h, w, packed_u8.device)
    count, oparr, blocks, keep = _stage_args(ops, params)
    L.call('risp_serve_classical_packed', _p(packed_u8), bits, stride, float(divisor), kind, count, oparr, blocks, _p(out),
           int(bool(reverse_channels)), coef, n, h, w, black, code, _stream())
    return out


def _on_frames_device(t, device, what):
    """``t`` (``what`` names it, with its verb) lives where the frames do; ``device`` None: not asked"""
    if device is not None and t.device != device and t.device != torch.device(device):
        raise ValueError('%s on %s, the frames on %s' % (what, t.device, device))


def _shading_cell(cell):
    """the cell size of a lens shading -> k with cell = 1 << k"""
    if isinstance(cell, bool) or not isinstance(cell, int) or cell not in (4, 8, 16, 32, 64, 128, 256):
        raise ValueError('lens shading cell %r: a power of two from 4 to 256' % (cell,))
    return cell.bit_length() - 1


def shading_check(shading, h, w, device=None):
    """A lens shading ``(gains, cell)`` for H x W frames, checked on the host before anything is launched -> (gains, k, GH, GW)
    with cell = 1 << k.  ``gains``: a contiguous (GH,GW,4) ``torch.uint16`` device tensor, Q12 (4096 is gain 1.0; every value
    is legal, so none is read here and the host never waits), 8-byte aligned, node (i,j) at sensor pixel (i * cell, j * cell)
    and plane 2 * (y & 1) + (x & 1) of the frame as stored; ``cell``: a power of two from 4 to 256;
    GH == (H-1) // cell + 2 and GW == (W-1) // cell + 2 exactly (include/risp.h has the definition)."""
    try:
        gains, cell = shading
    except (TypeError, ValueError):
        raise ValueError('a lens shading is (gains, cell): a (GH,GW,4) uint16 device tensor and the cell size in pixels') from None
    k = _shading_cell(cell)
    if not isinstance(gains, torch.Tensor) or gains.dtype != torch.uint16:
        raise ValueError('lens shading gains must be a uint16 tensor (Q12), got %s' % (getattr(gains, 'dtype', type(gains)),))
    gh, gw = ((int(h) - 1) >> k) + 2, ((int(w) - 1) >> k) + 2
    if tuple(gains.shape) != (gh, gw, 4) or not gains.is_contiguous():
        raise ValueError('lens shading gains of a %d x %d frame with cell %d must be contiguous (%d,%d,4): (H-1) // cell + 2 by '
                         '(W-1) // cell + 2 nodes of four planes; got %s' % (h, w, cell, gh, gw, tuple(gains.shape)))
    _need_gpu(gains, 'lens shading gains')
    _on_frames_device(gains, device, 'lens shading gains live')
    if gains.data_ptr() % 8:
        raise ValueError('lens shading gains must be 8-byte aligned')
    return gains, k, gh, gw


def shading_map(gain, H, W, cell):
    """Host helper: a float gain image -> the (GH,GW,4) ``torch.uint16`` Q12 node grid of a lens shading for H x W frames (on
    the CPU; move it to the device once).  ``gain``: (4,h,w) - a plane per Bayer position 2 * (y & 1) + (x & 1) - or (h,w) for
    all four, any size from 1 x 1, DNG GainMap style: its corner samples sit on the frame's corners (0,0) and (H-1,W-1).  It is
    resampled bilinearly in float64 at the nodes (i * cell, j * cell) - the nodes behind the last pixel take the image's linear
    continuation - and rounded to Q12.  A resampled value outside 0 .. 65535 / 4096 or not finite is refused."""
    import numpy as np
    k = _shading_cell(cell)
    if H != int(H) or W != int(W) or H < 1 or W < 1:
        raise ValueError('frame size %r x %r' % (H, W))
    g = np.asarray(gain.detach().cpu().numpy() if isinstance(gain, torch.Tensor) else gain, dtype=np.float64)
    if g.ndim == 2:
        g = np.broadcast_to(g, (4,) + g.shape)
    if g.ndim != 3 or g.shape[0] != 4 or g.shape[1] < 1 or g.shape[2] < 1:
        raise ValueError('a gain image is (4,h,w) or (h,w), got %s' % (tuple(g.shape),))
    if not np.isfinite(g).all():
        raise ValueError('the gain image has values that are not finite')
    gh, gw = ((int(H) - 1) >> k) + 2, ((int(W) - 1) >> k) + 2

    def axis(nodes, full, size):
        # node positions in image samples, the two samples beside each and the weight of the second
        pos = np.arange(nodes, dtype=np.float64) * cell * ((size - 1) / (full - 1) if full > 1 else 0.0)
        if size == 1:
            return np.zeros(nodes, dtype=np.int64), np.zeros(nodes, dtype=np.int64), np.zeros(nodes)
        lo = np.clip(np.floor(pos).astype(np.int64), 0, size - 2)
        return lo, lo + 1, pos - lo

    y0, y1, ty = axis(gh, int(H), g.shape[1])
    x0, x1, tx = axis(gw, int(W), g.shape[2])
    ty, tx = ty[None, :, None], tx[None, None, :]
    top = g[:, y0][:, :, x0] * (1 - tx) + g[:, y0][:, :, x1] * tx
    bot = g[:, y1][:, :, x0] * (1 - tx) + g[:, y1][:, :, x1] * tx
    q = np.rint((top * (1 - ty) + bot * ty) * 4096.0)
    if not np.isfinite(q).all() or q.min() < 0 or q.max() > 65535:
        raise ValueError('gains outside 0 .. 65535 / 4096 at the nodes (%g .. %g): Q12 in uint16 cannot hold them'
                         % (q.min() / 4096.0, q.max() / 4096.0))
    return torch.from_numpy(np.ascontiguousarray(q.transpose(1, 2, 0).astype(np.uint16)))


def raw_shade(frames, shading, black_level=0, bits=16, width=None, out=None):
    """Lens-shading correction of sensor frames in ONE launch (``risp_raw_shade``): (N,H,W) or (H,W) ``torch.uint16`` frames
    on the device (``bits=16``), or (N,H,stride) / (H,stride) ``torch.uint8`` MIPI-packed RAW10 / RAW12 (``bits`` 10 / 12,
    ``width`` as in ``raw_unpack``) -> (N,H,W) or (H,W) ``torch.uint16`` shaded samples
    min((max(s - black_level, 0) * g + 2048) >> 12, 65535), g the Q12 gain interpolated from ``shading`` = (gains, cell)
    (``shading_check``; include/risp.h has the definition to the bit).  The black level leaves here: what comes out has black
    level 0 and the divisor white_level - black_level.  W % 4 == 0.  With ``out`` (contiguous, 8-byte aligned) given nothing
    is allocated and the host does not wait."""
    n, h, w, stride, single = _raw_frames(frames, bits, width, 'frames')
    if w < 4 or w % 4:                          # (uint16 frames: a packed width is a multiple of 4 already)
        raise ValueError('frames %d wide: W must be a multiple of 4' % w)
    black = _black_level(black_level)
    gains, k, gh, gw = shading_check(shading, h, w, frames.device)
    out = _u16_out(out, (h, w) if single else (n, h, w), frames.device)
    L.call('risp_raw_shade', _p(frames), int(bits), stride, _p(out), _p(gains), k, gh, gw, black, n, h, w, _stream())
    return out


def _small_int(v, lo, hi):
    """v as an int when it is an integer (no bool) in lo .. hi, else None"""
    import numbers
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= int(v) <= hi:
        return None
    return int(v)


def defect_check(dc, h, w, device=None):
    """A defective-pixel correction ``(threshold, slope, defects)`` for H x W frames, checked on the host before anything is
    launched -> (threshold, slope, defects) normalised: ints, threshold -1 for None (the C ABI's 'no dynamic test').
    ``threshold``: an integer 0 .. 65535 in raw codes or None; ``slope``: an integer 0 .. 255, Q8, the part of the threshold
    that grows with the signal; ``defects``: None or the factory list as a contiguous (H, (W+31)//32) ``torch.int32`` device
    tensor, bit x & 31 of word x >> 5 of row y for pixel (y,x) (``defect_map`` builds one; bits at x >= W are ignored).  One
    of threshold and map must be given.  H >= 3, W >= 4, W % 4 == 0.  Nothing on the device is read: the host never waits
    (include/risp.h has the definition to the bit)."""
    try:
        threshold, slope, defects = dc
    except (TypeError, ValueError):
        raise ValueError('a defect correction is (threshold, slope, defects): raw codes or None, a Q8 slope, '
                         'an (H,(W+31)//32) int32 device bitmap or None') from None
    thr = -1 if threshold is None else _small_int(threshold, 0, 65535)
    if thr is None:
        raise ValueError('defect threshold %r: an integer in 0 .. 65535 (raw codes), or None for no dynamic test' % (threshold,))
    slp = _small_int(slope, 0, 255)
    if slp is None:
        raise ValueError('defect slope %r: an integer in 0 .. 255 (Q8)' % (slope,))
    if int(h) < 3 or int(w) < 4 or int(w) % 4:
        raise ValueError('defect correction on %d x %d frames: H >= 3, W >= 4 and a multiple of 4' % (h, w))
    if defects is None:
        if thr < 0:
            raise ValueError('a defect correction with neither a threshold nor a defect map corrects nothing')
        return thr, slp, None
    if not isinstance(defects, torch.Tensor) or defects.dtype != torch.int32:
        raise ValueError('the defect map must be an int32 tensor (a bit per pixel), got %s' % (getattr(defects, 'dtype', type(defects)),))
    words = (int(w) + 31) // 32
    if tuple(defects.shape) != (int(h), words) or not defects.is_contiguous():
        raise ValueError('the defect map of a %d x %d frame must be contiguous (%d,%d): a word per 32 pixels of a row; got %s'
                         % (h, w, h, words, tuple(defects.shape)))
    _need_gpu(defects, 'defect map')
    _on_frames_device(defects, device, 'the defect map lives')
    return thr, slp, defects


def defect_map(coords, H, W):
    """Host helper: defective pixels as an iterable or (K,2) array of integer (y, x) -> the (H, (W+31)//32) ``torch.int32``
    bitmap of ``defect_check`` (on the CPU; move it to the device once): bit x & 31 of word x >> 5 of row y, bit 31 being the
    sign bit of its word.  A coordinate outside the frame or not an integer is refused; no coordinates give an all-zero map;
    one given twice is set once."""
    import numpy as np
    if H != int(H) or W != int(W) or H < 1 or W < 1:
        raise ValueError('frame size %r x %r' % (H, W))
    H, W = int(H), int(W)
    if isinstance(coords, torch.Tensor):
        coords = coords.detach().cpu().numpy()
    c = coords if isinstance(coords, np.ndarray) else np.asarray(list(coords))
    words = np.zeros((H, (W + 31) // 32), dtype=np.uint32)
    if c.size:
        if c.ndim != 2 or c.shape[1] != 2:
            raise ValueError('defect coordinates are (K,2) pairs of (y, x), got %s' % (tuple(c.shape),))
        if c.dtype == np.bool_ or not np.issubdtype(c.dtype, np.integer):
            raise ValueError('defect coordinates must be integers, got %s' % (c.dtype,))
        y, x = c[:, 0].astype(np.int64), c[:, 1].astype(np.int64)
        if y.min() < 0 or y.max() >= H or x.min() < 0 or x.max() >= W:
            raise ValueError('defect coordinates outside the %d x %d frame' % (H, W))
        np.bitwise_or.at(words, (y, x >> 5), (np.uint32(1) << (x & 31).astype(np.uint32)))
    return torch.from_numpy(words.view(np.int32))


def raw_defect(frames, defect, bits=16, width=None, shading=None, black_level=0, out=None):
    """Defective-pixel correction of sensor frames in ONE launch (``risp_raw_defect``): (N,H,W) or (H,W) ``torch.uint16``
    frames on the device (``bits=16``), or (N,H,stride) / (H,stride) ``torch.uint8`` MIPI-packed RAW10 / RAW12 (``bits``
    10 / 12, ``width`` as in ``raw_unpack``) -> (N,H,W) or (H,W) ``torch.uint16``.  ``defect`` = (threshold, slope, defects)
    (``defect_check``): a pixel above the largest of its eight same-colour neighbours at distance 2 by more than
    threshold + (slope * that neighbour >> 8), below the smallest by more than the same of the smallest, or listed in the
    bitmap becomes the rounded mean of the pair - across, down, the two diagonals - that differs least; borders reflect;
    neighbours are the input's (include/risp.h has the definition to the bit).  Without ``shading`` the corrected raw codes
    come out, black level kept, and ``black_level`` must be 0.  With ``shading`` = (gains, cell) the same launch shades each
    corrected sample: word for word ``raw_shade(raw_defect(frames, defect, bits, width), shading, black_level)``.  H >= 3,
    W % 4 == 0.  ``out`` (contiguous, 8-byte aligned) must not share memory with the frames - the launch reads rows other
    threads write; with it nothing is allocated and the host does not wait."""
    n, h, w, stride, single = _raw_frames(frames, bits, width, 'frames')
    thr, slp, defects = defect_check(defect, h, w, frames.device)
    black = _black_level(black_level)
    if shading is None:
        if black:
            raise ValueError('black_level %r without a shading: the corrected codes keep their black level' % (black_level,))
        gains, k, gh, gw = None, 0, 0, 0
    else:
        gains, k, gh, gw = shading_check(shading, h, w, frames.device)
    out = _u16_out(out, (h, w) if single else (n, h, w), frames.device, ((frames, 'the frames'),), 'correction')
    L.call('risp_raw_defect', _p(frames), int(bits), stride, _p(out), thr, slp, _p(defects), _p(gains), k, gh, gw, black,
           n, h, w, _stream())
    return out


class TemporalState:
    """The state of the temporal noise reduction for (N,H,W) frames: ``.frames``, (N,H,W) ``torch.uint16``, contiguous and 8-byte
    aligned - the previous filtered frames, which every call that takes the state reads and then overwrites with what it returns -
    and ``.primed``, a host bool that starts False: the first call copies its frames into the state instead of filtering.
    ``.reset()`` clears the flag (a scene cut, a new stream).  Built once by the caller (``temporal_state``); one state belongs to
    one sequence (include/risp.h has the definition to the bit)."""

    def __init__(self, n, h, w, device=None):
        if _small_int(n, 1, 1 << 30) is None:
            raise ValueError('a temporal state of %r frames: N >= 1' % (n,))
        if _small_int(h, 3, 1 << 30) is None or _small_int(w, 4, 1 << 30) is None or w % 4:
            raise ValueError('a temporal state of %r x %r frames: H >= 3, W >= 4 and a multiple of 4' % (h, w))
        self.n, self.h, self.w = int(n), int(h), int(w)
        self.frames = torch.zeros((self.n, self.h, self.w), dtype=torch.uint16, device='cuda' if device is None else device)
        self.primed = False

    def reset(self):
        self.primed = False

    def __repr__(self):
        return 'TemporalState(%d, %d, %d, primed=%s)' % (self.n, self.h, self.w, self.primed)


def temporal_state(n, h, w, device=None):
    """A ``TemporalState`` for (N,H,W) frames on ``device`` (None: the current HIP device), N = 1 for an (H,W) frame: built once,
    it owns ``.frames``, which ``raw_temporal`` and ``serve(temporal_denoise=)`` read and advance, and ``.primed``."""
    return TemporalState(n, h, w, device)


def temporal_check(td, n, h, w, device=None):
    """A temporal noise reduction ``(state, strength, threshold, slope, ramp)`` for N frames of H x W on ``device``, checked on
    the host before anything is launched -> (state, strength, threshold, slope, ramp) with the numbers as ints.  ``state``: a
    ``TemporalState`` whose ``.frames`` are contiguous (N,H,W) ``torch.uint16`` on the device, 8-byte aligned; ``strength``: an
    integer 0 .. 256, Q8, the share of the new frame where nothing moves (256 passes the frames, 0 freezes); ``threshold``: an
    integer 0 .. 65535 in codes of mean difference over the 5 x 5 window; ``slope``: an integer 0 .. 255, Q8, the part of the
    threshold that grows with the signal; ``ramp``: an integer 0 .. 65535, Q8 per code of summed excess.  H >= 3, W >= 4,
    W % 4 == 0.  Nothing on the device is read: the host never waits (include/risp.h has the definition to the bit)."""
    try:
        state, strength, threshold, slope, ramp = td
    except (TypeError, ValueError):
        raise ValueError('a temporal noise reduction is (state, strength, threshold, slope, ramp): a TemporalState, a Q8 share '
                         '0 .. 256, codes 0 .. 65535, a Q8 slope 0 .. 255, a Q8 ramp 0 .. 65535') from None
    if not isinstance(state, TemporalState):
        raise ValueError('the temporal state must be a TemporalState (functional.temporal_state builds one), got %s'
                         % (type(state).__name__,))
    stg = _small_int(strength, 0, 256)
    if stg is None:
        raise ValueError('temporal strength %r: an integer in 0 .. 256 (Q8)' % (strength,))
    thr = _small_int(threshold, 0, 65535)
    if thr is None:
        raise ValueError('temporal threshold %r: an integer in 0 .. 65535 (codes of mean difference)' % (threshold,))
    slp = _small_int(slope, 0, 255)
    if slp is None:
        raise ValueError('temporal slope %r: an integer in 0 .. 255 (Q8)' % (slope,))
    rmp = _small_int(ramp, 0, 65535)
    if rmp is None:
        raise ValueError('temporal ramp %r: an integer in 0 .. 65535 (Q8 per code)' % (ramp,))
    if int(h) < 3 or int(w) < 4 or int(w) % 4:
        raise ValueError('temporal noise reduction on %d x %d frames: H >= 3, W >= 4 and a multiple of 4' % (h, w))
    t = state.frames
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.uint16 or tuple(t.shape) != (int(n), int(h), int(w))
            or not t.is_contiguous()):
        raise ValueError('the temporal state of %d frames of %d x %d must hold contiguous (%d,%d,%d) uint16 frames, got %s %s'
                         % (n, h, w, n, h, w, getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
    _need_gpu(t, 'temporal state')
    _on_frames_device(t, device, 'the temporal state lives')
    if t.data_ptr() % 8:
        raise ValueError('the temporal state must be 8-byte aligned')
    return state, stg, thr, slp, rmp


def _temporal_prime(state, capturing):
    """whether the call in hand primes ``state``; an unprimed state while the stream is capturing is refused"""
    if state.primed:
        return 0
    if capturing:
        raise RuntimeError('the temporal state is not primed and the stream is capturing: the graph would replay the priming '
                           'form forever.  Prime with one eager call, then capture')
    return 1


def raw_temporal(frames, td, black_level=0, out=None):
    """Temporal noise reduction of sensor frames in ONE launch and one copy (``risp_raw_temporal``): (N,H,W) or (H,W)
    ``torch.uint16`` frames on the device and ``td`` = (state, strength, threshold, slope, ramp) (``temporal_check``; N = 1 for
    an (H,W) frame) -> (N,H,W) or (H,W) ``torch.uint16``, the filtered frames, and ``state.frames`` advanced to them by a
    device-to-device copy on the same stream.  Per pixel the frame is blended over the state with a Q8 share k that starts at
    ``strength`` and climbs to 256 as the summed difference of the 5 x 5 window passes
    25 * threshold + (slope * max(sum of the state - 25 * black_level, 0) >> 8), by ``ramp`` / 256 per code; borders reflect;
    neighbours are the previous state's and the current frame's (include/risp.h has the definition to the bit).
    ``black_level`` is the pedestal of the samples: 0 behind a shading.  A state whose ``.primed`` is False is primed: the
    frames come back as they are and become the state; that is refused while the stream is capturing - prime with one eager
    call, then capture, and every replay advances the state.  Packed frames are not taken: they come through ``raw_unpack`` or a
    pre-pass first.  H >= 3, W % 4 == 0.  ``out`` (contiguous, 8-byte aligned) must share memory with neither the frames nor
    the state - the launch reads rows other threads write; with it nothing is allocated and the host does not wait."""
    n, h, w, _, single = _raw_frames(frames, 16, None, 'frames')
    state, stg, thr, slp, rmp = temporal_check(td, n, h, w, frames.device)
    black = _black_level(black_level)
    out = _u16_out(out, (h, w) if single else (n, h, w), frames.device,
                   ((frames, 'the frames'), (state.frames, 'the temporal state')), 'filter')
    prime = _temporal_prime(state, torch.cuda.is_current_stream_capturing())
    L.call('risp_raw_temporal', _p(frames), _p(state.frames), _p(out), prime, stg, thr, slp, rmp, black, n, h, w, _stream())
    state.primed = True
    return out


def _stats_spec(zone, bins, hist_shift, lo, hi):
    """the specification of the 3A statistics, checked on the host -> (zone_h, zone_w, bins, hist_shift, lo, hi) as ints"""
    try:
        zone_h, zone_w = zone
    except (TypeError, ValueError):
        raise ValueError('a statistics zone is (zone_h, zone_w) in pixels, got %r' % (zone,)) from None
    zh = _small_int(zone_h, 2, 1 << 30)
    if zh is None or zh % 2:
        raise ValueError('zone_h %r: an even integer, at least 2 (a Bayer row pair lies in one zone)' % (zone_h,))
    zw = _small_int(zone_w, 4, 1 << 30)
    if zw is None or zw % 4:
        raise ValueError('zone_w %r: a multiple of 4, at least 4' % (zone_w,))
    nb = _small_int(bins, 1, 1024)
    if nb is None:
        raise ValueError('bins %r: an integer in 1 .. 1024' % (bins,))
    shift = _small_int(hist_shift, 0, 16)
    if shift is None:
        raise ValueError('hist_shift %r: an integer in 0 .. 16' % (hist_shift,))
    low, high = _small_int(lo, 0, 65535), _small_int(hi, 0, 65535)
    if low is None or high is None or low > high:
        raise ValueError('lo %r, hi %r: integers with 0 <= lo <= hi <= 65535' % (lo, hi))
    return zh, zw, nb, shift, low, high


def _stats_shape(n, h, w, zh, zw):
    """the frames a statistics block is built for -> (ZH, ZW); N >= 1, H even, W >= 4 and a multiple of 4, at most 65536 zones"""
    if _small_int(n, 1, 1 << 30) is None:
        raise ValueError('statistics of %r frames: N >= 1' % (n,))
    if _small_int(h, 2, 1 << 30) is None or h % 2:
        raise ValueError('statistics of frames %r high: H must be even' % (h,))
    if _small_int(w, 4, 1 << 30) is None or w % 4:
        raise ValueError('statistics of frames %r wide: W must be a multiple of 4, at least 4' % (w,))
    gh, gw = -(-int(h) // zh), -(-int(w) // zw)
    if gh * gw > 65536:
        raise ValueError('%d x %d zones of %d x %d pixels on a %d x %d frame: more than 65536' % (gh, gw, zh, zw, h, w))
    return gh, gw


class RawStatistics:
    """The 3A statistics of (N,H,W) sensor frames and the buffers that take them: ``zone`` = (zone_h, zone_w) pixels per zone
    (even, a multiple of 4), ``bins`` histogram bins of ``1 << hist_shift`` codes (the last one takes everything above),
    ``lo`` .. ``hi`` the samples that enter ``sum`` and ``count``.  ``.zones``: (N,ZH,ZW,4,3) ``torch.int64`` holding
    [sum, count, sharp] per zone and plane 2 * (y & 1) + (x & 1) of the frame as stored (``stats_planes`` names the planes of a
    ``cfa``); ``.hist``: (N,4,bins) ``torch.int32``.  Both are views of one allocation, the histogram right behind the zones, so
    that ``risp_raw_stats`` zeroes them with one memset.  Built once by the caller (``raw_statistics``) and overwritten by
    every call that takes it (include/risp.h has the definition to the bit)."""

    def __init__(self, n, h, w, zone=(16, 16), bins=256, hist_shift=0, lo=0, hi=65535, device=None):
        self.zone_h, self.zone_w, self.bins, self.hist_shift, self.lo, self.hi = _stats_spec(zone, bins, hist_shift, lo, hi)
        self.grid = _stats_shape(n, h, w, self.zone_h, self.zone_w)
        self.n, self.h, self.w = int(n), int(h), int(w)
        self._checked = None                    # what stats_check validated last
        words, counts = self.n * self.grid[0] * self.grid[1] * 12, self.n * 4 * self.bins
        buf = torch.zeros(words + (counts + 1) // 2, dtype=torch.int64, device='cuda' if device is None else device)
        self.zones = buf[:words].view(self.n, self.grid[0], self.grid[1], 4, 3)
        self.hist = buf[words:].view(torch.int32)[:counts].view(self.n, 4, self.bins)

    def __repr__(self):
        return 'RawStatistics(%d, %d, %d, zone=(%d, %d), bins=%d, hist_shift=%d, lo=%d, hi=%d)' % (
            self.n, self.h, self.w, self.zone_h, self.zone_w, self.bins, self.hist_shift, self.lo, self.hi)


def raw_statistics(n, h, w, zone=(16, 16), bins=256, hist_shift=0, lo=0, hi=65535, device=None):
    """A ``RawStatistics`` for (N,H,W) frames on ``device`` (None: the current HIP device): built once, it owns ``.zones`` and
    ``.hist``, which ``raw_stats`` and ``serve(statistics=)`` overwrite.  Everything the definition refuses is refused here."""
    return RawStatistics(n, h, w, zone, bins, hist_shift, lo, hi, device)


def stats_check(st, n, h, w, device=None):
    """A ``RawStatistics`` for N frames of H x W on ``device``, checked on the host before anything is launched ->
    (zone_h, zone_w, bins, hist_shift, lo, hi).  The specification is checked again (its fields can be assigned), then the
    outputs: ``.zones`` contiguous (N,ZH,ZW,4,3) int64 and ``.hist`` contiguous (N,4,bins) int32, both on ``device``.  Nothing
    on the device is read: the host never waits."""
    if not isinstance(st, RawStatistics):
        raise ValueError('statistics must be a RawStatistics (functional.raw_statistics builds one), got %s' % (type(st).__name__,))
    # (a served call comes here three times and is bound by its host side: the integers are validated once per value)
    key = (st.zone_h, st.zone_w, st.bins, st.hist_shift, st.lo, st.hi, n, h, w)
    if st._checked is None or st._checked[0] != key:
        spec = _stats_spec((st.zone_h, st.zone_w), st.bins, st.hist_shift, st.lo, st.hi)
        st._checked = (key, spec, _stats_shape(n, h, w, spec[0], spec[1]))
    _, spec, (gh, gw) = st._checked
    bins = spec[2]
    for name, t, shape, dtype in (('zones', st.zones, (int(n), gh, gw, 4, 3), torch.int64),
                                  ('hist', st.hist, (int(n), 4, bins), torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError('statistics.%s for %d frames of %d x %d must be a contiguous %s %s tensor, got %s %s'
                             % (name, n, h, w, shape, str(dtype).replace('torch.', ''), getattr(t, 'dtype', type(t)),
                                tuple(getattr(t, 'shape', ()))))
        _on_frames_device(t, device, 'statistics.zones lives' if name == 'zones' else 'statistics.hist lives')
    return spec


def stats_planes(cfa):
    """The names of the four planes of ``.zones`` and ``.hist`` for a sensor of phase ``cfa``, in plane order
    2 * (y & 1) + (x & 1) of the frame as stored: 'r', 'gr' (green of the red rows), 'gb', 'b'."""
    code = cfa_code(cfa)
    return tuple(('r', 'gr', 'gb', 'b')[c ^ code] for c in range(4))


def raw_stats(frames, st, black_level=0, bits=16, width=None):
    """The 3A statistics of sensor frames in ONE launch behind the zeroing (``risp_raw_stats``): (N,H,W) or (H,W)
    ``torch.uint16`` frames on the device (``bits=16``), or (N,H,stride) / (H,stride) ``torch.uint8`` MIPI-packed RAW10 / RAW12
    (``bits`` 10 / 12, ``width`` as in ``raw_unpack``).  Fills ``st`` (a ``RawStatistics`` built for these N, H, W; N is 1 for a
    single frame) from the samples max(s - black_level, 0) and returns it: per zone and plane the sum and the count of the
    samples in lo .. hi and the focus measure sum |2 s(y,x) - s(y,x-2) - s(y,x+2)|, per image and plane the histogram
    (include/risp.h has the definition to the bit).  Integers throughout: the result is exact and has no summation order.
    H even, W % 4 == 0.  Nothing is allocated and the host does not wait."""
    n, h, w, stride, _ = _raw_frames(frames, bits, width, 'frames')
    black = _black_level(black_level)
    zh, zw, nb, shift, lo, hi = stats_check(st, n, h, w, frames.device)
    L.call('risp_raw_stats', _p(frames), int(bits), stride, black, _p(st.zones), _p(st.hist), zh, zw, nb, shift, lo, hi,
           n, h, w, _stream())
    return st


CONTROL_FIELDS = ('fill', 'y_lo', 'y_hi', 'rg_lo', 'rg_hi', 'bg_lo', 'bg_hi', 'min_share', 'wb_dead', 'wb_speed', 'wb_min', 'wb_max',
                  'pct', 'target', 'ceil', 'ae_dead', 'ae_speed', 'e_min', 'e_max')
_CONTROL_RANGES = dict(fill=(0, 256), y_lo=(0, 65535), y_hi=(0, 65535), rg_lo=(0, 4095), rg_hi=(0, 4095), bg_lo=(0, 4095),
                       bg_hi=(0, 4095), min_share=(0, 256), wb_dead=(0, 4095), wb_speed=(0, 256), wb_min=(256, 65535),
                       wb_max=(256, 65535), pct=(1, 65536), target=(1, 65535), ceil=(1, 65535), ae_dead=(0, 4095),
                       ae_speed=(0, 256), e_min=(256, 65535), e_max=(256, 65535))
_CONTROL_PAIRS = (('y_lo', 'y_hi'), ('rg_lo', 'rg_hi'), ('bg_lo', 'bg_hi'), ('wb_min', 'wb_max'), ('e_min', 'e_max'))
# settings for 10-bit samples with the black level taken off (tests/control_reference.py has the scene they were tried on): zones at
# least 3/4 inside lo .. hi, green mean 16 .. 900, red and blue within 1/4 .. 4 of green, 1/8 of the zones grey enough, a white
# balance that moves 5/8 of the way once it is more than 1 % off, the mean green level drawn to 170 unless the 99 % point would pass
# 900, 5/8 of the way once it is more than 3 % off; gains from 1/4 up
_CONTROL_DEFAULTS = dict(fill=192, y_lo=16, y_hi=900, rg_lo=64, rg_hi=1024, bg_lo=64, bg_hi=1024, min_share=32, wb_dead=40,
                         wb_speed=160, wb_min=1024, wb_max=65535, pct=64880, target=170, ceil=900, ae_dead=120, ae_speed=160,
                         e_min=1024, e_max=65535)


def control_spec(**fields):
    """The control specification of the device-side auto white balance / auto exposure, checked on the host -> the tuple of its
    nineteen integers in the order of ``CONTROL_FIELDS`` (include/risp.h has their meaning and ranges).  A field not given
    takes its default.  Bools, non-integers, values outside the ranges and a lower bound above its upper bound are refused."""
    unknown = sorted(set(fields) - set(CONTROL_FIELDS))
    if unknown:
        raise ValueError('unknown control field %s: one of %s' % (', '.join(unknown), ', '.join(CONTROL_FIELDS)))
    spec = {}
    for name in CONTROL_FIELDS:
        value = fields.get(name, _CONTROL_DEFAULTS[name])
        lo, hi = _CONTROL_RANGES[name]
        spec[name] = _small_int(value, lo, hi)
        if spec[name] is None:
            raise ValueError('%s %r: an integer in %d .. %d' % (name, value, lo, hi))
    for low, high in _CONTROL_PAIRS:
        if spec[low] > spec[high]:
            raise ValueError('%s %d above %s %d' % (low, spec[low], high, spec[high]))
    return tuple(spec[name] for name in CONTROL_FIELDS)


class GainControl:
    """The device-side 3A controller of a ``RawStatistics``: auto white balance and auto exposure whose output is a lens-shading
    map.  ``.state``: sixteen ``torch.int32`` on the device - [e, wr, wb, updates, M, P, K, flags, g[0..3], 0 x 4], Q12 gains
    (include/risp.h has the definition to the bit); ``.gains``: the (GH,GW,4) ``torch.uint16`` map of cell ``cell`` for the
    statistics' H x W frames, ``base`` (an existing lens shading of the same cell; kept, never written) times the plane gains, or
    the plane gains alone; ``.shading`` = (``.gains``, ``cell``) is what ``serve(lens_shading=, statistics=st)`` takes.  The
    statistics are taken behind the shading, so ``update(st)`` after a served frame closes the loop for the next one.  ``cfa``
    says which plane holds which colour (``stats_planes``); ``fields`` are those of ``control_spec``.  The N images of a call
    are pooled: one state, one map."""

    def __init__(self, st, cell=256, base=None, cfa='rggb', **fields):
        if not isinstance(st, RawStatistics):
            raise ValueError('a gain control is built for a RawStatistics (functional.raw_statistics builds one), got %s'
                             % (type(st).__name__,))
        zh, zw, bins, shift, _, _ = stats_check(st, st.n, st.h, st.w)
        self.spec = control_spec(**fields)
        self.cfa = cfa_code(cfa)
        _shading_cell(cell)
        self.n, self.h, self.w, self.grid, self.cell = st.n, st.h, st.w, st.grid, cell
        self.geometry = (zh, zw, bins, shift)
        if self.n * self.grid[0] * self.grid[1] > 1 << 24:
            raise ValueError('%d x %d x %d zones: more than 2^24' % ((self.n,) + tuple(self.grid)))
        if self.n * self.h * self.w // 2 >= 1 << 40:
            raise ValueError('%d frames of %d x %d: N * H * W / 2 reaches 2^40' % (self.n, self.h, self.w))
        _need_gpu(st.zones, 'statistics.zones')
        device = st.zones.device
        k = cell.bit_length() - 1
        self.base = None
        if base is not None:
            self.base = shading_check((base, cell), self.h, self.w, device)[0]
        self.state = torch.zeros(16, dtype=torch.int32, device=device)
        self._scratch = torch.zeros(5 + bins, dtype=torch.int64, device=device)     # [ticket, AR, AG, AB, K, Hg[bins]]
        self.gains = torch.empty((((self.h - 1) >> k) + 2, ((self.w - 1) >> k) + 2, 4), dtype=torch.uint16, device=device)
        shading_check(self.shading, self.h, self.w, device)
        self._spec_c = (C.c_int * len(self.spec))(*self.spec)
        self.reset()

    @property
    def shading(self):
        return self.gains, self.cell

    def reset(self, exposure=4096, wb=(4096, 4096)):
        """Start over from these Q12 gains (256 .. 65535 each): the scratch is zeroed, the state written and the map made, so the
        next frame is served with them.  -> self"""
        try:
            wr, wb_ = wb
        except (TypeError, ValueError):
            raise ValueError('wb is (red, blue), two Q12 gains, got %r' % (wb,)) from None
        words = []
        for name, value in (('exposure', exposure), ('wb red', wr), ('wb blue', wb_)):
            words.append(_small_int(value, 256, 65535))
            if words[-1] is None:
                raise ValueError('%s %r: a Q12 gain, an integer in 256 .. 65535' % (name, value))
        e, wr, wb_ = words
        gains = [wr if p ^ self.cfa == 0 else wb_ if p ^ self.cfa == 3 else 4096 for p in range(4)]
        words += [0] * 5 + [min((e * g + 2048) >> 12, 65535) for g in gains] + [0] * 4
        self._scratch.zero_()
        self.state.copy_(torch.tensor(words, dtype=torch.int32))
        L.call('risp_gain_map', _p(self.base), _p(self.state), _p(self.gains), self.gains.shape[0], self.gains.shape[1], _stream())
        return self

    def update(self, st):
        return control_update(self, st)

    def __repr__(self):
        return 'GainControl(%d, %d, %d, cell=%d, cfa=%d%s)' % (self.n, self.h, self.w, self.cell, self.cfa,
                                                              ', base' if self.base is not None else '')


def gain_control(st, cell=256, base=None, cfa='rggb', **fields):
    """A ``GainControl`` for the ``RawStatistics`` ``st``: built once, it owns ``.state``, ``.gains`` and its scratch, and its
    map holds the initial gains (1.0) from the start."""
    return GainControl(st, cell, base, cfa, **fields)


def control_update(ctl, st):
    """One step of the device-side 3A loop in TWO launches on the current stream (``risp_control_solve``, ``risp_gain_map``):
    the statistics ``st`` - those of a frame served with ``lens_shading=ctl.shading, statistics=st`` - move ``ctl.state`` and
    rewrite ``ctl.gains`` for the next frame.  ``st`` is checked again (``stats_check``) and must have the frames, zones and
    bins ``ctl`` was built for.  Nothing is allocated and nothing on the device is read by the host, so the call can be
    captured in a graph behind the serving call.  -> ctl"""
    if not isinstance(ctl, GainControl):
        raise ValueError('control_update takes a GainControl (functional.gain_control builds one), got %s' % (type(ctl).__name__,))
    zh, zw, bins, shift, _, _ = stats_check(st, ctl.n, ctl.h, ctl.w, ctl.state.device)
    if (zh, zw, bins, shift) != ctl.geometry:
        raise ValueError('statistics with zones of %d x %d, %d bins and hist_shift %d: the gain control was built for zones of '
                         '%d x %d, %d bins and hist_shift %d' % ((zh, zw, bins, shift) + ctl.geometry))
    L.call('risp_control_solve', _p(st.zones), _p(st.hist), _p(ctl.state), _p(ctl._scratch), ctl._spec_c, ctl.n, ctl.grid[0],
           ctl.grid[1], ctl.h, ctl.w, zh, zw, bins, shift, ctl.cfa, _stream())
    L.call('risp_gain_map', _p(ctl.base), _p(ctl.state), _p(ctl.gains), ctl.gains.shape[0], ctl.gains.shape[1], _stream())
    return ctl


def serve_classical_shaded(raw_u16, shading, divisor, demosaic, ops, params, reverse_channels=False, matrix=None, out=None,
                           black_level=0, cfa='rggb'):
    """``serve_classical_u8`` / ``serve_classical_nv12`` with the lens-shading correction inside the load, still ONE launch
    (``risp_serve_classical_shaded``): (N,H,W) ``torch.uint16`` frames and ``shading`` = (gains, cell) as in ``raw_shade`` ->
    (N,H,W,3) ``torch.uint8``, or with ``matrix`` (``nv12_matrix``) (N,3H/2,W) NV12.  ``divisor`` is
    white_level - black_level.  Byte for byte ``serve_classical_u8(raw_shade(raw_u16, shading, black_level), divisor, ...,
    black_level=0, cfa=cfa)`` without the shaded frames ever being written.  H even and >= 4, W % 4 == 0.  With ``out`` given
    nothing is allocated and the host does not wait."""
    n, h, w = _u16_frames(raw_u16)
    _check_counts(ops, params)
    kind = _demosaic_code(demosaic)
    black, code = _sensor(black_level, cfa, h, w)
    gains, k, gh, gw = shading_check(shading, h, w, raw_u16.device)
    coef, out = _packed_out(matrix, reverse_channels, out, n, h, w, raw_u16.device)
    count, oparr, blocks, keep = _stage_args(ops, params)
    L.call('risp_serve_classical_shaded', _p(raw_u16), float(divisor), kind, count, oparr, blocks, _p(out),
           int(bool(reverse_channels)), coef, _p(gains), k, gh, gw, n, h, w, black, code, _stream())
    return out


DENOISE = {'bilateral': 0, 'median': 1, 'fastnlm': 2}          # RISP_DENOISE_*


def serve_denoise_u8(raw_u16, divisor, kind, pre_ops, pre_params, denoise, denoise_args, post_ops, post_params,
                     reverse_channels=False, out=None, black_level=0, cfa='rggb'):
    """A classical pipeline with ONE classical denoiser as an ISP in ONE launch (``risp_serve_denoise_u8``): (N,H,W)
    ``torch.uint16`` frames on the device -> (N,H,W,3) ``torch.uint8``.  ``serve_classical_u8``'s input expression and
    demosaic ``kind``, the stages ``pre_ops`` / ``pre_params``, the denoiser, the stages ``post_ops`` / ``post_params`` (both
    lists hold what ``serve_classical_u8`` accepts, at most 8 stages together), then ``quantise_u8``'s conversion.
    ``denoise`` is a key of ``DENOISE`` and ``denoise_args`` what ``origin_denoise`` takes for it, at the sizes the reference's
    parameter rules give below a saturated parameter:

        'bilateral'  (3, sigma_color, sigma_space)    'median'  (3,)    'fastnlm'  (3, 3, decay)

    with (N,) float32 device tensors for the per-image values; any other window, size, block or search is refused (those
    pipelines compose).  Only the result is stored; its bytes are those of ``raw_crops`` -> ``origin_demosaic`` /
    ``chain_forward`` / ``origin_tonemap`` -> ``origin_denoise`` -> stages -> ``quantise_u8`` with scales (255, 255).  H even
    and >= 4, W % 4 == 0; ``black_level`` and ``cfa`` as in ``serve_u8``.  With ``out`` given nothing is allocated and the host
    does not wait."""
    args, code, keep = _denoise_frame_args(raw_u16, kind, pre_ops, pre_params, denoise, denoise_args, post_ops, post_params,
                                           black_level, cfa)
    n, h, w = raw_u16.shape
    out = _u8_out(out, (n, h, w, 3), raw_u16.device, 4)
    L.call('risp_serve_denoise_u8', _p(raw_u16), float(divisor), *args, _p(out), int(bool(reverse_channels)), n, h, w,
           int(black_level), code, _stream())
    return out


MEDIAN_SIZES = (5, 7, 9, 11, 13, 15)          # what risp_serve_median_u8 serves: OriginNoiseMedian's sizes for 1/7 <= p < 1


def serve_median_u8(raw_u16, divisor, kind, pre_ops, pre_params, size, post_ops, post_params, reverse_channels=False, out=None,
                    black_level=0, cfa='rggb'):
    """``serve_denoise_u8`` with a median of ``size`` 5, 7, 9, 11, 13 or 15, still ONE launch (``risp_serve_median_u8``):
    (N,H,W) ``torch.uint16`` frames on the device -> (N,H,W,3) ``torch.uint8``.  ``serve_classical_u8``'s input expression and
    demosaic ``kind``, the stages ``pre_ops`` / ``pre_params``, the ``size`` x ``size`` median of the 8-bit codes, the stages
    ``post_ops`` / ``post_params`` (both lists hold what ``serve_classical_u8`` accepts, at most 8 stages together), then
    ``quantise_u8``'s conversion.  Only the result is stored; its bytes are those of ``raw_crops`` -> ``origin_demosaic`` /
    ``chain_forward`` / ``origin_tonemap`` -> ``origin_denoise(x, 'median', {'size': size}, (255, 255))`` -> stages ->
    ``quantise_u8``.  Size 3 is ``serve_denoise_u8``'s and 17 (a saturated parameter) is not served: both are refused.  H even,
    >= 4 and > size // 2, W % 4 == 0 and > size // 2; ``black_level`` and ``cfa`` as in ``serve_u8``.  With ``out`` given nothing
    is allocated and the host does not wait."""
    n, h, w = _u16_frames(raw_u16)
    _check_counts(pre_ops, pre_params, post_ops, post_params)
    code_d = _demosaic_code(kind)
    if size != int(size) or int(size) not in MEDIAN_SIZES:
        raise ValueError('median size %r: one of %s (3 is serve_denoise_u8\'s)' % (size, ', '.join(str(k) for k in MEDIAN_SIZES)))
    black, code = _sensor(black_level, cfa, h, w)
    out = _u8_out(out, (n, h, w, 3), raw_u16.device, 4)
    pre = _stage_args(pre_ops, pre_params)
    post = _stage_args(post_ops, post_params)
    L.call('risp_serve_median_u8', _p(raw_u16), float(divisor), code_d, *pre[:3], int(size), *post[:3], _p(out),
           int(bool(reverse_channels)), n, h, w, black, code, _stream())
    return out


OP_GAIN3_Q8, OP_TONE_REINHARD = 9, 10      # stages of serve_scene_u8 / serve_scene_stats only: they take serve_scene_finish's constants
SCENE_MEAN3, SCENE_MAX3, SCENE_LOGLUM = 0, 1, 2       # RISP_SCENE_*
# (device, stream, tag, shape) -> float32 scratch of the scene route (partials, constants), kept until release_scene_scratch()
_scene_scratch = {}


def release_scene_scratch():
    """Drop the cached partials and constants of the scene route and the cached counts and blocks of the conditional route
    (every device and stream)."""
    _scene_scratch.clear()


def _scene_buffer(device, tag, shape, dtype=torch.float32):
    key = (device, _stream().value, tag, tuple(shape))
    buf = _scene_scratch.get(key)
    if buf is None:
        buf = _scene_scratch[key] = torch.empty(shape, device=device, dtype=dtype)
    return buf


def serve_scene_groups(h, w):
    """partial rows per image of ``serve_scene_stats`` (workgroups of 64 x 32 pixels)"""
    g = L.load().risp_serve_scene_groups(int(h), int(w))
    if g <= 0:
        raise ValueError('a %d x %d frame is outside the scene route: H even and >= 4, W a multiple of 4' % (h, w))
    return g


def _scene_frame_args(raw_u16, demosaic, ops, params, black_level, cfa):
    n, h, w = _u16_frames(raw_u16)
    _check_counts(ops, params)
    kind = _demosaic_code(demosaic)
    _, code = _sensor(black_level, cfa, h, w)
    _, oparr, blocks, keep = _stage_args(ops, params)
    return kind, code, keep, oparr, blocks


def serve_scene_stats(raw_u16, divisor, demosaic, ops, params, stat, partials=None, black_level=0, cfa='rggb', tag=0):
    """The statistics launch of the scene route (``risp_serve_scene_stats``): ``serve_classical_u8``'s pixel pipeline with the
    PREFIX stages ``ops`` / ``params`` in front of a scene stage, reduced per 64 x 32 pixel tile according to ``stat`` -
    SCENE_MEAN3 (sums of B, G, R), SCENE_MAX3 (maxima), SCENE_LOGLUM (sum of log-luminance) - into ``partials``
    (N, serve_scene_groups(H, W), 4) float32, every row written.  No image is stored.  The prefix may hold OP_GAIN3_Q8 /
    OP_TONE_REINHARD with the constants of an earlier ``serve_scene_finish``.  ``partials`` None: a buffer cached per
    device, stream, ``tag`` and shape."""
    kind, code, keep, oparr, blocks = _scene_frame_args(raw_u16, demosaic, ops, params, black_level, cfa)
    if stat not in (SCENE_MEAN3, SCENE_MAX3, SCENE_LOGLUM):
        raise ValueError('stat %r: SCENE_MEAN3, SCENE_MAX3 or SCENE_LOGLUM' % (stat,))
    n, h, w = raw_u16.shape
    shape = (n, serve_scene_groups(h, w), 4)
    if partials is None:
        partials = _scene_buffer(raw_u16.device, ('partials', tag), shape)
    elif (partials.dtype != torch.float32 or tuple(partials.shape) != shape or not partials.is_contiguous()
          or partials.device != raw_u16.device):
        raise ValueError('partials must be a contiguous float32 %s tensor on %s' % (shape, raw_u16.device))
    L.call('risp_serve_scene_stats', _p(raw_u16), float(divisor), kind, len(ops), oparr, blocks, int(stat), _p(partials), n, h, w,
           int(black_level), code, _stream())
    return partials


def serve_scene_finish(stat, partials, hw, a=None, b=None, consts=None, tag=0):
    """``partials`` (N,G,4) of ``serve_scene_stats`` -> the per-image constants of the scene stage (``risp_serve_scene_finish``;
    the rows are added in index order in double precision).  ``hw`` = H * W; ``a`` / ``b`` (N,) the plugin parameters:
    nothing for SCENE_MEAN3, the ratio for SCENE_MAX3, (white_point, middle_grey) for SCENE_LOGLUM.  Returns the block the
    stage takes: (N,3) gains for OP_GAIN3 (a view of the 4 N floats), (N,4) for OP_GAIN3_Q8 and OP_TONE_REINHARD.
    ``consts`` None: a buffer cached per device, stream, ``tag`` and shape."""
    _need_gpu(partials, 'partials')
    if partials.dtype != torch.float32 or partials.dim() != 3 or partials.shape[2] != 4 or not partials.is_contiguous():
        raise ValueError('expected contiguous float32 (N,G,4) partials, got %s %s' % (partials.dtype, tuple(partials.shape)))
    if stat not in (SCENE_MEAN3, SCENE_MAX3, SCENE_LOGLUM):
        raise ValueError('stat %r: SCENE_MEAN3, SCENE_MAX3 or SCENE_LOGLUM' % (stat,))
    n, g = partials.shape[:2]
    if consts is None:
        consts = _scene_buffer(partials.device, ('consts', tag), (n, 4))
    elif consts.dtype != torch.float32 or consts.numel() != 4 * n or not consts.is_contiguous() or consts.device != partials.device:
        raise ValueError('consts must be a contiguous float32 tensor of %d elements on %s' % (4 * n, partials.device))
    if (stat != SCENE_MEAN3 and a is None) or (stat == SCENE_LOGLUM and b is None):
        raise ValueError('stat %d needs its plugin parameters' % stat)
    a = None if a is None else _vec(a, n, partials.device)
    b = None if b is None else _vec(b, n, partials.device)
    L.call('risp_serve_scene_finish', int(stat), _p(partials), _p(a), _p(b), _p(consts), n, g, int(hw), _stream())
    return consts.view(-1)[:3 * n].view(n, 3) if stat == SCENE_MEAN3 else consts.view(n, 4)


def serve_scene_u8(raw_u16, divisor, demosaic, ops, params, reverse_channels=False, out=None, black_level=0, cfa='rggb'):
    """``serve_classical_u8`` with two more stages (``risp_serve_scene_u8``): OP_GAIN3_Q8 (white-world apply) and
    OP_TONE_REINHARD, whose blocks are the (N,4) constants of ``serve_scene_finish``; gray-world applies as OP_GAIN3 with
    that function's (N,3) gains.  Same frames, rules and bytes otherwise.  With ``out`` given nothing is allocated and the
    host does not wait."""
    kind, code, keep, oparr, blocks = _scene_frame_args(raw_u16, demosaic, ops, params, black_level, cfa)
    n, h, w = raw_u16.shape
    out = _u8_out(out, (n, h, w, 3), raw_u16.device, 4)
    L.call('risp_serve_scene_u8', _p(raw_u16), float(divisor), kind, len(ops), oparr, blocks, _p(out), int(bool(reverse_channels)),
           n, h, w, int(black_level), code, _stream())
    return out


def _denoise_frame_args(raw_u16, kind, pre_ops, pre_params, denoise, denoise_args, post_ops, post_params, black_level, cfa):
    """what ``serve_denoise_u8`` checks and forms, for the two launches that take a denoiser and scene constants together:
    (leading C arguments through post_params, CFA code, the tensors to keep alive across the call)"""
    n, h, w = _u16_frames(raw_u16)
    _check_counts(pre_ops, pre_params, post_ops, post_params)
    code_d = _demosaic_code(kind)
    code_n = DENOISE.get(denoise) if isinstance(denoise, str) else None
    if code_n is None:
        raise ValueError('unknown denoiser %r: one of %s' % (denoise, ', '.join(DENOISE)))
    if len(denoise_args) != (3, 1, 3)[code_n]:
        raise ValueError('%s takes %d arguments, got %d' % (denoise, (3, 1, 3)[code_n], len(denoise_args)))
    _, code = _sensor(black_level, cfa, h, w)
    window, search, vecs = int(denoise_args[0]), 0, []
    if code_n == 0:
        vecs = list(denoise_args[1:])
    elif code_n == 2:
        search, vecs = int(denoise_args[1]), [denoise_args[2]]
    for v in vecs:
        if not torch.is_tensor(v) or not v.is_cuda or v.dtype != torch.float32 or tuple(v.shape) != (n,) or not v.is_contiguous():
            raise ValueError('%s takes contiguous float32 (%d,) device tensors for its per-image values' % (denoise, n))
    pre = _stage_args(pre_ops, pre_params)
    post = _stage_args(post_ops, post_params)
    args = (code_d, *pre[:3], code_n, window, search, _p(vecs[0]) if vecs else None, _p(vecs[1]) if len(vecs) > 1 else None, *post[:3])
    return args, code, (pre[3], post[3], vecs)


def serve_denoise_stats(raw_u16, divisor, kind, pre_ops, pre_params, denoise, denoise_args, post_ops, post_params, stat,
                        partials=None, black_level=0, cfa='rggb', tag=0):
    """The statistics launch of a scene stage that lies BEHIND a denoiser (``risp_serve_denoise_stats``):
    ``serve_denoise_u8``'s tile pipeline - same frames, demosaic ``kind``, ``pre_ops`` / ``pre_params``, ``denoise`` /
    ``denoise_args`` (sizes 3 / 3 / (3, 3) only), ``post_ops`` / ``post_params`` - with the values behind the last post stage
    reduced per 64 x 32 pixel tile according to ``stat`` - SCENE_MEAN3 (sums of B, G, R) or SCENE_MAX3 (maxima); SCENE_LOGLUM
    is refused - into ``partials`` (N, serve_scene_groups(H, W), 4) float32 in ``serve_scene_stats``' layout, every row
    written, which ``serve_scene_finish`` takes unchanged.  No image is stored.  Either stage list may hold OP_GAIN3 /
    OP_GAIN3_Q8 with the constants of an earlier ``serve_scene_finish``; OP_TONE_REINHARD is refused.  MAX3 rows are the
    maxima of the composed route's plane exactly; a MEAN3 row lies within (64 * 32 - 1) * 2^-24 * sum|x| of its tile's exact
    sum.  ``partials`` None: a buffer cached per device, stream, ``tag`` and shape."""
    args, code, keep = _denoise_frame_args(raw_u16, kind, pre_ops, pre_params, denoise, denoise_args, post_ops, post_params,
                                           black_level, cfa)
    if stat not in (SCENE_MEAN3, SCENE_MAX3):
        raise ValueError('stat %r: SCENE_MEAN3 or SCENE_MAX3 (a log-average is not served behind a denoiser)' % (stat,))
    n, h, w = raw_u16.shape
    shape = (n, serve_scene_groups(h, w), 4)
    if partials is None:
        partials = _scene_buffer(raw_u16.device, ('partials', tag), shape)
    elif (partials.dtype != torch.float32 or tuple(partials.shape) != shape or not partials.is_contiguous()
          or partials.device != raw_u16.device):
        raise ValueError('partials must be a contiguous float32 %s tensor on %s' % (shape, raw_u16.device))
    L.call('risp_serve_denoise_stats', _p(raw_u16), float(divisor), *args, int(stat), _p(partials), n, h, w, int(black_level),
           code, _stream())
    return partials


def serve_denoise_scene_u8(raw_u16, divisor, kind, pre_ops, pre_params, denoise, denoise_args, post_ops, post_params,
                           reverse_channels=False, out=None, black_level=0, cfa='rggb'):
    """``serve_denoise_u8`` with one more stage accepted in front of and behind the denoiser
    (``risp_serve_denoise_scene_u8``): OP_GAIN3_Q8, white-world's apply step, whose block is the (N,4) constants
    ``serve_scene_finish`` gives for SCENE_MAX3; gray-world applies as OP_GAIN3 with that function's (N,3) gains.
    OP_TONE_REINHARD is refused.  Same frames, rules and - for every stage both accept - bytes as ``serve_denoise_u8``;
    given the constants, the bytes are those of the composed route evaluated with the same constants (``chain_forward`` with
    OP_GAIN3, ``origin_whiteworld`` at their places).  With ``out`` given nothing is allocated and the host does not wait."""
    args, code, keep = _denoise_frame_args(raw_u16, kind, pre_ops, pre_params, denoise, denoise_args, post_ops, post_params,
                                           black_level, cfa)
    n, h, w = raw_u16.shape
    out = _u8_out(out, (n, h, w, 3), raw_u16.device, 4)
    L.call('risp_serve_denoise_scene_u8', _p(raw_u16), float(divisor), *args, _p(out), int(bool(reverse_channels)), n, h, w,
           int(black_level), code, _stream())
    return out


COND_SHARDS = 32           # RISP_COND_SHARDS: rows of counts per image, which serve_cond_finish adds
COND_MAX_WIDTH, COND_MAX_LAYERS = 1024, 8      # the limits of risp_cond_fc_fwd and risp_serve_cond_finish


def serve_cond_hist(raw_u16, divisor, demosaic, ops, params, bins, counts=None, black_level=0, cfa='rggb', tag=0):
    """The histogram launch of the conditional route (``risp_serve_cond_hist``): ``serve_classical_u8``'s pixel pipeline with
    the PREFIX stages ``ops`` / ``params`` in front of a conditional head, binned with ``histc01``'s rule (a value counts only
    inside [0,1], 1 lands in the last bin) into ``counts`` (N, COND_SHARDS, 3 * bins) int32, channel order B, G, R.  No image
    is stored.  The histogram of image n is ``counts[n].sum(0)``: integers throughout, so ``histc01`` of the composed
    intermediate exactly.  The call zeroes ``counts`` itself.  An earlier head joins the prefix as its element-wise op with
    the block of its ``serve_cond_finish``.  H even and >= 4, W % 4 == 0, H * W <= 2^24, 3 * bins <= 1024.  ``counts`` None: a
    buffer cached per device, stream, ``tag`` and shape."""
    kind, code, keep, oparr, blocks = _scene_frame_args(raw_u16, demosaic, ops, params, black_level, cfa)
    if bins != int(bins) or not 1 <= bins or 3 * bins > COND_MAX_WIDTH:
        raise ValueError('bins %r: an integer with 1 <= bins and 3 * bins <= %d' % (bins, COND_MAX_WIDTH))
    n, h, w = raw_u16.shape
    serve_scene_groups(h, w)
    if n > 65535:
        raise ValueError('%d frames: at most 65535 in one call' % n)
    if h * w > 1 << 24:
        raise ValueError('a %d x %d frame has more than 2^24 pixels: float counts stop being exact' % (h, w))
    shape = (n, COND_SHARDS, 3 * int(bins))
    if counts is None:
        counts = _scene_buffer(raw_u16.device, ('cond_counts', tag), shape, torch.int32)
    elif (counts.dtype != torch.int32 or tuple(counts.shape) != shape or not counts.is_contiguous()
          or counts.device != raw_u16.device):
        raise ValueError('counts must be a contiguous int32 %s tensor on %s' % (shape, raw_u16.device))
    L.call('risp_serve_cond_hist', _p(raw_u16), float(divisor), kind, len(ops), oparr, blocks, int(bins), _p(counts), n, h, w,
           int(black_level), code, _stream())
    return counts


def cond_widths_ok(widths):
    """whether ``serve_cond_finish`` (and ``conditional_fc``) takes these layer widths: 1 .. 8 layers, every width in
    1 .. 1024, the first a multiple of 3"""
    widths = list(widths)
    return (2 <= len(widths) <= COND_MAX_LAYERS + 1 and all(int(v) == v and 1 <= v <= COND_MAX_WIDTH for v in widths)
            and widths[0] % 3 == 0)


def cond_param_count(widths):
    """entries of the flat vector the layers and the global scalar need"""
    return sum(widths[i] * widths[i + 1] + widths[i + 1] for i in range(len(widths) - 1)) + 1


def serve_cond_finish(counts, flat, widths, scale, block=None, tag=0):
    """``counts`` (N, shards, widths[0]) of ``serve_cond_hist`` -> the head's per-image block (``risp_serve_cond_finish``): the
    shards added in integers, ``conditional_fc``'s MLP on ``flat`` / ``widths`` (same arithmetic, no activations kept), then
    ``* scale`` in fp32 (1: nothing; 5 for ConditionalWbManual).  Returns (N, widths[-1]) float32, bit for bit
    ``conditional_fc(x, flat, widths) * scale`` of the image ``counts`` was taken from.  ``block`` None: a buffer cached per
    device, stream, ``tag`` and shape."""
    _need_gpu(counts, 'counts')
    if counts.dtype != torch.int32 or counts.dim() != 3 or not counts.is_contiguous():
        raise ValueError('expected contiguous int32 (N,shards,3*bins) counts, got %s %s' % (counts.dtype, tuple(counts.shape)))
    widths = [int(v) for v in widths]
    if not cond_widths_ok(widths):
        raise ValueError('widths %r: 2 .. %d entries in 1 .. %d, the first a multiple of 3'
                         % (widths, COND_MAX_LAYERS + 1, COND_MAX_WIDTH))
    n, shards, w0 = counts.shape
    if w0 != widths[0]:
        raise ValueError('counts rows hold %d words but the first layer takes %d' % (w0, widths[0]))
    _need_gpu(flat, 'params')
    if flat.dtype != torch.float32 or flat.dim() != 1 or not flat.is_contiguous() or flat.device != counts.device:
        raise ValueError('params must be a contiguous float32 vector on %s, got %s %s' % (counts.device, flat.dtype, tuple(flat.shape)))
    if flat.numel() < cond_param_count(widths):
        raise ValueError('%d parameters, the layers %r need %d' % (flat.numel(), widths, cond_param_count(widths)))
    scale = float(scale)
    if not 0.0 < scale < float('inf'):
        raise ValueError('scale %r: a positive finite number' % (scale,))
    shape = (n, widths[-1])
    if block is None:
        block = _scene_buffer(counts.device, ('cond_block', tag), shape)
    elif block.dtype != torch.float32 or tuple(block.shape) != shape or not block.is_contiguous() or block.device != counts.device:
        raise ValueError('block must be a contiguous float32 %s tensor on %s' % (shape, counts.device))
    L.call('risp_serve_cond_finish', _p(counts), shards, _p(flat), (C.c_int * len(widths))(*widths), len(widths) - 1, scale,
           _p(block), n, _stream())
    return block


class _FanOut(torch.autograd.Function):
    """k aliases of one tensor whose gradients are added by ONE launch (operand order, the order autograd's own pairwise
    additions take: the same bits) - the slot input of a super-net feeds the proxy group, Path-Restore and the fused mixture, and
    autograd otherwise spends k - 1 element-wise launches per slot and backward pass on the sum."""

    @staticmethod
    def forward(ctx, x, k):
        return tuple(x.view_as(x) for _ in range(k))

    @staticmethod
    def backward(ctx, *gs):
        live = [_aligned16(_dev(g, 'grad')) for g in gs if g is not None]
        if not live:
            return None, None
        if len(live) == 1:
            return live[0], None
        y = torch.empty_like(live[0])
        k = len(live)
        L.call('risp_mix_fwd', L.ptr_array([g.data_ptr() for g in live]), (C.c_float * k)(*([1.0] * k)), k, _p(y), y.numel(), _stream())
        return y, None


def fan_out(x, k):
    """[x] * k, or k aliases with a one-launch gradient sum (see _FanOut) when a gradient will flow into x on the device"""
    if k < 2 or not (x.is_cuda and x.requires_grad and torch.is_grad_enabled() and x.dtype == torch.float32 and k <= L.MIX_MAX
                     and x.is_contiguous() and x.numel() % 4 == 0 and x.data_ptr() % 16 == 0):
        return [x] * k
    return list(_FanOut.apply(x, k))


class _PixelLoss(torch.autograd.Function):
    """mean((y - gt)^2) / mean(|y - gt|) with the gradient formed in the same pass (risp_pixel_loss): two launches forward, a
    scaling backward - nn.MSELoss / nn.L1Loss are an element-wise launch + a reduction forward and two launches backward."""

    @staticmethod
    def forward(ctx, y, gt, kind):
        y, gt = _dev(y, 'output'), _dev(gt, 'target')
        if y.shape != gt.shape or y.numel() % 4 or (y.data_ptr() | gt.data_ptr()) % 16:
            raise ValueError('pixel_loss: shapes %s / %s must agree, numel %% 4 == 0, 16-byte aligned' % (tuple(y.shape), tuple(gt.shape)))
        lib = L.load()
        g = torch.empty_like(y) if ctx.needs_input_grad[0] else None
        loss = torch.empty((), device=y.device, dtype=torch.float32)
        scratch = torch.empty(lib.risp_loss_scratch_floats(), device=y.device, dtype=torch.float32)
        L.call('risp_pixel_loss', _p(y), _p(gt), _p(g), _p(loss), _p(scratch), y.numel(), kind, _stream())
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gl):
        g, = ctx.saved_tensors
        return (g * gl if g is not None else None), None, None


class _LocalGlobalL2(torch.autograd.Function):
    """local_global_loss with the mean-squared loss (utils/util_loss.py:26-64) - both branches on the device in one call
    (risp_local_global_l2), the flags never leave it; backward is a scaling of the gradient formed in the same pass."""

    @staticmethod
    def forward(ctx, y, gt, flag):
        y, gt = _dev(y, 'output'), _dev(gt, 'target')
        n, c, h, w = y.shape
        lib = L.load()
        flag = flag.to(device=y.device, dtype=torch.float32).contiguous()
        g = torch.empty_like(y) if ctx.needs_input_grad[0] else None
        loss = torch.empty((), device=y.device, dtype=torch.float32)
        scratch = torch.empty(lib.risp_local_global_scratch_floats(n, c), device=y.device, dtype=torch.float32)
        L.call('risp_local_global_l2', _p(y), _p(gt), _p(flag), _p(g), _p(loss), _p(scratch), n, c, h, w, _stream())
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gl):
        g, = ctx.saved_tensors
        return (g * gl if g is not None else None), None, None


def _ssim_args(x, y, data_range):
    """checked (x, y, per-image range tensor or None, scalar range) of the SSIM entry points"""
    if not (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor)) or x.dim() != 4 or x.shape != y.shape:
        raise ValueError('ssim: expected two (N,C,H,W) tensors of one shape, got %s / %s' % (
            tuple(getattr(x, 'shape', ())), tuple(getattr(y, 'shape', ()))))
    if x.shape[2] < 7 or x.shape[3] < 7:
        raise ValueError('ssim: the 7 x 7 window needs H, W >= 7, got H=%d W=%d' % (x.shape[2], x.shape[3]))
    x, y = _dev(x, 'image'), _dev(y, 'target')
    if isinstance(data_range, torch.Tensor):
        dr = _dev(data_range, 'data_range').reshape(-1)
        if dr.numel() == 1:
            dr = dr.expand(x.shape[0]).contiguous()
        if dr.numel() != x.shape[0]:
            raise ValueError('ssim: data_range must hold one value or one per image (N=%d), got %d' % (x.shape[0], dr.numel()))
        return x, y, dr, 0.0
    return x, y, None, float(data_range)


def _ssim_forward(x, y, dr, dr_scalar, quantise):
    n, c, h, w = x.shape
    out = torch.empty(n, device=x.device, dtype=torch.float32)
    scratch = torch.empty(L.load().risp_ssim_scratch_floats(n, c, h, w), device=x.device, dtype=torch.float32)
    L.call('risp_ssim_fwd', _p(x), _p(y), _p(dr), dr_scalar, int(quantise), _p(out), _p(scratch), scratch.numel(), n, c, h, w,
           _stream())
    return out


class _Ssim(torch.autograd.Function):
    """ssim[n] of (N,C,H,W) images (risp_ssim_fwd) with the gradient with respect to the first one (risp_ssim_bwd, one launch
    that recomputes the window terms: nothing but x and y is kept).  The target and the data range receive no gradient."""

    @staticmethod
    def forward(ctx, x, y, data_range):
        if ctx.needs_input_grad[1]:
            raise RuntimeError('ssim: the target receives no gradient (risp_ssim_bwd forms d/dx only); detach it')
        x, y, dr, dr_scalar = _ssim_args(x, y, data_range)
        ctx.save_for_backward(x, y, dr)
        ctx.dr_scalar = dr_scalar
        return _ssim_forward(x, y, dr, dr_scalar, False)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gs):
        x, y, dr = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        n, c, h, w = x.shape
        gx = torch.empty_like(x)
        L.call('risp_ssim_bwd', _p(x), _p(y), _p(dr), ctx.dr_scalar, _p(_dev(gs, 'gradient')), _p(gx), n, c, h, w, _stream())
        return gx, None, None


def _written(tensors):
    """The C ABI wrote these tensors in place: bump their version counters as a torch in-place op would - the mixture-weight
    cache and the step-level reuse of the super-net key on them (a shifted parameter must miss)."""
    torch.autograd.graph.increment_version(list(tensors))


def _tensor_table(rows, with_numel_of=0):
    """risp_list_desc from rows of (a, b, c, e) tensors (None = NULL); numel of column ``with_numel_of``"""
    if len(rows) > L.LIST_MAX:
        raise ValueError('at most %d tensors per table, got %d' % (L.LIST_MAX, len(rows)))
    d = L.ListDesc()
    d.n = len(rows)
    keep = []
    for t, row in enumerate(rows):
        d.numel[t] = row[with_numel_of].numel()
        for name, v in zip('abce', row):
            if v is not None:
                if not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()):
                    raise RuntimeError('reconfigisp_amd: table entries must be contiguous fp32 CUDA/HIP tensors (no CPU fallback)')
                getattr(d, name)[t] = v.data_ptr()
                keep.append(v)
    return d, keep


class _HipImpl:
    """The product implementation: every op runs in libreconfigisp_hip.so."""

    @staticmethod
    def skip(x, p=None):
        return x

    @staticmethod
    def pixel_loss(y, gt, kind):
        return _PixelLoss.apply(y, gt, {'l2': 0, 'l1': 1}[kind])

    @staticmethod
    def local_global_l2(y, gt, flag):
        return _LocalGlobalL2.apply(y, gt, flag)

    @staticmethod
    def ssim(x, y, data_range):
        return _Ssim.apply(x, y, data_range)

    @staticmethod
    def ssim_quantised(x, y):
        x, y, dr, dr_scalar = _ssim_args(x, y, 255.0)
        return _ssim_forward(x, y, dr, dr_scalar, True)

    @staticmethod
    def darts_virtual_step(rows, momentum, lr_meta):
        """rows of (twin parameter, parameter, gradient or None, momentum buffer or None): one launch (risp_darts_virtual_step)"""
        for at in range(0, len(rows), L.LIST_MAX):
            d, _keep = _tensor_table(rows[at: at + L.LIST_MAX], 1)
            L.call('risp_darts_virtual_step', C.byref(d), float(momentum), float(lr_meta), _stream())
        _written([r[0] for r in rows])

    @staticmethod
    def list_norm_eps(tensors):
        """(2,) device tensor: the 2-norm of the concatenated tensors (None skipped) and eps = 0 if norm < 1e-6 else 0.01 / norm"""
        live = [t for t in tensors if t is not None and t.numel()]
        dev = next(t.device for t in tensors if t is not None)
        out = torch.empty(2, device=dev, dtype=torch.float32)
        pieces = [live[at: at + L.LIST_MAX] for at in range(0, len(live), L.LIST_MAX)] or [[]]
        for k, piece in enumerate(pieces):          # any number of tensors (torch.cat(...).norm() has no limit): pieces of LIST_MAX
            d, _keep = _tensor_table([(t, None, t, None) for t in piece], 0)
            L.call('risp_list_norm_eps_part', C.byref(d), _p(out), int(k == 0), int(k == len(pieces) - 1), _stream())
        return out

    @staticmethod
    def list_axpy_scalar(pairs, scalar, factor):
        """p += (factor * scalar) * d for every (p, d), scalar a one-element device tensor"""
        for at in range(0, len(pairs), L.LIST_MAX):
            d, _keep = _tensor_table([(p, None, dd, None) for p, dd in pairs[at: at + L.LIST_MAX]], 0)
            L.call('risp_list_axpy_scalar', C.byref(d), _p(scalar), float(factor), _stream())
        _written([p for p, _ in pairs])

    @staticmethod
    def darts_alpha_grad(rows, eps, lr_meta):
        """rows of (out, dalpha or None, pos or None, neg or None) -> out = dalpha - lr_meta * (pos - neg) / 2 * eps, zeros where an
        input is missing or the finite-difference term holds a NaN; returns the (len(rows),) int32 NaN flags (on the device)"""
        flags = torch.zeros(len(rows), device=rows[0][0].device, dtype=torch.int32)
        for at in range(0, len(rows), L.LIST_MAX):
            d, _keep = _tensor_table(rows[at: at + L.LIST_MAX], 0)
            L.call('risp_darts_alpha_grad', C.byref(d), _p(eps), float(lr_meta), C.c_void_p(flags.data_ptr() + 4 * at), _stream())
        _written([r[0] for r in rows])
        return flags

    @staticmethod
    def wb_manual(x, p):
        return _Pointwise.apply(x, p, 'wb_manual', 3)

    @staticmethod
    def gamma(x, p):
        return _Pointwise.apply(x, p, 'gamma', 1)

    @staticmethod
    def gtm_manual(x, p):
        return _Pointwise.apply(x, p, 'gtm_manual', 3)

    @staticmethod
    def wb_quadratic(x, p):
        return _Pointwise.apply(x, p, 'wb_quadratic', 30)

    @staticmethod
    def grayworld(x, p=None):
        return _Grayworld.apply(x)

    @staticmethod
    def demosaic_nearest(x, p=None):
        return _DemosaicNearest.apply(x)

    @staticmethod
    def mix(w, outs, w_host=None, stacks=None):
        return _Mix.apply(w, w_host, stacks, *outs)

    @staticmethod
    def slot_mix(w, x, entries, w_host=None, stacks=None):
        kinds, flat = [], []
        for e in entries:
            if e[0] == 'tensor':
                kinds.append(L.SLOT_TENSOR)
                flat.append(e[1])
            else:
                kinds.append(SLOT_KINDS[e[1]])
                if e[1] not in ('skip', 'grayworld'):
                    flat.append(e[2])
        return _SlotMix.apply(w, w_host, x, tuple(kinds), stacks, *flat)

    @staticmethod
    def can_fuse_slot(x, names, tensors=()):
        """element-wise operands can be evaluated inside the mixture kernel: BGR input, 16-byte planes (the slot input and every
        materialised operand in ``tensors``), one of each kind"""
        return (x.is_cuda and x.dim() == 4 and x.shape[1] == 3 and (x.shape[2] * x.shape[3]) % 4 == 0 and
                x.data_ptr() % 16 == 0 and len(set(names)) == len(names) and all(nm in SLOT_KINDS for nm in names) and
                all(t.data_ptr() % 16 == 0 and t.is_contiguous() for t in tensors))

    @staticmethod
    def prune_softmax(alpha, threshold, unavailable=None):
        return _PruneSoftmax.apply(alpha, threshold, unavailable)

    @staticmethod
    def param_blocks(raws, n):
        out = []
        for at in range(0, len(raws), L.PARAM_OPS_MAX):
            out += list(_ParamBlocks.apply(n, *raws[at: at + L.PARAM_OPS_MAX]))
        return out

    @staticmethod
    def histc01(x, bins):
        return histc01(x, bins)

    @staticmethod
    def conditional_fc(img, flat, widths):
        return _hip_conditional_fc(img, flat, widths)

    @staticmethod
    def origin_demosaic(x, option, scales=(1.0, 1.0)):
        return _hip_origin_demosaic(x, option, scales)

    @staticmethod
    def origin_tonemap(x, option, params, scales=(1.0, 1.0)):
        return _hip_origin_tonemap(x, option, params, scales)

    @staticmethod
    def origin_whiteworld(x, ratio, scales=(1.0, 1.0)):
        return _hip_origin_whiteworld(x, ratio, scales)

    @staticmethod
    def origin_denoise(x, option, params, scales=(1.0, 1.0)):
        return _hip_origin_denoise(x, option, params, scales)

    # CNN families: `module` is the nn.Module that owns the reference-shaped parameters
    @staticmethod
    def srcnn_res(x, pv, module):
        from . import convnets as CN
        packs = _packs(module, lambda: CN.build_srcnn_packs(module.srcnn, residual=True))
        # weight gradients only on request (proxy fine-tuning sets module.train_weights); the search itself never
        # uses them, although the proxies' tensors nominally require grad
        training = getattr(module, 'train_weights', False) and torch.is_grad_enabled()
        return CN.srcnn_res(x, pv, packs, module if training else None)

    @staticmethod
    def srcnn_demosaic(x, module):
        from . import convnets as CN
        packs = _packs(module, lambda: CN.build_srcnn_packs(module.srcnn))
        return CN.srcnn_demosaic(x, packs)

    @staticmethod
    def srcnn_res_group(x, pvs, modules, cache):
        from . import convnets as CN
        packs = [_packs(m, (lambda m=m: CN.build_srcnn_packs(m.srcnn, residual=True))) for m in modules]
        return CN.srcnn_res_group(x, pvs, packs, cache)

    @staticmethod
    def srcnn_demosaic_group(x, modules, cache, record=None):
        from . import convnets as CN
        packs = [_packs(m, (lambda m=m: CN.build_srcnn_packs(m.srcnn))) for m in modules]
        return CN.srcnn_demosaic_group(x, packs, cache, record)

    @staticmethod
    def can_group(modules, x):
        """True when these same-class proxies can run as one grouped launch per layer on input x"""
        from . import convnets as CN
        from .codes.models.modules.srcnn_res_arch import SRCNNRes
        if len(modules) < 2 or not x.is_cuda or x.shape[3] % 4 or x.data_ptr() % 16:
            return False
        if any(getattr(m, 'train_weights', False) for m in modules) and torch.is_grad_enabled():
            return False                             # a proxy under fine-tuning needs its weight gradients: own launches
        if isinstance(modules[0], SRCNNRes):
            return CN._srcnn_fold_ok(x.shape[2], x.shape[3]) and all(m.srcnn[4].weight.shape[0] <= 4 for m in modules)
        return x.shape[2] % 2 == 0 and x.shape[3] % 8 == 0

    @staticmethod
    def path14l_bayer(x, module):
        from . import convnets as CN
        packs = _packs(module, lambda: CN.build_path14l_packs(module.path_restore_14l, False))
        return CN.path14l(x, packs, True, module.__dict__.get('_risp_reuse'))

    @staticmethod
    def path14l_bgr(x, module):
        from . import convnets as CN
        packs = _packs(module, lambda: CN.build_path14l_packs(module.path_restore_14l, True))
        return CN.path14l(x, packs, False, module.__dict__.get('_risp_reuse'))

    @staticmethod
    def demosaicnet(x, net, record=None):
        from . import convnets as CN
        return CN.demosaicnet(x, net.packs(x.device), record)


def _packs(module, build):
    from . import convnets as CN
    cache = module.__dict__.get('_risp_pack_cache')
    if cache is None:
        cache = module.__dict__['_risp_pack_cache'] = CN.PackCache()
    return cache.get(module, build)


_IMPL = _HipImpl


def skip(x, p=None):
    return _IMPL.skip(x, p)


def wb_manual(x, p):
    return _IMPL.wb_manual(x, p)


def gamma(x, p):
    return _IMPL.gamma(x, p)


def gtm_manual(x, p):
    return _IMPL.gtm_manual(x, p)


def wb_quadratic(x, p):
    return _IMPL.wb_quadratic(x, p)


def grayworld(x, p=None):
    return _IMPL.grayworld(x, p)


def demosaic_nearest(x, p=None):
    return _IMPL.demosaic_nearest(x, p)


def mix(w, outs, w_host=None, stacks=None):
    """sum_k w[k] * outs[k]; ``w_host``: the same weights as Python floats when the caller already holds them;
    ``stacks``: lists of operand positions whose gradients should come back as consecutive slices of one buffer (the
    members of a grouped launch read them in place)."""
    return _IMPL.mix(w, outs, w_host, stacks)


def slot_mix(w, x, entries, w_host=None, stacks=None):
    """The mixture of a slot with its element-wise operators evaluated on the fly.  entries[k] = ('tensor', o_k) for a
    materialised operand or ('op', name, block) with name in SLOT_KINDS and block the (N,P) parameter block the operator
    module would receive (None for skip / grayworld).  Same value as running the modules and ``mix``."""
    return _IMPL.slot_mix(w, x, entries, w_host, stacks)


def can_fuse_slot(x, names, tensors=()):
    return _IMPL.can_fuse_slot(x, names, tensors)


def pixel_loss(y, gt, kind='l2'):
    """nn.MSELoss ('l2') / nn.L1Loss ('l1') of the reference (models/darts_model.py:58-63, isp_model.py:29-34): a 0-dim tensor"""
    return _IMPL.pixel_loss(y, gt, kind)


def local_global_l2(y, gt, flag):
    """local_global_loss(y, gt, flag, nn.MSELoss()) of the reference (utils/util_loss.py:26-64): a 0-dim tensor"""
    return _IMPL.local_global_l2(y, gt, flag)


def ssim(x, y, data_range=1.0):
    """SSIM of every image of x against y, (N,C,H,W) -> (N,): get_ssim of the reference (utils/util_path_restore.py:27-44 -
    7 x 7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance, valid windows, mean over channels).  ``data_range``: a
    number, or a device tensor with one value per image.  Differentiable once with respect to x."""
    return _IMPL.ssim(x, y, data_range)


def ssim_loss(x, y, data_range=1.0):
    """1 - mean_n ssim(x, y)[n]: a 0-dim tensor"""
    return 1.0 - ssim(x, y, data_range).mean()


def ssim_quantised(x, y):
    """ssim of tensor2bgr(x) against tensor2bgr(y) (truncated 8-bit codes, data range 255) without leaving the GPU: (N,), no
    gradient - the twin of utils.util.psnr_tensors"""
    return _IMPL.ssim_quantised(x, y)


def darts_virtual_step(rows, momentum, lr_meta):
    return _IMPL.darts_virtual_step(rows, momentum, lr_meta)


def list_norm_eps(tensors):
    return _IMPL.list_norm_eps(tensors)


def list_axpy_scalar(pairs, scalar, factor):
    return _IMPL.list_axpy_scalar(pairs, scalar, factor)


def darts_alpha_grad(rows, eps, lr_meta):
    return _IMPL.darts_alpha_grad(rows, eps, lr_meta)


def prune_softmax(alpha, threshold, unavailable=None):
    """Mixture weights of a slot (super_prune_fifteen_demos_four_bayer_two.py:185-193): softmax, strict-< pruning
    against threshold * max on detached values, renormalisation by the detached sum.  ``unavailable``: uint8 mask of
    ops whose probability is forced to 0.  Returns post (K,), differentiable in alpha."""
    return _IMPL.prune_softmax(alpha, threshold, unavailable)


def param_blocks(raws, n):
    """[sigmoid(r).repeat(n, 1) for r in raws] (:204-209), one launch for the whole list."""
    return _IMPL.param_blocks(list(raws), n) if len(raws) else []


def hist_features(x, bins):
    return _IMPL.histc01(x, bins)


def conditional_fc(img, flat, widths):
    """(N, widths[-1]) = sigmoid(MLP(per-channel histograms of img) + flat[global]); widths = (3*bins, ..., out)."""
    return _IMPL.conditional_fc(img, flat, widths)


def srcnn_res(x, pv, module):
    return _IMPL.srcnn_res(x, pv, module)


def srcnn_demosaic(x, module):
    return _IMPL.srcnn_demosaic(x, module)


def srcnn_res_group(x, pvs, modules, cache):
    """[srcnn_res(x, pvs[g], modules[g]) for g] as ONE launch per layer (convnets.srcnn_res_group)."""
    return _IMPL.srcnn_res_group(x, pvs, modules, cache)


def srcnn_demosaic_group(x, modules, cache, record=None):
    return _IMPL.srcnn_demosaic_group(x, modules, cache, record)


def can_group(modules, x):
    return _IMPL.can_group(modules, x)


def path14l_bayer(x, module):
    return _IMPL.path14l_bayer(x, module)


def path14l_bgr(x, module):
    return _IMPL.path14l_bgr(x, module)


def demosaicnet(x, net, record=None):
    """DemosaicNet (include/risp.h): (N,1,H,W) RGGB mosaic in [0,1] -> (N,3,H,W) BGR, differentiable in x.  ``net``: a
    ``reconfigisp_amd.load_demosaicnet`` result; ``record``: step-level reuse (convnets._Path14l)."""
    return _IMPL.demosaicnet(x, net, record)


# ---------------------------------------------------------------------------
# classical "Origin" kernels (0..255 domain, non-differentiable)
# ---------------------------------------------------------------------------
def _vec(v, n, device, dtype=torch.float32):
    """per-image plugin parameter (numpy array / tensor / scalar) -> contiguous (N,) device tensor"""
    t = torch.as_tensor(v).detach().to(device=device, dtype=dtype).reshape(-1)
    if t.numel() == 1 and n > 1:
        t = t.repeat(n)
    if t.numel() != n:
        raise ValueError('expected %d per-image values, got %d' % (n, t.numel()))
    return t.contiguous()


def _check_odd(name, v):
    v = int(v)
    if v < 1 or v > 17 or v % 2 == 0:     # 17 = (1 * 7) * 2 + 3: a saturated sigmoid parameter (tools_origin.py:698,746,787)
        raise ValueError('%s must be an odd size in 1..17, got %d' % (name, v))
    return v


def _hip_origin_demosaic(x, option, scales=(1.0, 1.0)):
    x = _dev(x.detach(), 'img')
    if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] % 2 or x.shape[3] % 2:
        raise ValueError('expected a (N,1,H,W) RGGB mosaic with even H, W; got %s' % (tuple(x.shape),))
    n, _, h, w = x.shape
    y = torch.empty((n, 3, h, w), device=x.device, dtype=torch.float32)
    L.call('risp_origin_demosaic', _p(x), _p(y), int(option == 'laplacian'), n, h, w, scales[0], scales[1], _stream())
    return y


_TONEMAP = {'reinhard': (0, 'white_point', 'middle_grey'), 'crysisengine': (1, 'lum_adapted', None),
            'filmic': (2, 'white_point', 'exposure_bias')}


def _aligned16(x):
    """risp_origin_tonemap and risp_mix_fwd / _bwd read their planes in 16-byte vectors and refuse any other pointer: a
    contiguous view whose storage offset is no multiple of 4 floats is copied to a fresh tensor first"""
    return x.clone() if x.data_ptr() % 16 else x


def _hip_origin_tonemap(x, option, params, scales=(1.0, 1.0)):
    x = _dev(x.detach(), 'img')
    _check_bgr(x)
    x = _aligned16(x)
    n, hw = x.shape[0], x.shape[2] * x.shape[3]
    mode, ka, kb = _TONEMAP[option]
    a = _vec(params[ka], n, x.device)
    b = _vec(params[kb], n, x.device) if kb else None
    y = torch.empty_like(x)
    ws = torch.empty(L.load().risp_origin_tonemap_scratch_floats(n), device=x.device, dtype=torch.float32)
    L.call('risp_origin_tonemap', _p(x), _p(y), mode, _p(a), _p(b), None, _p(ws), n, hw, scales[0], scales[1],
           _stream())
    return y


def _hip_origin_whiteworld(x, ratio, scales=(1.0, 1.0)):
    x = _dev(x.detach(), 'img')
    _check_bgr(x)
    x = _aligned16(x)
    n, hw = x.shape[0], x.shape[2] * x.shape[3]
    stats, _ = channel_stats(x, want_arg=False)
    y = torch.empty_like(x)
    ws = torch.empty(L.load().risp_origin_tonemap_scratch_floats(n), device=x.device, dtype=torch.float32)
    r = _vec(ratio, n, x.device)          # keep every operand alive until the launch is enqueued
    L.call('risp_origin_tonemap', _p(x), _p(y), 3, _p(r), None, _p(stats), _p(ws), n, hw, scales[0], scales[1],
           _stream())
    return y


def _hip_origin_denoise(x, option, params, scales=(1.0, 1.0)):
    x = _dev(x.detach(), 'img')
    if option == 'bm3d':                  # any H, W >= n1
        return _hip_origin_bm3d(x, 2.55 * _vec(params['cff'], x.shape[0], x.device), params['n1'], params['cspace'],
                                params['wtransform'], params['neighborhood'], scales)[0]
    if x.dim() != 4 or x.shape[1] != 3:   # any H, W above the radius: the entry points pick the tile form themselves
        raise ValueError('expected a (N,3,H,W) BGR tensor, got %s' % (tuple(x.shape),))
    n, _, h, w = x.shape
    y = torch.empty_like(x)
    if option == 'median':
        L.call('risp_origin_median', _p(x), _p(y), _check_odd('median size', params['size']), n, h, w, scales[0],
               scales[1], _stream())
    elif option == 'bilateral':
        win = _vec(params['window_length'], n, x.device, torch.int32)
        sc, ss = _vec(params['sigma_color'], n, x.device), _vec(params['sigma_space'], n, x.device)
        wmax = _check_odd('window_length', params.get('max_window') or win.max().item())
        L.call('risp_origin_bilateral', _p(x), _p(y), _p(win), _p(sc), _p(ss), wmax, n, h, w, scales[0], scales[1],
               _stream())
    elif option == 'fastnlm':
        blk = _vec(params['block_size'], n, x.device, torch.int32)
        srch = _vec(params['search_block'], n, x.device, torch.int32)
        dec = _vec(params['decay_factor'], n, x.device)
        bmax = _check_odd('block_size', params.get('max_block') or blk.max().item())
        smax = _check_odd('search_block', params.get('max_search') or srch.max().item())
        L.call('risp_origin_fastnlm', _p(x), _p(y), _p(blk), _p(srch), _p(dec), bmax, smax, n, h, w, scales[0],
               scales[1], _stream())
    else:
        raise ValueError('unknown denoiser %r' % (option,))
    return y


BM3D_N1 = (4, 8)
BM3D_RADIUS_MAX = 9
BM3D_SCRATCH_CAP = 4 << 30        # bytes of BM3D scratch a batch may take before it runs in chunks
# (device, stream) -> uint8 buffer, grown on demand and kept: it holds at least one image (89 MB at 256 x 256, about
# 16 GB for a 4000 x 3000 frame, whatever the cap) until release_bm3d_scratch() drops it
_bm3d_scratch = {}


def bm3d_table_rows(h, w):
    """rows of the BM3D group table: the reference-block grid of n1 = 4 (risp.h 'bm3d')"""
    return ((h - 2) // 3 + 1) * ((w - 2) // 3 + 1)


def release_bm3d_scratch():
    """Drop the cached BM3D scratch of every device and stream (the memory returns to PyTorch's caching allocator;
    torch.cuda.empty_cache() hands it back to the device).  The next BM3D call allocates again."""
    _bm3d_scratch.clear()


def _bm3d_workspace(device, nbytes):
    key = (device, _stream().value)
    buf = _bm3d_scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _bm3d_scratch[key] = torch.empty(nbytes, device=device, dtype=torch.uint8)
    return buf


def _hip_origin_bm3d(x, sigma, n1, cspace, wtransform, radius, scales=(1.0, 1.0), scratch_bytes=None,
                     want_groups=False):
    """risp_origin_bm3d on a (N,3,H,W) batch; per-image parameters as in risp.h.  scratch_bytes: the scratch the batch
    may use (>= one image; default: the whole batch up to BM3D_SCRATCH_CAP); it is cached per (device, stream) until
    release_bm3d_scratch().  Returns (y, groups or None)."""
    x = _dev(x.detach(), 'img')
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError('expected a (N,3,H,W) BGR tensor, got %s' % (tuple(x.shape),))
    n, _, h, w = x.shape
    sig = _vec(sigma, n, x.device)
    blk, cs, wt, rad = (_vec(v, n, x.device, torch.int32) for v in (n1, cspace, wtransform, radius))
    host = torch.stack([blk, cs, wt, rad]).cpu()
    if not all(int(v) in BM3D_N1 for v in host[0]):
        raise ValueError('bm3d: n1 must be 4 or 8, got %s' % (host[0].tolist(),))
    if int(host[0].max()) > min(h, w):
        raise ValueError('bm3d: an n1 x n1 block does not fit a %d x %d image' % (h, w))
    if int(host[3].min()) < 1 or int(host[3].max()) > BM3D_RADIUS_MAX:
        raise ValueError('bm3d: the search radius must lie in 1..%d, got %s' % (BM3D_RADIUS_MAX, host[3].tolist()))
    lib = L.load()
    per = lib.risp_origin_bm3d_scratch_bytes(1, h, w)
    if per == 0:
        raise ValueError('bm3d: a %d x %d image is outside 4 <= H, W <= 65535, 3 H W < 2^31' % (h, w))
    if scratch_bytes is None:
        scratch_bytes = max(per, min(n * per, BM3D_SCRATCH_CAP // per * per))
    ws = _bm3d_workspace(x.device, scratch_bytes)
    y = torch.empty_like(x)
    groups = torch.empty((n, bm3d_table_rows(h, w), 17), device=x.device, dtype=torch.int32) if want_groups else None
    L.call('risp_origin_bm3d', _p(x), _p(y), _p(sig), _p(blk), _p(cs), _p(wt), _p(rad), n, h, w, scales[0], scales[1],
           _p(ws), scratch_bytes, _p(groups), _stream())
    return y, groups


def origin_bm3d(x, sigma, n1, cspace, wtransform, radius, scales=(1.0, 1.0), scratch_bytes=None, want_groups=False):
    """The classical BM3D of risp.h on a (N,3,H,W) BGR batch (0..255 after scales[0]); sigma in codes, the other
    parameters per image or scalar.  Returns (y, groups): groups (N, bm3d_table_rows(H, W), 17) int32 when
    want_groups, else None."""
    return _hip_origin_bm3d(x, sigma, n1, cspace, wtransform, radius, scales, scratch_bytes, want_groups)


def origin_demosaic(x, option, scales=(1.0, 1.0)):
    return _IMPL.origin_demosaic(x, option, scales)


def origin_tonemap(x, option, params, scales=(1.0, 1.0)):
    return _IMPL.origin_tonemap(x, option, params, scales)


def origin_whiteworld(x, ratio, scales=(1.0, 1.0)):
    return _IMPL.origin_whiteworld(x, ratio, scales)


def origin_denoise(x, option, params, scales=(1.0, 1.0)):
    return _IMPL.origin_denoise(x, option, params, scales)
