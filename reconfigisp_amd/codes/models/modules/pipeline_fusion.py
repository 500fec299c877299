"""Segment fusion for fixed pipelines (inference): maximal runs of element-wise stages are
executed by ONE ``risp_chain_fwd`` launch that reads the segment input once and writes every
stage output (``intermediate_results`` is API: test.py:74 consumes every stage).

Stages that need a whole-image quantity first (gray-world means, conditional-head histograms)
start a new segment: the reduction runs on the segment input, then the stage joins the next
chain as a per-image-parameter op.  CNN stages and the classical stencils run as themselves.
"""
import torch

from .... import functional as F
from . import tools_origin as T

_CHAIN_OP = {T.WbManual: F.OP_WB_MANUAL, T.Gamma: F.OP_GAMMA, T.GtmManual: F.OP_GTM_MANUAL,
             T.WbQuadratic: F.OP_WB_QUADRATIC, T.Skip: F.OP_SKIP}
_COND_OP = {T.ConditionalGamma: (F.OP_GAMMA, 1.0), T.ConditionalWbManual: (F.OP_WB_MANUAL, 5.0),
            T.ConditionalWbQuadratic: (F.OP_WB_QUADRATIC, 1.0)}
MAX_CHAIN = 8
_UNIT = (255.0, 255.0)     # the classical kernels work in 0..255: x255 on load, /255 on store, in the kernel


def _origin_call(mod, par):
    """Closure running one classical op directly on [0,1] tensors (no x255 / /255 passes, no host
    round trip per call): the plugin parameters are derived once per parameter version."""
    opt = mod.option
    if isinstance(mod, (T.OriginDemosBilinear, T.OriginDemosLaplacian)):
        return lambda x: F.origin_demosaic(x, opt, _UNIT)
    p = par.detach()
    if isinstance(mod, T.OriginToneReinhard):
        d = {'white_point': p[:, 0].contiguous(), 'middle_grey': p[:, 1].contiguous()}
        return lambda x: F.origin_tonemap(x, opt, d, _UNIT)
    if isinstance(mod, T.OriginToneCrysis):
        d = {'lum_adapted': p[:, 0].contiguous()}
        return lambda x: F.origin_tonemap(x, opt, d, _UNIT)
    if isinstance(mod, T.OriginToneFilmic):
        d = {'white_point': p[:, 0].contiguous(), 'exposure_bias': (p[:, 1] * 9. + 1.).contiguous()}
        return lambda x: F.origin_tonemap(x, opt, d, _UNIT)
    if isinstance(mod, T.OriginWbWhiteworld):
        r = p[:, 0].contiguous()
        return lambda x: F.origin_whiteworld(x, r, _UNIT)
    d = mod._params(p, {})                       # bilateral / median / fastnlm: the wrapper's own scaling rules
    if isinstance(mod, T.OriginNoiseBilateral):
        d['max_window'] = int(d['window_length'].max().item())
    elif isinstance(mod, T.OriginNoiseFastnlm):
        d['max_block'], d['max_search'] = int(d['block_size'].max().item()), int(d['search_block'].max().item())
    return lambda x: F.origin_denoise(x, opt, d, _UNIT)


def _run_origin(mod, x, par):
    key = None if par is None else (par.data_ptr(), par._version, tuple(par.shape))
    plan = mod.__dict__.get('_risp_origin_plan')
    if plan is None or plan[0] != key:
        plan = mod.__dict__['_risp_origin_plan'] = (key, _origin_call(mod, par))
    return plan[1](x)


def _wb_gain(mod, par):
    """params * 5 (tools_origin.py:214), computed once per parameter version."""
    key = (par.data_ptr(), par._version, tuple(par.shape))
    cached = mod.__dict__.get('_risp_gain')
    if cached is None or cached[0] != key:
        cached = mod.__dict__['_risp_gain'] = (key, par.detach() * 5)
    return cached[1]


def _chain_param(mod, par):
    return _wb_gain(mod, par) if type(mod) is T.WbManual else par


def _flush(x, ops, params, results, out_last=None):
    if not ops:
        return x
    if all(o == F.OP_SKIP for o in ops):
        results.extend([x] * len(ops))
        return x
    outs = F.chain_forward(x, ops, params, out_last)
    results.extend(outs)
    return outs[-1]


def _bilateral_args(mod, par):
    """(window int32, sigma_color, sigma_space, largest window) of a bilateral stage, derived once per parameter version."""
    key = (par.data_ptr(), par._version, tuple(par.shape))
    cached = mod.__dict__.get('_risp_bilateral_args')
    if cached is None or cached[0] != key:
        d = mod._params(par.detach(), {})
        cached = mod.__dict__['_risp_bilateral_args'] = (
            key, d['window_length'].to(torch.int32).contiguous(), d['sigma_color'].contiguous(),
            d['sigma_space'].contiguous(), int(d['window_length'].max().item()))
    return cached[1:]


def _bilateral_segment(mod, par, x, from_bayer, tail_ops, tail_params):
    """[demosaic ->] bilateral -> element-wise tail as one launch; returns the stage outputs."""
    win, sc, ss, wmax = _bilateral_args(mod, par)
    return F.BilateralChainPlan(x, from_bayer, win, sc, ss, wmax, tail_ops, tail_params).launch()


def fused_forward(modules, param_tensors, x, final_out=None):
    """modules[k](x, param_tensors[k]) for all k, fusing where possible.  Returns (y, stage outputs).  ``final_out``: where the caller
    wants the LAST stage (test_split: a slice of the frame's tile stack - no concatenation afterwards); honoured when the pipeline ends in
    an element-wise segment, otherwise the last stage is copied there."""
    results, ops, params = [], [], []
    seg_in = x                                    # input of the pending element-wise chain
    k, count = 0, len(modules)
    while k < count:
        mod, par = modules[k], param_tensors[k]
        kind = type(mod)
        if kind is T.DemosaicNearest:
            x = _flush(x, ops, params, results)
            seg_in, ops, params = x, [F.OP_DEMOSAIC_NEAREST], [None]
        elif kind is T.OriginNoiseBilateral and x.shape[3] % 4 == 0 and x.shape[2] % 2 == 0 and min(x.shape[2:]) > 8:
            from_bayer = ops == [F.OP_DEMOSAIC_NEAREST]
            if not from_bayer:
                x = _flush(x, ops, params, results)
                seg_in = x
            tail_ops, tail_params, j = [], [], k + 1
            while j < count and type(modules[j]) in _CHAIN_OP and len(tail_ops) < MAX_CHAIN:
                tail_ops.append(_CHAIN_OP[type(modules[j])])
                tail_params.append(_chain_param(modules[j], param_tensors[j]))
                j += 1
            outs = _bilateral_segment(mod, par, seg_in, from_bayer, tail_ops, tail_params)
            results.extend(outs)
            x, ops, params, k = outs[-1], [], [], j - 1
        elif kind in _CHAIN_OP and len(ops) < MAX_CHAIN:
            if not ops:
                seg_in = x
            ops.append(_CHAIN_OP[kind])
            params.append(_chain_param(mod, par))
        elif kind is T.Grayworld or kind in _COND_OP or kind in _CHAIN_OP:
            x = _flush(x, ops, params, results)
            seg_in = x
            if kind is T.Grayworld:
                ops, params = [F.OP_GAIN3], [F.grayworld_gains(x)]
            elif kind in _COND_OP:
                ops, params = [_COND_OP[kind][0]], [mod._fc_forward(x, par) * _COND_OP[kind][1]]
            else:
                ops, params = [_CHAIN_OP[kind]], [_chain_param(mod, par)]
        else:
            x = _flush(x, ops, params, results)
            ops, params = [], []
            x = _run_origin(mod, x, par) if isinstance(mod, T._OriginOp) else mod(x, par)
            results.append(x)
        k += 1
    x = _flush(x, ops, params, results, final_out)
    if final_out is not None and results and x.data_ptr() != final_out.data_ptr() and tuple(x.shape) == tuple(final_out.shape):
        final_out.copy_(x)
        x = results[-1] = final_out
    return x, results


def _serve_split(modules):
    """(index of the bilateral stage or None, indices of the chain stages) when the pipeline, Skips stripped, is
    DemosaicNearest [-> OriginNoiseBilateral] -> at most MAX_CHAIN element-wise stages; None otherwise."""
    idx = [k for k, m in enumerate(modules) if type(m) is not T.Skip]
    if not idx or type(modules[idx[0]]) is not T.DemosaicNearest:
        return None
    rest = idx[1:]
    bil = None
    if rest and type(modules[rest[0]]) is T.OriginNoiseBilateral:
        bil, rest = rest[0], rest[1:]
    if len(rest) > MAX_CHAIN or any(type(modules[k]) not in _CHAIN_OP for k in rest):
        return None
    return bil, rest


def serve_plan(modules):
    """What ``serve`` does with this module list (a pure function of it, no GPU needed): ``'fused'`` - one launch,
    uint16 in and packed bytes out - when the pipeline, Skips stripped, is the nearest demosaic, an optional classical
    bilateral and at most MAX_CHAIN WbManual / Gamma / GtmManual / WbQuadratic stages; ``'composed'`` otherwise - the
    uint16 -> fp32 input kernel, the ordinary ``fused_forward`` and ``quantise_u8`` on the last stage.  Gray-world and
    the conditional heads (a whole-image quantity first), CNN stages and the other classical stencils compose.  (A
    bilateral whose learned window exceeds 3 composes too: known only from the parameters, ``serve`` checks it.)
    ``'composed'`` here reads "not ``risp_serve_u8``": ``serve_route`` tells the classical one launch from the rest."""
    return 'fused' if _serve_split(modules) is not None else 'composed'


_CLASSICAL_DEMOSAIC = {T.DemosaicNearest: 'nearest', T.OriginDemosBilinear: 'bilinear', T.OriginDemosLaplacian: 'laplacian'}
_TONE_OP = {T.OriginToneCrysis: F.OP_TONE_CRYSIS, T.OriginToneFilmic: F.OP_TONE_FILMIC}


def _classical_head(modules):
    """(demosaic kind, indices of the stages behind it) when the pipeline, Skips stripped, opens with DemosaicNearest /
    OriginDemosBilinear / OriginDemosLaplacian; None otherwise"""
    idx = [k for k, m in enumerate(modules) if type(m) is not T.Skip]
    if not idx or type(modules[idx[0]]) not in _CLASSICAL_DEMOSAIC:
        return None
    return _CLASSICAL_DEMOSAIC[type(modules[idx[0]])], idx[1:]


def _classical_split(modules):
    """(demosaic kind, indices of the stages) when the pipeline, Skips stripped, is DemosaicNearest / OriginDemosBilinear /
    OriginDemosLaplacian -> at most MAX_CHAIN stages, each an element-wise one, OriginToneCrysis or OriginToneFilmic; None
    otherwise."""
    head = _classical_head(modules)
    if head is None:
        return None
    kind, rest = head
    if len(rest) > MAX_CHAIN or any(type(modules[k]) not in _CHAIN_OP and type(modules[k]) not in _TONE_OP for k in rest):
        return None
    return kind, rest


def serve_route(modules):
    """The route ``serve`` takes for this module list (a pure function of it): ``'fused'`` exactly where ``serve_plan``
    says so (``risp_serve_u8``); ``'classical'`` - still one launch, ``risp_serve_classical_u8`` - when the pipeline, Skips
    stripped, is the nearest, the classical bilinear or the classical Malvar-He-Cutler demosaic followed by at most
    MAX_CHAIN stages, each WbManual / Gamma / GtmManual / WbQuadratic or a classical Crysis / Filmic tone curve;
    ``'composed'`` otherwise.  A bilateral behind a stencil demosaic, Reinhard, white-world and gray-world (a whole-image
    quantity first), median / NLM / BM3D and every CNN stage compose on the default call; ``scene_plan`` and ``denoise_plan``
    name the lists among them that ``serve(fast_scene=True)`` / ``serve(fast_denoise=True)`` take without fp32 planes."""
    if _serve_split(modules) is not None:
        return 'fused'
    return 'classical' if _classical_split(modules) is not None else 'composed'


def _tone_block(mod, par):
    """the parameter block ``risp_serve_classical_u8`` takes for a tone curve - what ``_origin_call`` hands to
    ``F.origin_tonemap`` - derived once per parameter version"""
    key = (par.data_ptr(), par._version, tuple(par.shape))
    cached = mod.__dict__.get('_risp_tone_block')
    if cached is None or cached[0] != key:
        p = par.detach()
        if type(mod) is T.OriginToneCrysis:
            block = p[:, :1].float().contiguous()
        else:
            block = torch.stack([p[:, 0], p[:, 1] * 9. + 1.], dim=1).float().contiguous()
        cached = mod.__dict__['_risp_tone_block'] = (key, block, par)      # (par kept: its address stays its own while the key lives)
    return cached[1]


def _stage_op(mod, par):
    """(op code, parameter block) of an element-wise, Crysis or Filmic stage as the serving launches take it"""
    if type(mod) in _TONE_OP:
        return _TONE_OP[type(mod)], _tone_block(mod, par)
    return _CHAIN_OP[type(mod)], _chain_param(mod, par)


_SCENE_STAT = {T.Grayworld: F.SCENE_MEAN3, T.OriginWbWhiteworld: F.SCENE_MAX3, T.OriginToneReinhard: F.SCENE_LOGLUM}
_SCENE_OP = {T.Grayworld: F.OP_GAIN3, T.OriginWbWhiteworld: F.OP_GAIN3_Q8, T.OriginToneReinhard: F.OP_TONE_REINHARD}


def scene_plan(modules):
    """(demosaic kind, indices of the stages, which of them are scene stages) when ``serve(fast_scene=True)`` can take the
    scene route for this module list (a pure function of it): Skips stripped, a nearest, classical bilinear or classical
    Malvar-He-Cutler demosaic followed by at most MAX_CHAIN stages, each an element-wise one, a classical Crysis / Filmic
    tone curve or one of the scene stages Grayworld, OriginWbWhiteworld, OriginToneReinhard, with one or two scene stages
    among them.  None otherwise - without a scene stage ``serve_route`` already names a one-launch route."""
    head = _classical_head(modules)
    if head is None:
        return None
    kind, rest = head
    kinds = [type(modules[k]) for k in rest]
    if len(rest) > MAX_CHAIN or any(t not in _CHAIN_OP and t not in _TONE_OP and t not in _SCENE_STAT for t in kinds):
        return None
    scene = [t in _SCENE_STAT for t in kinds]
    if not 1 <= sum(scene) <= 2:
        return None
    return kind, rest, scene


def _scene_vectors(mod, par):
    """the (N,) plugin parameters ``risp_serve_scene_finish`` takes for a scene stage - what ``_origin_call`` hands to
    ``F.origin_whiteworld`` / ``F.origin_tonemap`` - derived once per parameter version"""
    if type(mod) is T.Grayworld:
        return None, None
    key = (par.data_ptr(), par._version, tuple(par.shape))
    cached = mod.__dict__.get('_risp_scene_vectors')
    if cached is None or cached[0] != key:
        p = par.detach().float()
        a = p[:, 0].contiguous()
        b = p[:, 1].contiguous() if type(mod) is T.OriginToneReinhard else None
        cached = mod.__dict__['_risp_scene_vectors'] = (key, a, b, par)
    return cached[1], cached[2]


def _serve_scene(plan, modules, param_tensors, raw_u16, divisor, reverse_channels, out, black_level, cfa):
    """2 S + 1 launches for S scene stages: per scene stage the statistics of its input (the mosaic read again, the pipeline
    evaluated up to the stage, earlier scene stages with their constants) and the finish launch, then the serving launch"""
    kind, stages, scene = plan
    n, h, w = raw_u16.shape
    ops, params, s = [], [], 0
    for k, is_scene in zip(stages, scene):
        mod, par = modules[k], param_tensors[k]
        t = type(mod)
        if is_scene:
            parts = F.serve_scene_stats(raw_u16, divisor, kind, ops, params, _SCENE_STAT[t], None, black_level, cfa)
            a, b = _scene_vectors(mod, par)
            params.append(F.serve_scene_finish(_SCENE_STAT[t], parts, h * w, a, b, None, tag=s))
            ops.append(_SCENE_OP[t])
            s += 1
        else:
            op, block = _stage_op(mod, par)
            ops.append(op)
            params.append(block)
    return F.serve_scene_u8(raw_u16, divisor, kind, ops, params, reverse_channels, out, black_level, cfa)


MAX_COND_HEADS = 3         # one head of each kind; every head costs one more read of the mosaic


def cond_plan(modules):
    """(demosaic kind, indices of the stages, which of them are conditional heads) when ``serve(fast_cond=True)`` can take the
    conditional route for this module list (a pure function of it): Skips stripped, a nearest, classical bilinear or classical
    Malvar-He-Cutler demosaic followed by at most MAX_CHAIN stages, each an element-wise one, a classical Crysis / Filmic tone
    curve or one of the heads ConditionalGamma, ConditionalWbManual, ConditionalWbQuadratic, with one to MAX_COND_HEADS heads
    among them.  None otherwise: without a head ``serve_route`` already names a one-launch route; a scene stage, a classical
    denoiser or BM3D, a CNN stage or a proxy demosaic beside a head keeps the list where it is today."""
    head = _classical_head(modules)
    if head is None:
        return None
    kind, rest = head
    kinds = [type(modules[k]) for k in rest]
    if len(rest) > MAX_CHAIN or any(t not in _CHAIN_OP and t not in _TONE_OP and t not in _COND_OP for t in kinds):
        return None
    heads = [t in _COND_OP for t in kinds]
    if not 1 <= sum(heads) <= MAX_COND_HEADS:
        return None
    return kind, rest, heads


def _cond_heads_ok(plan, modules, param_tensors):
    """whether every head of the plan is one the kernels take: 3 * bins and the layer widths within risp_cond_fc_fwd's limits,
    and the flat vector what ``_fc_forward`` expects (anything else is the composed route's to refuse)"""
    for k, is_head in zip(plan[1], plan[2]):
        if is_head:
            mod, par = modules[k], param_tensors[k]
            if not F.cond_widths_ok(mod.in_out_channels):
                return False
            if (not torch.is_tensor(par) or not par.is_cuda or par.dtype != torch.float32 or par.dim() != 1
                    or not par.is_contiguous() or par.numel() != mod.total_params):
                return False
    return True


def _serve_cond(plan, modules, param_tensors, raw_u16, divisor, reverse_channels, out, black_level, cfa):
    """2 S + 1 launches for S heads: per head the histogram of its input (the mosaic read again, the pipeline evaluated up to
    the head, earlier heads with their blocks) and the finish launch on the head's raw flat vector, then the classical serving
    launch with every head as its element-wise op"""
    kind, stages, heads = plan
    ops, params, s = [], [], 0
    for k, is_head in zip(stages, heads):
        mod, par = modules[k], param_tensors[k]
        t = type(mod)
        if is_head:
            counts = F.serve_cond_hist(raw_u16, divisor, kind, ops, params, mod.hist_bin, None, black_level, cfa, tag=s)
            params.append(F.serve_cond_finish(counts, par.detach(), mod.in_out_channels, _COND_OP[t][1], None, tag=s))
            ops.append(_COND_OP[t][0])
            s += 1
        else:
            op, block = _stage_op(mod, par)
            ops.append(op)
            params.append(block)
    return F.serve_classical_u8(raw_u16, divisor, kind, ops, params, reverse_channels, out, black_level, cfa)


_DENOISER = {T.OriginNoiseBilateral: 'bilateral', T.OriginNoiseMedian: 'median', T.OriginNoiseFastnlm: 'fastnlm'}


def denoise_plan(modules):
    """(demosaic kind, indices of the stages in front of the denoiser, index of the denoiser, indices of the stages behind it)
    when ``serve(fast_denoise=True)`` can take the denoise route for this module list (a pure function of it): Skips stripped,
    a nearest, classical bilinear or classical Malvar-He-Cutler demosaic, stages, exactly one of OriginNoiseBilateral /
    OriginNoiseMedian / OriginNoiseFastnlm, more stages - each stage an element-wise one or a classical Crysis / Filmic tone
    curve, at most MAX_CHAIN of them in all.  None otherwise: where ``serve_plan`` already says ``'fused'`` (the bilateral
    directly behind the nearest demosaic), for two denoisers, scene stages, BM3D, CNN stages and the proxy pipelines.  Whether
    the learned parameters give the sizes the route serves (3 / 3 / (3, 3)) is known only from them: ``serve`` checks it."""
    if _serve_split(modules) is not None:
        return None
    head = _classical_head(modules)
    if head is None:
        return None
    kind, rest = head
    den = [k for k in rest if type(modules[k]) in _DENOISER]
    if len(den) != 1:
        return None
    stages = [k for k in rest if k != den[0]]
    if len(stages) > MAX_CHAIN or any(type(modules[k]) not in _CHAIN_OP and type(modules[k]) not in _TONE_OP for k in stages):
        return None
    return kind, [k for k in stages if k < den[0]], den[0], [k for k in stages if k > den[0]]


def _denoise_args(mod, par):
    """(name, arguments) as ``F.serve_denoise_u8`` takes them, or None when the parameters give a size the denoise route does
    not serve - derived once per parameter version (the median's size and the non-local means' sizes need a host read)"""
    if type(mod) is T.OriginNoiseBilateral:
        _, sc, ss, wmax = _bilateral_args(mod, par)
        return ('bilateral', (3, sc, ss)) if wmax == 3 else None
    key = (par.data_ptr(), par._version, tuple(par.shape))
    cached = mod.__dict__.get('_risp_denoise_args')
    if cached is None or cached[0] != key:
        d = mod._params(par.detach(), {})
        if type(mod) is T.OriginNoiseMedian:
            args = ('median', (3,)) if d['size'] == 3 else None
        else:
            sizes = torch.stack([d['block_size'], d['search_block']]).cpu()
            ok = bool((sizes == 3).all())
            args = ('fastnlm', (3, 3, d['decay_factor'].float().contiguous())) if ok else None
        cached = mod.__dict__['_risp_denoise_args'] = (key, args, par)     # (par kept: its address stays its own while the key lives)
    return cached[1]


# the median sizes ``serve(fast_median=True)`` sends to ``risp_serve_median_u8``.  A size is listed only where
# tools/bench_serve_median.py found the launch faster than the default call by more than the larger spread of the two legs at both
# of its sizes, 64 x 256 x 256 and 1 x 3000 x 4000, with the bilinear and with the Malvar-He-Cutler demosaic
# (profiles/serve_median.txt); any other size stays composed under the keyword.  functional.serve_median_u8
# serves all six either way
_MEDIAN_SIZES = frozenset({5, 7, 9, 11, 13, 15})


def _median_args(mod, par):
    """the size OriginNoiseMedian's rule gives for ``par``: 2 * int(p * 7) + 3 from image 0's parameter alone, 3 .. 17 - derived
    once per parameter version (one host read), under a key of its own beside ``_denoise_args``' cache"""
    key = (par.data_ptr(), par._version, tuple(par.shape))
    cached = mod.__dict__.get('_risp_median_size')
    if cached is None or cached[0] != key:
        cached = mod.__dict__['_risp_median_size'] = (key, int(mod._params(par.detach(), {})['size']), par)
    return cached[1]


def _stage_lists(modules, param_tensors, stages):
    """(op codes, parameter blocks) of element-wise / Crysis / Filmic stages as the classical and the denoise launch take them"""
    pairs = [_stage_op(modules[k], param_tensors[k]) for k in stages]
    return [op for op, _ in pairs], [block for _, block in pairs]


_DENOISE_SCENE_STAT = {T.Grayworld: F.SCENE_MEAN3, T.OriginWbWhiteworld: F.SCENE_MAX3}
# (denoiser, where the scene stages lie: 'front' | 'behind' | 'both') combinations that tools/bench_serve_denoise_scene.py found no
# faster than the default call at one of its two sizes (profiles/serve_denoise_scene.txt): the plan leaves them where they are.
# A scene stage behind non-local means costs a second run of the denoiser, which is compute bound: at 64 x 256 x 256 the route
# took 193.1 us against 161.6 us composed (gray-world behind) and 213.1 against 192.1 (one scene stage each side); at
# 1 x 3000 x 4000 it won (522.7 against 753.9 us, 582.2 against 811.9), but the rule asks for both sizes
_DENOISE_SCENE_SLOWER = frozenset({('fastnlm', 'behind'), ('fastnlm', 'both')})


def denoise_scene_plan(modules):
    """(demosaic kind, indices of the stages around the denoiser in pipeline order, index of the denoiser, which of the stages
    are scene stages) when ``serve(fast_denoise_scene=True)`` can take the denoise + scene route for this module list (a pure
    function of it): Skips stripped, a nearest, classical bilinear or classical Malvar-He-Cutler demosaic followed by at most
    MAX_CHAIN stages and exactly one of OriginNoiseBilateral / OriginNoiseMedian / OriginNoiseFastnlm; one or two of the stages
    are Grayworld / OriginWbWhiteworld, at any position relative to the denoiser, every other stage an element-wise one or a
    classical Crysis / Filmic tone curve.  None otherwise: a Reinhard stage anywhere (its log-average has no order-free form
    and its apply step no entry point to be held to), two denoisers, three scene stages, BM3D, CNN stages, proxies,
    conditional heads - and lists without a scene stage (``denoise_plan``'s) or without a denoiser (``scene_plan``'s), so the
    plan is disjoint from every other.  None as well for non-local means with a scene stage behind it, which was measured
    slower than the default call at 64 x 256 x 256 (``_DENOISE_SCENE_SLOWER``); the kernels serve it all the same."""
    head = _classical_head(modules)
    if head is None:
        return None
    kind, rest = head
    den = [k for k in rest if type(modules[k]) in _DENOISER]
    if len(den) != 1:
        return None
    stages = [k for k in rest if k != den[0]]
    kinds = [type(modules[k]) for k in stages]
    if len(stages) > MAX_CHAIN or any(t not in _CHAIN_OP and t not in _TONE_OP and t not in _DENOISE_SCENE_STAT for t in kinds):
        return None
    scene = [t in _DENOISE_SCENE_STAT for t in kinds]
    if not 1 <= sum(scene) <= 2:
        return None
    sides = {k < den[0] for k, s in zip(stages, scene) if s}
    where = 'both' if len(sides) == 2 else ('front' if True in sides else 'behind')
    if (_DENOISER[type(modules[den[0]])], where) in _DENOISE_SCENE_SLOWER:
        return None
    return kind, stages, den[0], scene


def _serve_denoise_scene(plan, den_args, modules, param_tensors, raw_u16, divisor, reverse_channels, out, black_level, cfa):
    """2 S + 1 launches for S scene stages: per scene stage the statistics of its input - ``risp_serve_scene_stats`` while the
    denoiser lies behind the stage, ``risp_serve_denoise_stats`` once it lies in the stage's prefix; earlier scene stages enter
    the prefix with their constants - and the finish launch, then ``risp_serve_denoise_scene_u8`` serves"""
    kind, stages, den, scene = plan
    h, w = raw_u16.shape[1:]
    pre, post, s = ([], []), ([], []), 0
    for k, is_scene in zip(stages, scene):
        mod, par = modules[k], param_tensors[k]
        t = type(mod)
        ops, params = pre if k < den else post
        if is_scene:
            stat = _DENOISE_SCENE_STAT[t]
            if k < den:
                parts = F.serve_scene_stats(raw_u16, divisor, kind, ops, params, stat, None, black_level, cfa)
            else:
                parts = F.serve_denoise_stats(raw_u16, divisor, kind, pre[0], pre[1], den_args[0], den_args[1], ops, params, stat,
                                              None, black_level, cfa)
            a, b = _scene_vectors(mod, par)
            params.append(F.serve_scene_finish(stat, parts, h * w, a, b, None, tag=s))
            ops.append(_SCENE_OP[t])
            s += 1
        else:
            op, block = _stage_op(mod, par)
            ops.append(op)
            params.append(block)
    return F.serve_denoise_scene_u8(raw_u16, divisor, kind, pre[0], pre[1], den_args[0], den_args[1], post[0], post[1],
                                    reverse_channels, out, black_level, cfa)


def _nv12_plan(out_format, yuv_matrix, reverse_channels, h, w):
    """the twelve integers of ``yuv_matrix`` for ``out_format='nv12'``, None for 'bgr8'; everything else is refused"""
    if out_format == 'bgr8':
        return None
    if out_format != 'nv12':
        raise ValueError("unknown out_format %r: 'bgr8' or 'nv12'" % (out_format,))
    if reverse_channels:
        raise ValueError("reverse_channels has no meaning with out_format='nv12': the conversion knows the channel order")
    if h % 2 or w % 2:
        raise ValueError('a %d x %d frame has no 4:2:0 form: H and W must be even' % (h, w))
    return F.nv12_matrix(yuv_matrix)


def _check_black_level(black_level, white_level):
    if black_level != int(black_level) or not 0 <= black_level < white_level:
        raise ValueError('black_level %r: an integer with 0 <= black_level < white_level (%r)' % (black_level, white_level))


def _frame_shape(raw, raw_format, raw_width, dims, typed=True):
    """(the shape in front of the frames' own dimensions, H, W) of sensor frames as given, of ``dims`` dimensions: MIPI-packed
    ones as ``_packed_plan`` checks them, otherwise one sample per element - uint16 where ``typed``; everything else is refused"""
    names = lambda: ' or '.join('(N,H,W)' if d == 3 else '(H,W)' for d in dims)       # (only a refusal pays for it)
    shaped = isinstance(raw, torch.Tensor) and raw.dim() in dims
    if not typed and not shaped:
        raise ValueError('expected %s frames, got %s' % (names(), tuple(getattr(raw, 'shape', ()))))
    if raw_format != 'u16':
        w = _packed_plan(raw, raw_format, raw_width, dims)[1]
    elif typed and not (shaped and raw.dtype == torch.uint16):
        raise ValueError('expected %s uint16 frames, got %s %s' % (names(), getattr(raw, 'dtype', type(raw)), tuple(getattr(raw, 'shape', ()))))
    else:
        w = raw.shape[-1]
    return tuple(raw.shape[:-2]), raw.shape[-2], w


SERVE_ROUTES = ('fused', 'classical', 'scene', 'denoise', 'denoise_scene', 'cond', 'composed', 'tiled')
# (route, raw_format) whose one launch decodes the packed bytes itself.  A route is listed only where the fused load beat the
# unpack launch followed by the uint16 call by more than the spread on the 3000 x 4000 frame (profiles/serve_packed.txt,
# DESIGN.md 4.6).  The classical kernel does, by 10 us; the headline kernel with its bilateral does not - its 36 narrow loads and
# their shifts cost the issue-bound launch 10-14 %, what the unpack launch costs or more - and unpacks first.  risp_serve_packed exists
# either way (functional.serve_packed): it is correct and saves the intermediate frames
_FUSED_LOAD = frozenset({('classical', 'raw10'), ('classical', 'raw12')})


def serve_load(route, raw_format):
    """Who decodes MIPI-packed frames on ``route`` (a name of ``SERVE_ROUTES``): 'fused' - the route's one launch loads the
    packed bytes (``risp_serve_packed``, ``risp_serve_classical_packed``) - or 'pass' - ``risp_raw_unpack`` writes uint16
    frames first and the route runs as for them; None for ``raw_format='u16'``.  A pure function of its arguments: what
    ``serve`` does and what ``last_serve_load`` reports."""
    if route not in SERVE_ROUTES:
        raise ValueError('unknown route %r: one of %s' % (route, ', '.join(SERVE_ROUTES)))
    if not F.raw_format_bits(raw_format):
        return None
    return 'fused' if (route, raw_format) in _FUSED_LOAD else 'pass'


def _device_frames(raw, raw_format, raw_width, dims):
    """``_frame_shape`` of frames that must be on the device: uint16 frames name a missing device first, packed ones bad frames"""
    if raw_format == 'u16':
        F._need_gpu(raw, 'raw')
    shape = _frame_shape(raw, raw_format, raw_width, dims)
    F._need_gpu(raw, 'raw')
    return shape


def _packed_plan(raw, raw_format, raw_width, dims):
    """``serve`` / ``serve_frame`` on MIPI-packed frames, checked on the host before anything else: (bits, W) for uint8 frames
    of ``dims`` dimensions whose last is the row pitch in bytes; everything else is refused"""
    bits = F.raw_format_bits(raw_format)
    if not isinstance(raw, torch.Tensor) or raw.dtype != torch.uint8 or raw.dim() not in dims:
        raise ValueError("raw_format=%r takes %s uint8 frames (rows of stride bytes), got %s %s"
                         % (raw_format, ' or '.join('(N,H,stride)' if d == 3 else '(H,stride)' for d in dims),
                            getattr(raw, 'dtype', type(raw)), tuple(getattr(raw, 'shape', ()))))
    w = F.packed_width(bits, raw.shape[-1], raw_width)
    if raw.shape[-2] % 2:
        raise ValueError('packed frames of %d rows: H must be even' % raw.shape[-2])
    return bits, w


# (route, raw_format) whose one launch applies the lens-shading correction in its load.  Only ('classical', 'u16') has such a
# launch (risp_serve_classical_shaded), and it is listed only if it beats risp_raw_shade followed by the uint16 call by more than
# the larger spread of the two legs in all four rows of profiles/serve_shade.txt (two pipelines, two sizes) - the
# rule of _FUSED_LOAD and _MEDIAN_SIZES.  The verdict line of that file is this table.  Measured: the fused launch is 2.7 to 4.8 us
# faster in all four rows (0.86-0.97 x), which clears the spread in three of them; in the fourth one round of the two-launch leg ran
# 9.5 us long.  Not all four, so the table is empty and the classical route takes the shade launch too;
# functional.serve_classical_shaded keeps the one-launch form.  The headline kernel gets no fused shading: its 6 x 8 neighbourhood
# per thread lost with packed loads already, and nobody has measured it with shading.
_FUSED_SHADE = frozenset()


def serve_shade(route, raw_format):
    """Who applies a lens shading on ``route`` (a name of ``SERVE_ROUTES``) for frames of ``raw_format``: 'fused' - the route's
    one launch shades in its load (``risp_serve_classical_shaded``) - or 'pass' - ``risp_raw_shade`` writes shaded uint16 frames
    first (decoding packed ones on the way) and the route runs as for them.  A pure function of its arguments: what ``serve``
    does and what ``last_serve_shade`` reports for a call with ``lens_shading``."""
    if route not in SERVE_ROUTES:
        raise ValueError('unknown route %r: one of %s' % (route, ', '.join(SERVE_ROUTES)))
    F.raw_format_bits(raw_format)
    return 'fused' if (route, raw_format) in _FUSED_SHADE else 'pass'


# raw formats whose defective-pixel correction and lens shading run as ONE risp_raw_defect launch (with gains) instead of
# risp_raw_defect followed by risp_raw_shade.  A format is listed only if the one launch beats the two by more than the larger
# spread of the two legs in every measured row of profiles/serve_defect.txt (two sizes per format) - the rule of
# every measured table here, tools/serve_bench.beats.  The verdict line of that file is this table.  Measured: the one launch is 7.8 to
# 9.9 us faster in all six rows (0.83-0.92 x) against spreads of 0.2 to 2.0 us - the second launch costs a launch and a second trip
# of the frames through the cache, the gains cost the first one three multiplies per sample beside some sixty instructions.
_DEFECT_SHADE_FUSED = frozenset({'u16', 'raw10', 'raw12'})


def defect_shade(raw_format):
    """How a call with both ``defect_correction`` and ``lens_shading`` runs its pre-pass for frames of ``raw_format``: 'fused' -
    one ``risp_raw_defect`` launch with the gains - or 'pass' - ``risp_raw_defect``, then ``risp_raw_shade`` on its frames.  A
    pure function of its argument: what ``serve`` / ``serve_frame`` do and what ``last_serve_defect`` reports for such a call."""
    F.raw_format_bits(raw_format)
    return 'fused' if raw_format in _DEFECT_SHADE_FUSED else 'pass'


def _sensor_input(raw, lead, h, w, white_level, black_level, cfa, raw_format, lens_shading, defect, temporal, stats, report):
    """The sensor side of ``serve`` and ``serve_frame``, in front of the route or the tiles: contiguous device frames of
    ``lead`` + (H, W) samples, uint16 or MIPI-packed ``raw_format``, and the sensor keywords -> (white level, black level,
    aligned, packed, shade, frames).  The keywords are refused before anything is launched.  Behind a shading the samples have
    black level 0 and the white level white_level - black_level: the two come back so.
    ``frames()`` makes the uint16 frames the route reads, once, in buffers kept per (shape, device, stream): ``risp_raw_defect``
    (shading too, in its own launch or with ``risp_raw_shade`` behind it: ``defect_shade``) | ``risp_raw_shade`` |
    ``risp_raw_unpack``, or the uint16 input as given.  Each launch has a buffer of its own - a caller may hold another one's
    frames, the shade launch behind a correction reads the correction's, and the temporal launch may alias neither its input
    nor the state.  It is lazy: a route whose one launch loads ``packed`` = (uint8 frames, bits, W, raw_format) or applies
    ``shade`` = ((gains, cell), the sensor's black level) itself never calls it.  Both are None where nothing behind the
    pre-pass may see them: a correction or a shade launch decodes, a correction shades, and behind the temporal filter and
    the statistics of a pre-pass nothing is packed or unshaded any more.
    ``temporal`` runs here, once, on ``frames()`` - it advances the state - and ``stats`` behind it, on what the route is about
    to read: the frames of a pre-pass or of the filter, otherwise the input as given, packed or not.
    ``aligned``: whether what the route reads is 8-byte aligned (the cached buffers are).  ``report`` takes 'load', 'shade',
    'defect', 'temporal' and 'stats' where their launches are issued."""
    device, n = raw.device, lead[0] if lead else 1
    bits = F.raw_format_bits(raw_format) or 16
    code = F.cfa_code(cfa)
    _check_black_level(black_level, white_level)
    F._check_mirror(code, h, w)
    pre_shade = None
    if lens_shading is not None:
        if w % 4:
            raise ValueError('lens_shading on frames %d wide: W must be a multiple of 4' % w)
        F.shading_check(lens_shading, h, w, device)
        pre_shade, white_level, black_level = (lens_shading, int(black_level)), white_level - black_level, 0
    if defect is not None:
        F.defect_check(defect, h, w, device)
    if temporal is not None:                                # an unprimed state under capture is refused too
        temporal = F.temporal_check(temporal, n, h, w, device)
        F._temporal_prime(temporal[0], torch.cuda.is_current_stream_capturing())
    if stats is not None:
        F.stats_check(stats, n, h, w, device)
    made = []

    def buffer(tag):
        return F._scene_buffer(device, tag, lead + (h, w), torch.uint16)

    def make():
        if bits != 16:
            report['load'] = 'pass'                         # whichever launch comes first decodes on the way
        if defect is not None:
            if pre_shade is None:
                report['defect'] = 'pass'
                return F.raw_defect(raw, defect, bits, w, out=buffer('defect_u16'))
            report['defect'], report['shade'] = defect_shade(raw_format), 'pass'
            if report['defect'] == 'fused':
                return F.raw_defect(raw, defect, bits, w, pre_shade[0], pre_shade[1], buffer('defect_u16'))
            return F.raw_shade(F.raw_defect(raw, defect, bits, w, out=buffer('defect_u16')), pre_shade[0], pre_shade[1], 16, w,
                               buffer('shaded_u16'))
        if pre_shade is not None:
            report['shade'] = 'pass'
            return F.raw_shade(raw, pre_shade[0], pre_shade[1], bits, w, buffer('shaded_u16'))
        return raw if bits == 16 else F.raw_unpack(raw, bits, w, buffer('raw_u16'))

    def frames():
        if not made:
            made.append(make())
        return made[0]
    prepass = defect is not None or pre_shade is not None
    packed = (raw, bits, w, raw_format) if bits != 16 and not prepass else None
    shade = pre_shade if defect is None else None
    aligned = prepass or packed is not None or raw.data_ptr() % 8 == 0
    if temporal is not None:
        made[:] = [F.raw_temporal(frames(), temporal, black_level, buffer('temporal_u16'))]
        report['temporal'] = 'pass'
        packed, shade, aligned = None, None, True
    if stats is not None:
        if prepass or temporal is not None:
            shade = None
            F.raw_stats(frames(), stats, black_level, 16, w)
        else:
            F.raw_stats(raw, stats, black_level, bits, w)
        report['stats'] = 'pass'
    return white_level, black_level, aligned, packed, shade, frames


def temporal_plan(raw, raw_format, raw_width, dims, temporal_denoise):
    """``F.temporal_check`` of ``temporal_denoise`` from the frames as given - uint16 or packed, of ``dims`` dimensions, one image
    for an (H,W) frame -, nothing for None: what ``serve_frame`` and the modules' ``serve`` check before their first launch"""
    if temporal_denoise is None:
        return None
    lead, h, w = _frame_shape(raw, raw_format, raw_width, dims)
    checked = F.temporal_check(temporal_denoise, lead[0] if lead else 1, h, w, raw.device)
    F._temporal_prime(checked[0], torch.cuda.is_current_stream_capturing())     # an unprimed state under capture is refused here
    return checked


# output formats a resized call stores from the resize launch itself (risp_bgr8_resize with the matrix) instead of resizing to
# packed BGR and converting that with risp_bgr8_to_nv12.  'nv12' is listed only if the fused store beats the two launches by
# more than the larger spread of the two legs in every measured row of profiles/serve_resize.txt (two sizes, triangle and
# bicubic) - the rule of every measured table here, tools/serve_bench.beats.  The verdict line of that file is this
# table.  Measured: at 64 x 256 x 256 -> 128 x 128 the fused store is 6.4 us (triangle) and 4.3 us (bicubic) faster, far beyond
# the spread; on the 3000 x 4000 frame -> 1080 x 1920 it is 0.5 us faster against a spread of 0.4 us (triangle) and 1.4 us SLOWER
# (bicubic) - the NV12 store keeps half the threads of phase 2 idle, and the conversion launch costs 4 us there.  Three rows of
# four, and the rule asks for all, so the table is empty and serve takes the two launches.  Both
# forms stay reachable through functional.bgr8_resize.
_RESIZE_NV12_FUSED = frozenset()


def resize_store(out_format):
    """Who stores the image of a call with ``out_size`` / ``out_window``: None for ``out_format='bgr8'`` (the resize launch
    stores packed bytes); for 'nv12' 'fused' - ``risp_bgr8_resize`` stores NV12 itself - or 'pass' - it stores packed BGR into a
    cached image and ``risp_bgr8_to_nv12`` follows.  A pure function of its argument: what ``serve`` / ``serve_frame`` do, and
    ``last_serve_store`` reports 'resize' for 'fused' and 'pass' for 'pass'."""
    if out_format == 'bgr8':
        return None
    if out_format != 'nv12':
        raise ValueError("unknown out_format %r: 'bgr8' or 'nv12'" % (out_format,))
    return 'fused' if out_format in _RESIZE_NV12_FUSED else 'pass'


# warp kernels whose launch stages the source box of a tile in LDS (risp_bgr8_warp with stage = 1) instead of sampling global
# memory from every tile (stage = 0).  A kernel is listed only if stage = 1 beats stage = 0 by more than the larger spread of the
# two legs in every measured row of that kernel in profiles/serve_warp.txt (two sizes x identity, a 2-degree rotation and a radial
# correction) - the rule of every measured table here, tools/serve_bench.beats.  The verdict line
# of that file is this table.  Measured: staging LOSES in all twelve rows - 3000 x 4000 bilinear 284-292 us against 58-68 us, bicubic
# 336-344 against 180-215; 64 x 256 x 256 97-99 against 23-25 and 115-118 against 66-78, spreads under 8 us: a launch that asks for 64 KB
# of LDS keeps two workgroups on a CU, and a tile's chain of loads, barriers, taps and stores has nothing to hide behind.  So the
# table is empty and serve gathers.  Both forms are the same integer function and stay reachable through
# functional.bgr8_warp(stage=).
_WARP_STAGED = frozenset()


def warp_stage(kernel):
    """How the warp launch of ``serve`` / ``serve_frame`` (and ``functional.bgr8_warp`` with ``stage=None``) reads its source:
    'lds' - a workgroup stages its tile's source box in LDS where it fits - or 'gather' - every tile samples global memory.  A
    pure function of the kernel's name ('bilinear' | 'bicubic'); the bytes are the same either way."""
    if kernel not in F.WARP_KERNELS:
        raise ValueError('unknown warp kernel %r: one of %s' % (kernel, ', '.join(F.WARP_KERNELS)))
    return 'lds' if kernel in _WARP_STAGED else 'gather'


# output formats a sharpened call stores from the sharpen launch itself (risp_bgr8_sharpen with the matrix) instead of sharpening
# to packed BGR and converting that with risp_bgr8_to_nv12.  'nv12' is listed only if the fused store beats the two launches by
# more than the larger spread of the two legs in every measured row of profiles/serve_sharpen.txt (three sizes, both radii;
# DESIGN.md 4.6) - the rule of every measured table here, tools/serve_bench.beats.  The verdict line of that
# file is this table.  Measured: the fused store wins all six rows - 64 x 256 x 256 15.3 / 16.5 us (radius 1 / 2) against 21.9 / 23.0,
# 3000 x 4000 38.1 / 40.7 against 47.8 / 51.2, 1080 x 1920 9.8 / 9.9 against 16.3 / 16.3, spreads of at most 0.7 us: the NV12 store
# reads the sharpened tile from LDS, where the BGR store reads it too, and writes half the bytes, while the conversion launch reads
# the whole image again.  Both forms are the same integer function and stay reachable through functional.bgr8_sharpen.
_SHARPEN_NV12_FUSED = frozenset({'nv12'})


def sharpen_store(out_format):
    """Who stores the image of a call with ``sharpen``: None for ``out_format='bgr8'`` (the sharpen launch stores packed bytes);
    for 'nv12' 'fused' - ``risp_bgr8_sharpen`` stores NV12 itself - or 'pass' - it stores packed BGR into a cached image and
    ``risp_bgr8_to_nv12`` follows.  A pure function of its argument: what ``serve`` / ``serve_frame`` do, and
    ``last_serve_store`` reports 'sharpen' for 'fused' and 'pass' for 'pass'."""
    if out_format == 'bgr8':
        return None
    if out_format != 'nv12':
        raise ValueError("unknown out_format %r: 'bgr8' or 'nv12'" % (out_format,))
    return 'fused' if out_format in _SHARPEN_NV12_FUSED else 'pass'


def _output_plan(h, w, lead, device, sharpen, warp, out_size, out_window, resample, out_format, yuv_matrix, reverse_channels, out):
    """The output side of a call on H x W frames - ``warp`` -> ``out_size`` / ``out_window`` -> ``sharpen`` -> the NV12 store -,
    checked on the host before anything is launched: None without the four keywords, otherwise (steps, the twelve integers of
    an NV12 store or None, the size (FH, FW) of the image as returned, who stores NV12).  A step is (name - 'warp' | 'resize' |
    'sharpen' -, its checked arguments, the size of its input image), in pipeline order: the image size walks from the
    sensor's through the warp's to the resize's.  Who stores: None for 'bgr8', the last step's name where that launch stores
    NV12 itself (``resize_store``, ``sharpen_store``; the warp has no such store), 'pass' where ``risp_bgr8_to_nv12`` follows.
    The stages in front of a sharpen launch are planned for packed BGR; without one the warp is planned for NV12 even where a
    resize follows it.  ``out`` is checked against the final shape with the alignment the storing launch needs; ``lead`` is the
    shape in front of the image's own dimensions"""
    resize = out_size is not None or out_window is not None
    if sharpen is None and warp is None and not resize:
        return None
    nv12 = out_format == 'nv12'
    if sharpen is not None:
        F.sharpen_check(sharpen, nv12)
    steps = []
    if warp is not None:
        size = F.warp_check(warp, h, w, device, nv12 and sharpen is None)[2]
        steps.append(('warp', warp, (h, w)))
        h, w = size
    if resize:
        size, win = F.resize_check(out_size, out_window, resample, h, w, nv12 and sharpen is None)
        steps.append(('resize', (size, win), (h, w)))
        h, w = size
    if sharpen is not None:
        steps.append(('sharpen', F.sharpen_check(sharpen, nv12, h, w), (h, w)))
    coef = _nv12_plan(out_format, yuv_matrix, reverse_channels, h, w)
    last = steps[-1][0]
    fused = coef is not None and last != 'warp' and (resize_store if last == 'resize' else sharpen_store)('nv12') == 'fused'
    store = None if coef is None else (last if fused else 'pass')
    if out is not None:
        F._u8_out(out, tuple(lead) + ((h, w, 3) if coef is None else (h + h // 2, w)), device, 4 if store == 'resize' else 1)
    return steps, coef, (h, w), store


def output_plan(raw, raw_format, raw_width, dims, sharpen, warp, out_size, out_window, resample, out_format, yuv_matrix,
                reverse_channels, out):
    """``_output_plan`` from the frames as given - uint16 or packed, of ``dims`` dimensions -, None without the keywords: what
    ``serve_frame`` and the modules' ``serve`` check before their first launch"""
    if sharpen is None and warp is None and out_size is None and out_window is None:
        return None
    if sharpen is not None:
        F.sharpen_check(sharpen, out_format == 'nv12')
    lead, h, w = _frame_shape(raw, raw_format, raw_width, dims, False)
    return _output_plan(h, w, lead, raw.device, sharpen, warp, out_size, out_window, resample, out_format, yuv_matrix,
                        reverse_channels, out)


def _source_image(name, size, lead, device):
    """the cached packed image of ``size`` the launch ``name`` reads, kept per (shape, device, stream).  Every stage has an image of its
    own, and so has the NV12 conversion ('nv12_bgr'): their shapes can coincide - a warp may keep the sensor's size, a resize
    the warp's -, and a launch must not read the image it writes"""
    return F._scene_buffer(device, name + '_bgr', tuple(lead) + tuple(size) + (3,), torch.uint8)


def _deliver(img, plan, resample, reverse_channels, out, report):
    """The end of a call with an output plan: the packed BGR image served into the first step's source image -> one launch per
    step - ``risp_bgr8_warp`` (``warp_stage`` picks its form), ``risp_bgr8_resize``, ``risp_bgr8_sharpen`` (told the channel
    order) -, each into the next step's source image and the last one into ``out``.  With NV12 the last launch stores NV12
    itself where the plan says so; otherwise it writes the conversion's source image and ``risp_bgr8_to_nv12`` follows.
    ``report`` takes the steps and 'store' as the launches are issued"""
    steps, coef, final, store = plan
    lead, device = tuple(img.shape[:-3]), img.device
    for k, (name, args, _) in enumerate(steps):
        nv12 = None
        if k + 1 < len(steps):
            dst = _source_image(steps[k + 1][0], steps[k + 1][2], lead, device)
        elif coef is None:
            dst = out
        elif store == 'pass':
            dst = _source_image('nv12', final, lead, device)
        else:
            dst, nv12 = out, coef
        if name == 'warp':
            img = F.bgr8_warp(img, args, out=dst)
        elif name == 'resize':
            img = F.bgr8_resize(img, args[0], args[1], resample, nv12, 'bgr', dst)
        else:
            img = F.bgr8_sharpen(img, args, nv12, 'rgb' if reverse_channels else 'bgr', dst)
        report[name] = 'pass'
    report['store'] = store
    return F.bgr8_to_nv12(img, coef, 'bgr', out) if store == 'pass' else img


def stats_plan(raw, raw_format, raw_width, dims, statistics):
    """``F.stats_check`` of ``statistics`` from the frames as given - uint16 or packed, of ``dims`` dimensions, one image for an
    (H,W) frame -, nothing for None: what ``serve_frame`` and the modules' ``serve`` check before their first launch"""
    if statistics is None:
        return None
    if not isinstance(statistics, F.RawStatistics):
        raise ValueError('statistics must be a RawStatistics (functional.raw_statistics builds one), got %s'
                         % (type(statistics).__name__,))
    lead, h, w = _frame_shape(raw, raw_format, raw_width, dims)
    F._need_gpu(raw, 'raw')
    return F.stats_check(statistics, lead[0] if lead else 1, h, w, raw.device)


def serve(modules, param_tensors, raw_u16, white_level, reverse_channels=False, out=None, black_level=0, cfa='rggb',
          fast_scene=False, fast_denoise=False, fast_cond=False, *, sharpen=None, out_format='bgr8', yuv_matrix='bt601_full',
          out_size=None, out_window=None, resample='triangle', raw_format='u16', temporal_denoise=None, statistics=None,
          warp=None, raw_width=None, lens_shading=None, defect_correction=None, fast_median=False, fast_denoise_scene=False):
    """The pipeline as an ISP: (N,H,W) uint16 frames on the device -> ((N,H,W,3) uint8, route taken).  The bytes are
    ``tensor2bgr`` of what ``fused_forward`` gives for ``raw / white_level``, on every route: ``'fused'``
    (``risp_serve_u8[_cfa]``, one launch), ``'classical'`` (``risp_serve_classical_u8``, one launch: ``serve_route``, H even
    and >= 4, W % 4 == 0) or ``'composed'``.

    ``fast_scene=True`` opts in to the ``'scene'`` route where ``scene_plan`` is not None (a pipeline with one or two of
    gray-world, white-world, Reinhard), H is even and >= 4, W % 4 == 0, N <= 65535 and the frames are 8-byte aligned;
    otherwise the call runs exactly as without it.  The scene route reads the mosaic once per scene stage for its
    whole-image statistic and once to serve: 2 S + 1 launches for S scene stages, no fp32 plane written, ``black_level``,
    ``cfa`` and ``reverse_channels`` as on the classical route; with ``out`` given and a warm cache it allocates nothing
    and never waits for the device.  Its contract is weaker than the default's, which is why it is opt-in: a pipeline whose
    only scene stages are white-world has the composed route's bytes (a maximum has no order); gray-world and Reinhard take
    their sums in another order, their constants differ from the composed route's in the last bits, and the bytes agree
    with the float64 reference of tests/serve_scene_reference.py under its tie rule, not with ``torch.equal``.

    ``fast_denoise=True`` opts in to the ``'denoise'`` route (``risp_serve_denoise_u8``, one launch) where ``denoise_plan`` is
    not None - one classical bilateral, median or non-local means anywhere behind a classical demosaic -, the geometry is the
    classical route's and the learned parameters give the sizes every reference configuration below a saturated parameter
    produces (bilateral window 3, median 3, non-local means block 3 and search 3); otherwise the call runs exactly as without
    it.  The bytes are the composed route's (``torch.equal``); the keyword exists because the default call's route is pinned by
    tests.  The denoiser's arguments are derived once per parameter version: with ``out`` given a warm call launches once,
    allocates nothing and never waits for the device.

    ``fast_median=True`` opts a median of every learned size in to the ``'denoise'`` route: OriginNoiseMedian's rule gives
    2 * int(p * 7) + 3 from image 0's parameter, which is 3 only below p = 1/7 and 9 at the initial value, so for most found
    pipelines ``fast_denoise=True`` composes.  Where ``denoise_plan`` is not None, the denoiser is OriginNoiseMedian and the
    geometry is the classical route's, size 3 takes ``risp_serve_denoise_u8`` as under ``fast_denoise`` and a size in
    ``_MEDIAN_SIZES`` with min(H, W) > size // 2 takes ``risp_serve_median_u8`` - one launch, packed 8-bit codes in LDS, the
    composed route's bytes (``torch.equal``); the route reported is ``'denoise'``, the same route at another size.  Anything
    else - size 17 (a saturated parameter), a size measured no faster (profiles/serve_median.txt), every other denoiser, two
    denoisers, scene stages, proxies, other geometry - runs exactly as without the keyword.  The size is derived once per
    parameter version: with ``out`` given a warm call launches once, allocates nothing and never waits for the device.
    ``fast_denoise=True`` keeps its meaning: it alone still composes at size 5.

    ``fast_cond=True`` opts in to the ``'cond'`` route where ``cond_plan`` is not None - one to three conditional heads among
    element-wise stages and Crysis / Filmic curves behind a classical demosaic -, the geometry is the classical route's,
    H * W <= 2^24 and every head has 3 * bins <= 1024 and layer widths within ``risp_cond_fc_fwd``'s limits; otherwise the call
    runs exactly as without it.  Per head the mosaic is read once more: ``risp_serve_cond_hist`` bins the head's input into
    integer counts, ``risp_serve_cond_finish`` runs the head's MLP on them, and ``risp_serve_classical_u8`` serves with every
    head as its element-wise op - 2 S + 1 launches (and S capturable memsets) for S heads, no fp32 plane written.  Counts are
    integers and have no summation order, so the bytes are the composed route's (``torch.equal``); the keyword exists because
    the default call's route is pinned by tests.  The head's flat vector is read by the finish launch on every call: with
    ``out`` given a warm call allocates nothing and never waits for the device.

    ``fast_denoise_scene=True`` opts in to the ``'denoise_scene'`` route where ``denoise_scene_plan`` is not None - one
    classical bilateral, median or non-local means together with one or two of gray-world / white-world, anywhere behind a
    classical demosaic -, the geometry is the classical route's and the learned parameters give the sizes the denoise route
    serves; otherwise the call runs exactly as without it.  Per scene stage the mosaic is read once more for the statistic of
    the stage's input (``risp_serve_scene_stats`` in front of the denoiser, ``risp_serve_denoise_stats`` - the denoise route's
    tile pipeline, reduced instead of stored - behind it) and ``risp_serve_scene_finish`` forms its constants; then
    ``risp_serve_denoise_scene_u8`` serves: 2 S + 1 launches for S scene stages, no fp32 plane written; with ``out`` given and
    a warm cache the call allocates nothing and never waits for the device.  The contract, every part checkable exactly: a
    maximum has no order, so a list whose only scene stages are white-world has the default call's bytes (``torch.equal``);
    gray-world sums in another order than ``risp_channel_stats``, so (a) given the constants, the bytes are those of the
    composed route evaluated with the same constants, and (b) the constants are within the summation bound of the composed
    route's.  Which is why the route is opt-in, as ``fast_scene`` is.  The plan leaves non-local means with a scene stage behind
    it on the default route: there the route runs the denoiser twice and was measured slower at 64 x 256 x 256
    (profiles/serve_denoise_scene.txt).

    ``black_level`` (integer, 0 <= black_level < white_level) and ``cfa`` ('rggb' | 'grbg' | 'gbrg' | 'bggr') describe the
    sensor: the input becomes max(raw - black_level, 0) / (white_level - black_level) and the mosaic of another phase is
    read mirrored - which makes it RGGB for every stage, learned ones included - and the image stored un-mirrored.  No
    extra pass on either route: the kernels mirror their addresses (``risp_serve_u8_cfa``; ``risp_raw_crop_cfa`` and
    ``risp_quantise_u8_flip`` around the unchanged ``fused_forward``).  Byte for byte
    ``unflip(serve(flip(clamp(raw - black_level)), white_level - black_level))``.

    ``out_format='nv12'`` returns YUV 4:2:0 instead: (N,3H/2,W) uint8, H rows of Y and H/2 rows of interleaved U V, converted
    with ``yuv_matrix`` (a key of ``F.NV12_MATRIX`` or twelve integers) - byte for byte ``F.bgr8_to_nv12`` of what the same
    call returns without the keyword.  The route is chosen exactly as without it.  ``'fused'`` and ``'classical'`` store NV12
    from their one launch (``risp_serve_nv12``, ``risp_serve_classical_nv12``); every other route serves into a packed image
    kept per shape, device and stream and ``risp_bgr8_to_nv12`` follows, one launch more.  H and W even;
    ``reverse_channels`` is refused.  With ``out`` given a warm call allocates nothing.

    ``raw_format='raw10'`` / ``'raw12'`` takes MIPI-packed frames as a sensor delivers them: (N,H,stride) uint8, rows of
    ``stride`` bytes that hold ``raw_width`` pixels (None: all they can, ``stride * 8 // bits``) - four pixels in five bytes
    or two in three, include/risp.h has the layout -, padding behind them never read, any start address.  The bytes returned
    are those of the same call on ``F.raw_unpack(frames, bits, raw_width)``, on the route that call takes.  ``'fused'`` and
    ``'classical'`` decode the groups in their one launch where ``serve_load`` says 'fused' (``risp_serve_packed``,
    ``risp_serve_classical_packed``); every other route unpacks once into uint16 frames kept per shape, device and stream
    (``risp_raw_unpack``, one launch more) and runs as for them.  ``white_level`` is not implied by the format.  H even,
    ``raw_width`` a multiple of 4.  With ``out`` given a warm call allocates nothing.  ``raw_format='u16'`` is the call
    without the keyword.

    ``lens_shading=(gains, cell)`` corrects vignetting and colour shading in front of everything else: a contiguous (GH,GW,4)
    uint16 device tensor of Q12 gains on a mesh of ``cell`` pixels (a power of two from 4 to 256; ``F.shading_check``,
    ``F.shading_map`` builds one), per plane 2 * (y & 1) + (x & 1) of the frame as stored, whatever ``cfa`` - include/risp.h has
    the integer definition.  The bytes returned are those of the same call on ``F.raw_shade(frames, lens_shading, black_level)``
    with ``white_level - black_level`` and black level 0, on the route that call takes.  Where ``serve_shade`` says 'fused' the
    classical route shades in its one launch (``risp_serve_classical_shaded``); everywhere else ``risp_raw_shade`` writes the
    shaded frames once into uint16 frames kept per shape, device and stream, one launch more, and with packed input decodes them
    on the way: no ``risp_raw_unpack`` is issued.  The gains are never read on the host.  With ``out`` given a warm call
    allocates nothing and never waits for the device.  None is the call without the keyword.

    ``defect_correction=(threshold, slope, defects)`` replaces hot, dead and factory-listed pixels from their same-colour
    neighbours in front of everything else, the shading included (``F.defect_check``; ``F.defect_map`` builds the bitmap;
    include/risp.h has the integer definition, on the frame as stored, before the black level and whatever ``cfa``).  The
    bytes returned are those of the same call on ``F.raw_defect(frames, defect_correction, bits, raw_width)`` as uint16 input,
    and with ``lens_shading`` on ``F.raw_shade(F.raw_defect(...), lens_shading, black_level)``, on the route that call takes -
    the one uint16 frames from the allocator take.  ``risp_raw_defect`` is one launch in front of the route and decodes packed
    frames on the way: no ``risp_raw_unpack`` is issued and no fused packed or shading load is taken.  With ``lens_shading``
    the same launch shades where ``defect_shade`` says 'fused'; otherwise ``risp_raw_shade`` follows.  The corrected frames
    live in a buffer of their own per shape, device and stream.  H >= 3, W % 4 == 0.  With ``out`` given a warm call allocates
    nothing and never waits for the device.  None is the call without the keyword.

    ``temporal_denoise=(state, strength, threshold, slope, ramp)`` filters the frames over time, the one block with state across
    calls: each sample is blended over ``state.frames`` - the previous filtered frames, an ``F.TemporalState`` built once for
    these N, H, W (``F.temporal_state``) - with a Q8 share that starts at ``strength`` and climbs to 256 where the 5 x 5
    neighbourhood says that something moved (``F.temporal_check``; include/risp.h has the integer definition).  It runs behind
    ``defect_correction`` and ``lens_shading`` (fused into one launch where ``defect_shade`` says so, exactly as without the
    keyword) and in front of ``statistics`` and the route: ``risp_raw_temporal`` - one launch and one device-to-device copy that
    advances the state - reads the pre-pass's frames, or the uint16 input as given, or what ``risp_raw_unpack`` makes of packed
    input, and writes uint16 frames kept per shape, device and stream.  The bytes returned are those of the same call without the
    keyword on ``F.raw_temporal(pre(frames), (a state of equal content, ...), black_level')``, ``pre`` being today's pre-pass or
    the unpack and ``black_level'`` 0 behind a shading, and afterwards ``state.frames`` holds those filtered frames.  Behind
    it nothing sees packed bytes or a shading: no fused packed or shading load is taken, and the route is chosen exactly as
    without the keyword - the one uint16 frames from the allocator take.  A state whose ``.primed`` is False is primed by the
    call: the frames pass and become the state.  That is refused while the stream is capturing; with ``out`` given and a
    primed state a warm call allocates nothing and never waits, so it captures, and the captured copy makes every replay advance
    the state.  H >= 3, W % 4 == 0.  None is the call without the keyword.

    ``out_size=(OH, OW)`` and ``out_window=(y0, x0, h, w)`` deliver a scaled, cropped image: the window of the image as returned
    (default: all of it) resampled to ``out_size`` (default: the window's size, a crop) with ``resample`` 'box', 'triangle' or
    'bicubic' (``F.resize_check``; include/risp.h has the integer definition).  The route is chosen exactly as without the
    keywords, and so is every ``fast_*``, load, shade and defect choice; it serves packed BGR (``reverse_channels`` honoured
    there) into an image kept per shape, device and stream, and ONE ``risp_bgr8_resize`` launch writes ``out`` (N,OH,OW,3): the
    bytes of ``F.bgr8_resize`` of the call without the keywords.  With ``out_format='nv12'`` the routes that own a fused NV12
    store serve BGR too; the resize launch stores (N,3*OH/2,OW) NV12 itself where ``resize_store('nv12')`` says 'fused'
    (``out`` 4-byte aligned), otherwise ``risp_bgr8_to_nv12`` follows it; OH and OW even.  The tap tables live on the device per
    axis geometry and kernel: with ``out`` given a warm call uploads and allocates nothing and never waits.  Bad sizes, a window
    outside the image, an unknown kernel, more than 32 taps on an axis, odd OH / OW with NV12 and a wrong ``out`` are refused
    before anything is launched.  With both None the call is today's call, launch for launch, and ``resample`` is not read.

    ``statistics=st`` (an ``F.RawStatistics`` built once for these N, H, W: ``F.raw_statistics``) also fills ``st.zones`` and
    ``st.hist`` with the 3A statistics of the samples the route demosaics - per zone and Bayer plane of the frame as stored the
    sum and the count of the samples in lo .. hi and the horizontal focus measure, per image and plane a histogram
    (include/risp.h has the integer definition; ``F.stats_planes(cfa)`` names the planes).  ``st`` is checked before anything is
    launched; then ``risp_raw_stats`` - a memset and one launch - reads what the route is about to read: with
    ``defect_correction`` and / or ``lens_shading`` the cached corrected uint16 frames (black level 0 behind a shading),
    otherwise the input as given, packed or not, with ``black_level``.  With ``lens_shading`` the shade launch runs: no fused
    shading load is taken, as under ``defect_correction``.  Everything else about the route is chosen exactly as without the
    keyword and the image bytes are the same.  H even, W % 4 == 0.  With ``out`` given a warm call allocates nothing and never
    waits for the device; a captured call zeroes ``st`` on every replay.  None is today's call, launch for launch.

    ``warp=(mesh, cell, (WH, WW), kernel)`` delivers a geometry-corrected image (N,WH,WW,3) - lens distortion, rotation, flips,
    keystone, stabilisation: output pixel (y,x) is sampled at the Q8 source coordinate interpolated from the (MH,MW,2) int32
    ``mesh`` of ``cell``-pixel cells, with 'bilinear' or 'bicubic' taps and a replicate border (``F.warp_check``;
    ``F.warp_mesh`` / ``F.warp_homography`` / ``F.warp_radial`` build meshes; include/risp.h has the integer definition).  The
    route is chosen exactly as without the keyword, and so is every ``fast_*``, load, shade, defect and statistics choice -
    statistics describe the sensor frame and do not change; it serves packed BGR at the sensor's size (``reverse_channels``
    honoured there) into an image of its own kept per shape, device and stream, and ONE ``risp_bgr8_warp`` launch
    (``warp_stage(kernel)`` picks its form) writes the warped image into ``out``, into the resize's source image when
    ``out_size`` / ``out_window`` are given - they and ``resample`` then mean what they mean above, applied to the warped image
    of WH x WW -, or into the NV12 conversion's source image with ``out_format='nv12'`` (the routes that own a fused NV12 store
    serve BGR too; WH and WW even, OH and OW too when resizing).  Byte for byte
    ``nv12?(F.bgr8_resize?(F.bgr8_warp(serve(.. without warp, the resize keywords and out_format ..), warp), ..))``.  The warp
    and ``out`` are checked before anything is launched; with ``out`` given a warm call allocates nothing and never waits.
    None is today's call, launch for launch.

    ``sharpen=(amount, threshold, limit, radius)`` sharpens the image as returned - the edge-enhancement block between the
    scaler and the YUV output: an unsharp mask of the 8-bit luma with a binomial blur of ``radius`` 1 or 2, the detail cored
    softly by ``threshold`` codes, multiplied by ``amount`` / 256 (0 .. 4095), bounded by ``limit`` codes and added to B, G and R
    alike (``F.sharpen_check``; include/risp.h has the integer definition).  The route is chosen exactly as without the keyword,
    and so is every other choice; statistics and the temporal state do not change.  Whatever stage precedes the sharpening - the
    route, the warp launch or the resize launch - stores packed BGR (``reverse_channels`` honoured there; the routes that own a
    fused NV12 store serve BGR too) into an image of its own kept per shape, device and stream, and ONE ``risp_bgr8_sharpen``
    launch, told the channel order, writes ``out``; with ``out_format='nv12'`` it stores NV12 itself where
    ``sharpen_store('nv12')`` says 'fused' and writes the conversion's source image for ``risp_bgr8_to_nv12`` otherwise.  Byte
    for byte ``nv12?(F.bgr8_sharpen(F.bgr8_resize?(F.bgr8_warp?(serve(.. without these keywords ..)))))``.  The tuple, odd sizes
    with NV12 and ``out`` are refused before anything is launched; with ``out`` given a warm call allocates nothing and never
    waits.  None is today's call, launch for launch.

    ``sharpen``, ``out_format``, ``yuv_matrix``, ``out_size``, ``out_window``, ``resample``, ``raw_format``, ``temporal_denoise``, ``statistics``, ``warp``, ``raw_width``, ``lens_shading``, ``defect_correction`` and ``fast_median`` are keyword-only, and so is
    ``fast_denoise_scene``: it stays the last parameter (tests/test_serve_denoise_scene_plan_cpu.py holds every ``serve`` to that), the positional list in
    front of it is unchanged."""
    img, report = serve_reported(modules, param_tensors, raw_u16, white_level, reverse_channels, out, black_level, cfa, fast_scene,
                                 fast_denoise, fast_cond, sharpen=sharpen, out_format=out_format, yuv_matrix=yuv_matrix,
                                 out_size=out_size, out_window=out_window, resample=resample, raw_format=raw_format,
                                 temporal_denoise=temporal_denoise, statistics=statistics, warp=warp, raw_width=raw_width,
                                 lens_shading=lens_shading, defect_correction=defect_correction, fast_median=fast_median,
                                 fast_denoise_scene=fast_denoise_scene)
    return img, report['route']


# what a serving call records about itself, the values ``_FixedPipeline.last_serve_*`` documents: 'route' is a name of
# SERVE_ROUTES; every other entry is None where its keyword is not given, and otherwise says which launch did the work
SERVE_REPORT = ('route', 'load', 'shade', 'defect', 'temporal', 'stats', 'warp', 'resize', 'sharpen', 'store')


def serve_reported(modules, param_tensors, raw_u16, white_level, reverse_channels=False, out=None, black_level=0, cfa='rggb',
                   fast_scene=False, fast_denoise=False, fast_cond=False, *, sharpen=None, out_format='bgr8',
                   yuv_matrix='bt601_full', out_size=None, out_window=None, resample='triangle', raw_format='u16',
                   temporal_denoise=None, statistics=None, warp=None, raw_width=None, lens_shading=None, defect_correction=None,
                   fast_median=False, fast_denoise_scene=False):
    """``serve`` with the record of what ran in place of the route: (image, report), a dict with the keys of ``SERVE_REPORT``,
    each entry written where the launch that justifies it is issued"""
    report = dict.fromkeys(SERVE_REPORT)
    lead, h, w = _device_frames(raw_u16, raw_format, raw_width, (3,))
    device = raw_u16.device
    plan = _output_plan(h, w, lead, device, sharpen, warp, out_size, out_window, resample, out_format, yuv_matrix, reverse_channels,
                        out)                                # refused before anything is launched
    coef, dst = None, out
    if plan is not None:
        # the route serves packed BGR at the sensor's size into the source image of the first launch behind it
        dst = _source_image(plan[0][0][0], (h, w), lead, device)
    else:
        coef = _nv12_plan(out_format, yuv_matrix, reverse_channels, h, w)
        if coef is not None and out is not None:
            F._u8_out(out, lead + (h + h // 2, w), device, 1)           # refused before anything is launched
    img, report['route'] = _serve_routes(modules, param_tensors, raw_u16.contiguous(), lead, h, w, white_level, black_level, cfa,
                                         raw_format, lens_shading, defect_correction, temporal_denoise, statistics,
                                         reverse_channels, dst, coef, fast_scene, fast_denoise, fast_median, fast_denoise_scene,
                                         fast_cond, report)
    if plan is not None:
        img = _deliver(img, plan, resample, reverse_channels, out, report)
    elif coef is not None and report['store'] is None:
        img, report['store'] = F.bgr8_to_nv12(img, coef, 'bgr', out), 'pass'
    return img, report


def _serve_routes(modules, param_tensors, raw, lead, h, w, white_level, black_level, cfa, raw_format, lens_shading, defect, temporal,
                  stats, reverse_channels, out, coef, fast_scene, fast_denoise, fast_median, fast_denoise_scene, fast_cond, report):
    """``serve`` behind the checks of its output side: the sensor pre-pass (``_sensor_input``), the route and its launches ->
    (image, route).  The route is the one uint16 frames from the allocator take, whatever the pre-pass did.  'fused' and
    'classical' load ``packed`` bytes where ``serve_load`` says so, 'classical' shades in its load where ``serve_shade`` says so
    (uint16 input, 8-byte aligned), and every other launch reads ``frames()``.  With ``coef`` (NV12, ``out`` being the NV12
    buffer): 'fused' and 'classical' store NV12 into ``out`` themselves and report it, every other route serves BGR into the
    cached packed image for the conversion launch.  ``report`` takes 'load', 'shade' and 'store' where a launch fuses them"""
    n, device = lead[0], raw.device
    white_level, black_level, aligned, packed, shade, frames = _sensor_input(
        raw, lead, h, w, white_level, black_level, cfa, raw_format, lens_shading, defect, temporal, stats, report)
    divisor = white_level - black_level
    code = F.cfa_code(cfa)
    # where a route without the NV12 store writes its packed image
    dst = (lambda: out) if coef is None else (lambda: _source_image('nv12', (h, w), lead, device))
    geometry = h % 2 == 0 and h >= 4 and w % 4 == 0 and n <= 65535 and aligned      # what the classical kernels take
    if fast_scene and geometry:
        plan = scene_plan(modules)
        if plan is not None:
            return _serve_scene(plan, modules, param_tensors, frames(), divisor, reverse_channels, dst(), black_level, cfa), 'scene'
    if fast_denoise and geometry:
        plan = denoise_plan(modules)
        args = _denoise_args(modules[plan[2]], param_tensors[plan[2]]) if plan is not None else None
        if args is not None:
            pre_ops, pre_params = _stage_lists(modules, param_tensors, plan[1])
            post_ops, post_params = _stage_lists(modules, param_tensors, plan[3])
            return F.serve_denoise_u8(frames(), divisor, plan[0], pre_ops, pre_params, args[0], args[1], post_ops, post_params,
                                      reverse_channels, dst(), black_level, cfa), 'denoise'
    if fast_median and geometry:
        plan = denoise_plan(modules)
        if plan is not None and type(modules[plan[2]]) is T.OriginNoiseMedian:
            size = _median_args(modules[plan[2]], param_tensors[plan[2]])
            if size == 3 or (size in _MEDIAN_SIZES and min(h, w) > size // 2):
                pre_ops, pre_params = _stage_lists(modules, param_tensors, plan[1])
                post_ops, post_params = _stage_lists(modules, param_tensors, plan[3])
                if size == 3:
                    return F.serve_denoise_u8(frames(), divisor, plan[0], pre_ops, pre_params, 'median', (3,), post_ops, post_params,
                                              reverse_channels, dst(), black_level, cfa), 'denoise'
                return F.serve_median_u8(frames(), divisor, plan[0], pre_ops, pre_params, size, post_ops, post_params,
                                         reverse_channels, dst(), black_level, cfa), 'denoise'
    if fast_denoise_scene and geometry:
        plan = denoise_scene_plan(modules)
        args = _denoise_args(modules[plan[2]], param_tensors[plan[2]]) if plan is not None else None
        if args is not None:
            return _serve_denoise_scene(plan, args, modules, param_tensors, frames(), divisor, reverse_channels, dst(), black_level,
                                        cfa), 'denoise_scene'
    if fast_cond and geometry and h * w <= 1 << 24:
        plan = cond_plan(modules)
        if plan is not None and _cond_heads_ok(plan, modules, param_tensors):
            return _serve_cond(plan, modules, param_tensors, frames(), divisor, reverse_channels, dst(), black_level, cfa), 'cond'
    split = _serve_split(modules)
    if split is not None and h % 2 == 0 and w % 4 == 0 and n <= 65535 and aligned:
        bil, chain = split
        # (the bilateral joins a launch under fused_forward's own conditions, so both routes run the same kernel arithmetic)
        args = _bilateral_args(modules[bil], param_tensors[bil]) if bil is not None else None
        if args is None or (args[3] <= 3 and min(h, w) > 8):
            ops = [_CHAIN_OP[type(modules[k])] for k in chain]
            params = [_chain_param(modules[k], param_tensors[k]) for k in chain]
            if coef is not None:
                report['store'] = 'fused'
            if packed is not None and serve_load('fused', packed[3]) == 'fused':
                report['load'] = 'fused'
                return F.serve_packed(packed[0], packed[1], w, divisor, ops, params, args, reverse_channels, coef, out, black_level,
                                      cfa), 'fused'
            if coef is not None:
                return F.serve_nv12(frames(), divisor, ops, params, args, coef, out, black_level, cfa), 'fused'
            return F.serve_u8(frames(), divisor, ops, params, args, reverse_channels, out, black_level, cfa), 'fused'
    if serve_route(modules) == 'classical' and geometry:
        kind, stages = _classical_split(modules)
        ops, params = _stage_lists(modules, param_tensors, stages)
        if coef is not None:
            report['store'] = 'fused'
        if shade is not None and raw_format == 'u16' and serve_shade('classical', 'u16') == 'fused' and raw.data_ptr() % 8 == 0:
            report['shade'] = 'fused'
            return F.serve_classical_shaded(raw, shade[0], divisor, kind, ops, params, reverse_channels, coef, out, shade[1],
                                            cfa), 'classical'
        if packed is not None and serve_load('classical', packed[3]) == 'fused':
            report['load'] = 'fused'
            return F.serve_classical_packed(packed[0], packed[1], w, divisor, kind, ops, params, reverse_channels, coef, out,
                                            black_level, cfa), 'classical'
        if coef is not None:
            return F.serve_classical_nv12(frames(), divisor, kind, ops, params, coef, out, black_level, cfa), 'classical'
        return F.serve_classical_u8(frames(), divisor, kind, ops, params, reverse_channels, out, black_level, cfa), 'classical'
    from ...data.gpu_input import raw_crops
    sel = torch.zeros((n, 3), device=device, dtype=torch.int32)
    sel[:, 0] = torch.arange(n, device=device, dtype=torch.int32)
    x = raw_crops(frames(), sel, (h, w), white_level, black_level, cfa)
    if h % 2 == 0 and w % 2 == 0:
        x, _ = fused_forward(modules, param_tensors, x)
    else:
        for mod, par in zip(modules, param_tensors):
            x = mod(x, par)
    return F.quantise_u8(x, reverse_channels, dst(), code), 'composed'


_FRAME_GEOMETRY = {}


def _pair(v):
    return tuple(int(k) for k in v) if hasattr(v, '__len__') else (int(v), int(v))


def frame_geometry(H, W, size, stride, cfa, device):
    """(tile origins (T,2), ``sel`` rows (T,3)) of ``util_path_restore.frame_tile_sel`` as int32 tensors on ``device``, kept
    per (H, W, size, stride, cfa, device): a warm ``serve_frame`` call uploads nothing."""
    from ...utils.util_path_restore import frame_tile_sel
    device = torch.device(device)
    key = (int(H), int(W), _pair(size), _pair(stride), F.cfa_code(cfa), device.type, device.index)
    hit = _FRAME_GEOMETRY.get(key)
    if hit is None:
        origins, sel = frame_tile_sel(key[0], key[1], key[2], key[3], cfa)
        hit = _FRAME_GEOMETRY[key] = (torch.from_numpy(origins).to(device), torch.from_numpy(sel).to(device))
    return hit


def serve_frame(modules, param_tensors, raw_u16, white_level, patch_size, patch_stride, tile_batch=16, reverse_channels=False,
                out=None, black_level=0, cfa='rggb', out_format='bgr8', yuv_matrix='bt601_full', sharpen=None, *, out_size=None,
                out_window=None, resample='triangle', raw_format='u16', temporal_denoise=None, statistics=None, warp=None,
                raw_width=None, defect_correction=None, lens_shading=None):
    """A full sensor frame through the pipeline in overlapped tiles, the serving form of ``test_split.run_frame``: (H,W) or
    (N,H,W) uint16 mosaic on the device -> (H,W,3) or (N,H,W,3) uint8.  Per frame ONE ``raw_crops`` launch cuts the
    (T,1,h,w) tile stack out of the mosaic (``util_path_restore.frame_tile_sel``: pedestal in integers, divisor
    white_level - black_level, the windows of another phase read mirrored, which makes every tile RGGB), ``fused_forward``
    runs on slices of ``tile_batch`` tiles, each writing its last stage into its rows of one (T,3,h,w) stack
    (``final_out``), and ``risp_tile_blend_u8`` blends the stack straight into the packed image, stored un-mirrored.  No
    fp32 frame exists at either end.  The bytes are those ``test_split.py`` writes for ``raw / white_level`` (``run_frame``,
    then clip, x 255, truncate), and for a sensor byte for byte
    ``unflip(serve_frame(flip(clamp(raw - black_level)), white_level - black_level, ...))``.

    ``param_tensors``: the per-stage blocks of ``min(tile_batch, T)`` images, or a callable that returns them for a number
    of images (a shorter last slice takes the first rows of its blocks).
    ``out_format='nv12'`` returns (3H/2,W) or (N,3H/2,W) YUV 4:2:0 as ``serve`` does: ``risp_tile_blend_u8`` blends each frame
    into a packed image kept per shape, device and stream and ``risp_bgr8_to_nv12`` converts it with ``yuv_matrix``.
    ``raw_format='raw10'`` / ``'raw12'`` (keyword-only, with ``raw_width``) takes (H,stride) or (N,H,stride) uint8 MIPI-packed
    frames as ``serve`` does: ``risp_raw_unpack`` writes them into uint16 frames kept per shape, device and stream, one launch
    in front of everything else (``raw_crops`` has no packed load).
    ``lens_shading=(gains, cell)`` (keyword-only, as in ``serve``) shades the whole frame once in front of ``raw_crops``:
    ``risp_raw_shade`` writes uint16 frames kept per shape, device and stream - from packed frames too, in place of the unpack
    launch - and everything behind it runs with ``white_level - black_level`` and black level 0.
    ``defect_correction=(threshold, slope, defects)`` (keyword-only, as in ``serve``) corrects the whole frame once in front of
    everything else: ``risp_raw_defect`` writes uint16 frames kept per shape, device and stream - from packed frames too, in
    place of the unpack launch; with ``lens_shading`` it shades in the same launch where ``defect_shade`` says 'fused', and
    ``risp_raw_shade`` follows otherwise.
    ``temporal_denoise=(state, strength, threshold, slope, ramp)`` (keyword-only, as in ``serve``; an ``F.TemporalState`` for N
    frames, N = 1 for an (H,W) frame) filters the whole frame once in front of the tiles and of the statistics, behind the
    pre-passes above: ``risp_raw_temporal`` - one launch and the copy that advances the state - writes uint16 frames kept per
    shape, device and stream; packed frames without a pre-pass are unpacked first.  Checked before anything is launched.
    ``out_size``, ``out_window`` and ``resample`` (keyword-only, as in ``serve``) deliver a scaled, cropped image: every frame
    is blended into a packed sensor-size image kept per shape, device and stream (``reverse_channels`` honoured there) and ONE
    ``risp_bgr8_resize`` launch behind the last frame writes ``out``: (OH,OW,3) or (N,OH,OW,3), with ``out_format='nv12'``
    (3*OH/2,OW) or (N,3*OH/2,OW) - stored by that launch where ``resize_store('nv12')`` says 'fused', by ``risp_bgr8_to_nv12``
    behind it otherwise.  Their refusals come before anything is launched.  With both None nothing changes.
    ``statistics=st`` (keyword-only, as in ``serve``; an ``F.RawStatistics`` for N frames, N = 1 for an (H,W) frame) fills ``st``
    with the 3A statistics of the whole frames the tiles are cut from: ``risp_raw_stats`` runs once, on the frames of the
    pre-pass where ``defect_correction`` or ``lens_shading`` is given (black level 0 behind a shading), otherwise on the input
    as given, packed or not, with ``black_level``.  ``st`` is checked before anything is launched; the image is unchanged.
    ``warp=(mesh, cell, (WH, WW), kernel)`` (keyword-only, as in ``serve``) delivers a geometry-corrected image: every frame is
    blended into a packed sensor-size image of the warp's own (``reverse_channels`` honoured there) and ONE ``risp_bgr8_warp``
    launch behind the last frame writes (WH,WW,3) or (N,WH,WW,3) into ``out`` - or into the source image of the resize launch
    (``out_size`` / ``out_window``, then applied to the warped image) or of the NV12 conversion that follows it.  Its refusals
    come before anything is launched; statistics are unchanged.  None changes nothing.
    ``sharpen=(amount, threshold, limit, radius)`` (as in ``serve``; it stands in front of the ``*`` but is meant to be passed by
    name) sharpens the image as returned: every frame is blended at the sensor's size into a cached packed image, the warp and
    the resize launch follow where asked for, and ONE ``risp_bgr8_sharpen`` launch behind them writes ``out`` - or, with
    ``out_format='nv12'``, NV12 itself or the source image of ``risp_bgr8_to_nv12`` (``sharpen_store``).  Its refusals come before
    anything is launched; statistics and the temporal state are unchanged.  None changes nothing.
    ``patch_size`` / ``patch_stride``: an int or a (rows, columns) pair; H, W, sizes and strides even.  Everything is issued
    on the current stream; the tile origins live on the device per geometry (``frame_geometry``).  Argument checks are those
    of ``serve``."""
    return serve_frame_reported(modules, param_tensors, raw_u16, white_level, patch_size, patch_stride, tile_batch, reverse_channels,
                                out, black_level, cfa, out_format, yuv_matrix, sharpen, out_size=out_size, out_window=out_window,
                                resample=resample, raw_format=raw_format, temporal_denoise=temporal_denoise, statistics=statistics,
                                warp=warp, raw_width=raw_width, defect_correction=defect_correction, lens_shading=lens_shading)[0]


def serve_frame_reported(modules, param_tensors, raw_u16, white_level, patch_size, patch_stride, tile_batch=16,
                         reverse_channels=False, out=None, black_level=0, cfa='rggb', out_format='bgr8', yuv_matrix='bt601_full',
                         sharpen=None, *, out_size=None, out_window=None, resample='triangle', raw_format='u16',
                         temporal_denoise=None, statistics=None, warp=None, raw_width=None, defect_correction=None,
                         lens_shading=None):
    """``serve_frame`` with the record of what ran: (image, report), a dict with the keys of ``SERVE_REPORT`` as
    ``serve_reported`` fills it, the route being 'tiled'"""
    from ...data.gpu_input import raw_crops
    report = dict.fromkeys(SERVE_REPORT)
    plan = output_plan(raw_u16, raw_format, raw_width, (2, 3), sharpen, warp, out_size, out_window, resample, out_format,
                       yuv_matrix, reverse_channels, out)   # refused before anything is launched
    if statistics is not None:                              # likewise
        stats_plan(raw_u16, raw_format, raw_width, (2, 3), statistics)
        _check_black_level(black_level, white_level)
    if temporal_denoise is not None:                        # likewise
        temporal_plan(raw_u16, raw_format, raw_width, (2, 3), temporal_denoise)
        _check_black_level(black_level, white_level)
    if lens_shading is not None or defect_correction is not None:
        # what the host can tell about a pre-pass is named before a missing device: the frames, then the correction's tuple
        if raw_format == 'u16' and (not isinstance(raw_u16, torch.Tensor) or raw_u16.dtype != torch.uint16
                                    or raw_u16.dim() not in (2, 3) or raw_u16.shape[-1] % 4):
            raise ValueError('%s takes (H,W) or (N,H,W) uint16 frames with W a multiple of 4, got %s %s'
                             % ('lens_shading' if lens_shading is not None else 'defect_correction',
                                getattr(raw_u16, 'dtype', type(raw_u16)), tuple(getattr(raw_u16, 'shape', ()))))
        if defect_correction is not None:
            F.defect_check(defect_correction, *_frame_shape(raw_u16, raw_format, raw_width, (2, 3))[1:])
    lead, H, W = _device_frames(raw_u16, raw_format, raw_width, (2, 3))
    device, single = raw_u16.device, not lead
    # defect (+ shade) | shade | unpack -> temporal -> statistics, once for the whole frames, in front of the tiles
    white_level, black_level, _, _, _, frames = _sensor_input(raw_u16.contiguous(), lead, H, W, white_level, black_level, cfa,
                                                              raw_format, lens_shading, defect_correction, temporal_denoise,
                                                              statistics, report)
    frames = frames()[None] if single else frames()
    if int(tile_batch) < 1:
        raise ValueError('tile_batch %r: at least one tile per forward' % (tile_batch,))
    n, code = frames.shape[0], F.cfa_code(cfa)
    size, stride = _pair(patch_size), _pair(patch_stride)
    origins, sel = frame_geometry(H, W, size, stride, cfa, device)
    count, tile_batch = origins.shape[0], int(tile_batch)
    final, coef = out, None
    if plan is not None:
        # every frame is blended at the sensor's size into the source image of the first launch behind the loop
        out = _source_image(plan[0][0][0], (H, W), lead, device)
    else:
        coef = _nv12_plan(out_format, yuv_matrix, reverse_channels, H, W)
        out = F._u8_out(out, lead + ((H, W, 3) if coef is None else (H + H // 2, W)), device, 1)
        if coef is not None:
            bgr, report['store'] = _source_image('nv12', (H, W), (), device), 'pass'    # converted frame by frame behind the blend
    stack = torch.empty((count, 3) + size, device=device, dtype=torch.float32)
    if callable(param_tensors):
        param_tensors = param_tensors(min(tile_batch, count))
    with torch.no_grad():
        for k in range(n):
            tiles = raw_crops(frames[k:k + 1], sel, size, white_level, black_level, cfa)
            for at in range(0, count, tile_batch):
                chunk, dest = tiles[at:at + tile_batch], stack[at:at + tile_batch]
                m = chunk.shape[0]
                pars = [p[:m] if p is not None and p.dim() == 2 and p.shape[0] > m else p for p in param_tensors]
                y, _ = fused_forward(modules, pars, chunk, dest)
                if y.data_ptr() != dest.data_ptr():
                    dest.copy_(y)
            if coef is None:
                F.tile_blend_u8(stack, origins, (H, W), stride, reverse_channels, out if single else out[k], code)
            else:
                F.tile_blend_u8(stack, origins, (H, W), stride, False, bgr, code)
                F.bgr8_to_nv12(bgr, coef, 'bgr', out if single else out[k])
    report['route'] = 'tiled'
    if plan is not None:
        out = _deliver(out, plan, resample, reverse_channels, final, report)
    return out, report


def wants_grad(x, raw_params):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in raw_params))
