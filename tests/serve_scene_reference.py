"""Float64 statement of the scene route of the serving path (risp_serve_scene_stats / _finish / _u8): the pipeline of
tests/serve_reference.py with the three stages that need a whole-image quantity first.  It imports that file and restates
only its stage loop; every piece (normalise, the demosaics, code, elementwise, tone_raw, final_convert, check) is that
file's, with the same pins and tie bookkeeping.

Stage codes of THIS file (a pipeline's stages, not the C ABI's op codes): GRAYWORLD (no block), WHITEWORLD ((N,1): ratio),
REINHARD ((N,2): white_point, middle_grey), beside the OP_* of serve_reference.

OPSPEC restated (oracle/isp_oracle.py grayworld, origin_whiteworld, origin_tonemap 'reinhard'); x is the stage input in [0,1]:
  * gray-world: m_c = mean x_c, gray = (m_b + m_g + m_r) / 3, y_c = clamp(x_c * gray / max(m_c, 1e-6), 0, 1).  Leaves a
    clamped float: final kind 'final/grayworld', pins as Gain3;
  * white-world: mx_c = max(255 max x_c, 1e-3), big = max_c mx_c, y_c = code(255 x_c (1 + ratio (big / mx_c - 1))) / 255: a
    quantisation point of kind 'whiteworld';
  * Reinhard: v = max(x, 0), L = 0.114 v_b + 0.587 v_g + 0.299 v_r, lavg = exp(mean log(L + 1e-4)),
    ls = max(middle_grey, 0.01) L / lavg, lw = 10 max(white_point, 0.01),
    y = code(255 v ls (1 + ls / lw^2) / (1 + ls) / max(L, 1e-6)) / 255: a quantisation point of kind 'reinhard'.
Statistics are taken in float64 over the stage input.  ``dtype=numpy.float32`` evaluates the same expressions in float32,
statistics included (numpy.sum on float32; exp as exp2(x log2 e), the kernel's form).

A whole-image quantity couples the pixels: a pixel at an inner tie in front of a scene stage may take either code, which
moves the statistic and with it every byte of the image a little.  ``bias`` = +1 / -1 resolves every tie of the evaluation
upwards / downwards (a value within tau of a rounding boundary takes the upper / lower code); ``worlds`` evaluates all three
and keeps the main bytes with the tie distances of the WORST world: a byte is decided only if it is decided, and the same,
however the ties in front of the statistic fall.  For sums and maxima of monotone stages every actual outcome lies between
the two biased ones."""
import numpy as np
import torch

import serve_reference as S
from serve_reference import INF, OP_SKIP, OP_TONE_CRYSIS, OP_TONE_FILMIC, OP_GAMMA, OP_GTM_MANUAL, OP_WB_MANUAL, OP_GAIN3

GRAYWORLD, WHITEWORLD, REINHARD = 20, 21, 22
SCENE = (GRAYWORLD, WHITEWORLD, REINHARD)
SCENE_NAMES = {GRAYWORLD: 'grayworld', WHITEWORLD: 'whiteworld', REINHARD: 'reinhard'}
PARAM_WIDTH = {**S.PARAM_WIDTH, GRAYWORLD: 0, WHITEWORLD: 1, REINHARD: 2}
# RISP_SCENE_* and the op code the serving launch takes for the stage (include/risp.h)
SCENE_STAT = {GRAYWORLD: 0, WHITEWORLD: 1, REINHARD: 2}
SCENE_OP = {GRAYWORLD: OP_GAIN3, WHITEWORLD: 9, REINHARD: 10}


# ---------------------------------------------------------------------------------------------------- pieces
def pixel_count(x):
    """the count a mean is taken over: the image's pixels"""
    return x.shape[2] * x.shape[3]


def max_identity():
    """what a maximum starts from"""
    return -np.inf


def lum_weights():
    """luminance weights of the planes in their kept order B, G, R"""
    return 0.114, 0.587, 0.299


def log_floor():
    return 1e-4


def channel_means(x, dtype):
    n = x.shape[0]
    return x.reshape(n, 3, -1).sum(axis=2, dtype=dtype) / dtype(pixel_count(x))


def grayworld_gains(x, dtype=np.float64):
    """(N,3,H,W) -> (N,3) gains"""
    m = channel_means(x.astype(dtype), dtype)
    gray = (m[:, 0] + m[:, 1] + m[:, 2]) / dtype(3)
    return gray[:, None] / np.maximum(m, dtype(1e-6))


def whiteworld_gains(x, ratio, dtype=np.float64):
    """(N,3,H,W), (N,) -> (N,3) gains"""
    n = x.shape[0]
    mx = x.astype(dtype).reshape(n, 3, -1).max(axis=2, initial=max_identity())
    mx = np.maximum(mx.astype(dtype) * dtype(255), dtype(1e-3))
    big = mx.max(axis=1, keepdims=True)
    return dtype(1) + ratio.astype(dtype)[:, None] * (big / mx - dtype(1))


def luminance(v, dtype):
    wb, wg, wr = (dtype(w) for w in lum_weights())
    return wb * v[:, 0] + wg * v[:, 1] + wr * v[:, 2]


def reinhard_constants(x, white_point, middle_grey, dtype=np.float64):
    """(N,3,H,W), (N,), (N,) -> (p0 (N,), p1 (N,)): key / log-average luminance, 1 / Lwhite^2"""
    n = x.shape[0]
    v = np.maximum(x.astype(dtype), dtype(0))
    lsum = np.log(luminance(v, dtype) + dtype(log_floor())).reshape(n, -1).sum(axis=1, dtype=dtype)
    lavg = S._exp(lsum / dtype(pixel_count(x)))
    lw = np.maximum(white_point.astype(dtype), dtype(0.01)) * dtype(10)
    return np.maximum(middle_grey.astype(dtype), dtype(0.01)) / lavg, dtype(1) / (lw * lw)


def reinhard_raw(x, p0, p1, dtype=np.float64):
    """the curve x 255, in front of the clip-and-round"""
    v = np.maximum(x.astype(dtype), dtype(0))
    L = luminance(v, dtype)
    ls = p0.reshape(-1, 1, 1) * L
    s = ls * (dtype(1) + ls * p1.reshape(-1, 1, 1)) / (dtype(1) + ls) / np.maximum(L, dtype(1e-6))
    return v * s[:, None] * dtype(255)


TILE_H, TILE_W = 32, 64            # pixels of a workgroup's tile: one partial row each, row-major over the image


def tile_partials(stat_input, stat, dtype=np.float64):
    """(N,3,H,W) values in front of a scene stage -> (N,G,4) partial rows as risp_serve_scene_stats defines them: per 64 x 32
    pixel tile the sums of B, G, R (stat 0), their maxima (stat 1) or the sum of log-luminance in column 0 (stat 2); unused
    columns 0.  A maximum starts from ``max_identity()``: what an idle thread of a ragged tile holds"""
    x = stat_input.astype(dtype)
    n, _, h, w = x.shape
    gy, gx = -(-h // TILE_H), -(-w // TILE_W)
    out = np.zeros((n, gy * gx, 4), dtype)
    for ty in range(gy):
        for tx in range(gx):
            t = x[:, :, ty * TILE_H:(ty + 1) * TILE_H, tx * TILE_W:(tx + 1) * TILE_W].reshape(n, 3, -1)
            if stat == 0:
                out[:, ty * gx + tx, :3] = t.sum(axis=2, dtype=dtype)
            elif stat == 1:
                out[:, ty * gx + tx, :3] = t.max(axis=2, initial=max_identity())
            else:
                v = np.maximum(t, dtype(0))
                out[:, ty * gx + tx, 0] = np.log(luminance(v, dtype) + dtype(log_floor())).sum(axis=1, dtype=dtype)
    return out


def scene_constants(stage, stat_input, par, dtype=np.float64):
    """the (N,K) per-image constants of a scene stage from the values its statistic is taken over"""
    if stage == GRAYWORLD:
        return grayworld_gains(stat_input, dtype)
    if stage == WHITEWORLD:
        return whiteworld_gains(stat_input, par[:, 0], dtype)
    return np.stack(reinhard_constants(stat_input, par[:, 0], par[:, 1], dtype), axis=1)


# ---------------------------------------------------------------------------------------------------- the pipeline
def serve(raw, white, black, phase, demosaic, ops, params, reverse=False, dtype=np.float64, sync=None, bias=0, tau=None):
    """serve_reference.serve (no bilateral) with the scene stages.  -> Trace; ``Trace.consts``: per scene stage its (N,K)
    constants.  ``bias`` / ``tau``: see the module docstring."""
    raw = np.asarray(raw.cpu().numpy() if isinstance(raw, torch.Tensor) else raw)
    n, h, w = raw.shape
    assert phase in S.SITES and demosaic in S.DEMOSAIC and len(ops) == len(params)
    assert bias == 0 or tau is not None
    tr = S.Trace()
    tr.consts, tr.stat_inputs = [], []
    inner = np.full((n, h, w), INF)
    x, pin0 = S.normalise(raw, white, black, dtype)
    pin_dist = None

    def quantise(kind, unq):
        nonlocal inner
        k = len(tr.points)
        shifted = unq.astype(np.float64) + (bias * tau[kind] if bias else 0.0)
        codes = S.code(shifted if bias else unq).astype(np.int64)
        tr.points.append((kind, unq, codes))
        inner = np.minimum(inner, S.tie_distance(unq).min(axis=1))
        if sync is not None:
            assert sync.points[k][0] == kind
            codes = sync.points[k][2]
        return codes.astype(dtype) / dtype(255), codes, np.where(codes == 0, 1, np.where(codes == 255, 2, 0)).astype(np.int8)

    if demosaic == 'nearest':
        val, codes = S.demosaic_nearest(x, phase), None
        pin = S.demosaic_nearest(pin0, phase)
        pin_dist = np.full(val.shape, INF)
    else:
        val, codes, pin = quantise(demosaic, S.demosaic_stencil(x, phase, demosaic, dtype))
    last = 'nearest' if codes is None else None
    first_scene_input = None
    for op, par in zip(ops, params):
        if op == OP_SKIP:
            continue
        if par is not None:
            par = np.asarray(par.detach().cpu().numpy() if isinstance(par, torch.Tensor) else par, dtype=np.float64)
            par = np.stack([S.image_params(par, i) for i in range(n)])
            assert par.shape == (n, PARAM_WIDTH[op]), 'op %d: parameter block %s' % (op, par.shape)
        if op in (OP_TONE_CRYSIS, OP_TONE_FILMIC):
            val, codes, pin = quantise(S.OP_NAMES[op], S.tone_raw(op, val, par, dtype))
            pin_dist, last = np.full(val.shape, INF), None
            continue
        if op in SCENE:
            if first_scene_input is None:
                first_scene_input = val
            stat_input = scene_stat_input(val, first_scene_input, x, phase, demosaic, dtype)
            tr.stat_inputs.append(stat_input)
            c = scene_constants(op, stat_input, par, dtype)
            tr.consts.append(c)
        if op == WHITEWORLD:
            unq = (val.astype(dtype) * c[:, :, None, None]) * dtype(255)
            val, codes, pin = quantise('whiteworld', unq)
            pin_dist, last = np.full(val.shape, INF), None
            continue
        if op == REINHARD:
            val, codes, pin = quantise('reinhard', reinhard_raw(val, c[:, 0], c[:, 1], dtype))
            pin_dist, last = np.full(val.shape, INF), None
            continue
        if op == GRAYWORLD:
            pre = val.astype(dtype) * c[:, :, None, None]
            new, name = np.clip(pre, dtype(0), dtype(1)), 'grayworld'
        else:
            new, pre = S.elementwise(op, val, par, dtype)
            name = S.OP_NAMES[op]
        if op in (OP_GAMMA, OP_GTM_MANUAL):
            keep = pin
        elif op in (OP_WB_MANUAL, OP_GAIN3, GRAYWORLD):
            keep = np.where(pin == 1, 1, 0).astype(np.int8)
        else:
            keep = np.zeros(val.shape, np.int8)
        if pin_dist is None:
            pin_dist = np.full(val.shape, INF)
        pin_dist = np.where(keep == 2, pin_dist, INF)
        if pre is not None:
            p64 = pre.astype(np.float64)
            cut_hi, cut_lo = (keep == 0) & (p64 >= 1.0), (keep == 0) & (p64 <= 0.0)
            pin_dist = np.where(cut_hi, (p64 - 1.0) * 255.0, pin_dist)
            keep = np.where(cut_hi, 2, np.where(cut_lo, 1, keep)).astype(np.int8)
        val, codes, pin, last = new.astype(dtype), None, keep, name
    if pin_dist is None:
        pin_dist = np.full(val.shape, INF)
    tr.bytes, tr.final = S.final_convert(val, codes, pin, pin_dist, reverse)
    tr.inner, tr.final_kind = inner, last
    t = val.astype(np.float64) * 255.0 if dtype == np.float64 else (val * np.float32(255)).astype(np.float64)
    tr.final_t = np.where(pin != 0, np.nan, t) if codes is None else np.full(val.shape, np.nan)
    tr.final_pin = pin
    return tr


def scene_stat_input(stage_input, first_scene_input, x, phase, demosaic, dtype):
    """what a scene stage's statistic is taken over: the stage's own input (``first_scene_input``, the input of the
    pipeline's first scene stage, and the demosaic's input ``x`` are here for the wrong variants of the CPU test)"""
    return stage_input


def worlds(run, tau):
    """run(bias) -> Trace for bias 0, +1, -1; the main trace with the tie bookkeeping of the worst world.  A pixel whose codes
    at an inner point differ between the worlds is an inner tie; a byte that differs is a final tie (distance 0)."""
    main, up, down = run(0), run(1), run(-1)
    final = main.final.copy()
    for other in (up, down):
        for k, (kind, unq, codes) in enumerate(other.points):
            assert main.points[k][0] == kind
            moved = (codes != main.points[k][2]).any(axis=1, keepdims=True)
            # (a pixel whose code moved: put it on the boundary; every other keeps the other world's distance)
            main.points.append((kind, np.where(moved, np.floor(unq) + 0.5, unq), codes))
        final = np.minimum(final, np.where(other.bytes != main.bytes, 0.0, other.final))
        main.inner = np.minimum(main.inner, other.inner)
    main.final = final
    main.n_points = len(up.points)
    return main
