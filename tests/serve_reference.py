"""Float64 statement of what the serving entry points compute, from the sensor frame to the packed bytes:

    risp_serve_u8[_cfa]        max(s - b, 0) / (white - b) -> nearest demosaic [-> bilateral] -> element-wise stages -> bytes
    risp_serve_classical_u8    ... -> nearest | bilinear | Malvar-He-Cutler demosaic -> element-wise / Crysis / Filmic -> bytes

Truth of tests/test_serve_reference_cpu.py and of the case table tests/serve_space_cases.py.  Plain numpy / torch on the CPU, no HIP and
no import of the package.  It is the SECOND statement of a Bayer phase beside "phase by mirror": a phase is a table of
colour sites (``SITES``), every demosaic below is written for an arbitrary table, and no mirror appears in this file.

OPSPEC restated (constants as oracle/isp_oracle.py lists them, written out here):
  * input: max(s - b, 0) / (white - b), the subtraction in integers;
  * nearest demosaic: R and B from the pixel's own 2 x 2 quad, G from the pixel's own row of that quad; no rounding;
  * bilinear: the mean of the 2 or 4 nearest samples of the missing colour; Malvar-He-Cutler: the four 5 x 5 filters / 8 by
    site type.  Both on samples x 255 with reflect-101 borders (-1 -> 1, H -> H - 2) and the 8-bit code
    floor(clamp(v, 0, 255) + 0.5), returned as code / 255;
  * bilateral (serve_u8 only): fused_segment_reference.bilateral_raw and its code;
  * stages: fused_segment_reference.elementwise for the six element-wise operators; Crysis 1 - exp(-max(x,0) * 0.5 /
    (lum_adapted + 0.05)); Filmic hable(max(x,0) * exposure_bias) / hable(11.2 * max(white_point, 0.01)); both tone curves
    end in the 8-bit code;
  * final conversion floor(clamp(v * 255, 0, 255)), channels B, G, R (R, G, B when reversed).

Integers are carried beside the floats.  A value that is a code / 255 keeps its integer code and the final byte IS that
integer by definition: the reference does not depend on how a route turns the code back into a float (a product with the
reciprocal, k * (1 / 255.0) * 255.0, falls below k for some k in float64).  A value that is exactly 0 or 1 by construction - a
sample at or below the black level, a sample at the white level, the bound of an operator's clamp, the codes 0 and 255 - is
'pinned' and gives byte 0 or 255; Gamma, GtmManual and Skip keep a pin (0 -> 0, 1 -> 1 in any arithmetic), WbManual and
Gain3 keep a pinned 0.

The small functions green_row, far_ring (with its ``inside`` argument), malvar_terms, crysis_scale, filmic_block,
image_params, store_order, final_byte and code are each one sentence of the OPSPEC on its own, so that
tests/test_serve_reference_cpu.py can put a wrong variant of that one sentence in its place.

Tie bookkeeping: at every quantisation point the distance, in codes, of the unquantised float64 value from the nearest
decision boundary.  ``inner`` (N,H,W): the smallest over a pixel's three channels and all inner points (demosaic code,
bilateral code, tone-curve code) - WbQuadratic mixes channels, so a tie in one channel taints the pixel.  ``final``
(N,H,W,3), per byte in stored order: the distance of v * 255 from the nearest integer in 1 .. 255 for a float, infinite
for a carried code, and for a pinned 1 the distance of the operator's unclamped value from its bound.

Every function takes ``dtype``: numpy.float64 is the reference; numpy.float32 evaluates the same expressions in float32
(exp as exp2(x * log2 e), the form of the kernel's fast exponential) to measure what fp32 arithmetic costs (E32).
``sync``: a float32 run that takes the float64 run's codes at every quantisation point, so that each point's error is
that of its own segment and a flipped code does not cascade into the measurement."""
import numpy as np
import torch

import fused_segment_reference as R
import isp_oracle as O

# RISP_OP_* of include/risp.h
OP_SKIP, OP_DEMOSAIC_NEAREST, OP_WB_MANUAL, OP_GAMMA, OP_GTM_MANUAL, OP_WB_QUADRATIC, OP_GAIN3, OP_TONE_CRYSIS, OP_TONE_FILMIC = range(9)
OP_NAMES = {**R.OP_NAMES, OP_TONE_CRYSIS: 'crysis', OP_TONE_FILMIC: 'filmic'}
PARAM_WIDTH = {**R.PARAM_WIDTH, OP_TONE_CRYSIS: 1, OP_TONE_FILMIC: 2}
ELEMENTWISE = (OP_SKIP, OP_WB_MANUAL, OP_GAMMA, OP_GTM_MANUAL, OP_WB_QUADRATIC, OP_GAIN3)
CFA = {'rggb': 0, 'grbg': 1, 'gbrg': 2, 'bggr': 3}                         # RISP_CFA_*
DEMOSAIC = {'nearest': 0, 'bilinear': 1, 'laplacian': 2}                   # RISP_DEMOSAIC_*
# phase -> the colour (0 R, 1 G, 2 B) at (row parity, column parity) of the mosaic
SITES = {'rggb': ((0, 1), (1, 2)), 'grbg': ((1, 0), (2, 1)), 'gbrg': ((1, 2), (0, 1)), 'bggr': ((2, 1), (1, 0))}
INF = np.inf


# ---------------------------------------------------------------------------------------------------- pieces
def normalise(raw, white, black, dtype=np.float64):
    """(N,H,W) integer samples -> max(s - b, 0) / (white - b), and the pins (0: not pinned, 1: exact 0, 2: exact 1)"""
    s = np.maximum(np.asarray(raw).astype(np.int64) - int(black), 0)
    x = s.astype(dtype) / dtype(white - black)
    pin = np.where(s == 0, 1, np.where(s == white - black, 2, 0)).astype(np.int8)
    return x, pin


def reflect101(i, n):
    i = np.abs(i)
    i = np.where(i >= n, 2 * n - 2 - i, i)
    assert i.min() >= 0 and i.max() < n
    return i


def site_colours(phase, h, w):
    """(own, row, col) (H,W) int arrays: the colour of the site itself, of its horizontal and of its vertical neighbours"""
    t = np.array(SITES[phase])
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    return t[yy % 2, xx % 2], t[yy % 2, 1 - xx % 2], t[1 - yy % 2, xx % 2]


def green_row(y):
    """the row of its quad whose green sample a pixel of row y takes in the nearest demosaic: its own"""
    return y % 2


def demosaic_nearest(x, phase):
    """(N,H,W) -> (N,3,H,W) B, G, R: an index map, exact in any dtype"""
    n, h, w = x.shape
    t = SITES[phase]
    where = {t[py][px] if t[py][px] != 1 else ('g', py): (py, px) for py in range(2) for px in range(2)}
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    qy, qx = yy - yy % 2, xx - xx % 2
    red = x[:, qy + where[0][0], qx + where[0][1]]
    blue = x[:, qy + where[2][0], qx + where[2][1]]
    gr = green_row(yy)
    gcol = np.where(gr == 0, where[('g', 0)][1], where[('g', 1)][1])
    green = x[:, qy + gr, qx + gcol]
    return np.stack([blue, green, red], axis=1)


def malvar_terms(c, cross, diag, hor, ver, fh, fv, dtype):
    """the four Malvar-He-Cutler filters / 8: G at an R or B site, the row's colour and the column's colour at a G site, the
    opposite colour at an R or B site"""
    d = dtype
    far = fh + fv
    g_rb = (d(4) * c + d(2) * cross - far) / d(8)
    rb_hor = (d(5) * c + d(4) * hor - diag - fh + d(0.5) * fv) / d(8)
    rb_ver = (d(5) * c + d(4) * ver - diag - fv + d(0.5) * fh) / d(8)
    rb_diag = (d(6) * c + d(2) * diag - d(1.5) * far) / d(8)
    return g_rb, rb_hor, rb_ver, rb_diag


def far_ring(tap, inside):
    """the taps at distance 2: (left + right, above + below).  ``inside(dy, dx)`` tells which taps lie in the image; a tap
    outside is taken through the reflection like every other"""
    return tap(0, -2) + tap(0, 2), tap(-2, 0) + tap(2, 0)


def demosaic_stencil(x, phase, kind, dtype=np.float64):
    """(N,H,W) samples in the [0,1] domain -> (N,3,H,W) B, G, R in codes, IN FRONT of the clip-and-round"""
    n, h, w = x.shape
    assert h >= 4 and w >= 4 and h % 2 == 0 and w % 2 == 0
    m = x.astype(dtype) * dtype(255)
    rows, cols = np.arange(h), np.arange(w)
    tap = lambda dy, dx: m[:, reflect101(rows + dy, h)][:, :, reflect101(cols + dx, w)]
    c = tap(0, 0)
    cross = tap(-1, 0) + tap(1, 0) + tap(0, -1) + tap(0, 1)
    diag = tap(-1, -1) + tap(-1, 1) + tap(1, -1) + tap(1, 1)
    hor, ver = tap(0, -1) + tap(0, 1), tap(-1, 0) + tap(1, 0)
    if kind == 'bilinear':
        g_rb, rb_hor, rb_ver, rb_diag = cross / dtype(4), hor / dtype(2), ver / dtype(2), diag / dtype(4)
    elif kind == 'laplacian':
        inside = lambda dy, dx: (((rows + dy >= 0) & (rows + dy < h))[:, None] & ((cols + dx >= 0) & (cols + dx < w))[None, :])
        fh, fv = far_ring(tap, inside)
        g_rb, rb_hor, rb_ver, rb_diag = malvar_terms(c, cross, diag, hor, ver, fh, fv, dtype)
    else:
        raise ValueError(kind)
    own, row, col = site_colours(phase, h, w)
    out = {1: np.where(own == 1, c, g_rb)}
    for k in (0, 2):            # R, B: the sample itself; at a green site the row's or the column's colour; else the diagonal one
        out[k] = np.where(own == k, c, np.where((own == 1) & (row == k), rb_hor, np.where((own == 1) & (col == k), rb_ver, rb_diag)))
    return np.stack([out[2], out[1], out[0]], axis=1)


def code(v):
    """the 8-bit code of a value in the 0..255 domain"""
    return np.floor(np.clip(v, 0.0, 255.0) + v.dtype.type(0.5))


def tie_distance(raw):
    return R.tie_distance(torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float64))).numpy()


def final_byte(v):
    """floor(clamp(v * 255, 0, 255)) of a float"""
    return np.floor(np.clip(v * v.dtype.type(255), 0.0, 255.0))


def final_distance(t):
    """the truncation's analogue of tie_distance: distance of t = v * 255 from the nearest integer in 1 .. 255 (the byte
    changes where t crosses one); below 1 and above 255 the nearest boundary is 1 / 255"""
    t = np.asarray(t, np.float64)
    c = np.clip(t, 1.0, 255.0)
    d = np.minimum(c - np.floor(c), np.ceil(c) - c)
    return np.where(t < 1.0, 1.0 - t, np.where(t > 255.0, t - 255.0, d))


def _exp(x):
    if x.dtype == np.float32:                               # the form of the fast exponential: exp2(x * log2 e) in float32
        return np.exp2(x * np.float32(1.4426950408889634))
    return np.exp(x)


def hable(t):
    d = t.dtype.type
    A, B, C, D, E, F = d(0.15), d(0.50), d(0.10), d(0.20), d(0.02), d(0.30)
    return (t * (A * t + C * B) + D * E) / (t * (A * t + B) + D * F) - E / F


def crysis_scale(lum, dtype):
    return dtype(0.5) / (lum + dtype(0.05))


def filmic_block(par):
    """(white_point, exposure_bias) columns of the (N,2) block"""
    return par[:, 0], par[:, 1]


def tone_raw(op, x, par, dtype=np.float64):
    """(N,3,H,W) in the [0,1] domain, (N,P) block -> the curve x 255, in front of the clip-and-round"""
    n = x.shape[0]
    p = np.asarray(par, dtype=np.float64).astype(dtype)
    assert p.shape == (n, PARAM_WIDTH[op]), 'op %d: parameter block %s' % (op, p.shape)
    v = np.maximum(x.astype(dtype), dtype(0))
    col = lambda a: a.reshape(n, 1, 1, 1)
    if op == OP_TONE_CRYSIS:
        out = dtype(1) - _exp(-v * col(crysis_scale(p[:, 0], dtype)))
    elif op == OP_TONE_FILMIC:
        wp, bias = filmic_block(p)
        out = hable(v * col(bias)) / col(hable(np.maximum(wp, dtype(0.01)) * dtype(11.2)))
    else:
        raise ValueError(op)
    return out * dtype(255)


def elementwise(op, x, par, dtype=np.float64):
    """one element-wise stage on (N,3,H,W): fused_segment_reference.elementwise in float64; the same operators of the
    oracle on float32 tensors otherwise.  -> (value, value in front of the operator's clamp or None)"""
    if op == OP_SKIP:
        return x, None
    tt = torch.float64 if dtype == np.float64 else torch.float32
    xt, pt = torch.from_numpy(np.ascontiguousarray(x)).to(tt), torch.as_tensor(np.asarray(par, dtype=np.float64)).to(tt)
    n = x.shape[0]
    assert tuple(pt.shape) == (n, PARAM_WIDTH[op]), 'op %d: parameter block %s' % (op, tuple(pt.shape))
    pre = None
    if op == OP_GAIN3:
        pre = xt * pt.view(n, 3, 1, 1)
    elif op == OP_WB_QUADRATIC:
        pre = _wbq_unclamped(xt, pt)
    elif op == OP_GTM_MANUAL:
        pre = xt                                            # outside [0,1) the curve passes its input through to the clamp
    if dtype == np.float64:
        y = R.elementwise(op, xt, pt)
    elif op == OP_WB_MANUAL:
        y = xt * pt.view(n, 3, 1, 1)
    elif op == OP_GAMMA:
        y = O.gamma_manual(xt, pt)
    elif op == OP_GTM_MANUAL:
        y = O.gtm_manual(xt, pt)
    elif op == OP_WB_QUADRATIC:
        y = O.wb_quadratic(xt, pt)
    elif op == OP_GAIN3:
        y = pre.clamp(0.0, 1.0)
    else:
        raise ValueError(op)
    return y.numpy(), None if pre is None else pre.numpy()


def _wbq_unclamped(x, p):
    """the polynomial of WbQuadratic in front of its clamp (the oracle's expression, term by term)"""
    c = (p * 10 - 5).view(-1, 3, 10)
    b, g, r = x[:, 0:1], x[:, 1:2], x[:, 2:3]
    out = c[:, :, 9].view(-1, 3, 1, 1).expand(-1, -1, x.shape[2], x.shape[3])
    for j, f in enumerate([b * b, g * g, r * r, b * g, b * r, g * r, b, g, r]):
        out = out + f * c[:, :, j].view(-1, 3, 1, 1)
    return out


def image_params(par, i):
    """the parameter row image i takes from its (N,P) block: its own"""
    return par[i]


def final_convert(val, codes, pin, pin_dist, reverse):
    """-> (bytes (N,H,W,3) uint8, final distance (N,H,W,3))"""
    if codes is not None:
        byte, dist = codes.astype(np.float64), np.full(codes.shape, INF)
    else:
        byte = np.where(pin == 1, 0.0, np.where(pin == 2, 255.0, final_byte(val))).astype(np.float64)
        dist = np.where(pin == 1, 1.0, np.where(pin == 2, pin_dist, final_distance(val.astype(np.float64) * 255.0)))
    order = store_order(reverse)
    return (np.ascontiguousarray(byte[:, order].transpose(0, 2, 3, 1)).astype(np.uint8),
            np.ascontiguousarray(dist[:, order].transpose(0, 2, 3, 1)))


def store_order(reverse):
    """planes are kept B, G, R; the stored order is B, G, R, or R, G, B when reversed"""
    return [2, 1, 0] if reverse else [0, 1, 2]


# ---------------------------------------------------------------------------------------------------- the pipeline
class Trace:
    """what one evaluation leaves: bytes, the tie bookkeeping, and per quantisation point (kind, unquantised value, codes)"""

    def __init__(self):
        self.points, self.bytes, self.inner, self.final, self.final_kind, self.final_t = [], None, None, None, None, None
        self.bilateral_windows, self.final_pin = None, None        # per-image windows where a bilateral ran; pins at the truncation


def serve(raw, white, black, phase, demosaic, bilateral, ops, params, reverse=False, dtype=np.float64, sync=None):
    """raw (N,H,W) uint16 (or any integer) frames -> Trace.

    ``phase`` a key of SITES, ``demosaic`` a key of DEMOSAIC, ``bilateral`` None or (window (N,), sigma_color (N,),
    sigma_space (N,)) - behind the nearest demosaic only -, ``ops`` / ``params`` the stage list as the C ABI takes it
    (per-image (N,P) blocks, None for SKIP).  ``sync``: the float64 Trace whose codes a float32 run takes over."""
    raw = np.asarray(raw.cpu().numpy() if isinstance(raw, torch.Tensor) else raw)
    n, h, w = raw.shape
    assert phase in SITES and demosaic in DEMOSAIC and len(ops) == len(params)
    tr = Trace()
    inner = np.full((n, h, w), INF)
    x, pin0 = normalise(raw, white, black, dtype)
    pin_dist = None

    def quantise(kind, unq):
        """record a quantisation point, -> (value, codes)"""
        nonlocal inner
        k = len(tr.points)
        codes = code(unq).astype(np.int64)
        tr.points.append((kind, unq, codes))
        inner = np.minimum(inner, tie_distance(unq).min(axis=1))
        if sync is not None:
            assert sync.points[k][0] == kind
            codes = sync.points[k][2]
        return codes.astype(dtype) / dtype(255), codes, np.where(codes == 0, 1, np.where(codes == 255, 2, 0)).astype(np.int8)

    if demosaic == 'nearest':
        val, codes = demosaic_nearest(x, phase), None
        pin = demosaic_nearest(pin0, phase)
        pin_dist = np.full(val.shape, INF)
    else:
        assert bilateral is None, 'a bilateral follows the nearest demosaic only'
        val, codes, pin = quantise(demosaic, demosaic_stencil(x, phase, demosaic, dtype))
    last = 'nearest' if codes is None else None             # the kind of the last stage that left a float
    if bilateral is not None:
        window, sc, ss = bilateral
        if dtype == np.float64:
            unq = R.bilateral_raw(torch.from_numpy(val * 255.0), window, sc, ss).numpy()
        else:                                               # the oracle's own bilateral on float32 tensors
            p = {'window_length': torch.as_tensor(window), 'sigma_color': torch.as_tensor(sc), 'sigma_space': torch.as_tensor(ss)}
            with O.unquantized():
                unq = O.origin_denoise(torch.from_numpy(val) * 255.0, 'bilateral', p).numpy()
        win = np.asarray(window).reshape(-1)
        assert set(win.tolist()) <= {1, 3}
        val, codes, pin = quantise('bilateral', unq)
        tr.bilateral_windows = win
        pin_dist, last = np.full(val.shape, INF), None
    for op, par in zip(ops, params):
        if op == OP_SKIP:
            continue
        if par is not None:
            par = np.asarray(par.detach().cpu().numpy() if isinstance(par, torch.Tensor) else par, dtype=np.float64)
            par = np.stack([image_params(par, i) for i in range(n)])
        if op in (OP_TONE_CRYSIS, OP_TONE_FILMIC):
            val, codes, pin = quantise(OP_NAMES[op], tone_raw(op, val, par, dtype))
            pin_dist, last = np.full(val.shape, INF), None
            continue
        new, pre = elementwise(op, val, par, dtype)
        # pins: Gamma and GtmManual keep 0 and 1, WbManual and Gain3 keep 0; a clamp pins what it cuts
        if op == OP_GAMMA:
            keep = pin
        elif op == OP_GTM_MANUAL:
            keep = pin
        elif op in (OP_WB_MANUAL, OP_GAIN3):
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
        val, codes, pin, last = new.astype(dtype), None, keep, OP_NAMES[op]
    if pin_dist is None:
        pin_dist = np.full(val.shape, INF)
    tr.bytes, tr.final = final_convert(val, codes, pin, pin_dist, reverse)
    tr.inner, tr.final_kind = inner, last
    # the unclamped v * 255 of the last stage, for measuring E32 at the truncation (NaN where a code or a pin decides)
    t = val.astype(np.float64) * 255.0 if dtype == np.float64 else (val * np.float32(255)).astype(np.float64)
    tr.final_t = np.where(pin != 0, np.nan, t) if codes is None else np.full(val.shape, np.nan)
    tr.final_pin = pin
    return tr


def taus(tr, TAU):
    """-> (inner threshold per pixel's point folded into a mask of decided pixels (N,H,W), final TAU (scalar))"""
    n = tr.bytes.shape[0]
    decided = np.ones(tr.bytes.shape[:3], bool)
    for kind, unq, _ in tr.points:
        if kind == 'bilateral':
            tau = np.array([TAU['bilateral%d' % k] for k in tr.bilateral_windows]).reshape(n, 1, 1)
        else:
            tau = TAU[kind]
        decided &= tie_distance(unq).min(axis=1) > tau
    return decided, (TAU['final/' + tr.final_kind] if tr.final_kind else 0.0)


TIE_CAP = 2e-3                   # inner-tie pixels of one case (the cap of tests/test_gpu_fused_segment.py)
FINAL_CAP = 1e-2                 # bytes of one case under the +-1 rule


def tie_shares(tr, TAU):
    """(share of pixels with an inner tie, share of bytes of decided pixels under the +-1 rule): the input's properties"""
    decided, tau_f = taus(tr, TAU)
    loose = decided[..., None] & (tr.final <= tau_f)
    return 1.0 - decided.mean(), loose.mean()


def check(got, tr, TAU):
    """the comparison rule.  got (N,H,W,3) uint8 -> (list of violations, report dict)"""
    got = np.asarray(got.cpu().numpy() if isinstance(got, torch.Tensor) else got).astype(np.int64)
    want = tr.bytes.astype(np.int64)
    assert got.shape == want.shape, (got.shape, want.shape)
    decided, tau_f = taus(tr, TAU)
    d = np.abs(got - want)
    dec = np.broadcast_to(decided[..., None], d.shape)
    strict = dec & (tr.final > tau_f)
    loose = dec & ~(tr.final > tau_f)
    bad = []
    if (d[strict] != 0).any():
        k = np.argwhere(strict & (d != 0))[0]
        bad.append('%d decided bytes differ, first at %s: got %d want %d (inner %.3e, final %.3e codes)' % (
            (d[strict] != 0).sum(), tuple(k), got[tuple(k)], want[tuple(k)], tr.inner[tuple(k[:3])], tr.final[tuple(k)]))
    if (d[loose] > 1).any():
        bad.append('%d bytes at a final tie differ by more than 1' % (d[loose] > 1).sum())
    inner_share, loose_share = 1.0 - decided.mean(), loose.mean()
    if inner_share > TIE_CAP:
        bad.append('%.3e of the pixels at an inner tie (cap %.0e)' % (inner_share, TIE_CAP))
    if loose_share > FINAL_CAP:
        bad.append('%.3e of the bytes under the +-1 rule (cap %.0e)' % (loose_share, FINAL_CAP))
    diff = d != 0
    dist = np.where(dec, tr.final, np.broadcast_to(tr.inner[..., None], d.shape))
    report = dict(decided_differ=int((d[strict] != 0).sum()), decided_share=float((d[strict] != 0).sum() / d.size),
                  differ=int(diff.sum()), share=float(diff.mean()), worst=float(dist[diff].max()) if diff.any() else 0.0,
                  inner_share=float(inner_share), loose_share=float(loose_share))
    return bad, report


# ---------------------------------------------------------------------------------------------------- the plugin mapping
STAGE_OPS = {'wbmanual': OP_WB_MANUAL, 'gamma': OP_GAMMA, 'gtmmanual': OP_GTM_MANUAL, 'wbquadratic': OP_WB_QUADRATIC,
             'crysisengine': OP_TONE_CRYSIS, 'filmic': OP_TONE_FILMIC, 'skip': OP_SKIP}


def plugin_stages(step_names, blocks):
    """a fixed pipeline's stage names and its per-image (N,P) parameters after the sigmoid -> (demosaic, bilateral, ops,
    params) as the C ABI takes them, by the mapping the modules apply (in float32, the type of the blocks): WbManual
    gain = 5 p; Filmic (white_point, exposure_bias) = (p0, 1 + 9 p1); Crysis lum_adapted = p0; bilateral window =
    (int(p0) * 7) * 2 + 3, sigma_color = 1 + 99 p1, sigma_space = 1 + 99 p2; every other block is the parameter itself"""
    f = np.float32
    demosaic, bilateral, ops, params = None, None, [], []
    for name, p in zip(step_names, blocks):
        p = None if p is None else np.asarray(p, dtype=f)
        if name in DEMOSAIC:
            assert demosaic is None and not ops
            demosaic = name
        elif name == 'bilateral':
            assert demosaic == 'nearest' and not ops and bilateral is None
            bilateral = ((p[:, 0].astype(np.int32) * 7) * 2 + 3, p[:, 1] * f(99) + f(1), p[:, 2] * f(99) + f(1))
        else:
            op = STAGE_OPS[name]
            ops.append(op)
            if op == OP_WB_MANUAL:
                p = p * f(5)
            elif op == OP_TONE_FILMIC:
                p = np.stack([p[:, 0], p[:, 1] * f(9) + f(1)], axis=1)
            elif op == OP_TONE_CRYSIS:
                p = p[:, :1]
            params.append(p)
    return demosaic, bilateral, ops, params
