"""Float64 statement of what the serving entry points compute, from the sensor frame to the packed bytes:

    risp_serve_u8[_cfa]        max(s - b, 0) / (white - b) -> nearest demosaic [-> bilateral] -> element-wise stages -> bytes
    risp_serve_classical_u8    ... -> nearest | bilinear | Malvar-He-Cutler demosaic -> element-wise / Crysis / Filmic -> bytes
    risp_serve_denoise_u8      ... -> one of the three demosaics -> stages -> bilateral | median | non-local means -> stages -> bytes

Truth of tests/test_serve_reference_cpu.py, tests/test_serve_denoise_reference_cpu.py and of the case tables
tests/serve_space_cases.py and tests/serve_denoise_cases.py.  Plain numpy / torch on the CPU, no HIP and
no import of the package.  It is the SECOND statement of a Bayer phase beside "phase by mirror": a phase is a table of
colour sites (``SITES``), every demosaic below is written for an arbitrary table, and no mirror appears in this file.

OPSPEC restated (constants as oracle/isp_oracle.py lists them, written out here):
  * input: max(s - b, 0) / (white - b), the subtraction in integers;
  * nearest demosaic: R and B from the pixel's own 2 x 2 quad, G from the pixel's own row of that quad; no rounding;
  * bilinear: the mean of the 2 or 4 nearest samples of the missing colour; Malvar-He-Cutler: the four 5 x 5 filters / 8 by
    site type.  Both on samples x 255 with reflect-101 borders (-1 -> 1, H -> H - 2) and the 8-bit code
    floor(clamp(v, 0, 255) + 0.5), returned as code / 255;
  * bilateral (serve_u8 only): fused_segment_reference.bilateral_raw and its code;
  * denoisers (serve_denoise_u8; oracle/isp_oracle.py: origin_denoise), on the finished pixels x 255 with reflect-101
    borders in image coordinates: bilateral, window 3, weights exp(-(dy^2 + dx^2) / (2 ss^2) - d^2 / (2 sc^2)) with d the L1
    colour distance, one weighted mean per channel and its code; median 3 x 3 of the 8-bit codes of its input, per channel,
    an integer carried as a code; non-local means, block 3 and search 3: per shift d2 = the sum over the block and the
    channels of squared differences, weight exp(-(d2 / 27) / decay^2), the centre shift 1, the weighted mean and its code;
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
image_params, store_order, final_byte and code - and for the denoisers denoise_border, median_input, median_window,
colour_distance, spatial_term, nlm_normaliser, nlm_block_pair, nlm_weight, nlm_centre_weight and split_stages - are each
one sentence of the OPSPEC on its own, so that tests/test_serve_reference_cpu.py and
tests/test_serve_denoise_reference_cpu.py can put a wrong variant of that one sentence in its place.

Tie bookkeeping: at every quantisation point the distance, in codes, of the unquantised float64 value from the nearest
decision boundary.  ``inner`` (N,H,W): the smallest over a pixel's three channels and all inner points (demosaic code,
bilateral code, tone-curve code, the codes 'den-bilateral' and 'fastnlm' of the denoise route, and the median's input code
'median-in/<last op>' where a float stands in front of it: a carried code makes the median exact) - WbQuadratic mixes channels, so a tie in one channel taints the pixel.  A denoiser mixes
pixels: a code in front of it that may fall either way reaches every pixel of its footprint, which neighbour_taint excuses
where that code can change the denoiser's result (a second evaluation with every such code on its other side).  ``final``
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


# ---------------------------------------------------------------------------------------------------- the classical denoisers
DENOISERS = ('bilateral', 'median', 'fastnlm')             # RISP_DENOISE_* in this order


def denoise_border(i, n):
    """the denoisers take a neighbour outside the image from the FINISHED pixels through reflect-101 in image coordinates"""
    return reflect101(i, n)


def _taps(v):
    """v (N,3,H,W) -> tap(dy, dx): the image shifted by (dy, dx) under the denoisers' border rule"""
    h, w = v.shape[2:]
    rows, cols = np.arange(h), np.arange(w)
    return lambda dy, dx: v[:, :, denoise_border(rows + dy, h)][:, :, :, denoise_border(cols + dx, w)]


def colour_distance(q, c):
    """the bilateral's colour distance between a neighbour and the centre: L1 over the three channels"""
    return np.abs(q - c).sum(axis=1, keepdims=True)


def spatial_term(dy, dx, ss, dtype):
    """the bilateral's spatial exponent (dy^2 + dx^2) / (2 ss^2)"""
    return dtype(dy * dy + dx * dx) / (dtype(2) * ss * ss)


def denoise_bilateral(v, sigma_color, sigma_space, dtype=np.float64):
    """window 3.  v (N,3,H,W) in the 0..255 domain, (N,) sigmas -> the weighted mean in front of the clip-and-round.  The
    oracle's expression term by term (one reciprocal per pixel); in float64 it is fused_segment_reference.bilateral_raw at
    window 3 (tests/test_serve_denoise_reference_cpu.py), written out here so that one sentence of it can be replaced"""
    d, n = dtype, v.shape[0]
    v = v.astype(d)
    sc, ss = (np.asarray(a, np.float64).astype(d).reshape(n, 1, 1, 1) for a in (sigma_color, sigma_space))
    tap = _taps(v)
    num, den = np.zeros(v.shape, d), np.zeros((n, 1) + v.shape[2:], d)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            q = tap(dy, dx)
            dist = colour_distance(q, v)
            wgt = _exp(-spatial_term(dy, dx, ss, d) - dist * dist / (d(2) * sc * sc))
            num, den = num + wgt * q, den + wgt
    return num * (d(1) / den)


def median_input(v, codes, dtype):
    """what the median sorts: the 8-bit codes of its input, floor(clamp(v, 0, 255) + 0.5)"""
    return codes.astype(dtype)


def median_window(win):
    """win (N,3,H,W,9), the 3 x 3 neighbourhood of every channel -> the middle of the 9 values, per channel"""
    return np.sort(win, axis=-1)[..., 4]


def denoise_median(c):
    """3 x 3.  c (N,3,H,W) -> the median of every channel's neighbourhood"""
    tap = _taps(c)
    return median_window(np.stack([tap(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=-1))


def nlm_normaliser():
    """d2 is divided by channels x block x block"""
    return 3 * 3 * 3


def nlm_block_pair(tap, sy, sx, oy, ox):
    """the two pixels compared at block offset (oy, ox) for the shift (sy, sx): the offset moves both sides"""
    return tap(sy + oy, sx + ox), tap(oy, ox)


def nlm_weight(d2, decay, dtype):
    """exp(-(d2 / normaliser) / decay^2)"""
    return _exp(-(d2 / dtype(nlm_normaliser())) / (decay * decay))


def nlm_centre_weight():
    """the unshifted pixel takes part, with weight 1 (its d2 is 0)"""
    return 1


def denoise_fastnlm(v, decay, dtype=np.float64):
    """block 3, search 3.  v (N,3,H,W) in the 0..255 domain, (N,) decay -> the weighted mean in front of the clip-and-round"""
    d, n = dtype, v.shape[0]
    v = v.astype(d)
    decay = np.asarray(decay, np.float64).astype(d).reshape(n, 1, 1, 1)
    tap = _taps(v)
    num, den = np.zeros(v.shape, d), np.zeros((n, 1) + v.shape[2:], d)
    for sy in (-1, 0, 1):
        for sx in (-1, 0, 1):
            if (sy, sx) == (0, 0):
                wgt = np.full(den.shape, nlm_centre_weight(), d)
            else:
                d2 = np.zeros(den.shape, d)
                for oy in (-1, 0, 1):
                    for ox in (-1, 0, 1):
                        a, b = nlm_block_pair(tap, sy, sx, oy, ox)
                        d2 = d2 + ((a - b) * (a - b)).sum(axis=1, keepdims=True)
                wgt = nlm_weight(d2, decay, d)
            num, den = num + wgt * tap(sy, sx), den + wgt
    return num * (d(1) / den)


def split_stages(stages, n_pre):
    """the stage list as (stages in front of the denoiser, stages behind it): the first n_pre, the rest"""
    return stages[:n_pre], stages[n_pre:]


# ---------------------------------------------------------------------------------------------------- the pipeline
class Trace:
    """what one evaluation leaves: bytes, the tie bookkeeping, and per quantisation point (kind, unquantised value, codes)"""

    def __init__(self):
        self.points, self.bytes, self.inner, self.final, self.final_kind, self.final_t = [], None, None, None, None, None
        self.bilateral_windows, self.final_pin = None, None        # per-image windows where a bilateral ran; pins at the truncation
        # the denoise route: how many points stand in front of the denoiser's neighbourhood, (name, its output in front of
        # the code - the median's codes), the evaluation again with flipped ties (neighbour_taint), its cached result
        self.denoise_at, self.denoise_out, self.rerun, self.taint, self.taint_distance = None, None, None, None, None


def serve(raw, white, black, phase, demosaic, bilateral, ops, params, reverse=False, dtype=np.float64, sync=None, denoise=None,
          _flip=None):
    """raw (N,H,W) uint16 (or any integer) frames -> Trace.

    ``phase`` a key of SITES, ``demosaic`` a key of DEMOSAIC, ``bilateral`` None or (window (N,), sigma_color (N,),
    sigma_space (N,)) - behind the nearest demosaic only -, ``ops`` / ``params`` the stage list as the C ABI takes it
    (per-image (N,P) blocks, None for SKIP).  ``sync``: the float64 Trace whose codes a float32 run takes over.
    ``denoise`` None or (name, n_pre, args) - risp_serve_denoise_u8 -: ``name`` of DENOISERS at the sizes that entry point
    serves (window 3, 3 x 3, block 3 and search 3), behind the first ``n_pre`` entries of ``ops``, ``args`` its per-image (N,)
    blocks as the C ABI takes them: (sigma_color, sigma_space), () or (decay,).  ``_flip``: a TAU; every code in front of the
    denoiser that stands within it of a boundary takes the other side (neighbour_taint's second evaluation)."""
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
        if _flip is not None and tr.denoise_at is None:
            codes = np.where(tie_distance(unq) <= _flip[kind], other_code(unq, codes), codes)
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
    stages = list(zip(ops, params))
    if denoise is not None:
        name, n_pre, args = denoise
        assert bilateral is None and name in DENOISERS and 0 <= n_pre <= len(ops) and len(args) == {'bilateral': 2, 'median': 0, 'fastnlm': 1}[name]
        pre, post = split_stages(stages, n_pre)
        stages = list(pre) + [(name, args)] + list(post)
    for op, par in stages:
        if op == OP_SKIP:
            continue
        if op in DENOISERS:
            arg = [np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64).reshape(n) for a in par]
            arg = [np.stack([image_params(a, i) for i in range(n)]) for a in arg]
            # the pixels x 255; a carried code is its integer, whatever float stands for it
            v = codes.astype(dtype) if codes is not None else val.astype(dtype) * dtype(255)
            if op == 'median':
                cin = codes
                if cin is None:                             # a float in front: the median's input code is a quantisation point
                    _, cin, _ = quantise('median-in/' + last, v)
                tr.denoise_at = len(tr.points)
                m = denoise_median(median_input(v, cin, dtype))
                tr.denoise_out = (op, m)
                # the middle of nine codes is a code, carried on (were it taken on floats it would be a float)
                codes, last = (m.astype(np.int64), None) if np.array_equal(m, np.floor(m)) else (None, 'median')
                val = m / dtype(255)
                pin = np.where(m == 0, 1, np.where(m == 255, 2, 0)).astype(np.int8)
            elif op == 'bilateral':
                tr.denoise_at = len(tr.points)
                val, codes, pin = quantise('den-bilateral', denoise_bilateral(v, arg[0], arg[1], dtype))
                tr.denoise_out, last = (op, tr.points[-1][1]), None
            else:
                tr.denoise_at = len(tr.points)
                val, codes, pin = quantise('fastnlm', denoise_fastnlm(v, arg[0], dtype))
                tr.denoise_out, last = (op, tr.points[-1][1]), None
            pin_dist = np.full(val.shape, INF)
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
    if denoise is not None and _flip is None:
        tr.rerun = lambda TAU: serve(raw, white, black, phase, demosaic, None, ops, params, reverse, denoise=denoise, _flip=TAU)
    return tr


def other_code(unq, codes):
    """the code on the other side of the boundary nearest to the unquantised value"""
    return np.clip(np.where(unq >= codes, codes + 1, codes - 1), 0, 255)


def neighbour_taint(tr, TAU):
    """(N,H,W): pixels whose own points are decided but whose denoiser reads a neighbour that is not.  A denoiser mixes
    pixels, so a code in front of it that may fall either way (within TAU of its boundary; the median's input code among
    them) reaches every pixel of the footprint - 3 x 3 for the bilateral and the median, 5 x 5 for non-local means.  The
    pipeline is evaluated a second time with every such code on its other side.  A pixel with ONE such code in its
    footprint has exactly the two outcomes that the two evaluations hold: it stays decided when they give the denoiser the
    same code, the second one also further than TAU from a boundary (the median: the same middle code).  A pixel with two or
    more in its footprint (a reflected neighbour counts twice) is excused without looking"""
    key = tuple(sorted(TAU.items()))
    if tr.taint is None or tr.taint[0] != key:
        name, out = tr.denoise_out
        near = [(tie_distance(unq) <= TAU[kind]).sum(axis=1) for kind, unq, _ in tr.points[:tr.denoise_at]]
        mask = np.zeros(out.shape[:1] + out.shape[2:], bool)
        tr.taint_distance = np.full(mask.shape, INF)        # of the nearest boundary among the codes the denoiser reads (the report's)
        if near and sum(near).any():
            other = tr.rerun(TAU).denoise_out[1]
            r = 2 if name == 'fastnlm' else 1
            window = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
            tap = _taps(sum(near)[:, None])
            foot = sum(tap(dy, dx) for dy, dx in window)[:, 0]
            tap = _taps(np.minimum.reduce([tie_distance(unq).min(axis=1) for _, unq, _ in tr.points[:tr.denoise_at]])[:, None])
            tr.taint_distance = np.minimum.reduce([tap(dy, dx) for dy, dx in window])[:, 0]
            if name == 'median':
                moved = (out != other).any(axis=1)
            else:
                moved = (code(out) != code(other)).any(axis=1) | (tie_distance(other).min(axis=1) <= TAU[tr.points[tr.denoise_at][0]])
            mask = (foot >= 2) | ((foot >= 1) & moved)
        tr.taint = (key, mask)
    return tr.taint[1]


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
    if tr.denoise_at is not None:
        decided &= ~neighbour_taint(tr, TAU)
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
    inner = tr.inner if tr.denoise_at is None else np.where(neighbour_taint(tr, TAU), np.minimum(tr.inner, tr.taint_distance), tr.inner)
    dist = np.where(dec, tr.final, np.broadcast_to(inner[..., None], d.shape))
    report = dict(decided_differ=int((d[strict] != 0).sum()), decided_share=float((d[strict] != 0).sum() / d.size),
                  differ=int(diff.sum()), share=float(diff.mean()), worst=float(dist[diff].max()) if diff.any() else 0.0,
                  inner_share=float(inner_share), loose_share=float(loose_share))
    return bad, report


# ---------------------------------------------------------------------------------------------------- the plugin mapping
STAGE_OPS = {'wbmanual': OP_WB_MANUAL, 'gamma': OP_GAMMA, 'gtmmanual': OP_GTM_MANUAL, 'wbquadratic': OP_WB_QUADRATIC,
             'crysisengine': OP_TONE_CRYSIS, 'filmic': OP_TONE_FILMIC, 'skip': OP_SKIP}


def plugin_stages(step_names, blocks, denoise=False):
    """a fixed pipeline's stage names and its per-image (N,P) parameters after the sigmoid -> (demosaic, bilateral, ops,
    params) as the C ABI takes them, by the mapping the modules apply (in float32, the type of the blocks): WbManual
    gain = 5 p; Filmic (white_point, exposure_bias) = (p0, 1 + 9 p1); Crysis lum_adapted = p0; bilateral window =
    (int(p0) * 7) * 2 + 3, sigma_color = 1 + 99 p1, sigma_space = 1 + 99 p2; every other block is the parameter itself.

    ``denoise=True``: -> (demosaic, bilateral, ops, params, denoise) with ``denoise`` as ``serve`` takes it, for one classical
    denoiser that is not the bilateral directly behind the nearest demosaic (pipeline_fusion._denoise_args): a bilateral as
    above; median size = 2 int(7 p) + 3 of image 0; non-local means block = (int(p0) * 7) * 2 + 3, search the same of p1,
    decay = 1 + 99 p2.  The sizes must be the ones the route serves: 3, 3 x 3, (3, 3)"""
    f = np.float32
    demosaic, bilateral, ops, params, den = None, None, [], [], None
    for name, p in zip(step_names, blocks):
        p = None if p is None else np.asarray(p, dtype=f)
        if name in DEMOSAIC:
            assert demosaic is None and not ops
            demosaic = name
        elif name == 'bilateral' and not (denoise and (demosaic != 'nearest' or ops)):
            assert demosaic == 'nearest' and not ops and bilateral is None and den is None
            bilateral = ((p[:, 0].astype(np.int32) * 7) * 2 + 3, p[:, 1] * f(99) + f(1), p[:, 2] * f(99) + f(1))
        elif name in DENOISERS:
            assert denoise and demosaic is not None and bilateral is None and den is None
            if name == 'bilateral':
                assert ((p[:, 0].astype(np.int32) * 7) * 2 + 3 == 3).all()
                den = (name, len(ops), (p[:, 1] * f(99) + f(1), p[:, 2] * f(99) + f(1)))
            elif name == 'median':
                assert 2 * int(p[0, 0] * 7) + 3 == 3
                den = (name, len(ops), ())
            else:
                assert ((p[:, :2].astype(np.int32) * 7) * 2 + 3 == 3).all()
                den = (name, len(ops), (p[:, 2] * f(99) + f(1),))
        else:
            op = STAGE_OPS[name]
            if op == OP_SKIP and demosaic is None:          # a Skip on the mosaic, in front of the demosaic
                continue
            ops.append(op)
            if op == OP_WB_MANUAL:
                p = p * f(5)
            elif op == OP_TONE_FILMIC:
                p = np.stack([p[:, 0], p[:, 1] * f(9) + f(1)], axis=1)
            elif op == OP_TONE_CRYSIS:
                p = p[:, :1]
            params.append(p)
    return (demosaic, bilateral, ops, params, den) if denoise else (demosaic, bilateral, ops, params)
