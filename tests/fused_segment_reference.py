"""Float64 restatement of the fused stencil segment (risp_bilateral_chain_fwd, include/risp.h):

    [nearest demosaic ->] bilateral denoise -> element-wise tail

Truth of tests/test_fused_segment_reference_cpu.py and tests/test_gpu_fused_segment.py.  Plain torch / numpy on the CPU,
float64 throughout, no HIP.  It is a SECOND statement of the OPSPEC beside oracle/isp_oracle.py: the demosaic is written
as an index map, the borders as explicit reflect-101 indices and the window as a gather per tap - nothing here calls the
oracle's bilateral, its padding or its demosaic.  Only the element-wise operators are the oracle's own functions
(evaluated on float64 tensors).

OPSPEC restated:
  * nearest demosaic (RGGB -> BGR): every pixel of a 2 x 2 quad takes the quad's R and B; green is the sample of the
    pixel's own row (G1 on the even row, G2 on the odd row);
  * the bilateral works on samples x 255; per-image odd window k (radius k // 2), reflect-101 borders (index -1 -> 1);
  * colour distance: L1 over the three channels; weight exp(-(dy^2 + dx^2) / (2 ss^2) - dist^2 / (2 sc^2));
  * output code floor(clamp(v, 0, 255) + 0.5), returned as code / 255;
  * tail operators, parameters as the C ABI takes them: WB_MANUAL y = x * k (k = the gain, 5 * plugin parameter, no clip);
    GAMMA x^g with the linear toe below 1 / 1024; GTM_MANUAL the 4-segment curve through the knots of ROW 0 of its block;
    WB_QUADRATIC the 10-feature polynomial, clamped; GAIN3 y = clamp(x * k, 0, 1); SKIP aliases its input.
"""
import numpy as np
import torch

import isp_oracle as O

# RISP_OP_* of include/risp.h
OP_SKIP, OP_DEMOSAIC_NEAREST, OP_WB_MANUAL, OP_GAMMA, OP_GTM_MANUAL, OP_WB_QUADRATIC, OP_GAIN3 = range(7)
OP_NAMES = {OP_SKIP: 'skip', OP_WB_MANUAL: 'wb_manual', OP_GAMMA: 'gamma', OP_GTM_MANUAL: 'gtm_manual',
            OP_WB_QUADRATIC: 'wb_quadratic', OP_GAIN3: 'gain3'}
PARAM_WIDTH = {OP_SKIP: 0, OP_WB_MANUAL: 3, OP_GAMMA: 1, OP_GTM_MANUAL: 3, OP_WB_QUADRATIC: 30, OP_GAIN3: 3}


def _f64(t):
    return torch.as_tensor(np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t), dtype=torch.float64)


def demosaic(bay):
    """(N,1,H,W) RGGB -> (N,3,H,W) BGR, an index map (exact in any dtype)"""
    n, one, h, w = bay.shape
    assert one == 1 and h % 2 == 0 and w % 2 == 0
    yy = torch.arange(h).view(h, 1).expand(h, w)
    xx = torch.arange(w).view(1, w).expand(h, w)
    qy, qx = yy - yy % 2, xx - xx % 2                      # quad origin
    m = bay[:, 0]
    red = m[:, qy, qx]
    blue = m[:, qy + 1, qx + 1]
    green = m[:, yy, qx + 1 - yy % 2]                      # even row: (row, odd column); odd row: (row, even column)
    return torch.stack([blue, green, red], dim=1)


def _reflect101(i, n):
    i = np.abs(i)
    i = np.where(i >= n, 2 * n - 2 - i, i)
    assert i.min() >= 0 and i.max() < n, 'window radius must be smaller than the image'
    return i


def bilateral_raw(v, window, sigma_color, sigma_space):
    """v (N,3,H,W) float64 in the 0..255 domain -> the weighted mean IN FRONT of the clip-and-round, in codes"""
    v = _f64(v)
    n, c, h, w = v.shape
    assert c == 3
    window = [int(k) for k in _f64(window).tolist()]
    sc = _f64(sigma_color).reshape(-1).tolist()
    ss = _f64(sigma_space).reshape(-1).tolist()
    assert len(window) == len(sc) == len(ss) == n
    out = torch.empty_like(v)
    for i in range(n):
        k = window[i]
        assert k >= 1 and k % 2 == 1
        r = k // 2
        img = v[i]
        num = torch.zeros_like(img)
        den = torch.zeros((1, h, w), dtype=torch.float64)
        for dy in range(-r, r + 1):
            iy = torch.from_numpy(_reflect101(np.arange(h) + dy, h))
            for dx in range(-r, r + 1):
                ix = torch.from_numpy(_reflect101(np.arange(w) + dx, w))
                q = img[:, iy][:, :, ix]
                dist = (q - img).abs().sum(dim=0, keepdim=True)
                wgt = torch.exp(-(dy * dy + dx * dx) / (2.0 * ss[i] * ss[i]) - dist * dist / (2.0 * sc[i] * sc[i]))
                num += wgt * q
                den += wgt
        out[i] = num / den
    return out


def code(v):
    return torch.floor(v.clamp(0.0, 255.0) + 0.5)


def tie_distance(raw):
    """distance, in codes, of the unquantised value from the nearest rounding boundary of code(): the half-integers inside
    (0, 255).  Below 0 and above 255 the clip decides, and the nearest boundary is 0.5 / 254.5."""
    c = raw.clamp(0.0, 255.0)
    d = (c - torch.floor(c) - 0.5).abs()
    return torch.where(raw < 0.0, 0.5 - raw, torch.where(raw > 255.0, raw - 254.5, d))


def elementwise(op, x, par):
    """one tail stage on a float64 (N,3,H,W) tensor; par: its (N,P) block as the C ABI takes it (None for SKIP)"""
    if op == OP_SKIP:
        return x
    x, p = _f64(x), _f64(par)
    n = x.shape[0]
    assert tuple(p.shape) == (n, PARAM_WIDTH[op]), 'op %d: parameter block %s' % (op, tuple(p.shape))
    if op == OP_WB_MANUAL:
        return x * p.view(n, 3, 1, 1)
    if op == OP_GAMMA:
        return O.gamma_manual(x, p)
    if op == OP_GTM_MANUAL:
        return O.gtm_manual(x, p)
    if op == OP_WB_QUADRATIC:
        return O.wb_quadratic(x, p)
    if op == OP_GAIN3:
        return (x * p.view(n, 3, 1, 1)).clamp(0.0, 1.0)
    raise ValueError('op %r is not allowed after the stencil' % (op,))


def segment(x, from_bayer, window, sigma_color, sigma_space, ops, params):
    """-> (stage outputs, unquantised bilateral).

    x: (N,1,H,W) mosaic (from_bayer) or (N,3,H,W) BGR, samples in the [0,1] domain (any real value is admitted).
    Stage outputs, float64, in pipeline order as BilateralChainPlan.outs lists them: [demosaic,] bilateral (code / 255),
    then one entry per tail op (a SKIP entry is the very tensor in front of it).  The second value is the bilateral's
    weighted mean in codes before clip-and-round."""
    x = _f64(x)
    stages = []
    if from_bayer:
        x = demosaic(x)
        stages.append(x)
    raw = bilateral_raw(x * 255.0, window, sigma_color, sigma_space)
    cur = code(raw) / 255.0
    stages.append(cur)
    assert len(ops) == len(params)
    for op, par in zip(ops, params):
        cur = elementwise(op, cur, par)
        stages.append(cur)
    return stages, raw
