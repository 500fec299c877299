"""Float64 restatement of the classical Origin kernels (risp_origin_demosaic / _bilateral / _median / _fastnlm / _tonemap,
include/risp.h "Classical, non-differentiable Origin kernels").

Truth of tests/test_origin_reference_cpu.py and tests/test_gpu_origin_space.py.  Plain torch / numpy on the CPU, no HIP.
It is a SECOND statement of the OPSPEC beside oracle/isp_oracle.py: borders are explicit reflect-101 indices, windows a
gather per tap, the demosaic selects by site parity (strided assignment) - nothing here calls the oracle's padding, its
unfold or its masks.  The bilateral in float64 IS fused_segment_reference.bilateral_raw.

Every function takes ``v``, the samples AFTER the multiplication by in_scale (the 0..255 domain; see scaled()), and
returns the value IN FRONT of the clip-and-round, in codes (the median: the code itself).  ``_variant`` names a deliberately WRONG
reading of the OPSPEC (tests/test_origin_reference_cpu.py shows that the rule rejects each); None everywhere else.  ``dtype``: torch.float64 is
the truth; torch.float32 evaluates the same expressions in float32 (what fp32 arithmetic itself costs - the yardstick
of the tie budget, never a verdict).

OPSPEC restated:
  * demosaic (RGGB -> BGR), reflect-101 (keeps the Bayer phase).  bilinear: a missing colour is the mean of the nearest
    2 or 4 samples of it.  laplacian: Malvar-He-Cutler, coefficients / 8.
  * bilateral: per-image odd window, L1 colour distance, exp(-(dy^2 + dx^2) / (2 ss^2) - dist^2 / (2 sc^2)).
  * median: on codes q = floor(clamp(v, 0, 255) + 0.5); the smallest code whose rank reaches size * size / 2 + 1.
  * fastnlm: per image block b, search s, decay h: for every search offset the squared distance of the two b x b patches
    over the three channels, BOTH read from the reflected image (one reflection of the final index); weight
    exp(-(d2 / (3 b^2)) / h^2); one reciprocal per pixel.
  * tone curves on x = max(v, 0) / 255.  Reinhard: L = 0.114 b + 0.587 g + 0.299 r, key max(middle_grey, 0.01) over the
    per-image exp(mean(log(L + 1e-4))), Lw = 10 max(white_point, 0.01), x * Ld / max(L, 1e-6).  Crysis:
    1 - exp(-x * 0.5 / (lum_adapted + 0.05)).  Hable: f(x * exposure_bias) / f(11.2 max(white_point, 0.01)).
  * white-world: gain_c = 1 + ratio * (M / max_c - 1), max_c the channel maximum of the UNCLAMPED v floored at 1e-3.
  * output: code floor(clamp(value, 0, 255) + 0.5), stored as fp32(code) * fp32(1 / out_div); out_div < 0 stores
    fp32(value) * fp32(1 / |out_div|) instead (stored_code / stored_raw below).
"""
import numpy as np
import torch

from fused_segment_reference import _reflect101, bilateral_raw, code, tie_distance  # noqa: F401  (re-exported)

REINHARD, CRYSIS, FILMIC, WHITEWORLD = range(4)        # the mode of risp_origin_tonemap
F64, F32 = torch.float64, torch.float32


def _t(v, dtype):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().to(dtype)
    return torch.as_tensor(np.asarray(v), dtype=dtype)


def scaled(x, in_scale, dtype=F64):
    """the fp32 samples as the kernels see them: multiplied by in_scale first (in ``dtype``)"""
    return _t(x, dtype) * in_scale


def _idx(n, d):
    return torch.from_numpy(_reflect101(np.arange(n) + d, n))


def _tap(img, dy, dx):
    """img (..., H, W) -> the image of the neighbour (y + dy, x + dx), reflect-101"""
    h, w = img.shape[-2:]
    return img[..., _idx(h, dy), :][..., _idx(w, dx)]


# ---------------------------------------------------------------------------------------------------- demosaic
def demosaic(bay, laplacian, dtype=F64, _variant=None):
    """bay (N,1,H,W), RGGB, H and W even -> (N,3,H,W) BGR"""
    m = _t(bay, dtype)[:, 0]
    n, h, w = m.shape
    assert h % 2 == 0 and w % 2 == 0 and h >= 4 and w >= 4
    s = lambda dy, dx: _tap(m, dy, dx)
    c = m
    cross = s(-1, 0) + s(1, 0) + s(0, -1) + s(0, 1)
    diag = s(-1, -1) + s(-1, 1) + s(1, -1) + s(1, 1)
    hor, ver = s(0, -1) + s(0, 1), s(-1, 0) + s(1, 0)
    if laplacian:
        fh, fv = s(0, -2) + s(0, 2), s(-2, 0) + s(2, 0)
        far = fh + fv
        g_rb = (4 * c + 2 * cross - far) / 8
        rb_hor = (5 * c + 4 * hor - diag - fh + 0.5 * fv) / 8      # the colour left and right of a green
        rb_ver = (5 * c + 4 * ver - diag - fv + 0.5 * fh) / 8      # the colour above and below a green
        rb_diag = (6 * c + 2 * diag - 1.5 * far) / 8               # the opposite colour at an R or B site
    else:
        g_rb, rb_hor, rb_ver, rb_diag = cross / 4, hor / 2, ver / 2, diag / 4
    if _variant == 'swap':
        rb_hor, rb_ver = rb_ver, rb_hor
    out = torch.empty((n, 3, h, w), dtype=dtype)
    B, G, R = out[:, 0], out[:, 1], out[:, 2]
    ee, eo, oe, oo = (np.s_[:, 0::2, 0::2], np.s_[:, 0::2, 1::2], np.s_[:, 1::2, 0::2], np.s_[:, 1::2, 1::2])
    R[ee], G[ee], B[ee] = c[ee], g_rb[ee], rb_diag[ee]             # a red site
    G[eo], R[eo], B[eo] = c[eo], rb_hor[eo], rb_ver[eo]            # green on a red row
    G[oe], R[oe], B[oe] = c[oe], rb_ver[oe], rb_hor[oe]            # green on a blue row
    B[oo], G[oo], R[oo] = c[oo], g_rb[oo], rb_diag[oo]             # a blue site
    return out.flip(1) if _variant == 'rgb' else out


# ---------------------------------------------------------------------------------------------------- bilateral
def bilateral(v, window, sc, ss, dtype=F64, _variant=None):
    if dtype == F64 and _variant is None:
        return bilateral_raw(_t(v, F64), window, sc, ss)
    v = _t(v, dtype)                                               # bilateral_raw's expressions in ``dtype``
    window = [int(k) for k in _t(window, F64).tolist()]
    sc, ss = _t(sc, F64).reshape(-1).tolist(), _t(ss, F64).reshape(-1).tolist()
    out = torch.empty_like(v)
    for i, k in enumerate(window):
        assert k >= 1 and k % 2 == 1
        r, img = k // 2, v[i]
        num, den = torch.zeros_like(img), torch.zeros_like(img[:1])
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                q = _tap(img, dy, dx)
                dist = (q - img).abs().sum(dim=0, keepdim=True)
                if _variant == 'l2':
                    dist = ((q - img) ** 2).sum(dim=0, keepdim=True).sqrt()
                wgt = torch.exp(-(dy * dy + dx * dx) / (2.0 * ss[i] * ss[i]) - dist * dist / (2.0 * sc[i] * sc[i]))
                num += wgt * q
                den += wgt
        out[i] = num * (1.0 / den)
    return out


# ---------------------------------------------------------------------------------------------------- median
def median(v, size, dtype=F64, _variant=None):
    q = _t(v, dtype) if _variant == 'unquantised' else code(_t(v, dtype))
    k = int(size)
    assert k >= 1 and k % 2 == 1
    r = k // 2
    taps = torch.stack([_tap(q, dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)])
    need = (k * k) // 2 + 1                                        # the rank, counted from 1
    return torch.from_numpy(np.partition(taps.numpy(), need - 1, axis=0)[need - 1])


# ---------------------------------------------------------------------------------------------------- non-local means
def _reflected(img, R):
    """(3,H,W) -> (3,H+2R,W+2R): every index of the halo reflected ONCE (needs R < H, W)"""
    h, w = img.shape[-2:]
    iy = torch.from_numpy(_reflect101(np.arange(-R, h + R), h))
    ix = torch.from_numpy(_reflect101(np.arange(-R, w + R), w))
    return img[:, iy][:, :, ix]


def fastnlm(v, block, search, decay, dtype=F64, _variant=None):
    """a box sum (rows, then columns: sums of non-negative terms) over the per-offset squared differences"""
    v = _t(v, dtype)
    n, c, h, w = v.shape
    block, search = [int(b) for b in _t(block, F64).tolist()], [int(s) for s in _t(search, F64).tolist()]
    decay = _t(decay, F64).reshape(-1).tolist()
    out = torch.empty_like(v)
    for i in range(n):
        b, rb, rs, hd = block[i], block[i] // 2, search[i] // 2, decay[i]
        R = rb + rs
        P = _reflected(v[i], R)
        win = lambda y0, x0, hh, ww: P[:, R + y0: R + y0 + hh, R + x0: R + x0 + ww]
        base = win(-rb, -rb, h + 2 * rb, w + 2 * rb)
        if _variant == 'centre':             # the centre patch from an edge-repeated image instead
            base = v[i][:, np.clip(np.arange(-rb, h + rb), 0, h - 1)][:, :, np.clip(np.arange(-rb, w + rb), 0, w - 1)]
        norm = {None: 3 * b * b, 'centre': 3 * b * b, 'no3': b * b, 'norm1': 3 * min(b, 3) ** 2}[_variant]
        num, den = torch.zeros_like(v[i]), torch.zeros((1, h, w), dtype=dtype)
        for sy in range(-rs, rs + 1):
            for sx in range(-rs, rs + 1):
                diff = win(sy - rb, sx - rb, h + 2 * rb, w + 2 * rb) - base
                e = (diff * diff).sum(dim=0)                        # (H + 2 rb, W + 2 rb)
                rows = sum(e[oy: oy + h] for oy in range(b))        # (H, W + 2 rb)
                d2 = sum(rows[:, ox: ox + w] for ox in range(b))    # (H, W)
                wgt = torch.exp(-(d2 / norm) / (hd * hd)).unsqueeze(0)
                num += wgt * win(sy, sx, h, w)
                den += wgt
        out[i] = num * (1.0 / den)
    return out


def fastnlm_direct(v, block, search, decay):
    """the four-loop form, float64, pixel by pixel with reflected indices (for small images: the CPU test compares it
    with fastnlm once)"""
    v = _t(v, F64).numpy()
    n, c, h, w = v.shape
    out = np.empty_like(v)
    ry = lambda y: int(_reflect101(np.array([y]), h)[0])
    rx = lambda x: int(_reflect101(np.array([x]), w)[0])
    for i in range(n):
        b, rb, rs, hd = int(block[i]), int(block[i]) // 2, int(search[i]) // 2, float(decay[i])
        for y in range(h):
            for x in range(w):
                num, den = np.zeros(3), 0.0
                for sy in range(-rs, rs + 1):
                    for sx in range(-rs, rs + 1):
                        d2 = 0.0
                        for oy in range(-rb, rb + 1):
                            for ox in range(-rb, rb + 1):
                                d = v[i, :, ry(y + oy + sy), rx(x + ox + sx)] - v[i, :, ry(y + oy), rx(x + ox)]
                                d2 += float((d * d).sum())
                        wgt = np.exp(-(d2 / (3 * b * b)) / (hd * hd))
                        num += wgt * v[i, :, ry(y + sy), rx(x + sx)]
                        den += wgt
                out[i, :, y, x] = num * (1.0 / den)
    return torch.from_numpy(out)


# ---------------------------------------------------------------------------------------------------- tone curves
def _hable(t):
    A, B, C, D, E, F = 0.15, 0.50, 0.10, 0.20, 0.02, 0.30
    return (t * (A * t + C * B) + D * E) / (t * (A * t + B) + D * F) - E / F


def tonemap(v, mode, a, b=None, dtype=F64, _variant=None):
    """mode / a / b as risp_origin_tonemap takes them: REINHARD (white_point, middle_grey), CRYSIS (lum_adapted),
    FILMIC (white_point, exposure_bias)"""
    v = _t(v, dtype)
    n = v.shape[0]
    col = lambda p: _t(p, dtype).reshape(n, 1, 1, 1)
    x = v.clamp_min(0.0) / 255.0
    if mode == REINHARD:
        key, lw = col(b).clamp_min(0.01), col(a).clamp_min(0.01) * (1.0 if _variant == 'lw_white' else 10.0)
        L = 0.114 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.299 * x[:, 2:3]
        lavg = torch.exp(torch.log(L + (1e-30 if _variant == 'no_eps' else 1e-4)).mean(dim=(1, 2, 3), keepdim=True))
        ls = key * L / lavg
        out = x * (ls * (1.0 + ls / (lw * lw)) / (1.0 + ls) / L.clamp_min(1e-6))
    elif mode == CRYSIS:
        out = 1.0 - torch.exp(-x * (0.5 / (col(a) + (1e-30 if _variant == 'no_005' else 0.05))))
    elif mode == FILMIC:
        out = _hable(x * col(b)) / _hable(col(a).clamp_min(0.01) * (1.0 if _variant == 'no_112' else 11.2))
    else:
        raise ValueError(mode)
    return out * 255.0


def whiteworld(v, ratio, dtype=F64, _variant=None):
    v = _t(v, dtype)
    n = v.shape[0]
    mx = v.amax(dim=(2, 3), keepdim=True).clamp_min(1e-3)           # of the unclamped samples
    if _variant == 'means':
        mx = v.mean(dim=(2, 3), keepdim=True).clamp_min(1e-3)
    big = mx.amax(dim=1, keepdim=True)
    return v * (1.0 + _t(ratio, dtype).reshape(n, 1, 1, 1) * (big / mx - 1.0))


# ---------------------------------------------------------------------------------------------------- the stored forms
def rinv(out_div):
    """fp32(1 / |out_div|): every output is MULTIPLIED by it (risp.h)"""
    return np.float32(1.0) / np.float32(abs(out_div))


def stored_code(codes, out_div):
    """fp32 tensor the code form stores for these codes"""
    return torch.from_numpy(codes.numpy().astype(np.float32) * rinv(out_div))


def stored_raw(value, out_div):
    """fp32 tensor the raw form stores for a value computed in fp32"""
    return torch.from_numpy(value.numpy().astype(np.float32) * rinv(out_div))
