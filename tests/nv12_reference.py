"""The NV12 output format of the serving path, restated in numpy int64 - the yardstick of tests/test_gpu_serve_nv12.py.

For an image of H x W pixels, H and W even, the NV12 image is (3H/2, W) uint8: rows 0 .. H-1 are the Y plane, row H + j
holds U(j,0) V(j,0) U(j,1) V(j,1) ... for the W/2 chroma sites of quad row j.  With B, G, R the 8-bit codes of a pixel and
a matrix of twelve integers cy[4], cu[4], cv[4], each row kR, kG, kB, offset:

    Y(y,x) = (cy0*R + cy1*G + cy2*B + cy3) >> 8                     per pixel
    Rm     = (R00 + R01 + R10 + R11 + 2) >> 2  (Gm, Bm likewise)    per 2 x 2 quad: the rounded mean of the CODES
    U(j,i) = (cu0*Rm + cu1*Gm + cu2*Bm + cu3) >> 8
    V(j,i) = (cv0*Rm + cv1*Gm + cv2*Bm + cv3) >> 8

The table below is this file's own copy of the presets (not imported from the package)."""
import numpy as np

TABLE = {
    'bt601_full': (77, 150, 29, 128, -43, -84, 127, 32896, 127, -106, -21, 32896),
    'bt601_video': (66, 129, 25, 4224, -38, -74, 112, 32896, 112, -94, -18, 32896),
    'bt709_full': (54, 183, 19, 128, -29, -98, 127, 32896, 127, -115, -12, 32896),
    'bt709_video': (47, 157, 16, 4224, -26, -86, 112, 32896, 112, -102, -10, 32896),
}


def accepted(coef):
    """the acceptance rule: per row |k| <= 256, offset + 255 * (sum of positive k) <= 65535, offset + 255 * (sum of negative
    k) >= 0 - every sum is then in 0 .. 65535 for all codes"""
    coef = [int(k) for k in coef]
    if len(coef) != 12:
        return False
    for r in range(3):
        k, off = coef[4 * r:4 * r + 3], coef[4 * r + 3]
        if any(abs(v) > 256 for v in k):
            return False
        if off + 255 * sum(v for v in k if v > 0) > 65535 or off + 255 * sum(v for v in k if v < 0) < 0:
            return False
    return True


def planes(img, channels='bgr'):
    """(N,H,W,3) uint8 -> R, G, B as (N,H,W) int64"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 4 and img.shape[3] == 3 and channels in ('bgr', 'rgb')
    v = img.astype(np.int64)
    return (v[..., 0], v[..., 1], v[..., 2]) if channels == 'rgb' else (v[..., 2], v[..., 1], v[..., 0])


def dot(k, r, g, b):
    """one matrix row on codes; the sum must lie in 0 .. 65535"""
    s = k[0] * r + k[1] * g + k[2] * b + k[3]
    assert s.min() >= 0 and s.max() <= 65535, 'the matrix leaves 0 .. 65535'
    return s >> 8


def quad_mean(c):
    """(N,H,W) codes -> (N,H/2,W/2) rounded means of the 2 x 2 quads"""
    return (c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2] + 2) >> 2


def pack(y, u, v):
    """Y (N,H,W), U and V (N,H/2,W/2) -> (N,3H/2,W) uint8"""
    n, h, w = y.shape
    out = np.empty((n, h + h // 2, w), dtype=np.uint8)
    out[:, :h] = y
    out[:, h:, 0::2] = u
    out[:, h:, 1::2] = v
    return out


def nv12(img, coef, channels='bgr'):
    """(N,H,W,3) uint8 packed images and twelve integers -> (N,3H/2,W) uint8"""
    coef = [int(k) for k in coef]
    assert len(coef) == 12
    r, g, b = planes(img, channels)
    assert r.shape[1] % 2 == 0 and r.shape[2] % 2 == 0
    rm, gm, bm = quad_mean(r), quad_mean(g), quad_mean(b)
    return pack(dot(coef[0:4], r, g, b), dot(coef[4:8], rm, gm, bm), dot(coef[8:12], rm, gm, bm))
