"""MIPI-packed RAW10 / RAW12 in numpy, straight from the formulas of include/risp.h - the yardstick of
tests/test_gpu_serve_packed.py and tests/test_raw_packed_reference_cpu.py.

    RAW10: pixels 4g .. 4g+3 of a row live in bytes 5g .. 5g+4:  P[4g+k] = (byte[5g+k] << 2) | ((byte[5g+4] >> 2k) & 3)
    RAW12: pixels 2g, 2g+1 live in bytes 3g .. 3g+2:             P[2g]   = (byte[3g]   << 4) | (byte[3g+2] & 15)
                                                                 P[2g+1] = (byte[3g+1] << 4) | (byte[3g+2] >> 4)

An image is H rows of ``stride`` bytes, stride >= W * bits / 8, W % 4 == 0; the bytes of a row behind W * bits / 8 are padding.
Frames are (..., H, W) integers one way and (..., H, stride) uint8 the other.  ``unpack_drop_low``, ``unpack_swapped_low`` and
``unpack_neighbour_high`` are wrong on purpose: the CPU tests show that the frames the GPU tests use tell them from ``unpack``."""
import numpy as np


def row_bytes(width, bits):
    assert bits in (10, 12) and width >= 4 and width % 4 == 0
    return width * bits // 8


def pack(u16, bits, stride=None, pad=None):
    """(..., H, W) samples below 2^bits -> (..., H, stride) uint8; ``stride`` defaults to W * bits / 8, the padding holds
    ``pad``: a byte value, or None for pseudo-random bytes"""
    p = np.asarray(u16).astype(np.int64)
    w = p.shape[-1]
    used = row_bytes(w, bits)
    stride = used if stride is None else stride
    assert stride >= used and p.min(initial=0) >= 0 and p.max(initial=0) < 1 << bits
    if pad is None:
        out = np.random.default_rng(stride * 7 + w).integers(0, 256, p.shape[:-1] + (stride,)).astype(np.uint8)
    else:
        out = np.full(p.shape[:-1] + (stride,), pad, dtype=np.uint8)
    if bits == 10:
        g = p.reshape(p.shape[:-1] + (w // 4, 4))
        grp = np.empty(p.shape[:-1] + (w // 4, 5), dtype=np.int64)
        grp[..., :4] = g >> 2
        grp[..., 4] = (g[..., 0] & 3) | (g[..., 1] & 3) << 2 | (g[..., 2] & 3) << 4 | (g[..., 3] & 3) << 6
    else:
        g = p.reshape(p.shape[:-1] + (w // 2, 2))
        grp = np.empty(p.shape[:-1] + (w // 2, 3), dtype=np.int64)
        grp[..., :2] = g >> 4
        grp[..., 2] = (g[..., 0] & 15) | (g[..., 1] & 15) << 4
    out[..., :used] = grp.reshape(p.shape[:-1] + (used,)).astype(np.uint8)
    return out


def _groups(u8, bits, width):
    b = np.asarray(u8)
    assert b.dtype == np.uint8 and b.shape[-1] >= row_bytes(width, bits)
    b = b[..., :row_bytes(width, bits)].astype(np.int64)
    return b.reshape(b.shape[:-1] + ((width // 4, 5) if bits == 10 else (width // 2, 3)))


def _unpack(u8, bits, width, low10, low12, high=lambda g, k: g[..., k]):
    g = _groups(u8, bits, width)
    if bits == 10:
        px = [high(g, k) << 2 | low10(g[..., 4], k) for k in range(4)]
    else:
        px = [high(g, k) << 4 | low12(g[..., 2], k) for k in range(2)]
    return np.stack(px, axis=-1).reshape(g.shape[:-2] + (width,)).astype(np.uint16)


def unpack(u8, bits, width):
    """(..., H, stride) uint8 -> (..., H, width) uint16, the definition"""
    return _unpack(u8, bits, width, lambda lo, k: lo >> (2 * k) & 3, lambda lo, k: lo >> (4 * k) & 15)


def unpack_drop_low(u8, bits, width):
    """wrong: ignores the shared low-bits byte"""
    return _unpack(u8, bits, width, lambda lo, k: 0 * lo, lambda lo, k: 0 * lo)


def unpack_swapped_low(u8, bits, width):
    """wrong: assigns the low-bit fields in reverse order"""
    return _unpack(u8, bits, width, lambda lo, k: lo >> (2 * (3 - k)) & 3, lambda lo, k: lo >> (4 * (1 - k)) & 15)


def unpack_neighbour_high(u8, bits, width):
    """wrong: takes the high byte of the neighbouring pixel of the group"""
    return _unpack(u8, bits, width, lambda lo, k: lo >> (2 * k) & 3, lambda lo, k: lo >> (4 * k) & 15, high=lambda g, k: g[..., k ^ 1])


def low_bit_frame(n, h, w, seed):
    """samples uniform in 0 .. 15 (white level 15): every RAW12 high byte is 0 and a RAW10 high byte holds s >> 2 alone, so a
    decoder that drops or permutes the low-bits bytes loses what tells the samples apart"""
    return np.random.default_rng(seed).integers(0, 16, (n, h, w)).astype(np.uint16)


def full_range_frame(n, h, w, bits, seed):
    """samples uniform in 0 .. 2^bits - 1 (white level 2^bits - 1), the extremes present"""
    f = np.random.default_rng(seed).integers(0, 1 << bits, (n, h, w)).astype(np.uint16)
    f[0, 0, 0], f[0, -1, -1] = (1 << bits) - 1, 0
    return f
