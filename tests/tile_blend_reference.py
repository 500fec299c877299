"""The tiled blend followed by the 8-bit conversion, restated in float32 numpy: the CPU yardstick of ``risp_tile_blend_u8``.

``blend_u8`` is the reference's ``patch2whole`` (utils/util_path_restore.py:108-134) written as what it is - a sequential
``+=`` per tile, in tile order, of ``patch * mask`` and of ``mask``, then ``/ count`` - followed by ``tensor2bgr``
(utils/util.py:87-94): ``* 255`` in float32, clip to [0, 255], truncate.  Every operation is one float32 operation, so the
bytes are defined without a tolerance; tests/test_serve_frame_cpu.py holds it to ``isp_oracle.patch2whole`` +
``isp_oracle.tensor2bgr_uint8`` on the golden tiling fixture, and tests/test_gpu_tile_blend_u8.py holds the kernel to it.
"""
import numpy as np


def ramp(n, e):
    """create_patch_mask's ramp: (i+1)/(e+1) on the first e entries, mirrored on the last e, 1 between; float32 division"""
    r = np.ones(n, np.float32)
    for i in range(e):
        r[i] = r[n - 1 - i] = np.float32(i + 1) / np.float32(e + 1)
    return r


def blend_u8(patches, positions, full, stride, reverse_channels=False, flip=0):
    """patches (T,C,h,w) float32, positions (T,2) (y,x) -> (H,W,C) uint8; ``reverse_channels`` and ``flip`` (bit 0 x, bit 1
    y) as ``risp_quantise_u8_flip`` takes them"""
    patches = np.asarray(patches, np.float32)
    t, c, h, w = patches.shape
    H, W = full
    eh, ew = (h - stride[0]) // 2, (w - stride[1]) // 2
    mask = np.minimum(ramp(h, eh)[:, None], ramp(w, ew)[None, :])
    acc = np.zeros((c, H, W), np.float32)
    cnt = np.zeros((H, W), np.float32)
    for p, (y, x) in zip(patches, np.asarray(positions)):
        acc[:, y:y + h, x:x + w] += p * mask
        cnt[y:y + h, x:x + w] += mask
    img = acc / cnt
    out = np.clip(img * np.float32(255), np.float32(0), np.float32(255)).astype(np.uint8)
    out = np.transpose(out, (1, 2, 0))
    if reverse_channels:
        out = out[:, :, ::-1]
    if flip & 2:
        out = out[::-1]
    if flip & 1:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)
