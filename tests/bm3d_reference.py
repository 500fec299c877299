"""Float64 restatement of the build-defined BM3D OPSPEC (include/risp.h "'bm3d'").

Test-only: the HIP kernels of reconfigisp_amd/csrc/risp_bm3d.hip are checked against this file.  Integer block
matching is exact (the group table must match the kernel's bit for bit); the transforms, shrinkage and aggregation
run in float64 with the float64 forms of the constants the kernels hold as fp32.

    bm3d(x, sigma, n1, cspace, wtransform, radius, in_scale=1., out_div=1.) -> (y, groups)

x: (N,3,H,W) BGR float tensor, 0..255 after in_scale; the five parameters are per-image sequences (or scalars).
y: (N,3,H,W) float32 codes / out_div (out_div < 0: the unquantised value / |out_div|).
groups: (N, table_rows(H, W), 17) int32 - count N2, then the N2 member corners y*W+x (the reference block first),
-1 padded; rows beyond the image's own grid (an image with n1 = 8) are (0, -1, ...).
"""
import numpy as np
import torch

STEP = 3                 # reference-block grid stride
MAX_GROUP = 16
KEEP_PER_PIXEL = 22500   # D <= 22500 * n1^2 on S = B+G+R (2500 per pixel on the (R+G+B)/3 scale)
HARD = 2.7               # step 1 keeps |c| > 2.7 * sigma_c
KAISER_BETA = 2.0
TABLE_COLS = 1 + MAX_GROUP


def grid(n, n1):
    """top-left corners of the reference blocks along one axis: 0, 3, 6, ... and n - n1"""
    return sorted(set(range(0, n - n1 + 1, STEP)) | {n - n1})


def refs(h, w, n1):
    return len(grid(h, n1)) * len(grid(w, n1))


def table_rows(h, w):
    """rows of the group table: the grid of the smaller block (the larger grid)"""
    return refs(h, w, 4)


def dct_matrix(n):
    k, i = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    t = np.cos(np.pi * (2 * i + 1) * k / (2 * n)) * np.sqrt(2.0 / n)
    t[0] = np.sqrt(1.0 / n)
    return t


def haar_matrix(n):
    """orthonormal Haar, full decomposition: H_2m = [H_m (x) (1, 1); I_m (x) (1, -1)] / sqrt(2)"""
    if n == 1:
        return np.ones((1, 1))
    h = haar_matrix(n // 2)
    return np.vstack([np.kron(h, [1., 1.]), np.kron(np.eye(n // 2), [1., -1.])]) / np.sqrt(2.)


def colour_matrix(cspace):
    """rows = output channels, columns = (B, G, R)"""
    if cspace == 0:      # orthonormal opponent
        s3, s2, s6 = np.sqrt(3.), np.sqrt(2.), np.sqrt(6.)
        rgb = np.array([[1 / s3, 1 / s3, 1 / s3], [1 / s2, 0., -1 / s2], [1 / s6, -2 / s6, 1 / s6]])
    else:                # BT.601 full-range YCbCr, no offsets
        rgb = np.array([[.299, .587, .114], [-.168736, -.331264, .5], [.5, -.418688, -.081312]])
    return rgb[:, ::-1].copy()


def _per_image(v, n, dtype):
    a = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=dtype).reshape(-1)
    return np.repeat(a, n) if a.size == 1 and n > 1 else a


def codes(x, in_scale=1.0):
    """q = floor(clamp(x * in_scale, 0, 255) + 0.5), the product formed in fp32 as on the device"""
    v = (x.detach().cpu().float() * np.float32(in_scale)).double().numpy()
    return np.floor(np.clip(v, 0., 255.) + 0.5)


def match(q, n1, radius):
    """q: (3,H,W) codes -> list of member corner lists (y, x), one per reference block in row-major order"""
    h, w = q.shape[1:]
    s = q.sum(0).astype(np.int64)
    blocks = np.lib.stride_tricks.sliding_window_view(s, (n1, n1)).reshape(h - n1 + 1, w - n1 + 1, n1 * n1)
    gy, gx = np.array(grid(h, n1)), np.array(grid(w, n1))
    ref = blocks[gy][:, gx]                                           # (ny, nx, n1^2)
    keys = []
    big = np.iinfo(np.int64).max
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            cy, cx = gy + dy, gx + dx
            vy, vx = (cy >= 0) & (cy <= h - n1), (cx >= 0) & (cx <= w - n1)
            cand = blocks[np.clip(cy, 0, h - n1)][:, np.clip(cx, 0, w - n1)]
            d = ((cand - ref) ** 2).sum(-1)
            ok = vy[:, None] & vx[None, :] & (d <= KEEP_PER_PIXEL * n1 * n1)
            key = (d << 32) + (np.clip(cy, 0, None)[:, None] << 16) + np.clip(cx, 0, None)[None, :]
            key = np.where(ok, key, big)
            if dy == 0 and dx == 0:
                key = np.full_like(key, -1)                            # the reference block is rank 0
            keys.append(key.reshape(-1))
    keys = np.sort(np.stack(keys, 1), 1)
    out = []
    for row in keys:
        kept = int((row != big).sum())
        n2 = 1 << (min(kept, MAX_GROUP).bit_length() - 1)
        out.append(row[:n2])
    grid_pairs = [(y, x) for y in gy for x in gx]
    groups = []
    for (ry, rx), row in zip(grid_pairs, out):
        members = [(int(ry), int(rx))] + [(int((k >> 16) & 0xffff), int(k & 0xffff)) for k in row[1:]]
        groups.append(members)
    return groups


def _transform3d(g, t, hg):
    """g (M, N2, n1, n1) -> 3D coefficients: t X t^T per block, then the Haar hg along the group"""
    c = t @ g @ t.T
    return (hg @ c.reshape(c.shape[0], c.shape[1], -1)).reshape(c.shape)


def _inverse3d(c, t, hg):
    x = (hg.T @ c.reshape(c.shape[0], c.shape[1], -1)).reshape(c.shape)
    return t.T @ x @ t


def _filter(noisy, pilot, groups, n1, t, sig_c, kaiser, step):
    """one filtering pass + aggregation in the colour space: noisy / pilot (3,H,W) -> estimate (3,H,W)"""
    _, h, w = noisy.shape
    num, den = np.zeros((3, h * w)), np.zeros(h * w)
    kk = np.outer(kaiser, kaiser).reshape(-1)
    iy, ix = np.meshgrid(np.arange(n1), np.arange(n1), indexing='ij')
    for n2 in sorted({len(g) for g in groups}):
        sel = [g for g in groups if len(g) == n2]
        cy = np.array([[m[0] for m in g] for g in sel])                 # (M, N2)
        cx = np.array([[m[1] for m in g] for g in sel])
        pix = ((cy[:, :, None, None] + iy) * w + cx[:, :, None, None] + ix)   # (M, N2, n1, n1)
        hg = haar_matrix(n2)
        wsum = np.zeros(len(sel))
        ests = []
        for c in range(3):
            z = noisy[c].reshape(-1)[pix]
            tz = _transform3d(z, t, hg)
            if step == 1:
                keep = np.abs(tz) > HARD * sig_c[c]
                est = _inverse3d(np.where(keep, tz, 0.), t, hg)
                wsum += sig_c[c] ** 2 * np.maximum(keep.sum((1, 2, 3)), 1)
            else:
                tp = _transform3d(pilot[c].reshape(-1)[pix], t, hg)
                wien = tp * tp / (tp * tp + sig_c[c] ** 2)
                est = _inverse3d(wien * tz, t, hg)
                wsum += sig_c[c] ** 2 * np.maximum((wien * wien).sum((1, 2, 3)), 1.)
            ests.append(est)
        wgt = 1.0 / wsum
        flat = pix.reshape(len(sel), -1)
        for c in range(3):
            np.add.at(num[c], flat, (wgt[:, None] * ests[c].reshape(len(sel), -1) * np.tile(kk, n2)))
        np.add.at(den, flat, wgt[:, None] * np.tile(kk, n2))
    return (num / den).reshape(3, h, w)


def bm3d_image(q, sigma, n1, cspace, wtransform, radius):
    """q: (3,H,W) float64 codes -> (unquantised BGR estimate (3,H,W), groups)"""
    groups = match(q, n1, radius)
    if sigma < 1e-3:
        return q.copy(), groups
    m = colour_matrix(cspace)
    sig_c = sigma * np.linalg.norm(m, axis=1)
    t = dct_matrix(n1) if wtransform == 0 else haar_matrix(n1)
    kaiser = np.kaiser(n1, KAISER_BETA)
    z = np.einsum('ck,khw->chw', m, q)
    basic = _filter(z, None, groups, n1, t, sig_c, kaiser, 1)
    final = _filter(z, basic, groups, n1, t, sig_c, kaiser, 2)
    return np.einsum('ck,khw->chw', np.linalg.inv(m), final), groups


def bm3d(x, sigma, n1, cspace, wtransform, radius, in_scale=1.0, out_div=1.0):
    n, _, h, w = x.shape
    sigma = _per_image(sigma, n, np.float32).astype(np.float64)
    n1, cspace = _per_image(n1, n, np.int64), _per_image(cspace, n, np.int64)
    wtransform, radius = _per_image(wtransform, n, np.int64), _per_image(radius, n, np.int64)
    q = codes(x, in_scale)
    ys = np.zeros((n, 3, h, w), np.float32)
    table = np.full((n, table_rows(h, w), TABLE_COLS), -1, np.int32)
    table[:, :, 0] = 0
    inv = np.float32(1.0) / np.float32(abs(out_div))
    for i in range(n):
        v, groups = bm3d_image(q[i], sigma[i], int(n1[i]), int(cspace[i]), int(wtransform[i]), int(radius[i]))
        for r, g in enumerate(groups):
            table[i, r, 0] = len(g)
            table[i, r, 1:1 + len(g)] = [yy * w + xx for yy, xx in g]
        if sigma[i] < 1e-3:
            ys[i] = v.astype(np.float32) * inv
        elif out_div > 0:
            ys[i] = np.floor(np.clip(v, 0., 255.) + 0.5).astype(np.float32) * inv
        else:
            ys[i] = (v / abs(out_div)).astype(np.float32)
    return torch.from_numpy(ys), torch.from_numpy(table)


def group_table(x, n1, radius, in_scale=1.0):
    """the group table alone (matching only): (N, table_rows(H, W), 17) int32"""
    n, _, h, w = x.shape
    n1, radius = _per_image(n1, n, np.int64), _per_image(radius, n, np.int64)
    q = codes(x, in_scale)
    table = np.full((n, table_rows(h, w), TABLE_COLS), -1, np.int32)
    table[:, :, 0] = 0
    for i in range(n):
        for r, g in enumerate(match(q[i], int(n1[i]), int(radius[i]))):
            table[i, r, 0] = len(g)
            table[i, r, 1:1 + len(g)] = [yy * w + xx for yy, xx in g]
    return torch.from_numpy(table)
