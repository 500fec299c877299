"""The per-image reductions (risp_reduce.hip, risp_condfc.hip, risp_pixel_loss / risp_local_global_l2 of risp_step.hip),
restated plainly: numpy, float64 unless a ``dtype`` says otherwise, one function per entry point.  Each restates the
operation, not the kernel: no grids, no partial sums, no summation order.  Checked without a GPU against independent
implementations by tests/test_reduce_reference_cpu.py.

Where the operation itself fixes an fp32 step, that step is taken in fp32 here too: the bin of the histogram is
floor(fp32(v) * fp32(bins)) (torch.histc on float input), the 8-bit code of the squared error is the truncated fp32
product v * 255 (tensor2bgr's numpy arithmetic), and a mean handed on as data is fp32(sum) * fp32(1 / HW).
"""
import numpy as np

F32, F64 = np.float32, np.float64
GRAY_EPS = 1e-6


def channel_stats(x):
    """x (P, HW) -> min, max, sum and the FIRST row-major index of the minimum and of the maximum, per plane"""
    x = np.asarray(x, F64)
    return dict(mn=x.min(1), mx=x.max(1), sum=x.sum(1), imn=x.argmin(1), imx=x.argmax(1))    # numpy: the first occurrence


def stats_bwd(gx, g_min, g_mean, g_max, arg, C=1, gstride=1, dtype=F64):
    """gx (P, HW) + g_mean / HW everywhere, + g_min at the first argmin, + g_max at the first argmax (in that order, onto
    what gx holds).  The gradient of plane n * C + c sits at g_*[n * gstride + c]; arg (P, 2).  Written out by hand:
    autograd would split a tie.  dtype = float32 gives the three fp32 additions per element to the bit."""
    out = np.array(gx, dtype)
    P, HW = out.shape
    inv = dtype(1) / dtype(HW)
    for p in range(P):
        gi = (p // C) * gstride + p % C
        if g_mean is not None:
            out[p] = out[p] + dtype(g_mean[gi]) * inv
        if g_min is not None:
            out[p, arg[p, 0]] = out[p, arg[p, 0]] + dtype(g_min[gi])
        if g_max is not None:
            out[p, arg[p, 1]] = out[p, arg[p, 1]] + dtype(g_max[gi])
    return out


def grayworld_gains(sums, HW, dtype=F64):
    """oracle/isp_oracle.py::grayworld's gain: sums (N, 3) -> gray / max(m_c, eps), m = sums / HW, gray = mean_c m_c"""
    m = np.asarray(sums, dtype) * (dtype(1) / dtype(HW))
    gray = (m[:, 0] + m[:, 1] + m[:, 2]) / dtype(3)
    return gray[:, None] / np.maximum(m, dtype(GRAY_EPS))


def grayworld_gains_bwd(sums, gk, HW):
    """gk = dL / d gain (N, 3) -> dL / d mean (N, 3); clamp_min passes the gradient where m >= eps"""
    m = np.asarray(sums, F64) / HW
    gk = np.asarray(gk, F64)
    mc = np.maximum(m, GRAY_EPS)
    gray = m.mean(1, keepdims=True)
    common = (gk / mc).sum(1, keepdims=True) / 3.0
    own = np.where(m >= GRAY_EPS, gk * gray / (mc * mc), 0.0)
    return common - own


def srcnn_cvals(mn, sums, mx, pv, HW):
    """the SRCNNRes broadcast row [min(3) | mean(3) | max(3) | params(P)] per image, the mean as fp32(sum) * fp32(1 / HW);
    mn, sums, mx (N, 3) fp32, pv (N, P) fp32 -> (N, 9 + P) fp32: copies and one fp32 product, so exact"""
    mean = np.asarray(sums, F32) * (F32(1) / F32(HW))
    return np.concatenate([np.asarray(mn, F32), mean, np.asarray(mx, F32), np.asarray(pv, F32).reshape(len(mean), np.size(pv) // len(mean))], 1)


def srcnn_case_table(cvals, rcase):
    """cvals (N, 9 + P) @ rcase (9 + P, M)"""
    return np.asarray(cvals, F64) @ np.asarray(rcase, F64)


def hist_bin(x, bins):
    """the bin of each fp32 input, -1 where torch.histc(x, bins, 0, 1) ignores it (outside [0, 1], NaN)"""
    x = np.asarray(x, F32)
    ok = (x >= 0) & (x <= 1)                                    # NaN compares false
    pos = (np.where(ok, x, F32(0)) * F32(bins)).astype(np.int64)              # the fp32 product, truncated
    return np.where(ok, np.minimum(pos, bins - 1), -1)


def histc(x, bins):
    """x (P, HW) -> raw counts (P, bins)"""
    b = hist_bin(x, bins)
    return np.stack([np.bincount(r[r >= 0], minlength=bins) for r in b]).astype(F64)


def mix(outs, w, gy, dtype=F64):
    """y = sum_k w_k o_k, gw_k = <gy, o_k>, go_k = w_k gy"""
    o = [np.asarray(v, dtype) for v in outs]
    w, gy = np.asarray(w, dtype), np.asarray(gy, dtype)
    y = np.zeros_like(o[0])
    for k in range(len(o)):
        y = y + o[k] * w[k]
    return dict(y=y, gw=np.array([np.dot(gy.astype(F64), v.astype(F64)) for v in o]), go=[gy * w[k] for k in range(len(o))])


def plane_sums(x, c0, nc):
    """x (N, C, HW) -> sums over HW of channels c0 .. c0 + nc - 1: (N, nc)"""
    return np.asarray(x, F64)[:, c0: c0 + nc].sum(2)


def u8_code(v):
    """tensor2bgr's 8-bit code: clip(fp32(v) * fp32(255), 0, 255) truncated"""
    t = np.asarray(v, F32) * F32(255)
    return np.floor(np.clip(t, F32(0), F32(255))).astype(np.int64)


def sse_uint8(a, b):
    """sum over all elements of (code(a) / 255 - code(b) / 255)^2"""
    d = (u8_code(a) - u8_code(b)).astype(F64) / 255.0
    return float((d * d).sum())


def psnr_from_sse(sse, numel):
    """oracle/isp_oracle.py::psnr_uint8 (peak 1 after / 255)"""
    import math
    mse = sse / numel
    return float('inf') if mse == 0 else 10 * math.log10(1.0 / mse)


def fc_layout(widths):
    """offsets of (W_l, b_l) in the flat vector and of the global scalar"""
    at, offs = 0, []
    for fi, fo in zip(widths[:-1], widths[1:]):
        offs.append((at, at + fi * fo))
        at += fi * fo + fo
    return offs, at


def _mm(a, b):
    """a (R, K) @ b (K, M), the K terms added in index order in the operands' type (the order the kernels take them in)"""
    out = np.zeros((a.shape[0], b.shape[1]), a.dtype)
    for k in range(a.shape[1]):
        out = out + a[:, k: k + 1] * b[k: k + 1, :]
    return out


def cond_fc(hist, flat, widths, gout=None, dtype=F64):
    """sigmoid(MLP(hist) + flat[gofs]): hist (N, widths[0]); the weights (in, out) row-major, then the biases, layer by
    layer in ``flat``; ReLU between layers.  With gout (N, widths[-1]): also the gradient of the WHOLE flat vector - the
    tail beyond the global scalar exactly zero."""
    flat, a = np.asarray(flat, dtype), np.asarray(hist, dtype)
    offs, gofs = fc_layout(widths)
    acts, L = [a], len(widths) - 1
    for l, (wo, bo) in enumerate(offs):
        fi, fo = widths[l], widths[l + 1]
        z = _mm(acts[-1], flat[wo: bo].reshape(fi, fo)) + flat[bo: bo + fo]
        acts.append(np.maximum(z, 0) if l < L - 1 else z + flat[gofs])
    out = dtype(1) / (dtype(1) + np.exp(-acts[-1]))
    if gout is None:
        return out, acts
    dflat = np.zeros(flat.shape, dtype)
    delta = np.asarray(gout, dtype) * out * (dtype(1) - out)
    dflat[gofs] = delta.sum()
    for l in range(L - 1, -1, -1):
        wo, bo = offs[l]
        fi, fo = widths[l], widths[l + 1]
        dflat[wo: bo] = _mm(np.ascontiguousarray(acts[l].T), delta).reshape(-1)
        dflat[bo: bo + fo] = delta.sum(0)
        if l:
            delta = _mm(delta, np.ascontiguousarray(flat[wo: bo].reshape(fi, fo).T)) * (acts[l] > 0)
    return out, acts, dflat


def pixel_loss(y, gt, kind):
    """kind 0: mean (y - gt)^2 with gradient 2 (y - gt) / n; kind 1: mean |y - gt| with sign(y - gt) / n, sign(0) = 0"""
    d = np.asarray(y, F64) - np.asarray(gt, F64)
    if kind == 0:
        return float((d * d).mean()), 2.0 * d / d.size
    return float(np.abs(d).mean()), np.sign(d) / d.size


def lg_gain(a, b):
    """the detached gain of the local branch per (n, c): clamp(mean b / (clamp(mean a, 0) + 1e-6), 0.5, 2)"""
    ma, mb = np.asarray(a, F64).mean((2, 3)), np.asarray(b, F64).mean((2, 3))
    return np.clip(mb / (np.maximum(ma, 0.0) + 1e-6), 0.5, 2.0)


def lg_centres(x):
    """the 1/4-scale bilinear sample (align_corners False): the mean of the 2 x 2 centre of each 4 x 4 cell"""
    x = np.asarray(x, F64)
    return (x[..., 1::4, 1::4] + x[..., 1::4, 2::4] + x[..., 2::4, 1::4] + x[..., 2::4, 2::4]) / 4.0


def local_global_l2(a, b, flag):
    """utils/util_loss.py:26-64 with the mean squared loss: MSE(a * gain, b) over the images with flag < 1 plus
    MSE of the 1/4-scale samples over the others; -> loss, d loss / d a (the gain detached)"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    N, C, H, W = a.shape
    loc = np.asarray(flag, F32) < 1
    nl, ng = int(loc.sum()), int(N - loc.sum())
    g, loss = np.zeros_like(a), 0.0
    if nl:
        gain = lg_gain(a, b)[loc][:, :, None, None]
        d = a[loc] * gain - b[loc]
        loss += (d * d).mean()
        g[loc] = 2.0 * d * gain / d.size
    if ng:
        d = lg_centres(a[~loc]) - lg_centres(b[~loc])
        loss += (d * d).mean()
        v = 2.0 * d * 0.25 / d.size
        gg = np.zeros((ng, C, H, W))
        for i in (1, 2):
            for j in (1, 2):
                gg[..., i::4, j::4] = v
        g[~loc] = gg
    return float(loss), g
