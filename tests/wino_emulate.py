"""The two Winograd-along-x kernels restated with plain torch ops, exactly as they consume their packs (reconfigisp_amd/convnets.py:
wino43_weights / wino45_weights).  In float64 only the algebra is on trial (tests/test_pack_algebra_cpu.py); on float32 tensors the same
code is the float32 yardstick of the algorithm class (tests/conv_reference.py: ``e32``)."""
import torch
import torch.nn.functional as TF


def wino43_emulate(x, pack, ck, cout):
    """What conv_wino43_kernel computes from its pack: F(4,3), four outputs per quad from 6 products per filter row."""
    n, cin, h, w = x.shape
    nq = (w + 3) // 4
    xp = TF.pad(x, (1, 4 * nq - w + 4, 1, 1))
    d = [xp[:, :, :, j:j + 4 * nq:4] for j in range(6)]                  # d_j = x[4q - 1 + j]
    s12, s34, m12, m34, m13, m24 = d[1] + d[2], d[3] + d[4], d[1] - d[2], d[3] - d[4], d[1] - d[3], d[2] - d[4]
    v = torch.stack([4 * d[0] - 5 * d[2] + d[4], 4 * s12 - s34, m34 - 4 * m12, -2 * m13 - m24, 2 * m13 - m24,
                     4 * d[1] - 5 * d[3] + d[5]], dim=-1)
    ncb, nch = pack.shape[0], pack.shape[1]
    u = pack.permute(0, 5, 1, 4, 2, 3).reshape(ncb * 32, nch * ck, 3, 6)[:cout, :cin]
    m = torch.zeros(n, cout, h, nq, 6, dtype=x.dtype)
    for ky in range(3):
        m += torch.einsum('nchqt,oct->nohqt', v[:, :, ky:ky + h], u[:, :, ky])
    a12, s12, a34, s34 = m[..., 1] + m[..., 2], m[..., 1] - m[..., 2], m[..., 3] + m[..., 4], m[..., 3] - m[..., 4]
    y = torch.stack([m[..., 0] + a12 + a34, s12 + 2 * s34, a12 + 4 * a34, s12 + 8 * s34 + m[..., 5]], dim=-1)
    return y.reshape(n, cout, h, 4 * nq)[..., :w]


def wino45_emulate(x, pack, ck, cout, layout=0):
    """What conv_wino45_glds_kernel computes from its pack: F(4,5), four outputs per quad from 8 products per filter row
    (the input transform and the output combination exactly as the kernel writes them)."""
    n, cin, h, w = x.shape
    nq = (w + 3) // 4
    xp = TF.pad(x, (2, 4 * nq - w + 6, 2, 2))
    d = [xp[:, :, :, j:j + 4 * nq:4] for j in range(8)]                  # d_j = x[4q - 2 + j]
    e1, o1 = 4 * (d[2] + d[6]) - 17 * d[4], 4 * (d[1] + d[5]) - 17 * d[3]
    e3, o3 = d[2] - 5 * d[4] + 4 * d[6], d[1] - 5 * d[3] + 4 * d[5]
    e5, o5 = 4 * d[2] - 5 * d[4] + d[6], 4 * d[1] - 5 * d[3] + d[5]
    v = torch.stack([(d[0] - d[6]) + 5.25 * (d[4] - d[2]), e1 + o1, e1 - o1, e3 + 2 * o3, e3 - 2 * o3, 2 * e5 + o5, 2 * e5 - o5,
                     (d[7] - d[1]) + 5.25 * (d[3] - d[5])], dim=-1)     # (n,ci,h+4,quads,8)
    ncb, nch = pack.shape[0], pack.shape[1]
    if layout == 0:                                 # [cb][chunk][ky][t][ci][32]
        u = pack.permute(0, 5, 1, 4, 2, 3).reshape(ncb * 32, nch * ck, 5, 8)[:cout, :cin]     # (co, ci, ky, t)
    else:                                           # [cb][chunk][ky][point group][cout block of 16][ci][cout 16][4 points]
        u = pack.permute(0, 4, 6, 1, 5, 2, 3, 7).reshape(ncb * 32, nch * ck, 5, 8)[:cout, :cin]
    m = torch.zeros(n, cout, h, nq, 8, dtype=x.dtype)
    for ky in range(5):
        m += torch.einsum('nchqt,oct->nohqt', v[:, :, ky:ky + h], u[:, :, ky])
    a12, s12, a34, s34, a56, s56 = (m[..., 1] + m[..., 2], m[..., 1] - m[..., 2], m[..., 3] + m[..., 4], m[..., 3] - m[..., 4],
                                    m[..., 5] + m[..., 6], m[..., 5] - m[..., 6])
    y = torch.stack([m[..., 0] + a12 + a34 + a56, s12 + 2 * s34 + 0.5 * s56, a12 + 4 * a34 + 0.25 * a56,
                     s12 + 8 * s34 + 0.125 * s56 + m[..., 7]], dim=-1)
    return y.reshape(n, cout, h, 4 * nq)[..., :w]
