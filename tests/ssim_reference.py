"""Float64 reference of the SSIM the HIP path implements (truth of tests/test_ssim_cpu.py and tests/test_gpu_ssim.py).

The arithmetic is what the reference's ``get_ssim`` (utils/util_path_restore.py:27-44) selects in scikit-image,
``compare_ssim(ref, img, data_range=..., multichannel=True)`` with the package's published defaults: a uniform 7 x 7
window, K1 = 0.01, K2 = 0.03, C1 = (K1 L)^2, C2 = (K2 L)^2, SAMPLE covariance (cov_norm = 49 / 48), per channel

    S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2))

averaged over the windows that lie wholly inside the image (scikit-image filters the whole plane and crops 3 pixels per
side, so its border mode never reaches the result), then over the channels: one value per image.

Written with torch ops in whatever dtype the inputs have, so that the same text is the float64 truth, the differentiable
truth of the gradient (autograd) and - on float32 tensors - the "fp32 restatement" the error budget compares against.
``ssim_filter_crop`` is the independent filter-then-crop form built on scipy.ndimage.uniform_filter.
"""
import numpy as np
import torch
import torch.nn.functional as TF

WIN = 7
K1, K2 = 0.01, 0.03


def ssim(x, y, data_range=1.0):
    """x, y: (N,C,H,W) tensors of one dtype, H, W >= 7; data_range: a number or an (N,) tensor -> (N,) tensor"""
    if x.shape != y.shape or x.dim() != 4 or x.shape[2] < WIN or x.shape[3] < WIN:
        raise ValueError('ssim: two (N,C,H,W) tensors with H, W >= 7 expected, got %s / %s' % (tuple(x.shape), tuple(y.shape)))
    L = torch.as_tensor(data_range, dtype=x.dtype, device=x.device).reshape(-1, 1, 1, 1)
    c1, c2 = (K1 * L) ** 2, (K2 * L) ** 2
    npix = WIN * WIN
    cn = npix / (npix - 1.0)
    box = lambda t: TF.avg_pool2d(t, WIN, stride=1)                  # valid windows only
    ux, uy = box(x), box(y)
    vx = cn * (box(x * x) - ux * ux)
    vy = cn * (box(y * y) - uy * uy)
    vxy = cn * (box(x * y) - ux * uy)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return s.mean(dim=(1, 2, 3))


def ssim_numpy(x, y, data_range=1.0):
    """the same for float64 evaluation of numpy (N,C,H,W) arrays of any real dtype -> (N,) float64 array"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    dr = t(np.asarray(data_range, dtype=np.float64)) if np.ndim(data_range) else float(data_range)
    return ssim(t(x), t(y), dr).numpy()


def ssim_filter_crop(x, y, data_range=1.0):
    """scikit-image's own route for one (C,H,W) float64 pair: uniform_filter over the whole plane, crop 3 per side"""
    from scipy.ndimage import uniform_filter
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    cn = WIN * WIN / (WIN * WIN - 1.0)
    pad = (WIN - 1) // 2
    vals = []
    for a, b in zip(x, y):
        f = lambda t: uniform_filter(t, size=WIN)
        ux, uy = f(a), f(b)
        vx, vy, vxy = cn * (f(a * a) - ux * ux), cn * (f(b * b) - uy * uy), cn * (f(a * b) - ux * uy)
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        vals.append(s[pad:-pad, pad:-pad].mean())
    return float(np.mean(vals))


def tensor2bgr_codes(t):
    """tensor2bgr's arithmetic (utils/util.py) on an (N,C,H,W) tensor, kept NCHW: clip(v * 255, 0, 255) truncated to uint8"""
    return np.clip(t.detach().cpu().numpy() * 255, 0, 255).astype(np.uint8)


def smooth_pair(n, c, h, w, seed, noise=0.05):
    """a smooth float32 image in [0, 1] and a noisy copy of it (the test inputs), as (N,C,H,W) CPU tensors"""
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(0, 1, h).view(1, 1, h, 1)
    xx = torch.linspace(0, 1, w).view(1, 1, 1, w)
    ph = torch.rand(n, c, 1, 1, generator=g) * 6.28
    fr = 2 + 6 * torch.rand(n, c, 1, 1, generator=g)
    base = 0.5 + 0.25 * torch.sin(fr * xx * 3.1 + ph) * torch.cos(fr * yy * 2.3 - ph) + 0.2 * (xx - yy)
    base = base.clamp(0, 1).float()
    noisy = (base + noise * torch.randn(n, c, h, w, generator=g)).clamp(0, 1).float()
    return noisy, base
