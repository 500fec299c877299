"""The fused training step of an element-wise fixed pipeline (risp_chain_train_step), restated plainly and in any precision.

CPU only, and nothing of the package under test is imported: the forward is oracle/isp_oracle.py (nearest demosaic,
WbManual, Gamma, GtmManual, WbQuadratic, per stage ``sigmoid(raw).repeat(N, 1)`` as isp_universal.py:210-232 builds it),
the gradients are torch.autograd's, the mean loss and Adam are written out from their definitions.  One step starts from a
state that is handed in (parameters, both Adam moments, the 1-based number of the step), so that a multi-step run of the
kernel can be judged step by step from the kernel's own state: fp32 values are exact in float64.

    reference_step(ops, from_bayer, loss_kind, img, gt, raw, exp_avg, exp_avg_sq, step, lr, betas, eps, dtype,
                   zero_grad_at=None) -> y, loss, grads, raw', exp_avg', exp_avg_sq', blocks'
"""
import torch

import isp_oracle as O

# include/risp.h op codes
OP_SKIP, OP_DEMOSAIC_NEAREST, OP_WB_MANUAL, OP_GAMMA, OP_GTM_MANUAL, OP_WB_QUADRATIC, OP_GAIN3 = range(7)
OP_NAMES = {OP_WB_MANUAL: 'wbmanual', OP_GAMMA: 'gamma', OP_GTM_MANUAL: 'gtmmanual', OP_WB_QUADRATIC: 'wbquadratic'}
PARAM_WIDTH = {OP_WB_MANUAL: 3, OP_GAMMA: 1, OP_GTM_MANUAL: 3, OP_WB_QUADRATIC: 30}
LOSS_MSE, LOSS_L1 = 0, 1


def blocks_of(op, raw, n):
    """what the next forward reads for one stage: sigmoid(raw).repeat(N, 1), x 5 for the manual white balance (the gain
    of tools_origin.py:214) - (N, P)"""
    b = torch.sigmoid(raw).repeat(n, 1)
    return b * 5 if op == OP_WB_MANUAL else b


def reference_step(ops, from_bayer, loss_kind, img, gt, raw, exp_avg, exp_avg_sq, step, lr, betas, eps, dtype,
                   zero_grad_at=None):
    """One training step in ``dtype``.

    ops: op codes of the stages; img (N,1,H,W) mosaic or (N,3,H,W) BGR; gt (N,3,H,W); raw / exp_avg / exp_avg_sq: one 1-D
    tensor per stage (the state BEFORE the step, not modified); step: the 1-based number of this step; zero_grad_at: a
    boolean (N,3,H,W) mask of output positions whose d loss / d y is taken as exactly 0 (nn.L1Loss has gradient 0 where
    output == target; a restatement in another precision does not hit the tie itself).
    -> y, loss (0-d), [grad], [raw'], [exp_avg'], [exp_avg_sq'], [blocks' (N,P)]"""
    n = img.shape[0]
    x = img.detach().to(dtype)
    gt = gt.detach().to(dtype)
    pars = [r.detach().to(dtype).clone().requires_grad_(True) for r in raw]
    if from_bayer:
        x = O.demosaic_nearest(x)
    for op, p in zip(ops, pars):
        x = O.apply_op(OP_NAMES[op], x, torch.sigmoid(p).repeat(n, 1))
    y = x
    if zero_grad_at is not None:                 # same value, no gradient through the masked positions
        x = torch.where(zero_grad_at, y.detach(), y)
    d = x - gt
    if loss_kind == LOSS_MSE:
        loss = (d ** 2).mean()
    elif loss_kind == LOSS_L1:
        loss = d.abs().mean()
    else:
        raise ValueError(loss_kind)
    grads = torch.autograd.grad(loss, pars)
    # Adam (Kingma & Ba 2015, algorithm 1; no weight decay, no amsgrad)
    beta1, beta2 = betas
    new_raw, new_m, new_v, blocks = [], [], [], []
    for op, p, g, m, v in zip(ops, pars, grads, exp_avg, exp_avg_sq):
        m = beta1 * m.detach().to(dtype) + (1.0 - beta1) * g
        v = beta2 * v.detach().to(dtype) + (1.0 - beta2) * g * g
        m_hat = m / (1.0 - beta1 ** step)
        v_hat = v / (1.0 - beta2 ** step)
        r = p.detach() - lr * m_hat / (v_hat.sqrt() + eps)
        new_raw.append(r), new_m.append(m), new_v.append(v), blocks.append(blocks_of(op, r, n))
    return y.detach(), loss.detach(), list(grads), new_raw, new_m, new_v, blocks
