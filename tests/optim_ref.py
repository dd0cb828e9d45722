"""Reference (test infrastructure) for the grouped optimizer step: torch.optim.Adam / AdamW's single-tensor update written out, with weight decay in
both forms, amsgrad and the clip coefficient of torch.nn.utils.clip_grad_norm_.  Evaluated in the dtype of its arguments: fp64 is the reference,
fp32 the 'reference alone' condition.  tests/test_optim_cpu.py holds it to torch's own optimizers in fp64."""
import torch


def optim_update(p, g, m, v, vmax, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False, amsgrad=False, coef=1.0):
    """One step (`step` is 1-based) of Adam (decoupled False: L2 decay, g += wd * p) or AdamW (decoupled True: p *= 1 - lr * wd) on one tensor.
    `g` is the gradient as the optimizer sees it apart from the clip: g * coef is what enters.  Returns (p, m, v, vmax); vmax is returned as
    it came without amsgrad.  The decoupled decay is written p - (lr * wd) * p: the factor 1 - lr * wd itself is no fp32 number (1 - 3e-5 is 1.8e-8 off
    its nearest one), which would put that much per step into the fp32 evaluation of this very function."""
    g = g * coef
    if weight_decay != 0:
        if decoupled:
            p = p - (lr * weight_decay) * p
        else:
            g = g + weight_decay * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    if amsgrad:
        vmax = torch.maximum(vmax, v)
        denom = (vmax.sqrt() / (bc2 ** 0.5)) + eps
    else:
        denom = (v.sqrt() / (bc2 ** 0.5)) + eps
    return p - (lr / bc1) * (m / denom), m, v, vmax


def grad_norm(g):
    """Global L2 norm of the gradient tensors (or one tensor), in their dtype."""
    gs = [g] if torch.is_tensor(g) else list(g)
    return torch.sqrt(sum((t * t).sum() for t in gs))


def clip_coef(norm, max_norm):
    """clip_grad_norm_: the factor on every gradient, min(1, max_norm / (norm + 1e-6))."""
    c = max_norm / (norm + 1e-6)
    return torch.clamp(c, max=1.0) if torch.is_tensor(c) else min(1.0, c)
