"""The float64 restatement the optimizer tests compare against: adam_ref of test_gpu_rowops.py (torch's
single-tensor Adam) extended by the decoupled decay of torch.optim.AdamW (p *= 1 - lr * wd before the
step's update), a clip scale on the gradient, and the exponential moving average of
torch.optim.swa_utils.get_ema_multi_avg_fn(d) (e.lerp_(p_new, 1 - d)).  Pure torch, no device."""
import numpy as np
import torch


def f32(x):
    return float(np.float32(x))


def adamw_ema_step(p, g, m, v, t, lr, b1, b2, eps, wd=0.0, scale=1.0, e=None, d=None):
    """One update, number t (1-based), of float64 tensors; returns (p, m, v, e).  lr, wd and d are the
    f32 values the kernels read, as Python floats; e is None without an average."""
    g = g * scale
    p = p * (1 - lr * wd)                             # param.mul_(1 - lr * weight_decay)
    m = m + (g - m) * (1 - b1)                        # exp_avg.lerp_(grad, 1 - beta1)
    v = v * b2 + (1 - b2) * g * g                     # exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
    denom = v.sqrt() / np.sqrt(1 - b2 ** t) + eps     # (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p - (lr / (1 - b1 ** t)) * m / denom          # param.addcdiv_(exp_avg, denom, value=-step_size)
    if e is not None:
        e = e + (p - e) * (1 - d)                     # ema.lerp_(param, 1 - decay)
    return p, m, v, e


def adamw_ema_ref(p, grads, lr, b1, b2, eps, wd=0.0, scales=None, d=None):
    """adam_ref with the three options, from zero moments and an average that starts as a copy of p (the
    first AveragedModel update): [(p, m, v, e)] after each gradient; e is None when d is None."""
    p = p.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    e = p.clone() if d is not None else None
    out = []
    for t, g in enumerate(grads, 1):
        p, m, v, e = adamw_ema_step(p, g, m, v, t, lr, b1, b2, eps, wd, 1.0 if scales is None else scales[t - 1],
                                    e, d)
        out.append((p.clone(), m.clone(), v.clone(), None if e is None else e.clone()))
    return out
