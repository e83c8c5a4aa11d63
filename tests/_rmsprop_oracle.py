"""numpy oracles of the WGAN's three kernels (csrc/rmsprop.hip, mode 3 of mi_adv_loss in csrc/bn_seg.hip), in the dtype of their inputs:
float64 is the reference, the float32 run of the same code the yardstick.  tests/test_wgan_cpu.py checks them against torch."""
import numpy as np


def rmsprop_step(p, g, v, lr, alpha=0.99, eps=1e-8, gscale=1.0):
    """torch.optim.RMSprop's default update (no momentum, not centered, no weight decay) -> (p, v) after the step."""
    dt = p.dtype.type
    gr = g * dt(gscale)
    v = dt(alpha) * v + dt(1 - alpha) * gr * gr
    return p - dt(lr) * gr / (np.sqrt(v) + dt(eps)), v


def clamp(p, lo, hi):
    """torch.clamp: comparisons, so NaN stays NaN and -0.0 stays -0.0."""
    dt = p.dtype.type
    return np.where(p < dt(lo), dt(lo), np.where(p > dt(hi), dt(hi), p))


def critic_loss(logit, targets, scale=1.0):
    """Per segment: loss = -mean (real) | +mean (fake), the mean logit, dlogit = -+scale / M."""
    dt = logit.dtype.type
    S = len(targets)
    x = logit.reshape(S, -1)
    M = x.shape[1]
    sign = np.array([-1.0 if real else 1.0 for real in targets], dtype=logit.dtype)
    mean = x.mean(axis=1)
    d = np.repeat(sign * dt(scale) / dt(M), M)
    return sign * mean, mean, d.astype(logit.dtype)
