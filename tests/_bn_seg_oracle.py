"""numpy oracle of csrc/bn_seg.hip: segmented BatchNorm + activation (forward, backward) and the adversarial losses.

Every function computes in the dtype of its inputs (`cast` them to float64 for the oracle, to float32 for the yardstick the kernel
tests measure rounding against).  x: [S*M, C] rows, S segments of M rows each."""
import numpy as np

ACTS = (None, "relu", "leaky_relu")
MODES = ("vanilla", "lsgan", "hinge")


def cast(a, dtype):
    return None if a is None else np.asarray(a).astype(dtype)


def act(v, kind, slope):
    if kind == "relu":
        return np.maximum(v, 0)
    if kind == "leaky_relu":
        return np.where(v > 0, v, v * v.dtype.type(slope))
    return v


def act_grad(y, g, kind, slope):
    """From the activation's OUTPUT y, as mi_relu_bwd / mi_leaky_relu_bwd."""
    if kind == "relu":
        return np.where(y > 0, g, 0).astype(g.dtype)
    if kind == "leaky_relu":
        return np.where(y > 0, g, g * g.dtype.type(slope))
    return g


def bn_seg_fwd(x, gamma, beta, S, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, training=True, kind=None, slope=0.2):
    """-> y [S*M, C], mean [S, C], rstd [S, C], running_mean, running_var (after the S updates, segment 0 first; None stays None)."""
    dt = x.dtype.type
    C = x.shape[1]
    M = x.shape[0] // S
    xs = x.reshape(S, M, C)
    rm = None if running_mean is None else running_mean.copy()
    rv = None if running_var is None else running_var.copy()
    if training:
        mean = xs.mean(axis=1)
        var = ((xs - mean[:, None, :]) ** 2).mean(axis=1)
        for s in range(S):
            if rm is not None:
                rm = (1 - dt(momentum)) * rm + dt(momentum) * mean[s]
            if rv is not None:
                rv = (1 - dt(momentum)) * rv + dt(momentum) * (var[s] * dt(M) / dt(M - 1) if M > 1 else var[s])
    else:
        mean = np.broadcast_to(running_mean, (S, C)).copy()
        var = np.broadcast_to(running_var, (S, C)).copy()
    rstd = 1 / np.sqrt(var + dt(eps))
    y = act((xs - mean[:, None, :]) * rstd[:, None, :] * gamma + beta, kind, slope)
    return y.reshape(S * M, C), mean, rstd, rm, rv


def bn_seg_bwd(x, mean, rstd, gamma, y, dy, kind=None, slope=0.2):
    """-> dx [S*M, C], dgamma [C], dbeta [C] of the training-mode forward."""
    S, C = mean.shape
    M = x.shape[0] // S
    g = act_grad(y, dy, kind, slope).reshape(S, M, C)
    xh = (x.reshape(S, M, C) - mean[:, None, :]) * rstd[:, None, :]
    s0 = g.sum(axis=1)
    s1 = (g * xh).sum(axis=1)
    dx = gamma * rstd[:, None, :] * (g - s0[:, None, :] / M - xh * s1[:, None, :] / M)
    return dx.reshape(S * M, C), s1.sum(axis=0), s0.sum(axis=0)


def adv_loss(logit, targets, mode, scale=1.0):
    """The reference's adversarial_loss per segment: -> loss [S], mean_logit [S], dlogit [S*M] = scale * d loss_s / d logit.
    hinge is the reference's: max(1 - x, 1) for real targets (not the textbook max(1 - x, 0)), max(1 + x, 0) for fake ones; where
    the two operands of the maximum tie, half the gradient goes each way, as torch.maximum's backward does."""
    dt = logit.dtype.type
    S = len(targets)
    x = logit.reshape(S, -1)
    M = x.shape[1]
    loss, d = np.empty_like(x), np.empty_like(x)
    for s, real in enumerate(targets):
        v = x[s]
        if mode == "vanilla":
            e = np.exp(-np.abs(v))
            sig = np.where(v >= 0, 1 / (1 + e), e / (1 + e))
            nsig = np.where(v >= 0, e / (1 + e), 1 / (1 + e))
            loss[s] = np.maximum(-v if real else v, 0) + np.log1p(e)
            d[s] = -nsig if real else sig
        elif mode == "lsgan":
            u = v - dt(1.0 if real else 0.0)
            loss[s], d[s] = u * u, 2 * u
        elif mode == "hinge" and real:
            loss[s] = np.maximum(1 - v, 1)
            d[s] = np.where(v < 0, -1.0, np.where(v == 0, -0.5, 0.0))
        elif mode == "hinge":
            loss[s] = np.maximum(1 + v, 0)
            d[s] = np.where(v > -1, 1.0, np.where(v == -1, 0.5, 0.0))
        else:
            raise ValueError(mode)
    return loss.mean(axis=1), x.mean(axis=1), (dt(scale) * d / dt(M)).reshape(-1).astype(logit.dtype)
