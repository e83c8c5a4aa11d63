"""numpy oracle of the row-local latent discriminator (csrc/latent_disc_ln.hip): MLPEncoder(L, [256, 256], 1, norm_type="layer") of the
reference's src/networks/basic.py -- Linear -> GroupNorm(1, C) -> LeakyReLU(0.2) -> Linear -> GroupNorm(1, C) -> LeakyReLU(0.2) -> Linear --
over a batch of two segments with a target each, with the "vanilla" (binary cross-entropy on the logit) and the "lsgan" loss, its
forward and its hand-derived backward of c0 * loss0 + c1 * loss1.  Everything is computed in the dtype of the inputs: float64 is the
reference, the float32 run of the same code is the yardstick the tests scale with.

Parameters are a dict with torch's names and shapes, as in tests/_latent_disc_oracle.py.
"""
import numpy as np

from _latent_disc_oracle import NAMES, cast, make_params  # noqa: F401  (same ten tensors)

SLOPE, EPS = 0.2, 1e-5


def _leaky(v):
    return np.where(v > 0, v, SLOPE * v)


def _ln(a, dt):
    m = a.mean(axis=1, keepdims=True)
    v = ((a - m) ** 2).mean(axis=1, keepdims=True)
    r = 1 / np.sqrt(v + dt.type(EPS))
    return (a - m) * r, r


def row_loss(x, t, loss_mode):
    dt = x.dtype
    if loss_mode == "vanilla":                               # the stable form: finite for any finite logit
        return np.maximum(x, 0) - x * dt.type(t) + np.log1p(np.exp(-np.abs(x)))
    assert loss_mode == "lsgan"
    return (x - dt.type(t)) ** 2


def row_dloss(x, t, loss_mode):
    dt = x.dtype
    if loss_mode == "vanilla":
        e = np.exp(-np.abs(x))
        return np.where(x >= 0, 1 / (1 + e), e / (1 + e)) - dt.type(t)
    return dt.type(2) * (x - dt.type(t))


def forward(p, x0, t0, x1=None, t1=0.0, loss_mode="vanilla"):
    """-> dict(logit [N0 + N1], loss0, loss1, mean_logit0, mean_logit1, d_loss, tape).  An empty second segment gives loss1 = mean1 = 0."""
    dt = x0.dtype
    N0 = x0.shape[0]
    x = x0 if x1 is None or x1.shape[0] == 0 else np.concatenate([x0, x1], 0)
    N1 = x.shape[0] - N0
    a1 = x @ p["model.0.fc.weight"].T + p["model.0.fc.bias"]
    xh1, r1 = _ln(a1, dt)
    pre1 = xh1 * p["model.0.norm.weight"] + p["model.0.norm.bias"]
    h1 = _leaky(pre1)
    a2 = h1 @ p["model.1.fc.weight"].T + p["model.1.fc.bias"]
    xh2, r2 = _ln(a2, dt)
    pre2 = xh2 * p["model.1.norm.weight"] + p["model.1.norm.bias"]
    h2 = _leaky(pre2)
    logit = h2 @ p["classifier.fc.weight"][0] + p["classifier.fc.bias"][0]
    loss0 = row_loss(logit[:N0], t0, loss_mode).mean()
    loss1 = row_loss(logit[N0:], t1, loss_mode).mean() if N1 else dt.type(0)
    return dict(logit=logit, loss0=loss0, loss1=loss1, mean_logit0=logit[:N0].mean(), mean_logit1=logit[N0:].mean() if N1 else dt.type(0),
                d_loss=dt.type(0.5) * (loss0 + loss1), tape=(x, N0, N1, xh1, r1, pre1, h1, xh2, r2, pre2, h2, loss_mode))


def backward(p, fwd, t0, t1=0.0, c0=1.0, c1=0.0):
    """Gradients of c0 * loss0 + c1 * loss1: (dict of parameter gradients under torch's names, dx [N0 + N1, L])."""
    x, N0, N1, xh1, r1, pre1, h1, xh2, r2, pre2, h2, loss_mode = fwd["tape"]
    dt = x.dtype
    logit = fwd["logit"]
    dl = np.concatenate([dt.type(c0) / N0 * row_dloss(logit[:N0], t0, loss_mode)]
                        + ([dt.type(c1) / N1 * row_dloss(logit[N0:], t1, loss_mode)] if N1 else []))
    g = {"classifier.fc.weight": (dl @ h2)[None, :], "classifier.fc.bias": dl.sum(keepdims=True)}
    dn2 = dl[:, None] * p["classifier.fc.weight"][0][None, :] * np.where(pre2 > 0, dt.type(1), dt.type(SLOPE))
    g["model.1.norm.bias"] = dn2.sum(axis=0)
    g["model.1.norm.weight"] = (dn2 * xh2).sum(axis=0)
    dxh2 = dn2 * p["model.1.norm.weight"]
    da2 = r2 * (dxh2 - dxh2.mean(axis=1, keepdims=True) - xh2 * (dxh2 * xh2).mean(axis=1, keepdims=True))
    g["model.1.fc.weight"] = da2.T @ h1
    g["model.1.fc.bias"] = da2.sum(axis=0)
    dn1 = (da2 @ p["model.1.fc.weight"]) * np.where(pre1 > 0, dt.type(1), dt.type(SLOPE))
    g["model.0.norm.bias"] = dn1.sum(axis=0)
    g["model.0.norm.weight"] = (dn1 * xh1).sum(axis=0)
    dxh1 = dn1 * p["model.0.norm.weight"]
    da1 = r1 * (dxh1 - dxh1.mean(axis=1, keepdims=True) - xh1 * (dxh1 * xh1).mean(axis=1, keepdims=True))
    g["model.0.fc.weight"] = da1.T @ x
    g["model.0.fc.bias"] = da1.sum(axis=0)
    return g, da1 @ p["model.0.fc.weight"]
