"""numpy oracle of the latent discriminator (csrc/latent_disc.hip): MLPEncoder(L, [256, 256], 1) of the reference's
src/networks/basic.py -- Linear -> GroupNorm(1, C) -> LeakyReLU(0.2) -> Linear -> BatchNorm1d -> LeakyReLU(0.2) -> Linear -- with the
least-squares loss mean((logit - t)^2), its forward, its running statistics and its hand-derived backward.  Everything is computed
in the dtype of the inputs: float64 is the reference, the float32 run of the same code is the yardstick the tests scale with.

Parameters are a dict with torch's names and shapes:
    model.0.fc.weight [H, L], model.0.fc.bias [H], model.0.norm.weight [H], model.0.norm.bias [H],
    model.1.fc.weight [H, H], model.1.fc.bias [H], model.1.norm.weight [H], model.1.norm.bias [H],
    classifier.fc.weight [1, H], classifier.fc.bias [1]
"""
import numpy as np

NAMES = ("model.0.fc.weight", "model.0.fc.bias", "model.0.norm.weight", "model.0.norm.bias", "model.1.fc.weight", "model.1.fc.bias",
         "model.1.norm.weight", "model.1.norm.bias", "classifier.fc.weight", "classifier.fc.bias")
SLOPE, EPS, MOMENTUM = 0.2, 1e-5, 0.1


def make_params(L, H=256, seed=0, dtype=np.float64):
    """Every parameter away from its default (norm weights not 1, biases not 0)."""
    r = np.random.RandomState(seed)
    p = {"model.0.fc.weight": r.randn(H, L) / np.sqrt(L), "model.0.fc.bias": 0.1 * r.randn(H),
         "model.0.norm.weight": 1 + 0.2 * r.randn(H), "model.0.norm.bias": 0.1 * r.randn(H),
         "model.1.fc.weight": r.randn(H, H) / np.sqrt(H), "model.1.fc.bias": 0.1 * r.randn(H),
         "model.1.norm.weight": 1 + 0.2 * r.randn(H), "model.1.norm.bias": 0.1 * r.randn(H),
         "classifier.fc.weight": r.randn(1, H) / np.sqrt(H), "classifier.fc.bias": 0.1 * r.randn(1)}
    return {k: v.astype(dtype) for k, v in p.items()}


def cast(d, dtype):
    return {k: (np.asarray(v).astype(dtype) if np.asarray(v).dtype.kind == "f" else v) for k, v in d.items()}


def form_input(z=None, h=None, eps=None, perm=None):
    """The three input sources: rows z | mu + exp(log_sigma) eps from h = [mu | log_sigma] | that, column j gathered through perm[j]
    (the reference's permute_dims); an index outside [0, N) gives 0."""
    if z is not None:
        return np.array(z)
    L = eps.shape[1]
    zz = h[:, :L] + np.exp(h[:, L:2 * L]) * eps
    if perm is None:
        return zz
    N = zz.shape[0]
    x = np.zeros_like(zz)
    for j in range(L):
        idx = np.asarray(perm[j])
        ok = (idx >= 0) & (idx < N)
        x[ok, j] = zz[idx[ok], j]
    return x


def _leaky(v):
    return np.where(v > 0, v, SLOPE * v)


def forward(p, x, target, training=True, running=None):
    """-> dict(logit [N], loss, mean_logit, tape...).  running = (running_mean, running_var): used in evaluation mode; in training
    mode the updated pair comes back as out['running'] (unbiased variance, momentum 0.1)."""
    dt = x.dtype
    N = x.shape[0]
    a1 = x @ p["model.0.fc.weight"].T + p["model.0.fc.bias"]
    m1 = a1.mean(axis=1, keepdims=True)
    v1 = ((a1 - m1) ** 2).mean(axis=1, keepdims=True)
    r1 = 1 / np.sqrt(v1 + dt.type(EPS))
    xh1 = (a1 - m1) * r1
    pre1 = xh1 * p["model.0.norm.weight"] + p["model.0.norm.bias"]
    h1 = _leaky(pre1)
    a2 = h1 @ p["model.1.fc.weight"].T + p["model.1.fc.bias"]
    out = {}
    if training:
        m2 = a2.mean(axis=0)
        ss = ((a2 - m2) ** 2).sum(axis=0)
        v2 = ss / N
        if running is not None:
            mo = dt.type(MOMENTUM)
            out["running"] = ((1 - mo) * running[0] + mo * m2, (1 - mo) * running[1] + mo * ss / (N - 1))
    else:
        m2, v2 = running
    r2 = 1 / np.sqrt(v2 + dt.type(EPS))
    xh2 = (a2 - m2) * r2
    pre2 = xh2 * p["model.1.norm.weight"] + p["model.1.norm.bias"]
    h2 = _leaky(pre2)
    logit = h2 @ p["classifier.fc.weight"][0] + p["classifier.fc.bias"][0]
    out.update(logit=logit, loss=((logit - dt.type(target)) ** 2).mean(), mean_logit=logit.mean(),
               tape=(x, xh1, r1, pre1, h1, xh2, r2, pre2, h2, training))
    return out


def backward(p, fwd, target):
    """Gradients of mean((logit - target)^2): (dict of parameter gradients under torch's names, dx [N, L])."""
    x, xh1, r1, pre1, h1, xh2, r2, pre2, h2, training = fwd["tape"]
    dt = x.dtype
    N = x.shape[0]
    dl = dt.type(2.0) * (fwd["logit"] - dt.type(target)) / N
    g = {"classifier.fc.weight": (dl @ h2)[None, :], "classifier.fc.bias": dl.sum(keepdims=True)}
    dn2 = dl[:, None] * p["classifier.fc.weight"][0][None, :] * np.where(pre2 > 0, dt.type(1), dt.type(SLOPE))
    g["model.1.norm.bias"] = dn2.sum(axis=0)
    g["model.1.norm.weight"] = (dn2 * xh2).sum(axis=0)
    dxh2 = dn2 * p["model.1.norm.weight"]
    if training:
        da2 = r2 * (dxh2 - dxh2.mean(axis=0) - xh2 * (dxh2 * xh2).mean(axis=0))
    else:
        da2 = r2 * dxh2
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
