"""numpy oracle of BiGAN's pair head (csrc/pair_disc.hip): the reference's Discriminator (src/models/BiGAN.py:100-126) behind dis_x,
  dis_z    MLPEncoder(L, [H, H], H, output_act="leaky_relu"): Linear -> GroupNorm(1, H) -> LeakyReLU(0.2) -> Linear -> BatchNorm1d ->
           LeakyReLU -> Linear -> LeakyReLU
  dis_pair MLPEncoder(2H, [H], 1) on cat(z_feature, x_feature): Linear -> GroupNorm(1, H) -> LeakyReLU -> Linear
on 2 N rows as two segments (real pairs, then fake pairs: the reference's two calls), with BatchNorm1d's statistics per segment, both
adversarial losses (g_loss = adv(real, False) + adv(fake, True), d_loss = adv(real, True) + adv(fake, False); src/utils/losses.py) and
the hand-derived backward for either right-hand side.  Everything is computed in the dtype of the inputs: float64 is the reference,
the float32 run of the same code is the yardstick the kernel tests scale with.

Parameters are a dict with torch's names and shapes ("dis_z.model.0.fc.weight" [H, L], ...), NAMES in the C ABI's order.
"""
import numpy as np

SLOPE, EPS = 0.2, 1e-5
Z_KEYS = ("model.0.fc.weight", "model.0.fc.bias", "model.0.norm.weight", "model.0.norm.bias", "model.1.fc.weight", "model.1.fc.bias",
          "model.1.norm.weight", "model.1.norm.bias", "classifier.fc.weight", "classifier.fc.bias")
P_KEYS = ("model.0.fc.weight", "model.0.fc.bias", "model.0.norm.weight", "model.0.norm.bias", "classifier.fc.weight", "classifier.fc.bias")
NAMES = tuple("dis_z." + k for k in Z_KEYS) + tuple("dis_pair." + k for k in P_KEYS)
MATS = ("dis_z.model.0.fc.weight", "dis_z.model.1.fc.weight", "dis_z.classifier.fc.weight", "dis_pair.model.0.fc.weight",
        "dis_pair.classifier.fc.weight")
LOSSES = ("vanilla", "lsgan", "hinge")


def shapes(L, H):
    return {"dis_z.model.0.fc.weight": (H, L), "dis_z.model.0.fc.bias": (H,), "dis_z.model.0.norm.weight": (H,), "dis_z.model.0.norm.bias": (H,),
            "dis_z.model.1.fc.weight": (H, H), "dis_z.model.1.fc.bias": (H,), "dis_z.model.1.norm.weight": (H,), "dis_z.model.1.norm.bias": (H,),
            "dis_z.classifier.fc.weight": (H, H), "dis_z.classifier.fc.bias": (H,),
            "dis_pair.model.0.fc.weight": (H, 2 * H), "dis_pair.model.0.fc.bias": (H,), "dis_pair.model.0.norm.weight": (H,),
            "dis_pair.model.0.norm.bias": (H,), "dis_pair.classifier.fc.weight": (1, H), "dis_pair.classifier.fc.bias": (1,)}


def make_params(L, H=128, seed=0):
    """Every parameter away from its default (affine pairs near 1 / near 0, biases not 0), weights at nn.Linear's scale."""
    r = np.random.RandomState(seed)
    p = {}
    for k, s in shapes(L, H).items():
        if k.endswith("norm.weight"):
            p[k] = 1.0 + 0.3 * r.randn(*s)
        elif k.endswith("norm.bias"):
            p[k] = 0.2 * r.randn(*s)
        elif k.endswith("fc.bias"):
            p[k] = 0.1 * r.randn(*s)
        else:
            p[k] = r.randn(*s) / np.sqrt(s[1])
    return p


def cast(p, dtype):
    return {k: np.asarray(v, dtype=dtype) for k, v in p.items()}


def _leaky(v):
    return np.where(v > 0, v, v.dtype.type(SLOPE) * v)


def _dleaky(v):
    return np.where(v > 0, v.dtype.type(1), v.dtype.type(SLOPE))


def _ln(a):
    m = a.mean(axis=1, keepdims=True)
    v = ((a - m) ** 2).mean(axis=1, keepdims=True)
    r = 1 / np.sqrt(v + a.dtype.type(EPS))
    return (a - m) * r, r


def adv(x, real, mode):
    """(f, f') per logit: adversarial_loss's summand (its result is mean f) and its derivative."""
    dt = x.dtype.type
    if mode == "vanilla":
        e = np.exp(-np.abs(x))
        sg = np.where(x >= 0, 1 / (1 + e), e / (1 + e))
        return np.maximum(-x if real else x, 0) + np.log1p(e), sg - dt(1 if real else 0)
    if mode == "lsgan":
        u = x - dt(1 if real else 0)
        return u * u, dt(2) * u
    assert mode == "hinge"
    if real:                                                  # the reference's formula: max(1 - x, 1)
        return np.maximum(1 - x, dt(1)), np.where(x < 0, dt(-1), dt(0))
    return np.maximum(1 + x, dt(0)), np.where(x > -1, dt(1), dt(0))


def forward(p, e, z, xf, mode="vanilla", training=True, running_mean=None, running_var=None, momentum=0.1):
    """e, z [N, L], xf [2N, H] -> dict.  training: batch statistics per segment; the returned running statistics are the given ones
    after two updates, segment 0 first (None given: None).  Evaluation: the running statistics normalise both segments."""
    dt = e.dtype
    N = e.shape[0]
    x = np.concatenate([e, z], 0)
    a1 = x @ p["dis_z.model.0.fc.weight"].T + p["dis_z.model.0.fc.bias"]
    xh1, r1 = _ln(a1)
    pre1 = xh1 * p["dis_z.model.0.norm.weight"] + p["dis_z.model.0.norm.bias"]
    h1 = _leaky(pre1)
    a2 = h1 @ p["dis_z.model.1.fc.weight"].T + p["dis_z.model.1.fc.bias"]
    xh2, r2 = np.empty_like(a2), np.empty((2, a2.shape[1]), dtype=dt)
    rm, rv = running_mean, running_var
    for s in range(2):
        rows = slice(s * N, (s + 1) * N)
        if training:
            m = a2[rows].mean(axis=0)
            v = ((a2[rows] - m) ** 2).mean(axis=0)
            if rm is not None:
                mo = dt.type(momentum)
                rm = (1 - mo) * rm + mo * m
                rv = (1 - mo) * rv + mo * (v * dt.type(N) / dt.type(N - 1))
        else:
            m, v = running_mean, running_var
        r2[s] = 1 / np.sqrt(v + dt.type(EPS))
        xh2[rows] = (a2[rows] - m) * r2[s]
    pre2 = xh2 * p["dis_z.model.1.norm.weight"] + p["dis_z.model.1.norm.bias"]
    h2 = _leaky(pre2)
    a3 = h2 @ p["dis_z.classifier.fc.weight"].T + p["dis_z.classifier.fc.bias"]
    zf = _leaky(a3)
    cat = np.concatenate([zf, xf], 1)
    a4 = cat @ p["dis_pair.model.0.fc.weight"].T + p["dis_pair.model.0.fc.bias"]
    xh4, r4 = _ln(a4)
    pre4 = xh4 * p["dis_pair.model.0.norm.weight"] + p["dis_pair.model.0.norm.bias"]
    h4 = _leaky(pre4)
    logit = h4 @ p["dis_pair.classifier.fc.weight"][0] + p["dis_pair.classifier.fc.bias"][0]
    real, fake = logit[:N], logit[N:]
    fg_r, dg_r = adv(real, False, mode)
    fg_f, dg_f = adv(fake, True, mode)
    fd_r, dd_r = adv(real, True, mode)
    fd_f, dd_f = adv(fake, False, mode)
    return dict(logit=logit, g_loss=fg_r.mean() + fg_f.mean(), d_loss=fd_r.mean() + fd_f.mean(), mean_real=real.mean(), mean_fake=fake.mean(),
                d_loss_real=fd_r.mean(), d_loss_fake=fd_f.mean(), dlogit_g=np.concatenate([dg_r, dg_f]) / dt.type(N),
                dlogit_d=np.concatenate([dd_r, dd_f]) / dt.type(N), running_mean=rm, running_var=rv,
                tape=(x, N, xh1, r1, pre1, h1, a2, xh2, r2, pre2, h2, a3, cat, xh4, r4, pre4, h4, training))


def backward(p, fwd, dl):
    """Gradients of sum(dl * logit): (dict of the sixteen parameter gradients, dxf [2N, H], dx [2N, L] by the code rows)."""
    x, N, xh1, r1, pre1, h1, a2, xh2, r2, pre2, h2, a3, cat, xh4, r4, pre4, h4, training = fwd["tape"]
    H = h4.shape[1]
    g = {"dis_pair.classifier.fc.weight": (dl @ h4)[None, :], "dis_pair.classifier.fc.bias": dl.sum(keepdims=True)}
    dn4 = dl[:, None] * p["dis_pair.classifier.fc.weight"][0][None, :] * _dleaky(pre4)
    g["dis_pair.model.0.norm.bias"] = dn4.sum(axis=0)
    g["dis_pair.model.0.norm.weight"] = (dn4 * xh4).sum(axis=0)
    dxh4 = dn4 * p["dis_pair.model.0.norm.weight"]
    da4 = r4 * (dxh4 - dxh4.mean(axis=1, keepdims=True) - xh4 * (dxh4 * xh4).mean(axis=1, keepdims=True))
    g["dis_pair.model.0.fc.weight"] = da4.T @ cat
    g["dis_pair.model.0.fc.bias"] = da4.sum(axis=0)
    dcat = da4 @ p["dis_pair.model.0.fc.weight"]
    dzf, dxf = dcat[:, :H], dcat[:, H:]
    da3 = dzf * _dleaky(a3)
    g["dis_z.classifier.fc.weight"] = da3.T @ h2
    g["dis_z.classifier.fc.bias"] = da3.sum(axis=0)
    dn2 = (da3 @ p["dis_z.classifier.fc.weight"]) * _dleaky(pre2)
    g["dis_z.model.1.norm.bias"] = dn2.sum(axis=0)
    g["dis_z.model.1.norm.weight"] = (dn2 * xh2).sum(axis=0)
    dxh2 = dn2 * p["dis_z.model.1.norm.weight"]
    da2 = np.empty_like(dxh2)
    for s in range(2):
        rows = slice(s * N, (s + 1) * N)
        d, xh = dxh2[rows], xh2[rows]
        da2[rows] = r2[s] * (d - d.mean(axis=0) - xh * (d * xh).mean(axis=0)) if training else r2[s] * d
    g["dis_z.model.1.fc.weight"] = da2.T @ h1
    g["dis_z.model.1.fc.bias"] = da2.sum(axis=0)
    dn1 = (da2 @ p["dis_z.model.1.fc.weight"]) * _dleaky(pre1)
    g["dis_z.model.0.norm.bias"] = dn1.sum(axis=0)
    g["dis_z.model.0.norm.weight"] = (dn1 * xh1).sum(axis=0)
    dxh1 = dn1 * p["dis_z.model.0.norm.weight"]
    da1 = r1 * (dxh1 - dxh1.mean(axis=1, keepdims=True) - xh1 * (dxh1 * xh1).mean(axis=1, keepdims=True))
    g["dis_z.model.0.fc.weight"] = da1.T @ x
    g["dis_z.model.0.fc.bias"] = da1.sum(axis=0)
    return g, dxf, da1 @ p["dis_z.model.0.fc.weight"]
