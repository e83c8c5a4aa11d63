"""A fresh float64 CPU MADE forward and backward from a state_dict-like mapping (masks included), for the GPU parity tests.

Written from the reference's semantics (src/models/made.py): masked linear layers F.linear(x, W * mask, b) with a sigmoid between
layers and none after the last, logits rearranged (n (c h w a) -> n a c h w), bpd = mean cross-entropy / ln 2 with the truncating
target; `pick(probs, u)` is the samplers' inverse-CDF rule k = min{k : cdf_k > u}, clamped to 255."""
import torch
import torch.nn.functional as F


def n_layers(p):
    return sum(1 for k in p if k.endswith(".mask"))


def _wm(p, i):
    w = p[f"model.model.{i}.model.weight"].double()
    return w * p[f"model.model.{i}.mask"].to(w.dtype), p[f"model.model.{i}.model.bias"].double()


def hidden(p, x):
    """Sigmoid outputs of the hidden layers for x [N, C, H, W] (float64)."""
    h = x.reshape(x.shape[0], -1).double()
    acts = []
    for i in range(n_layers(p) - 1):
        w, b = _wm(p, i)
        h = torch.sigmoid(F.linear(h, w, b))
        acts.append(h)
    return acts


def forward(p, x):
    n, c, hh, ww = x.shape
    w, b = _wm(p, n_layers(p) - 1)
    out = F.linear(hidden(p, x)[-1], w, b)
    return out.reshape(n, c, hh, ww, 256).permute(0, 4, 1, 2, 3)


def target(x, normalize):
    return ((x + 1) / 2 * 255).long() if normalize else (x * 255).long()


def bpd_and_grads(p, x, normalize):
    """(bpd, {key: gradient}) in float64 through autograd on W * mask (masked entries get exactly 0)."""
    q = {k: (v.double().clone().requires_grad_() if v.is_floating_point() and k != "log2" else v) for k, v in p.items()}
    nll = F.cross_entropy(forward(q, x.double()), target(x, normalize), reduction="none")
    bpd = (nll.mean([1, 2, 3]) / torch.log(torch.tensor(2.0, dtype=torch.float64))).mean()
    bpd.backward()
    return bpd.detach(), {k: v.grad for k, v in q.items() if torch.is_tensor(v) and v.requires_grad}


def pick(probs, u):
    """probs [..., 256] (rows sum to 1), u [...]: (k, distance of u to the two CDF boundaries that bracket the pick)."""
    cdf = probs.cumsum(-1)
    k = (cdf <= u[..., None]).sum(-1).clamp(max=255)
    hi = cdf.gather(-1, k[..., None])[..., 0]
    lo = torch.where(k > 0, cdf.gather(-1, (k - 1).clamp(min=0)[..., None])[..., 0], torch.zeros_like(hi))
    return k, torch.minimum((u - lo).abs(), (hi - u).abs())
