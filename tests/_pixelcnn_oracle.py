"""CPU restatement of the reference PixelCNN (src/models/pixelcnn.py) in plain torch, for the GPU parity tests.

`forward(p, x, onehot)` takes a state_dict-like mapping (masks included) and returns logits [N, 256, C, H, W] with the weights
multiplied by their masks; `pick(probs, u)` is the sampler's inverse-CDF rule k = min{k : cdf_k > u}, clamped to 255."""
import torch
import torch.nn.functional as F

DILATIONS = (1, 2, 1, 4, 1, 2, 1, 4, 1, 2, 1)


def _mconv(p, pre, x, dilation=1):
    w = p[pre + ".conv.weight"] * p[pre + ".mask"]
    kh, kw = w.shape[2:]
    return F.conv2d(x, w, p[pre + ".conv.bias"], padding=(dilation * (kh - 1) // 2, dilation * (kw - 1) // 2), dilation=dilation)


def forward(p, x, onehot=None):
    x = x.double() if p["conv_out.weight"].dtype == torch.float64 else x
    v = _mconv(p, "conv_vstack", x)
    h = _mconv(p, "conv_hstack", x)
    y = None if onehot is None else onehot.reshape(onehot.shape[0], -1, 1, 1).to(x.dtype)
    for l, d in enumerate(DILATIONS):
        q = f"conv_layers.{l}."
        vc = _mconv(p, q + "vert_conv", v, d)
        v1, v2 = vc.chunk(2, 1)
        if y is not None:
            v1 = v1 + F.conv2d(y, p[q + "cond_proj_vert1.weight"])
            v2 = v2 + F.conv2d(y, p[q + "cond_proj_vert2.weight"])
        vout = torch.tanh(v1) * torch.sigmoid(v2)
        h1, h2 = (_mconv(p, q + "horiz_conv", h, d) + F.conv2d(vc, p[q + "conv1x1_1.weight"], p[q + "conv1x1_1.bias"])).chunk(2, 1)
        if y is not None:
            h1 = h1 + F.conv2d(y, p[q + "cond_proj_horiz1.weight"])
            h2 = h2 + F.conv2d(y, p[q + "cond_proj_horiz2.weight"])
        h = F.conv2d(torch.tanh(h1) * torch.tanh(h2), p[q + "conv1x1_2.weight"], p[q + "conv1x1_2.bias"]) + h
        v = vout
    out = F.conv2d(F.elu(h), p["conv_out.weight"], p["conv_out.bias"])
    return out.reshape(out.shape[0], 256, out.shape[1] // 256, out.shape[2], out.shape[3])


def target(x, normalize):
    return ((x + 1) / 2 * 255).long() if normalize else (x * 255).long()


def bpd(p, x, onehot, normalize):
    nll = F.cross_entropy(forward(p, x, onehot), target(x, normalize), reduction="none")
    return (nll.mean([1, 2, 3]) / torch.log(torch.tensor(2.0, dtype=nll.dtype))).mean()


def pick(probs, u):
    """probs [..., 256] (rows sum to 1), u [...]: (k, distance of u to the two CDF boundaries that bracket the pick, cdf_{k-1} and cdf_k)."""
    cdf = probs.cumsum(-1)
    k = (cdf <= u[..., None]).sum(-1).clamp(max=255)
    hi = cdf.gather(-1, k[..., None])[..., 0]
    lo = torch.where(k > 0, cdf.gather(-1, (k - 1).clamp(min=0)[..., None])[..., 0], torch.zeros_like(hi))
    return k, torch.minimum((u - lo).abs(), (hi - u).abs())
