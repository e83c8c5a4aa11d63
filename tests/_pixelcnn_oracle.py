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


# ---------------------------------------------------------------------------------------------------- kernel-level references
# float64 restatements of the single operations of csrc/pixelcnn.hip for tests/test_pixelcnn_kernels_gpu.py.  round_bf16: every
# matrix-core operand goes through .bfloat16() first (round to nearest even, as the kernels' bf16 mode rounds them where they feed
# the MFMA: x after its ELU when elu_in is set, x2, w * mask, w2, dy and the other operand of each gradient); bf16 x bf16 products are
# exact in fp32, so what is left between these and the kernel is fp32 accumulation order.  Biases, res, cond, aux and everything
# else in an epilogue stay unrounded.
LN2 = float(torch.log(torch.tensor(2.0, dtype=torch.float64)))     # the kernels' fp32 ln 2 is 2.7e-8 off


def op(t, round_bf16=False):
    t = t.detach().cpu()
    return t.float().bfloat16().double() if round_bf16 else t.double()


def elu_d(a):
    """ELU' as the kernel and torch define it: 1 for a > 0, exp(a) otherwise (1 at exactly 0)."""
    a = a.double()
    return torch.where(a > 0, torch.ones_like(a), torch.exp(a))


def _pad(mask, dil):
    return (dil * (mask.shape[0] - 1) // 2, dil * (mask.shape[1] - 1) // 2)


def conv_ref(x, w, mask, b, dil=1, round_bf16=False, elu_in=False):
    """y [N, Cout, H, W] = conv2d(elu?(x), w * mask) + b for x [N, Cin, H, W], mask [KH, KW]."""
    xx = F.elu(x.double()) if elu_in else x
    y = F.conv2d(op(xx, round_bf16), op(w * mask, round_bf16), None, padding=_pad(mask, dil), dilation=dil)
    return y if b is None else y + b.double()[None, :, None, None]


def conv_grads_ref(x, w, mask, dy, dil=1, round_bf16=False):
    """(dx, dw * mask) of conv_ref through float64 autograd, each gradient's two operands rounded when asked."""
    xr, wr = op(x, round_bf16).requires_grad_(), op(w * mask, round_bf16).requires_grad_()
    F.conv2d(xr, wr, None, padding=_pad(mask, dil), dilation=dil).backward(op(dy, round_bf16))
    return xr.grad, wr.grad * mask.double()


def gate(pre, cond, ts):
    """tanh(a) * sigmoid(b) (ts) or tanh(a) * tanh(b) of pre [N, 2C, H, W] (+ cond [N, 2C]) split in halves."""
    pre = pre.double()
    if cond is not None:
        pre = pre + cond.double()[:, :, None, None]
    a, b = pre.chunk(2, 1)
    return torch.tanh(a) * (torch.sigmoid(b) if ts else torch.tanh(b))


def gate_bwd_ref(pre, cond, dout, ts):
    """(d pre [N, 2C, H, W], sum over the pixels [N, 2C]) of gate() through float64 autograd."""
    p = pre.double().clone().requires_grad_()
    (gate(p, cond, ts) * dout.double()).sum().backward()
    return p.grad, p.grad.sum((2, 3))


def head_logits(h, w, b, dtype=torch.float64):
    """[P, Cc, 256] logits of elu(h) [P, Ch] under w [256 Cc, Ch] (row o = k * Cc + colour).  dtype float32: the kernel's own order, a
    sequential chain over the hidden units from the bias, each step rounded to fp32 (the CPU stand-in for the fp32 floor)."""
    a, w, b = F.elu(h.to(dtype)), w.to(dtype), b.to(dtype)
    if dtype == torch.float64:
        l = a @ w.t() + b
    else:
        l = b[None].expand(a.shape[0], -1).clone()
        for c in range(a.shape[1]):
            l += a[:, c:c + 1] * w[None, :, c]
    return l.reshape(a.shape[0], 256, -1).permute(0, 2, 1)


def head_ref(h, w, b, img, normalize, gscale=1.0, dtype=torch.float64):
    """The fused head on h [N, H, W, Ch] (NHWC), img [N, Cc, H, W]: (lse [N, H, W, Cc], bpd, dlogits [N, H, W, 256 Cc]) with
    dlogits = (softmax - onehot) * gscale / (N Cc H W ln 2) at column k * Cc + colour."""
    n, hh, ww, ch = h.shape
    cc = img.shape[1]
    l = head_logits(h.reshape(-1, ch), w, b, dtype)
    lse = torch.logsumexp(l, -1)
    t = target(img.float(), normalize).clamp(0, 255).permute(0, 2, 3, 1).reshape(-1, cc)
    nll = lse - l.gather(-1, t[..., None])[..., 0]
    units = n * hh * ww * cc
    dl = torch.exp(l - lse[..., None])
    dl.scatter_add_(-1, t[..., None], torch.full(t.shape + (1,), -1.0, dtype=dtype))
    dl = (dl * (gscale / (units * LN2))).permute(0, 2, 1).reshape(n, hh, ww, 256 * cc)
    return lse.reshape(n, hh, ww, cc), nll.sum() / (units * LN2), dl


def grid(k, normalize):
    """The value the samplers write for class k, in fp32 as the kernel forms it."""
    v = k.float() / 255
    return v * 2 - 1 if normalize else v


# The sampling step's direct test (and the CPU count of its skip band): N x Cc units on a 2 x 4 raster, hidden width 20, logits of
# standard deviation 16 (peaked, as a trained net's: the CDF boundaries of the near-zero classes coincide).
SAMPLE_UNITS = [(1, 1), (5, 3), (64, 4), (100, 3)]           # N * Cc = 1, 15, 256, 300
SAMPLE_HW = (2, 4)
SAMPLE_CH = 20
SAMPLE_PIXELS = (0, 3, 7, 2)


def sample_scenario(n, cc, normalize):
    """(h [N, H, W, Ch], w [256 Cc, Ch], b, tape [H W, N Cc], float64 logits [H W, N Cc, 256]) from a seed of its own."""
    g = torch.Generator().manual_seed(7000 + 10 * n + cc + (5 if normalize else 0))
    hh, ww = SAMPLE_HW
    h = torch.randn(n, hh, ww, SAMPLE_CH, generator=g)
    w = torch.randn(256 * cc, SAMPLE_CH, generator=g)
    b = torch.randn(256 * cc, generator=g)
    s = 16.0 / float(head_logits(h.reshape(-1, SAMPLE_CH), w, b).std())
    w, b = (w * s).float(), (b * s).float()
    tape = torch.rand(hh * ww, n * cc, generator=g)
    l = head_logits(h.reshape(-1, SAMPLE_CH), w, b).reshape(n, hh * ww, cc, 256).permute(1, 0, 2, 3).reshape(hh * ww, n * cc, 256)
    return h, w, b, tape, l


def sample_picks(l, tape, pix):
    """(k, near) of unit u at pixel pix: the float64 inverse-CDF pick and whether its uniform lies within 1e-5 of a CDF boundary."""
    k, dist = pick(F.softmax(l[pix], -1), tape[pix].double())
    return k, dist < 1e-5
