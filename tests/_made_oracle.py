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


# ---------------------------------------------------------------------------------------------------- kernel-level references
# float64 restatements of one masked layer, its gradients and the fused head, from degree vectors.  round_bf16: every matrix-core
# operand goes through .bfloat16() first (round to nearest even, as the kernels' bf16 mode rounds them); bf16 x bf16 products are
# exact in fp32, so what is left between these and the kernel is fp32 accumulation order (and expf).  The bias, the sigmoid,
# s (1 - s), the log-sum-exp and the softmax stay unrounded.  The mask is applied after rounding: the kernel selects after loading.
LN2 = float(torch.log(torch.tensor(2.0, dtype=torch.float64)))   # as bpd_and_grads; the kernels' fp32 ln 2 is 2.7e-8 off

# |sum over a pixel's 256 classes of exp(v - lse) - onehot| of an fp32 torch evaluation on the CPU, measured by
# test_made_cpu.py::test_dlogits_zero_sum_fp32_floor (6.26e-7).  The GPU tests allow 4x this.
ZERO_SUM_FP32 = 6.3e-7


def _op(t, round_bf16):
    return t.detach().cpu().float().bfloat16().double() if round_bf16 else t.detach().cpu().double()


def live_mask(din, dout):
    """M[o][i] = deg_out[o] >= deg_in[i]."""
    return dout.cpu()[:, None] >= din.cpu()[None, :]


def masked_linear_ref(x, w, b, din, dout, act, round_bf16=False):
    """y [N, out] = act(x (W .* M)^T + b)."""
    y = _op(x, round_bf16) @ (_op(w, round_bf16) * live_mask(din, dout)).t() + b.detach().cpu().double()
    return torch.sigmoid(y) if act else y


def masked_dgrad_ref(gy, w, din, dout, s_in=None, round_bf16=False):
    """dx [N, in] = (gy (W .* M)) * s_in (1 - s_in)  (s_in None: no factor)."""
    dx = _op(gy, round_bf16) @ (_op(w, round_bf16) * live_mask(din, dout))
    if s_in is not None:
        s = s_in.detach().cpu().double()
        dx = dx * s * (1 - s)
    return dx


def masked_wgrad_ref(gy, x, din, dout, round_bf16=False):
    """(dW [out, in] = (gy^T x) .* M, db [out] = column sums of the unrounded gy)."""
    return (_op(gy, round_bf16).t() @ _op(x, round_bf16)) * live_mask(din, dout), gy.detach().cpu().double().sum(0)


def head_ref(h, w, b, din, dout, img, normalize, round_bf16=False, gscale=1.0, chunk=64):
    """The fused head: (logits [N, D, 256], lse [N, D], bpd, dlogits [N, 256 D]) for h [N, Hd], w [256 D, Hd], img [N, D] (fp32: the
    target truncates in fp32 as the reference does).  dlogits = (softmax - onehot) * gscale / (N D ln 2).  Evaluated `chunk` pixels
    at a time, so the full-size head never holds a second float64 copy of its weights."""
    n, D = h.shape[0], w.shape[0] // 256
    hh = _op(h, round_bf16)
    dinc, doutc = din.cpu(), dout.cpu()
    logits = torch.empty(n, D, 256, dtype=torch.float64)
    for d0 in range(0, D, chunk):
        sl = slice(d0 * 256, min(D, d0 + chunk) * 256)
        wm = _op(w[sl], round_bf16) * live_mask(dinc, doutc[sl])
        logits[:, d0:d0 + chunk] = (hh @ wm.t() + b[sl].detach().cpu().double()).reshape(n, -1, 256)
    lse = torch.logsumexp(logits, -1)
    t = target(img.detach().cpu().float().reshape(n, D), normalize).clamp(0, 255)
    nll = lse - logits.gather(-1, t[..., None])[..., 0]
    bpd = nll.sum() / (n * D * LN2)
    dl = torch.exp(logits - lse[..., None])
    dl.scatter_add_(-1, t[..., None], torch.full((n, D, 1), -1.0, dtype=torch.float64))
    return logits, lse, bpd, (dl * (gscale / (n * D * LN2))).reshape(n, D * 256)
