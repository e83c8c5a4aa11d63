"""`MADE` with the reference's surface (src/models/made.py) on the HIP kernels of csrc/made.hip.

Same constructor, attributes (`model` is the MADENet, `model.layers`, `model.reset_mask()`, the `log2` buffer), `state_dict` keys
and order (`log2`, then per layer `model.model.{i}.mask` (bool), `.model.weight`, `.model.bias`), the same seeded init (every
nn.Linear in construction order, then the `randint` degree draws of `reset_mask`), the same logged keys (`train_bpd`,
`val_bpd`), Adam(lr) + StepLR(1, 0.99).  Every parameter is a PyTorch-shaped view of one flat fp32 buffer (what FlatAdam
updates in one launch).  The kernels never read the masks: they take int32 degree vectors derived from the mask buffers
(`mask[o][i] = deg_out[o] >= deg_in[i]`; a mask not of that form raises) at construction, after `reset_mask()` and after
`load_state_dict`, and select the live weights.  Masked weights get gradient exactly 0 and keep their values, as in the
reference.  `forward(x)` is the only place the [N, 256, C, H, W] logits are materialised: the training step fuses the output
head with the log-sum-exp and the NLL.  Sampling replays one captured hipGraph per raster position (src/runtime/made_sampler.py).

Supported sizes: D = C*H*W >= 1, `channels` 1..4, `hidden_dim` a multiple of 4 in 4..8192 (anything else raises here).  There
is no CPU path: a CPU tensor raises.

Compute modes (`compute_mode`, set from MI_DDPM_MODE or by `trainer.precision=bf16-mixed`): "fp32" runs every product on
fp32-exact MFMA, "bf16" rounds the operands to bf16 at the MFMA with fp32 accumulation.  Weights, moments, the log-sum-exp and
the sampling softmax stay fp32 in both modes; the bf16 operands are converted on the fly (no bf16 weight copy).

Sampling randomness: the value is the inverse CDF of the fp32 softmax at a Philox uniform (k = min{k : cdf_k > u}) instead of
`torch.multinomial`: the same distribution, different draws.  `uniform_source(shape, device)` supplies a tape.
"""
import math
import os

import torch
from torch import nn

from ..ops import functional as K
from .base import BaseModel, ValidationResult

N_CLASS = 256


class _Node(nn.Module):
    """Anonymous container; the module tree exists only to reproduce the reference's keys."""


def recover_degrees(masks):
    """Degree vectors [(deg_in, deg_out)] (int32, one pair per layer) with mask[o][i] == (deg_out[o] >= deg_in[i]) for every layer.

    The first layer's inputs have degrees 0..D-1.  A layer's output unit takes the largest input degree it sees; units that see
    the same inputs are ordered by how many units of the next layer see them (more consumers: lower degree), which is the order
    their true degrees have.  Each layer's pair is then ranked into a compact int32 range.  A mask that is not of the degree form
    raises ValueError."""
    dev = masks[0].device
    v_in = torch.arange(masks[0].shape[1], device=dev, dtype=torch.int64)
    out = []
    for l, mk in enumerate(masks):
        if mk.dtype != torch.bool or mk.dim() != 2 or mk.shape[1] != v_in.numel():
            raise ValueError(f"MADE: mask {l} has shape {tuple(mk.shape)} / dtype {mk.dtype}; a bool [out, in] mask chained to the previous layer expected")
        if l + 1 < len(masks):
            cnt = masks[l + 1].sum(0)
            _, s = torch.unique(-cnt, return_inverse=True)
            G = int(s.max()) + 2
        else:
            s, G = torch.zeros(mk.shape[0], dtype=torch.int64, device=dev), 1
        a = v_in * G
        a_sorted, _ = torch.sort(a)
        cnt_row = mk.sum(1)
        base = torch.where(cnt_row > 0, a_sorted[(cnt_row - 1).clamp(min=0)], a_sorted[0] - G)
        v_out = base + s
        u = torch.unique(torch.cat([a, v_out]))
        din = torch.searchsorted(u, a).to(torch.int32)
        dout = torch.searchsorted(u, v_out).to(torch.int32)
        for r0 in range(0, mk.shape[0], 8192):
            if not torch.equal(mk[r0:r0 + 8192], dout[r0:r0 + 8192, None] >= din[None, :]):
                raise ValueError(f"MADE: mask {l} is not of the degree form mask[o][i] = deg_out[o] >= deg_in[i]")
        out.append((din, dout))
        v_in = dout.to(torch.int64)
    return out


class MADENet(nn.Module):
    """The reference's MADENet as a key container: `layers` (a plain list) and `model` (nn.Sequential) hold the same masked
    layers; each has a bool `mask` buffer and a `model` child with `weight` / `bias` (views of the owner's flat buffer)."""

    def __init__(self, in_dim, hidden_dim, n_class, n_layer, on_mask=None):
        super().__init__()
        self.in_dim, self.hidden_dim, self.n_class, self.n_layer = in_dim, hidden_dim, n_class, n_layer
        dims = [in_dim] + [hidden_dim] * n_layer + [in_dim * n_class]
        self.layers = []
        for fi, fo in zip(dims[:-1], dims[1:]):
            node = _Node()
            node.register_buffer("mask", torch.ones(0, dtype=torch.bool))
            node.add_module("model", _Node())
            node.in_features, node.out_features = fi, fo
            self.layers.append(node)
        self.model = nn.Sequential(*self.layers)
        object.__setattr__(self, "_on_mask", on_mask)

    def reset_mask(self):
        """The reference's draws: hidden degrees torch.randint(low, D, (hidden,)), low = min of the previous draw."""
        low, high = 0, self.in_dim
        data_unit = torch.arange(0, high)
        units = [data_unit]
        for _ in range(self.n_layer):
            hu = torch.randint(low=low, high=high, size=(self.hidden_dim,))
            units.append(hu)
            low = int(hu.min())
        units.append(data_unit.unsqueeze(1).repeat(1, self.n_class).reshape(-1) - 1)
        for layer, iu, ou in zip(self.layers, units[:-1], units[1:]):
            layer.mask = (ou.unsqueeze(1) >= iu).to(layer.mask.device)
        if self._on_mask is not None:
            self._on_mask()


class _MADEStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, anchor, model):
        x = img.float().contiguous().reshape(img.shape[0], -1)
        acts = model._hidden(x)
        lw, lb = model._wb(model.n_layer)
        din, dout = model._deg[model.n_layer]
        loss, lse = K.made_head_fwd(acts[-1], lw, lb, din, dout, x, model.input_normalize, mode=model._mode())
        ctx.model, ctx.saved = model, (x, acts, lse)
        return loss.view(())

    @staticmethod
    def backward(ctx, dloss):
        model = ctx.model
        saved, ctx.saved = ctx.saved, None
        model._backward(*saved, dloss.reshape(1).float().contiguous())
        return None, None, None


class MADE(BaseModel):
    def __init__(self, datamodule, hidden_dim, n_layer, lr=1e-3):
        super().__init__(datamodule)
        self.save_hyperparameters()
        D = self.width * self.height * self.channels
        if not 1 <= self.channels <= 4:
            raise ValueError(f"MADE: channels={self.channels} is not supported; the head and the sampler take 1..4 channels")
        from ..ops.lib import load_library
        if n_layer < 1 or not load_library().mi_made_supported(D, hidden_dim, self.channels):
            raise ValueError(f"MADE: hidden_dim={hidden_dim}, n_layer={n_layer} is not supported; the HIP kernels take n_layer >= 1 and a "
                             "hidden_dim that is a multiple of 4 in 4..8192")
        self.D, self.hidden_dim, self.n_layer = D, hidden_dim, n_layer
        self.uniform_source = None
        self.compute_mode = os.environ.get("MI_DDPM_MODE", "fp32")
        self._samplers = {}
        self._deg = None
        self._gflat = None

        net = MADENet(D, hidden_dim, n_class=N_CLASS, n_layer=n_layer, on_mask=self._refresh_degrees)
        self.model = net
        self.register_buffer("log2", torch.log(torch.tensor(2, dtype=torch.float32)))
        # flat buffer: per layer weight [out][in] then bias [out], in construction order (= the reference's RNG draw order)
        self._entries = []
        off = 0
        for i, node in enumerate(net.layers):
            fi, fo = node.in_features, node.out_features
            self._entries.append((i, (fo, fi), off, (fo,), off + fo * fi))
            off += fo * fi + fo
        flat = torch.empty((off + 63) // 64 * 64)
        flat[off:].zero_()
        self._params = []
        for i, wshape, woff, bshape, boff in self._entries:       # nn.Linear.reset_parameters, in construction order
            w = flat[woff:woff + math.prod(wshape)].view(wshape)
            nn.init.kaiming_uniform_(w, a=math.sqrt(5))
            bound = 1 / math.sqrt(wshape[1])
            flat[boff:boff + bshape[0]].uniform_(-bound, bound)
            lin = net.layers[i].model
            for name, o, shp in (("weight", woff, wshape), ("bias", boff, bshape)):
                prm = nn.Parameter(flat[o:o + math.prod(shp)].view(shp))
                lin.register_parameter(name, prm)
                self._params.append(prm)
        self._bind(flat)
        net.reset_mask()
        object.__setattr__(self, "_anchor", torch.zeros(1, requires_grad=True))

    # ------------------------------------------------------------------ flat storage (the FlatNet contract)
    def _bind(self, flat):
        self._flat = flat
        views = []
        for i, wshape, woff, bshape, boff in self._entries:
            views += [(woff, wshape), (boff, bshape)]
        for (o, shp), p in zip(views, self._params):
            p.data = flat[o:o + math.prod(shp)].view(shp)
        if self._gflat is not None and self._gflat.device != flat.device:
            self._gflat = None
            for p in self._params:
                p.grad = None

    def _apply(self, fn, recurse=True):
        new = fn(self._flat)
        if new.dtype != torch.float32:
            raise RuntimeError("MADE keeps fp32 weights")
        if new is not self._flat:
            self._bind(new)
        for mod in self.modules():
            for key, buf in mod._buffers.items():
                if buf is not None:
                    mod._buffers[key] = fn(buf)
        if self._deg is not None:
            self._deg = [(a.to(new.device), b.to(new.device)) for a, b in self._deg]
        self._samplers = {}
        return self

    @property
    def flat_params(self):
        return self._flat

    @property
    def flat_grads(self):
        if self._gflat is None:
            self._gflat = torch.zeros_like(self._flat)          # masked entries are never written: they stay 0
            for p in self._params:
                off = (p.data.data_ptr() - self._flat.data_ptr()) // 4
                p.grad = self._gflat[off:off + p.numel()].view(p.shape)
        return self._gflat

    def mark_params_dirty(self):
        pass                                            # the kernels read the flat buffer itself; nothing is derived from it

    def flat_nets(self):
        return [self]

    def zero_grad(self, set_to_none: bool = False):
        if self._gflat is not None:
            self._gflat.zero_()

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(state_dict, strict=strict, assign=False)
        self._refresh_degrees()
        return out

    def _refresh_degrees(self):
        dev = self._flat.device
        self._deg = [(a.to(dev), b.to(dev)) for a, b in recover_degrees([l.mask for l in self.model.layers])]
        self._samplers = {}

    def _wb(self, i):
        lin = self.model.layers[i].model
        return lin.weight.data, lin.bias.data

    def _gwb(self, i):
        g = self.flat_grads
        _, wshape, woff, bshape, boff = self._entries[i]
        return g[woff:woff + math.prod(wshape)].view(wshape), g[boff:boff + bshape[0]]

    def _mode(self):
        if self.compute_mode not in ("fp32", "bf16"):
            raise ValueError(f"MADE: compute_mode={self.compute_mode!r}; 'fp32' or 'bf16'")
        return K.MODE_BF16 if self.compute_mode == "bf16" else K.MODE_FP32

    # ------------------------------------------------------------------ forward / backward on [N, D] rows
    def _hidden(self, x):
        """Sigmoid outputs of the hidden layers for x [N, D] (fp32, on the device)."""
        if not x.is_cuda:
            raise RuntimeError("MADE: input is not on a HIP device; this implementation has no CPU path")
        mode, acts, h = self._mode(), [], x
        for i in range(self.n_layer):
            w, b = self._wb(i)
            din, dout = self._deg[i]
            h = K.made_linear(h, w, b, din, dout, True, mode=mode)
            acts.append(h)
        return acts

    def _backward(self, x, acts, lse, gscale):
        mode, L = self._mode(), self.n_layer
        w, b = self._wb(L)
        din, dout = self._deg[L]
        dl = K.made_head_dlogits(acts[-1], w, b, din, dout, x, self.input_normalize, lse, gscale=gscale, mode=mode)
        gw, gb = self._gwb(L)
        K.made_wgrad(dl, acts[-1], din, dout, gw, gb, mode=mode)
        g = K.made_dgrad(dl, w, din, dout, s_in=acts[-1], mode=mode)
        for i in reversed(range(L)):
            xin = x if i == 0 else acts[i - 1]
            din, dout = self._deg[i]
            gw, gb = self._gwb(i)
            K.made_wgrad(g, xin, din, dout, gw, gb, mode=mode)
            if i > 0:
                g = K.made_dgrad(g, self._wb(i)[0], din, dout, s_in=acts[i - 1], mode=mode)

    # ------------------------------------------------------------------ the reference's surface
    def forward(self, x, y=None):
        """Logits [N, 256, C, H, W] for x in the datamodule's range (the only place they are materialised)."""
        with torch.no_grad():
            n, c, hh, ww = x.shape
            xf = x.float().contiguous().reshape(n, -1)
            acts = self._hidden(xf)
            w, b = self._wb(self.n_layer)
            din, dout = self._deg[self.n_layer]
            lg = K.made_linear(acts[-1], w, b, din, dout, False, mode=self._mode())
        return lg.view(n, c, hh, ww, N_CLASS).permute(0, 4, 1, 2, 3)

    def calc_likelihood(self, x, label=None):
        """Mean bits per dim; differentiable into the flat gradient buffer (one autograd node)."""
        if self._anchor.device != x.device:
            object.__setattr__(self, "_anchor", torch.zeros(1, device=x.device, requires_grad=True))
        anchor = self._anchor if torch.is_grad_enabled() else self._anchor.detach()
        return _MADEStep.apply(x, anchor, self)

    @torch.no_grad()
    def sample(self, img_shape, cond=None, img=None):
        """Autoregressive sampling in raster order over (h, w); pixels to fill are -1 in `img` (default: all).  `cond` is ignored."""
        from ..runtime.made_sampler import MADESampler
        shape = tuple(int(s) for s in img_shape)
        s = self._samplers.get(shape)
        if s is None:
            s = self._samplers[shape] = MADESampler(self, shape)
        return s.run(img=img)

    def configure_optimizers(self):
        from ..runtime.optim import FlatAdam
        opt = FlatAdam(self, lr=self.hparams.lr)
        scheduler = torch.optim.lr_scheduler.StepLR(opt, 1, gamma=0.99)
        return [opt], [scheduler]

    def training_step(self, batch, batch_idx):
        img, label = batch
        loss = self.calc_likelihood(img)
        self.log("train_bpd", loss.detach())
        return loss

    def validation_step(self, batch, batch_idx):
        img, label = batch
        with torch.no_grad():
            loss = self.calc_likelihood(img)
        self.log("val_bpd", loss)
        sample_img = None
        if batch_idx == 0:
            sample_img = self.sample(img.shape)
        return ValidationResult(real_image=img, fake_image=sample_img)
