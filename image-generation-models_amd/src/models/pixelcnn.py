"""`PixelCNN` with the reference's surface (src/models/pixelcnn.py) on the HIP kernels of csrc/pixelcnn.hip.

Same constructor, attribute names, `state_dict` keys and order (`log2`, then every masked conv's `mask` before its `conv.weight` /
`conv.bias`, ...), the same seeded init, the same logged keys (`train_bpd`, `val_bpd`), Adam(lr) + StepLR(1, 0.99).
Every parameter is a PyTorch-shaped view of one flat fp32 buffer (what FlatAdam updates in one launch); the kernels read the
weights in that layout directly.  `forward(x, y)` is the only place the [N, 256, C, H, W] logits are materialised: the training
step fuses ELU -> 1x1 -> log-sum-exp -> NLL and never writes them.  Sampling replays one captured hipGraph per pixel (full-image
forward + the sampling kernel, device-side pixel counter, uniforms drawn up front).

Supported shapes: `hidden_dim` a multiple of 8, `channels` 1..4 (anything else raises here).

Deliberate deviations from the reference:
  * Masked weight entries.  The reference re-masks the weights before every conv (`weight.data *= mask`), but its autograd still
    gives the masked entries non-zero gradients, so Adam moves them between forwards.  Here their gradient is 0 by definition
    (the kernels never touch masked taps); they are zeroed at the first forward and after `load_state_dict`, and stay 0.  The
    unmasked weights follow the reference's trajectory.
  * Sampling randomness.  The pixel value is the inverse CDF of the fp32 softmax at a Philox uniform (k = min{k : cdf_k > u})
    instead of `torch.multinomial`: the same distribution, different draws.  `uniform_source(shape, device)` supplies a tape.
Compute modes (`compute_mode`, set from MI_DDPM_MODE or by `trainer.precision=bf16-mixed`): "fp32" runs the convolutions on
fp32-exact MFMA, "bf16" rounds their operands to bf16 at the MFMA (fp32 accumulate, fp32 storage).  The output head's
log-sum-exp and the sampling softmax stay fp32 in both modes.
"""
import math
import os

import torch
from torch import nn

from ..ops import functional as K
from .base import BaseModel, ValidationResult

DILATIONS = (1, 2, 1, 4, 1, 2, 1, 4, 1, 2, 1)


class _Node(nn.Module):
    """Anonymous container; the module tree exists only to reproduce the reference's keys."""


def vertical_mask(k, mask_center=False):
    m = torch.ones(k, k)
    m[k // 2 + 1:, :] = 0
    if mask_center:
        m[k // 2] = 0
    return m


def horizontal_mask(k, mask_center=False):
    m = torch.ones(1, k)
    m[0, k // 2 + 1:] = 0
    if mask_center:
        m[0, k // 2] = 0
    return m


def live_taps(mask, dilation=1):
    """[(dy, dx, tap index)] of the mask's non-zero taps with nn.Conv2d's padding dilation*(k-1)//2 (pixelcnn.py:17)."""
    kh, kw = mask.shape
    ph, pw = dilation * (kh - 1) // 2, dilation * (kw - 1) // 2
    return [(i * dilation - ph, j * dilation - pw, i * kw + j) for i in range(kh) for j in range(kw) if mask[i, j] != 0]


def _neg(taps):
    return [(-a, -b, t) for a, b, t in taps]


_ONE = [(0, 0, 0)]


class _PixelCNNStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, cond, anchor, model):
        img = img.float().contiguous()
        xin = K.nchw_to_nhwc(img)
        h, tape, condb = model._forward_nhwc(xin, cond, record=True)
        loss, lse = K.pcnn_head_fwd(h, model._w("conv_out.weight"), model._w("conv_out.bias"), img, model.input_normalize)
        ctx.model, ctx.saved = model, (img, xin, cond, h, tape, condb, lse)
        return loss.view(())

    @staticmethod
    def backward(ctx, dloss):
        model = ctx.model
        saved, ctx.saved = ctx.saved, None
        model._backward(*saved, dloss.reshape(1).float().contiguous())
        return None, None, None, None


class PixelCNN(BaseModel):
    def __init__(self, datamodule, hidden_dim, class_condition=False, n_classes=None, lr=1e-3):
        super().__init__(datamodule)
        self.save_hyperparameters()
        if hidden_dim % 8 != 0 or hidden_dim < 8:
            raise ValueError(f"PixelCNN: hidden_dim={hidden_dim} is not supported; the HIP kernels take a positive multiple of 8")
        if not 1 <= self.channels <= 4:
            raise ValueError(f"PixelCNN: channels={self.channels} is not supported; the output head takes 1..4 colour channels")
        from ..ops.lib import load_library
        if not load_library().mi_pcnn_head_supported(self.channels, hidden_dim):
            raise ValueError(f"PixelCNN: hidden_dim={hidden_dim} is not supported; the output head takes at most 248 hidden channels")
        if class_condition and not (n_classes and n_classes >= 1):
            raise ValueError("PixelCNN: class_condition=True needs n_classes")
        C, ch = hidden_dim, self.channels
        ncls = n_classes if class_condition else 0
        self.hidden_dim, self.n_cond = C, ncls
        self.uniform_source = None
        self.compute_mode = os.environ.get("MI_DDPM_MODE", "fp32")
        self._samplers = {}

        # parameter table in the reference's construction order (= its RNG draw order); cond_proj weights of all layers go to one
        # contiguous [11 * 4 * C][n_classes] block at the end of the flat buffer (one launch computes every layer's conditioning)
        ents, masks = [], []

        def conv(pre, o, i, kh, kw, bias=True, cond=False):
            ents.append((pre + "weight", (o, i, kh, kw), "cond" if cond else "main"))
            if bias:
                ents.append((pre + "bias", (o,), "main"))

        conv("conv_vstack.conv.", C, ch, 5, 5)
        conv("conv_hstack.conv.", C, ch, 1, 5)
        masks += [("conv_vstack", vertical_mask(5, True)), ("conv_hstack", horizontal_mask(5, True))]
        for l in range(len(DILATIONS)):
            p = f"conv_layers.{l}."
            conv(p + "horiz_conv.conv.", 2 * C, C, 1, 3)
            conv(p + "vert_conv.conv.", 2 * C, C, 3, 3)
            conv(p + "conv1x1_1.", 2 * C, 2 * C, 1, 1)
            conv(p + "conv1x1_2.", C, C, 1, 1)
            masks += [(p + "horiz_conv", horizontal_mask(3)), (p + "vert_conv", vertical_mask(3))]
            if class_condition:
                for nm in ("cond_proj_vert1", "cond_proj_vert2", "cond_proj_horiz1", "cond_proj_horiz2"):
                    conv(p + nm + ".", C, ncls, 1, 1, bias=False, cond=True)
        conv("conv_out.", 256 * ch, C, 1, 1)

        off, offs = 0, {}
        for key, shape, kind in ents:
            if kind == "main":
                offs[key] = off
                off += math.prod(shape)
        self._cond_off = off
        for key, shape, kind in ents:
            if kind == "cond":
                offs[key] = off
                off += math.prod(shape)
        flat = torch.zeros((off + 63) // 64 * 64)
        for key, shape, _ in ents:                      # nn.Conv2d.reset_parameters, in construction order
            n = math.prod(shape)
            view = flat[offs[key]:offs[key] + n].view(shape)
            if key.endswith("weight"):
                w = torch.empty(shape)
                nn.init.kaiming_uniform_(w, a=math.sqrt(5))
                view.copy_(w)
            else:
                fan = math.prod(next(s for k, s, _ in ents if k == key[:-4] + "weight")[1:])
                bound = 1 / math.sqrt(fan)
                view.copy_(torch.empty(shape).uniform_(-bound, bound))

        # module tree with the reference's keys: log2, then per masked conv its mask before conv.weight / conv.bias
        self.register_buffer("log2", torch.log(torch.tensor(2, dtype=torch.float32)))
        mask_of = dict(masks)
        self._entries = [(key, shape, offs[key]) for key, shape, _ in ents]
        self._params = []
        for key, shape, _ in ents:
            parts = key.split(".")
            node = self
            for i, name in enumerate(parts[:-1]):
                if name not in node._modules:
                    sub = _Node()
                    node.add_module(name, sub)
                    path = ".".join(parts[:i + 1])
                    if path in mask_of:
                        sub.register_buffer("mask", mask_of[path])
                node = node._modules[name]
            prm = nn.Parameter(flat[offs[key]:offs[key] + math.prod(shape)].view(shape))
            node.register_parameter(parts[-1], prm)
            self._params.append(prm)
        self._masked = [pre for pre, _ in masks]
        self._taps = {"v5": live_taps(vertical_mask(5, True)), "h5": live_taps(horizontal_mask(5, True))}
        for d in set(DILATIONS):
            self._taps[f"v{d}"] = live_taps(vertical_mask(3), d)
            self._taps[f"h{d}"] = live_taps(horizontal_mask(3), d)
        self._gflat = None
        self._mask_stale = True
        self._bind(flat)
        object.__setattr__(self, "_anchor", torch.zeros(1, requires_grad=True))

    # ------------------------------------------------------------------ flat storage (the FlatNet contract)
    def _bind(self, flat):
        self._flat = flat
        for (key, shape, off), p in zip(self._entries, self._params):
            p.data = flat[off:off + math.prod(shape)].view(shape)
        self._views = {key: p.data for (key, _, _), p in zip(self._entries, self._params)}
        if self._gflat is not None and self._gflat.device != flat.device:
            self._gflat = None
            for p in self._params:
                p.grad = None

    def _apply(self, fn, recurse=True):
        new = fn(self._flat)
        if new.dtype != torch.float32:
            raise RuntimeError("PixelCNN keeps fp32 weights")
        if new is not self._flat:
            self._bind(new)
        for mod in self.modules():
            for key, buf in mod._buffers.items():
                if buf is not None:
                    mod._buffers[key] = fn(buf)
        self._samplers = {}
        return self

    @property
    def flat_params(self):
        return self._flat

    @property
    def flat_grads(self):
        if self._gflat is None:
            self._gflat = torch.zeros_like(self._flat)
            self._gviews = {}
            for (key, shape, off), p in zip(self._entries, self._params):
                p.grad = self._gflat[off:off + math.prod(shape)].view(shape)
                self._gviews[key] = p.grad
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
        self._mask_stale = True
        return out

    def _w(self, key):
        return self._views[key]

    def _g(self, key):
        return self._gviews[key]

    def _apply_masks(self):
        """The reference's `weight.data *= mask`, once: masked entries get no gradient here, so they stay 0 afterwards."""
        if self._mask_stale:
            with torch.no_grad():
                for pre in self._masked:
                    node = self
                    for name in pre.split("."):
                        node = node._modules[name]
                    self._w(pre + ".conv.weight").mul_(node.mask)
            self._mask_stale = False

    # ------------------------------------------------------------------ NHWC forward / backward
    def _mode(self):
        if self.compute_mode not in ("fp32", "bf16"):
            raise ValueError(f"PixelCNN: compute_mode={self.compute_mode!r}; 'fp32' or 'bf16'")
        return K.MODE_BF16 if self.compute_mode == "bf16" else K.MODE_FP32

    def _cond_w(self):
        J = len(DILATIONS) * 4 * self.hidden_dim
        return self._flat[self._cond_off:self._cond_off + J * self.n_cond].view(J, self.n_cond)

    def _cond_bias(self, cond):
        """Per-(sample, channel) gate biases of every layer [N, 11 * 4C] from int64 labels [N] or a float one-hot [N, n_classes]."""
        if cond is None:
            return None
        N, J = cond.shape[0], len(DILATIONS) * 4 * self.hidden_dim
        condb = torch.empty((N, J), device=cond.device)
        if cond.dtype == torch.int64:
            return K.pcnn_cond_rows(cond, self._cond_w(), condb)
        K.pcnn_small_mm(N, J, self.n_cond, cond, self.n_cond, 1, self._cond_w(), 1, self.n_cond, condb, J)
        return condb

    def _forward_nhwc(self, xin, cond, record=False):
        if not xin.is_cuda:
            raise RuntimeError("PixelCNN: input is not on a HIP device; this implementation has no CPU path")
        self._apply_masks()
        C, ch, w = self.hidden_dim, self.channels, self._w
        condb = self._cond_bias(cond)
        mode = self._mode()
        v = K.pcnn_conv(xin, w("conv_vstack.conv.weight"), self._taps["v5"], (25, 25 * ch), C, bias=w("conv_vstack.conv.bias"), mode=mode)
        h = K.pcnn_conv(xin, w("conv_hstack.conv.weight"), self._taps["h5"], (5, 5 * ch), C, bias=w("conv_hstack.conv.bias"), mode=mode)
        tape = []
        for l, d in enumerate(DILATIONS):
            p = f"conv_layers.{l}."
            cv = ch_ = None
            if condb is not None:
                cv, ch_ = condb[:, l * 4 * C:l * 4 * C + 2 * C], condb[:, l * 4 * C + 2 * C:(l + 1) * 4 * C]
            vout, vpre = K.pcnn_conv(v, w(p + "vert_conv.conv.weight"), self._taps[f"v{d}"], (9, 9 * C), 2 * C,
                                     bias=w(p + "vert_conv.conv.bias"), epi=K.PCNN_GATE_TS, cond=cv, mode=mode)
            g, hpre = K.pcnn_conv(h, w(p + "horiz_conv.conv.weight"), self._taps[f"h{d}"], (3, 3 * C), 2 * C,
                                  bias=w(p + "horiz_conv.conv.bias"), x2=vpre, w2=w(p + "conv1x1_1.weight"), w2_strides=(1, 2 * C),
                                  bias2=w(p + "conv1x1_1.bias"), epi=K.PCNN_GATE_TT, cond=ch_, mode=mode)
            hout = K.pcnn_conv(g, w(p + "conv1x1_2.weight"), _ONE, (1, C), C, bias=w(p + "conv1x1_2.bias"), res=h, mode=mode)
            if record:
                tape.append((v, h, vpre, hpre, g))
            v, h = vout, hout
        return h, tape, condb

    def _backward(self, img, xin, cond, h, tape, condb, lse, gscale):
        C, ch, w = self.hidden_dim, self.channels, self._w
        mode = self._mode()
        gflat = self.flat_grads
        K.pcnn_zero(gflat)
        g = self._g
        dcond = None
        if condb is not None:
            dcond = torch.empty_like(condb)
            K.pcnn_zero(dcond)
        dl = K.pcnn_head_dlogits(h, w("conv_out.weight"), w("conv_out.bias"), img, self.input_normalize, lse, gscale=gscale)
        K.pcnn_wgrad(h, dl, g("conv_out.weight"), _ONE, (1, C), elu_in=True, mode=mode)
        K.pcnn_colsum(dl, g("conv_out.bias"))
        dH = K.pcnn_conv(dl, w("conv_out.weight"), _ONE, (C, 1), C, epi=K.PCNN_ELU_GRAD, aux=h, mode=mode)
        dV = None
        for l in reversed(range(len(DILATIONS))):
            d, p = DILATIONS[l], f"conv_layers.{l}."
            v, hx, vpre, hpre, gh = tape[l]
            cv = chh = dcv = dch = None
            if condb is not None:
                a = l * 4 * C
                cv, chh, dcv, dch = condb[:, a:a + 2 * C], condb[:, a + 2 * C:a + 4 * C], dcond[:, a:a + 2 * C], dcond[:, a + 2 * C:a + 4 * C]
            K.pcnn_wgrad(gh, dH, g(p + "conv1x1_2.weight"), _ONE, (1, C), mode=mode)
            K.pcnn_colsum(dH, g(p + "conv1x1_2.bias"))
            dg = K.pcnn_conv(dH, w(p + "conv1x1_2.weight"), _ONE, (C, 1), C, mode=mode)
            dhpre = K.pcnn_gate_bwd(hpre, dg, K.PCNN_GATE_TT, cond=chh, dcond=dch)
            K.pcnn_colsum(dhpre, g(p + "horiz_conv.conv.bias"), g(p + "conv1x1_1.bias"))
            K.pcnn_wgrad(hx, dhpre, g(p + "horiz_conv.conv.weight"), self._taps[f"h{d}"], (3, 3 * C), mode=mode)
            K.pcnn_wgrad(vpre, dhpre, g(p + "conv1x1_1.weight"), _ONE, (1, 2 * C), mode=mode)
            dhx = K.pcnn_conv(dhpre, w(p + "horiz_conv.conv.weight"), _neg(self._taps[f"h{d}"]), (3 * C, 3), C, res=dH, mode=mode)
            if dV is not None:
                dvpre = K.pcnn_gate_bwd(vpre, dV, K.PCNN_GATE_TS, cond=cv, dcond=dcv)
                K.pcnn_conv(dhpre, w(p + "conv1x1_1.weight"), _ONE, (2 * C, 1), 2 * C, out=dvpre, accumulate=True, mode=mode)
            else:                                       # the last layer's vertical output is not used
                dvpre = K.pcnn_conv(dhpre, w(p + "conv1x1_1.weight"), _ONE, (2 * C, 1), 2 * C, mode=mode)
            K.pcnn_colsum(dvpre, g(p + "vert_conv.conv.bias"))
            K.pcnn_wgrad(v, dvpre, g(p + "vert_conv.conv.weight"), self._taps[f"v{d}"], (9, 9 * C), mode=mode)
            dV = K.pcnn_conv(dvpre, w(p + "vert_conv.conv.weight"), _neg(self._taps[f"v{d}"]), (9 * C, 9), C, mode=mode)
            dH = dhx
        K.pcnn_wgrad(xin, dV, g("conv_vstack.conv.weight"), self._taps["v5"], (25, 25 * ch), mode=mode)
        K.pcnn_colsum(dV, g("conv_vstack.conv.bias"))
        K.pcnn_wgrad(xin, dH, g("conv_hstack.conv.weight"), self._taps["h5"], (5, 5 * ch), mode=mode)
        K.pcnn_colsum(dH, g("conv_hstack.conv.bias"))
        if dcond is not None:                           # d cond_proj[j][k] = sum_n dcond[n][j] onehot[n][k]
            gw = gflat[self._cond_off:self._cond_off + dcond.shape[1] * self.n_cond].view(dcond.shape[1], self.n_cond)
            if cond.dtype == torch.int64:
                K.pcnn_cond_wgrad(cond, dcond, gw)
            else:
                J = dcond.shape[1]
                K.pcnn_small_mm(J, self.n_cond, cond.shape[0], dcond, 1, J, cond, self.n_cond, 1, gw, self.n_cond)

    def _cond(self, y, device):
        """Labels stay int64 labels (the conditioning kernels gather by label: no one-hot in the step); a float y is a one-hot."""
        if not self.hparams.class_condition or y is None:
            return None
        if not y.is_floating_point():
            return y.to(device=device, dtype=torch.int64)
        return y.reshape(-1, self.n_cond).to(device=device, dtype=torch.float32).contiguous()

    # ------------------------------------------------------------------ the reference's surface
    def forward(self, x, y=None):
        """Logits [N, 256, C, H, W] for x in the datamodule's range; y: one-hot [N, n_classes] (or labels) when conditioned."""
        with torch.no_grad():
            xin = K.nchw_to_nhwc(x.float().contiguous())
            h, _, _ = self._forward_nhwc(xin, self._cond(y, x.device))
            C, mode = self.hidden_dim, self._mode()
            logits = K.pcnn_conv(h, self._w("conv_out.weight"), _ONE, (1, C), 256 * self.channels, bias=self._w("conv_out.bias"),
                                 elu_in=True, mode=mode)
            out = K.nhwc_to_nchw(logits)
        return out.reshape(out.shape[0], 256, out.shape[1] // 256, out.shape[2], out.shape[3])

    def calc_likelihood(self, x, label=None):
        """Mean bits per dim; differentiable into the flat gradient buffer (one autograd node)."""
        if self._anchor.device != x.device:
            object.__setattr__(self, "_anchor", torch.zeros(1, device=x.device, requires_grad=True))
        anchor = self._anchor if torch.is_grad_enabled() else self._anchor.detach()
        return _PixelCNNStep.apply(x, self._cond(label, x.device), anchor, self)

    @torch.no_grad()
    def sample(self, img_shape, cond=None, img=None):
        """Autoregressive sampling in raster order; pixels to fill are -1 in `img` (default: all)."""
        from ..runtime.pixelcnn_sampler import PixelSampler
        shape = tuple(int(s) for s in img_shape)
        c = self._cond(cond, self.device) if cond is not None else None
        key = (shape, None if c is None else c.dtype)
        s = self._samplers.get(key)
        if s is None:
            s = self._samplers[key] = PixelSampler(self, shape, cond_like=c)
        return s.run(img=img, cond=c)

    def configure_optimizers(self):
        from ..runtime.optim import FlatAdam
        opt = FlatAdam(self, lr=self.hparams.lr)
        scheduler = torch.optim.lr_scheduler.StepLR(opt, 1, gamma=0.99)
        return [opt], [scheduler]

    def training_step(self, batch, batch_idx):
        img, label = batch
        loss = self.calc_likelihood(img, label if self.hparams.class_condition else None)
        self.log("train_bpd", loss.detach())
        return loss

    def validation_step(self, batch, batch_idx):
        img, label = batch
        N, C, H, W = img.shape
        with torch.no_grad():
            loss = self.calc_likelihood(img, label if self.hparams.class_condition else None)
        self.log("val_bpd", loss)
        sample_img = None
        if batch_idx == 0:
            if self.hparams.class_condition:
                n = self.hparams.n_classes
                sample_label = torch.arange(n, device=img.device).repeat_interleave(8)
                sample_img = self.sample((n * 8, C, H, W), cond=sample_label)
            else:
                sample_img = self.sample(img.shape)
        return ValidationResult(real_image=img, fake_image=sample_img)
