"""MNIST-sized conv encoder / decoder with the reference's surface (src/networks/basic.py:147-204: `ConvEncoder`, `ConvDecoder`,
what configs/networks/conv_mnist.yaml instantiates) on the HIP kernels.  `norm_type` "batch" (the config default:
nn.BatchNorm2d with running statistics) and "layer" (nn.GroupNorm(1, C)) are built; same constructors, parameter / buffer names
(`network.N.weight`, `network.N.running_mean`, ...) and seeded initial weights.
Of the MLP networks of that file, `MLPEncoder` is built in the one shape the FactorVAE's latent discriminator uses
(src/models/factor_vae.py:48), on the fused kernels of csrc/latent_disc.hip; `MLPDecoder` is not on any shipped config's path.
"""
import torch

from ..models.ddpm import _Entry
from ..ops import functional as K
from .flatnet import FlatNet


class _NormMixin:
    # Opt-in (the GAN sets it on its two nets): BatchNorm and the activation behind it run as one segmented pass (K.bn_seg_fwd / K.bn_seg_bwd,
    # csrc/bn_seg.hip) -- 2 launches each way where the default path takes 4, and statistics per segment of the batch.  The default
    # path, which the VAE, cVAE and AAE run, launches what it always launched.
    fused_norm_act = False

    def use_fused_norm_act(self, on=True):
        if on and self.norm_type != "batch":
            raise NotImplementedError("fused_norm_act: the segmented kernels are BatchNorm's (norm_type='batch')")
        self.fused_norm_act = bool(on)
        return self

    def _check_segments(self, segments, bn_updates=1):
        if segments != 1 and not self.fused_norm_act:
            raise RuntimeError("segments > 1 needs the segmented BatchNorm path: use_fused_norm_act()")
        if self.fused_norm_act and bn_updates != 1:
            raise RuntimeError("bn_updates is the default path's; the segmented path counts one update per segment")

    def _norm_act_fwd(self, a, pre, act, slope, segments):
        """-> (h, st): the activated output and the tape's statistics entry, ("seg", mean[S, C], rstd[S, C])."""
        h, mean, rstd = self._bn_seg_fwd(a, pre, act, slope, segments)
        return h, ("seg", mean, rstd)

    def _norm_act_bwd(self, a, st, h, pre, act, slope, g, gv):
        """Through the activation and the norm in one pass, in place in g; gv = {}: no parameter gradients."""
        return K.bn_seg_bwd(a, st[1], st[2], self._sv[pre + "weight"], h, g, act=act, slope=slope, dgamma=gv.get(pre + "weight"),
                            dbeta=gv.get(pre + "bias"), accumulate=True, out=g)

    def _declare_norm(self, pre, c):
        if self.norm_type == "batch":
            self._batchnorm_params(pre, c)
        else:
            self._norm_params(pre, c)

    def _norm_fwd(self, a, pre, bn_updates=1):
        if self.norm_type == "batch":
            y, mean, rstd = self._bn_fwd(a, pre, updates=bn_updates)
            return y, (mean, rstd)
        y, st = K.sample_norm_fwd(a, self._sv[pre + "weight"], self._sv[pre + "bias"])
        return y, st

    def _norm_bwd(self, a, st, pre, g, gv):
        if self.norm_type == "batch":
            return K.batchnorm_bwd(a, st[0], st[1], self._sv[pre + "weight"], g, dgamma=gv[pre + "weight"], dbeta=gv[pre + "bias"], out=g)
        return K.sample_norm_bwd(a, st, self._sv[pre + "weight"], g, dgamma=gv[pre + "weight"], dbeta=gv[pre + "bias"], out=g)


def _is_seg(st):
    return isinstance(st, tuple) and len(st) == 3 and isinstance(st[0], str)


def _check_norm(norm_type):
    if norm_type not in ("batch", "layer"):
        raise NotImplementedError(f"norm_type={norm_type!r}: only 'batch' and 'layer' are built on the HIP path")


class ConvDecoder(FlatNet, _NormMixin):
    """z [N, C_in] -> [N, C_out, 28, 28]: ConvT(4,1,0) -> ConvT(3,2,1) -> ConvT(4,2,1) -> ConvT(4,2,1), norm + ReLU between, output act."""
    GEOM = ((4, 1, 0), (3, 2, 1), (4, 2, 1), (4, 2, 1))
    BF16_SHADOWS = False

    def __init__(self, input_channel, output_channel, ngf, norm_type="batch", output_act="tanh"):
        super().__init__()
        _check_norm(norm_type)
        if output_act not in ("tanh", "identity"):
            raise NotImplementedError("output_act: 'tanh' (normalised inputs) or 'identity'")
        self.input_channel, self.output_channel, self.norm_type, self.output_act = input_channel, output_channel, norm_type, output_act
        chans = [input_channel, ngf * 4, ngf * 2, ngf, output_channel]
        for i in range(4):
            self._conv_params(f"network.{3 * i}.", chans[i], chans[i + 1], self.GEOM[i][0], transposed=True)
            if i < 3:
                self._declare_norm(f"network.{3 * i + 1}.", chans[i + 1])
        self._finish()

    def forward(self, x):
        return super().forward(x.reshape(x.shape[0], -1, 1, 1))

    def forward_nhwc(self, z, record=False, segments=1):
        """segments = S (the segmented path only): the batch is S equal batches, each with its own BatchNorm statistics."""
        self._check_segments(segments)
        tape = [z] if record else None
        h = z
        for i in range(3):
            k, s, p = self.GEOM[i]
            a = self._conv(h, f"network.{3 * i}.", k, s, p, transposed=True)
            if self.fused_norm_act:
                h, st = self._norm_act_fwd(a, f"network.{3 * i + 1}.", "relu", 0.0, segments)
            else:
                n, st = self._norm_fwd(a, f"network.{3 * i + 1}.")
                h = K.relu_fwd(n, inplace=True)
            if record:
                tape.append((a, st, h))
        k, s, p = self.GEOM[3]
        out = self._conv(h, "network.9.", k, s, p, transposed=True)
        if self.output_act == "tanh":
            base = out._base if out._base is not None else out
            K.tanh_fwd(base, inplace=True)                                   # padded lanes stay 0
        if record:
            tape.append(out)
        return out, tape

    def backward_nhwc(self, tape, dy, need_dx=False, param_grads=True, own_dy=False):
        """param_grads=False: the input gradient only -- no weight, bias or affine gradient is computed and the gradient buffer is
        left alone (the AGE's encoder phase sends its reconstruction gradient through the frozen decoder).
        own_dy: dy is a view of a dense buffer with the output's pixel pitch whose padded lanes are 0, and the caller gives it up:
        the backward works in it instead of filling a copy (two launches less)."""
        gv = self._begin_backward() if param_grads else {}
        y = tape[-1]
        yb = y._base if y._base is not None else y
        db = dy._base if dy._base is not None else dy
        if own_dy and db.shape == yb.shape and db.is_contiguous() and db.data_ptr() == dy.data_ptr():
            d = db
        else:
            d = torch.zeros_like(yb)
            d[..., :self.output_channel] = dy
        if self.output_act == "tanh":
            K.tanh_bwd(yb, d, out=d)
        g = d[..., :self.output_channel]
        for i in range(3, 0, -1):
            a, st, h = tape[i]
            k, s, p = self.GEOM[i]
            g = self._conv_bwd(g, h, f"network.{3 * i}.", k, s, p, transposed=True, want_dw=param_grads)
            if _is_seg(st):
                g = self._norm_act_bwd(a, st, h, f"network.{3 * i - 2}.", "relu", 0.0, g, gv)
                continue
            if not param_grads:
                raise RuntimeError("param_grads=False is built on the segmented BatchNorm path: use_fused_norm_act()")
            K.relu_bwd(h, g, out=g)
            g = self._norm_bwd(a, st, f"network.{3 * i - 2}.", g, gv)
        k, s, p = self.GEOM[0]
        return self._conv_bwd(g, tape[0], "network.0.", k, s, p, transposed=True, want_dx=need_dx, want_dw=param_grads)


class ConvEncoder(FlatNet, _NormMixin):
    """[N, C_in, 28, 28] -> [N, C_out]: Conv(4,2,1)+LeakyReLU, Conv(4,2,1)+norm+LeakyReLU, Conv(3,2,1)+norm+LeakyReLU, Conv(4,1,0)."""
    CONVS = (("network.0.", 4, 2, 1, None), ("network.2.", 4, 2, 1, "network.3."), ("network.5.", 3, 2, 1, "network.6."))
    BF16_SHADOWS = False

    def __init__(self, input_channel, output_channel, ndf, norm_type="batch", return_features=False):
        super().__init__()
        _check_norm(norm_type)
        # return_features (the VAE-GAN's netD): forward also returns the activation after network.7 -- the reference's FeatureExtractor
        # hook, which holds no parameters, so the state-dict keys are the same either way
        self.return_features = bool(return_features)
        self.input_channel, self.output_channel, self.norm_type = input_channel, output_channel, norm_type
        chans = [input_channel, ndf, ndf * 2, ndf * 4]
        for i, (pre, k, s, p, norm) in enumerate(self.CONVS):
            self._conv_params(pre, chans[i], chans[i + 1], k)
            if norm:
                self._declare_norm(norm, chans[i + 1])
        self._conv_params("network.8.", ndf * 4, output_channel, 4)
        self._finish()

    def forward(self, x):
        if self.return_features:
            # (output [N, C_out], features): the 1-D ravel of the NCHW [N, 4 ndf, 4, 4] activation after network.7, the reference's
            # layout (basic.py:196-202).  Inference only: a training step drives forward_nhwc / backward_nhwc(dfeat=...) itself.
            if not (torch.is_tensor(x) and x.is_cuda):
                raise RuntimeError("libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
            with torch.no_grad():
                out, tape = self.forward_nhwc(K.nchw_to_nhwc(x.float()), record=True)
                return out.reshape(-1, self.output_channel), K.nhwc_to_nchw(self.features_nhwc(tape)).reshape(-1)
        return super().forward(x).reshape(-1, self.output_channel)

    @staticmethod
    def features_nhwc(tape):
        """The last hidden activation (after network.7) of a recorded forward: dense NHWC [rows, 4, 4, 4 ndf], the tape's own tensor."""
        return tape[3][2]

    def forward_nhwc(self, x, record=False, bn_updates=1, segments=1):
        """bn_updates = u: the forward counts as u successive training-mode forwards of this batch for the BatchNorm running
        statistics and counters (FlatNet._bn_fwd); the default is the single update.
        segments = S (the segmented path only, `use_fused_norm_act`): x holds S equal batches one after the other; every BatchNorm
        layer keeps statistics per batch and updates its running statistics S times, first batch first -- what S forwards do."""
        self._check_segments(segments, bn_updates)
        tape = [x] if record else None
        h = x
        for pre, k, s, p, norm in self.CONVS:
            a = self._conv(h, pre, k, s, p)
            if norm and self.fused_norm_act:
                h, st = self._norm_act_fwd(a, norm, "leaky_relu", 0.2, segments)
                if record:
                    tape.append((a, st, h))
                continue
            if norm:
                n, st = self._norm_fwd(a, norm, bn_updates)
            else:
                n, st = a, None
            h = K.leaky_relu_fwd(n, 0.2, inplace=True)
            if record:
                tape.append((a if st is not None else None, st, h))
        out = self._conv(h, "network.8.", 4, 1, 0)
        return out, tape

    def backward_nhwc(self, tape, dout, need_dx=False, param_grads=True, dfeat=None):
        """param_grads=False: the input gradient only -- no weight, bias or affine gradient is computed and the gradient buffer is
        left alone (a GAN's generator phase needs nothing else from its discriminator).
        dfeat: a gradient by the last hidden activation (`features_nhwc`), added to what network.8's input-gradient conv produced
        before the norm + activation backward: a tensor of that shape, or a callable that adds into the buffer it is handed (the
        VAE-GAN's K.feat_match with accumulate, which touches the recon segment's rows alone)."""
        gv = self._begin_backward() if param_grads else {}
        g = self._conv_bwd(dout, tape[3][2], "network.8.", 4, 1, 0, want_dw=param_grads)
        if callable(dfeat):
            dfeat(g)
        elif dfeat is not None:
            if dfeat.shape != g.shape:
                raise RuntimeError(f"dfeat: {tuple(g.shape)} expected, got {tuple(dfeat.shape)}")
            K.axpby(1.0, dfeat, g, True)
        for i in range(2, -1, -1):
            pre, k, s, p, norm = self.CONVS[i]
            a, st, h = tape[i + 1]
            if _is_seg(st):
                g = self._norm_act_bwd(a, st, h, norm, "leaky_relu", 0.2, g, gv)
            else:
                K.leaky_relu_bwd(h, g, 0.2, out=g)
                if st is not None:
                    if not param_grads:
                        raise RuntimeError("param_grads=False is built on the segmented BatchNorm path: use_fused_norm_act()")
                    g = self._norm_bwd(a, st, norm, g, gv)
            g = self._conv_bwd(g, tape[0] if i == 0 else tape[i][2], pre, k, s, p, want_dx=(i > 0 or need_dx), want_dw=param_grads)
        return g


class MLPEncoder(FlatNet):
    """The reference's MLPEncoder (src/networks/basic.py:64-112) in the shape the latent discriminators build:
    Linear(C*w*h, 256) -> GroupNorm(1, 256) -> LeakyReLU(0.2) -> Linear(256, 256) -> BatchNorm1d(256) -> LeakyReLU(0.2) -> Linear(256, 1).
    Same constructor, parameter / buffer names (`model.0.fc.weight`, `model.1.norm.running_mean`, `classifier.fc.weight`, ...),
    construction order and seeded default init.  Anything the kernels do not cover raises NotImplementedError.
    The network is fp32 in every compute mode (`compute_mode="bf16"` too): it is launch-bound, not arithmetic-bound.
    `disc_forward` / `disc_backward` are what a training step calls (no autograd graph); `forward(x)` gives the logits alone."""
    KEYS = ("model.0.fc.weight", "model.0.fc.bias", "model.0.norm.weight", "model.0.norm.bias", "model.1.fc.weight", "model.1.fc.bias",
            "model.1.norm.weight", "model.1.norm.bias", "classifier.fc.weight", "classifier.fc.bias")
    BF16_SHADOWS = False

    def __init__(self, input_channel, output_channel, hidden_dims, width, height, dropout=0, norm_type="batch", return_features=False,
                 output_act="identity"):
        super().__init__()
        hidden_dims = [int(h) for h in hidden_dims]
        in_features = int(input_channel) * int(width) * int(height)
        if (hidden_dims != [K.LATENT_DISC_H] * 2 or int(output_channel) != 1 or dropout != 0 or norm_type != "batch" or return_features
                or output_act != "identity" or not 1 <= in_features <= 64):
            raise NotImplementedError("MLPEncoder on the HIP path: hidden_dims=[256, 256], output_channel=1, at most 64 input features, "
                                      "dropout=0, norm_type='batch', return_features=False, output_act='identity'")
        self.input_channel, self.output_channel, self.in_features, self.return_features = input_channel, output_channel, in_features, False
        dims = [in_features] + hidden_dims
        for i in range(2):
            self._linear_params(f"model.{i}.fc.", dims[i], dims[i + 1])
            if i == 0:
                self._norm_params("model.0.norm.", dims[1])               # first layer: GroupNorm(1, C), no batch norm
            else:
                self._batchnorm_params("model.1.norm.", dims[2])
        self._linear_params("classifier.fc.", dims[2], 1)
        self._finish()

    def _linear_params(self, pre, i, o):
        """nn.Linear: weight logical [out, in] stored input-major, torch's seeded default init."""
        self._entries.append(_Entry(pre + "weight", (o, i), "linear", "kaiming", i, 0))
        self._entries.append(_Entry(pre + "bias", (o,), "plain", "ubias", i, 0))

    def _tensors(self, views):
        return [views[k] for k in self.KEYS]

    def disc_forward(self, target, z=None, h=None, eps=None, perm=None):
        """Logits, least-squares loss against `target` and the tape, from rows z, from (h, eps) or from (h, eps, perm)
        (K.latent_disc_fwd).  Training mode uses batch statistics and updates the running ones; evaluation mode uses those."""
        return K.latent_disc_fwd(self._tensors(self._sv), target, z=z, h=h, eps=eps, perm=perm, training=self.training,
                                 running_mean=self._buffer("model.1.norm.running_mean"), running_var=self._buffer("model.1.norm.running_var"),
                                 num_batches_tracked=self._buffer("model.1.norm.num_batches_tracked"))

    def disc_backward(self, rec, target, param_grads=True, accumulate=False, scale=1.0, dz=None, dz_scale=1.0, accumulate_dz=False):
        """Gradients of mean((logit - target)^2) from a `disc_forward` record.  param_grads: into the flat gradient buffer, stored
        (accumulate=False: every gradient element is written, nothing needs zeroing) or added; dz: see K.latent_disc_bwd."""
        grads = None
        if param_grads:
            self.flat_grads
            grads = self._tensors(self._gv)
        return K.latent_disc_bwd(self._tensors(self._sv), rec, target, grads=grads, param_scale=scale, accumulate_params=accumulate, dz=dz,
                                 dz_scale=dz_scale, accumulate_dz=accumulate_dz)

    def forward(self, x):
        n = x.shape[0]
        x = x.reshape(n, -1)
        if not x.is_cuda:
            raise RuntimeError("libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
        return self.disc_forward(0.0, z=x.float().contiguous())["logit"].view(n, 1)
