"""BiGAN's `Discriminator` (reference src/models/BiGAN.py:100-126) on the HIP kernels: D(x, z) scores an (image, code) pair.
    dis_z    MLPEncoder(latent_dim, [H, H], H, output_act="leaky_relu"): Linear -> GroupNorm(1, H) -> LeakyReLU(0.2) -> Linear ->
             BatchNorm1d -> LeakyReLU -> Linear -> LeakyReLU                                                    (`PairCodeMLP`)
    dis_x    the encoder config with H outputs: the 28x28 `ConvEncoder` with BatchNorm, on its segmented path
    dis_pair MLPEncoder(2H, [H], 1) on cat(z_feature, x_feature): Linear -> GroupNorm(1, H) -> LeakyReLU -> Linear (`PairHeadMLP`)
Same constructor, submodule names and construction order, `state_dict` keys, buffer dtypes and seeded default init as the reference.
dis_z and dis_pair are `FlatNet`s that hold parameters alone: everything they compute is the fused pair head (csrc/pair_disc.hip,
K.pair_disc_fwd / K.pair_disc_bwd), which takes the real and the fake pairs as two segments of one pass -- the reference's two calls,
real first: every BatchNorm layer keeps statistics per segment and updates its running statistics twice.  Only H = 128 and
1 <= latent_dim <= 128 are built; `src.networks.basic.MLPEncoder` stays the FactorVAE's network and keeps refusing these shapes.
"""
import torch
from torch import nn

from ..ops import functional as K
from .basic import ConvEncoder, MLPEncoder
from .flatnet import FlatNet


def _refuse(cls, what):
    raise NotImplementedError(f"{cls} on the HIP path: {what}, width=height=1, dropout=0, norm_type='batch', return_features=False")


class PairCodeMLP(FlatNet):
    """dis_z.  The reference's MLPEncoder constructor; only (L, [128, 128], 128, output_act="leaky_relu") with 1 <= L <= 128 is built."""
    KEYS = MLPEncoder.KEYS
    BF16_SHADOWS = False

    def __init__(self, input_channel, output_channel, hidden_dims, width, height, dropout=0, norm_type="batch", return_features=False,
                 output_act="identity"):
        super().__init__()
        H = K.PAIR_DISC_H
        in_features = int(input_channel) * int(width) * int(height)
        if ([int(h) for h in hidden_dims] != [H, H] or int(output_channel) != H or dropout != 0 or norm_type != "batch" or return_features
                or output_act != "leaky_relu" or (int(width), int(height)) != (1, 1) or not 1 <= in_features <= 128):
            _refuse("PairCodeMLP", f"hidden_dims=[{H}, {H}], output_channel={H}, output_act='leaky_relu', 1 to 128 input features")
        self.input_channel, self.output_channel, self.in_features, self.return_features = input_channel, output_channel, in_features, False
        self._linear_params("model.0.fc.", in_features, H)
        self._norm_params("model.0.norm.", H)                             # first layer: GroupNorm(1, C), no batch norm
        self._linear_params("model.1.fc.", H, H)
        self._batchnorm_params("model.1.norm.", H)
        self._linear_params("classifier.fc.", H, H)
        self._finish()

    _linear_params = MLPEncoder._linear_params

    def forward(self, x):
        raise NotImplementedError("PairCodeMLP holds dis_z's parameters; the pair head (Discriminator.pair_forward / forward) computes with them")


class PairHeadMLP(FlatNet):
    """dis_pair.  The reference's MLPEncoder constructor; only (2 * 128, [128], 1) with the identity output is built."""
    KEYS = ("model.0.fc.weight", "model.0.fc.bias", "model.0.norm.weight", "model.0.norm.bias", "classifier.fc.weight", "classifier.fc.bias")
    BF16_SHADOWS = False

    def __init__(self, input_channel, output_channel, hidden_dims, width, height, dropout=0, norm_type="batch", return_features=False,
                 output_act="identity"):
        super().__init__()
        H = K.PAIR_DISC_H
        if ([int(h) for h in hidden_dims] != [H] or int(output_channel) != 1 or dropout != 0 or norm_type != "batch" or return_features
                or output_act != "identity" or (int(width), int(height)) != (1, 1) or int(input_channel) != 2 * H):
            _refuse("PairHeadMLP", f"input_channel={2 * H}, hidden_dims=[{H}], output_channel=1, output_act='identity'")
        self.input_channel, self.output_channel, self.in_features, self.return_features = input_channel, output_channel, 2 * H, False
        self._linear_params("model.0.fc.", 2 * H, H)
        self._norm_params("model.0.norm.", H)
        self._linear_params("classifier.fc.", H, 1)
        self._finish()

    _linear_params = MLPEncoder._linear_params
    forward = PairCodeMLP.forward


class Discriminator(nn.Module):
    def __init__(self, encoder, input_channel, latent_dim, hidden_dim) -> None:
        super().__init__()
        try:                                                    # pragma: no cover - hydra is not in this image
            from hydra.utils import instantiate
        except Exception:                                       # noqa: BLE001
            from ..runtime.config import instantiate
        if int(hidden_dim) != K.PAIR_DISC_H or not 1 <= int(latent_dim) <= 128:
            raise NotImplementedError(f"BiGAN's discriminator on the HIP path: hidden_dim={K.PAIR_DISC_H} and 1 <= latent_dim <= 128 "
                                      f"(csrc/pair_disc.hip), got hidden_dim={hidden_dim}, latent_dim={latent_dim}")
        self.dis_z = PairCodeMLP(input_channel=latent_dim, output_channel=hidden_dim, width=1, height=1, hidden_dims=[hidden_dim, hidden_dim],
                                 output_act="leaky_relu")
        self.dis_x = instantiate(encoder, input_channel=input_channel, output_channel=hidden_dim)
        self.dis_pair = PairHeadMLP(input_channel=2 * hidden_dim, output_channel=1, width=1, height=1, hidden_dims=[hidden_dim])
        if not isinstance(self.dis_x, ConvEncoder) or self.dis_x.norm_type != "batch":
            raise NotImplementedError("BiGAN's discriminator on the HIP path: dis_x is src.networks.basic.ConvEncoder with norm_type='batch'")
        self.dis_x.use_fused_norm_act()
        for n in self.flat_nets():
            n.reproducible = True                               # no atomics anywhere: two runs give the same bits
        self.latent_dim, self.hidden_dim = int(latent_dim), int(hidden_dim)

    def flat_nets(self):
        return [self.dis_z, self.dis_x, self.dis_pair]

    def _params(self, views_z, views_p):
        return [views_z[k] for k in PairCodeMLP.KEYS] + [views_p[k] for k in PairHeadMLP.KEYS]

    def _head(self, xf, e, z, loss_mode, update):
        bn = "model.1.norm."
        buf = self.dis_z._buffer
        stats = update or not self.training                     # training mode without an update: batch statistics, buffers untouched
        return K.pair_disc_fwd(self._params(self.dis_z._sv, self.dis_pair._sv), e, z, xf, loss_mode=loss_mode, training=self.training,
                               running_mean=buf(bn + "running_mean") if stats else None, running_var=buf(bn + "running_var") if stats else None,
                               num_batches_tracked=buf(bn + "num_batches_tracked") if update else None)

    @staticmethod
    def _rows(t):
        """[N, 1, 1, C] (a view of a padded buffer will do) as pitched rows [N, C]."""
        return t.squeeze(2).squeeze(1) if t.dim() == 4 else t

    def pair_forward(self, x, e, z, loss_mode="vanilla", record=True):
        """x: NHWC images [2N, h, w, C], the real half first; e: the encoder's output for the real half, [N, 1, 1, L] or [N, L] (read in
        place with its pitch); z [N, L]: the fake half's codes.  One `segments=2` pass of dis_x, then the pair head.  Returns
        K.pair_disc_fwd's record (logit, dlogit_g, dlogit_d, the six scalars) with dis_x's tape in it."""
        xf, tape_x = self.dis_x.forward_nhwc(x, record=record, segments=2)
        rec = self._head(self._rows(xf), self._rows(e), z, loss_mode, update=self.training)
        rec["tape_x"] = tape_x
        return rec

    def pair_backward_inputs(self, rec):
        """The generator side, from dlogit_g: (dX_fake, de) -- the gradient by the fake half's images (NHWC, as dis_x's input-gradient
        pass hands it over) and by the real half's codes ([N, 1, 1, L], a view of a zero-padded buffer).  No parameter gradient is
        computed and no gradient buffer is touched; the tapes stay intact for `pair_backward_params`."""
        N, L, H = rec["N"], rec["L"], self.hidden_dim
        dev = rec["tape"].device
        dxf = torch.empty((2 * N, 1, 1, H), device=dev, dtype=torch.float32)
        deb = torch.zeros((N, 1, 1, (L + 3) // 4 * 4), device=dev, dtype=torch.float32)
        K.pair_disc_bwd(self._params(self.dis_z._sv, self.dis_pair._sv), rec, dxf=dxf.view(2 * N, H), de=self._rows(deb)[:, :L])
        dx = self.dis_x.backward_nhwc(rec["tape_x"], dxf, need_dx=True, param_grads=False)
        return dx[N:], deb[..., :L]

    def pair_backward_params(self, rec):
        """The discriminator side, from dlogit_d on the same record: the gradients of all three parts into their flat gradient buffers
        (stored: nothing needs zeroing)."""
        N, H = rec["N"], self.hidden_dim
        self.dis_z.flat_grads, self.dis_pair.flat_grads
        dxf_d = torch.empty((2 * N, 1, 1, H), device=rec["tape"].device, dtype=torch.float32)
        K.pair_disc_bwd(self._params(self.dis_z._sv, self.dis_pair._sv), rec, grads=self._params(self.dis_z._gv, self.dis_pair._gv),
                        dxf_d=dxf_d.view(2 * N, H))
        self.dis_x.backward_nhwc(rec["tape_x"], dxf_d, need_dx=False)

    def forward(self, x, z):
        """Logits [N, 1] of the pairs (x [N, C, h, w], z [N, L]) without an autograd graph, for inference: evaluation mode, where every
        BatchNorm layer uses its running statistics and no buffer is touched.  Training goes through `pair_forward`."""
        if not (torch.is_tensor(x) and x.is_cuda and torch.is_tensor(z) and z.is_cuda):
            raise RuntimeError("libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
        if self.training:
            raise NotImplementedError("Discriminator.forward is the inference path: call .eval() first (a training step drives pair_forward)")
        n = x.shape[0]
        with torch.no_grad():
            xn = K.nchw_to_nhwc(x.float())
            xb = xn._base if xn._base is not None else xn
            x2 = torch.cat([xb, xb])[..., :x.shape[1]]            # the head works on two segments: the same rows twice
            xf, _ = self.dis_x.forward_nhwc(x2, record=False, segments=2)
            zz = z.reshape(n, -1).float().contiguous()
            return self._head(self._rows(xf), zz, zz, "vanilla", update=False)["logit"][:n].reshape(n, 1)
