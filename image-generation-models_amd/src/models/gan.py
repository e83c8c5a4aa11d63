"""`GAN` (https://arxiv.org/abs/1406.2661) with the reference's surface (src/models/gan.py:7-81) on the HIP kernels --
`experiment=vanilla_gan/mnist_conv`, `lsgan/conv_mnist`, `ggan/mnist_conv`, which differ in `loss_mode` alone.

Same constructor and defaults, attribute names (`netG`, `netD`), construction order (the seeded default weights are the reference's),
`state_dict` keys, `forward(z)`, two Adam optimizers (one `FlatAdam` per net), manual optimization, the four logged keys and
`validation_step`.  `sample(N)` is added (the reference inherits it from its BaseModel).  The nets are the 28x28 `ConvDecoder` /
`ConvEncoder` with BatchNorm (configs/networks/conv_mnist.yaml) on their segmented BatchNorm + activation path (csrc/bn_seg.hip);
the reference's MLP and conv32 / conv64 experiments are not built.

`training_step(batch, batch_idx, z=None)` follows the reference's alternation (gan.py:45-75) without recording an autograd graph:
  even batch_idx  generator      G forward -> D forward on the fake in training mode (D's running statistics update, as in the
                                 reference) -> loss against "real" -> D backward for the input gradient alone -> G backward -> G's Adam;
  odd batch_idx   discriminator  G forward in training mode without a tape (G's running statistics update) -> D forward on
                                 [imgs | fake] as ONE pass of N + N rows with `segments=2`, real first: every BatchNorm layer keeps
                                 statistics per half and updates its running statistics twice, real half first, exactly what the
                                 reference's two D calls do -> d_loss = (real + fake) / 2 -> D backward with parameter gradients and
                                 no input gradient -> D's Adam.
`loss_mode` "vanilla", "lsgan" and "hinge" are the reference's adversarial_loss (src/utils/losses.py:4-24) in one launch
(K.adv_loss).  "hinge" is the reference's formula, whose real branch is max(1 - pred, 1) and not the hinge loss max(1 - pred, 0):
parity with the reference is the contract.  z is a device draw, every logged scalar stays a device tensor, nothing in the step
synchronises with the host.  A CPU tensor raises.
"""
import torch

from ..ops import functional as K
from .base import BaseModel, ValidationResult

# Whether the nets run BatchNorm + activation on the segmented kernels (csrc/bn_seg.hip).  tools/bench_gan.py measures them against
# the per-segment K.batchnorm_* + activation kernels on the discriminator phase's tensors; they stay the model's path while they
# are not slower (README, docs/kernels.md 4j).
SEGMENTED_NORM = True


class GAN(BaseModel):
    def __init__(self, datamodule, netG=None, netD=None, latent_dim: int = 100, loss_mode: str = "vanilla", lrG: float = 2e-4,
                 lrD: float = 2e-4, b1: float = 0.5, b2: float = 0.999):
        super().__init__(datamodule)
        self.save_hyperparameters()
        if loss_mode not in K.ADV_LOSSES:
            raise NotImplementedError(f"loss_mode={loss_mode!r}: 'vanilla', 'lsgan' and 'hinge' are built")
        try:                                                    # pragma: no cover - hydra is not in this image
            from hydra.utils import instantiate
        except Exception:                                       # noqa: BLE001
            from ..runtime.config import instantiate
        self.netG = instantiate(netG, input_channel=latent_dim, output_channel=self.channels)
        self.netD = instantiate(netD, input_channel=self.channels, output_channel=1)
        from ..networks.basic import ConvDecoder, ConvEncoder
        if (not isinstance(self.netG, ConvDecoder) or not isinstance(self.netD, ConvEncoder) or self.netG.norm_type != "batch"
                or self.netD.norm_type != "batch" or (self.height, self.width) != (28, 28)):
            raise NotImplementedError("GAN on the HIP path: src.networks.basic.ConvDecoder / ConvEncoder with norm_type='batch' on 28x28 "
                                      "images (configs/networks/conv_mnist.yaml); the MLP and conv32 / conv64 experiments are not built")
        self.netG.use_fused_norm_act(SEGMENTED_NORM)
        self.netD.use_fused_norm_act(SEGMENTED_NORM)
        self.netG.reproducible = self.netD.reproducible = True  # no atomics anywhere in the step: two runs give the same bits
        self.automatic_optimization = False

    def forward(self, z):
        output = self.netG(z)
        return output.reshape(z.shape[0], self.channels, self.height, self.width)

    def flat_nets(self):
        return [self.netG, self.netD]

    def configure_optimizers(self):
        from ..runtime.optim import FlatAdam
        hp = self.hparams
        opt_g = FlatAdam(self.netG, lr=hp.lrG, betas=(hp.b1, hp.b2))
        opt_d = FlatAdam(self.netD, lr=hp.lrD, betas=(hp.b1, hp.b2))
        return [opt_g, opt_d]

    def sample(self, N: int):
        with torch.no_grad():
            return self.forward(torch.randn(N, int(self.hparams.latent_dim), device=self.device))

    def _sync(self, net):
        from ..runtime.ddp import allreduce_flat_grads
        allreduce_flat_grads([net])

    @staticmethod
    def _on_gpu(t, what):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError(f"{what}: libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
        return t.float().contiguous()

    def _z_nhwc(self, z, N):
        """z [N, L] as the generator's NHWC input [N, 1, 1, L]: a view when L % 4 == 0 (the convolutions' pixel pitch), else repacked."""
        L = int(self.hparams.latent_dim)
        if z is None:
            z = torch.randn(N, L, device=self.device)
        z = self._on_gpu(z, "z")
        if z.shape != (N, L):
            raise RuntimeError(f"z: [{N}, {L}] expected, got {tuple(z.shape)}")
        return z.view(N, 1, 1, L) if L % 4 == 0 else K.nchw_to_nhwc(z.view(N, L, 1, 1))

    def _d_forward(self, x, segments, record=True):
        """D on NHWC images -> (logit [rows, 1, 1, 1], tape).  Without the segmented kernels the segments go through one by one, in
        order, and their tapes are kept side by side."""
        D = self.netD
        if D.fused_norm_act or segments == 1:
            return D.forward_nhwc(x, record=record, segments=segments)
        n = x.shape[0] // segments
        parts = [D.forward_nhwc(x[s * n:(s + 1) * n], record=record) for s in range(segments)]
        return torch.cat([_base(o) for o, _ in parts])[..., :1], [t for _, t in parts]

    def training_step(self, batch, batch_idx, z=None):
        imgs, _ = batch  # (N, C, H, W)
        imgs = self._on_gpu(imgs, "images")
        N = imgs.shape[0]
        G, D, mode = self.netG, self.netD, self.hparams.loss_mode
        zin = self._z_nhwc(z, N)
        opt_g, opt_d = self.optimizers()

        if batch_idx % 2 == 0:
            # ---- generator phase (gan.py:45-56)
            fake, tape_g = G.forward_nhwc(zin, record=True)
            pred_fake, tape_d = D.forward_nhwc(fake, record=True)
            loss, _, dlogit = K.adv_loss(pred_fake, [True], mode)
            if D.fused_norm_act:
                dfake = D.backward_nhwc(tape_d, dlogit, need_dx=True, param_grads=False)
            else:
                dfake = D.backward_nhwc(tape_d, dlogit, need_dx=True)             # D's gradient buffer is scratch here: its Adam does not step
            G.backward_nhwc(tape_g, dfake[..., :self.channels])
            self._sync(G)
            opt_g.step()
            self.log("train_loss/g_loss", loss[0])
            return

        # ---- discriminator phase (gan.py:57-75)
        fake, _ = G.forward_nhwc(zin, record=False)                                # detached in the reference (:62)
        x = torch.cat([_base(K.nchw_to_nhwc(imgs)), _base(fake)])[..., :self.channels]   # real first: the reference's order of D calls
        pred, tape = self._d_forward(x, 2)
        loss, mean_logit, dlogit = K.adv_loss(pred, [True, False], mode, scale=0.5)
        if D.fused_norm_act:
            D.backward_nhwc(tape, dlogit, need_dx=False)
        else:
            D.backward_nhwc(tape[0], dlogit[:N], need_dx=False)
            D.accumulate_grads = True
            try:
                D.backward_nhwc(tape[1], dlogit[N:], need_dx=False)
            finally:
                D.accumulate_grads = False
        self._sync(D)
        opt_d.step()
        self.log("train_loss/d_loss", (loss[0] + loss[1]) / 2)
        self.log("train_log/pred_real", mean_logit[0])
        self.log("train_log/pred_fake", mean_logit[1])

    def validation_step(self, batch, batch_idx):
        img, _ = batch
        with torch.no_grad():
            z = torch.randn(img.shape[0], int(self.hparams.latent_dim), device=img.device)
            fake_imgs = self.forward(z)
        return ValidationResult(real_image=img, fake_image=fake_imgs)


def _base(t):
    """The padded [N, H, W, 4k] buffer behind an NHWC view."""
    return t._base if t._base is not None else t
