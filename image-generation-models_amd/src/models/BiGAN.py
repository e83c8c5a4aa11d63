"""`BiGAN` ("Adversarial Feature Learning", https://arxiv.org/abs/1605.09782) with the reference's surface (src/models/BiGAN.py:16-97)
on the HIP kernels -- `experiment=bigan/mnist`.

Same constructor and defaults, attribute names and construction order (`decoder`, `encoder`, `discriminator`: the seeded default
weights are the reference's), `state_dict` keys, `forward(z)`, two Adam optimizers (`opt_g` over encoder + decoder, `opt_d` over the
discriminator's three parts), manual optimization, the four logged keys and `validation_step`.  `sample(N)` is added.  The nets are
the 28x28 `ConvDecoder` / `ConvEncoder` with BatchNorm (configs/networks/conv_mnist.yaml) on their segmented BatchNorm + activation
path (csrc/bn_seg.hip); the discriminator is src/networks/pair_disc.py, whose two MLPs and both losses are the fused pair head
(csrc/pair_disc.hip), built for hidden_dim = 128 and latent_dim <= 128.

There are no alternating phases: every batch steps both optimizers.  `training_step(batch, batch_idx, z=None)` follows BiGAN.py:61-88
without recording an autograd graph:
  forward  encoder on imgs (real pair = (imgs, e)) and decoder on z (fake pair = (fake, z)), each once -> dis_x on [imgs | fake] as ONE
           `segments=2` pass, real first -> the pair head on the 2 N rows: logits, g_loss = adv(real, False) + adv(fake, True),
           d_loss = adv(real, True) + adv(fake, False) (neither halved) and both derivatives by the logits;
  opt_g    head backward for the input gradients alone -> dis_x backward without parameter gradients -> its fake half into the
           decoder's backward, the head's code gradient into the encoder's -> Adam over both;
  opt_d    head and dis_x backward for the parameter gradients from the SAME tapes (the activations from before opt_g stepped, as
           the reference's retained graph holds them; a backward pass writes nothing into a tape) -> Adam.
In the generator side's dis_x pass the real half's image gradient is computed and not read (segments are independent); slicing the
tape to the fake half alone is left undone.  `loss_mode` "vanilla", "lsgan" and "hinge" are the reference's adversarial_loss; "hinge"
is its formula, whose real branch is max(1 - pred, 1).  z is a device draw, every logged scalar stays a device tensor, nothing in the
step synchronises with the host.  A CPU tensor raises.  Under data parallelism the gradients of each optimizer's nets are all-reduced
before it steps.
"""
import torch

from ..networks.pair_disc import Discriminator
from ..ops import functional as K
from .base import BaseModel, ValidationResult
from .gan import SEGMENTED_NORM, _base

LOGS = ("train_loss/g_loss", "train_loss/d_loss", "train_log/real_logit", "train_log/fake_logit")

__all__ = ["BiGAN", "Discriminator", "LOGS"]


class BiGAN(BaseModel):
    def __init__(self, datamodule, encoder=None, decoder=None, latent_dim=100, hidden_dim=512, loss_mode="vanilla", lrG: float = 0.0002,
                 lrD: float = 0.0002, b1: float = 0.5, b2: float = 0.999):
        super().__init__(datamodule)
        self.save_hyperparameters()
        if loss_mode not in K.ADV_LOSSES:
            raise NotImplementedError(f"loss_mode={loss_mode!r}: 'vanilla', 'lsgan' and 'hinge' are built")
        if int(hidden_dim) != K.PAIR_DISC_H or not 1 <= int(latent_dim) <= 128:
            raise NotImplementedError(f"BiGAN on the HIP path: hidden_dim={K.PAIR_DISC_H} (the experiments' value; the constructor default "
                                      f"512 is not built) and 1 <= latent_dim <= 128, got hidden_dim={hidden_dim}, latent_dim={latent_dim}")
        try:                                                    # pragma: no cover - hydra is not in this image
            from hydra.utils import instantiate
        except Exception:                                       # noqa: BLE001
            from ..runtime.config import instantiate
        self.decoder = instantiate(decoder, input_channel=latent_dim, output_channel=self.channels)
        self.encoder = instantiate(encoder, input_channel=self.channels, output_channel=latent_dim)
        from ..networks.basic import ConvDecoder, ConvEncoder
        if (not isinstance(self.decoder, ConvDecoder) or not isinstance(self.encoder, ConvEncoder) or self.decoder.norm_type != "batch"
                or self.encoder.norm_type != "batch" or (self.height, self.width) != (28, 28)):
            raise NotImplementedError("BiGAN on the HIP path: src.networks.basic.ConvDecoder / ConvEncoder with norm_type='batch' on 28x28 "
                                      "images (configs/networks/conv_mnist.yaml); the MLP and conv32 / conv64 nets are not built")
        self.discriminator = Discriminator(encoder, self.channels, latent_dim, hidden_dim)
        for n in (self.decoder, self.encoder):
            n.use_fused_norm_act(SEGMENTED_NORM)
            n.reproducible = True                               # no atomics anywhere in the step: two runs give the same bits
        self.automatic_optimization = False

    # ------------------------------------------------------------------ surface
    def forward(self, z):
        output = self.decoder(z)
        return output.reshape(z.shape[0], self.channels, self.height, self.width)

    def flat_nets(self):
        return [self.decoder, self.encoder] + self.discriminator.flat_nets()

    def configure_optimizers(self):
        from ..runtime.optim import FlatAdam
        hp = self.hparams
        # host_complements: 1 - beta rounded once from double, as torch's Adam takes them (csrc/elementwise.hip, adam_c_kernel)
        opt_g = FlatAdam([self.encoder, self.decoder], lr=hp.lrG, betas=(hp.b1, hp.b2), host_complements=True)
        opt_d = FlatAdam(self.discriminator.flat_nets(), lr=hp.lrD, betas=(hp.b1, hp.b2), host_complements=True)
        return [opt_g, opt_d]

    @staticmethod
    def _on_gpu(t, what):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError(f"{what}: libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
        return t.float().contiguous()

    def _draw(self, z, N):
        L = int(self.hparams.latent_dim)
        if z is None:
            return torch.randn(N, L, device=self.device)
        z = self._on_gpu(z, "z")
        if z.shape != (N, L):
            raise RuntimeError(f"z: [{N}, {L}] expected, got {tuple(z.shape)}")
        return z

    def sample(self, N: int):
        with torch.no_grad():
            return self.forward(torch.randn(N, int(self.hparams.latent_dim), device=self.device))

    def _sync(self, nets):
        from ..runtime.ddp import allreduce_flat_grads
        allreduce_flat_grads(list(nets))

    # ------------------------------------------------------------------ training
    def training_step(self, batch, batch_idx, z=None):
        imgs, _ = batch  # (N, C, H, W)
        imgs = self._on_gpu(imgs, "images")
        N, L, C = imgs.shape[0], int(self.hparams.latent_dim), self.channels
        z = self._draw(z, N)
        E, G, D = self.encoder, self.decoder, self.discriminator
        opt_g, opt_d = self.optimizers()

        # ---- forward (BiGAN.py:67-75)
        x_real = K.nchw_to_nhwc(imgs)
        e, tape_e = E.forward_nhwc(x_real, record=True)                            # [N, 1, 1, L]: the real pair's code
        zin = z.view(N, 1, 1, L) if L % 4 == 0 else K.nchw_to_nhwc(z.view(N, L, 1, 1))
        fake, tape_g = G.forward_nhwc(zin, record=True)
        x = torch.cat([_base(x_real), _base(fake)])[..., :C]                       # real first: the reference's order of D calls
        rec = D.pair_forward(x, e, z, self.hparams.loss_mode)

        # ---- opt_g (BiGAN.py:77-79)
        dx_fake, de = D.pair_backward_inputs(rec)
        G.backward_nhwc(tape_g, dx_fake[..., :C])
        E.backward_nhwc(tape_e, de, need_dx=False)
        self._sync([E, G])
        opt_g.step()

        # ---- opt_d (BiGAN.py:81-83): the same forward, which ran before opt_g stepped
        D.pair_backward_params(rec)
        self._sync(D.flat_nets())
        opt_d.step()

        self.log("train_loss/g_loss", rec["g_loss"])
        self.log("train_loss/d_loss", rec["d_loss"])
        self.log("train_log/real_logit", rec["mean_real"])
        self.log("train_log/fake_logit", rec["mean_fake"])

    def validation_step(self, batch, batch_idx):
        img, _ = batch
        with torch.no_grad():
            fake_img = self.sample(img.shape[0])
            encode_z = self.encoder(img)
            recon_img = self.forward(encode_z)
        return ValidationResult(real_image=img, fake_image=fake_img, recon_image=recon_img, encode_latent=encode_z)
