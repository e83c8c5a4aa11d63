"""`FactorVAE` with the reference's surface (src/models/factor_vae.py:24-129) on the HIP kernels -- `experiment=factor_vae/celeba`.

A VAE whose encoder is also trained against a discriminator on the LATENT code: `netD` tells latents z ~ q(z|x) from latents whose
columns were shuffled across the batch (the product of the marginals), least-squares adversarial loss.  Same constructor and
defaults, attribute names and construction order (`decoder`, `encoder`, `netD`: the seeded default weights are the reference's),
manual optimization with two Adam optimizers, logged keys, `forward(z)` = decode, `encode`, `vae` -> (z, recon, mu, log_sigma) --
the reference's order here, which is not `VAE.vae`'s.  `sample(N)` is added (the reference inherits it from its BaseModel).

`training_step` follows the reference line by line without recording an autograd graph:
  encoder phase        encoder -> [mu | log_sigma] -> z1 (KL term) -> decoder -> Gaussian reconstruction term on the first half of the
                       batch; netD(z1) against target 1 = g_adv_loss; the gradient of recon + reg + adv_weight * g_adv goes through
                       the decoder and -- adv_weight * d g_adv / d z added onto the decoder's input gradient by netD's own backward --
                       through the encoder; Adam over encoder + decoder;
  discriminator phase  the UPDATED encoder on the second half (no tape); netD reads (h2, eps2, perm) directly -- the permuted
                       latents are never written to memory -- against target 1, and the fake logits of the encoder phase against
                       target 0 (netD has not changed since: nothing is recomputed); both parameter gradients into one buffer; Adam.
netD is the fused kernel pair of csrc/latent_disc.hip (fp32 in `compute_mode="bf16"` too).  Every random draw is a device draw
(eps by `torch.randn`, the column permutations as an argsort of uniform noise), every logged scalar stays a device tensor, nothing
in the step synchronises with the host.  A CPU tensor raises.
"""
import math

import torch

from ..networks.basic import MLPEncoder
from ..ops import functional as K
from .base import BaseModel, ValidationResult
from .vae import _GaussianDistribution


def _decoder_input(z):
    """z [N, L] -> the decoder's NHWC input [N, 1, 1, L]: a view of a buffer whose pixel pitch is a multiple of 4 with zero padding
    lanes, which the convolution kernels ask for (latent_dim = 10 is not one); one launch."""
    n, L = z.shape
    return K.nchw_to_nhwc(z.reshape(n, L, 1, 1))


def permute_dims_index(n, latent_dim, device):
    """perm [L, N] int64: one uniform random permutation of the batch per latent column (the reference's permute_dims draws
    torch.randperm(B) per column, factor_vae.py:13-22), drawn on the device."""
    return torch.argsort(torch.rand(latent_dim, n, device=device), dim=1)


class FactorVAE(BaseModel):
    def __init__(self, datamodule, encoder=None, decoder=None, loss_mode: str = "lsgan", adv_weight: float = 1, latent_dim=10,
                 lr: float = 0.0002, lrD: float = 0.0001, ae_b1: float = 0.9, ae_b2: float = 0.999, adv_b1: float = 0.5,
                 adv_b2: float = 0.999, decoder_dist="gaussian"):
        super().__init__(datamodule)
        self.save_hyperparameters()
        try:                                                    # pragma: no cover - hydra is not in this image
            from hydra.utils import instantiate
        except Exception:                                       # noqa: BLE001
            from ..runtime.config import instantiate
        self.decoder = instantiate(decoder, input_channel=latent_dim, output_channel=self.channels, output_act=self.output_act)
        if decoder_dist != "gaussian":
            raise NotImplementedError(f"decoder_dist={decoder_dist!r}: the reference's get_decode_dist knows 'gaussian' and 'bernoulli'; "
                                      "only the Gaussian decoder is built here (the dsprites experiment is not ported)")
        self.decoder_dist = _GaussianDistribution()
        self.encoder = instantiate(encoder, input_channel=self.channels, output_channel=latent_dim * 2)
        self.netD = MLPEncoder(input_channel=latent_dim, hidden_dims=[256, 256], output_channel=1, width=1, height=1)
        if loss_mode != "lsgan":
            raise NotImplementedError(f"loss_mode={loss_mode!r}: the fused discriminator carries the least-squares loss of the shipped configs")
        self.automatic_optimization = False  # disable automatic optimization

    def forward(self, z):
        """Generate images given latent code."""
        output = self.decoder_dist.sample(self.decoder(z))
        return output.reshape(output.shape[0], self.channels, self.height, self.width)

    def sample(self, N: int):
        z = torch.randn(N, self.hparams.latent_dim, device=self.device)
        with torch.no_grad():
            return self.forward(z)

    def flat_nets(self):
        return [self.decoder, self.encoder, self.netD]

    def configure_optimizers(self):
        from ..runtime.optim import FlatAdam
        hp = self.hparams
        ae_optim = FlatAdam([self.encoder, self.decoder], lr=hp.lr, betas=(hp.ae_b1, hp.ae_b2))
        discriminator_optim = FlatAdam(self.netD, lr=hp.lrD, betas=(hp.adv_b1, hp.adv_b2))
        return ae_optim, discriminator_optim

    def _sync(self, nets):
        from ..runtime.ddp import allreduce_flat_grads
        allreduce_flat_grads(list(nets))

    @staticmethod
    def _on_gpu(imgs):
        if not imgs.is_cuda:
            raise RuntimeError("libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
        return imgs.float().contiguous()

    def _encode_rows(self, imgs, record=False):
        n = imgs.shape[0]
        h, tape = self.encoder.forward_nhwc(K.nchw_to_nhwc(imgs), record=record)          # [N,1,1,2L]
        return h.reshape(n, -1), tape

    def encode(self, imgs, eps=None):
        """(z, mu, log_sigma) like the reference (factor_vae.py:74-78); inference only -- training goes through training_step."""
        with torch.no_grad():
            imgs = self._on_gpu(imgs)
            hrows, _ = self._encode_rows(imgs)
            if eps is None:
                eps = torch.randn(imgs.shape[0], self.hparams.latent_dim, device=imgs.device)
            z, _ = K.vae_latent_fwd(hrows, eps)
            mu, log_sigma = torch.chunk(hrows, 2, dim=1)
            return z, mu, log_sigma

    def vae(self, imgs):
        """(z, recon_imgs, mu, log_sigma): the reference's order (factor_vae.py:80-83)."""
        with torch.no_grad():
            z, mu, log_sigma = self.encode(imgs)
            out, _ = self.decoder.forward_nhwc(_decoder_input(z), record=False)
            return z, K.nhwc_to_nchw(out), mu, log_sigma

    def training_step(self, batch, batch_idx, eps1=None, eps2=None, perm=None):
        ae_optim, discriminator_optim = self.optimizers()
        imgs, _ = batch
        imgs = self._on_gpu(imgs)
        imgs1, imgs2 = torch.chunk(imgs, 2, dim=0)
        enc, dec, D, hp = self.encoder, self.decoder, self.netD, self.hparams
        L, n1, n2, dev = int(hp.latent_dim), imgs1.shape[0], imgs2.shape[0], imgs.device
        if eps1 is None:
            eps1 = torch.randn(n1, L, device=dev)                                         # where Normal.rsample() draws
        eps1 = eps1.to(device=dev, dtype=torch.float32)

        # ---- auto-encoding (factor_vae.py:90-102): recon + reg + adv_weight * g_adv into encoder and decoder
        hrows, tape_e = self._encode_rows(imgs1, record=True)
        z1, reg_loss = K.vae_latent_fwd(hrows, eps1)
        out, tape_d = dec.forward_nhwc(_decoder_input(z1), record=True)
        chw = imgs1[0].numel()
        mse, dout = K.eps_loss(out, imgs1, 1, want_grad=True, gscale=0.5 * chw)
        recon_loss = 0.5 * chw * mse + 0.5 * chw * math.log(2 * math.pi)                  # -mean over the batch of sum log N(x; recon, 1)
        fake = D.disc_forward(1.0, z=z1)                                                  # running statistics: first update
        g_adv_loss = fake["loss"]
        dz = dec.backward_nhwc(tape_d, dout, need_dx=True)[:, 0, 0, :]                    # [N, L] view of the pitched buffer (lddz = its pitch)
        D.disc_backward(fake, 1.0, param_grads=False, dz=dz, dz_scale=float(hp.adv_weight), accumulate_dz=True)
        dh = K.vae_latent_bwd(hrows, eps1, dz, 1.0)
        enc.backward_nhwc(tape_e, dh.view(n1, 1, 1, -1), need_dx=False)
        self._sync([enc, dec])
        ae_optim.step()

        # ---- discrimination (factor_vae.py:104-113), with the updated encoder
        if eps2 is None:
            eps2 = torch.randn(n2, L, device=dev)
        eps2 = eps2.to(device=dev, dtype=torch.float32)
        if perm is None:
            perm = permute_dims_index(n2, L, dev)
        elif not (torch.is_tensor(perm) and perm.is_cuda):
            raise RuntimeError("perm: an int64 tensor [latent_dim, N] on the images' HIP device is expected")
        h2rows, _ = self._encode_rows(imgs2, record=False)
        real = D.disc_forward(1.0, h=h2rows, eps=eps2, perm=perm)                         # running statistics: second update
        d_adv_loss = real["loss"] + fake["mean_sq_logit"]
        D.disc_backward(real, 1.0, accumulate=False)                                      # stores every gradient element
        D.disc_backward(fake, 0.0, accumulate=True)
        self._sync([D])
        discriminator_optim.step()

        self.log("train_loss/reg_loss", reg_loss)
        self.log("train_loss/recon_loss", recon_loss, prog_bar=True)
        self.log("train_loss/d_adv_loss", d_adv_loss)
        self.log("train_loss/g_adv_loss", g_adv_loss)
        self.log("train_log/real_logit", real["mean_logit"])
        self.log("train_log/fake_logit", fake["mean_logit"])

    def validation_step(self, batch, batch_idx):
        imgs, label = batch
        N = imgs.shape[0]
        z, recon_imgs, mu, log_sigma = self.vae(imgs)
        fake_image = self.sample(N)
        return ValidationResult(real_image=imgs, fake_image=fake_image, recon_image=recon_imgs, encode_latent=z, label=label)
