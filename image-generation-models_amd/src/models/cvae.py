"""`cVAE` with the reference's surface (src/models/cvae.py:16-106) on the HIP kernels -- `experiment=cvae/mnist`.

The label-conditioned VAE: q(z | x, c) reads the image with one one-hot label plane per class appended to every pixel, p(x | z, c)
decodes [z | class_embedding(c)].  Same constructor (including the `decoder_dist="guassian"` default that the reference's own
`get_decode_dist` rejects -- the configs pass "gaussian"), attribute names (`decoder`, `encoder`, `class_embedding`, `n_classes`),
construction order (decoder, encoder, embedding: the seeded default weights are the reference's), logged keys, `forward(z, labels)`
= decode, `sample(N)` = N images per class, Adam + StepLR(1, 0.99).
`training_step` is one autograd node like the VAE's; what differs is label-indexed data movement, each one launch (csrc/cvae_ops.hip):
the encoder input is packed from the NCHW batch and the labels (no one-hot tensor, no cat), the latent block writes the decoder's
input [z | E[label]] itself, and its backward returns the embedding table's gradient as a fixed-order segmented sum.
Labels travel as int64 on the images' device; nothing in the step reads them on the host.  A CPU tensor raises.
"""
import math

import torch

from ..networks.embedding import ClassEmbedding
from ..ops import functional as K
from .base import BaseModel, ValidationResult
from .vae import _GaussianDistribution


def _encoder_input(model, imgs, labels):
    if model.hparams.encode_label:
        return K.cvae_pack_input(imgs, labels, model.n_classes)
    return K.nchw_to_nhwc(imgs)


class _CVAEStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, imgs, labels, eps, anchor, model):
        enc, dec, emb, hp = model.encoder, model.decoder, model.class_embedding, model.hparams
        record = ctx.needs_input_grad[3]
        imgs = imgs.float().contiguous()
        n = imgs.shape[0]
        h, tape_e = enc.forward_nhwc(_encoder_input(model, imgs, labels), record=record)       # [N,1,1,2L]
        hrows = h.reshape(n, -1)
        zc, kld = K.cvae_latent_fwd(hrows, eps, labels, emb.table)                             # [N,2L] = [z | E[label]]
        out, tape_d = dec.forward_nhwc(zc.view(n, 1, 1, -1), record=record)
        chw = imgs[0].numel()
        mse, dout = K.eps_loss(out, imgs, 1, want_grad=record, gscale=0.5 * float(hp.recon_weight) * chw)
        log_p = -0.5 * chw * mse - 0.5 * chw * math.log(2 * math.pi)                           # mean over the batch of sum log N(x; recon, 1)
        elbo = -float(hp.beta) * kld + float(hp.recon_weight) * log_p
        ctx.model, ctx.tapes, ctx.saved = model, (tape_e, tape_d), (hrows, eps, labels, dout)
        ctx.mark_non_differentiable(kld, log_p)
        return -elbo, kld, log_p, zc[:, :hrows.shape[1] // 2], K.nhwc_to_nchw(out)

    @staticmethod
    def backward(ctx, dloss, *_):
        model = ctx.model
        tape_e, tape_d = ctx.tapes
        hrows, eps, labels, dout = ctx.saved
        ctx.tapes = ctx.saved = None
        K.scale_by_device_scalar(dout, dloss)
        dzc = model.decoder.backward_nhwc(tape_d, dout, need_dx=True)
        n = hrows.shape[0]
        dh = K.cvae_latent_bwd(hrows, eps, labels, dzc.reshape(n, -1), float(model.hparams.beta), model.class_embedding.grad_table(),
                               g_dev=dloss.reshape(1).float())
        model.encoder.backward_nhwc(tape_e, dh.view(n, 1, 1, -1), need_dx=False)
        return None, None, None, None, None


class cVAE(BaseModel):
    def __init__(self, datamodule=None, encoder=None, decoder=None, latent_dim: int = 100, beta: float = 1.0, recon_weight: float = 1.0,
                 lr: float = 1e-4, b1: float = 0.9, b2: float = 0.999, n_classes: int = None, encode_label: bool = True,
                 decoder_dist="guassian"):
        super().__init__(datamodule)
        self.save_hyperparameters()
        if n_classes is None or int(n_classes) < 1:
            raise ValueError("n_classes: the number of label classes is needed (configs take it from datamodule.n_classes)")
        try:                                                    # pragma: no cover - hydra is not in this image
            from hydra.utils import instantiate
        except Exception:                                       # noqa: BLE001
            from ..runtime.config import instantiate
        n_classes = int(n_classes)
        self.decoder = instantiate(decoder, input_channel=latent_dim * 2, output_channel=self.channels, output_act=self.output_act)
        self.encoder = instantiate(encoder, input_channel=self.channels + (n_classes if encode_label else 0), output_channel=2 * latent_dim)
        self.class_embedding = ClassEmbedding(n_classes, latent_dim)
        if decoder_dist != "gaussian":
            raise NotImplementedError(f"decoder_dist={decoder_dist!r}: the reference's get_decode_dist knows 'gaussian' and 'bernoulli'; "
                                      "only the Gaussian decoder of the shipped configs is built here")
        self.decoder_dist = _GaussianDistribution()
        self.n_classes = n_classes
        object.__setattr__(self, "_anchor", torch.zeros(1, requires_grad=True))

    @staticmethod
    def _labels(labels, like):
        """int64 labels on the images' device (an asynchronous copy when they are elsewhere: no host synchronisation)."""
        if not like.is_cuda:
            raise RuntimeError("libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
        return torch.as_tensor(labels).to(device=like.device, dtype=torch.int64, non_blocking=True)

    def forward(self, z, labels):
        """Generate images given latent code and labels."""
        n = z.shape[0]
        zc, _ = K.cvae_latent_fwd(None, z.float(), self._labels(labels, z), self.class_embedding.table)
        out, _ = self.decoder.forward_nhwc(zc.view(n, 1, 1, -1), record=False)
        output = self.decoder_dist.sample(K.nhwc_to_nchw(out))
        return output.reshape(n, self.channels, self.height, self.width)

    def sample(self, N: int):
        """N images of every class, class-major: labels [0]*N + [1]*N + ..."""
        labels = torch.arange(self.n_classes, device=self.device).reshape(self.n_classes, 1).repeat(1, N).reshape(-1)
        z = torch.randn(N * self.n_classes, self.hparams.latent_dim).to(self.device)
        with torch.no_grad():
            return self.forward(z, labels)

    def flat_nets(self):
        return [self.decoder, self.encoder, self.class_embedding]

    def configure_optimizers(self):
        from ..runtime.optim import FlatAdam
        hp = self.hparams
        opt = FlatAdam(self.flat_nets(), lr=hp.lr, betas=(hp.b1, hp.b2))
        scheduler = torch.optim.lr_scheduler.StepLR(opt, 1, gamma=0.99)
        return [opt], [scheduler]

    def _step(self, imgs, labels, eps=None):
        labels = self._labels(labels, imgs)
        if eps is None:
            eps = torch.randn(imgs.shape[0], self.hparams.latent_dim, device=imgs.device)      # where Normal.rsample() draws
        if self._anchor.device != imgs.device:
            object.__setattr__(self, "_anchor", torch.zeros(1, device=imgs.device, requires_grad=True))
        anchor = self._anchor if (torch.is_grad_enabled() and self.training) else self._anchor.detach()
        return _CVAEStep.apply(imgs, labels, eps, anchor, self)

    def vae(self, imgs, labels):
        """(mu, log_sigma, z, recon_imgs) like the reference (cvae.py:64-74); inference only -- training goes through training_step."""
        with torch.no_grad():
            n = imgs.shape[0]
            labels = self._labels(labels, imgs)
            h, _ = self.encoder.forward_nhwc(_encoder_input(self, imgs.float().contiguous(), labels), record=False)
            hrows = h.reshape(n, -1)
            eps = torch.randn(n, self.hparams.latent_dim, device=imgs.device)
            zc, _ = K.cvae_latent_fwd(hrows, eps, labels, self.class_embedding.table)
            out, _ = self.decoder.forward_nhwc(zc.view(n, 1, 1, -1), record=False)
            mu, log_sigma = torch.chunk(hrows, 2, dim=1)
            return mu, log_sigma, zc[:, :self.hparams.latent_dim], K.nhwc_to_nchw(out)

    def training_step(self, batch, batch_idx, eps=None):
        imgs, labels = batch
        neg_elbo, kld, log_p_x_of_z, _, _ = self._step(imgs, labels, eps)
        self.log("train_log/elbo", -neg_elbo.detach())
        self.log("train_log/kl_divergence", kld)
        self.log("train_log/log_p_x_of_z", log_p_x_of_z)
        return neg_elbo

    def validation_step(self, batch, batch_idx):
        imgs, labels = batch
        with torch.no_grad():
            mu, log_sigma, z, recon_imgs = self.vae(imgs, labels)
            chw = imgs[0].numel()
            mse, _ = K.eps_loss(K.nchw_to_nhwc(recon_imgs), imgs.float(), 1, want_grad=False)
            log_p_x_of_z = -0.5 * chw * mse - 0.5 * chw * math.log(2 * math.pi)
            fake_imgs = self.sample(8)
        self.log("val_log/log_p_x_of_z", log_p_x_of_z)
        return ValidationResult(real_image=imgs, fake_image=fake_imgs, recon_image=recon_imgs, label=labels, encode_latent=z)
