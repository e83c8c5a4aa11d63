"""`AAE` (adversarial autoencoder, https://arxiv.org/abs/1511.05644) with the reference's surface (src/models/aae.py:17-123) on the HIP
kernels -- `experiment=aae/mnist`.

An autoencoder whose latent code is pushed towards a prior by a discriminator on the LATENT code.  Same constructor and defaults,
attribute names and construction order (`decoder`, `encoder`, `discriminator`: the seeded default weights are the reference's), manual
optimization with two Adam optimizers, the five logged keys, `forward(z)` = decode, `sample_prior`, `validation_step`.  `sample(N)` is
added (the reference inherits it from its BaseModel).  The constructor's `netD` is accepted and ignored, as in the reference, which
builds MLPEncoder(latent_dim, [256, 256], 1, norm_type="layer") itself: here `LayerNormMLPEncoder` on csrc/latent_disc_ln.hip.

`training_step` follows the reference's three phases (aae.py:75-113) without recording an autograd graph:
  reconstruction   encoder -> q_z -> decoder, mean squared error (K.eps_loss, gradient scaled by recon_weight), decoder backward ->
                   encoder backward; opt_g steps both nets;
  discriminator    ONE forward of the updated encoder, which stands for the reference's second and third forward (same weights, same
                   batch: identical outputs) -- its BatchNorm running statistics take two momentum updates and num_batches_tracked
                   += 2; D reads [prior | q_z] as one pass of N + N rows with targets 1 and 0 (q_z in place from the encoder's NHWC
                   output), backward of 0.5 loss_real + 0.5 loss_fake into D's parameters only (the gradient the reference puts on
                   the encoder here is thrown away by its next zero_grad); opt_d steps;
  generator        the updated D on q_z against target 1, backward for the input gradient alone (one launch) -> encoder backward on
                   the discriminator phase's tape; the encoder's Adam steps ALONE.
In that last phase the reference's decoder has `grad = None` and torch's Adam skips it entirely -- no moment decay, no step count: after
k training steps the encoder's Adam state is at step 2k and the decoder's at k.  `PerNetAdam` keeps one `FlatAdam` per net for that.
`loss_mode` "vanilla" (the default) and "lsgan" are built.  "hinge" is refused: the reference's hinge loss for real targets is
max(1 - x, 1), which is not the hinge loss.  `prior="toy_gmm"` is refused: the reference cannot run it (ToyGMM(10) lacks its `device`
argument).  Every random draw is a device draw, every logged scalar stays a device tensor, nothing in the step synchronises with the
host.  A CPU tensor raises.
"""
import torch

from ..networks.latent_mlp import LayerNormMLPEncoder
from ..ops import functional as K
from .base import BaseModel, ValidationResult


class PerNetAdam:
    """One `FlatAdam` per net behind one optimizer object: `step()` steps every net, `step(nets=[...])` only those, and each net keeps
    its own step count and moments -- what torch.optim.Adam does per parameter when some parameters have no gradient."""

    def __init__(self, nets, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        from ..runtime.optim import FlatAdam
        self.nets = list(nets)
        self.parts = [FlatAdam(n, lr=lr, betas=betas, eps=eps) for n in self.nets]

    @property
    def param_groups(self):
        return [g for p in self.parts for g in p.param_groups]

    @property
    def grad_scale(self):
        return self.parts[0].grad_scale

    @grad_scale.setter
    def grad_scale(self, v):
        for p in self.parts:
            p.grad_scale = v

    def zero_grad(self, set_to_none: bool = False):
        pass                                                   # every backward overwrites the flat gradient buffers

    def step(self, closure=None, nets=None):
        loss = closure() if closure is not None else None
        for n, p in zip(self.nets, self.parts):
            if nets is None or any(n is m for m in nets):
                p.step()
        return loss

    def step_counts(self):
        return [p.device_step_count() for p in self.parts]

    def state_dict(self):
        return {"parts": [p.state_dict() for p in self.parts]}

    def load_state_dict(self, sd):
        parts = sd["parts"]
        if len(parts) != len(self.parts):
            raise ValueError(f"optimizer state holds {len(parts)} nets, the optimizer has {len(self.parts)}")
        for p, s in zip(self.parts, parts):
            p.load_state_dict(s)


class AAE(BaseModel):
    def __init__(self, datamodule, encoder=None, decoder=None, netD=None, latent_dim=100, loss_mode="vanilla", lrG: float = 0.0002,
                 lrD: float = 0.0002, b1: float = 0.5, b2: float = 0.999, recon_weight=1, prior="normal"):
        super().__init__(datamodule)
        self.save_hyperparameters()
        if loss_mode == "hinge":
            raise NotImplementedError("loss_mode='hinge': the reference's hinge loss for real targets is max(1 - x, 1) "
                                      "(src/utils/losses.py:17-21), which is not the hinge loss; 'vanilla' and 'lsgan' are built")
        if loss_mode not in K.LATENT_DISC_LN_LOSSES:
            raise NotImplementedError(f"loss_mode={loss_mode!r}: 'vanilla' and 'lsgan' are built")
        if prior == "toy_gmm":
            raise NotImplementedError("prior='toy_gmm': the reference cannot run it (aae.py:72 builds ToyGMM(10) without its device "
                                      "argument); only prior='normal' is built")
        if prior != "normal":
            raise NotImplementedError(f"prior={prior!r}: only 'normal' is built")
        if not 1 <= int(latent_dim) <= 64:
            raise NotImplementedError(f"latent_dim={latent_dim}: the latent discriminator's kernels take 1 to 64 input features")
        try:                                                    # pragma: no cover - hydra is not in this image
            from hydra.utils import instantiate
        except Exception:                                       # noqa: BLE001
            from ..runtime.config import instantiate
        self.decoder = instantiate(decoder, input_channel=latent_dim, output_channel=self.channels)
        self.encoder = instantiate(encoder, input_channel=self.channels, output_channel=latent_dim)
        self.discriminator = LayerNormMLPEncoder(input_channel=latent_dim, output_channel=1, hidden_dims=[256, 256], width=1, height=1,
                                                 norm_type="layer")
        self.automatic_optimization = False

    def forward(self, z):
        output = self.decoder(z)
        return output.reshape(z.shape[0], self.channels, self.height, self.width)

    def flat_nets(self):
        return [self.decoder, self.encoder, self.discriminator]

    def configure_optimizers(self):
        from ..runtime.optim import FlatAdam
        hp = self.hparams
        opt_g = PerNetAdam([self.encoder, self.decoder], lr=hp.lrG, betas=(hp.b1, hp.b2))
        opt_d = FlatAdam(self.discriminator, lr=hp.lrD, betas=(hp.b1, hp.b2))
        return opt_g, opt_d

    def sample_prior(self, N):
        return torch.randn(N, int(self.hparams.latent_dim), device=self.device)

    def sample(self, N: int):
        with torch.no_grad():
            return self.forward(self.sample_prior(N))

    def _sync(self, nets):
        from ..runtime.ddp import allreduce_flat_grads
        allreduce_flat_grads(list(nets))

    @staticmethod
    def _on_gpu(imgs):
        if not imgs.is_cuda:
            raise RuntimeError("libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
        return imgs.float().contiguous()

    def _decode_nhwc(self, q, record):
        """q: the encoder's NHWC output [N, 1, 1, L].  The convolution kernels want a pixel pitch that is a multiple of 4 with zero padding
        lanes: the encoder's output is that when L % 4 == 0 (no padding); otherwise the rows are repacked (one launch)."""
        if q.shape[-1] % 4 != 0:
            q = K.nchw_to_nhwc(q[:, 0, 0, :].reshape(q.shape[0], -1, 1, 1))
        return self.decoder.forward_nhwc(q, record=record)

    def training_step(self, batch, batch_idx, optimizer_idx=None, prior=None):
        imgs, _ = batch  # (N, C, H, W)
        imgs = self._on_gpu(imgs)
        N, dev = imgs.shape[0], imgs.device
        opt_g, opt_d = self.optimizers()
        enc, dec, D, hp = self.encoder, self.decoder, self.discriminator, self.hparams
        L, mode = int(hp.latent_dim), hp.loss_mode
        x = K.nchw_to_nhwc(imgs)

        # ---- reconstruction phase (aae.py:80-88)
        q, tape_e = enc.forward_nhwc(x, record=True)                                      # [N,1,1,L]
        out, tape_d = self._decode_nhwc(q, record=True)
        recon_loss, dout = K.eps_loss(out, imgs, 1, want_grad=True, gscale=float(hp.recon_weight))
        dq = dec.backward_nhwc(tape_d, dout, need_dx=True)
        enc.backward_nhwc(tape_e, dq[..., :L], need_dx=False)
        self._sync([enc, dec])
        opt_g.step()

        # ---- regularization phase: update the discriminator (aae.py:90-104), with the updated encoder
        if prior is None:
            prior = self.sample_prior(N)
        elif not (torch.is_tensor(prior) and prior.is_cuda):
            raise RuntimeError("prior: a float tensor [N, latent_dim] on the images' HIP device is expected")
        prior = prior.to(dtype=torch.float32).contiguous()
        q, tape_e = enc.forward_nhwc(x, record=True, bn_updates=2)                        # the reference's second AND third forward
        q_rows = q[:, 0, 0, :]                                                            # [N, L] view: its pitch goes to the kernel
        rec = D.disc_forward(prior, 1.0, x1=q_rows, target1=0.0, loss_mode=mode)
        D.disc_backward(rec, 1.0, 0.0, c0=0.5, c1=0.5, param_grads=True, accumulate=False)  # stores every gradient element
        self._sync([D])
        opt_d.step()

        # ---- update the generator (aae.py:106-113), with the updated discriminator
        gen = D.disc_forward(q_rows, 1.0, loss_mode=mode)
        dqz = torch.zeros((N, 1, 1, (L + 3) // 4 * 4), device=dev, dtype=torch.float32)
        D.disc_backward(gen, 1.0, c0=1.0, param_grads=False, dx0=dqz[:, 0, 0, :L])
        enc.backward_nhwc(tape_e, dqz[..., :L], need_dx=False)
        self._sync([enc])
        opt_g.step(nets=[enc])                                                            # the decoder has no gradient: Adam skips it

        self.log("train_loss/recon_loss", recon_loss)
        self.log("train_loss/d_loss", rec["d_loss"])
        self.log("train_log/real_logit", rec["mean_logit0"])
        self.log("train_log/fake_logit", rec["mean_logit1"])
        self.log("train_loss/adv_encoder_loss", gen["loss0"])

    def validation_step(self, batch, batch_idx):
        imgs, label = batch
        with torch.no_grad():
            x = self._on_gpu(imgs)
            q, _ = self.encoder.forward_nhwc(K.nchw_to_nhwc(x), record=False)
            out, _ = self._decode_nhwc(q, record=False)
            z = q[:, 0, 0, :].contiguous()
            sample_imgs = self.forward(self.sample_prior(imgs.shape[0]))
        return ValidationResult(real_image=imgs, fake_image=sample_imgs, recon_image=K.nhwc_to_nchw(out), label=label, encode_latent=z)
