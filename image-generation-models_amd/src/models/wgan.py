"""`WGAN` (https://arxiv.org/abs/1701.07875) with the reference's surface (src/models/wgan.py:6-97) on the HIP kernels --
`experiment=wgan/mnist_conv`: the weight-clipped critic, RMSprop, `n_critic` critic steps per generator step.

Same constructor and defaults, attribute names (`generator`, `discriminator`), construction order (the seeded default weights are the
reference's), `state_dict` keys, `forward(z)`, two RMSprop optimizers (one `FlatRMSprop` per net), manual optimization, the logged keys
and `validation_step`.  `sample(N)` is added (the reference inherits it from its BaseModel).  The nets are the GAN's: the 28x28
`ConvDecoder` / `ConvEncoder` with BatchNorm (configs/networks/conv_mnist.yaml) on their segmented BatchNorm + activation path
(csrc/bn_seg.hip), without atomics.  The reference's conv32 / conv64 experiments (no BatchNorm nets here) and its MLP experiment
(its MLP nets cannot be constructed) are not built; `eval_fid=True` is refused (there is no FID callback).

`training_step(batch, batch_idx, z=None)` follows the reference (wgan.py:58-90) without recording an autograd graph:
  every step      clip the critic's parameters to [-clip_weight, clip_weight]: one K.clamp_ over the critic's flat buffer (conv weights
                  and biases and the BatchNorm affine pairs; the running statistics are not in it and are not clipped, as in the
                  reference; the buffer's zero padding stays zero);
  batch_idx % (n_critic + 1) == 0
                  generator   G forward -> D forward on the fake in training mode (D's running statistics update) ->
                              g_loss = -mean -> D backward for the input gradient alone -> G backward -> G's RMSprop;
  otherwise       critic      G forward in training mode without a tape (G's running statistics update) -> D forward on
                              [imgs | fake] as ONE pass of N + N rows with `segments=2`, real first -> d_loss = -mean(real) + mean(fake)
                              -> D backward with parameter gradients and no input gradient -> the output bias' gradient set to its
                              analytic 0 -> D's RMSprop.
The clip is a launch of its own and not part of the optimizer kernel: after a critic step the reference's state_dict holds the UNCLIPPED
result of the RMSprop update, and after a generator step the clipped weights although only G stepped.  Clamping is idempotent, so the
launch is skipped when the critic's flat buffer has not changed since the last clip -- keyed as `FlatNet._shadows` keys its repack
(data_ptr, _version, _dirty), and on the parameters' own version counters -- which is every step that follows a generator step (only G
stepped); after a `load_state_dict` or a move to another device the next step clips.  `ALWAYS_CLIP = True` clips in every step
regardless.
In the critic phase the gradient of the critic's output bias is -1 + 1 = 0; it is stored as that exact 0, as the reference's autograd
computes it, and not as the rounding noise of the kernels' sum, which RMSprop would turn into steps (see `training_step`).
z is a device draw, every logged scalar stays a device tensor, nothing in the step synchronises with the host.  A CPU tensor raises.
"""
import torch

from ..ops import functional as K
from .base import BaseModel, ValidationResult
from .gan import GAN, _base

# True: launch the critic's clip in every step even when its flat buffer has not changed since the last clip (tools/bench_wgan_clip.py and
# tests/test_wgan_clip_gpu.py compare both: the states are bit-identical).
ALWAYS_CLIP = False


class WGAN(BaseModel):
    def __init__(self, datamodule, netG=None, netD=None, latent_dim: int = 100, n_critic: int = 5, clip_weight: float = 0.01,
                 lrG: float = 5e-5, lrD: float = 5e-5, alpha: float = 0.99, eval_fid: bool = False):
        super().__init__(datamodule)
        self.save_hyperparameters()
        if eval_fid:
            raise NotImplementedError("eval_fid=True: there is no FID callback in this package")
        try:                                                    # pragma: no cover - hydra is not in this image
            from hydra.utils import instantiate
        except Exception:                                       # noqa: BLE001
            from ..runtime.config import instantiate
        self.generator = instantiate(netG, input_channel=latent_dim, output_channel=self.channels)
        self.discriminator = instantiate(netD, input_channel=self.channels, output_channel=1)
        from ..networks.basic import ConvDecoder, ConvEncoder
        G, D = self.generator, self.discriminator
        if (not isinstance(G, ConvDecoder) or not isinstance(D, ConvEncoder) or G.norm_type != "batch" or D.norm_type != "batch"
                or (self.height, self.width) != (28, 28)):
            raise NotImplementedError("WGAN on the HIP path: src.networks.basic.ConvDecoder / ConvEncoder with norm_type='batch' on 28x28 "
                                      "images (configs/networks/conv_mnist.yaml); the MLP and conv32 / conv64 experiments are not built")
        G.use_fused_norm_act(True)                              # the critic phase's two-segment pass needs the segmented kernels
        D.use_fused_norm_act(True)
        G.reproducible = D.reproducible = True                  # no atomics anywhere in the step: two runs give the same bits
        self.automatic_optimization = False
        self._clip_key = None                                   # the critic's flat buffer as the last clip left it

    def forward(self, z):
        output = self.generator(z)
        return output.reshape(z.shape[0], self.channels, self.height, self.width)

    def flat_nets(self):
        return [self.generator, self.discriminator]

    def configure_optimizers(self):
        from ..runtime.optim import FlatRMSprop
        hp = self.hparams
        opt_g = FlatRMSprop(self.generator, lr=hp.lrG, alpha=hp.alpha)
        opt_d = FlatRMSprop(self.discriminator, lr=hp.lrD, alpha=hp.alpha)
        return [opt_g, opt_d]

    def sample(self, N: int):
        with torch.no_grad():
            return self.forward(torch.randn(N, int(self.hparams.latent_dim), device=self.device))

    _sync = GAN._sync
    _on_gpu = staticmethod(GAN._on_gpu)
    _z_nhwc = GAN._z_nhwc

    def _clip_critic(self):
        """wgan.py:67-68 over the critic's flat buffer; skipped when nothing wrote the buffer since the last clip."""
        D = self.discriminator
        if ALWAYS_CLIP or self._critic_key() != self._clip_key:
            c = float(self.hparams.clip_weight)
            with torch.no_grad():
                K.clamp_(D.flat_params, -c, c)                  # behind torch's back: no version counter moves
            D.mark_params_dirty()
            self._clip_key = self._critic_key()

    def _critic_key(self):
        """What `FlatNet._shadows` keys its repack on, and the parameters' own version counters: once the net has moved to another
        device a parameter no longer shares the flat buffer's counter, and `load_state_dict` writes through the parameters."""
        D = self.discriminator
        flat = D.flat_params
        return (flat.data_ptr(), flat._version, D._dirty) + tuple(p._version for _, p in D._plist)

    def training_step(self, batch, batch_idx, z=None):
        imgs, _ = batch  # (N, C, H, W)
        imgs = self._on_gpu(imgs, "images")
        N = imgs.shape[0]
        G, D = self.generator, self.discriminator
        zin = self._z_nhwc(z, N)
        opt_g, opt_d = self.optimizers()

        self._clip_critic()

        if batch_idx % (int(self.hparams.n_critic) + 1) == 0:
            # ---- generator phase (wgan.py:70-78)
            fake, tape_g = G.forward_nhwc(zin, record=True)
            pred_fake, tape_d = D.forward_nhwc(fake, record=True)
            loss, _, dlogit = K.critic_loss(pred_fake, [True])                      # -mean(D(G(z)))
            dfake = D.backward_nhwc(tape_d, dlogit, need_dx=True, param_grads=False)
            G.backward_nhwc(tape_g, dfake[..., :self.channels])
            self._sync(G)
            opt_g.step()
            self.log("train_loss/g_loss", loss[0])
            return

        # ---- critic phase (wgan.py:80-90)
        fake, _ = G.forward_nhwc(zin, record=False)                                # detached in the reference (:82)
        x = torch.cat([_base(K.nchw_to_nhwc(imgs)), _base(fake)])[..., :self.channels]   # real first: the reference's order of D calls
        pred, tape = D.forward_nhwc(x, record=True, segments=2)
        loss, mean_logit, dlogit = K.critic_loss(pred, [True, False])
        D.backward_nhwc(tape, dlogit, need_dx=False)
        # d d_loss / d (the critic's output bias) = -1 + 1: the reference's autograd hands RMSprop an exact 0 and the bias stays where it
        # is.  The sum of N times -1/N and N times +1/N that the kernels form is rounding noise instead, and RMSprop from v = 0 turns any
        # noise above eps into a step of lr / sqrt(1 - alpha) (docs/kernels.md 4k) that shifts every logit.  Store the analytic value.
        D._gv["network.8.bias"].zero_()
        self._sync(D)
        opt_d.step()
        self.log("train_loss/d_loss", loss[0] + loss[1])
        self.log("train_log/real_logit", mean_logit[0])
        self.log("train_log/fake_logit", mean_logit[1])

    def validation_step(self, batch, batch_idx):
        img, _ = batch
        with torch.no_grad():
            z = torch.randn(img.shape[0], int(self.hparams.latent_dim), device=img.device)
            fake_imgs = self.forward(z)
        return ValidationResult(real_image=img, fake_image=fake_imgs)
