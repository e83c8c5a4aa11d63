"""`AGE` ("It Takes (Only) Two: Adversarial Generator-Encoder Networks", https://arxiv.org/abs/1704.02304) with the reference's surface
(src/models/age.py:11-159) on the HIP kernels -- `experiment=age/mnist`.

Same constructor and defaults, attribute names and construction order (`decoder`, then `encoder`: the seeded default weights are the
reference's), `state_dict` keys, `forward(z)`, `encode`, `calculate_kl`'s arithmetic, two Adam optimizers (one `FlatAdam` per net, lrE /
lrG) each with the reference's `LambdaLR` of 0.5 ** (epoch // drop_lr_epoch), the logged keys and `validation_step`.  `sample(N)` is
added.  The nets are the 28x28 `ConvDecoder` / `ConvEncoder` with BatchNorm (configs/networks/conv_mnist.yaml) on their segmented
BatchNorm + activation path (csrc/bn_seg.hip); everything between the encoder's output and the scalar losses -- the normalisation
onto the sphere, the batch moments of the code, the KL of the fitted diagonal Gaussian to N(0, I), the code-reconstruction terms --
and its backward is csrc/age_ops.hip (K.age_moments_fwd / K.age_moments_bwd).  There is no discriminator.  The reference's age/cifar10
and age/celeba experiments (conv32 / conv64 nets, which carry no BatchNorm here) are not built.

The reference runs under Lightning's automatic optimization with `frequency` 1 : g_updates, so batch b belongs to the encoder when
b % (1 + g_updates) == 0 and to the decoder otherwise; the net that does not step is frozen, gradients still flow through it, and
both nets run in training mode in both phases (both update their BatchNorm running statistics).  Here optimization is manual and
`training_step(batch, batch_idx, z=None)` picks the phase from batch_idx, without recording an autograd graph:
  encoder phase   decoder on z (no tape) -> encoder on [imgs | fake] as ONE pass of N + N rows with `segments=2` -> moments: real_kl,
                  fake_kl, 1 - cos(fake_z, z) -> with e_recon_x_weight > 0 the decoder on real_z, the image MSE (K.age_image_mse: K.eps_loss's
                  arithmetic with the loss summed in a fixed order, not with an atomic), and the decoder's
                  backward for the input gradient alone -> moments backward with c = (+1, -1) -> encoder backward -> encoder's Adam;
  decoder phase   decoder on z -> encoder on the fake (on [fake | imgs] when g_recon_x_weight > 0) -> fake_kl, mse(fake_z, z) ->
                  moments backward with c = +1 -> encoder backward for the input gradient alone -> decoder backward -> with
                  g_recon_x_weight > 0 the decoder on real_z (which carries no gradient: the encoder is frozen and the images are
                  data), the image MSE and its backward accumulated -> decoder's Adam.
Each net sees its forward calls in the reference's order, so the running statistics move as the reference's do.  z is a device
draw, every logged scalar stays a device tensor, nothing in the step synchronises with the host.  A CPU tensor raises.  Under data
parallelism the stepping net's gradients are all-reduced; the moments are per rank, as in the reference under DDP.
"""
import torch

from ..ops import functional as K
from .base import BaseModel, ValidationResult
from .gan import SEGMENTED_NORM, _base

E_LOGS = ("train_loss/real_kl", "train_loss/fake_kl", "train_loss/total_e_loss", "train_log/real_mu", "train_log/real_var",
          "train_log/fake_mu", "train_log/fake_var")           # and train_loss/recon_x when e_recon_x_weight > 0
G_LOGS = ("train_loss/g_recon_z", "train_loss/g_loss")


class AGE(BaseModel):
    def __init__(self, datamodule, encoder=None, decoder=None, lrE: float = 2e-4, lrG: float = 2e-4, latent_dim=128, b1: float = 0.5,
                 b2: float = 0.999, e_recon_z_weight=1000, e_recon_x_weight=0, g_recon_z_weight=0, g_recon_x_weight=10, norm_z=True,
                 drop_lr_epoch=20, g_updates=2):
        super().__init__(datamodule)
        self.save_hyperparameters()
        if int(g_updates) < 1 or int(drop_lr_epoch) < 1 or not 1 <= int(latent_dim) <= K.AGE_LMAX:
            raise NotImplementedError(f"AGE: g_updates and drop_lr_epoch of at least 1, latent_dim in [1, {K.AGE_LMAX}]")
        try:                                                    # pragma: no cover - hydra is not in this image
            from hydra.utils import instantiate
        except Exception:                                       # noqa: BLE001
            from ..runtime.config import instantiate
        self.decoder = instantiate(decoder, input_channel=latent_dim, output_channel=self.channels)
        self.encoder = instantiate(encoder, input_channel=self.channels, output_channel=latent_dim)
        from ..networks.basic import ConvDecoder, ConvEncoder
        if (not isinstance(self.decoder, ConvDecoder) or not isinstance(self.encoder, ConvEncoder) or self.decoder.norm_type != "batch"
                or self.encoder.norm_type != "batch" or (self.height, self.width) != (28, 28)):
            raise NotImplementedError("AGE on the HIP path: src.networks.basic.ConvDecoder / ConvEncoder with norm_type='batch' on 28x28 "
                                      "images (configs/networks/conv_mnist.yaml); the MLP and conv32 / conv64 experiments are not built")
        self.decoder.use_fused_norm_act(SEGMENTED_NORM)
        self.encoder.use_fused_norm_act(SEGMENTED_NORM)
        self.decoder.reproducible = self.encoder.reproducible = True    # no atomics anywhere in the step: two runs give the same bits
        self.automatic_optimization = False

    # ------------------------------------------------------------------ surface
    def forward(self, z):
        output = self.decoder(z)
        return output.reshape(z.shape[0], self.channels, self.height, self.width)

    def flat_nets(self):
        return [self.decoder, self.encoder]

    def configure_optimizers(self):
        from ..runtime.optim import FlatAdam
        hp = self.hparams
        drop = int(hp.drop_lr_epoch)

        def lambda_func(epoch):
            return 0.5 ** (epoch // drop)
        # host_complements: 1 - beta rounded once from double, as torch's Adam takes them (csrc/elementwise.hip, adam_c_kernel)
        opt_e = FlatAdam(self.encoder, lr=hp.lrE, betas=(hp.b1, hp.b2), host_complements=True)
        opt_g = FlatAdam(self.decoder, lr=hp.lrG, betas=(hp.b1, hp.b2), host_complements=True)
        scheds = [torch.optim.lr_scheduler.LambdaLR(opt_e, lr_lambda=lambda_func), torch.optim.lr_scheduler.LambdaLR(opt_g, lr_lambda=lambda_func)]
        return [opt_e, opt_g], scheds

    def optimizers(self):
        """[opt_e, opt_g].  Without a trainer (which binds them and steps the schedulers itself) they are built here, and the two
        epoch schedulers are kept for `lr_schedulers()`."""
        if getattr(self, "_optimizers", None) is None:
            opts, scheds = self.configure_optimizers()
            object.__setattr__(self, "_optimizers", list(opts))
            object.__setattr__(self, "_lr_schedulers", list(scheds))
        return self._optimizers

    def lr_schedulers(self):
        self.optimizers()
        trainer = getattr(self, "trainer", None)
        return getattr(self, "_lr_schedulers", None) or list(getattr(trainer, "lr_schedulers", []))

    def phase(self, batch_idx: int) -> str:
        """"E" or "G": Lightning's alternation of two optimizers with frequencies 1 and g_updates."""
        return "E" if int(batch_idx) % (1 + int(self.hparams.g_updates)) == 0 else "G"

    @staticmethod
    def _on_gpu(t, what):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError(f"{what}: libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
        return t.float().contiguous()

    def _prior(self, N, z=None):
        """The prior draw [N, L], on the sphere when norm_z is set (age.py:90-92)."""
        L = int(self.hparams.latent_dim)
        if z is None:
            z = torch.randn(N, L, device=self.device)
        z = self._on_gpu(z, "z")
        if z.shape != (N, L):
            raise RuntimeError(f"z: [{N}, {L}] expected, got {tuple(z.shape)}")
        return K.age_normalize(z) if self.hparams.norm_z else z

    def _z_nhwc(self, z):
        """Code rows [N, L] as the decoder's NHWC input [N, 1, 1, L]: a view when they are dense and L % 4 == 0 (the convolutions' pixel
        pitch), else repacked."""
        N, L = z.shape
        if L % 4 == 0 and z.is_contiguous():
            return z.view(N, 1, 1, L)
        return K.nchw_to_nhwc(z.contiguous().view(N, L, 1, 1))

    def _code(self, x_nhwc, record=False, segments=1, recon=(None, None), target=None):
        """The encoder on NHWC images and the moments of its (normalised) output -> (record of K.age_moments_fwd, encoder tape)."""
        e, tape = self.encoder.forward_nhwc(x_nhwc, record=record, segments=segments)
        return K.age_moments_fwd(e, segments, normalize=bool(self.hparams.norm_z), recon=recon, target=target), tape

    def encode(self, imgs):
        """[N, L]: the encoder's output, on the sphere when norm_z is set, in whatever mode the module is in."""
        imgs = self._on_gpu(imgs, "images")
        with torch.no_grad():
            e, _ = self.encoder.forward_nhwc(K.nchw_to_nhwc(imgs), record=False)
            e = e.reshape(imgs.shape[0], -1)
            return K.age_normalize(e) if self.hparams.norm_z else e.contiguous()

    def calculate_kl(self, samples, return_state=False):
        """KL of the diagonal Gaussian fitted to the rows of `samples` [M, L] to N(0, I) (age.py:64-74), on the kernels."""
        rec = K.age_moments_fwd(self._on_gpu(samples, "samples"), 1, normalize=False)
        if return_state:
            return rec["kl"][0], rec["mean_mu"][0], rec["mean_var"][0]
        return rec["kl"][0]

    def sample(self, N: int):
        with torch.no_grad():
            return self.forward(self._prior(N))

    def _sync(self, net):
        from ..runtime.ddp import allreduce_flat_grads
        allreduce_flat_grads([net])

    # ------------------------------------------------------------------ training
    def training_step(self, batch, batch_idx, z=None):
        imgs, _ = batch  # (N, C, H, W)
        imgs = self._on_gpu(imgs, "images")
        zt = self._prior(imgs.shape[0], z)
        if self.phase(batch_idx) == "E":
            self._encoder_phase(imgs, zt)
        else:
            self._decoder_phase(imgs, zt)

    def _encoder_phase(self, imgs, zt):
        """age.py:95-125."""
        hp, G, E, N = self.hparams, self.decoder, self.encoder, imgs.shape[0]
        wx, wz = float(hp.e_recon_x_weight), float(hp.e_recon_z_weight)
        opt_e, _ = self.optimizers()
        fake, _ = G.forward_nhwc(self._z_nhwc(zt), record=False)                  # the decoder is frozen: nothing flows back through the fake
        x = torch.cat([_base(K.nchw_to_nhwc(imgs)), _base(fake)])[..., :self.channels]    # real first: the reference's order of encoder calls
        rec, tape_e = self._code(x, record=True, segments=2, recon=(None, "cosine" if wz > 0 else None), target=zt)
        total = rec["kl"][0] - rec["kl"][1]
        dz = None
        if wx > 0:
            recon, tape_g = G.forward_nhwc(self._z_nhwc(rec["z"][:N]), record=True)
            recon_x, dout = K.age_image_mse(recon, imgs, want_grad=True, gscale=wx)
            dz = G.backward_nhwc(tape_g, dout, need_dx=True, param_grads=False)[..., :int(hp.latent_dim)]
            self.log("train_loss/recon_x", recon_x)
            total = total + wx * recon_x
        if wz > 0:
            total = total + wz * rec["recon"][1]
        de = K.age_moments_bwd(rec, c=(1.0, -1.0), w=(0.0, wz), dz_ext=(dz, None))
        E.backward_nhwc(tape_e, de, need_dx=False)
        self._sync(E)
        opt_e.step()
        self.log("train_loss/real_kl", rec["kl"][0])
        self.log("train_loss/fake_kl", rec["kl"][1])
        self.log("train_loss/total_e_loss", total)
        self.log("train_log/real_mu", rec["mean_mu"][0])
        self.log("train_log/real_var", rec["mean_var"][0])
        self.log("train_log/fake_mu", rec["mean_mu"][1])
        self.log("train_log/fake_var", rec["mean_var"][1])

    def _decoder_phase(self, imgs, zt):
        """age.py:128-148."""
        hp, G, E, N = self.hparams, self.decoder, self.encoder, imgs.shape[0]
        wx, wz = float(hp.g_recon_x_weight), float(hp.g_recon_z_weight)
        _, opt_g = self.optimizers()
        fake, tape_g = G.forward_nhwc(self._z_nhwc(zt), record=True)
        if wx > 0:
            x = torch.cat([_base(fake), _base(K.nchw_to_nhwc(imgs))])[..., :self.channels]    # fake first: the reference's order of encoder calls
        else:
            x = fake
        S = 2 if wx > 0 else 1
        rec, tape_e = self._code(x, record=True, segments=S, recon=("mse" if wz > 0 else None, None), target=zt)
        total = rec["kl"][0]
        recon_z = rec["recon"][0]                                                 # 0 without the term, as the reference logs it
        if wz > 0:
            total = total + wz * recon_z
        de = K.age_moments_bwd(rec, c=(1.0, 0.0), w=(wz, 0.0))                    # real_z carries no gradient: its rows of de are 0
        # with g_recon_x_weight > 0 the encoder's backward walks all 2N rows although the second segment's gradient is zero: correct, and
        # one N-row pass wasted; walking segment 0 alone would need the segmented tape sliced, and no shipped config takes this path
        dx = E.backward_nhwc(tape_e, de, need_dx=True, param_grads=False)
        G.backward_nhwc(tape_g, dx[:N][..., :self.channels])
        if wx > 0:
            recon, tape_r = G.forward_nhwc(self._z_nhwc(rec["z"][N:]), record=True)
            recon_x, dout = K.age_image_mse(recon, imgs, want_grad=True, gscale=wx)
            G.accumulate_grads = True
            try:
                G.backward_nhwc(tape_r, dout)
            finally:
                G.accumulate_grads = False
            total = total + wx * recon_x
        self._sync(G)
        opt_g.step()
        self.log("train_loss/g_recon_z", recon_z)
        self.log("train_loss/g_loss", total)

    def validation_step(self, batch, batch_idx):
        img, _ = batch
        with torch.no_grad():
            fake_img = self.forward(self._prior(img.shape[0]))
            encode_z = self.encode(img)
            recon_img = self.forward(encode_z)
        return ValidationResult(real_image=img, fake_image=fake_img, recon_image=recon_img, encode_latent=encode_z)
