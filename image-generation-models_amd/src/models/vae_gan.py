"""`VAEGAN` ("Autoencoding beyond pixels using a learned similarity metric", https://arxiv.org/abs/1512.09300) with the reference's
surface (src/models/vae_gan.py:14-113) on the HIP kernels -- `experiment=vaegan/mnist`.

Same constructor and defaults, attribute names and construction order (`decoder`, `encoder` with 2 L outputs, `netD` = the encoder
config with one output and `return_features=True`: the seeded default weights are the reference's), `state_dict` keys, `forward(z)`,
two Adam optimizers (`optim_ae` over encoder + decoder, `optim_d` over netD), manual optimization, the seven logged keys and
`validation_step` (which logs `val_log/van_mse`, the reference's spelling).  `sample(N)` is added.  The nets are the 28x28
`ConvDecoder` / `ConvEncoder` with BatchNorm (configs/networks/conv_mnist.yaml) on their segmented BatchNorm + activation path
(csrc/bn_seg.hip); the reference's vaegan/cifar10 and vaegan/celeba experiments (conv32 / conv64 nets, which carry no BatchNorm here)
are not built.

There are no alternating phases: every batch steps both optimizers.  `training_step(batch, batch_idx, eps=None, prior_z=None)`
follows vae_gan.py:63-102 without recording an autograd graph:
  forward     encoder on imgs -> [mu | log_sigma] -> K.vaegan_latent_fwd writes the decoder's input [z | prior_z] and the KL term ->
              decoder on the 2 N rows as ONE `segments=2` pass (recon half first: its two calls in the reference's order) ->
              K.vaegan_pack_fwd -> netD on [fake | imgs | recon] as ONE `segments=3` pass (the reference's order of netD calls: every
              BatchNorm layer keeps statistics per segment and updates its running statistics three times) -> K.adv_loss per segment;
  optim_ae    netD backward for the input gradient alone (`param_grads=False`): dlogit of BCE(fake, 1) on the fake segment, and on
              the recon segment the feature gradient, which K.feat_match adds at netD's last hidden activation (`dfeat`) while it
              forms feature_recon_loss = sum (real_feat - recon_feat)^2 / N from the tape in place; the real segment carries nothing
              (what the feature loss sends to netD's parameters, optim_d.zero_grad() throws away) -> K.vaegan_unpack_bwd gives the
              decoder dy = [recon_weight dX_recon | dX_fake]: its backward is linear and BatchNorm's is per segment, so one
              `segments=2` backward yields recon_weight d feat / d theta_G + d g_adv / d theta_G -> K.vaegan_latent_bwd divides the
              recon half's dz by recon_weight again and adds the KL gradient -> encoder backward -> Adam over both;
  optim_d     netD backward from the same tape with dlogit of BCE(real, 1) + BCE(fake, 0) and zero on recon -> Adam.
The reference calls `adversarial_loss` without its mode, so `loss_mode` is stored and never read: every setting computes "vanilla".
Parity with the reference is the contract.  The draws are device draws, every logged scalar stays a device tensor, nothing in the
step synchronises with the host.  A CPU tensor raises.  Under data parallelism the gradients of each optimizer's nets are
all-reduced before it steps.
"""
import torch

from ..ops import functional as K
from .base import BaseModel, ValidationResult
from .gan import SEGMENTED_NORM

LOGS = ("train_loss/reg_loss", "train_loss/feature_recon_loss", "train_loss/g_adv_loss", "train_loss/d_adv_loss", "train_log/real_logit",
        "train_log/fake_logit", "train_log/recon_logit")


class VAEGAN(BaseModel):
    def __init__(self, datamodule, encoder=None, decoder=None, latent_dim=100, lr: float = 0.0002, b1: float = 0.5, b2: float = 0.999,
                 recon_weight: float = 1e-4, loss_mode: str = "vanilla"):
        super().__init__(datamodule)
        self.save_hyperparameters()
        if not float(recon_weight) > 0:
            raise NotImplementedError("VAEGAN: recon_weight > 0 (the step sends recon_weight x the feature gradient through the decoder and "
                                      "divides it out again for the encoder; the shipped values are 1e-3 and 1e-4)")
        try:                                                    # pragma: no cover - hydra is not in this image
            from hydra.utils import instantiate
        except Exception:                                       # noqa: BLE001
            from ..runtime.config import instantiate
        self.decoder = instantiate(decoder, input_channel=latent_dim, output_channel=self.channels)
        self.encoder = instantiate(encoder, input_channel=self.channels, output_channel=2 * latent_dim)
        self.netD = instantiate(encoder, input_channel=self.channels, output_channel=1, return_features=True)
        from ..networks.basic import ConvDecoder, ConvEncoder
        nets = (self.decoder, self.encoder, self.netD)
        if (not isinstance(self.decoder, ConvDecoder) or not all(isinstance(n, ConvEncoder) for n in nets[1:])
                or any(n.norm_type != "batch" for n in nets) or (self.height, self.width) != (28, 28)):
            raise NotImplementedError("VAEGAN on the HIP path: src.networks.basic.ConvDecoder / ConvEncoder with norm_type='batch' on 28x28 "
                                      "images (configs/networks/conv_mnist.yaml); the conv32 / conv64 experiments are not built")
        for n in nets:
            n.use_fused_norm_act(SEGMENTED_NORM)
            n.reproducible = True                               # no atomics anywhere in the step: two runs give the same bits
        self.automatic_optimization = False

    # ------------------------------------------------------------------ surface
    def forward(self, z):
        output = self.decoder(z)
        return output.reshape(output.shape[0], self.channels, self.height, self.width)

    def flat_nets(self):
        return [self.decoder, self.encoder, self.netD]

    def configure_optimizers(self):
        from ..runtime.optim import FlatAdam
        hp = self.hparams
        # host_complements: 1 - beta rounded once from double, as torch's Adam takes them (csrc/elementwise.hip, adam_c_kernel)
        optim_ae = FlatAdam([self.encoder, self.decoder], lr=hp.lr, betas=(hp.b1, hp.b2), host_complements=True)
        optim_d = FlatAdam(self.netD, lr=hp.lr, betas=(hp.b1, hp.b2), host_complements=True)
        return optim_ae, optim_d

    @staticmethod
    def _on_gpu(t, what):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError(f"{what}: libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
        return t.float().contiguous()

    def _draw(self, t, N, what):
        L = int(self.hparams.latent_dim)
        if t is None:
            return torch.randn(N, L, device=self.device)
        t = self._on_gpu(t, what)
        if t.shape != (N, L):
            raise RuntimeError(f"{what}: [{N}, {L}] expected, got {tuple(t.shape)}")
        return t

    def vae(self, imgs, eps=None, prior_z=None):
        """(mu, log_sigma, z, recon_imgs, fake_imgs): vae_gan.py:56-61 and a decode of a prior draw in the same decoder pass.  Inference
        only -- training goes through training_step."""
        imgs = self._on_gpu(imgs, "images")
        N, L = imgs.shape[0], int(self.hparams.latent_dim)
        with torch.no_grad():
            h, _ = self.encoder.forward_nhwc(K.nchw_to_nhwc(imgs), record=False)
            zz, _ = K.vaegan_latent_fwd(h, self._draw(eps, N, "eps"), self._draw(prior_z, N, "prior_z"))
            out, _ = self.decoder.forward_nhwc(zz, record=False, segments=2)
            both = K.nhwc_to_nchw(out)
            hr = h.reshape(N, 2 * L)
            return hr[:, :L], hr[:, L:], zz[:N].reshape(N, L), both[:N], both[N:]

    def sample(self, N: int):
        with torch.no_grad():
            return self.forward(torch.randn(N, int(self.hparams.latent_dim), device=self.device))

    def _sync(self, nets):
        from ..runtime.ddp import allreduce_flat_grads
        allreduce_flat_grads(list(nets))

    # ------------------------------------------------------------------ training
    def training_step(self, batch, batch_idx, eps=None, prior_z=None):
        imgs, _ = batch  # (N, C, H, W)
        imgs = self._on_gpu(imgs, "images")
        N, rw = imgs.shape[0], float(self.hparams.recon_weight)
        eps, prior_z = self._draw(eps, N, "eps"), self._draw(prior_z, N, "prior_z")
        E, G, D = self.encoder, self.decoder, self.netD
        optim_ae, optim_d = self.optimizers()

        # ---- forward (vae_gan.py:69-81)
        h, tape_e = E.forward_nhwc(K.nchw_to_nhwc(imgs), record=True)             # [N, 1, 1, 2 L] = [mu | log_sigma]
        zz, reg_loss = K.vaegan_latent_fwd(h, eps, prior_z)                        # [z | prior_z]
        out, tape_g = G.forward_nhwc(zz, record=True, segments=2)                  # [recon | fake]
        pred, tape_d = D.forward_nhwc(K.vaegan_pack_fwd(out, imgs), record=True, segments=3)       # [fake | imgs | recon]
        dl = torch.zeros((2, 3 * N, 1, 1, 4), device=imgs.device, dtype=torch.float32)
        dl_ae, dl_d = dl[0][..., :1], dl[1][..., :1]
        g_adv, _, _ = K.adv_loss(pred[:N], [True], "vanilla", dlogit_out=dl_ae[:N])
        d_adv, mean_logit, _ = K.adv_loss(pred[:2 * N], [False, True], "vanilla", dlogit_out=dl_d[:2 * N])
        _, recon_logit, _ = K.adv_loss(pred[2 * N:], [True], "vanilla", want_grad=False)

        # ---- optim_ae (vae_gan.py:83-89)
        feat, box = D.features_nhwc(tape_d), {}

        def feature_gradient(g):
            box["loss"], _ = K.feat_match(feat[N:2 * N], feat[2 * N:], drecon=g[2 * N:], accumulate=True)
        dx = D.backward_nhwc(tape_d, dl_ae, need_dx=True, param_grads=False, dfeat=feature_gradient)
        dzz = G.backward_nhwc(tape_g, K.vaegan_unpack_bwd(dx, s_recon=rw, s_fake=1.0), need_dx=True, own_dy=True)
        E.backward_nhwc(tape_e, K.vaegan_latent_bwd(h, eps, dzz, g_kld=1.0, dz_scale=1.0 / rw), need_dx=False)
        self._sync([E, G])
        optim_ae.step()

        # ---- optim_d (vae_gan.py:91-94): the same forward, which ran before optim_ae stepped
        D.backward_nhwc(tape_d, dl_d, need_dx=False)
        self._sync([D])
        optim_d.step()

        self.log("train_loss/reg_loss", reg_loss)
        self.log("train_loss/feature_recon_loss", box["loss"])
        self.log("train_loss/g_adv_loss", g_adv[0])
        self.log("train_loss/d_adv_loss", d_adv[1] + d_adv[0])
        self.log("train_log/real_logit", mean_logit[1])
        self.log("train_log/fake_logit", mean_logit[0])
        self.log("train_log/recon_logit", recon_logit[0])

    def validation_step(self, batch, batch_idx):
        imgs, labels = batch
        mu, log_sigma, z, recon_imgs, fake_imgs = self.vae(imgs)
        with torch.no_grad():
            val_mse, _ = K.age_image_mse(K.nchw_to_nhwc(recon_imgs), imgs.float().contiguous(), want_grad=False)
        self.log("val_log/van_mse", val_mse)
        return ValidationResult(real_image=imgs, fake_image=fake_imgs, recon_image=recon_imgs, label=labels, encode_latent=z)
