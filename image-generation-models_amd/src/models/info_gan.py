"""`InfoGAN` (https://arxiv.org/abs/1606.03657) with the reference's surface (src/models/info_gan.py:11-169) on the HIP kernels --
`experiment=infogan/mnist`.

Same constructor and defaults, attribute names (`netG`, `common_layer`, `netD`, `netQ`), construction order (the seeded default weights
are the reference's), `state_dict` keys (`netD.1.*`, `netQ.1.*`, `netQ.3.*`), `encode`, `decode`, two Adam optimizers -- `opt_g` a
`FlatAdam` over netG and netQ with a learning rate each (lrG, lrQ: the reference's two parameter groups), `opt_d` over netD and
common_layer at lrD --, the six logged keys and `on_train_epoch_end`'s four image grids.  `forward(z_full)`, `sample(N)` and
`validation_step` are added.  The conv nets are the 28x28 `ConvDecoder` / `ConvEncoder` with BatchNorm (configs/networks/conv_mnist.yaml)
on their segmented BatchNorm + activation path (csrc/bn_seg.hip); the two heads, the mutual-information loss and the structured
generator input [one-hot codes | continuous codes | noise] are csrc/info_head.hip.  MLP and conv32 / conv64 nets are not built (the
reference ships no such InfoGAN config).

The generator's input holds the one-hot of code d with value v at column v * discrete_dim + d (the reference flattens a [N, V, Dd]
tensor), and netQ's first Dd * V outputs have the same layout.  The heads' LeakyReLUs have torch's default slope 0.01, not the conv
nets' 0.2.  `continuous_dim >= 1` is required (the reference's `[:, :-0]` is empty).

`loss_mode` is stored and NEVER USED, as in the reference: both of its phases call adversarial_loss(...) without it, so the loss is
always binary cross-entropy with logits ("vanilla") -- `experiment=infogan/mnist` sets "lsgan" and computes exactly what "vanilla"
computes (tools/gen_golden_infogan.py asserts it on the reference).  Parity with the reference is the contract.

The reference runs under Lightning's automatic optimization with two optimizers: per batch, optimizer 0 then optimizer 1, each with
its own training_step(..., optimizer_idx) -> zero_grad -> backward -> step.  Here optimization is manual and
`training_step(batch, batch_idx, optimizer_idx=None, latents=None)` runs both phases (`optimizer_idx` 0 or 1: that phase alone), without
recording an autograd graph:
  phase 0  generator + Q   latent draw -> G forward -> common_layer forward on the fake in training mode (its running
                           statistics update, as in the reference) -> both heads, BCE against "real", cross-entropy of the Dd
                           softmaxes and MSE of the continuous codes -> heads backward (Q gradients, feature gradient) -> common_layer
                           backward for the input gradient alone -> G backward -> Adam on netG (lrG) and netQ (lrQ);
  phase 1  discriminator   a NEW latent draw -> G forward in training mode without a tape (the G phase 0 just updated) -> common_layer
                           on [imgs | fake] as ONE pass of N + N rows with `segments=2`, real first -> D head, targets [real, fake],
                           d_loss = (real + fake) / 2 -> D-head gradients and feature gradient -> common_layer backward with
                           parameter gradients -> Adam on netD and common_layer (lrD).  netQ does not run.
`latents = ((dis_c_index, cont_c, z) for phase 0, (dis_c_index, cont_c, z) for phase 1)` injects the draws (a single triple when one
phase is asked for); otherwise they are torch.randint / uniform_(-1, 1) / randn on the device.  Every logged scalar stays a device
tensor, nothing in the step synchronises with the host.  A CPU tensor raises.  A discrete index outside [0, discrete_value) is not
detected (that would need a host synchronisation): its code's one-hot columns are all zero.
"""
import torch

from ..ops import functional as K
from .base import BaseModel, ValidationResult
from .gan import SEGMENTED_NORM, _base


class InfoGAN(BaseModel):
    def __init__(self, datamodule, netG=None, netD=None, lambda_I=1, discrete_dim=1, discrete_value=10, continuous_dim=2, noise_dim=62,
                 encode_dim=1024, loss_mode="vanilla", lrG: float = 0.001, lrD: float = 0.0002, lrQ: float = 0.0002, b1: float = 0.5,
                 b2: float = 0.999):
        super().__init__(datamodule)
        self.save_hyperparameters()
        if loss_mode not in K.ADV_LOSSES:
            raise NotImplementedError(f"loss_mode={loss_mode!r}: 'vanilla', 'lsgan' and 'hinge' are accepted (and all compute 'vanilla', as the "
                                      "reference does)")
        if int(discrete_dim) < 1 or int(discrete_value) < 1 or int(continuous_dim) < 1 or int(noise_dim) < 0:
            raise NotImplementedError("InfoGAN: discrete_dim, discrete_value and continuous_dim of at least 1 (the reference's slice "
                                      "[:, :-continuous_dim] is empty for 0) and noise_dim >= 0")
        try:                                                    # pragma: no cover - hydra is not in this image
            from hydra.utils import instantiate
        except Exception:                                       # noqa: BLE001
            from ..runtime.config import instantiate
        from ..networks.basic import ConvDecoder, ConvEncoder
        from ..networks.info_heads import InfoDHead, InfoQHead
        self.code_dim = int(discrete_dim) * int(discrete_value) + int(continuous_dim)
        self.latent_dim = self.code_dim + int(noise_dim)
        self.netG = instantiate(netG, input_channel=self.latent_dim, output_channel=self.channels)
        self.common_layer = instantiate(netD, input_channel=self.channels, output_channel=encode_dim)
        if (not isinstance(self.netG, ConvDecoder) or not isinstance(self.common_layer, ConvEncoder) or self.netG.norm_type != "batch"
                or self.common_layer.norm_type != "batch" or (self.height, self.width) != (28, 28)):
            raise NotImplementedError("InfoGAN on the HIP path: src.networks.basic.ConvDecoder / ConvEncoder with norm_type='batch' on "
                                      "28x28 images (configs/networks/conv_mnist.yaml); MLP and conv32 / conv64 nets are not built")
        self.netD = InfoDHead(encode_dim)
        self.netQ = InfoQHead(encode_dim, self.code_dim)
        self.netG.use_fused_norm_act(SEGMENTED_NORM)
        self.common_layer.use_fused_norm_act(SEGMENTED_NORM)
        self.netG.reproducible = self.common_layer.reproducible = True      # no atomics anywhere in the step: two runs give the same bits
        self.automatic_optimization = False

    # ------------------------------------------------------------------ surface
    def flat_nets(self):
        return [self.netG, self.common_layer, self.netD, self.netQ]

    def configure_optimizers(self):
        from ..runtime.optim import FlatAdam
        hp = self.hparams
        opt_g = FlatAdam([self.netG, self.netQ], lr=[hp.lrG, hp.lrQ], betas=(hp.b1, hp.b2))
        opt_d = FlatAdam([self.netD, self.common_layer], lr=hp.lrD, betas=(hp.b1, hp.b2))
        return [opt_g, opt_d]

    def forward(self, z_full):
        """The generator on a full latent row [N, latent_dim] = [one-hot codes | continuous codes | noise]."""
        output = self.netG(z_full)
        return output.reshape(z_full.shape[0], self.channels, self.height, self.width)

    @staticmethod
    def _on_gpu(t, what, dtype=torch.float32):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError(f"{what}: libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
        return t.to(dtype).contiguous()

    def _latents(self, N, dis_c_index=None, cont_c=None, z=None):
        """The three draws of the reference's decode (info_gan.py:81-90), on the device; given ones are checked."""
        hp, dev = self.hparams, self.device
        Dd, V, Cc, Nz = int(hp.discrete_dim), int(hp.discrete_value), int(hp.continuous_dim), int(hp.noise_dim)
        if dis_c_index is None:
            dis_c_index = torch.randint(0, V, (N, Dd), device=dev)
        if cont_c is None:
            cont_c = torch.zeros(N, Cc, device=dev).uniform_(-1, 1)
        if z is None:
            z = torch.randn(N, Nz, device=dev)
        dis_c_index = self._on_gpu(dis_c_index, "dis_c_index", torch.int64)
        cont_c, z = self._on_gpu(cont_c, "cont_c"), self._on_gpu(z, "z")
        if dis_c_index.dim() == 2 and dis_c_index.shape == (N, 1) and Dd > 1:
            # the reference scatters an index [N, 1] into its [N, V, Dd] one-hot: code 0 alone is set, the others stay all zero
            dis_c_index = torch.cat([dis_c_index, dis_c_index.new_full((N, Dd - 1), -1)], dim=1)
        if dis_c_index.shape != (N, Dd) or cont_c.shape != (N, Cc) or z.shape != (N, Nz):
            raise RuntimeError(f"latents: dis_c_index [{N}, {Dd}], cont_c [{N}, {Cc}] and z [{N}, {Nz}] expected, got "
                               f"{tuple(dis_c_index.shape)}, {tuple(cont_c.shape)}, {tuple(z.shape)}")
        return dis_c_index, cont_c, z

    def decode(self, N, dis_c_index=None, cont_c=None, z=None, return_latents=False):
        """[N, C, H, W] from the given or drawn latents, in whatever mode the module is in (training mode updates G's running
        statistics, as in the reference)."""
        dis_c_index, cont_c, z = self._latents(N, dis_c_index, cont_c, z)
        with torch.no_grad():
            fake, _ = self.netG.forward_nhwc(K.info_latent(dis_c_index, cont_c, z, int(self.hparams.discrete_value)), record=False)
            output = K.nhwc_to_nchw(fake).reshape(N, self.channels, self.height, self.width)
        if return_latents:
            return output, (dis_c_index, cont_c, z)
        return output

    def encode(self, x, return_posterior=False):
        """adv_logit [N, 1], and with return_posterior the discrete logits [N, V, Dd] and the continuous codes [N, Cc]."""
        hp = self.hparams
        x = self._on_gpu(x, "images")
        with torch.no_grad():
            feat, _ = self.common_layer.forward_nhwc(K.nchw_to_nhwc(x), record=False)
            feat = feat.reshape(x.shape[0], -1)
            adv_logit = self.netD(feat)
            if not return_posterior:
                return adv_logit
            output = self.netQ(feat)
        Cc = int(hp.continuous_dim)
        return adv_logit, output[:, :-Cc].reshape(-1, int(hp.discrete_value), int(hp.discrete_dim)), output[:, -Cc:]

    def sample(self, N: int):
        return self.decode(N)

    def validation_step(self, batch, batch_idx):
        img, _ = batch
        return ValidationResult(real_image=img, fake_image=self.decode(img.shape[0]))

    def _sync(self, *nets):
        from ..runtime.ddp import allreduce_flat_grads
        for n in nets:
            allreduce_flat_grads([n])

    def _head_params(self, with_q):
        wd, bd = self.netD.tensors()
        return [wd.view(-1), bd] + (self.netQ.tensors() if with_q else [None] * 4)

    # ------------------------------------------------------------------ training
    def training_step(self, batch, batch_idx, optimizer_idx=None, latents=None):
        if optimizer_idx not in (None, 0, 1):
            raise ValueError(f"optimizer_idx={optimizer_idx!r}: None (both phases), 0 or 1")
        imgs, _ = batch  # (N, C, H, W)
        imgs = self._on_gpu(imgs, "images")
        N = imgs.shape[0]
        if latents is None:
            latents = ((None, None, None), (None, None, None))
        elif optimizer_idx is not None and len(latents) == 3:
            latents = (latents, latents)
        if optimizer_idx in (None, 0):
            self._generator_phase(N, self._latents(N, *latents[0]))
        if optimizer_idx in (None, 1):
            self._discriminator_phase(imgs, self._latents(N, *latents[1]))

    def _generator_phase(self, N, draws):
        """info_gan.py:104-118."""
        hp, G, Cm, Q = self.hparams, self.netG, self.common_layer, self.netQ
        idx, cont, z = draws
        opt_g, _ = self.optimizers()
        fake, tape_g = G.forward_nhwc(K.info_latent(idx, cont, z, int(hp.discrete_value)), record=True)
        feat, tape_c = Cm.forward_nhwc(fake, record=True)
        params = self._head_params(True)
        rec = K.info_head_fwd(feat, params, [True], codes=(idx, cont, int(hp.discrete_value)), lambda_I=float(hp.lambda_I))
        df = K.info_head_bwd(params, rec, grads=[None, None] + Q.grad_tensors())
        dfake = Cm.backward_nhwc(tape_c, df, need_dx=True, param_grads=False)
        G.backward_nhwc(tape_g, dfake[..., :self.channels])
        self._sync(G, Q)
        opt_g.step()
        self.log("train_loss/g_loss", rec["loss"][0])
        self.log("train_loss/I_discrete_loss", rec["I_disc"])
        self.log("train_loss/I_continuous", rec["I_cont"])

    def _discriminator_phase(self, imgs, draws):
        """info_gan.py:120-133."""
        hp, G, Cm, D = self.hparams, self.netG, self.common_layer, self.netD
        idx, cont, z = draws
        _, opt_d = self.optimizers()
        fake, _ = G.forward_nhwc(K.info_latent(idx, cont, z, int(hp.discrete_value)), record=False)   # detached in the reference (:124)
        x = torch.cat([_base(K.nchw_to_nhwc(imgs)), _base(fake)])[..., :self.channels]     # real first: the reference's order of calls
        feat, tape = Cm.forward_nhwc(x, record=True, segments=2)
        params = self._head_params(False)
        rec = K.info_head_fwd(feat, params, [True, False], scale=0.5)
        df = K.info_head_bwd(params, rec, grads=D.grad_tensors() + [None] * 4)
        Cm.backward_nhwc(tape, df, need_dx=False)
        self._sync(D, Cm)
        opt_d.step()
        self.log("train_loss/d_loss", (rec["loss"][0] + rec["loss"][1]) / 2)
        self.log("train_log/pred_real", rec["mean_logit"][0])
        self.log("train_log/pred_fake", rec["mean_logit"][1])

    # ------------------------------------------------------------------ the reference's image grids (info_gan.py:135-169)
    def _image_logger(self):
        trainer = getattr(self, "trainer", None)
        logger = getattr(trainer, "logger", None) if trainer is not None else None
        experiment = getattr(logger, "experiment", None)
        return experiment if hasattr(experiment, "add_image") else None

    def on_train_epoch_end(self) -> None:
        """The sample grid, the traverse over the discrete values and the traverses over the first two continuous codes, logged with
        `logger.experiment.add_image`; nothing when the logger has no such method.  decode runs in the module's mode: at the end of a
        training epoch that is training mode, so the four decodes move G's running statistics, as in the reference.  Under data
        parallelism every rank decodes (the BatchNorm counters stay in step across ranks) and rank 0 alone builds and logs the grids."""
        experiment = self._image_logger()
        if experiment is None:
            return
        from ..callbacks.visualization import get_grid_images
        step = int(getattr(self.trainer, "current_epoch", 0))
        dev = self.device
        logs = bool(getattr(self.trainer, "is_global_zero", True))

        def add(name, imgs, nimgs, nrow):
            if logs:
                experiment.add_image(name, get_grid_images(imgs, self, nimgs, nrow), global_step=step)
        add("images/sample", self.decode(64), 64, 8)

        N = 8  # rows of images
        a, b, c = int(self.hparams.discrete_value), int(self.hparams.continuous_dim), int(self.hparams.noise_dim)
        disc_c = torch.arange(a).reshape(1, a).repeat(N, 1).reshape(N * a, 1).to(dev)
        cont_c = torch.randn(N, 1, b).repeat(1, a, 1).reshape(N * a, b).to(dev)
        z = torch.randn(N, 1, c).repeat(1, a, 1).reshape(N * a, c).to(dev)
        imgs = self.decode(N * a, disc_c, cont_c, z)
        add("visual/traverse over discrete values", imgs, N * a, a)

        col = 10
        disc_c = torch.randint(low=0, high=a, size=(N, 1)).repeat(1, col).reshape(N * col, 1).to(dev)
        variation = torch.linspace(-2, 2, col).reshape(1, col).repeat(N, 1).reshape(N * col).to(dev)
        cont_c = torch.randn(N, 1, b).repeat(1, col, 1).reshape(N * col, b).to(dev)
        z = torch.randn(N, 1, c).repeat(1, col, 1).reshape(N * col, c).to(dev)
        for i, name in ((0, "first"), (1, "second")):
            cont_c_mix = cont_c.clone()
            cont_c_mix[:, i] = variation
            imgs = self.decode(N * col, disc_c, cont_c_mix, z)
            add(f"visual/traverse over {name} continuous values", imgs, N * col, col)
