"""`LayerNormMLPEncoder`: the reference's MLPEncoder (src/networks/basic.py:64-112) with `norm_type="layer"`, in the one shape the
adversarial autoencoder's latent discriminator builds (src/models/aae.py:42-44), on the row-local kernels of csrc/latent_disc_ln.hip:
    Linear(C*w*h, 256) -> GroupNorm(1, 256) -> LeakyReLU(0.2) -> Linear(256, 256) -> GroupNorm(1, 256) -> LeakyReLU(0.2) -> Linear(256, 1).
`src.networks.basic.MLPEncoder` stays the BatchNorm1d network of the FactorVAE and keeps refusing `norm_type="layer"`; this is a class of
its own because nothing here depends on the batch: no buffers, N = 1 is legal, and two batches with a target each go through as one pass.
"""
from ..ops import functional as K
from .basic import MLPEncoder
from .flatnet import FlatNet


class LayerNormMLPEncoder(FlatNet):
    """Same constructor as the reference's MLPEncoder, the ten parameter names `model.0.fc.weight` ... `classifier.fc.bias`, no buffers,
    the reference's construction order and seeded default init.  Only `norm_type="layer"`, `hidden_dims=[256, 256]`,
    `output_channel=1`, at most 64 input features, `dropout=0` and the identity output are built; anything else raises
    NotImplementedError.  fp32 in every compute mode.  `disc_forward` / `disc_backward` are what a training step calls (no autograd
    graph); `forward(x)` gives the logits alone."""
    KEYS = MLPEncoder.KEYS
    BF16_SHADOWS = False

    def __init__(self, input_channel, output_channel, hidden_dims, width, height, dropout=0, norm_type="batch", return_features=False,
                 output_act="identity"):
        super().__init__()
        hidden_dims = [int(h) for h in hidden_dims]
        in_features = int(input_channel) * int(width) * int(height)
        if (hidden_dims != [K.LATENT_DISC_H] * 2 or int(output_channel) != 1 or dropout != 0 or norm_type != "layer" or return_features
                or output_act != "identity" or not 1 <= in_features <= 64):
            raise NotImplementedError("LayerNormMLPEncoder on the HIP path: hidden_dims=[256, 256], output_channel=1, at most 64 input "
                                      "features, dropout=0, norm_type='layer', return_features=False, output_act='identity'")
        self.input_channel, self.output_channel, self.in_features, self.return_features = input_channel, output_channel, in_features, False
        dims = [in_features] + hidden_dims
        for i in range(2):
            self._linear_params(f"model.{i}.fc.", dims[i], dims[i + 1])
            self._norm_params(f"model.{i}.norm.", dims[i + 1])            # GroupNorm(1, C): no buffers, no random draw
        self._linear_params("classifier.fc.", dims[2], 1)
        self._finish()

    _linear_params = MLPEncoder._linear_params

    def _tensors(self, views):
        return [views[k] for k in self.KEYS]

    def disc_forward(self, x0, target0, x1=None, target1=0.0, loss_mode="vanilla"):
        """One pass over the rows of x0 (against target0) and, when given, of x1 (against target1): K.latent_disc_ln_fwd's record."""
        return K.latent_disc_ln_fwd(self._tensors(self._sv), x0, target0, x1=x1, target1=target1, loss_mode=loss_mode)

    def disc_backward(self, rec, target0, target1=0.0, c0=1.0, c1=0.0, param_grads=True, accumulate=False, scale=1.0, dx0=None, dx_scale=1.0,
                      accumulate_dx=False):
        """Gradients of c0 loss0 + c1 loss1 from a `disc_forward` record.  param_grads: into the flat gradient buffer, stored
        (accumulate=False: every gradient element is written, nothing needs zeroing) or added; dx0: see K.latent_disc_ln_bwd."""
        grads = None
        if param_grads:
            self.flat_grads
            grads = self._tensors(self._gv)
        return K.latent_disc_ln_bwd(self._tensors(self._sv), rec, target0, target1, c0=c0, c1=c1, grads=grads, param_scale=scale,
                                    accumulate_params=accumulate, dx0=dx0, dx_scale=dx_scale, accumulate_dx=accumulate_dx)

    def forward(self, x):
        n = x.shape[0]
        x = x.reshape(n, -1)
        if not x.is_cuda:
            raise RuntimeError("libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
        return self.disc_forward(x.float().contiguous(), 0.0)["logit"].view(n, 1)
