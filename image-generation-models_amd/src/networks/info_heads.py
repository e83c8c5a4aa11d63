"""The InfoGAN's two heads on the shared feature (reference src/models/info_gan.py:37-43) on the kernels of csrc/info_head.hip:
  InfoDHead(encode_dim)            nn.Sequential(LeakyReLU(), Linear(encode_dim, 1))
  InfoQHead(encode_dim, out_dim)   nn.Sequential(LeakyReLU(), Linear(encode_dim, 128), LeakyReLU(), Linear(128, out_dim))
with the Sequential's parameter names (`1.weight`, `1.bias`, `3.weight`, `3.bias`), construction order and seeded default init.  The
LeakyReLUs have torch's default slope 0.01.  Both are fp32 in every compute mode: they are launch-bound, not arithmetic-bound.
The training step calls K.info_head_fwd / K.info_head_bwd on both heads at once (src/models/info_gan.py); `forward(x)` gives what
the reference's module gives, for a device tensor.
"""
import torch

from ..models.ddpm import _Entry
from ..ops import functional as K
from .flatnet import FlatNet


class _InfoHead(FlatNet):
    BF16_SHADOWS = False

    def _linear_params(self, pre, i, o):
        """nn.Linear: weight logical [out, in] stored input-major, torch's seeded default init (as MLPEncoder._linear_params)."""
        self._entries.append(_Entry(pre + "weight", (o, i), "linear", "kaiming", i, 0))
        self._entries.append(_Entry(pre + "bias", (o,), "plain", "ubias", i, 0))

    def _features(self, x):
        if not (torch.is_tensor(x) and x.is_cuda):
            raise RuntimeError("libmi_ddpm kernels need tensors on an MI355X (HIP) device; there is no CPU fallback")
        x = x.float().contiguous()
        if x.dim() != 2 or x.shape[1] != self.encode_dim:
            raise RuntimeError(f"features [N, {self.encode_dim}] expected, got {tuple(x.shape)}")
        return x

    def tensors(self, views=None):
        views = self._sv if views is None else views
        return [views[k] for k in self.KEYS]

    def grad_tensors(self):
        self.flat_grads
        return self.tensors(self._gv)


class InfoDHead(_InfoHead):
    KEYS = ("1.weight", "1.bias")

    def __init__(self, encode_dim):
        super().__init__()
        self.encode_dim = int(encode_dim)
        if not K.info_head_shape_ok(self.encode_dim):
            raise NotImplementedError(f"encode_dim={encode_dim}: the head kernels take a multiple of 4 in [4, 4096]")
        self._linear_params("1.", self.encode_dim, 1)
        self._finish()

    def forward(self, x):
        x = self._features(x)
        w, b = self.tensors()
        return K.info_head_fwd(x, [w.view(-1), b, None, None, None, None], [True])["logit"].view(-1, 1)


class InfoQHead(_InfoHead):
    KEYS = ("1.weight", "1.bias", "3.weight", "3.bias")

    def __init__(self, encode_dim, out_dim):
        super().__init__()
        self.encode_dim, self.out_dim = int(encode_dim), int(out_dim)
        if not K.info_head_shape_ok(self.encode_dim) or not 2 <= self.out_dim <= 64:
            raise NotImplementedError(f"encode_dim={encode_dim}, out_dim={out_dim}: the head kernels take encode_dim a multiple of 4 in "
                                      "[4, 4096] and at most 64 outputs")
        self._linear_params("1.", self.encode_dim, K.INFO_HEAD_H)
        self._linear_params("3.", K.INFO_HEAD_H, self.out_dim)
        self._finish()

    def forward(self, x):
        """q [N, out_dim]: the Q head alone, one launch (K.info_q_fwd)."""
        return K.info_q_fwd(self._features(x), self.tensors())
