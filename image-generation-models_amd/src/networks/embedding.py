"""`nn.Embedding(n_classes, dim)` as a `FlatNet`: the table is one more flat fp32 buffer for `FlatAdam`, its parameter is registered
as `weight` (state_dict key `<name>.weight`) and drawn N(0, 1) like torch's.  The cVAE's latent kernels read the table and accumulate
its gradient in place (src/models/cvae.py); `forward(labels)` is the plain lookup.
"""
import torch

from ..models.ddpm import _Entry
from ..ops import functional as K
from .flatnet import FlatNet


class ClassEmbedding(FlatNet):
    BF16_SHADOWS = False

    def __init__(self, num_embeddings, embedding_dim):
        super().__init__()
        self.num_embeddings, self.embedding_dim = int(num_embeddings), int(embedding_dim)
        self._entries.append(_Entry("weight", (self.num_embeddings, self.embedding_dim), "plain", "normal", 0, 0))
        self._finish()

    @property
    def table(self) -> torch.Tensor:
        """[num_embeddings, embedding_dim] view of the flat parameter buffer (what the kernels read)."""
        return self._sv["weight"]

    def grad_table(self) -> torch.Tensor:
        """The matching view of the flat gradient buffer, zeroed unless gradients are being accumulated (the kernels add into it)."""
        return self._begin_backward()["weight"]

    def forward(self, labels):
        """Rows of the table for int64 labels on the table's device (inference only; a label out of range gives a zero row)."""
        z = torch.zeros((labels.shape[0], self.embedding_dim), device=self._flat.device)
        zc, _ = K.cvae_latent_fwd(None, z, labels, self.table)
        return zc[:, self.embedding_dim:]
