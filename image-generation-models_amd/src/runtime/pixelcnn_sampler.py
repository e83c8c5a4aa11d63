"""hipGraph-replayed PixelCNN sampler (the DDPM sampler's pattern, src/runtime/sampler.py).

One pixel step = the full-image network forward + mi_pcnn_sample_step, which reads the pixel index from a device counter, writes
the drawn value into both the NCHW image and the NHWC network input, and advances the counter.  The step is captured once over
static buffers and replayed H*W times with no host synchronisation in the loop.  The uniforms of the whole run are drawn up front
with the device Philox generator, one launch into a static buffer; `model.uniform_source(shape, device)` (parity runs) replaces
them with a tape.  Restricting the forward to rows <= h is not done: the replay is one graph for every pixel."""
from __future__ import annotations

import torch

from ..ops import functional as K


class PixelSampler:
    def __init__(self, model, shape, cond_like=None):
        self.model, self.shape = model, tuple(shape)
        N, Cc, H, W = self.shape
        dev = model.flat_params.device
        self.img = torch.full(self.shape, -1.0, device=dev)
        self.xin = torch.zeros((N, H, W, Cc), device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.uniforms = torch.zeros((H * W, N * Cc), device=dev)
        # conditioning: int64 labels [N] or a float one-hot [N, n_classes], in a static buffer the captured step reads
        self.cond = None if cond_like is None else torch.zeros(cond_like.shape, dtype=cond_like.dtype, device=dev)
        self.graph = None
        self._key = None

    def _iteration(self):
        m = self.model
        h, _, _ = m._forward_nhwc(self.xin, self.cond, record=False)
        K.pcnn_sample_step(h, m._w("conv_out.weight"), m._w("conv_out.bias"), self.counter, self.uniforms, self.img, self.xin,
                           m.input_normalize)

    def _capture(self):
        self.model._apply_masks()                       # eager, before capture: the captured step only reads the weights
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                      # warm-up outside capture (allocator, lazy init)
            self.counter.zero_()
            self._iteration()
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._iteration()
        self._key = self.model.flat_params.data_ptr()

    @torch.no_grad()
    def run(self, img=None, cond=None, record=None):
        m = self.model
        N, Cc, H, W = self.shape
        if self.cond is not None:
            self.cond.copy_(cond)
        if self.graph is None or self._key != m.flat_params.data_ptr():
            self._capture()
        else:
            m._apply_masks()
        if img is None:
            self.img.fill_(-1.0)
        else:
            self.img.copy_(img)
        self.xin.copy_(K.nchw_to_nhwc(self.img))
        self.counter.zero_()
        if m.uniform_source is None:
            self.uniforms.uniform_()                   # every draw of the run, one Philox launch
        else:
            self.uniforms.copy_(m.uniform_source((H * W, N * Cc), self.img.device))
        for _ in range(H * W):
            self.graph.replay()
            if record is not None:
                record.append(self.img.clone())
        return self.img.clone()
