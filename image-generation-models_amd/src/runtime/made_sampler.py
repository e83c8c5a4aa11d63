"""hipGraph-replayed MADE sampler (PixelSampler's pattern, src/runtime/pixelcnn_sampler.py).

One step = the hidden stack on the current image (-1 marks a pixel not yet filled, as in the reference), the 256*C head rows of
the C units at raster position (h, w) only (mi_made_head_rows, which reads the position from a device counter), and
mi_made_sample_step, which draws, writes the image in place and advances the counter.  The step is captured once over static
buffers and replayed H*W times with no host synchronisation in the loop.  The uniforms of the whole run are drawn up front with
the device Philox generator, one launch into a static buffer; `model.uniform_source(shape, device)` replaces them with a tape.
The draws differ from the reference's `torch.multinomial` but follow the same distribution (k = min{k : cdf_k > u} under the
fp32 softmax).  For C > 1 the order is the reference's: position by position, all channels at once."""
from __future__ import annotations

import torch

from ..ops import functional as K


class MADESampler:
    def __init__(self, model, shape):
        self.model, self.shape = model, tuple(shape)
        N, Cc, H, W = self.shape
        dev = model.flat_params.device
        self.img = torch.full(self.shape, -1.0, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.uniforms = torch.zeros((H * W, N * Cc), device=dev)
        self.logits = torch.zeros((N, 256 * Cc), device=dev)
        self.graph = None
        self._key = None

    def _iteration(self):
        m = self.model
        N, Cc, H, W = self.shape
        acts = m._hidden(self.img.view(N, -1))
        w, b = m._wb(m.n_layer)
        din, dout = m._deg[m.n_layer]
        K.made_head_rows(acts[-1], w, b, din, dout, self.counter, Cc, H * W, self.logits, mode=m._mode())
        K.made_sample_step(self.logits, self.counter, self.uniforms, self.img, m.input_normalize)

    def _capture(self):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                      # warm-up outside capture (allocator, lazy init)
            self.counter.zero_()
            self._iteration()
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._iteration()
        m = self.model
        self._key = (m.flat_params.data_ptr(), m.compute_mode, id(m._deg))

    @torch.no_grad()
    def run(self, img=None, record=None):
        m = self.model
        N, Cc, H, W = self.shape
        if self.graph is None or self._key != (m.flat_params.data_ptr(), m.compute_mode, id(m._deg)):
            self._capture()
        if img is None:
            self.img.fill_(-1.0)
        else:
            self.img.copy_(img)
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
