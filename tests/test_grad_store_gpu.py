"""Unet.backward_nhwc in store mode (MI_DDPM_GRAD_STORE, the default): the weight gradients of the convs with Ci % 64 == 0 and Cj >= 32
are WRITTEN by their one writer and the rest of flat_grads is zero-filled by one mi_zero_ranges launch.  The dim-32 / 1-2-4 UNet in
three configurations:
  * fp32 mode, B = 4, 16x16 (tests/golden/mid_unet.npz): the 64- and 128-channel layers at 16x16 and 8x8 take the batched exact-fp32
    kernels in store mode; the 4x4 level and every stride-2 layer take kernels that can only add (their range is filled first);
  * bf16 mode, B = 4, 16x16 (the same golden batch): at B % 8 != 0 the model keeps no bf16 copies of its activations, so EVERY stored
    weight takes the adding fallbacks -- the fill in front of each of them is what this configuration tests;
  * bf16 mode, B = 8, 32x32, random batch: the benchmark's path -- Unet.backward_nhwc -> WgradQueue -> the bf16 3x3, 1x1 and stride-2
    (Downsample 64 ch 16 -> 8, Upsample 64 ch 8 -> 16) batched kernels with MI_WGRAD_STORE; at least 15 stored weights, those two among
    them, must take the batched kernels.

flat_grads is NaN before every backward pass: one element nobody wrote, or one read before it was written (a `+=` where a `=` belongs),
is a NaN in the result."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _util import rel_err  # noqa: E402
from test_runtime_gpu import _graph_node_types  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GTOL = {"fp32": 2e-3, "bf16": 1.8e-1}        # worst per-parameter rel-L2 against the golden gradients: tests/test_unet_gpu.py::test_mid_unet_golden


def _t(a):
    return torch.from_numpy(np.asarray(a))


CFGS = [("fp32", 4, 16), ("bf16", 4, 16), ("bf16", 8, 32)]          # (compute mode, batch, image size)
cfgs = pytest.mark.parametrize("cfg", CFGS, ids=[f"{m}-b{b}-{s}" for m, b, s in CFGS])
S2_KEYS = ("downs.1.3.conv.weight", "ups.0.3.conv.weight")             # the stored Downsample / Upsample weights (64 channels)


def _setup(golden_dir, cfg):
    """-> (golden gradients or None, net, diffusion, (x, t, noise))"""
    from src.models.ddpm import GaussianDiffusion, Unet
    mode, B, size = cfg
    torch.manual_seed(0)
    net = Unet(dim=32, dim_mults=(1, 2, 4), channels=3)
    net.compute_mode = mode
    net = net.to(DEV).train()
    gd = GaussianDiffusion(net, image_size=(size, size), timesteps=1000).to(DEV)
    if (B, size) == (4, 16):
        g = dict(np.load(os.path.join(golden_dir, "mid_unet.npz")))
        x, t, noise = _t(g["x"]), _t(g["t"]), _t(g["noise"])
        assert tuple(x.shape) == (4, 3, 16, 16)
    else:
        gen = torch.Generator().manual_seed(7)
        g = None
        x, noise = torch.rand(B, 3, size, size, generator=gen) * 2 - 1, torch.randn(B, 3, size, size, generator=gen)
        t = torch.randint(0, 1000, (B,), generator=gen)
    return g, net, gd, (x.to(DEV), t.to(DEV), noise.to(DEV))


def _backward(net, gd, batch, poison=True):
    if poison:
        net.flat_grads.fill_(float("nan"))
    gd.p_losses(*batch).backward()
    return net.flat_grads.clone()


def _stored_mask(net):
    """Elements of flat_grads the zero table leaves out: the weights of the convs and transposed convs with Ci % 64 == 0 and Cj >= 32."""
    m = torch.zeros(net._arch.flat_numel, dtype=torch.bool)
    for e in net._arch.entries:
        if e.layout in ("conv", "convT"):
            kh, kw, ci, co = e.storage_view(net._flat).shape
            if ci % 64 == 0 and co >= 32:
                m[e.offset:e.offset + e.numel] = True
    return m


def _masks(net, gd, batch, monkeypatch, cfg):
    """(stored, exact): `exact` are the stored weights no atomic takes part in -- summed in a fixed order by the LDS-DMA kernels (the
    batched 3x3 / 1x1 / stride-2 ones and fp32 mode's gathered stride-2 taps).  The others went through conv_wgrad, whose generic
    kernels add their k-slices atomically; which layers those are is read off one backward pass, not restated here."""
    import src.ops.functional as K
    stored, seen, orig = _stored_mask(net), set(), K.conv_wgrad

    def spy(P, Q, dW, **kw):
        seen.add((dW.data_ptr() - net.flat_grads.data_ptr()) // 4)
        return orig(P, Q, dW, **kw)
    monkeypatch.setattr(K, "conv_wgrad", spy)
    _backward(net, gd, batch)
    monkeypatch.setattr(K, "conv_wgrad", orig)
    exact = stored.clone()
    nfall = 0
    for e in net._arch.entries:
        if e.offset in seen and bool(stored[e.offset]):
            exact[e.offset:e.offset + e.numel] = False
            nfall += 1
    nexact = sum(1 for e in net._arch.entries if bool(exact[e.offset]))
    if cfg[1] == 4:
        assert nfall >= 1, "no stored weight took a fallback: the fill before a kernel that can only add is not exercised"
    if cfg == ("bf16", 4, 16):                   # (module docstring) every stored weight falls back: the fills are what is tested
        assert nexact == 0, nexact
    else:
        assert nexact >= 15, nexact
    if cfg == ("bf16", 8, 32):                   # the stride-2 launch of the queue runs in store mode
        offs = {e.key: e.offset for e in net._arch.entries}
        assert all(bool(exact[offs[k]]) for k in S2_KEYS), [k for k in S2_KEYS if not bool(exact[offs[k]])]
    return stored, exact


@cfgs
def test_store_matches_zero_fill(golden_dir, cfg, monkeypatch):
    g, net, gd, batch = _setup(golden_dir, cfg)
    assert net.grad_store, "store mode is the default"
    mode = cfg[0]
    net.flat_grads                                   # (the table is built with the buffer)
    table, n, keys = net._zero_tab
    tab = table.cpu()
    assert n == tab.shape[0] and n >= 2 and len(keys) >= 20
    assert bool((tab[1:, 0] > tab[:-1, 0] + tab[:-1, 1]).all()), "ranges sorted, adjacent ones merged"
    stored, mask = _masks(net, gd, batch, monkeypatch, cfg)
    covered = torch.zeros_like(stored)
    for off, cnt in tab.tolist():
        covered[off:off + cnt] = True
    assert bool((covered ^ stored).all()), "the table is exactly the complement of the stored weights"
    on = _backward(net, gd, batch).cpu()
    on2 = _backward(net, gd, batch).cpu()
    net.grad_store = False
    off = _backward(net, gd, batch).cpu()
    net.grad_store = True
    assert bool(torch.isfinite(on).all()), int((~torch.isfinite(on)).sum())
    # fixed-order sums: bit-equal (a stored -0.0 against an accumulated +0.0 aside) to the zero-fill-and-add path, and from run to run
    assert torch.equal((on[mask] + 0.0).view(torch.int32), (off[mask] + 0.0).view(torch.int32))
    assert torch.equal(on[mask].view(torch.int32), on2[mask].view(torch.int32))
    # everything else (atomics take part): per parameter against the golden gradients, the bound of test_mid_unet_golden; parameters the
    # golden file does not hold against the zero-fill path, same bound
    params = dict(net.named_parameters())
    _backward(net, gd, batch)
    bad = {}
    for k in g or ():
        if k.startswith("grad."):
            e = rel_err(params[k[5:]].grad, _t(g[k]))
            if not e < GTOL[mode]:
                bad[k] = e
    assert not bad, bad
    for e in net._arch.entries:
        a, b = on[e.offset:e.offset + e.numel], off[e.offset:e.offset + e.numel]
        if float(b.abs().max()) > 1e-7:
            assert rel_err(a, b) < GTOL[mode], (e.key, rel_err(a, b))
        else:
            assert float((a - b).abs().max()) < 1e-6, e.key


@cfgs
def test_captured_step_replays(golden_dir, cfg, monkeypatch):
    """The step captured as one graph: kernel nodes only (the zero table is a kernel, not a memset), and every replay -- flat_grads NaN
    before each -- leaves finite gradients with the eager pass's conv weights."""
    _, net, gd, batch = _setup(golden_dir, cfg)
    _, mask = _masks(net, gd, batch, monkeypatch, cfg)
    eager = _backward(net, gd, batch).cpu()
    _backward(net, gd, batch)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, stream=s):
            gd.p_losses(*batch).backward()
    torch.cuda.current_stream().wait_stream(s)
    kinds = _graph_node_types(graph)
    assert set(kinds) == {"kernel"} and kinds["kernel"] > 50, kinds
    for _ in range(3):
        net.flat_grads.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = net.flat_grads.cpu()
        assert bool(torch.isfinite(got).all())
        assert torch.equal(got[mask].view(torch.int32), eager[mask].view(torch.int32))


@cfgs
def test_accumulate_grads_adds(golden_dir, cfg, monkeypatch):
    """accumulate_grads: nothing is zeroed, nothing is stored -- two passes give twice the gradient (exactly, on the fixed-order sums)."""
    _, net, gd, batch = _setup(golden_dir, cfg)
    _, mask = _masks(net, gd, batch, monkeypatch, cfg)
    one = _backward(net, gd, batch).cpu()
    net.accumulate_grads = True
    net.flat_grads.zero_()
    _backward(net, gd, batch, poison=False)
    two = _backward(net, gd, batch, poison=False).cpu()
    net.accumulate_grads = False
    assert bool(torch.isfinite(two).all())
    assert torch.equal(two[mask], 2 * one[mask])
    # (atomics: the order of the additions varies from pass to pass, by a few ulp of the largest term)
    assert rel_err(two[~mask], 2 * one[~mask]) < 1e-5


@cfgs
def test_ranges_final_when_reported(golden_dir, cfg):
    """A grad-ready hook (data parallelism): every range is final -- bit for bit what it holds after backward -- when it is reported."""
    _, net, gd, batch = _setup(golden_dir, cfg)
    seen = []
    try:
        net.grad_ready_hook = lambda lo, hi: seen.append((lo, hi, net.flat_grads[lo:hi].clone()))
        final = _backward(net, gd, batch)
    finally:
        net.grad_ready_hook = None
    torch.cuda.synchronize()
    assert bool(torch.isfinite(final).all())
    assert len(seen) >= 10
    for lo, hi, snap in seen:
        assert torch.equal(snap.view(torch.int32), final[lo:hi].view(torch.int32)), (lo, hi)
