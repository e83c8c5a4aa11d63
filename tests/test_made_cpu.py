"""MADE host layer without a GPU: config composition, state_dict contract and seeded init against the reference's fixture,
the flat buffer, size checks, and the degree vectors recovered from the masks."""
import hashlib
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "image-generation-models_amd")


def _dm(ch, H, W, normalize=False):
    return types.SimpleNamespace(width=W, height=H, channels=ch, transforms=types.SimpleNamespace(normalize=normalize))


@pytest.fixture(scope="module")
def kats(golden_dir):
    return np.load(os.path.join(golden_dir, "made_kats.npz"))


@pytest.mark.parametrize("exp", ["mnist", "synthetic"])
def test_made_experiments_compose(exp):
    from src.runtime.config import Composer
    c = Composer(os.path.join(PKG, "configs")).compose("config", [f"experiment=made/{exp}"])
    assert c.model._target_ == "src.models.made.MADE"
    assert c.model.hidden_dim == 1024 and c.model.n_layer == 3 and float(c.model.lr) == 1e-3
    assert c.datamodule.channels == 1 and c.datamodule.width == 28 and c.datamodule.height == 28
    assert c.datamodule.transforms.normalize is False
    assert "sample" in c.callbacks and "tqdm" in c.callbacks
    assert c.exp_name == f"made/{exp}"


def test_made_state_dict_and_seeded_init_match_reference(kats):
    from src.models.made import MADE
    torch.manual_seed(0)
    m = MADE(_dm(1, 28, 28), 1024, 3)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in kats["keys"]]
    for v, s, dt in zip(sd.values(), kats["shapes"], kats["dtypes"]):
        assert list(v.shape) == [int(d) for d in s if d >= 0]
        assert str(v.dtype) == str(dt)
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().contiguous().numpy().tobytes())
    assert h.hexdigest() == str(kats["sha"])
    assert isinstance(m.model.layers, list) and len(m.model.layers) == 4
    assert m.model.layers[3] is m.model.model[3]
    assert float(m.log2) == float(torch.log(torch.tensor(2.0)))


def test_made_parameters_are_views_of_one_flat_buffer():
    from src.models.made import MADE
    m = MADE(_dm(3, 3, 3), 8, 2)
    base = m.flat_params.data_ptr()
    end = base + m.flat_params.numel() * 4
    for p in m.parameters():
        assert base <= p.data_ptr() < end
    n = sum(p.numel() for p in m.parameters())
    assert n <= m.flat_params.numel() < n + 64
    g = m.flat_grads
    for p in m.parameters():
        assert g.data_ptr() <= p.grad.data_ptr() < g.data_ptr() + g.numel() * 4


@pytest.mark.parametrize("hidden,n_layer,ch", [(0, 2, 1), (6, 2, 1), (8, 0, 1), (8192 + 4, 1, 1), (8, 2, 5)])
def test_made_unsupported_sizes_raise(hidden, n_layer, ch):
    from src.models.made import MADE
    with pytest.raises(ValueError, match="not supported"):
        MADE(_dm(ch, 4, 4), hidden, n_layer)


def test_made_non_degree_mask_raises_on_load():
    from src.models.made import MADE
    torch.manual_seed(3)
    m = MADE(_dm(1, 4, 5), 8, 2)
    sd = m.state_dict()
    bad = dict(sd)
    mk = sd["model.model.1.mask"].clone()
    # two output units whose live sets cross: {0} vs {1} on inputs of different degree cannot both be down-sets
    mk[0] = False
    mk[1] = False
    i0, i1 = 0, 1
    mk[0, i0] = True
    mk[1, i1] = True
    d = m._deg[0][1]
    if int(d[i0]) == int(d[i1]):                   # the two inputs need different degrees for the crossing to be illegal
        i1 = int(torch.nonzero(d != d[i0])[0])
        mk[1] = False
        mk[1, i1] = True
    bad["model.model.1.mask"] = mk
    with pytest.raises(ValueError, match="degree form"):
        m.load_state_dict(bad)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_made_degrees_rebuild_the_masks(seed):
    from src.models.made import MADE, recover_degrees
    torch.manual_seed(seed)
    m = MADE(_dm(1, 12, 12), 256, 3)
    for _ in range(3):
        m.model.reset_mask()
        masks = [l.mask for l in m.model.layers]
        for mk, (din, dout) in zip(masks, recover_degrees(masks)):
            assert din.dtype == torch.int32 and dout.dtype == torch.int32
            assert torch.equal(mk, dout[:, None] >= din[None, :])
        for mk, (din, dout) in zip(masks, m._deg):
            assert torch.equal(mk, dout[:, None] >= din[None, :])


def test_made_abi_symbols_declared_bound_exported():
    import re
    import subprocess
    from src.ops.lib import SIGNATURES, OTHER, library_path, load_library
    hdr = open(os.path.join(ROOT, "include", "mi_ddpm.h")).read()
    names = set(re.findall(r"\b(mi_made_[a-z0-9_]+)\s*\(", hdr))
    assert {"mi_made_linear", "mi_made_dgrad", "mi_made_wgrad", "mi_made_head_fwd", "mi_made_head_dlogits", "mi_made_head_rows",
            "mi_made_sample_step", "mi_made_supported"} <= names
    assert names <= set(SIGNATURES) | set(OTHER)
    out = subprocess.run(["nm", "-D", "--defined-only", library_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert names <= exported
    lib = load_library()
    assert lib.mi_made_supported(784, 1024, 1) == 1 and lib.mi_made_supported(784, 1022, 1) == 0


def test_made_oracle_reproduces_the_fixture(kats):
    """The float64 restatement the GPU tests compare against gives the reference's logits, bpd and gradients."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _made_oracle as O
    for tag, norm in (("u", False), ("c", True)):
        p = {k[len(tag) + 5:]: torch.from_numpy(kats[k]) for k in kats.files if k.startswith(tag + ".sd0.")}
        x = torch.from_numpy(kats[tag + ".x"])
        pos = kats[tag + ".pos"]
        got = O.forward(p, x)[pos[:, 0], :, pos[:, 1], pos[:, 2], pos[:, 3]]
        ref = torch.from_numpy(kats[tag + ".logits"]).double()
        assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
        bpd, grads = O.bpd_and_grads(p, x, norm)
        assert abs(float(bpd) - float(kats[tag + ".bpd"])) <= 1e-5 * float(kats[tag + ".bpd"])
        for k, g in grads.items():
            r = torch.from_numpy(kats[f"{tag}.grad.{k}"]).double()
            assert float((g - r).abs().max()) <= 1e-4 * max(float(r.abs().max()), 1e-30), k


# ---------------------------------------------------------------------------------------------------- kernel-level references
def _oracle():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _made_oracle as O
    return O


def _ties_degrees(fin, fout):
    din = torch.randint(0, 97, (fin,))
    dout = torch.randint(int(din.min()), int(din.max()) + 1, (fout,))
    return din.int(), dout.int()


@pytest.mark.parametrize("tag,norm", [("u", False), ("c", True)])
def test_kernel_refs_chain_to_the_model_oracle(kats, tag, norm):
    """The unrounded layer / head helpers, chained by hand through the tiny fixture net, give bpd_and_grads' bpd and gradients."""
    from src.models.made import recover_degrees
    O = _oracle()
    p = {k[len(tag) + 5:]: torch.from_numpy(kats[k]) for k in kats.files if k.startswith(tag + ".sd0.")}
    x = torch.from_numpy(kats[tag + ".x"])
    L = O.n_layers(p)
    W = [p[f"model.model.{i}.model.weight"] for i in range(L)]
    B = [p[f"model.model.{i}.model.bias"] for i in range(L)]
    deg = recover_degrees([p[f"model.model.{i}.mask"] for i in range(L)])
    acts = [x.reshape(x.shape[0], -1)]
    for i in range(L - 1):
        acts.append(O.masked_linear_ref(acts[-1], W[i], B[i], *deg[i], True))
    for a, r in zip(acts[1:], O.hidden(p, x)):
        assert float((a - r).abs().max()) <= 1e-13
    logits, lse, bpd, g = O.head_ref(acts[-1], W[-1], B[-1], *deg[-1], acts[0], norm, chunk=5)
    ref_logits = O.forward(p, x).permute(0, 2, 3, 4, 1).reshape(logits.shape)
    assert float((logits - ref_logits).abs().max()) <= 1e-12 * float(ref_logits.abs().max())
    assert float((lse - torch.logsumexp(ref_logits, -1)).abs().max()) <= 1e-12
    ref_bpd, grads = O.bpd_and_grads(p, x, norm)
    assert abs(float(bpd) - float(ref_bpd)) <= 1e-12 * float(ref_bpd)

    def close(a, r, what):
        assert float((a - r).abs().max()) <= 1e-10 * max(float(r.abs().max()), 1e-300), what
    for i in range(L - 1, -1, -1):
        dw, db = O.masked_wgrad_ref(g, acts[i], *deg[i])
        close(dw, grads[f"model.model.{i}.model.weight"], f"dW{i}")
        close(db, grads[f"model.model.{i}.model.bias"], f"db{i}")
        if i:
            g = O.masked_dgrad_ref(g, W[i], *deg[i], s_in=acts[i])


def test_kernel_refs_rounded_operands_rule():
    """round_bf16 rounds exactly the matrix-core operands, before the mask, and nothing else."""
    O = _oracle()
    torch.manual_seed(0)
    din, dout = _ties_degrees(19, 11)
    m = O.live_mask(din, dout)
    x, w, b, gy, s = torch.randn(5, 19), torch.randn(11, 19), torch.randn(11), torch.randn(5, 11), torch.rand(5, 19)
    rb = lambda t: t.bfloat16().double()
    assert torch.equal(O.masked_linear_ref(x, w, b, din, dout, True, True), torch.sigmoid(rb(x) @ (rb(w) * m).t() + b.double()))
    assert torch.equal(O.masked_dgrad_ref(gy, w, din, dout, s, True), (rb(gy) @ (rb(w) * m)) * s.double() * (1 - s.double()))
    dw, db = O.masked_wgrad_ref(gy, x, din, dout, True)
    assert torch.equal(dw, (rb(gy).t() @ rb(x)) * m) and torch.equal(db, gy.double().sum(0))
    assert not torch.equal(O.masked_linear_ref(x, w, b, din, dout, True, True), O.masked_linear_ref(x, w, b, din, dout, True, False))
    D = 3
    hdin = torch.randint(0, D, (19,)).int()
    hdout = (torch.arange(D).repeat_interleave(256) - 1).int()
    hw, hb, img = torch.randn(256 * D, 19), torch.randn(256 * D), torch.randint(0, 256, (5, D)).float() / 255
    lg, lse, bpd, dl = O.head_ref(x, hw, hb, hdin, hdout, img, False, True, gscale=2.0)
    want = (rb(x) @ (rb(hw) * O.live_mask(hdin, hdout)).t() + hb.double()).reshape(5, D, 256)
    assert torch.equal(lg, want) and torch.equal(lg[:, 0], hb[:256].double().expand(5, 256))
    assert float(dl.reshape(5, D, 256).sum(-1).abs().max()) <= 1e-15
    t = O.target(img, False)
    nll = torch.nn.functional.cross_entropy(want.reshape(-1, 256), t.reshape(-1), reduction="sum")
    assert abs(float(bpd) - float(nll) / (5 * D * math.log(2.0))) <= 1e-13 * float(bpd)


@pytest.mark.parametrize("n,fin,fout", [(128, 784, 1024), (128, 1024, 1024), (3, 27, 40), (16, 4096, 8)])
def test_rounded_operands_leave_only_fp32_accumulation(n, fin, fout):
    """bf16 x bf16 products are exact in fp32.  With both operands rounded as the kernel rounds them, an fp32 evaluation of the
    forward, the data gradient and the weight gradient lies within 1e-6 of max |fp64 value| (measured: <= 4e-7 on these shapes,
    the last one a 4096-long signed contraction).  This is the evidence that 1e-5 is a fair bound for the GPU's bf16 mode."""
    O = _oracle()
    torch.manual_seed(n + fin)
    din, dout = _ties_degrees(fin, fout)
    m = O.live_mask(din, dout)
    w, b = torch.randn(fout, fin) / math.sqrt(fin), torch.randn(fout) * 0.1
    x = torch.rand(n, fin) if fin != 4096 else torch.randn(n, fin)
    gy = torch.randn(n, fout)
    r32 = lambda t: t.bfloat16().float()

    def rel(a, ref):
        return float((a.double() - ref).abs().max()) / float(ref.abs().max())
    errs = (rel(r32(x) @ (r32(w) * m).t() + b, O.masked_linear_ref(x, w, b, din, dout, False, True)),
            rel(r32(gy) @ (r32(w) * m), O.masked_dgrad_ref(gy, w, din, dout, None, True)),
            rel((r32(gy).t() @ r32(x)) * m, O.masked_wgrad_ref(gy, x, din, dout, True)[0]))
    print("fp32 evaluation of the rounded operands vs fp64:", errs)
    assert max(errs) <= 1e-6, errs


def test_dlogits_zero_sum_fp32_floor():
    """What an fp32 evaluation of exp(v - lse) - onehot leaves of the zero sum over a pixel's 256 classes (in units of the dlogits'
    scale factor), summed in fp32 and in fp64.  Measured: 6.3e-7 (= _made_oracle.ZERO_SUM_FP32; lse is 4..8, so half an ulp of it
    alone moves the sum by 2.4e-7).  tests/test_made_kernels_gpu.py allows the GPU 4x that for its own expf and summation order."""
    O = _oracle()
    torch.manual_seed(7)
    worst = 0.0
    for n, hd, D in ((96, 36, 48), (200, 64, 35), (64, 1024, 16)):
        din = torch.randint(0, D, (hd,)).int()
        dout = (torch.arange(D).repeat_interleave(256) - 1).int()
        w, b, h = torch.randn(256 * D, hd) / math.sqrt(hd), torch.randn(256 * D) * 0.1, torch.rand(n, hd)
        t = torch.randint(0, 256, (n, D))
        v = (h @ (w * O.live_mask(din, dout)).t() + b).reshape(n, D, 256)
        lse = torch.logsumexp(v, -1)
        dl = torch.exp(v - lse[..., None])
        dl.scatter_add_(-1, t[..., None], torch.full((n, D, 1), -1.0))
        worst = max(worst, float(dl.sum(-1).abs().max()), float(dl.double().sum(-1).abs().max()))
    print("zero-sum floor of the fp32 evaluation:", worst)
    assert worst <= 1.05 * O.ZERO_SUM_FP32
