"""The float64 oracle of the InfoGAN head kernels (tests/_info_head_oracle.py) against torch autograd on plain torch.nn modules and
against the reference's records (tests/golden/infogan_kats.npz, tools/gen_golden_infogan.py); the latent layout; FlatAdam's
state_dict layout with a scalar and with a per-net learning rate; the host-side refusals.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _info_head_oracle as O  # noqa: E402
from oracle import vae_oracle  # noqa: E402


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "infogan_kats.npz"))


def _params_of(netD, netQ):
    """torch's [out, in] weights as the kernels' input-major dict."""
    n = lambda t: t.detach().double().numpy()                                    # noqa: E731
    return {"wd": n(netD[1].weight).reshape(-1), "bd": n(netD[1].bias), "w1": n(netQ[1].weight).T, "b1": n(netQ[1].bias),
            "w2": n(netQ[3].weight).T, "b2": n(netQ[3].bias)}


def _params_of_sd(sd, pre=""):
    n = lambda k: np.asarray(sd[pre + k], dtype=np.float64)                      # noqa: E731
    return {"wd": n("netD.1.weight").reshape(-1), "bd": n("netD.1.bias"), "w1": n("netQ.1.weight").T, "b1": n("netQ.1.bias"),
            "w2": n("netQ.3.weight").T, "b2": n("netQ.3.bias")}


@pytest.mark.parametrize("Dd,V,Cc,E,rows", [(1, 10, 2, 64, 6), (2, 3, 3, 36, 5), (3, 2, 1, 4, 1)])
def test_oracle_matches_torch_autograd(Dd, V, Cc, E, rows):
    """Phase 0's arithmetic (both heads, the three losses) and phase 1's (the D head on two segments) in float64."""
    torch.manual_seed(Dd + E)
    netD = nn.Sequential(nn.LeakyReLU(), nn.Linear(E, 1)).double()
    netQ = nn.Sequential(nn.LeakyReLU(), nn.Linear(E, 128), nn.LeakyReLU(), nn.Linear(128, Dd * V + Cc)).double()
    lam = 0.75
    f = torch.randn(rows, E, dtype=torch.float64, requires_grad=True)
    idx, cont = torch.randint(0, V, (rows, Dd)), torch.rand(rows, Cc, dtype=torch.float64) * 2 - 1
    logit, q = netD(f), netQ(f)
    g_loss = F.binary_cross_entropy_with_logits(logit, torch.ones_like(logit))
    i_disc = F.cross_entropy(q[:, :-Cc].reshape(-1, V, Dd), idx)
    i_cont = F.mse_loss(q[:, -Cc:], cont)
    (g_loss + lam * (i_disc + i_cont)).backward()
    p = _params_of(netD, netQ)
    o = O.head_fwd(f.detach().numpy(), p, [True], 1.0, (idx.numpy(), cont.numpy(), V), lam)
    close = lambda a, b: np.testing.assert_allclose(a, np.asarray(b.detach() if torch.is_tensor(b) else b), rtol=1e-12, atol=1e-14)   # noqa: E731
    close(o["logit"], logit.reshape(-1)); close(o["q"], q); close(o["loss"][0], g_loss); close(o["I_disc"], i_disc); close(o["I_cont"], i_cont)
    close(o["mean_logit"][0], logit.mean())
    b = O.head_bwd(f.detach().numpy(), p, o["dlogit"], o["q1"], o["dq"])
    close(b["df"], f.grad); close(b["wd"], netD[1].weight.grad.reshape(-1)); close(b["bd"], netD[1].bias.grad)
    close(b["w1"], netQ[1].weight.grad.T); close(b["b1"], netQ[1].bias.grad); close(b["w2"], netQ[3].weight.grad.T); close(b["b2"], netQ[3].bias.grad)
    # phase 1: [real | fake] as two segments, (real + fake) / 2
    for m in (netD, netQ):
        m.zero_grad()
    f2 = torch.randn(2 * rows, E, dtype=torch.float64, requires_grad=True)
    l2 = netD(f2)
    real = F.binary_cross_entropy_with_logits(l2[:rows], torch.ones_like(l2[:rows]))
    fake = F.binary_cross_entropy_with_logits(l2[rows:], torch.zeros_like(l2[rows:]))
    ((real + fake) / 2).backward()
    o2 = O.head_fwd(f2.detach().numpy(), p, [True, False], 0.5)
    close(o2["loss"], torch.stack([real, fake])); close(o2["mean_logit"], torch.stack([l2[:rows].mean(), l2[rows:].mean()]))
    b2 = O.head_bwd(f2.detach().numpy(), p, o2["dlogit"])
    close(b2["df"], f2.grad); close(b2["wd"], netD[1].weight.grad.reshape(-1)); close(b2["bd"], netD[1].bias.grad)


def test_latent_layout_is_value_major():
    """Dd = 2: the one-hot of code d with value v sits at column v * Dd + d, what flattening the reference's [N, V, Dd] tensor gives."""
    idx = torch.tensor([[0, 2], [1, 1], [2, 0]])
    N, V, Dd = 3, 3, 2
    dis_c = torch.zeros(N, V, Dd)
    dis_c.scatter_(1, idx.unsqueeze(1), torch.ones_like(dis_c))                          # info_gan.py:83-84
    cont, z = torch.full((N, 3), 0.5), torch.full((N, 5), -2.0)
    want = torch.cat([dis_c.reshape(N, -1), cont, z], dim=1).numpy()                     # info_gan.py:92
    got = O.pack_latent(idx.numpy(), cont.numpy(), z.numpy(), V)
    assert got.shape == (N, 16) and np.array_equal(got[:, :14], want) and not got[:, 14:].any()
    assert got[0, 0 * Dd + 0] == 1 and got[0, 2 * Dd + 1] == 1 and got[0, :6].sum() == 2


def _tiny_features(g, tag):
    """The common layer's output in a recorded tiny phase, from sd0 and the stored latents, with the conv nets of oracle/vae_oracle.py
    in float64: phase 0 -> the fake's features [N, E]; phase 1 -> [real | fake] [2N, E] (each half with its own batch statistics)."""
    sd = {str(k): torch.from_numpy(g[f"tiny.sd0.{k}"]).double() for k in g["tiny.names"] if not str(k).endswith("num_batches_tracked")}
    V = int(g["tiny.cfg.discrete_value"])
    L = g[f"{tag}.idx"].shape[1] * V + g[f"{tag}.cont"].shape[1] + g[f"{tag}.z"].shape[1]
    z_full = torch.from_numpy(O.pack_latent(g[f"{tag}.idx"], g[f"{tag}.cont"], g[f"{tag}.z"], V)[:, :L]).double()
    fake = vae_oracle.decoder(sd, z_full, pre="netG.")
    if tag.endswith("p0"):
        return vae_oracle.encoder(sd, fake, pre="common_layer.").numpy(), sd
    imgs = torch.from_numpy(g["tiny.imgs_u8"].astype(np.float32) / np.float32(127.5) - np.float32(1)).double()
    return torch.cat([vae_oracle.encoder(sd, imgs, pre="common_layer."), vae_oracle.encoder(sd, fake, pre="common_layer.")]).numpy(), sd


def test_oracle_matches_reference_tiny_phase0(g):
    """The reference's float32 step against the float64 oracle: 2e-5 relative to the tensor's largest magnitude, float32's error through the conv nets."""
    f, sd = _tiny_features(g, "tiny.p0")
    p = _params_of_sd({k: v.numpy() for k, v in sd.items()})
    V, lam = int(g["tiny.cfg.discrete_value"]), float(g["tiny.cfg.lambda_I"])
    o = O.head_fwd(f, p, [True], 1.0, (g["tiny.p0.idx"], g["tiny.p0.cont"], V), lam)
    close = lambda a, b, what: np.testing.assert_allclose(a, b, rtol=0, atol=2e-5 * float(np.abs(b).max()) + 1e-7, err_msg=what)   # noqa: E731
    close(o["logit"], g["tiny.p0.logit"], "logit"); close(o["q"], g["tiny.p0.q"], "q")
    close(o["loss"][0], g["tiny.p0.log.train_loss/g_loss"], "g_loss")
    close(o["I_disc"], g["tiny.p0.log.train_loss/I_discrete_loss"], "I_disc"); close(o["I_cont"], g["tiny.p0.log.train_loss/I_continuous"], "I_cont")
    close(o["loss"][0] + lam * (o["I_disc"] + o["I_cont"]), g["tiny.p0.total"], "total")
    b = O.head_bwd(f, p, o["dlogit"], o["q1"], o["dq"])
    for k, name, tr in (("w1", "netQ.1.weight", True), ("b1", "netQ.1.bias", False), ("w2", "netQ.3.weight", True), ("b2", "netQ.3.bias", False)):
        close(b[k].T if tr else b[k], g[f"tiny.p0.grad.{name}"], name)


def test_oracle_matches_reference_tiny_phase1(g):
    f, sd = _tiny_features(g, "tiny.p1")
    p = _params_of_sd({k: v.numpy() for k, v in sd.items()})
    o = O.head_fwd(f, p, [True, False], 0.5)
    close = lambda a, b, what: np.testing.assert_allclose(a, b, rtol=0, atol=2e-5 * float(np.abs(b).max()) + 1e-7, err_msg=what)   # noqa: E731
    close(o["logit"], g["tiny.p1.logit"], "logit")
    close((o["loss"][0] + o["loss"][1]) / 2, g["tiny.p1.log.train_loss/d_loss"], "d_loss")
    close(o["mean_logit"][0], g["tiny.p1.log.train_log/pred_real"], "pred_real"); close(o["mean_logit"][1], g["tiny.p1.log.train_log/pred_fake"], "pred_fake")
    b = O.head_bwd(f, p, o["dlogit"])
    close(b["wd"].reshape(1, -1), g["tiny.p1.grad.netD.1.weight"], "netD.1.weight"); close(b["bd"], g["tiny.p1.grad.netD.1.bias"], "netD.1.bias")


def test_oracle_matches_reference_default_heads(g):
    """The heads at the shipped widths, float64 against float64: agreement to rounding."""
    p = _params_of_sd({k[len("heads.sd."):]: g[k] for k in g.files if k.startswith("heads.sd.")})
    f, idx, cont = g["heads.f"], g["heads.idx"], g["heads.cont"]
    o = O.head_fwd(f, p, [True], 1.0, (idx, cont, 10), 1.0)
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-11, atol=1e-13)          # noqa: E731
    close(o["logit"], g["heads.logit"]); close(o["q"], g["heads.q"]); close(o["loss"][0], g["heads.g_loss64"])
    close(o["I_disc"], g["heads.I_disc64"]); close(o["I_cont"], g["heads.I_cont64"])
    b = O.head_bwd(f, p, o["dlogit"], o["q1"], o["dq"])
    close(b["df"], g["heads.df"])
    close(b["w1"][g["heads.w1_rows"]].T, g["heads.grad.netQ.1.weight"]); close(b["b1"], g["heads.grad.netQ.1.bias"])
    close(b["w2"].T, g["heads.grad.netQ.3.weight"]); close(b["b2"], g["heads.grad.netQ.3.bias"])
    # the kernels' number formats (f32=True) stay within float32's resolution of it
    o32 = O.head_fwd(f, p, [True], 1.0, (idx, cont, 10), 1.0, f32=True)
    assert abs(o32["I_disc"] - o["I_disc"]) <= O.ce_bound(o["I_disc"])
    np.testing.assert_allclose(o32["q"], o["q"], rtol=0, atol=2.0 ** -23 * float(np.abs(o["q"]).max()))


def test_ce_bound_is_the_measured_one(g):
    """The constant in the oracle file is the reference's own float32 deviation on the default-heads record, times 4."""
    dev = abs(float(g["heads.I_disc32"]) - float(g["heads.I_disc64"]))
    assert dev / float(g["heads.I_disc64"]) == pytest.approx(O.CE_REL_MEASURED, rel=1e-9)
    assert O.CE_REL_BOUND == 4 * O.CE_REL_MEASURED
    assert int(g["loss_mode.lsgan_equals_vanilla"]) == 1


class _Net(nn.Module):
    """What FlatAdam asks of a net, on the CPU."""

    def __init__(self, n):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(n))
        self.flat_params, self.flat_grads = self.w.data, torch.zeros(n)

    def mark_params_dirty(self):
        pass


def test_flat_adam_groups():
    from src.runtime.optim import FlatAdam
    a, b = _Net(64), _Net(128)
    opt = FlatAdam([a, b], lr=2e-4, betas=(0.5, 0.999))
    sd = opt.state_dict()                                                                # a scalar lr: the layout of before
    assert list(sd) == ["step", "m", "v", "param_groups"] and sd["step"] == 0 and sd["m"] is None and sd["v"] is None
    assert sd["param_groups"] == [{"lr": 2e-4, "betas": (0.5, 0.999), "eps": 1e-8}]
    assert len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == 2 and not opt.per_net_lr
    opt2 = FlatAdam([a, b], lr=[1e-3, 2e-4], betas=(0.5, 0.999))
    assert [gr["lr"] for gr in opt2.param_groups] == [1e-3, 2e-4] and [len(gr["params"]) for gr in opt2.param_groups] == [1, 1]
    sd2 = opt2.state_dict()
    assert sd2["param_groups"] == [{"lr": 1e-3, "betas": (0.5, 0.999), "eps": 1e-8}, {"lr": 2e-4, "betas": (0.5, 0.999), "eps": 1e-8}]
    sd2["param_groups"][1]["lr"] = 5e-5
    opt2.load_state_dict(sd2)
    assert [gr["lr"] for gr in opt2.param_groups] == [1e-3, 5e-5]
    with pytest.raises(NotImplementedError):
        FlatAdam([a, b], lr=[1e-3, 2e-4], device_state=True)
    with pytest.raises(ValueError):
        FlatAdam([a, b], lr=[1e-3])


def test_host_side_refusals():
    from src.networks.info_heads import InfoDHead, InfoQHead
    from src.ops import functional as K
    for bad in (6, 0, 4100):
        with pytest.raises(NotImplementedError):
            InfoDHead(bad)
    with pytest.raises(NotImplementedError):
        InfoQHead(36, 65)
    with pytest.raises(NotImplementedError):
        InfoQHead(38, 9)
    d, q = InfoDHead(36), InfoQHead(36, 9)
    assert [k for k, _ in d.named_parameters()] == ["1.weight", "1.bias"] and d.state_dict()["1.weight"].shape == (1, 36)
    assert [k for k, _ in q.named_parameters()] == ["1.weight", "1.bias", "3.weight", "3.bias"]
    assert q.state_dict()["1.weight"].shape == (128, 36) and q.state_dict()["3.weight"].shape == (9, 128)
    assert d.tensors()[0].shape == (36, 1) and q.tensors()[0].shape == (36, 128) and q.tensors()[2].shape == (128, 9)     # input-major storage
    for call in (lambda: d(torch.zeros(2, 36)), lambda: q(torch.zeros(2, 36)),
                 lambda: K.info_head_fwd(torch.zeros(2, 36), [torch.zeros(36), torch.zeros(1)] + [None] * 4, [True]),
                 lambda: K.info_latent(torch.zeros(2, 1, dtype=torch.int64), torch.zeros(2, 2), torch.zeros(2, 3), 10)):
        with pytest.raises(RuntimeError):                                                # a CPU tensor raises: there is no fallback
            call()
