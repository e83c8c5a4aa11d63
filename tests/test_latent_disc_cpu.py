"""The numpy oracle of the latent discriminator (tests/_latent_disc_oracle.py) against torch autograd in float64 on the CPU, and
against the reference's own netD numbers of the FactorVAE `tiny` case (tests/golden/factor_vae_kats.npz)."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _latent_disc_oracle as O  # noqa: E402


def _torch_net(p, L, H=256):
    """The same layers as a torch Sequential in float64, weights from the oracle's dict."""
    net = nn.Sequential(nn.Linear(L, H), nn.GroupNorm(1, H), nn.LeakyReLU(0.2), nn.Linear(H, H), nn.BatchNorm1d(H), nn.LeakyReLU(0.2),
                        nn.Linear(H, 1)).double()
    order = {0: "model.0.fc.", 1: "model.0.norm.", 3: "model.1.fc.", 4: "model.1.norm.", 6: "classifier.fc."}
    with torch.no_grad():
        for i, pre in order.items():
            net[i].weight.copy_(torch.from_numpy(p[pre + "weight"]))
            net[i].bias.copy_(torch.from_numpy(p[pre + "bias"]))
    return net, order


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("N,L,target", [(2, 1, 1.0), (3, 10, 0.0), (33, 37, 1.0)])
def test_oracle_matches_torch_autograd_float64(N, L, target):
    r = np.random.RandomState(N * 100 + L)
    p = O.make_params(L, seed=L)
    x = r.randn(N, L)
    net, order = _torch_net(p, L)
    net.train()
    xt = torch.from_numpy(x).requires_grad_(True)
    logit = net(xt)[:, 0]
    loss = ((logit - target) ** 2).mean()
    loss.backward()
    f = O.forward(p, x, target, training=True, running=(np.zeros(256), np.ones(256)))
    g, dx = O.backward(p, f, target)
    assert _rel(f["logit"], logit.detach().numpy()) < 1e-12
    assert abs(float(f["loss"]) - float(loss)) < 1e-12 * max(1.0, abs(float(loss)))
    assert abs(float(f["mean_logit"]) - float(logit.mean())) < 1e-12
    assert _rel(dx, xt.grad.numpy()) < 1e-10
    for i, pre in order.items():
        for leaf in ("weight", "bias"):
            ref = getattr(net[i], leaf).grad.numpy()
            if pre + leaf == "model.1.fc.bias":                   # in front of BatchNorm: analytically zero
                assert np.abs(g[pre + leaf]).max() < 1e-12 * np.abs(g["model.1.fc.weight"]).max()
                continue
            assert _rel(g[pre + leaf], ref) < 1e-10, pre + leaf
    # running statistics after two passes (the second on other rows), then an evaluation-mode pass
    x2 = r.randn(N, L)
    net(torch.from_numpy(x2))
    f2 = O.forward(p, x2, target, training=True, running=f["running"])
    assert _rel(f2["running"][0], net[4].running_mean.numpy()) < 1e-12
    assert _rel(f2["running"][1], net[4].running_var.numpy()) < 1e-12
    assert int(net[4].num_batches_tracked) == 2
    net.eval()
    xe = torch.from_numpy(x).requires_grad_(True)
    le = net(xe)[:, 0]
    ((le - target) ** 2).mean().backward()
    fe = O.forward(p, x, target, training=False, running=f2["running"])
    ge, dxe = O.backward(p, fe, target)
    assert _rel(fe["logit"], le.detach().numpy()) < 1e-12 and _rel(dxe, xe.grad.numpy()) < 1e-10


def test_input_sources():
    r = np.random.RandomState(5)
    N, L = 7, 4
    h, eps = r.randn(N, 2 * L + 3), r.randn(N, L)
    z = h[:, :L] + np.exp(h[:, L:2 * L]) * eps
    assert np.array_equal(O.form_input(h=h, eps=eps), z)
    ident = np.tile(np.arange(N), (L, 1))
    assert np.array_equal(O.form_input(h=h, eps=eps, perm=ident), z)
    perm = np.stack([r.permutation(N) for _ in range(L)])
    x = O.form_input(h=h, eps=eps, perm=perm)
    zt = torch.from_numpy(z)
    ref = torch.cat([zj[torch.from_numpy(perm[j])] for j, zj in enumerate(zt.split(1, 1))], 1).numpy()     # the reference's permute_dims
    assert np.array_equal(x, ref)
    perm[2, 3] = N
    perm[0, 0] = -1
    x = O.form_input(h=h, eps=eps, perm=perm)
    assert x[3, 2] == 0 and x[0, 0] == 0


def test_oracle_reproduces_the_reference_netD_numbers(golden_dir):
    """FactorVAE `tiny`: the reference's netD on its own two inputs -- logits' means, both adversarial losses, the gradients of the
    discriminator loss and the running statistics after the two passes."""
    g = np.load(os.path.join(golden_dir, "factor_vae_kats.npz"))
    p = {k: g["tiny.sd0.netD." + k].astype(np.float64) for k in O.NAMES}
    z1, pz2 = g["tiny.netD_in"].astype(np.float64)
    run0 = (g["tiny.sd0.netD.model.1.norm.running_mean"].astype(np.float64), g["tiny.sd0.netD.model.1.norm.running_var"].astype(np.float64))
    fake = O.forward(p, z1, 1.0, training=True, running=run0)
    real = O.forward(p, pz2, 1.0, training=True, running=fake["running"])
    tol = 2e-6                                                    # the golden numbers are a float32 run
    assert abs(fake["mean_logit"] - g["tiny.log.train_log/fake_logit"]) < tol
    assert abs(real["mean_logit"] - g["tiny.log.train_log/real_logit"]) < tol
    assert abs(fake["loss"] - g["tiny.log.train_loss/g_adv_loss"]) < tol * 2
    d_adv = real["loss"] + (fake["logit"] ** 2).mean()
    assert abs(d_adv - g["tiny.log.train_loss/d_adv_loss"]) < tol * 3
    gr, _ = O.backward(p, real, 1.0)
    gf, _ = O.backward(p, fake, 0.0)
    wmax = np.abs(g["tiny.grad.netD.model.1.fc.weight"]).max()
    for k in O.NAMES:
        ref = g["tiny.grad.netD." + k].astype(np.float64)
        got = gr[k] + gf[k]
        if k == "model.1.fc.bias":
            assert np.abs(got).max() < 1e-12 * wmax and np.abs(ref).max() < 1e-5 * wmax
            continue
        assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max(), k
    for i, leaf in enumerate(("running_mean", "running_var")):
        ref = run0[i] + g["tiny.dsd1.netD.model.1.norm." + leaf].astype(np.float64)
        assert np.abs(real["running"][i] - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0), leaf
    assert int(g["tiny.sd1.netD.model.1.norm.num_batches_tracked"]) == 2
