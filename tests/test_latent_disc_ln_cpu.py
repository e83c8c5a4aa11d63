"""The numpy oracle of the row-local latent discriminator (tests/_latent_disc_ln_oracle.py) against torch autograd in float64 on the
CPU, and against what the reference's own discriminator read and returned in the AAE `tiny` case (tests/golden/aae_kats.npz)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _latent_disc_ln_oracle as O  # noqa: E402


def _torch_net(p, L, H=256):
    """The same layers as a torch Sequential in float64, weights from the oracle's dict."""
    net = nn.Sequential(nn.Linear(L, H), nn.GroupNorm(1, H), nn.LeakyReLU(0.2), nn.Linear(H, H), nn.GroupNorm(1, H), nn.LeakyReLU(0.2),
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


def _torch_loss(logit, t, loss_mode):
    target = torch.full_like(logit, t)
    return F.binary_cross_entropy_with_logits(logit, target) if loss_mode == "vanilla" else F.mse_loss(logit, target)


@pytest.mark.parametrize("loss_mode", ["vanilla", "lsgan"])
@pytest.mark.parametrize("N0,N1,L", [(1, 0, 1), (3, 6, 8), (33, 0, 37)])
@pytest.mark.parametrize("t0,t1,c0,c1", [(1.0, 0.0, 0.5, 0.5), (0.0, 1.0, 1.0, 0.0), (1.0, 1.0, 0.3, 1.7)])
def test_oracle_matches_torch_autograd_float64(N0, N1, L, loss_mode, t0, t1, c0, c1):
    r = np.random.RandomState(N0 * 100 + N1 * 10 + L)
    p = O.make_params(L, seed=L)
    x0, x1 = r.randn(N0, L), r.randn(N1, L)
    net, order = _torch_net(p, L)
    xt = torch.from_numpy(np.concatenate([x0, x1], 0)).requires_grad_(True)
    logit = net(xt)[:, 0]
    loss0 = _torch_loss(logit[:N0], t0, loss_mode)
    loss1 = _torch_loss(logit[N0:], t1, loss_mode) if N1 else torch.zeros((), dtype=torch.float64)
    (c0 * loss0 + c1 * loss1).backward()
    f = O.forward(p, x0, t0, x1 if N1 else None, t1, loss_mode)
    g, dx = O.backward(p, f, t0, t1, c0, c1)
    assert _rel(f["logit"], logit.detach().numpy()) < 1e-12
    for got, ref in ((f["loss0"], loss0), (f["loss1"], loss1), (f["d_loss"], 0.5 * (loss0 + loss1)), (f["mean_logit0"], logit[:N0].mean())):
        ref = float(ref.detach())
        assert abs(float(got) - ref) < 1e-12 * max(1.0, abs(ref))
    if N1:
        assert abs(float(f["mean_logit1"]) - float(logit[N0:].detach().mean())) < 1e-12
    assert _rel(dx, xt.grad.numpy()) < 1e-10
    for i, pre in order.items():
        for leaf in ("weight", "bias"):
            assert _rel(g[pre + leaf], getattr(net[i], leaf).grad.numpy()) < 1e-10, pre + leaf


def test_backward_against_other_targets_than_the_forward():
    """The tape holds nothing that depends on the targets but the per-row loss."""
    r = np.random.RandomState(3)
    p = O.make_params(8, seed=2)
    x0, x1 = r.randn(4, 8), r.randn(5, 8)
    fa = O.forward(p, x0, 1.0, x1, 0.0, "vanilla")
    fb = O.forward(p, x0, 0.0, x1, 1.0, "vanilla")
    ga, dxa = O.backward(p, fa, 0.0, 1.0, 0.5, 0.5)
    gb, dxb = O.backward(p, fb, 0.0, 1.0, 0.5, 0.5)
    assert np.array_equal(dxa, dxb) and all(np.array_equal(ga[k], gb[k]) for k in O.NAMES)


def test_vanilla_loss_is_finite_at_large_logits():
    for dt in (np.float64, np.float32):
        x = np.array([-200.0, -30.0, 0.0, 30.0, 200.0], dtype=dt)
        for t in (0.0, 1.0):
            ref = F.binary_cross_entropy_with_logits(torch.from_numpy(x.astype(np.float64)), torch.full((5,), t, dtype=torch.float64),
                                                     reduction="none").numpy()
            got = O.row_loss(x, t, "vanilla")
            assert np.isfinite(got).all() and np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()
            d = O.row_dloss(x, t, "vanilla")
            assert np.isfinite(d).all() and np.abs(d - (1 / (1 + np.exp(-x.astype(np.float64))) - t)).max() <= 1e-6


def test_oracle_reproduces_the_reference_discriminator_numbers(golden_dir):
    """AAE `tiny`: the reference's discriminator on its own three inputs.  The first two calls run on the weights of the initial state
    dict (the discriminator phase: prior against 1, q_z against 0), so logits, d_loss, both mean logits and the gradients handed to
    opt_d are reproduced; the third call runs on the updated discriminator (sd0 + dsd1)."""
    g = np.load(os.path.join(golden_dir, "aae_kats.npz"))
    pre = "discriminator."
    p = {k: g["tiny.sd0." + pre + k].astype(np.float64) for k in O.NAMES}
    x0, x1 = g["tiny.disc_in1"].astype(np.float64), g["tiny.disc_in2"].astype(np.float64)
    assert np.array_equal(g["tiny.disc_in1"], g["tiny.prior"])
    f = O.forward(p, x0, 1.0, x1, 0.0, "vanilla")
    n0 = x0.shape[0]
    tol = 2e-6                                                    # the golden numbers are a float32 run
    assert np.abs(f["logit"][:n0] - g["tiny.disc_out1"][:, 0]).max() < tol and np.abs(f["logit"][n0:] - g["tiny.disc_out2"][:, 0]).max() < tol
    assert abs(f["d_loss"] - g["tiny.log.train_loss/d_loss"]) < tol
    assert abs(f["mean_logit0"] - g["tiny.log.train_log/real_logit"]) < tol
    assert abs(f["mean_logit1"] - g["tiny.log.train_log/fake_logit"]) < tol
    gr, _ = O.backward(p, f, 1.0, 0.0, 0.5, 0.5)
    for k in O.NAMES:
        ref = g["tiny.grad2." + pre + k].astype(np.float64)
        assert np.abs(gr[k] - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-9, k
    p1 = {k: (g["tiny.sd1." + pre + k].astype(np.float64) if "tiny.sd1." + pre + k in g.files
              else p[k] + g["tiny.dsd1." + pre + k].astype(np.float64)) for k in O.NAMES}
    f3 = O.forward(p1, g["tiny.disc_in3"].astype(np.float64), 1.0, None, 0.0, "vanilla")
    assert np.abs(f3["logit"] - g["tiny.disc_out3"][:, 0]).max() < tol
    assert abs(f3["loss0"] - g["tiny.log.train_loss/adv_encoder_loss"]) < tol
    for i in range(3):
        assert abs(float(g["tiny.max_logit"][i]) - float(np.abs(g[f"tiny.disc_out{i + 1}"]).max())) < 1e-6
