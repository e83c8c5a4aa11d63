"""The float64 oracle of the segmented BatchNorm + activation kernels and of the adversarial losses (tests/_bn_seg_oracle.py) against
torch: nn.BatchNorm2d plus the activation run once per segment, in order, and torch.nn.functional's losses.  No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_seg_oracle as O  # noqa: E402


def _torch_act(kind, slope):
    return {None: lambda v: v, "relu": torch.relu, "leaky_relu": lambda v: F.leaky_relu(v, slope)}[kind]


def _case(S, M, C, seed):
    r = np.random.RandomState(seed)
    x = r.randn(S * M, C) * 1.5 + r.randn(C)
    return x, 1 + 0.3 * r.randn(C), 0.2 * r.randn(C), r.randn(S * M, C), 0.5 * r.randn(C), 0.5 + r.rand(C)


@pytest.mark.parametrize("kind", O.ACTS)
@pytest.mark.parametrize("S,M,C", [(1, 7, 4), (2, 12, 8), (3, 5, 4), (2, 1, 8)])
def test_oracle_matches_batchnorm2d_per_segment(S, M, C, kind):
    slope = 0.2
    x, gamma, beta, dy, rm0, rv0 = _case(S, M, C, 3 * S + M + C)
    bn = torch.nn.BatchNorm2d(C).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(rm0)); bn.running_var.copy_(torch.from_numpy(rv0))
    xt = torch.from_numpy(x).requires_grad_(True)
    ys = []
    for s in range(S):                                                                  # [M, C] rows as an NCHW batch [M, C, 1, 1]
        if M == 1:                                                                      # torch refuses one value per channel in training
            seg = xt[s * M:(s + 1) * M]
            ys.append(_torch_act(kind, slope)((seg - seg.mean(0)) / torch.sqrt(seg.var(0, unbiased=False) + 1e-5) * bn.weight + bn.bias))
            continue
        ys.append(_torch_act(kind, slope)(bn(xt[s * M:(s + 1) * M].reshape(M, C, 1, 1)).reshape(M, C)))
    yt = torch.cat(ys)
    (yt * torch.from_numpy(dy)).sum().backward()
    y, mean, rstd, rm, rv = O.bn_seg_fwd(x, gamma, beta, S, rm0, rv0, kind=kind, slope=slope)
    np.testing.assert_allclose(y, yt.detach().numpy(), rtol=1e-12, atol=1e-12)
    if M > 1:
        np.testing.assert_allclose(rm, bn.running_mean.numpy(), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(rv, bn.running_var.numpy(), rtol=1e-12, atol=1e-13)
        assert int(bn.num_batches_tracked) == S
    else:                                                                               # the guard: the biased variance (0) goes in
        want_m, want_v = rm0.copy(), rv0.copy()
        for s in range(S):
            want_m, want_v = 0.9 * want_m + 0.1 * x[s], 0.9 * want_v
        np.testing.assert_allclose(rm, want_m, rtol=1e-12)
        np.testing.assert_allclose(rv, want_v, rtol=1e-12)
    dx, dgamma, dbeta = O.bn_seg_bwd(x, mean, rstd, gamma, y, dy, kind=kind, slope=slope)
    np.testing.assert_allclose(dx, xt.grad.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(dgamma, bn.weight.grad.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(dbeta, bn.bias.grad.numpy(), rtol=1e-9, atol=1e-9)


def test_oracle_evaluation_mode_uses_running_statistics():
    S, M, C = 2, 6, 8
    x, gamma, beta, _, rm0, rv0 = _case(S, M, C, 11)
    bn = torch.nn.BatchNorm2d(C).double().eval()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(rm0)); bn.running_var.copy_(torch.from_numpy(rv0))
        want = F.leaky_relu(bn(torch.from_numpy(x).reshape(S * M, C, 1, 1)).reshape(S * M, C), 0.2).numpy()
    y, mean, rstd, rm, rv = O.bn_seg_fwd(x, gamma, beta, S, rm0, rv0, training=False, kind="leaky_relu")
    np.testing.assert_allclose(y, want, rtol=1e-12, atol=1e-12)
    assert np.array_equal(rm, rm0) and np.array_equal(rv, rv0) and np.array_equal(mean[0], rm0) and np.array_equal(mean[1], rm0)


def _torch_loss(pred, real, mode):
    """The reference's adversarial_loss, written with torch.nn.functional (src/utils/losses.py:4-24)."""
    if mode == "vanilla":
        return F.binary_cross_entropy_with_logits(pred, torch.ones_like(pred) if real else torch.zeros_like(pred))
    if mode == "lsgan":
        return F.mse_loss(pred, torch.ones_like(pred) if real else torch.zeros_like(pred))
    if real:
        return torch.maximum(1 - pred, torch.ones_like(pred)).mean()
    return torch.maximum(1 + pred, torch.zeros_like(pred)).mean()


@pytest.mark.parametrize("mode", O.MODES)
def test_oracle_losses_match_torch(mode):
    r = np.random.RandomState(5)
    x = r.randn(2 * 9) * 2
    x[[0, 3, 9, 12]] = [0.0, -1.0, 0.0, -1.0]                                          # the ties of the hinge's maximum, in both segments
    for targets in ((True, False), (False, True), (True, True)):
        loss, mean_logit, d = O.adv_loss(x, targets, mode, scale=0.5)
        xt = torch.from_numpy(x).requires_grad_(True)
        parts = [_torch_loss(xt[s * 9:(s + 1) * 9], t, mode) for s, t in enumerate(targets)]
        (0.5 * (parts[0] + parts[1])).backward()
        np.testing.assert_allclose(loss, [float(p.detach()) for p in parts], rtol=1e-12)
        np.testing.assert_allclose(mean_logit, x.reshape(2, 9).mean(1), rtol=1e-12)
        np.testing.assert_allclose(d, xt.grad.numpy(), rtol=1e-12, atol=1e-15)


def test_oracle_vanilla_loss_is_finite_at_large_logits():
    x = np.array([200.0, -200.0, 200.0, -200.0])
    loss, _, d = O.adv_loss(x, (True, False), "vanilla")
    want = [F.binary_cross_entropy_with_logits(torch.tensor(x[:2]), torch.ones(2, dtype=torch.float64)).item(),
            F.binary_cross_entropy_with_logits(torch.tensor(x[2:]), torch.zeros(2, dtype=torch.float64)).item()]
    assert np.isfinite(loss).all() and np.isfinite(d).all()
    np.testing.assert_allclose(loss, want, rtol=1e-12)
    loss32, _, d32 = O.adv_loss(x.astype(np.float32), (True, False), "vanilla")
    assert np.isfinite(loss32).all() and np.isfinite(d32).all() and loss32.dtype == np.float32


def test_reference_hinge_is_not_the_textbook_hinge():
    """max(1 - x, 1) for real targets: 1 wherever x >= 0, where the hinge loss max(1 - x, 0) would fall to 0."""
    loss, _, d = O.adv_loss(np.array([2.0, 3.0]), (True,), "hinge")
    assert loss[0] == 1.0 and np.array_equal(d, [0.0, 0.0])
