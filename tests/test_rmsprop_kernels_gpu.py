"""The WGAN's three kernels through their wrappers: mi_rmsprop_step and mi_clamp_inplace (csrc/rmsprop.hip) and mode 3 of mi_adv_loss
(csrc/bn_seg.hip, K.critic_loss), against the numpy oracles of tests/_rmsprop_oracle.py (float64 the reference, float32 the yardstick).

RMSprop's tolerance is the project's yardstick form (tests/test_wgan_gpu.py): per tensor
|hip - f64| <= 4 |torch-CPU-fp32 RMSprop - f64| + 1e-4 scale + 1e-7, for the parameters and for the square average alike.  The clamp is
bit-exact against torch.clamp.  The Wasserstein loss is held to tests/test_bn_seg_kernels_gpu.py's bounds for the other modes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_seg_oracle as BO  # noqa: E402
import _rmsprop_oracle as RO  # noqa: E402

pytestmark = pytest.mark.gpu
WRAP = 4096 * 256 * 4 + 3                 # blocks cap x threads x 4 floats: every thread takes a second float4, and a 3-float tail
SIZES = (1, 3, 4, 5, 63, 64, 1027, WRAP)
LR, EPS, GSCALE = 6e-4, 1e-8, 0.5


@pytest.fixture(scope="module")
def K():
    from src.ops import functional as K
    return K


def _yardstick(name, got, f64, f32):
    got, f64, f32 = (np.asarray(a, dtype=np.float64) for a in (got, f64, f32))
    scale, yard, err = float(np.abs(f64).max()), float(np.abs(f32 - f64).max()), float(np.abs(got - f64).max())
    tol = 4 * yard + 1e-4 * scale + 1e-7
    print(f"{name}: |hip - f64| {err:.3e}  |torch fp32 - f64| {yard:.3e}  scale {scale:.3e}  tol {tol:.3e}")
    assert np.isfinite(got).all() and err <= tol, (name, err, tol)


@pytest.mark.parametrize("alpha", (0.99, 0.9))
@pytest.mark.parametrize("n", SIZES)
def test_rmsprop_three_chained_steps(K, n, alpha):
    r = np.random.RandomState(n % 1000 + int(alpha * 100))
    p0 = r.randn(n).astype(np.float32)
    gs = [(r.randn(n) * 10.0 ** r.randint(-3, 2, n)).astype(np.float32) for _ in range(3)]
    still = np.arange(n) % 7 == 2 if n > 1 else np.zeros(1, bool)                       # never a gradient: g = 0 and v = 0 throughout
    for g in gs:
        g[still] = 0.0
    # float64 oracle; torch.optim.RMSprop on the CPU in float32 as the yardstick
    p64, v64 = p0.astype(np.float64), np.zeros(n)
    t = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.RMSprop([t], lr=LR, alpha=alpha, eps=EPS)
    p = torch.from_numpy(p0).cuda()
    v = torch.zeros(n, device="cuda")
    for i, g in enumerate(gs):
        p64, v64 = RO.rmsprop_step(p64, g.astype(np.float64), v64, LR, alpha, EPS, GSCALE)
        t.grad = torch.from_numpy(g) * GSCALE
        opt.step()
        gd = torch.from_numpy(g).cuda()
        K.rmsprop_step(p, gd, v, LR, alpha, EPS, GSCALE)
        assert torch.equal(gd.cpu(), torch.from_numpy(g))                               # the gradient is read only
        _yardstick(f"n={n} step {i} p", p.cpu().numpy(), p64, t.detach().numpy())
        _yardstick(f"n={n} step {i} v", v.cpu().numpy(), v64, opt.state[t]["square_avg"].numpy())
        if i == 0:
            # the first update is lr g' / (sqrt(1 - alpha) |g'| + eps), g' = gscale g: about lr / sqrt(1 - alpha) >= 1.9e-3 once |g'| >> eps
            took = np.abs(g) > 1e-4
            assert not took.any() or float(np.abs(p.cpu().numpy()[took] - p0[took]).min()) > 0
    assert np.array_equal(p.cpu().numpy()[still].view(np.uint32), p0[still].view(np.uint32))      # untouched, bit for bit
    assert not v.cpu().numpy()[still].any()


def test_rmsprop_updates_a_sub_range_only_and_refuses(K):
    n, off = 1027, 64
    buf_p, buf_v = torch.randn(n + 128, device="cuda"), torch.rand(n + 128, device="cuda")
    p0, v0 = buf_p.clone(), buf_v.clone()
    g = torch.randn(n, device="cuda")
    K.rmsprop_step(buf_p[off:off + n], g, buf_v[off:off + n], LR)
    for b, b0 in ((buf_p, p0), (buf_v, v0)):
        assert torch.equal(b[:off], b0[:off]) and torch.equal(b[off + n:], b0[off + n:])
        assert float((b[off:off + n] - b0[off:off + n]).abs().min()) > 0
    with pytest.raises(RuntimeError):
        K.rmsprop_step(buf_p[1:1 + n], g, buf_v[:n], LR)                                 # not 16-byte aligned
    with pytest.raises(RuntimeError):
        K.rmsprop_step(buf_p[:n], g[:5], buf_v[:n], LR)
    with pytest.raises(RuntimeError):
        K.rmsprop_step(p0[:n].cpu(), g.cpu(), v0[:n].cpu(), LR)


SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 0.1, -0.1, 0.25, -0.25, 1e-40, -1e-40], dtype=np.float32)


def _clamp_values(n, seed, lo, hi):
    r = np.random.RandomState(seed)
    x = (r.randn(n) * 0.2).astype(np.float32)
    x[r.permutation(n)[:len(SPECIALS)]] = SPECIALS[:n]
    if n > 16:
        x[-1], x[-2], x[-3] = np.nan, np.float32(hi), np.float32(lo)                    # in the scalar tail too
    return x


@pytest.mark.parametrize("n", SIZES)
def test_clamp_is_bit_exact(K, n):
    for lo, hi in ((-0.1, 0.1), (-0.25, 0.01)):
        x = _clamp_values(n, n % 1000, lo, hi)
        want = torch.clamp(torch.from_numpy(x), lo, hi).numpy()
        assert np.array_equal(want.view(np.uint32), RO.clamp(x, lo, hi).view(np.uint32))
        t = torch.from_numpy(x).cuda()
        out = K.clamp_(t, lo, hi)
        assert out is t
        got = t.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8]
        K.clamp_(t, lo, hi)                                                             # idempotent
        assert np.array_equal(t.cpu().numpy().view(np.uint32), want.view(np.uint32))
    if n >= len(SPECIALS):
        assert np.isnan(got).sum() == np.isnan(x).sum() >= 1 and np.signbit(got[(x == 0) & np.signbit(x)]).all()


@pytest.mark.parametrize("n", SIZES[:-1])
@pytest.mark.parametrize("off", (64, 1, 3))
def test_clamp_of_a_sub_range_leaves_its_neighbours(K, n, off):
    """A range inside a larger buffer, on and off a 16-byte boundary: the floats in front of it and behind it keep their bits."""
    x = _clamp_values(n + 200, n + off, -0.1, 0.1)
    x[off - 1], x[off + n] = 7.0, -7.0                                                  # out of range, right next to it
    want = x.copy()
    want[off:off + n] = torch.clamp(torch.from_numpy(x[off:off + n]), -0.1, 0.1).numpy()
    t = torch.from_numpy(x).cuda()
    K.clamp_(t[off:off + n], -0.1, 0.1)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_clamp_refusals(K):
    t = torch.randn(16, device="cuda")
    with pytest.raises(RuntimeError):
        K.clamp_(t, 0.1, -0.1)
    with pytest.raises(RuntimeError):
        K.clamp_(t.cpu(), -0.1, 0.1)
    with pytest.raises(AssertionError):
        K.clamp_(t[::2], -0.1, 0.1)                                                     # not dense


# --------------------------------------------------------------------------- mi_adv_loss, mode 3
def _check(name, got, f64, f32, floor_scale=None):
    """tests/test_bn_seg_kernels_gpu.py::_check"""
    got, f64, f32 = (np.asarray(a, dtype=np.float64) for a in (got, f64, f32))
    scale = float(np.abs(f64).max()) if floor_scale is None else floor_scale
    tol = 4.0 * float(np.abs(f32 - f64).max()) + 1e-6 * scale
    err = float(np.abs(got - f64).max())
    print(f"{name}: max|hip - f64| {err:.3e}  max|f32 - f64| {float(np.abs(f32 - f64).max()):.3e}  scale {scale:.3e}  tol {tol:.3e}")
    assert np.isfinite(got).all(), name
    assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("nhwc", (False, True))
@pytest.mark.parametrize("M", (1, 5, 64, 257))
@pytest.mark.parametrize("targets", ((True,), (False,), (True, False), (False, True)))
def test_critic_loss_matches_oracle(K, targets, M, nhwc):
    S = len(targets)
    x = (np.random.RandomState(M + S).randn(S * M) * 2 + 0.3).astype(np.float32)
    for scale in (1.0, 0.5):
        f64, f32 = RO.critic_loss(x.astype(np.float64), targets, scale), RO.critic_loss(x, targets, scale)
        if nhwc:                                                                        # a critic's output: a view of the padded buffer
            buf = torch.full((S * M, 1, 1, 4), float("nan"), device="cuda")
            buf[:, 0, 0, 0] = torch.from_numpy(x).cuda()
            logit = buf[..., :1]
        else:
            logit = torch.from_numpy(x).cuda()
        runs = [K.critic_loss(logit, targets, scale=scale) for _ in range(2)]
        loss, mean, d = runs[0]
        assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))                 # fixed summation order: the same bits
        _check("loss", loss.cpu().numpy(), f64[0], f32[0])
        _check("mean_logit", mean.cpu().numpy(), f64[1], f32[1], floor_scale=float(np.abs(x).max()))
        if nhwc:
            assert d.shape == (S * M, 1, 1, 1) and float(d._base[..., 1:].abs().max()) == 0.0
            d = d[:, 0, 0, 0]
        _check("dlogit", d.cpu().numpy(), f64[2], f32[2])
        for s, real in enumerate(targets):                                              # the signs, plainly
            assert float(loss[s]) == (-1 if real else 1) * float(mean[s])
            assert bool((d[s * M:(s + 1) * M] == float(np.float32((-scale if real else scale) / M))).all())
    assert K.critic_loss(logit, targets, want_grad=False)[2] is None


def test_critic_loss_refusals_and_the_gan_s_table(K):
    x = torch.randn(10, device="cuda")
    assert K.ADV_LOSSES == {"vanilla": 0, "lsgan": 1, "hinge": 2}
    with pytest.raises(NotImplementedError):
        K.adv_loss(x, (True,), "wgan")
    with pytest.raises(NotImplementedError):
        K.adv_loss(x, (True,), "wasserstein")
    with pytest.raises(RuntimeError):
        K.critic_loss(x.cpu(), (True,))
    with pytest.raises(RuntimeError):
        K.critic_loss(x, (True, False, True))                                           # 10 logits in 3 segments


@pytest.mark.parametrize("mode", BO.MODES)
def test_the_other_modes_are_what_they_were(K, mode):
    """The three existing modes through K.adv_loss before and after a Wasserstein call on the same inputs: the same bits, and within
    tests/test_bn_seg_kernels_gpu.py's bounds of tests/_bn_seg_oracle.py."""
    x = (np.random.RandomState(9).randn(2 * 37) * 2).astype(np.float32)
    x[[0, 1, 37, 38]] = [0.0, -1.0, 0.0, -1.0]                                          # the ties of the reference's hinge
    xd = torch.from_numpy(x).cuda()
    before = K.adv_loss(xd, (True, False), mode, scale=0.5)
    K.critic_loss(xd, (True, False), scale=0.5)
    after = K.adv_loss(xd, (True, False), mode, scale=0.5)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    f64, f32 = BO.adv_loss(x.astype(np.float64), (True, False), mode, 0.5), BO.adv_loss(x, (True, False), mode, 0.5)
    _check(f"{mode} loss", after[0].cpu().numpy(), f64[0], f32[0])
    _check(f"{mode} mean_logit", after[1].cpu().numpy(), f64[1], f32[1], floor_scale=float(np.abs(x).max()))
    _check(f"{mode} dlogit", after[2].cpu().numpy(), f64[2], f32[2])
