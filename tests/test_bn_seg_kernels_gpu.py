"""The segmented BatchNorm + activation kernels and the adversarial-loss kernel (csrc/bn_seg.hip) through their C ABI wrappers against
the float64 oracle (tests/_bn_seg_oracle.py).

Tolerance, per tensor, is the one of tests/test_latent_disc_ln_kernels_gpu.py for fp32 tensors with fp64 sums:
max|hip - f64| <= 4 * max|oracle_f32 - f64| + 1e-6 * max|f64| -- the float32 run of the same oracle is the yardstick.  A mean logit is a
mean of signed logits that can cancel, so its floor is 1e-6 * max|logit|.  Every input is float32-representable, every output starts
as NaN."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_seg_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
SLOPE = 0.2
CS = (4, 8, 64, 1024)                                                                  # C/4 == 1 ... the widest allowed
MKINDS = ("one", "three", "49", "share+1", "ragged")


@pytest.fixture(scope="module")
def K():
    from src.ops import functional as K
    return K


def _rows(kind, C):
    """M for a kind: one row (variance 0, the unbiased-variance guard) | 3 | 49 (a 7x7 map) | one row more than a sums workgroup's
    share (a second partial of one row) | two shares and a ragged rest."""
    from src.ops.lib import load_library
    R = load_library().mi_bn_seg_rows_per_workgroup(49, C)
    assert R == 64 * max(1, 256 // C)
    return {"one": 1, "three": 3, "49": 49, "share+1": R + 1, "ragged": 2 * R + 5}[kind]


def _check(name, got, f64, f32, floor_scale=None):
    """tests/test_latent_disc_ln_kernels_gpu.py::_check"""
    got, f64, f32 = (np.asarray(a, dtype=np.float64) for a in (got, f64, f32))
    scale = float(np.abs(f64).max()) if floor_scale is None else floor_scale
    tol = 4.0 * float(np.abs(f32 - f64).max()) + 1e-6 * scale
    err = float(np.abs(got - f64).max())
    print(f"{name}: max|hip - f64| {err:.3e}  max|f32 - f64| {float(np.abs(f32 - f64).max()):.3e}  scale {scale:.3e}  tol {tol:.3e}")
    assert np.isfinite(got).all(), name
    assert err <= tol, (name, err, tol)


def _inputs(S, M, C, seed, offset=0.0):
    r = np.random.RandomState(seed)
    f = lambda a: a.astype(np.float32)                                                  # noqa: E731
    host = dict(x=f(r.randn(S * M, C) * (1.0 if offset else 1.5) + (offset if offset else r.randn(C))), gamma=f(1 + 0.3 * r.randn(C)),
                beta=f(0.2 * r.randn(C)), dy=f(r.randn(S * M, C)), rm=f(0.5 * r.randn(C)), rv=f(0.5 + r.rand(C)))
    return host, {k: torch.from_numpy(v).cuda() for k, v in host.items()}


def _oracle_fwd(h, S, dtype, training=True, kind=None, running=True):
    c = lambda k: O.cast(h[k], dtype)                                                   # noqa: E731
    return O.bn_seg_fwd(c("x"), c("gamma"), c("beta"), S, c("rm") if running else None, c("rv") if running else None, training=training,
                        kind=kind, slope=SLOPE)


def _oracle_bwd(h, fwd, dtype, kind):
    c = lambda a: O.cast(a, dtype)                                                      # noqa: E731
    return O.bn_seg_bwd(c(h["x"]), c(fwd[1]), c(fwd[2]), c(h["gamma"]), c(fwd[0]), c(h["dy"]), kind=kind, slope=SLOPE)


def _host(t):
    return t.detach().cpu().numpy().reshape(-1, t.shape[-1]) if t.dim() > 1 else t.detach().cpu().numpy()


def _run_case(K, S, M, C, kind, seed, offset=0.0):
    h, d = _inputs(S, M, C, seed, offset)
    f64, f32 = _oracle_fwd(h, S, np.float64, kind=kind), _oracle_fwd(h, S, np.float32, kind=kind)
    # ---- forward, training mode, running statistics updated S times
    rm, rv = d["rm"].clone(), d["rv"].clone()
    y, mean, rstd = K.bn_seg_fwd(d["x"], d["gamma"], d["beta"], S, rm, rv, training=True, act=kind, slope=SLOPE)
    assert mean.shape == rstd.shape == (S, C)
    for name, got, i in (("y", y, 0), ("mean", mean, 1), ("rstd", rstd, 2), ("running_mean", rm, 3), ("running_var", rv, 4)):
        _check(name, _host(got), f64[i], f32[i])
    if M == 1:                                                                          # variance 0: rstd = 1 / sqrt(eps); the unbiased-variance guard
        assert float((rv - d["rv"] * 0.9 ** S).abs().max()) <= 1e-6 and float((rstd - 1e-5 ** -0.5).abs().max()) <= 1e-3
    # null running statistics: the same output bits, nothing else touched
    y2, mean2, rstd2 = K.bn_seg_fwd(d["x"], d["gamma"], d["beta"], S, None, None, training=True, act=kind, slope=SLOPE)
    assert torch.equal(y2, y) and torch.equal(mean2, mean) and torch.equal(rstd2, rstd)
    # ---- backward: stored parameter gradients into NaN, a fresh dx
    b64 = _oracle_bwd(h, f64, np.float64, kind)
    b32 = O.bn_seg_bwd(O.cast(h["x"], np.float32), f32[1], f32[2], O.cast(h["gamma"], np.float32), f32[0], O.cast(h["dy"], np.float32), kind=kind, slope=SLOPE)
    dg, db = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
    dx = K.bn_seg_bwd(d["x"], mean, rstd, d["gamma"], y, d["dy"], act=kind, slope=SLOPE, dgamma=dg, dbeta=db)
    _check("dx", _host(dx), b64[0], b32[0])
    _check("dgamma", _host(dg), b64[1], b32[1])
    _check("dbeta", _host(db), b64[2], b32[2])
    # dx in place of dy, no parameter gradients: the same bits
    g = d["dy"].clone()
    dx2 = K.bn_seg_bwd(d["x"], mean, rstd, d["gamma"], y, g, act=kind, slope=SLOPE, out=g)
    assert dx2 is g and torch.equal(g, dx)
    # accumulated onto what is there; onto zero it equals the stored bits
    base_g, base_b = torch.randn(C, device="cuda"), torch.randn(C, device="cuda")
    ag, ab = base_g.clone(), base_b.clone()
    K.bn_seg_bwd(d["x"], mean, rstd, d["gamma"], y, d["dy"], act=kind, slope=SLOPE, dgamma=ag, dbeta=ab, accumulate=True)
    assert torch.equal(ag, base_g + dg) and torch.equal(ab, base_b + db)
    zg = torch.zeros(C, device="cuda")
    K.bn_seg_bwd(d["x"], mean, rstd, d["gamma"], y, d["dy"], act=kind, slope=SLOPE, dgamma=zg, accumulate=True)
    assert torch.equal(zg, dg)
    # ---- evaluation mode: every segment uses the running statistics, which stay as they are
    e64 = _oracle_fwd(h, S, np.float64, training=False, kind=kind)
    e32 = _oracle_fwd(h, S, np.float32, training=False, kind=kind)
    rm, rv = d["rm"].clone(), d["rv"].clone()
    ye, me, re = K.bn_seg_fwd(d["x"], d["gamma"], d["beta"], S, rm, rv, training=False, act=kind, slope=SLOPE)
    _check("y (eval)", _host(ye), e64[0], e32[0])
    _check("rstd (eval)", _host(re), e64[2], e32[2])
    assert torch.equal(rm, d["rm"]) and torch.equal(rv, d["rv"]) and torch.equal(me, d["rm"].expand(S, C))


@pytest.mark.parametrize("mkind", MKINDS)
@pytest.mark.parametrize("C", CS)
def test_matches_oracle(K, C, mkind):
    """Every (C, M) pair; the segment count and the activation rotate through {1, 2, 3} x {none, relu, leaky relu} so that every
    pairing of them occurs."""
    i = CS.index(C) * len(MKINDS) + MKINDS.index(mkind)
    S, kind = 1 + i % 3, O.ACTS[(i // 3) % 3]
    _run_case(K, S, _rows(mkind, C), C, kind, seed=100 + i)


@pytest.mark.parametrize("kind", O.ACTS)
@pytest.mark.parametrize("S", (1, 2, 3))
def test_every_segment_count_with_every_activation(K, S, kind):
    _run_case(K, S, 49, 8, kind, seed=7 * S + len(str(kind)))


def test_rows_with_a_large_common_offset(K):
    """Mean 1e3, spread 1: E[x^2] - mean^2 loses seven digits in float32 sums; the fp64 sums keep the variance."""
    _run_case(K, 2, 517, 64, "leaky_relu", seed=9, offset=1000.0)
    h, d = _inputs(2, 517, 64, 9, 1000.0)
    _, _, rstd = K.bn_seg_fwd(d["x"], d["gamma"], d["beta"], 2, None, None, act=None)
    want = 1.0 / h["x"].astype(np.float64).reshape(2, 517, 64).std(axis=1)
    assert float(np.abs(rstd.cpu().numpy() / want - 1).max()) <= 1e-4


def test_segments_equal_separate_calls_bit_for_bit(K):
    """Segment s of an S-segment call = a one-segment call on its rows: outputs, statistics, input gradient and running statistics."""
    S, M, C = 3, 301, 64
    _, d = _inputs(S, M, C, 21)
    rm, rv = d["rm"].clone(), d["rv"].clone()
    y, mean, rstd = K.bn_seg_fwd(d["x"], d["gamma"], d["beta"], S, rm, rv, act="leaky_relu")
    dx = K.bn_seg_bwd(d["x"], mean, rstd, d["gamma"], y, d["dy"], act="leaky_relu")
    rm1, rv1 = d["rm"].clone(), d["rv"].clone()
    for s in range(S):
        sl = slice(s * M, (s + 1) * M)
        xs = d["x"][sl].contiguous()
        ys, ms, rs = K.bn_seg_fwd(xs, d["gamma"], d["beta"], 1, rm1, rv1, act="leaky_relu")
        assert torch.equal(ys, y[sl]) and torch.equal(ms[0], mean[s]) and torch.equal(rs[0], rstd[s])
        assert torch.equal(K.bn_seg_bwd(xs, ms, rs, d["gamma"], ys, d["dy"][sl].contiguous(), act="leaky_relu"), dx[sl])
    assert torch.equal(rm1, rm) and torch.equal(rv1, rv)


def test_two_runs_are_bit_identical(K):
    S, M, C = 2, 2 * 256 + 37, 64
    _, d = _inputs(S, M, C, 31)

    def run():
        rm, rv = d["rm"].clone(), d["rv"].clone()
        y, mean, rstd = K.bn_seg_fwd(d["x"], d["gamma"], d["beta"], S, rm, rv, act="relu")
        dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        dx = K.bn_seg_bwd(d["x"], mean, rstd, d["gamma"], y, d["dy"], act="relu", dgamma=dg, dbeta=db)
        return [t.view(torch.int32) for t in (y, mean, rstd, rm, rv, dx, dg, db)]
    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


def test_matches_the_unsegmented_kernels(K):
    """One segment against K.batchnorm_fwd + K.leaky_relu_fwd and their backward: the same function, sums in another order."""
    M, C = 49 * 5, 16
    h, d = _inputs(1, M, C, 41)
    x4 = d["x"].view(5, 7, 7, C)
    y, mean, rstd = K.bn_seg_fwd(x4, d["gamma"], d["beta"], 1, None, None, act="leaky_relu", slope=SLOPE)
    n, m0, r0 = K.batchnorm_fwd(x4, d["gamma"], d["beta"], None, None)
    y0 = K.leaky_relu_fwd(n, SLOPE)
    assert float((y - y0).abs().max()) <= 1e-6 * float(y0.abs().max()) and float((mean[0] - m0).abs().max()) <= 1e-6
    dy4 = d["dy"].view(5, 7, 7, C)
    dx = K.bn_seg_bwd(x4, mean, rstd, d["gamma"], y, dy4, act="leaky_relu", slope=SLOPE)
    dx0 = K.batchnorm_bwd(x4, m0, r0, d["gamma"], K.leaky_relu_bwd(y0, dy4, SLOPE))
    assert float((dx - dx0).abs().max()) <= 1e-5 * float(dx0.abs().max())


def test_refusals(K):
    from src.ops.lib import load_library
    lib = load_library()
    P = lambda t: C.c_void_p(t.data_ptr())                                              # noqa: E731
    x, y = torch.randn(8, 16, device="cuda"), torch.empty(8, 16, device="cuda")
    g, b, m, r = (torch.ones(32, device="cuda") for _ in range(4))
    ws = torch.empty(1 << 12, device="cuda", dtype=torch.float64)

    def fwd(S=1, M=8, Cc=16, x_=x, y_=y, g_=g, training=1, ws_=ws, rm=None, act=0):
        return lib.mi_bn_seg_fwd(S, M, Cc, P(x_), P(g_), P(b), P(y_), P(m), P(r), rm, rm, 0.1, 1e-5, training, act, 0.2, P(ws_) if ws_ is not None else None, None)

    def bwd(Cc=16, dx_=y, y_=None, ws_=ws):
        y_ = x if y_ is None else y_
        return lib.mi_bn_seg_bwd(1, 8, Cc, P(x), P(m), P(r), P(g), P(y_), P(y_), P(dx_), None, None, 0, 0, 0.2, P(ws_) if ws_ is not None else None, None)
    assert fwd() == 0 and bool(torch.isfinite(y).all())
    before = y.clone()
    for bad in (dict(Cc=6), dict(Cc=12), dict(Cc=2), dict(Cc=2048), dict(S=0), dict(M=0), dict(x_=x.view(-1)[1:]), dict(g_=g[1:]),
                dict(y_=x), dict(ws_=None), dict(training=0), dict(act=3)):
        assert fwd(**bad) != 0 and lib.mi_last_error(), bad                            # refused with a message ...
    torch.cuda.synchronize()
    assert torch.equal(y, before)                                                       # ... and nothing launched
    assert b"alias" in (fwd(y_=x), lib.mi_last_error())[1]
    for bad in (dict(Cc=6), dict(dx_=x), dict(ws_=None), dict(dx_=y.view(-1)[1:])):
        assert bwd(**bad) != 0 and lib.mi_last_error(), bad
    assert lib.mi_bn_seg_workspace(2, 8, 6) == 0 and lib.mi_bn_seg_workspace(2, 8, 16) == 2 * 1 * 2 * 16 * 8
    with pytest.raises(RuntimeError):
        K.bn_seg_fwd(torch.randn(8, 16), g[:16], b[:16], 1)                              # a CPU tensor
    with pytest.raises(RuntimeError):
        K.bn_seg_fwd(torch.randn(9, 7, 7, 16, device="cuda"), g[:16], b[:16], 2)         # 9 samples do not split in two
    with pytest.raises(RuntimeError):
        K.bn_seg_fwd(torch.randn(8, 6, device="cuda"), g[:6], b[:6], 1)                  # C % 4 != 0


# --------------------------------------------------------------------------- mi_adv_loss
def _adv_check(K, x, targets, mode, scale=1.0):
    f64 = O.adv_loss(x.astype(np.float64), targets, mode, scale)
    f32 = O.adv_loss(x.astype(np.float32), targets, mode, scale)
    loss, mean_logit, d = K.adv_loss(torch.from_numpy(x).cuda(), targets, mode, scale=scale)
    _check(f"{mode} loss", loss.cpu().numpy(), f64[0], f32[0])
    _check(f"{mode} mean_logit", mean_logit.cpu().numpy(), f64[1], f32[1], floor_scale=float(np.abs(x).max()))
    _check(f"{mode} dlogit", d.cpu().numpy(), f64[2], f32[2])
    return loss, mean_logit, d


@pytest.mark.parametrize("mode", O.MODES)
def test_adv_loss_matches_oracle(K, mode):
    r = np.random.RandomState(3)
    for M in (1, 5, 300):                                                               # one logit | fewer than a wave | more than a workgroup
        x = (r.randn(2 * M) * 2).astype(np.float32)
        if M >= 5:
            x[[0, 1, M, M + 1]] = [0.0, -1.0, 0.0, -1.0]                                # the ties of the reference's hinge
        for targets in ((True,), (False,), (True, False), (False, True)):               # real, fake, and two segments with different targets
            _adv_check(K, x, targets, mode)
        _adv_check(K, x, (True, False), mode, scale=0.5)                               # the discriminator phase's (real + fake) / 2
        loss, _, d = _adv_check(K, x, (True, False), mode, scale=-1.75)
        d1 = K.adv_loss(torch.from_numpy(x).cuda(), (True, False), mode)[2]
        assert float((d - (-1.75) * d1).abs().max()) <= 1e-6 * float(d1.abs().max())


def test_adv_loss_vanilla_is_finite_at_large_logits(K):
    x = np.array([200.0, -200.0, 150.0, 3.0, -200.0, 200.0, -150.0, -3.0], dtype=np.float32)
    for targets in ((True, False), (False, True)):
        loss, _, d = _adv_check(K, x, targets, "vanilla")
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(d).all())
    assert 50.0 < float(K.adv_loss(torch.from_numpy(x).cuda(), (True, False), "vanilla")[0][0]) < 50.1    # mean(0, 200, 0, 0.049): not inf


def test_adv_loss_reads_a_discriminator_output_and_is_reproducible(K):
    """[N, 1, 1, 1] logits as a view of the padded [N, 1, 1, 4] buffer the last convolution writes: the gradient comes back in the
    same shape, padding lanes zero; the reference's hinge for real targets is 1 wherever the logit is positive."""
    N = 10
    buf = torch.full((N, 1, 1, 4), float("nan"), device="cuda")
    x = torch.randn(N, device="cuda") * 2
    buf[:, 0, 0, 0] = x
    dense = K.adv_loss(x, (True, False), "vanilla", scale=0.5)
    for _ in range(2):
        got = K.adv_loss(buf[..., :1], (True, False), "vanilla", scale=0.5)
        assert torch.equal(got[0], dense[0]) and torch.equal(got[1], dense[1]) and torch.equal(got[2][:, 0, 0, 0], dense[2])
        assert got[2].shape == (N, 1, 1, 1) and float(got[2]._base[..., 1:].abs().max()) == 0.0
    loss, _, d = K.adv_loss(torch.tensor([2.0, 3.0], device="cuda"), (True,), "hinge")
    assert float(loss[0]) == 1.0 and float(d.abs().max()) == 0.0
    assert K.adv_loss(x, (True,), "lsgan", want_grad=False)[2] is None
    with pytest.raises(NotImplementedError):
        K.adv_loss(x, (True,), "wgan")
    with pytest.raises(RuntimeError):
        K.adv_loss(x.cpu(), (True,), "vanilla")
    with pytest.raises(RuntimeError):
        K.adv_loss(x, (True, False, True), "vanilla")                                  # 10 logits in 3 segments
