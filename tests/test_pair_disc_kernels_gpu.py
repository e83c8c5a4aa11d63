"""BiGAN's pair-head kernels (csrc/pair_disc.hip) through their C ABI against the float64 oracle (tests/_pair_disc_oracle.py).

Tolerance, per tensor: max|hip - f64| <= 4 * max|oracle_f32 - f64| + 1e-6 * max|f64| -- the float32 run of the same oracle is the
yardstick, as in tests/test_latent_disc_ln_kernels_gpu.py.  A mean logit is a mean of signed logits that can cancel, so its floor is
1e-6 * max|logit|.  Parameters and inputs are float32-representable, every input is a pitched view of a NaN-filled buffer, every
output, tape and gradient starts as NaN and must come back finite.  The inputs are continuous random numbers: no logit is exactly 0
or -1, where the hinge's max has a tie."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pair_disc_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
H, RT = 128, 8
# (N per segment, L): minimum batch, one feature | the segment boundary inside a row tile, L = 6 with pitch 8 | the boundary on a tile
# edge, the shipped L | many tiles, ragged last tile in both segments | widest L
CASES = [(2, 1), (3, 6), (RT, 100), (37, 10), (5, 128)]
FWD_KEYS = ("g_loss", "d_loss", "d_loss_real", "d_loss_fake")


@pytest.fixture(scope="module")
def K():
    from src.ops import functional as K
    return K


def _params(L, seed):
    return O.cast(O.cast(O.make_params(L, H, seed=seed), np.float32), np.float64)


def _dev_params(p):
    """The sixteen tensors in the C ABI's order, weights input-major."""
    out = []
    for k in O.NAMES:
        v = np.asarray(p[k], dtype=np.float32)
        out.append(torch.from_numpy(np.ascontiguousarray(v.T if k in O.MATS else v)).cuda())
    return out


def _host_grads(gs):
    return {k: (g.cpu().numpy().T if k in O.MATS else g.cpu().numpy()).astype(np.float64) for k, g in zip(O.NAMES, gs)}


def _nan_like(ts):
    return [torch.full_like(t, float("nan")) for t in ts]


def _pitched(x, ld):
    buf = torch.full((x.shape[0], ld), float("nan"))
    buf[:, :x.shape[1]] = torch.from_numpy(x).float()
    return buf.cuda()[:, :x.shape[1]]


def _inputs(N, L, seed):
    """float64 host arrays (float32-representable) and pitched device views: e with L = 6 at pitch 8, as the encoder hands it over."""
    r = np.random.RandomState(seed)
    host = [r.randn(n, w).astype(np.float32).astype(np.float64) for n, w in ((N, L), (N, L), (2 * N, H))]
    lde = 8 if L == 6 else L + 3
    return host, (_pitched(host[0], lde), _pitched(host[1], L + 5), _pitched(host[2], H + 4))


def _stats(seed):
    r = np.random.RandomState(seed)
    rm = (0.3 * r.randn(H)).astype(np.float32).astype(np.float64)
    rv = (0.5 + r.rand(H)).astype(np.float32).astype(np.float64)
    return rm, rv


def _oracle(p, host, mode, training, rm, rv, dtype):
    p = O.cast(p, dtype)
    e, z, xf = (a.astype(dtype) for a in host)
    f = O.forward(p, e, z, xf, mode, training, rm.astype(dtype), rv.astype(dtype))
    gi = O.backward(p, f, f["dlogit_g"])
    gp = O.backward(p, f, f["dlogit_d"])
    return f, gi, gp


def _check(name, got, f64, f32, floor_scale=None):
    got, f64, f32 = (np.asarray(a, dtype=np.float64) for a in (got, f64, f32))
    scale = float(np.abs(f64).max()) if floor_scale is None else floor_scale
    tol = 4.0 * float(np.abs(f32 - f64).max()) + 1e-6 * scale
    err = float(np.abs(got - f64).max())
    print(f"{name}: max|hip - f64| {err:.3e}  max|f32 - f64| {float(np.abs(f32 - f64).max()):.3e}  scale {scale:.3e}  tol {tol:.3e}")
    assert np.isfinite(got).all(), name
    assert err <= tol, (name, err, tol)


def _fwd(K, params, dev, mode, training, rm, rv):
    bufs = (torch.from_numpy(rm).float().cuda(), torch.from_numpy(rv).float().cuda(), torch.tensor(5, dtype=torch.int64, device="cuda"))
    rec = K.pair_disc_fwd(params, *dev, loss_mode=mode, training=training, running_mean=bufs[0], running_var=bufs[1],
                          num_batches_tracked=bufs[2])
    return rec, bufs


def _check_fwd(rec, bufs, f64, f32, training, rm, rv):
    lmax = float(np.abs(f64["logit"]).max())
    for k in ("logit", "dlogit_g", "dlogit_d"):
        _check(k, rec[k].cpu().numpy(), f64[k], f32[k])
    for k in FWD_KEYS:
        _check(k, rec[k].item(), f64[k], f32[k])
    for k in ("mean_real", "mean_fake"):
        _check(k, rec[k].item(), f64[k], f32[k], floor_scale=lmax)
    nf = rec["tape"].numel() - 8 * H                                                   # every element is stored: the float32 part, and
    assert torch.isfinite(rec["tape"][:nf]).all()                                      # BatchNorm's (mean, rstd) per segment, kept as float64
    assert torch.isfinite(rec["tape"][nf:].view(torch.float64)).all()
    if training:
        _check("running_mean", bufs[0].cpu().numpy(), f64["running_mean"], f32["running_mean"])
        _check("running_var", bufs[1].cpu().numpy(), f64["running_var"], f32["running_var"])
        assert bufs[2].item() == 7                                                     # two updates
    else:
        assert np.array_equal(bufs[0].cpu().numpy(), rm.astype(np.float32)) and np.array_equal(bufs[1].cpu().numpy(), rv.astype(np.float32))
        assert bufs[2].item() == 5


def _check_grads(got, g64, g32, scale=1.0, base=None):
    for k in O.NAMES:
        b = 0.0 if base is None else base[k]
        _check(k, got[k], b + scale * g64[k], b + scale * g32[k].astype(np.float64))


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("mode", O.LOSSES)
@pytest.mark.parametrize("N,L", CASES)
def test_pass_matches_oracle(K, N, L, mode, training):
    p = _params(L, 3 * N + L)
    host, dev = _inputs(N, L, seed=7 * N + L)
    rm, rv = _stats(N)
    f64, gi64, gp64 = _oracle(p, host, mode, training, rm, rv, np.float64)
    f32, gi32, gp32 = _oracle(p, host, mode, training, rm, rv, np.float32)
    params = _dev_params(p)
    l0 = K.LAUNCHES
    rec, bufs = _fwd(K, params, dev, mode, training, rm, rv)
    assert K.LAUNCHES - l0 == 3
    assert rec["logit"].shape == (2 * N,) and rec["tape"].numel() == 6 * 2 * N * H + 4 * N + 8 * H
    _check_fwd(rec, bufs, f64, f32, training, rm, rv)

    def new_inputs():
        return torch.full((2 * N, H + 4), float("nan"), device="cuda"), torch.full((N, L + 2), float("nan"), device="cuda")

    # both right-hand sides in one call: stored, with scales; the pitch padding is not written
    xs, ps = -1.3, 0.7
    dxf, de = new_inputs()
    grads, dxf_d = _nan_like(params), torch.full((2 * N, H), float("nan"), device="cuda")
    l0 = K.LAUNCHES
    K.pair_disc_bwd(params, rec, dxf=dxf[:, :H], de=de[:, :L], in_scale=xs, grads=grads, dxf_d=dxf_d, param_scale=ps)
    assert K.LAUNCHES - l0 == 3
    _check("dxf", dxf[:, :H].cpu().numpy(), xs * gi64[1], xs * gi32[1].astype(np.float64))
    _check("de", de[:, :L].cpu().numpy(), xs * gi64[2][:N], xs * gi32[2][:N].astype(np.float64))
    assert torch.isnan(dxf[:, H:]).all() and torch.isnan(de[:, L:]).all()
    _check_grads(_host_grads(grads), gp64[0], gp32[0], scale=ps)
    _check("dxf_d", dxf_d.cpu().numpy(), gp64[1], gp32[1])
    # inputs only (two launches; one without de) and parameters only (three): the same bits
    dxf2, de2 = new_inputs()
    l0 = K.LAUNCHES
    K.pair_disc_bwd(params, rec, dxf=dxf2[:, :H], de=de2[:, :L], in_scale=xs)
    assert K.LAUNCHES - l0 == 2
    assert torch.equal(dxf2[:, :H], dxf[:, :H]) and torch.equal(de2[:, :L], de[:, :L])
    dxf3, _ = new_inputs()
    l0 = K.LAUNCHES
    K.pair_disc_bwd(params, rec, dxf=dxf3[:, :H], in_scale=xs)
    assert K.LAUNCHES - l0 == 1 and torch.equal(dxf3[:, :H], dxf[:, :H])
    grads2, dxf_d2 = _nan_like(params), torch.full((2 * N, H), float("nan"), device="cuda")
    l0 = K.LAUNCHES
    K.pair_disc_bwd(params, rec, grads=grads2, dxf_d=dxf_d2, param_scale=ps)
    assert K.LAUNCHES - l0 == 3
    assert torch.equal(dxf_d2, dxf_d) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


@pytest.mark.parametrize("mode", O.LOSSES)
def test_accumulate_adds_onto_what_is_there(K, mode):
    N, L = 11, 10
    p = _params(L, 5)
    host, dev = _inputs(N, L, seed=30)
    rm, rv = _stats(1)
    _, gi64, gp64 = _oracle(p, host, mode, True, rm, rv, np.float64)
    _, gi32, gp32 = _oracle(p, host, mode, True, rm, rv, np.float32)
    params = _dev_params(p)
    rec, _ = _fwd(K, params, dev, mode, True, rm, rv)
    g0 = [torch.randn_like(t) * 0.01 for t in params]
    grads = [t.clone() for t in g0]
    x0, e0 = torch.randn(2 * N, H + 4, device="cuda") * 0.01, torch.randn(N, L + 2, device="cuda") * 0.01
    dxf, de = x0.clone(), e0.clone()
    xs, ps = 6.4, 2.5
    K.pair_disc_bwd(params, rec, dxf=dxf[:, :H], de=de[:, :L], in_scale=xs, accumulate_in=True, grads=grads, param_scale=ps,
                    accumulate_params=True)
    _check_grads(_host_grads(grads), gp64[0], gp32[0], scale=ps, base=_host_grads(g0))
    b = x0[:, :H].cpu().numpy().astype(np.float64)
    _check("dxf", dxf[:, :H].cpu().numpy(), b + xs * gi64[1], b + xs * gi32[1].astype(np.float64))
    b = e0[:, :L].cpu().numpy().astype(np.float64)
    _check("de", de[:, :L].cpu().numpy(), b + xs * gi64[2][:N], b + xs * gi32[2][:N].astype(np.float64))
    assert torch.equal(dxf[:, H:], x0[:, H:]) and torch.equal(de[:, L:], e0[:, L:])
    stored, added = _nan_like(params), [torch.zeros_like(t) for t in params]
    K.pair_disc_bwd(params, rec, grads=stored)
    K.pair_disc_bwd(params, rec, grads=added, accumulate_params=True)
    for a, b in zip(stored, added):
        assert torch.equal(a, b)


def _run_all(K, params, dev, mode, rm, rv):
    N, L = dev[0].shape
    rec, bufs = _fwd(K, params, dev, mode, True, rm, rv)
    grads = _nan_like(params)
    dxf, de, dxf_d = (torch.full(s, float("nan"), device="cuda") for s in ((2 * N, H), (N, L), (2 * N, H)))
    K.pair_disc_bwd(params, rec, dxf=dxf, de=de, grads=grads, dxf_d=dxf_d)
    return [t.view(torch.int32) for t in [rec["tape"], rec["out6"], rec["logit"], rec["dlogit_g"], rec["dlogit_d"], bufs[0], bufs[1], dxf, de,
                                          dxf_d] + grads]


@pytest.mark.parametrize("mode", O.LOSSES)
def test_two_runs_are_bit_identical(K, mode):
    N, L = 37, 10
    params = _dev_params(_params(L, 7))
    _, dev = _inputs(N, L, seed=50)
    rm, rv = _stats(2)
    for x, y in zip(_run_all(K, params, dev, mode, rm, rv), _run_all(K, params, dev, mode, rm, rv)):
        assert torch.equal(x, y)


def test_refusals(K):
    from src.ops.lib import load_library
    lib = load_library()
    assert K.pair_disc_supported(2, 1) and K.pair_disc_supported(128, 100) and K.pair_disc_supported(1, 128, training=False)
    for N, L, Hd, tr in ((4, 8, 256, True), (4, 129, 128, True), (4, 0, 128, True), (1, 8, 128, True), (0, 8, 128, False)):
        assert not K.pair_disc_supported(N, L, Hd, tr)
        assert lib.mi_last_error()                                                     # refused with a message
    N, L = 4, 10
    params = _dev_params(_params(L, 9))
    _, dev = _inputs(N, L, seed=60)
    l0 = K.LAUNCHES
    with pytest.raises(RuntimeError):
        K.pair_disc_fwd(params, dev[0][:1], dev[1][:1], dev[2][:2])                    # one row per segment in training mode
    with pytest.raises(RuntimeError):
        K.pair_disc_fwd(params, dev[0].cpu(), dev[1], dev[2])                          # a CPU tensor
    with pytest.raises(RuntimeError):
        K.pair_disc_fwd(params, dev[0], dev[1][:, :9], dev[2])                         # another width
    with pytest.raises(RuntimeError):
        K.pair_disc_fwd(params, dev[0], dev[1], dev[2][:, :64])                        # not H features
    with pytest.raises(NotImplementedError):
        K.pair_disc_fwd(params, *dev, loss_mode="wasserstein")
    with pytest.raises(RuntimeError):
        K.pair_disc_fwd(params, *dev, training=False)                                  # evaluation mode without running statistics
    shifted = torch.empty(params[4].numel() + 1, device="cuda")[1:].view_as(params[4]).copy_(params[4])
    with pytest.raises(RuntimeError):
        K.pair_disc_fwd(params[:4] + [shifted] + params[5:], *dev)                     # a parameter that is not 16-byte aligned
    assert K.LAUNCHES == l0                                                            # nothing was launched
    rec = K.pair_disc_fwd(params, *dev)
    with pytest.raises(RuntimeError):
        K.pair_disc_bwd(params, rec)                                                   # nothing asked for
    with pytest.raises(RuntimeError):
        K.pair_disc_bwd(params, rec, de=torch.zeros(N, L, device="cuda"))              # de without dxf
    with pytest.raises(RuntimeError):
        K.pair_disc_bwd(params, rec, dxf=torch.zeros(N, H, device="cuda"))             # not 2N rows
    # the C ABI itself returns a non-zero code with a message and launches nothing
    ptrs = (C.c_void_p * 16)(*[t.data_ptr() for t in params])
    bad = (C.c_void_p * 16)(*[t.data_ptr() + (4 if i == 4 else 0) for i, t in enumerate(params)])
    tape = torch.empty(lib.mi_pair_disc_tape_floats(N, H), device="cuda")
    ws = torch.empty(lib.mi_pair_disc_workspace_floats(N, H), device="cuda")
    out = torch.full((3, 2 * N), float("nan"), device="cuda")
    out6 = torch.empty(6, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(Hd=H, lde=None, pp=ptrs, mode=0, n=N):
        return lib.mi_pair_disc_fwd(n, L, Hd, P(dev[0]), dev[0].stride(0) if lde is None else lde, P(dev[1]), dev[1].stride(0), P(dev[2]),
                                    dev[2].stride(0), pp, 1, mode, 0.1, None, None, None, P(tape), P(ws), P(out[0]), P(out[1]), P(out[2]),
                                    P(out6), None)
    assert call(Hd=256) != 0 and b"128" in lib.mi_last_error()
    assert call(lde=L - 1) != 0 and b"lde" in lib.mi_last_error()
    assert call(pp=bad) != 0 and b"aligned" in lib.mi_last_error()
    assert call(mode=3) != 0 and b"loss_mode" in lib.mi_last_error()
    assert call(n=1) != 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
