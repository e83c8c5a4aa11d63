"""The row-local latent-discriminator kernels (csrc/latent_disc_ln.hip) through their C ABI against the float64 oracle
(tests/_latent_disc_ln_oracle.py).

Tolerance, per tensor: max|hip - f64| <= 4 * max|oracle_f32 - f64| + 1e-6 * max|f64| -- the float32 run of the same oracle is the
yardstick, as in tests/test_latent_disc_kernels_gpu.py.  A mean logit is a mean of signed logits that can cancel to nearly nothing,
so its own magnitude says nothing about its rounding error: its floor is 1e-6 * max|logit|, the scale of the terms that are summed.
Both inputs are pitched views (ld > L) of NaN-filled buffers, every output starts as NaN."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _latent_disc_ln_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
H = 256
MATS = ("model.0.fc.weight", "model.1.fc.weight", "classifier.fc.weight")
LOSSES = ("vanilla", "lsgan")
# (N0, N1, L): one row, one feature | two one-row segments | segment boundary inside a tile, ragged last tile | boundary on a tile edge,
# widest L | many tiles, odd L | second segment empty
CASES = [(1, 0, 1), (1, 1, 8), (3, 6, 8), (8, 8, 64), (5, 130, 37), (33, 0, 10)]


@pytest.fixture(scope="module")
def K():
    from src.ops import functional as K
    return K


def _params(L, seed):
    """The oracle's parameters, every one of them away from its default and float32-representable: the device gets exactly the numbers
    the float64 oracle computes with, so the comparison measures the kernels' arithmetic and not the rounding of their inputs."""
    return O.cast(O.cast(O.make_params(L, seed=seed), np.float32), np.float64)


def _dev_params(p):
    """The ten tensors in the C ABI's order, weights input-major."""
    out = []
    for k in O.NAMES:
        v = np.asarray(p[k], dtype=np.float32)
        out.append(torch.from_numpy(np.ascontiguousarray(v.T if k in MATS else v)).cuda())
    return out


def _host_grads(gs):
    return {k: (g.cpu().numpy().T if k in MATS else g.cpu().numpy()).astype(np.float64) for k, g in zip(O.NAMES, gs)}


def _nan_like(ts):
    return [torch.full_like(t, float("nan")) for t in ts]


def _pitched(x, pad):
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"))
    buf[:, :x.shape[1]] = torch.from_numpy(x).float()
    return buf.cuda()[:, :x.shape[1]]


def _inputs(N0, N1, L, seed):
    """float64 host rows (float32-representable) + the pitched device views (ld0 = L + 3, ld1 = L + 5)."""
    r = np.random.RandomState(seed)
    x0 = r.randn(N0, L).astype(np.float32).astype(np.float64)
    x1 = r.randn(N1, L).astype(np.float32).astype(np.float64) if N1 else None
    return (x0, x1), (_pitched(x0, 3), _pitched(x1, 5) if N1 else None)


def _oracle(p, host, t0, t1, loss_mode, c0=1.0, c1=0.0, bt0=None, bt1=None, dtype=np.float64):
    p = O.cast(p, dtype)
    x0, x1 = (None if x is None else x.astype(dtype) for x in host)
    f = O.forward(p, x0, t0, x1, t1, loss_mode)
    g, dx = O.backward(p, f, t0 if bt0 is None else bt0, t1 if bt1 is None else bt1, c0, c1)
    return f, g, dx


def _check(name, got, f64, f32, floor_scale=None):
    got, f64, f32 = (np.asarray(a, dtype=np.float64) for a in (got, f64, f32))
    scale = float(np.abs(f64).max()) if floor_scale is None else floor_scale
    tol = 4.0 * float(np.abs(f32 - f64).max()) + 1e-6 * scale
    err = float(np.abs(got - f64).max())
    print(f"{name}: max|hip - f64| {err:.3e}  max|f32 - f64| {float(np.abs(f32 - f64).max()):.3e}  scale {scale:.3e}  tol {tol:.3e}")
    assert np.isfinite(got).all(), name
    assert err <= tol, (name, err, tol)


def _check_fwd(rec, f64, f32, N1):
    lmax = float(np.abs(f64["logit"]).max())
    _check("logit", rec["logit"].cpu().numpy(), f64["logit"], f32["logit"])
    for k in ("loss0", "loss1", "d_loss"):
        _check(k, rec[k].item(), f64[k], f32[k])
    _check("mean_logit0", rec["mean_logit0"].item(), f64["mean_logit0"], f32["mean_logit0"], floor_scale=lmax)
    _check("mean_logit1", rec["mean_logit1"].item(), f64["mean_logit1"], f32["mean_logit1"], floor_scale=lmax)
    if not N1:
        assert rec["loss1"].item() == 0.0 and rec["mean_logit1"].item() == 0.0
    assert torch.isfinite(rec["tape"]).all() and torch.isfinite(rec["out5"]).all()         # every element is stored


def _check_grads(got, g64, g32, scale=1.0, base=None):
    for k in O.NAMES:
        b = 0.0 if base is None else base[k]
        _check(k, got[k], b + scale * g64[k], b + scale * g32[k].astype(np.float64))


@pytest.mark.parametrize("loss_mode", LOSSES)
@pytest.mark.parametrize("N0,N1,L", CASES)
def test_pass_matches_oracle(K, N0, N1, L, loss_mode):
    p = _params(L, N0 + N1 + L)
    host, (x0, x1) = _inputs(N0, N1, L, seed=7 * N0 + 3 * N1 + L)
    t0, t1, c0, c1 = 1.0, 0.0, 0.5, 0.5
    f64, g64, dx64 = _oracle(p, host, t0, t1, loss_mode, c0, c1)
    f32, g32, dx32 = _oracle(p, host, t0, t1, loss_mode, c0, c1, dtype=np.float32)
    params = _dev_params(p)
    rec = K.latent_disc_ln_fwd(params, x0, t0, x1=x1, target1=t1, loss_mode=loss_mode)
    assert rec["logit"].shape == (N0 + N1,) and rec["tape"].numel() == 3 * (N0 + N1) * H + 4 * (N0 + N1)
    _check_fwd(rec, f64, f32, N1)
    # store, with scales on the parameters and on dx; the pitch padding of dx is not written
    grads = _nan_like(params)
    ps, zs = 0.7, -1.3
    dxbuf = torch.full((N0, L + 2), float("nan"), device="cuda")
    K.latent_disc_ln_bwd(params, rec, t0, t1, c0=c0, c1=c1, grads=grads, param_scale=ps, dx0=dxbuf[:, :L], dx_scale=zs)
    _check_grads(_host_grads(grads), g64, g32, scale=ps)
    _check("dx0", dxbuf[:, :L].cpu().numpy(), zs * dx64[:N0], zs * dx32[:N0].astype(np.float64))
    assert torch.isnan(dxbuf[:, L:]).all()
    # the input gradient alone (one launch) equals the one of the full backward bit for bit
    dx2 = torch.full((N0, L + 2), float("nan"), device="cuda")
    K.latent_disc_ln_bwd(params, rec, t0, t1, c0=c0, c1=c1, dx0=dx2[:, :L], dx_scale=zs)
    assert torch.equal(dx2[:, :L], dxbuf[:, :L]) and torch.isnan(dx2[:, L:]).all()
    # the other targets and the weights (1, 0) on the same tape
    _, g64o, dx64o = _oracle(p, host, t0, t1, loss_mode, 1.0, 0.0, bt0=0.0, bt1=1.0)
    _, g32o, dx32o = _oracle(p, host, t0, t1, loss_mode, 1.0, 0.0, bt0=0.0, bt1=1.0, dtype=np.float32)
    grads2 = _nan_like(params)
    dx3 = torch.full((N0, L), float("nan"), device="cuda")
    K.latent_disc_ln_bwd(params, rec, 0.0, 1.0, c0=1.0, c1=0.0, grads=grads2, dx0=dx3)
    _check_grads(_host_grads(grads2), g64o, g32o)
    _check("dx0 (other targets)", dx3.cpu().numpy(), dx64o[:N0], dx32o[:N0])


@pytest.mark.parametrize("loss_mode", LOSSES)
def test_accumulate_adds_onto_what_is_there(K, loss_mode):
    N0, N1, L = 5, 12, 10
    p = _params(L, 5)
    host, (x0, x1) = _inputs(N0, N1, L, seed=30)
    _, g64, dx64 = _oracle(p, host, 1.0, 0.0, loss_mode, 0.5, 0.5)
    _, g32, dx32 = _oracle(p, host, 1.0, 0.0, loss_mode, 0.5, 0.5, dtype=np.float32)
    params = _dev_params(p)
    rec = K.latent_disc_ln_fwd(params, x0, 1.0, x1=x1, target1=0.0, loss_mode=loss_mode)
    g0 = [torch.randn_like(t) * 0.01 for t in params]
    grads = [t.clone() for t in g0]
    dx0 = torch.randn(N0, L + 2, device="cuda") * 0.01
    dxbuf = dx0.clone()
    ps, zs = 2.5, 6.4
    K.latent_disc_ln_bwd(params, rec, 1.0, 0.0, c0=0.5, c1=0.5, grads=grads, param_scale=ps, accumulate_params=True, dx0=dxbuf[:, :L],
                         dx_scale=zs, accumulate_dx=True)
    _check_grads(_host_grads(grads), g64, g32, scale=ps, base=_host_grads(g0))
    b = dx0[:, :L].cpu().numpy().astype(np.float64)
    _check("dx0", dxbuf[:, :L].cpu().numpy(), b + zs * dx64[:N0], b + zs * dx32[:N0].astype(np.float64))
    assert torch.equal(dxbuf[:, L:], dx0[:, L:])
    # stored and accumulated-onto-zero agree bit for bit
    stored, added = _nan_like(params), [torch.zeros_like(t) for t in params]
    K.latent_disc_ln_bwd(params, rec, 1.0, 0.0, c0=0.5, c1=0.5, grads=stored)
    K.latent_disc_ln_bwd(params, rec, 1.0, 0.0, c0=0.5, c1=0.5, grads=added, accumulate_params=True)
    for a, b in zip(stored, added):
        assert torch.equal(a, b)


def test_joint_pass_equals_the_two_separate_passes_bit_for_bit(K):
    """A row's logit depends on that row alone: not on its tile, its position in the tile or its segment."""
    N0, N1, L = 5, 4, 8
    params = _dev_params(_params(L, 6))
    _, (x0, x1) = _inputs(N0, N1, L, seed=40)
    joint = K.latent_disc_ln_fwd(params, x0, 1.0, x1=x1, target1=0.0)
    a = K.latent_disc_ln_fwd(params, x0, 1.0)
    b = K.latent_disc_ln_fwd(params, x1, 0.0)
    assert torch.equal(joint["logit"][:N0], a["logit"]) and torch.equal(joint["logit"][N0:], b["logit"])
    assert torch.equal(joint["loss0"], a["loss0"]) and torch.equal(joint["loss1"], b["loss0"])
    assert torch.equal(joint["mean_logit0"], a["mean_logit0"]) and torch.equal(joint["mean_logit1"], b["mean_logit0"])
    swapped = K.latent_disc_ln_fwd(params, x1, 0.0, x1=x0, target1=1.0)
    assert torch.equal(swapped["logit"][N1:], a["logit"]) and torch.equal(swapped["logit"][:N1], b["logit"])


def _run_all(K, params, x0, x1, loss_mode):
    rec = K.latent_disc_ln_fwd(params, x0, 1.0, x1=x1, target1=0.0, loss_mode=loss_mode)
    grads = _nan_like(params)
    dx = torch.full(tuple(x0.shape), float("nan"), device="cuda")
    K.latent_disc_ln_bwd(params, rec, 1.0, 0.0, c0=0.5, c1=0.5, grads=grads, dx0=dx)
    return [t.view(torch.int32) for t in [rec["tape"], rec["out5"], dx] + grads]


@pytest.mark.parametrize("loss_mode", LOSSES)
def test_two_runs_are_bit_identical(K, loss_mode):
    N0, N1, L = 5, 130, 37
    params = _dev_params(_params(L, 7))
    _, (x0, x1) = _inputs(N0, N1, L, seed=50)
    for x, y in zip(_run_all(K, params, x0, x1, loss_mode), _run_all(K, params, x0, x1, loss_mode)):
        assert torch.equal(x, y)


def test_vanilla_loss_and_gradient_stay_finite_at_large_logits(K):
    """The head weight is scaled so that |logit| reaches about 200: exp(200) would overflow float32, the stable form does not."""
    N0, N1, L = 9, 9, 8
    p = _params(L, 8)
    host, (x0, x1) = _inputs(N0, N1, L, seed=60)
    base = float(np.abs(O.forward(p, host[0], 1.0, host[1], 0.0)["logit"]).max())
    p["classifier.fc.weight"] = p["classifier.fc.weight"] * (200.0 / base)
    p["classifier.fc.bias"] = p["classifier.fc.bias"] * (200.0 / base)
    p = O.cast(O.cast(p, np.float32), np.float64)
    f64, g64, dx64 = _oracle(p, host, 1.0, 0.0, "vanilla", 0.5, 0.5)
    f32, g32, dx32 = _oracle(p, host, 1.0, 0.0, "vanilla", 0.5, 0.5, dtype=np.float32)
    assert 150.0 < float(np.abs(f64["logit"]).max()) < 250.0
    params = _dev_params(p)
    rec = K.latent_disc_ln_fwd(params, x0, 1.0, x1=x1, target1=0.0, loss_mode="vanilla")
    _check_fwd(rec, f64, f32, N1)
    grads = _nan_like(params)
    dx = torch.full((N0, L), float("nan"), device="cuda")
    K.latent_disc_ln_bwd(params, rec, 1.0, 0.0, c0=0.5, c1=0.5, grads=grads, dx0=dx)
    _check_grads(_host_grads(grads), g64, g32)
    _check("dx0", dx.cpu().numpy(), dx64[:N0], dx32[:N0])


def test_refusals(K):
    from src.ops.lib import LATENT_DISC_LN_NMAX, load_library
    lib = load_library()
    assert LATENT_DISC_LN_NMAX >= 4096
    assert K.latent_disc_ln_supported(1, 0, 1) and K.latent_disc_ln_supported(LATENT_DISC_LN_NMAX, 0, 64)
    assert K.latent_disc_ln_supported(2048, 2048, 8, 256)
    for N0, N1, L, Hd in ((0, 4, 8, 256), (4, -1, 8, 256), (4, 4, 65, 256), (4, 4, 0, 256), (4, 4, 8, 128), (LATENT_DISC_LN_NMAX, 1, 8, 256)):
        assert not K.latent_disc_ln_supported(N0, N1, L, Hd)
        assert lib.mi_last_error()                                                    # refused with a message
    params = _dev_params(_params(10, 9))
    x = torch.randn(4, 10, device="cuda")
    with pytest.raises(RuntimeError):
        K.latent_disc_ln_fwd(params, torch.randn(4, 65, device="cuda"), 1.0)
    with pytest.raises(RuntimeError):
        K.latent_disc_ln_fwd(params, torch.randn(0, 10, device="cuda"), 1.0)          # the first segment needs a row
    with pytest.raises(RuntimeError):
        K.latent_disc_ln_fwd(params, torch.randn(4, 10), 1.0)                         # a CPU tensor
    with pytest.raises(RuntimeError):
        K.latent_disc_ln_fwd(params, x, 1.0, x1=torch.randn(4, 9, device="cuda"))     # another width
    with pytest.raises(RuntimeError):
        K.latent_disc_ln_fwd(params, x, 1.0, loss_mode="hinge")
    rec = K.latent_disc_ln_fwd(params, x, 1.0)
    with pytest.raises(RuntimeError):
        K.latent_disc_ln_bwd(params, rec, 1.0)                                        # nothing asked for
    with pytest.raises(RuntimeError):
        K.latent_disc_ln_bwd(params, rec, 1.0, dx0=torch.zeros(3, 10, device="cuda"))  # not the first segment's shape
    # the C ABI itself returns a non-zero code with a message
    import ctypes as C
    ptrs = (C.c_void_p * 10)(*[t.data_ptr() for t in params])
    out5, tape = torch.empty(5, device="cuda"), torch.empty(lib.mi_latent_disc_ln_tape_floats(4), device="cuda")
    rc = lib.mi_latent_disc_ln_fwd(4, 0, 10, 256, C.c_void_p(x.data_ptr()), 9, None, 0, ptrs, 0, 1.0, 0.0, C.c_void_p(tape.data_ptr()),
                                   C.c_void_p(out5.data_ptr()), None)
    assert rc != 0 and b"ld0" in lib.mi_last_error()                                  # a pitch below L
    rc = lib.mi_latent_disc_ln_fwd(4, 0, 10, 256, C.c_void_p(x.data_ptr()), 10, None, 0, ptrs, 2, 1.0, 0.0, C.c_void_p(tape.data_ptr()),
                                   C.c_void_p(out5.data_ptr()), None)
    assert rc != 0 and b"loss_mode" in lib.mi_last_error()
