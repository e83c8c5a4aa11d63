"""The latent-discriminator kernels (csrc/latent_disc.hip) through their C ABI against the float64 oracle (tests/_latent_disc_oracle.py).

Tolerance, per tensor: max|hip - f64| <= 4 * max|oracle_f32 - f64| + 1e-6 * max|f64| -- the float32 run of the same oracle is the
yardstick, the factor 4 is the one tests/test_wgan_gpu.py uses.  fc2.bias sits in front of BatchNorm, its gradient is analytically
zero: it is held to the absolute floor alone, 1e-6 * max|d fc2.weight|.  `mean_logit` is a mean of signed logits that can cancel
to nearly nothing (the shipped sizes' fake_logit is 3e-4 with logits of order 1), so its own magnitude says nothing about its
rounding error: its floor is 1e-6 * max|logit|, the scale of the terms that are summed -- the same argument as for fc2.bias."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _latent_disc_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
H = 256
MATS = ("model.0.fc.weight", "model.1.fc.weight", "classifier.fc.weight")


@pytest.fixture(scope="module")
def K():
    from src.ops import functional as K
    return K


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


def _inputs(N, L, source, seed):
    """float64 host inputs + what the kernels get (rows wider than needed: ldz > L, ldh > 2L)."""
    r = np.random.RandomState(seed)
    if source == "z":
        host = dict(z=r.randn(N, L).astype(np.float32).astype(np.float64))
        buf = torch.full((N, L + 3), float("nan"))
        buf[:, :L] = torch.from_numpy(host["z"]).float()
        return host, dict(z=buf.cuda()[:, :L])
    host = dict(h=np.concatenate([r.randn(N, L), 0.3 * r.randn(N, L)], 1).astype(np.float32).astype(np.float64),
                eps=r.randn(N, L).astype(np.float32).astype(np.float64))
    buf = torch.full((N, 2 * L + 5), float("nan"))
    buf[:, :2 * L] = torch.from_numpy(host["h"]).float()
    dev = dict(h=buf.cuda()[:, :2 * L], eps=torch.from_numpy(host["eps"]).float().cuda())
    if source == "perm":
        host["perm"] = np.stack([r.permutation(N) for _ in range(L)]).astype(np.int64)
        dev["perm"] = torch.from_numpy(host["perm"]).cuda()
    return host, dev


def _oracle(p, host, target, training=True, running=None, dtype=np.float64):
    p, host = O.cast(p, dtype), O.cast(host, dtype)
    x = O.form_input(**host)
    if running is not None:
        running = tuple(np.asarray(v).astype(dtype) for v in running)
    f = O.forward(p, x, target, training=training, running=running)
    g, dx = O.backward(p, f, target)
    return f, g, dx


def _check(name, got, f64, f32, floor_scale=None, only_floor=False):
    got, f64, f32 = (np.asarray(a, dtype=np.float64) for a in (got, f64, f32))
    scale = float(np.abs(f64).max()) if floor_scale is None else floor_scale
    tol = (0.0 if only_floor else 4.0 * float(np.abs(f32 - f64).max())) + 1e-6 * scale
    err = float(np.abs(got - f64).max())
    print(f"{name}: max|hip - f64| {err:.3e}  max|f32 - f64| {float(np.abs(f32 - f64).max()):.3e}  scale {scale:.3e}  tol {tol:.3e}")
    assert np.isfinite(got).all(), name
    assert err <= tol, (name, err, tol)


def _check_grads(got, g64, g32, scale=1.0):
    wmax = float(np.abs(g64["model.1.fc.weight"]).max()) * abs(scale)
    for k in O.NAMES:
        if k == "model.1.fc.bias":
            _check(k, got[k], 0 * g64[k], 0 * g64[k], floor_scale=wmax, only_floor=True)
        else:
            _check(k, got[k], scale * g64[k], scale * g32[k].astype(np.float64))


CASES = [(2, 1, "z", 1.0), (3, 10, "h", 0.0), (33, 16, "perm", 1.0), (64, 10, "z", 0.0), (130, 37, "perm", 1.0), (64, 37, "h", 1.0),
         (130, 1, "z", 0.0), (33, 10, "perm", 0.0), (9, 64, "h", 1.0)]


@pytest.mark.parametrize("N,L,source,target", CASES)
def test_training_pass_matches_oracle(K, N, L, source, target):
    p = O.make_params(L, seed=N + L)
    host, dev = _inputs(N, L, source, seed=7 * N + L)
    r = np.random.RandomState(1)
    run0 = (0.1 * r.randn(H), 1 + 0.2 * r.rand(H))
    f64, g64, dx64 = _oracle(p, host, target, running=run0)
    f32, g32, dx32 = _oracle(p, host, target, running=run0, dtype=np.float32)
    params = _dev_params(p)
    rm, rv = (torch.from_numpy(v).float().cuda() for v in run0)
    nbt = torch.tensor(5, dtype=torch.int64, device="cuda")
    rec = K.latent_disc_fwd(params, target, training=True, running_mean=rm, running_var=rv, num_batches_tracked=nbt, **dev)
    _check("logit", rec["logit"].cpu().numpy(), f64["logit"], f32["logit"])
    _check("loss", rec["loss"].item(), f64["loss"], f32["loss"])
    _check("mean_logit", rec["mean_logit"].item(), f64["mean_logit"], f32["mean_logit"], floor_scale=float(np.abs(f64["logit"]).max()))
    _check("mean_sq_logit", rec["mean_sq_logit"].item(), (f64["logit"] ** 2).mean(), (f32["logit"] ** 2).mean())
    _check("running_mean", rm.cpu().numpy(), f64["running"][0], f32["running"][0])
    _check("running_var", rv.cpu().numpy(), f64["running"][1], f32["running"][1])
    assert int(nbt) == 6
    tape, nf = rec["tape"], 3 * N * H + 2 * N                                         # every element of the tape is stored: fp32 tensors,
    assert torch.isfinite(tape[:nf]).all() and torch.isfinite(tape[nf + 4 * H:]).all()  # the BatchNorm statistics as fp64, the logits
    assert tape.numel() == nf + 4 * H + N and torch.isfinite(tape[nf:nf + 4 * H].view(torch.float64)).all()
    grads = _nan_like(params)
    ps, zs = 0.7, -1.3
    dz = None
    if source != "perm":
        dzbuf = torch.full((N, L + 2), float("nan"), device="cuda")
        dz = dzbuf[:, :L]
    K.latent_disc_bwd(params, rec, target, grads=grads, param_scale=ps, dz=dz, dz_scale=zs)
    _check_grads(_host_grads(grads), g64, g32, scale=ps)
    if dz is not None:
        _check("dz", dz.cpu().numpy(), zs * dx64, zs * dx32.astype(np.float64))
        assert torch.isnan(dzbuf[:, L:]).all()                                        # the pitch padding is not written
    # the other target on the same tape (the discriminator phase reuses the encoder phase's fake pass)
    other = 1.0 - target
    _, g64o, _ = _oracle(p, host, other, running=run0)
    _, g32o, _ = _oracle(p, host, other, running=run0, dtype=np.float32)
    grads2 = _nan_like(params)
    K.latent_disc_bwd(params, rec, other, grads=grads2)
    _check_grads(_host_grads(grads2), g64o, g32o)


@pytest.mark.parametrize("N,L,source", [(33, 10, "z"), (3, 16, "perm")])
def test_evaluation_mode_uses_the_running_statistics(K, N, L, source):
    p = O.make_params(L, seed=3)
    host, dev = _inputs(N, L, source, seed=11)
    r = np.random.RandomState(2)
    run = (0.1 * r.randn(H), 0.5 + r.rand(H))
    f64, g64, dx64 = _oracle(p, host, 1.0, training=False, running=run)
    f32, g32, dx32 = _oracle(p, host, 1.0, training=False, running=run, dtype=np.float32)
    params = _dev_params(p)
    rm, rv = (torch.from_numpy(v).float().cuda() for v in run)
    rm0, rv0 = rm.clone(), rv.clone()
    nbt = torch.tensor(3, dtype=torch.int64, device="cuda")
    rec = K.latent_disc_fwd(params, 1.0, training=False, running_mean=rm, running_var=rv, num_batches_tracked=nbt, **dev)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and int(nbt) == 3
    _check("logit", rec["logit"].cpu().numpy(), f64["logit"], f32["logit"])
    _check("loss", rec["loss"].item(), f64["loss"], f32["loss"])
    grads = _nan_like(params)
    dz = torch.full((N, L), float("nan"), device="cuda") if source == "z" else None
    K.latent_disc_bwd(params, rec, 1.0, grads=grads, dz=dz)
    got = _host_grads(grads)
    for k in O.NAMES:                                                                 # no batch statistics: fc2.bias has a gradient here
        _check(k, got[k], g64[k], g32[k])
    if dz is not None:
        _check("dz", dz.cpu().numpy(), dx64, dx32)
    with pytest.raises(RuntimeError):
        K.latent_disc_fwd(params, 1.0, training=False, **dev)                         # no running statistics to use


def test_running_statistics_after_two_passes(K):
    N, L = 33, 10
    p = O.make_params(L, seed=4)
    params = _dev_params(p)
    rm, rv = torch.zeros(H, device="cuda"), torch.ones(H, device="cuda")
    nbt = torch.tensor(0, dtype=torch.int64, device="cuda")
    run64, run32 = (np.zeros(H), np.ones(H)), (np.zeros(H), np.ones(H))
    for i, source in enumerate(("z", "perm")):
        host, dev = _inputs(N, L, source, seed=20 + i)
        run64 = _oracle(p, host, 1.0, running=run64)[0]["running"]
        run32 = _oracle(p, host, 1.0, running=run32, dtype=np.float32)[0]["running"]
        K.latent_disc_fwd(params, 1.0, training=True, running_mean=rm, running_var=rv, num_batches_tracked=nbt, **dev)
    _check("running_mean", rm.cpu().numpy(), run64[0], run32[0])
    _check("running_var", rv.cpu().numpy(), run64[1], run32[1])
    assert int(nbt) == 2


def test_accumulate_adds_onto_what_is_there(K):
    N, L = 33, 10
    p = O.make_params(L, seed=5)
    host, dev = _inputs(N, L, "h", seed=30)
    _, g64, dx64 = _oracle(p, host, 0.0)
    _, g32, dx32 = _oracle(p, host, 0.0, dtype=np.float32)
    params = _dev_params(p)
    rec = K.latent_disc_fwd(params, 0.0, training=True, **dev)
    g0 = [torch.randn_like(t) * 0.01 for t in params]
    grads = [t.clone() for t in g0]
    dz0 = torch.randn(N, L + 2, device="cuda") * 0.01
    dzbuf = dz0.clone()
    ps, zs = 2.5, 6.4
    K.latent_disc_bwd(params, rec, 0.0, grads=grads, param_scale=ps, accumulate_params=True, dz=dzbuf[:, :L], dz_scale=zs, accumulate_dz=True)
    base = _host_grads(g0)
    got = _host_grads(grads)
    wmax = float(np.abs(g64["model.1.fc.weight"]).max()) * ps
    for k in O.NAMES:
        if k == "model.1.fc.bias":
            _check(k, got[k] - base[k], 0 * g64[k], 0 * g64[k], floor_scale=wmax + float(np.abs(base[k]).max()), only_floor=True)
        else:
            _check(k, got[k], base[k] + ps * g64[k], base[k] + ps * g32[k].astype(np.float64))
    b = dz0[:, :L].cpu().numpy().astype(np.float64)
    _check("dz", dzbuf[:, :L].cpu().numpy(), b + zs * dx64, b + zs * dx32.astype(np.float64))
    assert torch.equal(dzbuf[:, L:], dz0[:, L:])
    # stored and accumulated-onto-zero agree bit for bit
    stored, added = _nan_like(params), [torch.zeros_like(t) for t in params]
    K.latent_disc_bwd(params, rec, 0.0, grads=stored)
    K.latent_disc_bwd(params, rec, 0.0, grads=added, accumulate_params=True)
    for a, b in zip(stored, added):
        assert torch.equal(a, b)


def _run_all(K, params, dev, want_dz):
    rec = K.latent_disc_fwd(params, 1.0, training=True, **dev)
    grads = _nan_like(params)
    N, L = rec["N"], rec["L"]
    dz = torch.full((N, L), float("nan"), device="cuda") if want_dz else None
    K.latent_disc_bwd(params, rec, 1.0, grads=grads, dz=dz)
    return [t.view(torch.int32) for t in [rec["tape"], rec["out3"]] + grads + ([dz] if want_dz else [])]   # bits (the tape holds fp64 words too)


def test_identity_permutation_equals_the_unpermuted_source_bit_for_bit(K):
    N, L = 33, 10
    params = _dev_params(O.make_params(L, seed=6))
    _, dev = _inputs(N, L, "h", seed=40)
    ident = torch.arange(N, device="cuda").repeat(L, 1)
    a = _run_all(K, params, dev, False)
    b = _run_all(K, params, dict(dev, perm=ident), False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_two_runs_are_bit_identical(K):
    N, L = 130, 37
    params = _dev_params(O.make_params(L, seed=7))
    for source in ("z", "perm"):
        _, dev = _inputs(N, L, source, seed=50)
        a = _run_all(K, params, dev, source == "z")
        b = _run_all(K, params, dev, source == "z")
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_out_of_range_index_gives_a_zero_element(K):
    """The kernel compares the index with [0, N) before anything else and returns 0 for that element (load_x in
    csrc/latent_disc.hip): it never becomes an address."""
    N, L = 33, 10
    p = O.make_params(L, seed=8)
    host, dev = _inputs(N, L, "perm", seed=60)
    host["perm"][4, 7], host["perm"][0, 0], host["perm"][9, 32] = N, -1, 2 ** 40
    dev["perm"] = torch.from_numpy(host["perm"]).cuda()
    x = O.form_input(**host)
    assert x[7, 4] == 0 and x[0, 0] == 0 and x[32, 9] == 0
    f64, g64, _ = _oracle(p, host, 1.0)
    f32, g32, _ = _oracle(p, host, 1.0, dtype=np.float32)
    params = _dev_params(p)
    rec = K.latent_disc_fwd(params, 1.0, training=True, **dev)
    _check("logit", rec["logit"].cpu().numpy(), f64["logit"], f32["logit"])
    grads = _nan_like(params)
    K.latent_disc_bwd(params, rec, 1.0, grads=grads)
    _check_grads(_host_grads(grads), g64, g32)


def test_refusals(K):
    from src.ops.lib import LATENT_DISC_NMAX, load_library
    lib = load_library()
    assert LATENT_DISC_NMAX >= 512
    assert K.latent_disc_supported(2, 1) and K.latent_disc_supported(LATENT_DISC_NMAX, 64) and K.latent_disc_supported(64, 10, 256)
    for N, L, Hd in ((1, 10, 256), (64, 65, 256), (64, 10, 128), (64, 0, 256), (LATENT_DISC_NMAX + 1, 10, 256)):
        assert not K.latent_disc_supported(N, L, Hd)
        assert lib.mi_last_error()                                                    # refused with a message
    params = _dev_params(O.make_params(10, seed=9))
    with pytest.raises(RuntimeError):
        K.latent_disc_fwd(params, 1.0, z=torch.randn(1, 10, device="cuda"))           # N = 1: BatchNorm1d has no batch statistics
    with pytest.raises(RuntimeError):
        K.latent_disc_fwd(params, 1.0, z=torch.randn(4, 65, device="cuda"))
    with pytest.raises(RuntimeError):
        K.latent_disc_fwd(params, 1.0, z=torch.randn(4, 10))                          # a CPU tensor
    with pytest.raises(RuntimeError):
        K.latent_disc_fwd(params, 1.0, z=torch.randn(4, 10, device="cuda"), eps=torch.randn(4, 10, device="cuda"))
    _, dev = _inputs(4, 10, "perm", seed=1)
    rec = K.latent_disc_fwd(params, 1.0, **dev)
    with pytest.raises(RuntimeError):
        K.latent_disc_bwd(params, rec, 1.0, dz=torch.zeros(4, 10, device="cuda"))     # no input gradient through a permutation
    with pytest.raises(RuntimeError):
        K.latent_disc_bwd(params, rec, 1.0)                                           # nothing asked for
    with pytest.raises(RuntimeError):
        K.latent_disc_fwd(params, 1.0, h=dev["h"], eps=dev["eps"], perm=dev["perm"].cpu())
