"""The InfoGAN head and latent-packing kernels (csrc/info_head.hip) through their C ABI against the float64 oracle
(tests/_info_head_oracle.py).

Tolerance, per tensor: max|hip - f64| <= 4 * max|oracle_f32 - f64| + 1e-6 * max|f64| -- the float32 run of the same oracle is the
yardstick, as in tests/test_latent_disc_ln_kernels_gpu.py (a mean logit's floor is 1e-6 * max|logit| there and here).  The mean
cross-entropy takes the bound measured on the reference, `ce_bound` of the oracle file.  The feature rows are a pitched view
(ld > E) of a NaN-filled buffer, every output starts as NaN (the allocator of tests/conftest.py hands out NaN-filled blocks)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _info_head_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
H = 128
NAMES = ("wd", "bd", "w1", "b1", "w2", "b2")
CODES = [(1, 10, 2), (2, 3, 3), (3, 2, 1)]                    # (Dd, V, Cc): the shipped codes | the tiny model's | V = 2, one continuous code
# rows per segment: one row | a ragged tile (RT = 4) | many tiles and, with S = 2, a segment boundary inside a tile
ROWS = [(M, S) for M in (1, 5, 33) for S in (1, 2)]
WIDTHS = (4, 36, 1024)                                          # the narrowest | not a multiple of the 256-wide staging chunk | 4 chunks


@pytest.fixture(scope="module")
def K():
    from src.ops import functional as K
    return K


def _dev(p):
    return [torch.from_numpy(np.ascontiguousarray(np.asarray(p[k], dtype=np.float32))).cuda() for k in NAMES]


def _pitched(x, pad=4):
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"))
    buf[:, :x.shape[1]] = torch.from_numpy(np.asarray(x)).float()
    return buf.cuda()[:, :x.shape[1]]


def _case(M, S, E, code, seed):
    Dd, V, Cc = code
    r = np.random.RandomState(seed)
    rows = M * S
    f = r.randn(rows, E).astype(np.float32).astype(np.float64)
    idx = r.randint(0, V, (rows, Dd)).astype(np.int64)
    cont = r.uniform(-1, 1, (rows, Cc)).astype(np.float32).astype(np.float64)
    return f, idx, cont, O.make_params(E, Dd * V + Cc, seed + 1)


def _check(name, got, f64, f32, floor_scale=None, tol=None):
    got, f64, f32 = (np.asarray(a, dtype=np.float64) for a in (got, f64, f32))
    scale = float(np.abs(f64).max()) if floor_scale is None else floor_scale
    tol = 4.0 * float(np.abs(f32 - f64).max()) + 1e-6 * scale if tol is None else tol
    err = float(np.abs(got - f64).max())
    print(f"{name}: max|hip - f64| {err:.3e}  max|f32 - f64| {float(np.abs(f32 - f64).max()):.3e}  scale {scale:.3e}  tol {tol:.3e}")
    assert got.shape == f64.shape and np.isfinite(got).all(), name
    assert err <= tol, (name, err, tol)


def _h(t):
    return t.detach().cpu().numpy()


def _run_pass(K, M, S, E, code, seed):
    """Phase 0's and phase 1's calls on one case: forward with and without the Q head, each of the backward's gradient selections."""
    f, idx, cont, p = _case(M, S, E, code, seed)
    V = code[1]
    targets = [True, False][:S]
    scale, lam = 0.5, 0.75
    o64 = O.head_fwd(f, p, targets, scale, (idx, cont, V), lam)
    o32 = O.head_fwd(f, p, targets, scale, (idx, cont, V), lam, dtype=np.float32)
    fd, par = _pitched(f), _dev(p)
    didx, dcont = torch.from_numpy(idx).cuda(), _pitched(cont, 3)
    rec = K.info_head_fwd(fd, par, targets, scale=scale, codes=(didx, dcont, V), lambda_I=lam)
    lmax = float(np.abs(o64["logit"]).max())
    for k in ("logit", "loss", "dlogit", "q1", "q", "dq"):
        _check(k, _h(rec[k]), o64[k], o32[k])
    _check("mean_logit", _h(rec["mean_logit"]), o64["mean_logit"], o32["mean_logit"], floor_scale=lmax)
    _check("I_cont", rec["I_cont"].item(), o64["I_cont"], o32["I_cont"])
    _check("I_disc", rec["I_disc"].item(), o64["I_disc"], o32["I_disc"], tol=O.ce_bound(o64["I_disc"]))
    # the D head alone gives the same logits, losses and dlogit bit for bit, and leaves the Q outputs out
    rec_d = K.info_head_fwd(fd, par[:2] + [None] * 4, targets, scale=scale)
    for k in ("logit", "loss", "mean_logit", "dlogit"):
        assert torch.equal(rec_d[k], rec[k]), k
    assert rec_d["q"] is None and rec_d["I_disc"].item() == 0.0 and rec_d["I_cont"].item() == 0.0
    # backward
    b64 = O.head_bwd(f, p, o64["dlogit"], o64["q1"], o64["dq"])
    b32 = O.head_bwd(f, p, o32["dlogit"], o32["q1"], o32["dq"], dtype=np.float32)
    nan = [torch.full_like(t, float("nan")) for t in par]
    df = K.info_head_bwd(par, rec, grads=[None, None] + nan[2:])               # phase 0: the Q gradients and df
    assert df.shape == (M * S, 1, 1, E)
    _check("df", _h(df).reshape(-1, E), b64["df"], b32["df"])
    for k, g in zip(NAMES[2:], nan[2:]):
        _check("d" + k, _h(g), b64[k], b32[k])
    assert all(bool(torch.isnan(g).all()) for g in nan[:2])                      # not asked for: not touched
    df_only = K.info_head_bwd(par, rec)                                          # neither
    assert torch.equal(df_only, df)
    both = [torch.full_like(t, float("nan")) for t in par]
    assert torch.equal(K.info_head_bwd(par, rec, grads=both), df)                # both groups at once
    for g, h in zip(both[2:], nan[2:]):
        assert torch.equal(g, h)
    d64 = O.head_bwd(f, p, o64["dlogit"])
    d32 = O.head_bwd(f, p, o32["dlogit"], dtype=np.float32)
    nan_d = [torch.full_like(t, float("nan")) for t in par[:2]]
    df_d = K.info_head_bwd(par[:2] + [None] * 4, rec_d, grads=nan_d + [None] * 4)   # phase 1: the D-head gradients and df
    _check("df (D head)", _h(df_d).reshape(-1, E), d64["df"], d32["df"])
    for k, g, b in zip(NAMES[:2], nan_d, both[:2]):
        _check("d" + k, _h(g), d64[k], d32[k])
        assert torch.equal(g, b)
    # two runs of every launch agree bit for bit
    rec2 = K.info_head_fwd(fd, par, targets, scale=scale, codes=(didx, dcont, V), lambda_I=lam)
    for k in ("logit", "loss", "mean_logit", "dlogit", "q1", "q", "dq", "I_disc", "I_cont"):
        assert torch.equal(rec2[k], rec[k]), k
    again = [torch.full_like(t, float("nan")) for t in par]
    assert torch.equal(K.info_head_bwd(par, rec2, grads=again), df)
    for g, h in zip(again, both):
        assert torch.equal(g, h)


@pytest.mark.parametrize("E", WIDTHS)
@pytest.mark.parametrize("M,S", ROWS)
def test_pass_matches_oracle(K, M, S, E):
    i = ROWS.index((M, S)) + WIDTHS.index(E)
    _run_pass(K, M, S, E, CODES[i % 3], seed=100 * M + 10 * S + E)


@pytest.mark.parametrize("S", (1, 2))
@pytest.mark.parametrize("code", CODES)
def test_every_code_layout(K, code, S):
    _run_pass(K, 5, S, 36, code, seed=7 + S)


@pytest.mark.parametrize("M,E,code", [(1, 4, CODES[2]), (5, 36, CODES[1]), (33, 1024, CODES[0])])
def test_q_head_alone(K, M, E, code):
    """K.info_q_fwd (no D head, no losses) gives the q of the full forward bit for bit, on a pitched f."""
    f, idx, cont, p = _case(M, 1, E, code, seed=M + E)
    fd, par = _pitched(f), _dev(p)
    rec = K.info_head_fwd(fd, par, [True], codes=(torch.from_numpy(idx).cuda(), _pitched(cont, 3), code[1]))
    q = K.info_q_fwd(fd, par[2:])
    assert q.shape == rec["q"].shape and torch.equal(q, rec["q"]) and torch.equal(K.info_q_fwd(fd, par[2:]), q)
    o64 = O.head_fwd(f, p, [True], 1.0, (idx, cont, code[1]))
    o32 = O.head_fwd(f, p, [True], 1.0, (idx, cont, code[1]), dtype=np.float32)
    _check("q", _h(q), o64["q"], o32["q"])


def test_supported_range(K):
    ok = K.info_head_supported
    assert ok(1, 128, 1024, 1, 10, 2) and ok(2, 128, 1024) and ok(1, 1, 4, 3, 2, 1) and ok(2, 5, 36, 2, 3, 3) and ok(1, 1, 4096, 6, 10, 4)
    assert not ok(1, 5, 6) and not ok(1, 5, 0) and not ok(1, 5, 4100) and not ok(3, 5, 36) and not ok(0, 5, 36) and not ok(1, 0, 36)
    assert not ok(1, 5, 36, 6, 10, 5) and not ok(1, 5, 36, 1, 10, 0) and not ok(1, 5, 36, H=256)


def test_saturated_logits(K):
    """Logits at +-200: the loss is finite (0 or 200) and the gradient saturates at 0 or +-scale / M."""
    E = 4
    f = np.array([[1.0] * E, [-100.0] * E, [1.0] * E, [-100.0] * E])
    p = {"wd": np.full(E, 50.0), "bd": np.zeros(1)}
    for targets in ([True, False], [False, True]):
        o = O.head_fwd(f, p, targets, 0.5)
        rec = K.info_head_fwd(_pitched(f), [torch.full((E,), 50.0).cuda(), torch.zeros(1).cuda()] + [None] * 4, targets, scale=0.5)
        logit, loss, d = _h(rec["logit"]), _h(rec["loss"]), _h(rec["dlogit"])
        assert np.allclose(logit, [200, -200, 200, -200], rtol=1e-6) and np.isfinite(loss).all() and np.isfinite(d).all()
        np.testing.assert_allclose(loss, o["loss"], rtol=1e-6)
        np.testing.assert_allclose(d, o["dlogit"], rtol=1e-6, atol=1e-30)
        sat = np.array([0.0, -0.25, 0.25, 0.0]) if targets[0] else np.array([0.25, 0.0, 0.0, -0.25])
        np.testing.assert_allclose(d, sat, atol=1e-30)


def _pow2(r, shape, lo=-2, hi=1):
    return (r.choice([-1.0, 1.0], shape) * 2.0 ** r.randint(lo, hi + 1, shape)).astype(np.float64)


def test_exact_sums(K):
    """Small-integer features and power-of-two weights: every product and every float64 sum is exact, so logit, q and df equal the
    oracle in the kernels' number formats (f32=True) bit for bit, whatever the order of summation."""
    M, S, E, (Dd, V, Cc) = 5, 2, 36, CODES[1]
    Qd, rows = Dd * V + Cc, M * S
    r = np.random.RandomState(3)
    f = r.randint(-8, 9, (rows, E)).astype(np.float64)
    p = {"wd": _pow2(r, (E,)), "bd": np.array([3.0]), "w1": _pow2(r, (E, H)), "b1": r.randint(-4, 5, (H,)).astype(np.float64),
         "w2": _pow2(r, (H, Qd)), "b2": r.randint(-4, 5, (Qd,)).astype(np.float64)}
    idx, cont = r.randint(0, V, (rows, Dd)).astype(np.int64), r.randint(-2, 3, (rows, Cc)).astype(np.float64)
    o = O.head_fwd(f, p, [True, False], 0.5, (idx, cont, V), 1.0, f32=True)
    fd, par = _pitched(f), _dev(p)
    rec = K.info_head_fwd(fd, par, [True, False], scale=0.5, codes=(torch.from_numpy(idx).cuda(), _pitched(cont, 1), V))
    for k in ("logit", "q1", "q"):
        assert np.array_equal(_h(rec[k]).astype(np.float64), o[k]), k
    dlogit = (r.randint(-3, 4, (rows,)) / 16.0).astype(np.float64)
    q1 = r.randint(-6, 7, (rows, H)).astype(np.float64)
    dq = (r.randint(-3, 4, (rows, Qd)) / 8.0).astype(np.float64)
    b = O.head_bwd(f, p, dlogit, q1, dq, f32=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()      # noqa: E731
    grads = [torch.full_like(x, float("nan")) for x in par]
    df = K.info_head_bwd(par, rec, grads=grads, dlogit=t(dlogit), q1=t(q1), dq=t(dq))
    assert np.array_equal(_h(df).reshape(rows, E).astype(np.float64), b["df"])
    for k, g in zip(NAMES, grads):
        got = _h(g).astype(np.float64).reshape(b[k].shape)
        if k == "w1":     # a^T dq1 multiplies two 24-bit numbers (both hold 0.01f factors): its float64 sums are not exact, one ulp is allowed
            np.testing.assert_allclose(got, b[k], rtol=2.0 ** -23, atol=0)
        else:
            assert np.array_equal(got, b[k]), k


@pytest.mark.parametrize("Dd,V,Cc,Nz", [(1, 10, 2, 62), (2, 3, 3, 5), (2, 3, 3, 7), (3, 2, 1, 0)])     # widths 74, 14 (% 4 = 2), 16, 7
def test_latent_packing(K, Dd, V, Cc, Nz):
    from src.ops.lib import load_library
    N, L = 6, Dd * V + Cc + Nz
    r = np.random.RandomState(L)
    idx = r.randint(0, V, (N, Dd)).astype(np.int64)
    idx[0, 0], idx[1, Dd - 1] = V - 1, 0
    cont = r.uniform(-1, 1, (N, Cc)).astype(np.float32)
    z = r.randn(N, Nz).astype(np.float32)
    want = O.pack_latent(idx, cont, z, V)
    di, dc, dz = torch.from_numpy(idx).cuda(), _pitched(cont, 2), (_pitched(z, 5) if Nz else torch.zeros((N, 0)).cuda())
    out = K.info_latent(di, dc, dz, V)
    assert out.shape == (N, 1, 1, L) and out._base.shape == (N, 1, 1, (L + 3) // 4 * 4)
    assert np.array_equal(_h(out._base).reshape(N, -1), want)                    # padded lanes exactly 0
    assert torch.equal(K.info_latent(di, dc, dz, V)._base, out._base)
    # a wider pitch on a NaN-filled buffer through the C ABI: every element is written
    ld = (L + 3) // 4 * 4 + 4
    buf = torch.full((N, ld), float("nan")).cuda()
    lib = load_library()
    p = lambda t_: C.c_void_p(t_.data_ptr())                                    # noqa: E731
    rc = lib.mi_info_latent(N, Dd, V, Cc, Nz, p(di), p(dc), dc.stride(0), p(dz) if Nz else None, dz.stride(0) if Nz else 0, p(buf), ld, None)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(_h(buf), O.pack_latent(idx, cont, z, V, ld=ld))
    # an index outside [0, V): that code's columns stay 0, nothing else changes
    bad = idx.copy()
    bad[2, 0], bad[3, Dd - 1] = V, -1
    got = _h(K.info_latent(torch.from_numpy(bad).cuda(), dc, dz, V)._base).reshape(N, -1)
    assert np.array_equal(got, O.pack_latent(bad, cont, z, V))


def test_refusals_launch_nothing(K):
    """E % 4 != 0, S = 3, a code wider than 64, a null required pointer: a non-zero return, and the outputs keep their NaN."""
    from src.ops.lib import load_library
    lib = load_library()
    M, E, (Dd, V, Cc) = 5, 36, CODES[1]
    f, idx, cont, pp = _case(M, 1, E, CODES[1], 1)
    fd, par = _pitched(f), _dev(pp)
    didx, dcont = torch.from_numpy(idx).cuda(), torch.from_numpy(cont).float().cuda()
    outs = {k: torch.full(s, float("nan")).cuda() for k, s in
            (("logit", (3 * M,)), ("dlogit", (3 * M,)), ("q1", (3 * M, H)), ("q", (3 * M, 80)), ("dq", (3 * M, 80)), ("out6", (6,)),
             ("df", (3 * M, E)), ("dq1", (3 * M, H)))}
    ws = torch.full((12 * M,), float("nan"), dtype=torch.float64).cuda()
    p = lambda t_: C.c_void_p(0 if t_ is None else t_.data_ptr())               # noqa: E731
    ptrs = lambda ts: (C.c_void_p * 6)(*[0 if t_ is None else t_.data_ptr() for t_ in ts])   # noqa: E731

    def fwd(S=1, M_=M, E_=E, Dd_=Dd, V_=V, Cc_=Cc, f_=fd, par_=par, logit=outs["logit"], ws_=ws, idx_=didx):
        return lib.mi_info_head_fwd(S, M_, E_, H, p(f_), f_.stride(0) if f_ is not None else 0, ptrs(par_), 1, 0, 1.0, Dd_, V_, Cc_, p(idx_),
                                    p(dcont), dcont.stride(0), 1.0, p(logit), p(outs["dlogit"]), p(outs["q1"]), p(outs["q"]), p(outs["dq"]),
                                    p(ws_), p(outs["out6"]), None)

    def bwd(S=1, E_=E, Qd=Dd * V + Cc, f_=fd, dlogit=outs["dlogit"], df=outs["df"], grads=None, dq1=outs["dq1"]):
        return lib.mi_info_head_bwd(S, M, E_, H, Qd, p(f_), fd.stride(0), ptrs(par), p(dlogit), p(outs["q1"]), p(outs["dq"]), p(df), E,
                                    p(dq1), grads, None)
    assert fwd(E_=6) != 0 and fwd(S=3) != 0 and fwd(Dd_=8, V_=8, Cc_=1) != 0 and fwd(Cc_=0) != 0 and fwd(M_=0) != 0
    assert fwd(f_=None) != 0 and fwd(logit=None) != 0 and fwd(ws_=None) != 0 and fwd(idx_=None) != 0 and fwd(par_=par[:2] + [None] * 4) != 0
    assert bwd(E_=6) != 0 and bwd(S=3) != 0 and bwd(Qd=65) != 0 and bwd(f_=None) != 0 and bwd(dlogit=None) != 0 and bwd(df=None) != 0
    nan_g = [torch.full_like(t_, float("nan")) for t_ in par]
    assert bwd(grads=ptrs(nan_g), dq1=None) != 0 and bwd(grads=ptrs(nan_g[:1] + [None] * 5)) != 0 and bwd(grads=ptrs([None] * 2 + nan_g[2:5] + [None])) != 0
    assert lib.mi_info_latent(M, Dd, V, Cc, 5, p(didx), p(dcont), Cc, p(dcont), 1, p(outs["q"]), 80, None) != 0        # ldz < Nz
    assert lib.mi_info_latent(M, Dd, V, Cc, 5, p(didx), p(dcont), Cc, p(dcont), 5, p(outs["q"]), 8, None) != 0         # ld < the latent width
    assert lib.mi_info_latent(M, Dd, V, Cc, 5, None, p(dcont), Cc, p(dcont), 5, p(outs["q"]), 80, None) != 0
    torch.cuda.synchronize()
    for k, t_ in list(outs.items()) + [("ws", ws)] + [(f"g{i}", g) for i, g in enumerate(nan_g)]:
        assert bool(torch.isnan(t_).all()), k
    with pytest.raises(RuntimeError):
        K.info_head_fwd(torch.from_numpy(f).float(), par, [True])                 # a CPU tensor raises
    with pytest.raises(RuntimeError):
        K.info_head_fwd(torch.zeros(5, 6).cuda(), par, [True])
