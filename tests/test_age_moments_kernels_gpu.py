"""The AGE latent-moment kernels (csrc/age_ops.hip) through their C ABI against the float64 oracle (tests/_age_oracle.py, itself checked
against torch's float64 autograd in tests/test_age_moments_cpu.py).

Tolerance, per quantity: max|hip - f64| <= 4 * max|oracle_f32 - f64| + 1e-6 * max|f64| -- the float32 run of the same oracle is the
yardstick, the `_check` rule of tests/test_info_head_kernels_gpu.py (a mean over columns takes the columns' own scale as its floor, as
the mean logit does there).  The inputs are standard-normal rows scaled by 3: the column variances stay far from 0 (asserted).
Every pitched input sits in a NaN-filled buffer, every output starts as NaN."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _age_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
RPB = 4                                                        # rows per workgroup of the two row kernels
MS = (2, 3, 5, RPB, RPB + 1, 2 * RPB + 1, 33)                  # the smallest | odd | one row tile | one more | two tiles plus one | many
LS = (2, 6, 10, 128, 130)                                      # below a wave | the tiny model's | the shipped | two lanes' worth | ragged over 64
# segments, KL coefficients, reconstruction mode and weight per segment, dz_ext per segment, normalisation
CONFIGS = [
    dict(S=1, c=(1.0,), modes=(0,), w=(0.0,), ext=(False,), norm=True),
    dict(S=1, c=(1.0,), modes=(2,), w=(1000.0,), ext=(False,), norm=True),
    dict(S=2, c=(1.0, -1.0), modes=(0, 1), w=(0.0, 1000.0), ext=(True, False), norm=True),
    dict(S=2, c=(1.0, 0.0), modes=(2, 0), w=(3.0, 0.0), ext=(False, False), norm=True),
    dict(S=2, c=(0.0, 1.0), modes=(1, 2), w=(2.0, 5.0), ext=(False, True), norm=True),
    dict(S=2, c=(1.0, -1.0), modes=(0, 1), w=(0.0, 7.0), ext=(True, False), norm=False),
    dict(S=1, c=(1.0,), modes=(1,), w=(2.0,), ext=(True,), norm=False),
    dict(S=2, c=(1.0, -1.0), modes=(2, 2), w=(1.5, 0.5), ext=(True, True), norm=False),
]


@pytest.fixture(scope="module")
def lib():
    from src.ops.lib import load_library
    return load_library()


def _stream():
    from src.ops import functional as K
    return K._stream()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _pitched(x, ld):
    """x [rows, L] as a view of a NaN-filled [rows, ld] device buffer."""
    x = np.asarray(x, dtype=np.float32)
    buf = torch.full((x.shape[0], ld), float("nan"))
    buf[:, :x.shape[1]] = torch.from_numpy(x)
    return buf.cuda()


def _pitches(L):
    up = (L + 3) // 4 * 4
    return (L, up if up > L else L + 4, L + 3)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype)


def _h(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _check(name, got, f64, f32, floor_scale=None):
    got, f64, f32 = (np.asarray(a, dtype=np.float64) for a in (got, f64, f32))
    scale = float(np.abs(f64).max()) if floor_scale is None else floor_scale
    tol = 4.0 * float(np.abs(f32 - f64).max()) + 1e-6 * scale
    err = float(np.abs(got - f64).max())
    print(f"{name}: max|hip - f64| {err:.3e}  max|f32 - f64| {float(np.abs(f32 - f64).max()):.3e}  scale {scale:.3e}  tol {tol:.3e}")
    assert got.shape == f64.shape and np.isfinite(got).all(), name
    assert err <= tol, (name, err, tol)


def _case(M, L, cfg, seed, zero_row=None):
    r = np.random.RandomState(seed)
    rows = cfg["S"] * M
    e = (r.randn(rows, L) * 3).astype(np.float32)
    if zero_row is not None:
        e[zero_row] = 0.0
    t = r.randn(M, L)
    t = (t / np.sqrt((t * t).sum(axis=1, keepdims=True))).astype(np.float32)
    dz = [(r.randn(M, L) * 0.01).astype(np.float32) if x else None for x in cfg["ext"]]
    return e, t, dz


def _forward(lib, e_buf, S, M, L, ld, cfg, t_buf, ldt, ws=None, stats=True):
    rows, norm_on = S * M, cfg["norm"]
    modes = (list(cfg["modes"]) + [0])[:2] if stats else [0, 0]
    out = {"z": _nan(rows, L) if norm_on else None, "norm": _nan(rows) if norm_on else None,
           "mu": _nan(S, L) if stats else None, "var": _nan(S, L) if stats else None, "out4": _nan(S, 4) if stats else None}
    if ws is None and any(modes):
        ws = _nan(int(lib.mi_age_moments_workspace_doubles(S, M)), dtype=torch.float64)
    rc = lib.mi_age_moments_fwd(S, M, L, _p(e_buf), ld, int(norm_on), _p(out["z"]), _p(out["norm"]), int(stats), modes[0], modes[1],
                                _p(t_buf) if any(modes) else None, ldt if any(modes) else 0, _p(out["mu"]), _p(out["var"]), _p(out["out4"]),
                                _p(ws) if any(modes) else None, _stream())
    out["rc"], out["modes"] = rc, modes
    return out


def _backward(lib, fw, e_buf, S, M, L, ld, cfg, t_buf, ldt, dz_bufs, ldx, ldde):
    c, w = (list(cfg["c"]) + [0.0])[:2], (list(cfg["w"]) + [0.0])[:2]
    de = _nan(S * M, ldde)
    z, ldz = (fw["z"], L) if cfg["norm"] else (e_buf, ld)
    rc = lib.mi_age_moments_bwd(S, M, L, _p(z), ldz, _p(fw["norm"]), _p(fw["mu"]), _p(fw["var"]), c[0], c[1], fw["modes"][0], fw["modes"][1],
                                w[0], w[1], _p(t_buf) if any(fw["modes"]) else None, ldt if any(fw["modes"]) else 0, _p(dz_bufs[0]),
                                _p(dz_bufs[1]), ldx if any(d is not None for d in dz_bufs) else 0, _p(de), ldde, _stream())
    return rc, de


def _run(lib, M, L, cfg, ld, seed, zero_row=None, forward_only=False):
    """Forward and backward of one case against the oracle; returns (forward outputs, de, the oracle's de in float64 and float32)."""
    S = cfg["S"]
    ldt, ldx, ldde = L + 1, L + 2, (ld + 5 if ld % 2 else ld + 4)
    assert ldde != ld
    for attempt in range(2000):                             # redrawn until the columns are well conditioned: few rows leave some column flat
        e, t, dz = _case(M, L, cfg, seed + 7919 * attempt, zero_row)
        o64 = O.fwd(e, S, cfg["norm"], cfg["modes"], t)
        if forward_only or (o64["var"] > 2e-3).all():
            break
    o32 = O.fwd(e, S, cfg["norm"], cfg["modes"], t, dtype=np.float32)
    assert forward_only or (o64["var"] > 1e-3).all()                                    # log var and 1 / var are well conditioned
    e_buf, t_buf = _pitched(e, ld), _pitched(t, ldt)
    dz_bufs = [None if d is None else _pitched(d, ldx) for d in (dz + [None])[:2]]
    fw = _forward(lib, e_buf, S, M, L, ld, cfg, t_buf, ldt)
    assert fw["rc"] == 0, lib.mi_last_error()
    tag = f"M={M} L={L} ld={ld} S={S} modes={cfg['modes']} norm={cfg['norm']}"
    if cfg["norm"]:
        _check(f"{tag} z", _h(fw["z"]), o64["z"], o32["z"])
        _check(f"{tag} norm", _h(fw["norm"]), o64["norm"], o32["norm"])
    _check(f"{tag} mu", _h(fw["mu"]), o64["mu"], o32["mu"])
    _check(f"{tag} var", _h(fw["var"]), o64["var"], o32["var"])
    if forward_only:                                        # z, norm, mu and var need no log var and no 1 / var
        return fw, None, None, None
    out4 = _h(fw["out4"])
    _check(f"{tag} kl", out4[:, 0], o64["kl"], o32["kl"])
    _check(f"{tag} mean_mu", out4[:, 1], o64["mean_mu"], o32["mean_mu"], floor_scale=float(np.abs(o64["mu"]).max()))
    _check(f"{tag} mean_var", out4[:, 2], o64["mean_var"], o32["mean_var"])
    _check(f"{tag} recon", out4[:, 3], o64["recon"], o32["recon"], floor_scale=max(float(np.abs(o64["recon"]).max()), 1.0 if 1 in cfg["modes"] else 0.0))
    d64, _ = O.bwd(o64, cfg["c"], cfg["w"], dz)
    d32, _ = O.bwd(o32, cfg["c"], cfg["w"], dz)
    rc, de = _backward(lib, fw, e_buf, S, M, L, ld, cfg, t_buf, ldt, dz_bufs, ldx, ldde)
    assert rc == 0, lib.mi_last_error()
    de = _h(de)
    assert (de[:, L:] == 0).all(), tag                                                  # pad columns are written, as zero
    if zero_row is None:
        _check(f"{tag} c={cfg['c']} w={cfg['w']} de", de[:, :L], d64, d32)
    return fw, de, d64, d32


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("M", MS)
def test_forward_and_backward_match_the_oracle(lib, M, L):
    """Every configuration at this shape, the pitch rotating through ld in {L, the next multiple of 4, L + 3}; ldde != ld throughout."""
    for i, cfg in enumerate(CONFIGS):
        # on the sphere var_j is about 1 / L = 8e-3: with L >= 128 fewer than 9 rows always leave a column under 1e-3, where log var and
        # 1 / var are not conditioned as the tolerance assumes; there z, norm, mu and var alone are checked
        few = cfg["norm"] and L >= 128 and M < 2 * RPB + 1
        _run(lib, M, L, cfg, _pitches(L)[(i + M + L) % 3], seed=1000 * M + 10 * L + i, forward_only=few)


@pytest.mark.parametrize("ld_i", (0, 1, 2))
def test_every_pitch_at_the_shipped_and_tiny_widths(lib, ld_i):
    for L in (6, 10):
        for i, cfg in enumerate(CONFIGS):
            _run(lib, 5, L, cfg, _pitches(L)[ld_i], seed=77 + i)


@pytest.mark.parametrize("cfg_i", (2, 4))
def test_zero_row(lib, cfg_i):
    """z = 0 exactly for an all-zero row; its de is finite and the oracle's g / 1e-12 to 1e-6 of the row's largest element.  The other
    rows keep the tolerance of every other case."""
    cfg, M, L = CONFIGS[cfg_i], 6, 10
    row = 2 * M - 2                                                                     # in segment 1, which carries a reconstruction term
    fw, de, d64, d32 = _run(lib, M, L, cfg, 12, seed=5, zero_row=row)
    assert bool((fw["z"][row] == 0).all()) and float(fw["norm"][row]) == 0.0
    assert np.isfinite(de).all()
    err, scale = float(np.abs(de[row, :L] - d64[row]).max()), float(np.abs(d64[row]).max())
    print(f"zero row: max|de - g / eps| {err:.3e}, max|g / eps| {scale:.3e}")
    assert scale > 1e6 and err <= 1e-6 * scale
    rest = [i for i in range(2 * M) if i != row]
    _check("zero-row case, the other rows' de", de[rest, :L], d64[rest], d32[rest])


def test_prior_normalisation_alone(lib):
    """want_stats = 0: one launch that normalises the rows (the prior draw); a single row is accepted there."""
    for M, L, ld in ((1, 6, 6), (5, 10, 13), (9, 130, 132)):
        e = (np.random.RandomState(M).randn(M, L) * 3).astype(np.float32)
        cfg = dict(S=1, modes=(0,), norm=True)
        fw = _forward(lib, _pitched(e, ld), 1, M, L, ld, cfg, None, 0, stats=False)
        assert fw["rc"] == 0, lib.mi_last_error()
        o64 = e.astype(np.float64) / np.maximum(np.sqrt((e.astype(np.float64) ** 2).sum(axis=1, keepdims=True)), 1e-12)
        o32 = e / np.maximum(np.sqrt((e * e).sum(axis=1, keepdims=True)), np.float32(1e-12))
        _check(f"prior M={M} L={L} z", _h(fw["z"]), o64, o32)
        assert float((fw["z"].double().pow(2).sum(dim=1) - 1).abs().max()) < 1e-6


def test_two_calls_and_a_poisoned_workspace_give_the_same_bits(lib):
    cfg, M, L, ld = CONFIGS[4], 9, 130, 133
    e, t, dz = _case(M, L, cfg, 11)
    e_buf, t_buf = _pitched(e, ld), _pitched(t, L + 1)
    dz_bufs = [None if d is None else _pitched(d, L + 2) for d in dz]
    n = int(lib.mi_age_moments_workspace_doubles(2, M))
    runs = []
    for ws in (_nan(n, dtype=torch.float64), _nan(n, dtype=torch.float64), torch.full((n,), 1e300, device="cuda", dtype=torch.float64),
               torch.randn(n, device="cuda", dtype=torch.float64)):
        fw = _forward(lib, e_buf, 2, M, L, ld, cfg, t_buf, L + 1, ws=ws)
        rc, de = _backward(lib, fw, e_buf, 2, M, L, ld, cfg, t_buf, L + 1, dz_bufs, L + 2, ld + 3)
        assert fw["rc"] == 0 and rc == 0
        runs.append([fw[k] for k in ("z", "norm", "mu", "var", "out4")] + [de])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert all(bool(torch.isfinite(a).all()) for a in runs[0])


def test_pad_columns_of_e_are_never_read_and_wrappers_agree(lib):
    """The NaN pads of e, t and dz_ext reach no output (every case above already runs on such buffers); the Python wrappers give the C
    ABI's bits on the encoder's NHWC layout [rows, 1, 1, L] with pitch 12."""
    from src.ops import functional as K
    cfg, M, L = CONFIGS[2], 5, 10
    e, t, dz = _case(M, L, cfg, 3)
    e_buf, t_buf, dz_buf = _pitched(e, 12), _pitched(t, 12), _pitched(dz[0], 12)
    fw = _forward(lib, e_buf, 2, M, L, 12, cfg, t_buf, 12)
    rc, de = _backward(lib, fw, e_buf, 2, M, L, 12, cfg, t_buf, 12, [dz_buf, None], 12, 12)
    assert fw["rc"] == 0 and rc == 0
    rec = K.age_moments_fwd(e_buf.view(2 * M, 1, 1, 12)[..., :L], 2, normalize=True, recon=(None, "cosine"), target=t_buf[:, :L])
    got = K.age_moments_bwd(rec, c=cfg["c"], w=cfg["w"], dz_ext=(dz_buf.view(M, 1, 1, 12)[..., :L], None))
    assert got.shape == (2 * M, 1, 1, L) and got.stride(0) == 12
    assert torch.equal(got.reshape(2 * M, L), de[:, :L]) and torch.equal(rec["z"], fw["z"]) and torch.equal(rec["kl"], fw["out4"][:, 0])
    assert torch.equal(rec["recon"], fw["out4"][:, 3]) and torch.equal(rec["mean_var"], fw["out4"][:, 2])
    assert torch.equal(K.age_normalize(e_buf[:, :L]), fw["z"])
    with pytest.raises(RuntimeError):
        K.age_moments_fwd(e_buf[:1, :L], 1)                                             # M = 1: no unbiased variance
    with pytest.raises(RuntimeError):
        K.age_moments_fwd(e_buf.cpu()[:, :L], 2)


@pytest.mark.parametrize("S,M,L", [(1, 1, 6), (1, 5, 0), (1, 5, 513), (3, 5, 6)])
def test_refusals_launch_nothing(lib, S, M, L):
    assert lib.mi_age_moments_supported(S, M, L) == 0 and lib.mi_last_error()
    assert lib.mi_age_moments_supported(min(S, 2), max(M, 2), min(max(L, 1), 512)) == 1
    rows, Lb = max(S * M, 1), max(L, 1)
    e = torch.randn(rows, Lb, device="cuda")
    z, norm, mu, var, out4, de = _nan(rows, Lb), _nan(rows), _nan(max(S, 1), Lb), _nan(max(S, 1), Lb), _nan(max(S, 1), 4), _nan(rows, Lb)
    rc = lib.mi_age_moments_fwd(S, M, L, _p(e), Lb, 1, _p(z), _p(norm), 1, 0, 0, None, 0, _p(mu), _p(var), _p(out4), None, _stream())
    assert rc != 0 and lib.mi_last_error()
    rc = lib.mi_age_moments_bwd(S, M, L, _p(e), Lb, None, _p(mu), _p(var), 1.0, 0.0, 0, 0, 0.0, 0.0, None, 0, None, None, 0, _p(de), Lb, _stream())
    assert rc != 0 and lib.mi_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (z, norm, mu, var, out4, de))


@pytest.mark.parametrize("B,C,HW,ld", [(1, 1, 1, 1), (5, 1, 784, 4), (3, 3, 50, 4), (2, 5, 7, 7), (512, 1, 784, 4)])
def test_image_mse_is_exact_in_order_and_repeatable(lib, B, C, HW, ld):
    """mi_age_image_mse against float64: the loss within a float32 rounding (its sums are fp64), the gradient within a float32 rounding
    per element, pad lanes written as 0 and never read, a poisoned workspace, the same bits on every run.  The last shape has more
    pixels than the grid's 256 x 256 threads: the strided walk."""
    r = np.random.RandomState(B + HW)
    pred = r.uniform(-1, 1, (B * HW, C)).astype(np.float32)
    target = r.uniform(-1, 1, (B, C, HW)).astype(np.float32)
    d = pred.astype(np.float64).reshape(B, HW, C) - target.astype(np.float64).transpose(0, 2, 1)
    want, gscale = float((d * d).mean()), 10.0
    pbuf, tbuf = _pitched(pred, ld), torch.from_numpy(target).cuda()
    n = int(lib.mi_age_image_mse_workspace_doubles(B, HW))
    assert 1 <= n <= 256
    runs = []
    for ws in (_nan(n, dtype=torch.float64), torch.full((n,), 1e300, device="cuda", dtype=torch.float64), _nan(n, dtype=torch.float64)):
        loss, dp = _nan(1), _nan(B * HW, ld)
        assert lib.mi_age_image_mse(B, C, HW, _p(pbuf), ld, _p(tbuf), _p(loss), _p(dp), gscale, _p(ws), _stream()) == 0, lib.mi_last_error()
        runs.append((loss, dp))
    for loss, dp in runs[1:]:
        assert torch.equal(loss.view(torch.int32), runs[0][0].view(torch.int32)) and torch.equal(dp.view(torch.int32), runs[0][1].view(torch.int32))
    loss, dp = float(runs[0][0]), _h(runs[0][1])
    print(f"B={B} C={C} HW={HW} ld={ld}: loss {loss:.9g} float64 {want:.9g}")
    assert abs(loss - want) <= 2.0 ** -23 * want
    gref = gscale * 2.0 * d.reshape(B * HW, C) / (B * C * HW)
    assert (dp[:, C:] == 0).all() and np.abs(dp[:, :C] - gref).max() <= 2.0 ** -23 * np.abs(gref).max()
    loss_only = _nan(1)
    assert lib.mi_age_image_mse(B, C, HW, _p(pbuf), ld, _p(tbuf), _p(loss_only), None, gscale, _p(_nan(n, dtype=torch.float64)), _stream()) == 0
    assert torch.equal(loss_only, runs[0][0])
    assert lib.mi_age_image_mse(B, C, HW, _p(pbuf), C - 1, _p(tbuf), _p(loss_only), None, gscale, _p(runs[0][1]), _stream()) != 0 and lib.mi_last_error()
