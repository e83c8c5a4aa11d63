"""float64 numpy oracle of csrc/info_head.hip: the InfoGAN's latent packing, the two heads on the shared feature with their losses, and
the heads' backward (reference src/models/info_gan.py:37-43, 64-133).

Parameters are a dict with the kernels' layout (weights input-major): wd [E], bd [1], w1 [E, 128], b1 [128], w2 [128, Qd], b2 [Qd],
Qd = Dd * V + Cc.  q's first Dd * V columns are [V][Dd]: value v of code d is column v * Dd + d.  The LeakyReLU slope is torch's
default 0.01.

`dtype=np.float32` runs the same formulas in float32 arithmetic throughout: the yardstick of the kernel tests' tolerance
(max|hip - f64| <= 4 * max|oracle_f32 - f64| + 1e-6 * max|f64|, as tests/test_latent_disc_ln_kernels_gpu.py).
`f32=True` (float64 arithmetic only) follows the kernels' number formats: every TENSOR is float32 (the slope, the activation
a = LeakyReLU(f), logit, q1, q, dlogit, dq, dq1, df and the gradients are rounded to float32 where the kernels store or form them),
every sum is float64 and rounded once.  With operands whose sums are exact in float64 (small integers, powers of two) the result is
then the kernels' bit for bit, whatever the order of summation.  The default is plain float64 arithmetic, what torch computes in
float64.
"""
import numpy as np

SLOPE = 0.01

# Cross-entropy bound of tests/test_info_head_kernels_gpu.py.  The other quantities take the bound tests/test_latent_disc_ln_kernels_gpu.py
# uses for fp32 outputs of fp64-accumulated sums; the mean cross-entropy has no counterpart there, so its bound is MEASURED on the
# reference: on the `heads` record of tests/golden/infogan_kats.npz (tools/gen_golden_infogan.py) the reference's float32 heads give
# I_disc = 2.223496675491333 where its float64 heads give 2.2234966619453673, a deviation of 1.354596568248212e-08 (relative 6.09e-09;
# tests/test_info_head_cpu.py::test_ce_bound_is_the_measured_one recomputes it from the stored numbers).  The kernels sum in another
# order than torch does, so the bound is 4 times that, relative to the loss, plus the rounding of the float32 the kernel stores
# (half an ulp, 2^-24 relative).
CE_REL_MEASURED = 1.354596568248212e-08 / 2.2234966619453673
CE_REL_BOUND = 4 * CE_REL_MEASURED


def ce_bound(ref):
    """|I_disc - ref| allowed against the oracle's float64 value."""
    return (CE_REL_BOUND + 2.0 ** -24) * abs(float(ref))


def _r(x, f32, dt=np.float64):
    return np.asarray(x, dtype=np.float32).astype(dt) if f32 else np.asarray(x, dtype=dt)


def _slope(f32, dt=np.float64):
    return dt(np.float32(SLOPE)) if f32 else dt(SLOPE)


def leaky(x, f32=False, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    return _r(np.where(x > 0, x, _slope(f32, dtype) * x), f32, dtype)


def leaky_d(x, f32=False, dtype=np.float64):
    return np.where(np.asarray(x, dtype=dtype) > 0, dtype(1.0), _slope(f32, dtype))


def pack_latent(idx, cont, z, V, ld=None):
    """[N, ld]: ones at v * Dd + d for v = idx[n, d] (none for an index outside [0, V)), cont, z, zeros up to ld (default: the width
    rounded up to 4)."""
    idx = np.asarray(idx)
    N, Dd = idx.shape
    Cc, Nz = cont.shape[1], z.shape[1]
    L = Dd * V + Cc + Nz
    ld = (L + 3) // 4 * 4 if ld is None else ld
    out = np.zeros((N, ld), dtype=np.float32)
    for n in range(N):
        for d in range(Dd):
            if 0 <= idx[n, d] < V:
                out[n, int(idx[n, d]) * Dd + d] = 1.0
    out[:, Dd * V:Dd * V + Cc] = cont
    out[:, Dd * V + Cc:L] = z
    return out


def bce_logits(x, t):
    return np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def _par(P, k, dt):
    return np.asarray(P[k], dtype=dt)


def head_fwd(f, P, targets, scale=1.0, codes=None, lambda_I=1.0, f32=False, dtype=np.float64):
    """f [rows, E]; targets: one bool per segment (equal segments).  -> dict: logit, loss [S], mean_logit [S], dlogit, and with
    codes = (idx [rows, Dd], cont [rows, Cc], V): q1, q, I_disc, I_cont, dq = lambda_I * d (I_disc + I_cont) / dq."""
    assert not (f32 and dtype != np.float64)
    dt = dtype
    f = np.asarray(f, dtype=dt)
    rows = f.shape[0]
    S = len(targets)
    M = rows // S
    a = leaky(f, f32, dt)
    out = {}
    logit = _r(a @ _par(P, "wd", dt) + _par(P, "bd", dt).reshape(-1)[0], f32, dt)
    t = np.repeat(np.array([1.0 if x else 0.0 for x in targets], dtype=dt), M)
    rl = bce_logits(logit, t)
    out["logit"] = logit
    out["loss"] = _r([rl[s * M:(s + 1) * M].sum() / dt(M) for s in range(S)], f32, dt)
    out["mean_logit"] = _r([logit[s * M:(s + 1) * M].sum() / dt(M) for s in range(S)], f32, dt)
    out["dlogit"] = _r(dt(scale) / dt(M) * (sigmoid(logit) - t), f32, dt)
    if codes is None:
        return out
    idx, cont, V = np.asarray(codes[0]), np.asarray(codes[1], dtype=dt), int(codes[2])
    Dd, Cc = idx.shape[1], cont.shape[1]
    q1 = leaky(_r(a @ _par(P, "w1", dt) + _par(P, "b1", dt), f32, dt), f32, dt)
    q = _r(q1 @ _par(P, "w2", dt) + _par(P, "b2", dt), f32, dt)
    lg = q[:, :Dd * V].reshape(rows, V, Dd)
    m = lg.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(lg - m).sum(axis=1, keepdims=True))                          # [rows, 1, Dd]
    onehot = np.zeros_like(lg)
    for n in range(rows):
        for d in range(Dd):
            if 0 <= idx[n, d] < V:
                onehot[n, int(idx[n, d]), d] = 1.0
    ce = lse[:, 0, :] - (lg * onehot).sum(axis=1)
    diff = q[:, Dd * V:] - cont
    dq = np.empty_like(q)
    dq[:, :Dd * V] = (dt(lambda_I) / dt(rows * Dd) * (np.exp(lg - lse) - onehot)).reshape(rows, Dd * V)
    dq[:, Dd * V:] = dt(lambda_I) * dt(2.0) * diff / dt(rows * Cc)
    out.update(q1=q1, q=q, I_disc=float(_r(ce.sum() / dt(rows * Dd), f32, dt)), I_cont=float(_r((diff * diff).sum() / dt(rows * Cc), f32, dt)),
               dq=_r(dq, f32, dt))
    return out


def head_bwd(f, P, dlogit, q1=None, dq=None, f32=False, dtype=np.float64):
    """-> dict: df, the D-head gradients wd, bd, and with q1 / dq the Q gradients w1, b1, w2, b2 (input-major, like P)."""
    assert not (f32 and dtype != np.float64)
    dt = dtype
    f = np.asarray(f, dtype=dt)
    dlogit = np.asarray(dlogit, dtype=dt)
    a = leaky(f, f32, dt)
    out = {"wd": _r(a.T @ dlogit, f32, dt), "bd": _r([dlogit.sum()], f32, dt)}
    acc = np.outer(dlogit, _par(P, "wd", dt))
    if dq is not None:
        q1, dq = np.asarray(q1, dtype=dt), np.asarray(dq, dtype=dt)
        dq1 = _r((dq @ _par(P, "w2", dt).T) * leaky_d(q1, f32, dt), f32, dt)
        acc = acc + dq1 @ _par(P, "w1", dt).T
        out.update(w1=_r(a.T @ dq1, f32, dt), b1=_r(dq1.sum(axis=0), f32, dt), w2=_r(q1.T @ dq, f32, dt), b2=_r(dq.sum(axis=0), f32, dt), dq1=dq1)
    out["df"] = _r(acc * leaky_d(f, f32, dt), f32, dt)
    return out


def make_params(E, Qd, seed, dtype=np.float64):
    """Random head parameters, float32-representable, at the scale of torch's default init."""
    r = np.random.RandomState(seed)
    def u(shape, fan):
        return (r.uniform(-1, 1, shape) / np.sqrt(fan)).astype(np.float32).astype(dtype)
    return {"wd": u((E,), E), "bd": u((1,), E), "w1": u((E, 128), E), "b1": u((128,), E), "w2": u((128, Qd), 128), "b2": u((Qd,), 128)}
