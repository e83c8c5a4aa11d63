"""numpy oracle of the AGE latent-moment operators (csrc/age_ops.hip; reference src/models/age.py:64-81, 90-144): the forward, the
losses and the ANALYTIC backward, in float64 by default and in float32 (`dtype=np.float32`: the same formulas with every array and
every intermediate in float32 -- what float32 arithmetic alone costs, the yardstick of the kernel tests' tolerance).
tests/test_age_moments_cpu.py checks the backward against torch's float64 autograd, which pins the eps semantics of F.normalize and
F.cosine_similarity as the installed torch computes them:
  normalize          z = e / max(||e||, 1e-12); clamp_min passes no gradient to the norm below eps, so de = g / eps there;
  cosine_similarity  each row is divided by its norm clamped at 1e-8 and the products are summed; the clamp is applied in place
                     outside the graph, so the norm's own derivative a / ||a|| (0 at a = 0) applies on both sides of the clamp."""
import numpy as np

NORM_EPS, COS_EPS = 1e-12, 1e-8
MODES = {None: 0, "none": 0, "cosine": 1, "mse": 2, 0: 0, 1: 1, 2: 2}


def _rownorm(x):
    return np.sqrt((x * x).sum(axis=1, keepdims=True))


def fwd(e, S=1, normalize=True, modes=(0, 0), t=None, dtype=np.float64):
    """e [S * M, L], t [M, L] -> dict: z, norm [rows], mu [S, L], var [S, L], kl [S], mean_mu [S], mean_var [S], recon [S]."""
    e = np.asarray(e, dtype=dtype)
    rows, L = e.shape
    M = rows // S
    modes = [MODES[m] for m in (list(modes) + [0])[:2]]
    out = {"S": S, "M": M, "L": L, "modes": modes, "normalize": normalize, "dtype": dtype}
    if normalize:
        n = _rownorm(e)
        z = e / np.maximum(n, dtype(NORM_EPS))
        out["norm"] = n[:, 0]
    else:
        z = e
    out["z"] = z
    out["t"] = None if t is None else np.asarray(t, dtype=dtype)
    for k in ("mu", "var"):
        out[k] = np.zeros((S, L), dtype=dtype)
    for k in ("kl", "mean_mu", "mean_var", "recon"):
        out[k] = np.zeros(S, dtype=dtype)
    for s in range(S):
        zs = z[s * M:(s + 1) * M]
        mu = zs.sum(axis=0) / dtype(M)
        var = ((zs - mu) ** 2).sum(axis=0) / dtype(M - 1)
        out["mu"][s], out["var"][s] = mu, var
        out["kl"][s] = (mu * mu + var - np.log(var)).sum() / dtype(L) / dtype(2)
        out["mean_mu"][s], out["mean_var"][s] = mu.sum() / dtype(L), var.sum() / dtype(L)
        if modes[s] == 1:
            tt = out["t"]
            cos = ((zs / np.maximum(_rownorm(zs), dtype(COS_EPS))) * (tt / np.maximum(_rownorm(tt), dtype(COS_EPS)))).sum(axis=1)
            out["recon"][s] = dtype(1) - cos.sum() / dtype(M)
        elif modes[s] == 2:
            out["recon"][s] = ((zs - out["t"]) ** 2).sum() / dtype(M * L)
    return out


def bwd(f, c, w=(0.0, 0.0), dz_ext=(None, None)):
    """From fwd's dict: (de [rows, L], g [rows, L]) for the loss sum_s c_s kl_s + w_s recon_s + <dz_ext_s, z_s>."""
    dtype, S, M, L, z = f["dtype"], f["S"], f["M"], f["L"], f["z"]
    c, w, dz_ext = (list(c) + [0.0])[:2], (list(w) + [0.0])[:2], (list(dz_ext) + [None])[:2]
    g = np.zeros_like(z)
    for s in range(S):
        zs, mu, var = z[s * M:(s + 1) * M], f["mu"][s], f["var"][s]
        gs = np.zeros_like(zs)
        if c[s] != 0:
            gs = gs + dtype(c[s]) / dtype(L) * (mu / dtype(M) + (dtype(1) - dtype(1) / var) * (zs - mu) / dtype(M - 1))
        if f["modes"][s] == 1:
            tt = f["t"]
            na, nt = _rownorm(zs), _rownorm(tt)
            nah, nth = np.maximum(na, dtype(COS_EPS)), np.maximum(nt, dtype(COS_EPS))
            tn = tt / nth
            dot = (zs * tn).sum(axis=1, keepdims=True)
            with np.errstate(divide="ignore", invalid="ignore"):
                unit = np.where(na > 0, zs / np.where(na > 0, na, dtype(1)), dtype(0))
            gs = gs - dtype(w[s]) / dtype(M) * (tn / nah - dot / (nah * nah) * unit)
        elif f["modes"][s] == 2:
            gs = gs + dtype(w[s]) * dtype(2) * (zs - f["t"]) / dtype(M * L)
        if dz_ext[s] is not None:
            gs = gs + np.asarray(dz_ext[s], dtype=dtype)
        g[s * M:(s + 1) * M] = gs
    if not f["normalize"]:
        return g, g
    n = f["norm"][:, None]
    big = n >= dtype(NORM_EPS)
    de = np.where(big, (g - z * (z * g).sum(axis=1, keepdims=True)) / np.where(big, n, dtype(1)), g / dtype(NORM_EPS))
    return de, g
