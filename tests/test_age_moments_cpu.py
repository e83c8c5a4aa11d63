"""tests/_age_oracle.py against torch's float64 autograd on F.normalize, mean / var, F.cosine_similarity and F.mse_loss, to 1e-12
relative: the oracle's forward and ANALYTIC backward are what the installed torch computes, eps semantics included."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _age_oracle as O  # noqa: E402


def _torch_run(e, S, normalize, modes, t, c, w, dz_ext):
    e = torch.from_numpy(e).requires_grad_(True)
    z = F.normalize(e) if normalize else e
    M = e.shape[0] // S
    total, res = 0.0, {"kl": [], "recon": [], "mean_mu": [], "mean_var": []}
    tt = None if t is None else torch.from_numpy(t)
    for s in range(S):
        zs = z[s * M:(s + 1) * M]
        mu, var = zs.mean(dim=0), zs.var(dim=0)
        kl = (mu ** 2 + var - torch.log(var)).mean() / 2
        recon = torch.zeros((), dtype=torch.float64)
        if modes[s] == 1:
            recon = 1 - F.cosine_similarity(zs, tt).mean()
        elif modes[s] == 2:
            recon = F.mse_loss(zs, tt)
        total = total + c[s] * kl + w[s] * recon
        if dz_ext[s] is not None:
            total = total + (zs * torch.from_numpy(dz_ext[s])).sum()
        for k, v in (("kl", kl), ("recon", recon), ("mean_mu", mu.mean()), ("mean_var", var.mean())):
            res[k].append(float(v.detach()))
    total.backward()
    res["z"], res["de"] = z.detach().numpy(), e.grad.numpy()
    return res


def _rel(a, b):
    """Largest error relative to the largest reference value, row by row for a matrix (a zero row's gradient is 1e12 times the others')."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.ndim == 2:
        return max(_rel(x, y) for x, y in zip(a, b))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


CASES = [
    # S, M, L, normalize, modes, c, w, with dz_ext, zero row
    (1, 5, 6, True, (0, 0), (1.0,), (0.0,), False, False),
    (1, 5, 6, True, (2, 0), (1.0,), (1000.0,), False, False),
    (1, 7, 10, True, (1, 0), (1.0,), (3.0,), True, False),
    (2, 5, 6, True, (0, 1), (1.0, -1.0), (0.0, 1000.0), True, False),
    (2, 5, 6, True, (0, 0), (1.0, -1.0), (0.0, 0.0), True, False),
    (2, 4, 10, True, (2, 0), (1.0, 0.0), (2.5, 0.0), False, False),
    (2, 5, 6, False, (0, 1), (1.0, -1.0), (0.0, 7.0), True, False),
    (1, 5, 6, False, (2, 0), (1.0,), (1.5,), False, False),
    (2, 6, 5, True, (0, 1), (1.0, -1.0), (0.0, 2.0), True, True),
    (1, 6, 5, True, (2, 0), (1.0,), (2.0,), False, True),
    (2, 6, 5, False, (1, 1), (0.5, -1.0), (3.0, 2.0), False, True),
]


@pytest.mark.parametrize("S,M,L,normalize,modes,c,w,ext,zero", CASES)
def test_oracle_matches_torch_autograd(S, M, L, normalize, modes, c, w, ext, zero):
    r = np.random.RandomState(1000 * S + 10 * M + L)
    e = r.randn(S * M, L) * 3
    if zero:
        e[S * M - 2] = 0.0                                     # an exactly-zero row (in the segment the cosine term reads, when there is one)
    t = r.randn(M, L)
    t = t / np.sqrt((t * t).sum(axis=1, keepdims=True))
    dz = [r.randn(M, L) * 0.01 if (ext and s == 0) else None for s in range(2)]
    c2, w2 = (list(c) + [0.0])[:2], (list(w) + [0.0])[:2]
    ref = _torch_run(e, S, normalize, modes, t, c2, w2, dz)
    f = O.fwd(e, S, normalize, modes, t)
    de, _ = O.bwd(f, c2, w2, dz)
    assert (f["var"] > 1e-3).all()
    for k in ("kl", "recon", "mean_mu", "mean_var"):
        for s in range(S):
            assert abs(f[k][s] - ref[k][s]) <= 1e-12 * max(abs(ref[k][s]), 1.0), (k, s, f[k][s], ref[k][s])
    assert _rel(f["z"], ref["z"]) <= 1e-12
    assert np.isfinite(de).all()
    assert _rel(de, ref["de"]) <= 1e-12, _rel(de, ref["de"])
    if zero and normalize:
        row = S * M - 2
        assert (f["z"][row] == 0).all() and np.abs(de[row]).max() > 1e6          # g / 1e-12


def test_float32_twin_stays_float32_and_close():
    r = np.random.RandomState(3)
    e = (r.randn(10, 6) * 3).astype(np.float32)
    t = r.randn(5, 6).astype(np.float32)
    f32 = O.fwd(e, 2, True, (0, 1), t, dtype=np.float32)
    f64 = O.fwd(e, 2, True, (0, 1), t)
    d32, _ = O.bwd(f32, (1.0, -1.0), (0.0, 10.0))
    d64, _ = O.bwd(f64, (1.0, -1.0), (0.0, 10.0))
    assert all(f32[k].dtype == np.float32 for k in ("z", "norm", "mu", "var", "kl", "recon")) and d32.dtype == np.float32
    assert 0 < _rel(d32, d64) < 1e-4 and _rel(f32["kl"], f64["kl"]) < 1e-5
