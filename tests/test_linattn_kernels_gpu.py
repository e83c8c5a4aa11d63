"""The thirteen kernel instantiations of csrc/linattn.hip on the MI355X against tests/_linattn_oracle.py: forward phases 0-3 and
backward phases 0-2 with fp32 and bf16 storage, and the fold.  The library is called directly (load_library()): qkv and dout are
views between NaN, every output and the workspace carry a sentinel behind them.

Bounds.  fp32 storage: kmax bit-equal; ksum, ctx, out <= 1e-5 rel-L2 and dq, dk, dv each <= 5e-5 against the float64 oracle (the
project's bounds, in both regimes: the fp32 emulation's peaked dk sits at 2.3e-6, so no other bound is needed for it).  bf16 storage, against
the round_bf16 model: kmax bit-equal, ksum <= 1e-5, ctx <= BOUND_CTX_BF16 = 4 x the fp32 emulation's 8.8e-6, and the stored bf16
tensors (out, dq, dk, dv, W_eff) bit for bit against bf16(model) with at most FLIP_CAP = 2 % of a tensor's elements differing
(the emulation: <= 0.46 %), the old 4e-3 against the unrounded oracle beside it (peaked dk: 4 x the rounding model's own
1.9e-5 relative to ||P|| ||dP - r||, see the oracle's header).  Where the figures come from:
tests/_linattn_oracle.py's header and tests/test_linattn_cpu.py::test_fp32_emulation_sets_the_bounds."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _linattn_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -776.0                        # never-written sentinel: finite and bf16-representable, so it compares bit for bit in both dtypes
PAD = 64                             # elements of NaN in front of and behind an input view (a multiple of 16 bytes in both dtypes)
BF, F32 = torch.bfloat16, torch.float32
STORAGE = ["fp32", "bf16"]
GRADS = ("dq", "dk", "dv")


def _lib():
    from src.ops.lib import load_library
    return load_library()


def _ptr(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _between_nan(t64, dtype):
    """(buffer, flat view): the values of t64 inside a NaN-filled buffer, PAD elements from either end."""
    buf = torch.full((t64.numel() + 2 * PAD,), float("nan"), dtype=dtype, device=DEV)
    view = buf[PAD:PAD + t64.numel()]
    view.copy_(t64.reshape(-1).to(dtype))
    assert view.data_ptr() % 16 == 0
    return buf, view


def _sentinel(numel, extra, dtype=F32):
    return torch.full((numel + extra,), SENT, dtype=dtype, device=DEV)


def _tail_intact(buf, numel):
    return bool((buf[numel:] == SENT).all()) and buf.numel() > numel


def _workspace(lib, case, how):
    """(buffer, pointer, bytes, floats that may be written) for a workspace given as `how`."""
    B, H, W, heads = case
    need = lib.mi_linattn_workspace(B, H * W, heads)
    buf = _sentinel(need // 4, 256)
    assert buf.data_ptr() % 16 == 0
    if how == "exact":
        return buf, _ptr(buf) if need else ctypes.c_void_p(0), need, need // 4
    if how == "null":
        return buf, ctypes.c_void_p(0), 0, 0
    if how == "small":
        return buf, _ptr(buf), need - 4, 0
    assert how == "misaligned"
    return buf, _ptr(buf, 4), need, 0


def _forward(lib, case, b16, qkv, ws="exact", entry="ws"):
    """One forward launch.  -> dict of kmax, ksum, ctx, out (device tensors) after the sentinel / NaN checks."""
    B, H, W, heads = case
    n, hid = H * W, heads * 32
    out = _sentinel(B * n * hid, n * hid, BF if b16 else F32)
    ctx = _sentinel(B * heads * 1024, heads * 1024)
    kstat = _sentinel(B * heads * 64, heads * 64)
    wbuf, wptr, wbytes, wlive = _workspace(lib, case, ws)
    if entry == "ws":
        rc = lib.mi_linattn_fwd_ws(B, n, heads, _ptr(qkv), _ptr(out), _ptr(ctx), _ptr(kstat), int(b16), wptr, wbytes, _stream())
    elif entry == "io":
        rc = lib.mi_linattn_fwd_io(B, n, heads, _ptr(qkv), _ptr(out), _ptr(ctx), _ptr(kstat), int(b16), _stream())
    else:
        assert entry == "plain" and not b16
        rc = lib.mi_linattn_fwd(B, n, heads, _ptr(qkv), _ptr(out), _ptr(ctx), _ptr(kstat), _stream())
    assert rc == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    assert _tail_intact(out, B * n * hid) and _tail_intact(ctx, B * heads * 1024) and _tail_intact(kstat, B * heads * 64)
    assert _tail_intact(wbuf, wlive), "workspace written past its size (or written at all in a fallback)"
    r = dict(out=out[:B * n * hid].view(B, n, heads, 32), ctx=ctx[:B * heads * 1024].view(B, heads, 32, 32),
             kstat=kstat[:B * heads * 64].view(B, heads, 32, 2))
    for k, t in r.items():
        assert bool(torch.isfinite(t.float()).all()), f"non-finite {k}"
    r["kmax"], r["ksum"] = r["kstat"][..., 0], r["kstat"][..., 1]
    return r


def _backward(lib, case, b16, qkv, dout, ctx, kstat, ws="exact", entry="ws"):
    """One backward launch on the given ctx [B][heads][32][32] / kstat [B][heads][32][2] (fp32, device).  -> dq, dk, dv."""
    B, H, W, heads = case
    n, ldq = H * W, 3 * heads * 32
    ctx, kstat = ctx.contiguous(), kstat.contiguous()
    dqkv = _sentinel(B * n * ldq, n * ldq, BF if b16 else F32)
    wbuf, wptr, wbytes, wlive = _workspace(lib, case, ws)
    if entry == "ws":
        rc = lib.mi_linattn_bwd_ws(B, n, heads, _ptr(qkv), _ptr(ctx), _ptr(kstat), _ptr(dout), _ptr(dqkv), int(b16), wptr, wbytes, _stream())
    elif entry == "io":
        rc = lib.mi_linattn_bwd_io(B, n, heads, _ptr(qkv), _ptr(ctx), _ptr(kstat), _ptr(dout), _ptr(dqkv), int(b16), _stream())
    else:
        assert entry == "plain" and not b16
        rc = lib.mi_linattn_bwd(B, n, heads, _ptr(qkv), _ptr(ctx), _ptr(kstat), _ptr(dout), _ptr(dqkv), _stream())
    assert rc == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    assert _tail_intact(dqkv, B * n * ldq) and _tail_intact(wbuf, wlive)
    g = dqkv[:B * n * ldq].view(B, n, 3, heads, 32)
    assert bool(torch.isfinite(g.float()).all()), "non-finite dqkv"
    return dict(dq=g[:, :, 0], dk=g[:, :, 1], dv=g[:, :, 2])


def _check_forward(r, R, b16, regime, tag):
    M, Pl = R["model"], R["plain"]
    assert torch.equal(r["kmax"].cpu(), M["kmax"].float()), f"{tag}: kmax is not the maximum"
    e = dict(ksum=O.rel(r["ksum"], M["ksum"]), ctx=O.rel(r["ctx"], M["ctx"]))
    if not b16:
        e["out"] = O.rel(r["out"], M["out"])
        print(f"{tag}: " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))
        assert e["ksum"] <= 1e-5 and e["ctx"] <= 1e-5 and e["out"] <= 1e-5, (tag, e)
        return
    e["out flips"] = O.flips(r["out"], M["out"])
    e["out loose"] = O.rel(r["out"], Pl["out"])
    e["ctx loose"] = O.rel(r["ctx"], Pl["ctx"])
    print(f"{tag}: " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))
    assert r["out"].dtype == BF
    assert e["ksum"] <= 1e-5 and e["ctx"] <= O.BOUND_CTX_BF16 and e["ctx loose"] <= 2.5e-3, (tag, e)
    assert e["out flips"] <= O.FLIP_CAP and e["out loose"] <= 4e-3, (tag, e)


def _check_backward(g, M, Pl, b16, regime, tag):
    """g against M (the model evaluated on the ctx / kstat the launch was given) and, bf16 storage, loosely against the plain oracle."""
    e = {k: O.rel(g[k], M[k]) for k in GRADS}
    e["dk scaled"] = O.dk_scaled(g["dk"], M)
    if not b16:
        print(f"{tag}: " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))
        assert e["dq"] <= 5e-5 and e["dk"] <= 5e-5 and e["dv"] <= 5e-5, (tag, e)
        return
    for k in GRADS:
        assert g[k].dtype == BF
        e[k + " flips"] = O.flips(g[k], M[k])
        e[k + " loose"] = O.dk_scaled(g[k], Pl) if (k == "dk" and regime == "peaked") else O.rel(g[k], Pl[k])
    print(f"{tag}: " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))
    for k in GRADS:
        loose = O.BOUND_DK_PEAKED_BF16 if (k == "dk" and regime == "peaked") else 4e-3
        assert e[k + " flips"] <= O.FLIP_CAP and e[k + " loose"] <= loose, (tag, k, e)


def _model_backward(R, ctx, kstat, b16):
    """The backward model on the ctx / kstat a launch was given (fp32 device tensors)."""
    return O.backward(R["qkv"], R["dout"], ctx.cpu(), kstat[..., 0].cpu(), kstat[..., 1].cpu(), round_bf16=b16)


def _same(a, b, keys):
    return all(torch.equal(a[k], b[k]) for k in keys)


def test_case_list_is_the_oracles():
    """The slices every case takes, from the library: mi_linattn_workspace == B * heads * S * 1088 * 4 (0 for S = 1)."""
    lib = _lib()
    assert len(O.CASES) == len(O.EXPECTED_S) >= 10
    for (B, H, W, heads), S in zip(O.CASES, O.EXPECTED_S):
        assert lib.mi_linattn_workspace(B, H * W, heads) == (B * heads * S * 1088 * 4 if S > 1 else 0), (B, H, W, heads)


@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("regime", O.REGIMES)
@pytest.mark.parametrize("case", O.CASES, ids=lambda c: "x".join(map(str, c)))
def test_linattn_case(case, regime, storage):
    """Forward and backward of one case: against the oracle, run twice, sliced against unsliced, the backward on the kernel's own and
    on the oracle's ctx / kstat."""
    lib = _lib()
    b16 = storage == "bf16"
    B, H, W, heads = case
    S = O.EXPECTED_S[O.CASES.index(case)]
    assert lib.mi_linattn_workspace(B, H * W, heads) == (B * heads * S * 1088 * 4 if S > 1 else 0)
    R = O.reference(case, regime, b16)
    M = R["model"]
    dt = BF if b16 else F32
    qbuf, qkv = _between_nan(R["qkv"], dt)
    dbuf, dout = _between_nan(R["dout"], dt)
    tag = f"{case} {regime} {storage} S={S}"

    f = _forward(lib, case, b16, qkv)
    _check_forward(f, R, b16, regime, tag + " fwd")
    f2 = _forward(lib, case, b16, qkv)
    assert _same(f, f2, ("out", "ctx", "kstat")), "forward not reproducible"

    # backward on the kernel's own forward results ...
    g = _backward(lib, case, b16, qkv, dout, f["ctx"], f["kstat"])
    _check_backward(g, _model_backward(R, f["ctx"], f["kstat"], b16), R["plain"], b16, regime, tag + " bwd(own)")
    g2 = _backward(lib, case, b16, qkv, dout, f["ctx"], f["kstat"])
    assert _same(g, g2, GRADS), "backward not reproducible"
    # ... and on the oracle's (fp32 casts)
    octx = M["ctx"].float().to(DEV)
    okst = torch.stack([M["kmax"], M["ksum"]], -1).float().to(DEV)
    go = _backward(lib, case, b16, qkv, dout, octx, okst)
    _check_backward(go, _model_backward(R, octx, okst, b16), R["plain"], b16, regime, tag + " bwd(oracle)")

    if S > 1:                                             # the same calls without a workspace: one workgroup per (batch, head)
        u = _forward(lib, case, b16, qkv, ws="null")
        assert torch.equal(u["kmax"], f["kmax"])
        _check_forward(u, R, b16, regime, tag + " fwd(unsliced)")
        gu = _backward(lib, case, b16, qkv, dout, f["ctx"], f["kstat"], ws="null")
        _check_backward(gu, _model_backward(R, f["ctx"], f["kstat"], b16), R["plain"], b16, regime, tag + " bwd(unsliced)")
    assert bool(torch.isnan(qbuf[:PAD]).all()) and bool(torch.isnan(qbuf[-PAD:]).all()) and bool(torch.isnan(dbuf[:PAD]).all())


# mi_linattn_fwd / mi_linattn_bwd ("plain") are the fp32-storage entry points
@pytest.mark.parametrize("how,storage", [(h, s) for h in ("null", "small", "misaligned", "io", "plain") for s in STORAGE if (h, s) != ("plain", "bf16")])
def test_linattn_workspace_fallbacks(how, storage):
    """(2, 24, 24, 4) wants four slices; without a usable workspace -- null, 4 bytes short, 4 bytes off alignment, or through the entry
    points that take none -- it runs one workgroup per (batch, head), to the same bounds, and leaves the buffer it was offered alone.
    The backward also runs in fallback on the ctx / kstat of the sliced forward."""
    lib = _lib()
    b16 = storage == "bf16"
    case, regime = (2, 24, 24, 4), "normal"
    assert lib.mi_linattn_workspace(2, 576, 4) == 2 * 4 * 4 * 1088 * 4
    R = O.reference(case, regime, b16)
    dt = BF if b16 else F32
    _, qkv = _between_nan(R["qkv"], dt)
    _, dout = _between_nan(R["dout"], dt)
    ws, entry = (how, "ws") if how in ("null", "small", "misaligned") else ("null", how)
    tag = f"{case} {storage} fallback {how}"
    sliced = _forward(lib, case, b16, qkv)
    f = _forward(lib, case, b16, qkv, ws=ws, entry=entry)
    assert torch.equal(f["kmax"], sliced["kmax"])
    _check_forward(f, R, b16, regime, tag + " fwd")
    for name, src in (("own", f), ("sliced", sliced)):
        g = _backward(lib, case, b16, qkv, dout, src["ctx"], src["kstat"], ws=ws, entry=entry)
        _check_backward(g, _model_backward(R, src["ctx"], src["kstat"], b16), R["plain"], b16, regime, f"{tag} bwd({name})")
    # every fallback is the same launch: bit-equal to the null-workspace run
    u = _forward(lib, case, b16, qkv, ws="null")
    assert _same(f, u, ("out", "ctx", "kstat"))


@pytest.mark.parametrize("regime", O.REGIMES)
@pytest.mark.parametrize("case", O.FOLD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_linattn_fold(case, regime):
    """mi_linattn_fold_fwd called directly: W_eff decoded from its fragment order, bit for bit against the fold model."""
    lib = _lib()
    B, H, W, heads, C = case
    n, hid = H * W, heads * 32
    R = O.fold_reference(case, regime)
    qbuf, qkv = _between_nan(R["qkv"], BF)
    wbuf, wout = _between_nan(R["wout"], BF)
    weff = _sentinel(B * C * hid, C * hid, BF)
    assert weff.data_ptr() % 16 == 0 and wout.data_ptr() % 16 == 0
    runs = []
    for _ in range(2):
        weff[:B * C * hid].fill_(float("nan"))
        rc = lib.mi_linattn_fold_fwd(B, n, heads, _ptr(qkv), _ptr(wout), C, _ptr(weff), _stream())
        assert rc == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        assert _tail_intact(weff, B * C * hid)
        runs.append(weff[:B * C * hid].clone())
    assert torch.equal(runs[0], runs[1]) and bool(torch.isfinite(runs[0].float()).all())
    got = O.weff_decode(runs[0].cpu(), B, C, hid)
    e = dict(flips=O.flips(got, R["model"]), loose=O.rel(got, R["plain"]), model=O.rel(got, R["model"]))
    print(f"{case} {regime} fold: " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))
    assert e["flips"] <= O.FLIP_CAP and e["loose"] <= 4e-3, e
    assert bool(torch.isnan(qbuf[:PAD]).all()) and bool(torch.isnan(wbuf[-PAD:]).all())
