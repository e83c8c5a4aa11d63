"""csrc/norm_act.hip on the MI355X against tests/_norm_oracle.py, through the C ABI (load_library()): every GroupNorm + Mish instantiation
the product library can reach, the statistics-only and sum-fed entry points, and the channel LayerNorm.  Inputs are views between NaN
with NaN in their pitch padding; every output has a sentinel behind it and in its padding; every launch runs twice.

Bounds.  Against the float64 oracle on the stored values (the project's bounds): y <= 1e-5, dx / dgamma / dbeta / dtemb / dg / db <= 5e-5
rel-L2, statistics and coefficients <= 2e-6 of the largest.  dbias, a cancelled sum: per channel relative to sum |dx|,
4 x EMU_DBIAS_F32 = 1.2e-6 (fp32 x) and 4 x EMU_DBIAS_BF16 = 3.2e-5 (bf16 x); dgamma / dbeta with bf16 x: 4 x EMU_DPARAM_BF16 = 2.6e-5
(the float32 emulation's figures, asserted by tests/test_norm_cpu.py::test_emulation_sets_the_bounds; the factor 4 covers the order
of the reductions).  Stored bf16 tensors (y, the dual copy, dx): bit for bit against bf16(rounding model) -- at most FLIP_CAP = 0.5 %
of a tensor's elements may differ, and each of those by one bf16 ulp (or, where the element's terms cancel, by ALLOW = 2^-19 of their
magnitude: the oracle's flips()) -- with the old 6e-3 (y) / 8e-3 (dx) against the unrounded oracle beside it.

Measured on the MI355X: y <= 2.1e-6 (x near 100: 2.6e-5 under a bound of 2.9e-4), gradients <= 6.7e-7 -- except an fp32 dx formed from
bf16(dz) (io 1, 5 on the packed-cache paths), 1e-6 ... 4.0e-5 under the same 5e-5: a few dz in ten thousand land one bf16 ulp off the
model's, and each is 2^-8 of its element -- statistics <= 1.5e-7, dbias <= 7.1e-7 (fp32 x) / 6.1e-7 (bf16 x), flips <= 0.043 %,
excess <= 3.0e-7 = 0.16 ALLOW.

What the product library cannot reach: MI_GN_VEC8, MI_GN_FULL and MI_GN_WIDE16 are compile-time constants there (mi_knob reads the
environment only in -DMI_EXPERIMENT builds), so <8,4,IO> / <8,8,IO>, the guarded form at HW == 8 PP and the uncached form at the wide
shapes have no test here; a child process with those variables set would run the same kernels as its parent."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _norm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -776.0                        # never-written sentinel: finite and bf16-representable
PAD = 64                             # elements of NaN in front of and behind an input (a multiple of 16 bytes in both dtypes)
BF, F32 = torch.bfloat16, torch.float32
EPS = O.GN_EPS
PITCH = dict(x=8, y=16, r=24, do=32, dx=40, t=48, y16=56)       # added to C: all different, all multiples of 8
NULL = ctypes.c_void_p(0)


def _lib():
    from src.ops.lib import load_library
    return load_library()


def _desc(case, ldx, ldy=0, ldr=0):
    from src.ops.lib import MiGnDesc
    N, HW, C, G = case
    return ctypes.byref(MiGnDesc(N=N, HW=HW, C=C, G=G, eps=EPS, ldx=ldx, ldy=ldy, ldr=ldr))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class In:
    """Rows of t64 [R][C] at pitch ld inside a NaN-filled buffer: NaN in front, behind and in the padding of every row."""

    def __init__(self, t64, ld=None, dtype=F32):
        t64 = t64.reshape(-1, t64.shape[-1])
        R, C = t64.shape
        self.ld = ld or C
        self.buf = torch.full((2 * PAD + R * self.ld,), float("nan"), dtype=dtype, device=DEV)
        self.rows = self.buf[PAD:PAD + R * self.ld].view(R, self.ld)
        self.rows[:, :C].copy_(t64.to(dtype))
        assert self.rows.data_ptr() % 16 == 0
        self.ptr = ctypes.c_void_p(self.rows.data_ptr())


class Out:
    """R rows of C elements at pitch ld, `off` elements into a sentinel-filled buffer with a sentinel tail."""

    def __init__(self, R, C, ld=None, dtype=F32, off=0, init=None):
        self.R, self.C, self.ld, self.off = R, C, ld or C, off
        self.buf = torch.full((off + R * self.ld + 256,), SENT, dtype=dtype, device=DEV)
        self.rows = self.buf[off:off + R * self.ld].view(R, self.ld)
        if init is not None:
            self.rows[:, :C].copy_(init.reshape(R, C).to(dtype))
        self.ptr = ctypes.c_void_p(self.rows.data_ptr())

    def get(self):
        """The written part, after checking that nothing else was."""
        assert bool((self.buf[:self.off] == SENT).all()) and bool((self.buf[self.off + self.R * self.ld:] == SENT).all()), "written outside"
        assert bool((self.rows[:, self.C:] == SENT).all()), "pitch padding written"
        return self.rows[:, :self.C].clone()

    def untouched(self):
        return bool((self.buf == SENT).all())


def _finite(*ts):
    return all(bool(torch.isfinite(t.float()).all()) for t in ts if t is not None)


def _ld(C, key, pitched):
    return C + PITCH[key] if pitched else C


# ---------------------------------------------------------------------------------------------------- GroupNorm launches
def gn_forward(lib, case, inp, io=None, pitched=True, temb=True, res=True, dual=False, n0=None):
    """One forward launch (n0: the N = 1 launch of sample n0 on the same buffers' values).  io None: mi_gn_mish_fwd."""
    N, HW, C, G = case
    x16, y16 = bool(io and io & 1), bool(io and io & 2)
    sl = slice(None) if n0 is None else slice(n0, n0 + 1)
    Nl = N if n0 is None else 1
    x = In(inp["x"][sl], _ld(C, "x", pitched), BF if x16 else F32)
    ga, be = In(inp["gamma"][None]), In(inp["beta"][None])
    tb = In(inp["temb"][sl], _ld(C, "t", pitched)) if temb else None
    rs = In(inp["res"][sl], _ld(C, "r", pitched)) if res else None
    y = Out(Nl * HW, C, _ld(C, "y", pitched), BF if y16 else F32)
    yc = Out(Nl * HW, C, _ld(C, "y16", pitched), BF) if dual else None
    st = Out(Nl * G, 2)
    d = _desc((Nl, HW, C, G), x.ld, y.ld, rs.ld if rs else 0)
    a = (d, x.ptr, ga.ptr, be.ptr, tb.ptr if tb else NULL, tb.ld if tb else 0, rs.ptr if rs else NULL, y.ptr)
    if dual:
        rc = lib.mi_gn_mish_fwd_dual(*a, yc.ptr, yc.ld, st.ptr, io, _stream())
    elif io is None:
        rc = lib.mi_gn_mish_fwd(*a, st.ptr, _stream())
    else:
        rc = lib.mi_gn_mish_fwd_io(*a, st.ptr, io, _stream())
    assert rc == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    r = dict(y=y.get().view(Nl, HW, C), stats=st.get().view(Nl, G, 2), y16=yc.get().view(Nl, HW, C) if dual else None)
    assert _finite(r["y"], r["stats"], r["y16"]), "non-finite output"
    assert bool(torch.isnan(x.buf[:PAD]).all()) and bool(torch.isnan(x.buf[-PAD:]).all())
    return r


def gn_backward(lib, case, inp, stats32, io=None, pitched=True, sums=True, init=None, variant="", n0=None):
    """One backward launch on the statistics it is given ((mean, rstd) float32 [N][G]).  sums: with dgamma, dbeta, dtemb, dbias."""
    N, HW, C, G = case
    x16, dx16, do16 = bool(io and io & 1), bool(io and io & 2), bool(io and io & 4)
    sl = slice(None) if n0 is None else slice(n0, n0 + 1)
    Nl = N if n0 is None else 1
    x = In(inp["x"][sl], _ld(C, "x", pitched), BF if x16 else F32)
    lddo = C + 36 if variant == "lddo4" else _ld(C, "do", pitched)
    do = In(inp["dout"][sl], lddo, BF if do16 else F32)
    ga, be = In(inp["gamma"][None]), In(inp["beta"][None])
    st = In(torch.stack([stats32[0][sl], stats32[1][sl]], -1).reshape(Nl * G, 2).double())
    off = 4 if variant == "dx8" else 0
    assert not off or dx16
    dx = Out(Nl * HW, C, _ld(C, "dx", pitched), BF if dx16 else F32, off=off)
    assert dx.rows.data_ptr() % 16 == 2 * off
    z = torch.zeros(C, dtype=torch.float64)
    dga, dbe, dbi = (Out(1, C, init=(init[k] if init else z)) for k in ("dgamma", "dbeta", "dbias"))
    dtb = Out(Nl, C, _ld(C, "t", pitched))
    a = (_desc((Nl, HW, C, G), x.ld), x.ptr, st.ptr, ga.ptr, be.ptr, do.ptr, do.ld, dx.ptr, dx.ld,
         dga.ptr if sums else NULL, dbe.ptr if sums else NULL, dtb.ptr if sums else NULL, dtb.ld, dbi.ptr if sums else NULL)
    rc = lib.mi_gn_mish_bwd(*a, _stream()) if io is None else lib.mi_gn_mish_bwd_io(*a, io, _stream())
    assert rc == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    r = dict(dx=dx.get().view(Nl, HW, C))
    if sums:
        r.update(dgamma=dga.get().view(C), dbeta=dbe.get().view(C), dbias=dbi.get().view(C), dtemb=dtb.get())
    else:
        assert dga.untouched() or init is not None
        assert dtb.untouched()
    assert _finite(*r.values()), "non-finite output"
    assert bool(torch.isnan(do.buf[:PAD]).all()) and bool(torch.isnan(do.buf[-PAD:]).all())
    return r


def _stats32(inp, G):
    m, r = O.gn_stats_ref(inp["x"], G, EPS)
    return m.float(), r.float()


def _init(C):
    k = torch.arange(C, dtype=torch.float64)
    return dict(dgamma=0.5 - (k % 3) * 0.25, dbeta=(k % 5) * 0.125 - 0.25, dbias=0.75 - (k % 2) * 1.5)


def _check_stats(got, inp, G, tag):
    m, r = O.gn_stats_ref(inp["x"], G, EPS)
    e = (O.rel_max(got[..., 0], m), O.rel_max(got[..., 1], r))
    print(f"{tag}: mean {e[0]:.3g} rstd {e[1]:.3g}")
    assert max(e) <= 2e-6, (tag, e)


def _check_stored(got, model, scale, alts, loose_ref, loose, tag):
    """A stored bf16 tensor to the bf16 rule, the old loose bound beside it."""
    assert got.dtype == BF
    share, excess = O.flips(got, model, scale, alts)
    lo = O.rel(got, loose_ref)
    print(f"{tag}: flips {share:.3g} excess {excess:.3g} loose {lo:.3g}")
    assert share <= O.FLIP_CAP and excess <= O.ALLOW and lo <= loose, (tag, share, excess, lo)


def _check_grads(r, ref, init, x_bf16, tag, with_dx=True):
    """fp32 results of a backward launch against ref = gn_mish_grads_ref(...) on the statistics the launch was given."""
    i = init or dict(dgamma=0.0, dbeta=0.0, dbias=0.0)
    e = dict(dgamma=O.rel(r["dgamma"].double().cpu() - i["dgamma"], ref["dgamma"]), dbeta=O.rel(r["dbeta"].double().cpu() - i["dbeta"], ref["dbeta"]),
             dtemb=O.rel(r["dtemb"], ref["dtemb"]), dbias=O.dbias_err(r["dbias"].double().cpu() - i["dbias"], ref["dbias"], ref["dx"]))
    if with_dx:
        e["dx"] = O.rel(r["dx"], ref["dx"])
    print(f"{tag}: " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))
    bp = 4 * O.EMU_DPARAM_BF16 if x_bf16 else 5e-5
    assert e["dgamma"] <= bp and e["dbeta"] <= bp and e["dtemb"] <= 5e-5 and e.get("dx", 0.0) <= 5e-5, (tag, e)
    assert e["dbias"] <= 4 * (O.EMU_DBIAS_BF16 if x_bf16 else O.EMU_DBIAS_F32), (tag, e)


# ---------------------------------------------------------------------------------------------------- GroupNorm, fp32 storage
@pytest.mark.parametrize("case", [c for c, _ in O.GN_F32_CASES], ids=lambda c: "x".join(map(str, c)))
def test_gn_fp32(case):
    """mi_gn_mish_fwd / mi_gn_mish_bwd: with and without temb / residual / the summed gradients, twice, and (N % 8 == 0) sample by sample."""
    lib = _lib()
    N, HW, C, G = case
    pitched = case in O.GN_F32_PITCHED
    inp = O.gn_inputs(case)
    st = _stats32(inp, G)
    init = _init(C)
    ref = O.gn_mish_grads_ref(inp["x"], inp["gamma"], inp["beta"], G, EPS, inp["dout"], stats=st)
    for full in (True, False):
        tag = f"{case} fp32 {'temb+res' if full else 'plain'}"
        f = gn_forward(lib, case, inp, pitched=pitched, temb=full, res=full)
        f2 = gn_forward(lib, case, inp, pitched=pitched, temb=full, res=full)
        assert torch.equal(f["y"], f2["y"]) and torch.equal(f["stats"], f2["stats"]), "forward not reproducible"
        yr = O.gn_mish_ref(inp["x"], inp["gamma"], inp["beta"], G, EPS, inp["temb"] if full else None, inp["res"] if full else None)[0]
        e = O.rel(f["y"], yr)
        print(f"{tag}: y {e:.3g}")
        assert e <= 1e-5, (tag, e)
        _check_stats(f["stats"], inp, G, tag)
        b = gn_backward(lib, case, inp, st, pitched=pitched, sums=full, init=init)
        b2 = gn_backward(lib, case, inp, st, pitched=pitched, sums=full, init=init)
        assert torch.equal(b["dx"], b2["dx"]) and (not full or torch.equal(b["dtemb"], b2["dtemb"])), "backward not reproducible"
        if full:
            _check_grads(b, ref, init, False, tag)
        else:
            e = O.rel(b["dx"], ref["dx"])
            assert e <= 5e-5, (tag, e)
        if N % 8 == 0 and full:                      # the XCD remap: sample n of the batch is the N = 1 launch of sample n, bit for bit
            for n in range(N):
                f1 = gn_forward(lib, case, inp, pitched=pitched, n0=n)
                b1 = gn_backward(lib, case, inp, st, pitched=pitched, n0=n)
                assert torch.equal(f1["y"][0], f["y"][n]) and torch.equal(f1["stats"][0], f["stats"][n]), (tag, n)
                assert torch.equal(b1["dx"][0], b["dx"][n]) and torch.equal(b1["dtemb"][0], b["dtemb"][n]), (tag, n)


@pytest.mark.parametrize("edge", O.EDGES)
@pytest.mark.parametrize("case", O.GN_F32_EDGE_SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_gn_fp32_edges(case, edge):
    """A constant slice (rstd = 1 / sqrt(eps), y = mish(beta)), x = 100 + 0.1 randn, and z beyond Mish's threshold on alternating channels.
    mean100: the float32 mean of values near 100 is off by a few 2^-24 x 100 whatever the order of the sum (64 terms per thread, then a
    tree: about 2 x 2^-24 relative by a random-walk estimate), and xhat = (x - mean) rstd carries that times rstd = 10: the forward bound
    there is 1e-5 + the oracle's own change of y under a mean 8 x 2^-24 x |mean| off.  The backward is given its statistics and needs none."""
    lib = _lib()
    N, HW, C, G = case
    inp = O.gn_inputs(case, edge=edge)
    st = _stats32(inp, G)
    tag = f"{case} {edge}"
    f = gn_forward(lib, case, inp)
    yr, mean, rstd = O.gn_mish_ref(inp["x"], inp["gamma"], inp["beta"], G, EPS, inp["temb"], inp["res"])
    bound = 1e-5
    if edge == "mean100":
        off = O.gn_mish_ref(inp["x"], inp["gamma"], inp["beta"], G, EPS, inp["temb"], inp["res"], stats=(mean * (1 + 8 * 2.0 ** -24), rstd))[0]
        bound += O.rel(off, yr)
    e = O.rel(f["y"], yr)
    print(f"{tag}: y {e:.3g} (bound {bound:.3g})")
    assert e <= bound, (tag, e, bound)
    _check_stats(f["stats"], inp, G, tag)
    if edge == "constant_slice":
        cg = C // G
        assert abs(float(f["stats"][N - 1, G - 1, 1]) * math.sqrt(EPS) - 1) <= 2e-6 and float(f["stats"][N - 1, G - 1, 0]) == 0.75
        want = O.mish(inp["beta"][C - cg:])[None] + inp["temb"][N - 1, C - cg:][None] + inp["res"][N - 1, :, C - cg:]
        assert O.rel(f["y"][N - 1, :, C - cg:], want) <= 1e-5
    if edge.startswith("threshold"):
        for par in (0, 1):
            assert O.rel(f["y"][..., par::2], yr[..., par::2]) <= 1e-5, (tag, par)
    ref = O.gn_mish_grads_ref(inp["x"], inp["gamma"], inp["beta"], G, EPS, inp["dout"], stats=st)
    b = gn_backward(lib, case, inp, st, init=_init(C))
    _check_grads(b, ref, _init(C), False, tag)
    if edge.startswith("threshold"):
        for par in (0, 1):
            assert O.rel(b["dx"][..., par::2], ref["dx"][..., par::2]) <= 5e-5, (tag, par)


@pytest.mark.parametrize("io", [2, 4, 6])
@pytest.mark.parametrize("case", O.GN_F32_IO_BWD, ids=lambda c: "x".join(map(str, c)))
def test_gn_bwd_io_fp32_x(case, io):
    """mi_gn_mish_bwd_io with fp32 x: bf16 dx (io 2, 6) and bf16 dout (io 4, 6) on the fp32-x instantiations."""
    lib = _lib()
    N, HW, C, G = case
    inp = O.gn_inputs(case, bf16_dout=bool(io & 4))
    st = _stats32(inp, G)
    ref = O.gn_mish_grads_ref(inp["x"], inp["gamma"], inp["beta"], G, EPS, inp["dout"], stats=st)
    tag = f"{case} io {io}"
    b = gn_backward(lib, case, inp, st, io=io, init=_init(C))
    b2 = gn_backward(lib, case, inp, st, io=io, init=_init(C))
    assert torch.equal(b["dx"], b2["dx"]) and torch.equal(b["dtemb"], b2["dtemb"])
    _check_grads(b, ref, _init(C), False, tag, with_dx=not io & 2)
    if io & 2:
        _check_stored(b["dx"], ref["dx"], ref["scale"], (), ref["dx"], 8e-3, tag + " dx")


# ---------------------------------------------------------------------------------------------------- GroupNorm, bf16 storage
def _bf16_id(p):
    return "x".join(map(str, p[0])) + ("-" + p[1] if p[1] else "")


@pytest.mark.parametrize("params", ["std", "wide"])
@pytest.mark.parametrize("entry", O.GN_BF16_CASES, ids=_bf16_id)
def test_gn_bf16(entry, params):
    """mi_gn_mish_fwd_io (io 1, 2, 3), mi_gn_mish_fwd_dual and mi_gn_mish_bwd_io (io 1, 3, 5, 7) with three distinct pitches.
    wide: gamma = 4 randn + 1, beta = 10 randn (z on both sides of Mish's threshold inside one packed pair)."""
    lib = _lib()
    case, variant, want = entry
    N, HW, C, G = case
    wide = params == "wide"
    inp = O.gn_inputs(case, bf16_x=True, wide_params=wide)
    inp16 = O.gn_inputs(case, bf16_x=True, bf16_dout=True, wide_params=wide)
    st = _stats32(inp, G)
    init = _init(C)
    lds = [C + PITCH["x"], C + 36 if variant == "lddo4" else C + PITCH["do"], C + PITCH["dx"]]
    rounds = want[1] > 4
    refs = {b16: O.gn_mish_grads_ref(s_["x"], s_["gamma"], s_["beta"], G, EPS, s_["dout"], stats=st, round_dz=rounds) for b16, s_ in ((False, inp), (True, inp16))}
    for io in ((3, 7) if variant == "dx8" else O.BWD_IO16):
        plan = O.launch_plan(N, HW, C, G, io=io, pitches=lds, alignments=[0, 0, 8 if variant == "dx8" else 0, 0, 0])
        assert (plan["kernel"][0], plan["kernel"][1], plan["kernel"][3]) == want and plan["rounds_dz"] == rounds
        src = inp16 if io & 4 else inp
        ref = refs[bool(io & 4)]
        tag = f"{case} {variant} {params} bwd io {io} <{plan['kernel'][0]},{plan['kernel'][1]}{',FULL' if plan['kernel'][3] else ''}>"
        b = gn_backward(lib, case, src, st, io=io, init=init, variant=variant)
        b2 = gn_backward(lib, case, src, st, io=io, init=init, variant=variant)
        assert torch.equal(b["dx"], b2["dx"]) and torch.equal(b["dtemb"], b2["dtemb"]), "backward not reproducible"
        _check_grads(b, ref, init, True, tag, with_dx=not io & 2)
        if io & 2:
            _check_stored(b["dx"], ref["dx"], ref["scale"], ref["alts"], ref["dx_plain"], 8e-3, tag + " dx")
        if N % 8 == 0 and io == 3:
            for n in range(N):
                b1 = gn_backward(lib, case, src, st, io=io, n0=n)
                assert torch.equal(b1["dx"][0], b["dx"][n]) and torch.equal(b1["dtemb"][0], b["dtemb"][n]), (tag, n)
    if variant:
        return
    exact = O.gn_mish_ref(inp["x"], inp["gamma"], inp["beta"], G, EPS, inp["temb"], inp["res"])[0]
    models = {}
    for io, dual in ((1, False), (2, False), (3, False), (1, True)):
        tag = f"{case} {params} fwd io {io}{' dual' if dual else ''}"
        f = gn_forward(lib, case, inp, io=io, dual=dual)
        f2 = gn_forward(lib, case, inp, io=io, dual=dual)
        assert torch.equal(f["y"], f2["y"]) and torch.equal(f["stats"], f2["stats"]), "forward not reproducible"
        _check_stats(f["stats"], inp, G, tag)
        own = (f["stats"][..., 0].cpu(), f["stats"][..., 1].cpu())          # the model on the launch's own (checked) statistics
        if io & 2 or dual:
            key = f["stats"].cpu().numpy().tobytes()
            if key not in models:
                models[key] = (O.gn_mish_ref(inp["x"], inp["gamma"], inp["beta"], G, EPS, inp["temb"], inp["res"], stats=own)[0],
                               O.gn_y_scale(inp["x"], inp["gamma"], inp["beta"], G, EPS, inp["temb"], inp["res"], stats=own))
            yr, ys = models[key]
            _check_stored(f["y16"] if dual else f["y"], yr, ys, (), exact, 6e-3, tag + " y")
        if not io & 2:
            e = O.rel(f["y"], exact)
            print(f"{tag}: y {e:.3g}")
            assert f["y"].dtype == F32 and e <= 1e-5, (tag, e)
        if dual:
            assert f["y16"].dtype == BF and torch.equal(f["y16"], f["y"].bfloat16()), "the copy is not bf16(y)"
            assert torch.equal(f["y16"], f2["y16"])
        if N % 8 == 0 and io == 3:
            for n in range(N):
                f1 = gn_forward(lib, case, inp, io=io, n0=n)
                assert torch.equal(f1["y"][0], f["y"][n]) and torch.equal(f1["stats"][0], f["stats"][n]), (tag, n)


# ---------------------------------------------------------------------------------------------------- statistics-only, sum-fed
@pytest.mark.parametrize("case,x16", [((2, 600, 64, 4), False), ((2, 1025, 32, 2), False), ((1, 2100, 32, 2), False),
                                      ((3, 49, 64, 8), True), ((2, 150, 256, 8), True), ((2, 289, 512, 4), True)])
def test_gn_stats_coef(case, x16):
    """mi_gn_stats_coef: the statistics of mi_gn_mish_fwd(_io) bit for bit, and coef = (rstd gamma, beta - mean rstd gamma, temb)."""
    lib = _lib()
    N, HW, C, G = case
    inp = O.gn_inputs(case, bf16_x=x16)
    f = gn_forward(lib, case, inp, io=1 if x16 else None)
    x = In(inp["x"], C + PITCH["x"], BF if x16 else F32)
    ga, be, tb = In(inp["gamma"][None]), In(inp["beta"][None]), In(inp["temb"], C + PITCH["t"])
    runs = []
    for _ in range(2):
        st, coef = Out(N * G, 2), Out(3 * N, C)
        rc = lib.mi_gn_stats_coef(_desc(case, x.ld), x.ptr, ga.ptr, be.ptr, tb.ptr, tb.ld, st.ptr, coef.ptr, int(x16), _stream())
        assert rc == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        runs.append((st.get().view(N, G, 2), coef.get().view(3, N, C)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][0], f["stats"]), "statistics differ from the forward's"
    for got, want, name in zip(runs[0][1], O.coef_ref(inp["x"], inp["gamma"], inp["beta"], G, EPS, inp["temb"]), ("scale", "shift", "tbias")):
        assert _finite(got) and O.rel_max(got, want) <= 2e-6, (case, name, O.rel_max(got, want))


def _sums(inp):
    from src.ops import functional as K
    return K.gn_sums_encode(O.sums_ref(inp["x"])).to(DEV)


def _apply_sums(lib, case, inp, variant, sums, ldx=None, y_off=0):
    """One mi_gn_mish_apply_sums launch -> (rc, y Out, y16 Out or None, stats Out)."""
    N, HW, C, G = case
    x = In(inp["x"], ldx or C + PITCH["x"], BF)
    ga, be, tb = In(inp["gamma"][None]), In(inp["beta"][None]), In(inp["temb"], C + PITCH["t"])
    res = In(inp["res"], C + PITCH["r"]) if "res" in variant else None
    y = Out(N * HW, C, C + PITCH["y"], BF if variant == "bf16" else F32, off=y_off)
    yc = Out(N * HW, C, C + PITCH["y16"], BF) if "copy" in variant else None
    st = Out(N * G, 2)
    rc = lib.mi_gn_mish_apply_sums(_desc(case, x.ld, y.ld, res.ld if res else 0), x.ptr, ctypes.c_void_p(sums.data_ptr()), ga.ptr, be.ptr, tb.ptr, tb.ld,
                                   res.ptr if res else NULL, y.ptr, int(variant == "bf16"), yc.ptr if yc else NULL, yc.ld if yc else 0, st.ptr, _stream())
    torch.cuda.synchronize()
    return rc, y, yc, st


def _coef_from_sums(lib, case, inp, sums):
    N, HW, C, G = case
    ga, be, tb = In(inp["gamma"][None]), In(inp["beta"][None]), In(inp["temb"], C + PITCH["t"])
    st, coef = Out(N * G, 2), Out(3 * N, C)
    rc = lib.mi_gn_coef_from_sums(N, C, G, HW, EPS, ctypes.c_void_p(sums.data_ptr()), ga.ptr, be.ptr, tb.ptr, tb.ld, st.ptr, coef.ptr, _stream())
    assert rc == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    return st.get().view(N, G, 2), coef.get().view(3, N, C)


@pytest.mark.parametrize("variant", ["bf16", "fp32", "fp32+res+copy"])
@pytest.mark.parametrize("case", O.SUMS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gn_sum_fed(case, variant):
    """mi_gn_coef_from_sums and mi_gn_mish_apply_sums on sums built exactly from the stored values."""
    lib = _lib()
    N, HW, C, G = case
    inp = O.gn_inputs(case, bf16_x=True)
    sums = _sums(inp)
    plan = O.apply_sums_plan(HW, C, G, residual="res" in variant)
    assert plan["UNR"] == O.SUMS_UNR[HW]["res" in variant]
    mean, var = O.stats_from_sums_ref(inp["x"], G)
    sref = (mean, 1.0 / torch.sqrt(var + EPS))
    st_c, coef = _coef_from_sums(lib, case, inp, sums)
    assert _finite(st_c, coef)
    assert O.rel_max(st_c[..., 0], sref[0]) <= 2e-6 and O.rel_max(st_c[..., 1], sref[1]) <= 2e-6
    for got, want, name in zip(coef, O.coef_ref(inp["x"], inp["gamma"], inp["beta"], G, EPS, inp["temb"], stats=sref), ("scale", "shift", "tbias")):
        assert O.rel_max(got, want) <= 2e-6, (case, name)
    outs = []
    for _ in range(2):
        rc, y, yc, st = _apply_sums(lib, case, inp, variant, sums)
        assert rc == 0, lib.mi_last_error()
        outs.append((y.get().view(N, HW, C), yc.get().view(N, HW, C) if yc else None, st.get().view(N, G, 2)))
    (y, yc, st), (y2, yc2, st2) = outs
    assert torch.equal(y, y2) and torch.equal(st, st2) and _finite(y, yc, st)
    assert torch.equal(st, st_c), "statistics differ from mi_gn_coef_from_sums'"
    own = (st[..., 0].cpu(), st[..., 1].cpu())
    res = inp["res"] if "res" in variant else None
    yr = O.gn_mish_ref(inp["x"], inp["gamma"], inp["beta"], G, EPS, inp["temb"], res, stats=own)[0]
    exact = O.gn_mish_ref(inp["x"], inp["gamma"], inp["beta"], G, EPS, inp["temb"], res)[0]
    tag = f"{case} sums {variant} UNR {plan['UNR']}"
    if variant == "bf16":
        _check_stored(y, yr, O.gn_y_scale(inp["x"], inp["gamma"], inp["beta"], G, EPS, inp["temb"], res, stats=own), (), exact, 6e-3, tag)
    else:
        e = O.rel(y, exact)
        print(f"{tag}: y {e:.3g}")
        assert y.dtype == F32 and e <= 1e-5, (tag, e)
    if yc is not None:
        assert torch.equal(yc, y.bfloat16()) and torch.equal(yc, yc2)


@pytest.mark.parametrize("how", ["HW24", "ldx4", "y8"])
def test_gn_sum_fed_refusals(how):
    """Shapes mi_gn_mish_apply_sums does not take: it returns 1 and writes nothing."""
    lib = _lib()
    case = (2, 24 if how == "HW24" else 16, 128, 8)
    inp = O.gn_inputs(case, bf16_x=True)
    rc, y, yc, st = _apply_sums(lib, case, inp, "bf16", _sums(inp), ldx=132 if how == "ldx4" else None, y_off=4 if how == "y8" else 0)
    assert rc == 1 and y.untouched() and st.untouched()
    assert O.apply_sums_plan(case[1], 128, 8, pitches=[132 if how == "ldx4" else 136], alignments=[8 if how == "y8" else 0]) is None


def test_gn_sum_fed_constant_slab_and_poison():
    """A constant (sample, group): E[x^2] - mean^2 is clamped at 0 (rstd = 1 / sqrt(eps)).  A poisoned sum: NaN statistics and NaN y for that
    group -- never finite garbage -- and nothing else disturbed."""
    lib = _lib()
    case = (2, 16, 128, 8)
    N, HW, C, G = case
    inp = O.gn_inputs(case, bf16_x=True)
    inp["x"][1, :, 16:32] = 0.75
    sums = _sums(inp)
    rc, y, _, st = _apply_sums(lib, case, inp, "fp32", sums)
    assert rc == 0
    s = st.get().view(N, G, 2)
    assert float(s[1, 1, 0]) == 0.75 and abs(float(s[1, 1, 1]) * math.sqrt(EPS) - 1) <= 2e-6 and _finite(y.get(), s)
    assert torch.equal(s, _coef_from_sums(lib, case, inp, sums)[0])
    sums[(0 * (C // 16) + 2) * 2] = 1 << 62                 # sample 0, slab 2 (group 2): the sum
    rc, y, _, st = _apply_sums(lib, case, inp, "fp32", sums)
    assert rc == 0
    s, yv = st.get().view(N, G, 2), y.get().view(N, HW, C)
    sc, coef = _coef_from_sums(lib, case, inp, sums)
    bad = torch.zeros(N, G, dtype=torch.bool, device=DEV)
    bad[0, 2] = True
    for t in (s, sc):
        assert bool(torch.isnan(t[..., 0][bad]).all()) and _finite(t[~bad])
    assert bool(torch.isnan(yv[0, :, 32:48]).all()) and _finite(yv[0, :, :32], yv[0, :, 48:], yv[1])
    assert bool(torch.isnan(coef[:2, 0, 32:48]).all()) and _finite(coef[:, 1], coef[:, 0, :32], coef[:, 0, 48:])


# ---------------------------------------------------------------------------------------------------- channel LayerNorm
LN_PITCH = dict(x=4, y=8, dy=12, dx=16)


def _ln_fwd(lib, case, inp, y16):
    M, C = case
    x, g, b = In(inp["x"], C + LN_PITCH["x"]), In(inp["g"][None]), In(inp["b"][None])
    y = Out(M, C, C + LN_PITCH["y"], BF if y16 else F32)
    if y16:
        rc = lib.mi_chan_layernorm_fwd_io(M, C, x.ptr, x.ld, g.ptr, b.ptr, O.LN_EPS, y.ptr, y.ld, 1, _stream())
    else:
        rc = lib.mi_chan_layernorm_fwd(M, C, x.ptr, x.ld, g.ptr, b.ptr, O.LN_EPS, y.ptr, y.ld, _stream())
    assert rc == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    out = y.get()
    assert _finite(out)
    return out


def _ln_check_fwd(lib, case, inp, y16):
    M, C = case
    y, y2 = _ln_fwd(lib, case, inp, y16), _ln_fwd(lib, case, inp, y16)
    assert torch.equal(y, y2), "forward not reproducible"
    yr = O.ln_ref(inp["x"], inp["g"], inp["b"], O.LN_EPS)
    tag = f"LayerNorm {case} {'bf16' if y16 else 'fp32'} y"
    if y16:
        _check_stored(y, yr, (yr - inp["b"][None]).abs() + inp["b"][None].abs(), (), yr, 6e-3, tag)
    else:
        e = O.rel(y, yr)
        print(f"{tag}: {e:.3g}")
        assert e <= 1e-5, (tag, e)
    assert torch.equal(y[0].double().cpu(), O.rb(inp["b"]) if y16 else inp["b"]) and torch.equal(y[0], y[M - 1]), "sigma == 0: y = b"


def _ln_bwd(lib, case, inp, dy16, accumulate, part_rows=None):
    M, C = case
    x, g = In(inp["x"], C + LN_PITCH["x"]), In(inp["g"][None])
    dy = In(inp["dy"], C + LN_PITCH["dy"], BF if dy16 else F32)
    dx = Out(M, C, C + LN_PITCH["dx"], init=inp["prev"])
    a = (M, C, x.ptr, x.ld, g.ptr, O.LN_EPS, dy.ptr, dy.ld, dx.ptr, dx.ld, int(accumulate))
    if part_rows is not None:
        part = Out(part_rows + 3, 2 * C)
        rc = lib.mi_chan_layernorm_bwd_part(*a, part.ptr, int(dy16), _stream())
    else:
        init = _init(C)
        dg, db = Out(1, C, init=init["dgamma"]), Out(1, C, init=init["dbeta"])
        if dy16:
            rc = lib.mi_chan_layernorm_bwd_io(*a, dg.ptr, db.ptr, 1, _stream())
        else:
            rc = lib.mi_chan_layernorm_bwd(*a, dg.ptr, db.ptr, _stream())
    assert rc == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    r = dict(dx=dx.get())
    if part_rows is not None:
        p = part.get()
        assert bool((p[:part_rows] != SENT).all()), "a partial row was not written"
        assert bool((p[part_rows:] == SENT).all()), "a row past mi_chan_layernorm_bwd_part_rows was written"
        r.update(dg=p[:part_rows, :C].double().sum(0).cpu(), db=p[:part_rows, C:].double().sum(0).cpu())
    else:
        r.update(dg=dg.get().view(C).double().cpu() - init["dgamma"], db=db.get().view(C).double().cpu() - init["dbeta"])
    assert _finite(*r.values())
    return r


@pytest.mark.parametrize("y16", [False, True], ids=["y32", "y16"])
@pytest.mark.parametrize("case", O.LN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_chan_layernorm_forward(case, y16):
    """mi_chan_layernorm_fwd(_io): pitched x and y, an all-equal pixel in the first and in the last wave (y = b there)."""
    _ln_check_fwd(_lib(), case, O.ln_inputs(case), y16)


@pytest.mark.parametrize("dy16", [False, True], ids=["dy32", "dy16"])
@pytest.mark.parametrize("case", O.LN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_chan_layernorm_backward(case, dy16):
    """mi_chan_layernorm_bwd(_io) and _bwd_part: four distinct pitches, dx written and accumulated onto non-zero content, dg / db added onto
    non-zero content, an all-equal pixel in the first and in the last wave (their dx is 1 / eps times larger than the others': measured apart)."""
    lib = _lib()
    M, C = case
    inp = O.ln_inputs(case, bf16_dy=dy16)
    dxr, dgr, dbr = O.ln_grads_ref(inp["x"], inp["g"], O.LN_EPS, inp["dy"])
    rows = lib.mi_chan_layernorm_bwd_part_rows(M, C)
    assert rows == O.ln_plan(M, C, "bwd")["blocks"]
    mid, ends = slice(1, M - 1), [0, M - 1]
    for acc in (False, True):
        tag = f"LayerNorm {case} {'dy16' if dy16 else 'dy32'} {'accumulate' if acc else 'write'}"
        r = _ln_bwd(lib, case, inp, dy16, acc)
        r2 = _ln_bwd(lib, case, inp, dy16, acc)
        assert torch.equal(r["dx"], r2["dx"]), "dx not reproducible"
        got = r["dx"].double().cpu() - (inp["prev"] if acc else 0.0)
        e = dict(dx=O.rel(got[mid], dxr[mid]), dx_ends=O.rel(got[ends], dxr[ends]), dg=O.rel(r["dg"], dgr), db=O.rel(r["db"], dbr))
        p = _ln_bwd(lib, case, inp, dy16, acc, part_rows=rows)
        assert torch.equal(p["dx"], r["dx"]), "dx of the partial-row variant differs"
        e.update(dg_part=O.rel(p["dg"], dgr), db_part=O.rel(p["db"], dbr))
        print(f"{tag}: " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))
        assert max(e.values()) <= 5e-5, (tag, e)


@pytest.mark.parametrize("y16", [False, True], ids=["y32", "y16"])
def test_chan_layernorm_forward_block_cap(y16):
    """M beyond 4096 workgroups x 4 pixels: the forward's grid-stride loop runs a second iteration."""
    case = O.LN_FWD_ONLY[0]
    assert O.ln_plan(*case)["iterations"] == 2
    _ln_check_fwd(_lib(), case, O.ln_inputs(case), y16)
