"""wgrad_kernel<MODE, BI, BJ>, wgrad_fast_kernel<BI, BJ>, the slab mode and the column sums (csrc/wgrad.hip) on the MI355X against
tests/_igemm_oracle.py, through the C ABI (mi_conv_wgrad, mi_conv_wgrad_slabs, mi_colsum, mi_colsum_ordered): every case of the
oracle's lists (tests/test_igemm_cpu.py holds them to the instantiations and edges they reach), in every mode the case names, with
atomics and -- on the generic kernel -- with slabs, integer-valued and randn operands.  mi_conv_wgrad_plan must name the plan the
oracle's restated planner gives.

Buffers.  P, P2 and Q are views at their pitch inside NaN-filled buffers (NaN in front, behind and in every row's padding).  dW and the
column sums start from non-zero integers between sentinels.  The slab workspace is exactly mi_conv_wgrad_slabs_workspace bytes of NaN
between sentinels: a slab element nobody stored adds NaN, a store past the end hits a sentinel.  Every launch runs twice from the same
start; slab results must be bit-equal between the runs, atomics too with integers.

Integer operands (p in {-4..4}, q in {-3..3}, prior content non-zero in {-3..3}): every partial sum is an integer below 2^24, so dW
must be torch.equal to prior + the float64 reference under atomics and slabs alike.

randn operands: mode 0 against float64 on the fp32 operands, mode 1 against the operands rounded once to bf16 (nearest even).  Bounds:
rel-L2 <= 2e-5 (of the gradient alone) and per element <= (N H W + 2) 2^-24 sum |p||q|, column sums <= (M + 2) 2^-24 sum |x|: N H W + 2
roundings of at most 2^-24 relative each, whatever the order.  Those hold on a launch that starts from zero.  On the non-zero integer
start the prior content p0 counts as a term, as it does in the convolution's bound: the one fp32 add of p0 errs by up to
2^-24 |p0 + s| whatever the kernel does, which sum |p||q| cannot cover where it is small against p0 (N H W = 1).  Both launches run.

The measured figures and the mutation check are in docs/kernels.md, "igemm_conv.hip, wgrad.hip, tests"."""
import ctypes
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _igemm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
WORST = {}
T0 = [0.0]


def _lib():
    from src.ops.lib import load_library
    return load_library()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _wd(d):
    from src.ops.lib import MiWgradDesc
    return ctypes.byref(MiWgradDesc(**d._asdict()))


def _plan(lib, d, al, slab):
    from src.ops.lib import MiWgradPlan
    p = MiWgradPlan()
    assert lib.mi_conv_wgrad_plan(_wd(d), int(al), int(slab), ctypes.byref(p)) == 0, lib.mi_last_error().decode()
    return O.WgradPlan(p.fast, p.big, p.splits, p.chunk, p.xcd_map, p.grid)


@pytest.fixture(scope="module", autouse=True)
def _report():
    T0[0] = time.time()
    yield
    print("\nworst measured: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())) + f"; the file took {time.time() - T0[0]:.1f} s")


def check(tag, fam, kind, got, ref, prior, absref, T):
    """got against prior + ref; the rel-L2 figure is of got - prior against ref."""
    got, ref, prior = got.to(F64).reshape(-1), ref.reshape(-1), prior.reshape(-1)
    assert bool(torch.isfinite(got).all()), (tag, "non-finite")
    if kind == "int":
        bad = (got != ref + prior).nonzero().flatten()
        assert bad.numel() == 0, (tag, f"{bad.numel()} wrong elements, first at {int(bad[0])}: {float(got[bad[0]])} != {float((ref + prior)[bad[0]])}")
        return
    e = O.rel(got - prior, ref)
    worst = float(((got - prior - ref).abs() / ((T + 2) * O.U * (absref.reshape(-1) + prior.abs())).clamp_min(1e-300)).max())
    print(f"{tag}: rel-L2 {e:.3g}, worst element {worst:.3g} of its bound")
    WORST[f"{fam} rel-L2"] = max(WORST.get(f"{fam} rel-L2", 0.0), e)
    WORST[f"{fam} element/bound"] = max(WORST.get(f"{fam} element/bound", 0.0), worst)
    assert e <= 2e-5 and worst <= 1.0, (tag, e, worst)


class Launch:
    def __init__(self, c, mode, ops):
        self.c, self.d = c, O.wg_desc(c, mode)
        d = self.d
        self.P = O.In(ops["P"], d.ldp, off=c.poff, device=DEV)
        self.P2 = O.In(ops["P2"], d.ldp2, device=DEV) if c.I1 else None
        self.Q = O.In(ops["Q"], d.ldq, device=DEV)
        self.dW = O.Out(d.KH * d.KW * d.Ci, d.Cj, init64=ops["prior"], device=DEV)
        self.ws = None
        self.ins = [t for t in (self.P, self.P2, self.Q) if t is not None]

    def ptrs(self):
        return (ctypes.c_void_p(self.P.ptr), ctypes.c_void_p(self.P2.ptr) if self.P2 else None, ctypes.c_void_p(self.Q.ptr), ctypes.c_void_p(self.dW.ptr))

    def run(self, lib, slab, zero=False):
        self.dW.reset()
        if zero:
            self.dW.rows[:, :self.dW.C] = 0.0
        if slab:
            nbytes = lib.mi_conv_wgrad_slabs_workspace(_wd(self.d))
            assert nbytes == O.slabs_workspace(self.d) and nbytes % 4 == 0
            if self.ws is None:
                self.ws = O.Out(1, nbytes // 4, nan=True, device=DEV)
            self.ws.reset()
            rc = lib.mi_conv_wgrad_slabs(_wd(self.d), *self.ptrs(), ctypes.c_void_p(self.ws.ptr), nbytes, _stream())
        else:
            rc = lib.mi_conv_wgrad(_wd(self.d), *self.ptrs(), _stream())
        assert rc == 0, lib.mi_last_error().decode()
        torch.cuda.synchronize()
        if slab:
            self.ws.get()                      # (nothing written outside the workspace)
        return self.dW.get()


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.WG_CASES, ids=repr)
def test_wgrad(case, kind):
    c, lib = case, _lib()
    ops = O.wg_operands(c, kind)
    refs = {}
    T = c.N * c.D[0] * c.D[1]
    for mi, mode in enumerate(c.modes):
        d = O.wg_desc(c, mode)
        rounded = mode == 1 and kind == "randn"
        if rounded not in refs:
            refs[rounded] = O.wg_reference(c, mode, ops, rounded)
        ref, ab = refs[rounded]
        L = Launch(c, mode, ops)
        for slab in (False, True):
            want = O.wgrad_plan(d, O.wg_aligned(c), slab)
            p = _plan(lib, d, O.wg_aligned(c), slab)
            assert p == want and (mi or slab or O.wgrad_plan_name(p, mode) == c.plan), (c, p, want)
            assert not (slab and p.fast)
            name = O.wgrad_plan_name(p, mode) + ("/slab" if slab else "")
            tag = f"{c.name}:{name}:{kind}"
            a, b = L.run(lib, slab), L.run(lib, slab)
            if slab or kind == "int":
                assert O.same_bits(a, b), (tag, "two runs differ")
            assert all(t.intact() for t in L.ins), (tag, "an input was written")
            fam = ("ring" if p.fast else f"generic mode {mode}") + (" slabs" if slab else "")
            for g in (a, b):
                check(tag, fam, kind, g, ref, ops["prior"], ab, T)
            if kind == "randn":                # the bound without a term for the prior content, on a launch that starts from zero
                check(tag + ":from zero", fam, kind, L.run(lib, slab, zero=True), ref, torch.zeros_like(ops["prior"]), ab, T)


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.COLSUM_CASES, ids=lambda t: "m%d_c%d_ld%d_off%d" % t)
def test_colsum(case, kind):
    M, C, ld, off = case
    lib = _lib()
    x = O.operand((M, C), kind, O.seed("colsum", case, kind))
    prior = O.init_content((1, C), O.seed("colsum", case, "p"), "int")
    X = O.In(x, ld, off=off, device=DEV)
    out = O.Out(1, C, init64=prior, device=DEV)
    ref, ab = O.colsum_ref(x), O.colsum_ref(x, absolute=True)
    for ordered in (False, True):
        res = []
        for it in range(3 if kind == "randn" else 2):
            out.reset()
            if it == 2:
                out.rows[:, :C] = 0.0
            if ordered:
                need = lib.mi_colsum_ordered_workspace(M, C)
                assert need == O._cdiv(M, 256) * C * 4
                ws = O.Out(1, need // 4, nan=True, device=DEV)
                rc = lib.mi_colsum_ordered(M, C, ctypes.c_void_p(X.ptr), ld, ctypes.c_void_p(out.ptr), ctypes.c_void_p(ws.ptr), need, _stream())
            else:
                rc = lib.mi_colsum(M, C, ctypes.c_void_p(X.ptr), ld, ctypes.c_void_p(out.ptr), _stream())
            assert rc == 0, lib.mi_last_error().decode()
            torch.cuda.synchronize()
            if ordered:
                ws.get()
            res.append(out.get())
        tag = f"colsum{'_ordered' if ordered else ''}:{case}:{kind}"
        if ordered or kind == "int":
            assert O.same_bits(res[0], res[1]), tag
        assert X.intact(), tag
        for g in res[:2]:
            check(tag, "colsum ordered" if ordered else "colsum", kind, g, ref, prior, ab, M)
        if kind == "randn":
            check(tag + ":from zero", "colsum ordered" if ordered else "colsum", kind, res[2], ref, torch.zeros_like(prior), ab, M)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_dw_and_the_workspace_alone():
    lib = _lib()
    c = O.wg_case("g_two_i1_36")
    L = Launch(c, 1, O.wg_operands(c, "int"))
    d = L.d
    nbytes = O.slabs_workspace(d)
    ws = O.Out(1, nbytes // 4, nan=True, device=DEV)
    n = [0]

    def refused(text, d=d, slab=False, wsp=ws.ptr, wsb=nbytes, **null):
        P, P2, Q, dW = L.ptrs()
        a = dict(P=P, P2=P2, Q=Q, dW=dW)
        for k in null:
            a[k] = None
        dd = _wd(d) if d is not None else None
        if slab:
            rc = lib.mi_conv_wgrad_slabs(dd, a["P"], a["P2"], a["Q"], a["dW"], ctypes.c_void_p(wsp) if wsp else None, wsb, _stream())
        else:
            rc = lib.mi_conv_wgrad(dd, a["P"], a["P2"], a["Q"], a["dW"], _stream())
        torch.cuda.synchronize()
        assert rc != 0 and text in lib.mi_last_error().decode(), (rc, text, lib.mi_last_error().decode())
        assert L.dW.untouched() and ws.untouched(), ("a refused call wrote", text, d, slab)
        n[0] += 1

    for slab in (False, True):
        refused("null argument" if not slab else "needs a workspace", d=None, slab=slab)
        for k in ("P", "Q", "dW"):
            refused("null argument", slab=slab, **{k: 1})
        refused("mode must be 0 or 1", d._replace(mode=2), slab)
        refused("bad two-source split", d._replace(I1=34), slab)
        refused("bad two-source split", d._replace(I1=d.Ci + 4), slab)
        refused("bad two-source split", slab=slab, P2=1)
    refused("needs a workspace", slab=True, wsp=None)
    refused("needs a workspace", slab=True, wsp=ws.ptr + 2)
    refused("workspace smaller than", slab=True, wsb=nbytes - 4)
    # column sums
    out = O.Out(1, 5, init64=O.init_content((1, 5), 3), device=DEV)
    X = O.In(O.ints((300, 5), -4, 4, 1), 8, device=DEV)
    need = lib.mi_colsum_ordered_workspace(300, 5)
    w2 = O.Out(1, need // 4, nan=True, device=DEV)
    for a in ((300, 5, X.ptr, 4, out.ptr, w2.ptr, need), (300, 5, X.ptr, 8, out.ptr, None, need), (300, 5, X.ptr, 8, out.ptr, w2.ptr, need - 4), (300, 5, None, 8, out.ptr, w2.ptr, need)):
        assert lib.mi_colsum_ordered(*a, _stream()) != 0 and "bad argument or workspace" in lib.mi_last_error().decode()
        torch.cuda.synchronize()
        assert out.untouched() and w2.untouched()
    assert lib.mi_colsum(0, 5, X.ptr, 8, out.ptr, _stream()) != 0 and out.untouched()
    assert n[0] >= 18
