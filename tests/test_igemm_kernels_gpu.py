"""igemm_kernel<MODE, BM, BN> and igemm_fast_kernel<BM, BN, IN16> (csrc/igemm_conv.hip) on the MI355X against tests/_igemm_oracle.py,
through the C ABI (mi_conv_igemm, mi_conv_igemm_bf16w, mi_conv_igemm_bf16w_io; load_library(), ctypes, torch's current stream): every
case of the oracle's list (tests/test_igemm_cpu.py holds the list to the sixteen instantiations and the edges it reaches), in every
variant the case names, with integer-valued and with randn operands.  After every launch mi_conv_igemm_plan must name the plan the
oracle's restated planner gives.

Buffers.  x, x2, the weights (fp32 in either layout, or the bf16 copy [tap][Nc][K]), bias and residual are views at their pitch inside
NaN-filled buffers: NaN in front, behind and in every row's padding (K = 1 / 3 at ldx = 4: the padding channels are NaN).  y sits
between sentinels with sentinel padding in every row (ldy = Nc + 3 unless the case sets it); with accumulate it starts from non-zero
integers, a k-sliced case without accumulate starts from NaN.  Every launch runs twice from the same start and the two results must be
bit-equal (except k-slices adding randn values atomically); inputs must come back intact.

Integer operands (x in {-4..4}, w in {-3..3}, bias / residual / prior content in {-3..3}): every value is exact in bf16 and every
partial sum is an integer below 2^24 (tests/test_igemm_cpu.py), so y must be torch.equal to the float64 reference in both modes, on
both kernels, under atomics too.  No tolerance: one wrong, dropped or doubled (pixel, tap, channel) is a wrong integer.

randn operands: mode 0 against float64 on the fp32 operands, mode 1 against float64 on the operands rounded once to bf16, to nearest
even (the bf16 weight copy and bf16-stored x are rounded before they are stored).  Bounds: the project's rel-L2 <= 2e-5 and per element
|got - ref| <= (T + 2) 2^-24 (sum |x||w| + |bias| + |res| + |prior|), T the summed terms (most taps of a parity class times K, plus
the epilogue's operands): T + 2 roundings of at most 2^-24 relative each, whatever the order.  Nothing is fitted to the kernel.

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
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
WORST = {}
T0 = [0.0]


def _lib():
    from src.ops.lib import load_library
    return load_library()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cd(d):
    from src.ops.lib import MiConvDesc
    return ctypes.byref(MiConvDesc(**d._asdict()))


def _plan(lib, d, wb, i16, al):
    from src.ops.lib import MiIgemmPlan
    p = MiIgemmPlan()
    assert lib.mi_conv_igemm_plan(_cd(d), int(wb), int(i16), int(al), ctypes.byref(p)) == 0, lib.mi_last_error().decode()
    return O.IgemmPlan(p.kernel, p.bm, p.bn, p.classes, p.ragged, p.ksplit, tuple(p.ntap), tuple(p.stages))


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    T0[0] = time.time()
    yield
    print("\nworst measured: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())) + f"; the file took {time.time() - T0[0]:.1f} s")


def check(tag, fam, kind, got, ref, absref, T):
    got, ref = got.to(F64).reshape(-1), ref.reshape(-1)
    assert bool(torch.isfinite(got).all()), (tag, "non-finite")
    if kind == "int":
        bad = (got != ref).nonzero().flatten()
        assert bad.numel() == 0, (tag, f"{bad.numel()} wrong elements, first at {int(bad[0])}: {float(got[bad[0]])} != {float(ref[bad[0]])}")
        return
    e = O.rel(got, ref)
    worst = float(((got - ref).abs() / ((T + 2) * O.U * absref.reshape(-1)).clamp_min(1e-300)).max())
    print(f"{tag}: rel-L2 {e:.3g}, worst element {worst:.3g} of its bound")
    _note(f"{fam} rel-L2", e)
    _note(f"{fam} element/bound", worst)
    assert e <= 2e-5 and worst <= 1.0, (tag, e, worst)


class Launch:
    """The device operands of one variant of a case and its launch."""

    def __init__(self, c, kind, mode, wb, i16, ops):
        self.c, self.d = c, O.conv_desc(c, mode)
        d = self.d
        r = O.bf16_round
        xdt = BF if i16 else F32
        self.x = O.In(r(ops["x"]) if i16 else ops["x"], d.ldx, xdt, off=c.xoff, device=DEV)
        self.x2 = O.In(r(ops["x2"]) if i16 else ops["x2"], d.ldx2, xdt, device=DEV) if c.K1 else None
        if wb:
            self.w = O.In(r(ops["W"]).transpose(1, 2).contiguous().reshape(1, -1), dtype=BF, device=DEV)
        else:
            self.w = O.In(O.w_memory(ops["W"], d.w_kn).reshape(1, -1), off=c.woff, device=DEV)
        self.bias = O.In(ops["bias"].reshape(1, -1), device=DEV) if ops["bias"] is not None else None
        self.res = O.In(ops["res"], d.ldr, device=DEV) if ops["res"] is not None else None
        R = d.N * d.OH * d.OW
        self.y = O.Out(R, d.Nc, d.ldy, init64=ops["prior"], nan=ops["prior"] is None and d.ldy == d.Nc, device=DEV)
        self.wb, self.i16 = wb, i16
        self.ins = [t for t in (self.x, self.x2, self.w, self.bias, self.res) if t is not None]

    def args(self):
        p = lambda t: ctypes.c_void_p(t.ptr) if t is not None else None  # noqa: E731
        return p(self.x), p(self.x2), p(self.w), p(self.bias), p(self.res), ctypes.c_void_p(self.y.ptr)

    def run(self, lib):
        self.y.reset()
        a = self.args()
        if self.i16:
            rc = lib.mi_conv_igemm_bf16w_io(_cd(self.d), *a, 1, _stream())
        elif self.wb:
            rc = lib.mi_conv_igemm_bf16w(_cd(self.d), *a, _stream())
        else:
            rc = lib.mi_conv_igemm(_cd(self.d), *a, _stream())
        assert rc == 0, lib.mi_last_error().decode()
        torch.cuda.synchronize()
        return self.y.get()


def _family(p, i16, mode):
    return ("ring" + ("16" if i16 else "")) if p.kernel else f"generic mode {mode}" + (" k-sliced" if p.ksplit > 1 else "")


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.CONV_CASES, ids=repr)
def test_conv(case, kind):
    c, lib = case, _lib()
    ops = O.conv_operands(c, kind)
    refs = {}
    for vi, (mode, wb, i16) in enumerate(O.conv_variants(c)):
        d = O.conv_desc(c, mode)
        want = O.igemm_plan(d, wb, i16, O.conv_aligned(c))
        p = _plan(lib, d, wb, i16, O.conv_aligned(c))
        assert p == want and (vi or O.igemm_plan_name(p, mode, i16) == c.plan), (c, p, want)
        rounded = mode == 1 and kind == "randn"
        if rounded not in refs:
            refs[rounded] = O.conv_reference(c, mode, ops, rounded)
        ref, ab = refs[rounded]
        L = Launch(c, kind, mode, wb, i16, ops)
        y1, y2 = L.run(lib), L.run(lib)
        tag = f"{c.name}:{O.igemm_plan_name(p, mode, i16)}:{kind}"
        if not (p.ksplit > 1 and kind == "randn"):
            assert O.same_bits(y1, y2), (tag, "two runs differ")
        assert all(t.intact() for t in L.ins), (tag, "an input was written")
        for y in (y1, y2):
            check(tag, _family(p, i16, mode), kind, y, ref, ab, O.conv_terms(c, mode))


def test_wb_and_fp32_weights_agree_on_the_generic_kernel():
    """The same ragged transposed layer through mi_conv_igemm (fp32 weights, mode 1) and through the bf16 copy: bit-equal integers and,
    with randn, the same rounded operands -- so the same sums up to the order the MFMA adds them, which is the same code."""
    c, lib = O.conv_case("wb_ragged_4to7"), _lib()
    for kind in ("int", "randn"):
        ops = O.conv_operands(c, kind)
        a = Launch(c, kind, 1, True, False, ops).run(lib)
        b = Launch(c._replace(wb=False), kind, 1, False, False, ops).run(lib)
        assert O.same_bits(a, b), kind


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_y_alone():
    lib = _lib()
    c = O.conv_case("ring_t3_k128_two_x16")
    ops = O.conv_operands(c, "int")
    L16 = Launch(c, "int", 1, True, True, ops)
    L32 = Launch(c._replace(in16=False), "int", 1, True, False, ops)
    g = O.conv_case("two_k1_36")
    Lg = Launch(g, "int", 0, False, False, O.conv_operands(g, "int"))
    n = [0]

    def refused(L, entry, d=None, text=None, **kw):
        d = L.d if d is None else d
        x, x2, w, b, r, y = L.args()
        a = dict(x=x, x2=x2, w=w, y=y)
        for k, v in kw.items():
            a[k] = None if v is None else ctypes.c_void_p(a[k].value + v)
        dd = _cd(d) if d != "null" else None
        if entry == "io":
            rc = lib.mi_conv_igemm_bf16w_io(dd, a["x"], a["x2"], a["w"], b, r, a["y"], 1, _stream())
        elif entry == "wb":
            rc = lib.mi_conv_igemm_bf16w(dd, a["x"], a["x2"], a["w"], b, r, a["y"], _stream())
        else:
            rc = lib.mi_conv_igemm(dd, a["x"], a["x2"], a["w"], b, r, a["y"], _stream())
        torch.cuda.synchronize()
        assert rc != 0, ("accepted", entry, d, kw)
        assert text is None or text in lib.mi_last_error().decode(), (lib.mi_last_error().decode(), text)
        assert L.y.untouched(), ("y written by a refused call", entry, d, kw)
        n[0] += 1

    d = Lg.d
    refused(Lg, "fp32", "null", "null argument")
    for k in ("x", "w", "y"):
        refused(Lg, "fp32", text="null argument", **{k: None})
    for f in ("N", "K", "Nc", "KH", "KW", "stride"):
        refused(Lg, "fp32", d._replace(**{f: 0}), "bad sizes")
        refused(Lg, "fp32", d._replace(**{f: -2}), "bad sizes")
    refused(Lg, "fp32", d._replace(mode=2), "mode must be 0")
    refused(Lg, "fp32", d._replace(K1=34), "bad two-source split")
    refused(Lg, "fp32", d._replace(K1=d.K + 4), "bad two-source split")
    refused(Lg, "fp32", text="bad two-source split", x2=None)
    refused(Lg, "fp32", d._replace(ldx=d.ldx + 2), "ldx must be a multiple of 4")
    refused(Lg, "fp32", d._replace(ldy=d.Nc - 1), "ldy >= Nc")
    refused(Lg, "fp32", d._replace(ldr=d.Nc - 1), "ldr < Nc")
    refused(Lg, "fp32", d._replace(transposed=1, stride=2, KH=1, KW=2), "kernel smaller than stride")
    d = L32.d
    refused(L32, "wb", d._replace(mode=0), "needs mode 1")
    refused(L32, "wb", d._replace(K=d.K + 4), "needs mode 1")
    refused(L32, "wb", text="needs mode 1", w=8)
    refused(L32, "wb", text="needs mode 1", w=None)
    d = L16.d
    assert O.io_supported(d) and lib.mi_conv_igemm_bf16w_io_supported(_cd(d)) == 1
    for bad in (d._replace(mode=0), d._replace(K=d.K + 32), d._replace(K1=32), d._replace(ldx=d.ldx + 4), d._replace(ldx2=d.ldx2 + 4), d._replace(KH=5, KW=5),
                d._replace(KH=1, KW=1), d._replace(OH=7, OW=7), d._replace(stride=3), d._replace(KH=1, KW=2), d._replace(ldy=d.Nc - 4)):
        assert lib.mi_conv_igemm_bf16w_io_supported(_cd(bad)) == 0 == O.io_supported(bad), bad
        refused(L16, "io", bad, "mi_conv_igemm_bf16w_io: bf16 activations need")
    refused(L16, "io", text="mi_conv_igemm_bf16w_io: bf16 activations need", x=8)
    refused(L16, "io", text="mi_conv_igemm_bf16w_io: bf16 activations need", x2=8)
    refused(L16, "io", text="mi_conv_igemm_bf16w_io: bf16 activations need", w=8)
    assert n[0] >= 40 and all(t.intact() for L in (L16, L32, Lg) for t in L.ins)
