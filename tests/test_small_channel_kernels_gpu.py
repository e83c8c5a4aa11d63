"""csrc/small_channel.hip on the MI355X against tests/_small_channel_oracle.py, through the C ABI (load_library(), ctypes, torch's
current stream): every case of the oracle's lists (tests/test_small_channel_cpu.py holds them to the instantiations and edges they
reach), each with integer-valued and with randn operands.

Buffers.  Inputs are views at their pitch inside NaN-filled buffers: NaN in front, behind and in the padding of every row -- for
Cin < 4 at ldx = 4 that includes the image's padding channels, which the 16-byte loads fetch and must not use.  Outputs sit between
sentinels with sentinel padding inside every row, except the padding channels Cs .. 3 of a 4-wide pixel that the small-Cout forward
kernels promise to write as zeros.  dW, and dx under accumulate, start from non-zero small integers.  The workspace is exactly the
bytes mi_conv_small_wgrad_workspace reports inside a NaN-filled buffer whose surroundings must survive; four bytes less must send
the call to the atomic path and leave the buffer untouched.  Every launch runs twice from the same start: workspace-mode dW and every
forward / data-gradient output bit-equal, atomic-mode dW bit-equal with integer operands.

Integer operands (x, bias in {-4..4}, w, dy in {-3..3}, initial content in {-3..3} \\ {0}): every product and partial sum is exact in
fp32 under any order, atomics included, so the result must be torch.equal to the float64 reference cast to fp32 -- for a bf16 output
to the reference rounded to nearest even onto bf16 (27 taps reach sums above 256: the rounding is pinned).  No tolerance.

randn operands: the project's bounds (tests/test_kernels_gpu.py) rel-L2 <= 1e-5, <= 2e-6 for the 1x1 res_conv output, <= 4e-3 for a
bf16 output; and per element |got - ref| <= (T + 2) 2^-24 sum |terms| with T the number of summed terms (ks ks Cin, C, Cs, or N H W
for a weight gradient; bias and prior content count) -- a bf16 output adds its rounding, 2^-8 of the value.  A bf16 output must also be
the fp32 instantiation's output rounded once, bit for bit, and bf16 accumulate follows the model widen, add in fp32, round.

GroupNorm-fused final conv: rel-L2 <= 2e-5 against float64 true Mish on the stored bf16 tensor, and per pixel
|got - ref| <= 4 f (sum_c |mish(z_c)| |w_c| + |bias|) with f the float32 emulation's figure (tests/test_small_channel_cpu.py):
f = 3.5e-7 (emulation 2.94e-7), and f = 4.0e-6 (emulation 3.23e-6) for a sample of constant x, whose x sc + sh cancels at
rstd = 1 / sqrt(eps).

Measured on the MI355X (worst over the cases; not used as bounds): rel-L2 forward 1.2e-7 untiled, 1.3e-7 tiled and dual, bf16 outputs
2.0e-3 (their rounding); weight gradients 1.4e-7 through the workspace, 5.1e-7 with atomics; small-Cout forward 2.4e-7, data gradient
4.9e-8, weight gradient 1.1e-7 / 5.1e-7; the worst fp32 element at 0.54 of its bound (bf16 outputs 0.996: the half ulp).  GroupNorm-fused:
rel-L2 1.4e-6, worst pixel 1.55e-7 of its scale (bound 1.4e-6), constant sample 2.85e-6 (bound 1.6e-5).

What the product library cannot reach: MI_SMALL_CIN_TILED is a constant outside -DMI_EXPERIMENT builds, so the untiled kernels run
on a tiled geometry only where another tiling condition fails (512 / 1024 channels, ldx 8, fp32 dy at 64 channels); and
small_cin3x3_wgrad_tiled_kernel<4, false> has no caller's shape (Cin 4 admits 64 channels only, whose fp32 dy goes untiled)."""
import ctypes
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _small_channel_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -776.0                        # never-written sentinel (exact in bf16)
PAD = 64                             # elements in front of and behind a view
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
U = 2.0 ** -24
WORST = {}
GN_FIGURE, GN_FIGURE_CONST = O.GN_EMUL_FIGURE, O.GN_EMUL_FIGURE_CONST


def _lib():
    from src.ops.lib import load_library
    return load_library()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst measured: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


class In:
    """Rows of t64 [R][C] at pitch ld inside a NaN-filled buffer (NaN in front, behind and in every row's padding); off: elements the view
    is shifted by (1: four bytes past a 16-byte boundary)."""

    def __init__(self, t64, ld=None, dtype=F32, off=0):
        t64 = t64.reshape(-1, t64.shape[-1])
        R, C = t64.shape
        ld = C if ld is None else ld
        assert ld >= C
        self.buf = torch.full((2 * PAD + R * ld + off,), NAN, dtype=dtype, device=DEV)
        rows = self.buf[PAD + off:PAD + off + R * ld].view(R, ld)
        rows[:, :C].copy_(t64.to(dtype))
        self.ptr = rows.data_ptr()
        assert self.ptr % 16 == off * self.buf.element_size()
        self.snap = self.buf.clone()

    def intact(self):
        return _same(self.buf, self.snap)


class Out:
    """R rows of C results at pitch ld between PAD sentinels, sentinel padding inside every row; init64: what the rows hold before the
    launch (else sentinels); zero_to: columns C .. zero_to - 1 must come back exactly 0 (the padding channels a kernel promises to write)."""

    def __init__(self, R, C, ld=None, dtype=F32, init64=None, zero_to=None):
        ld = C if ld is None else ld
        self.R, self.C, self.ld, self.zero_to = R, C, ld, (C if zero_to is None else zero_to)
        self.buf = torch.full((2 * PAD + R * ld,), SENT, dtype=dtype, device=DEV)
        self.rows = self.buf[PAD:PAD + R * ld].view(R, ld)
        if init64 is not None:
            self.rows[:, :C].copy_(init64.reshape(R, C).to(dtype))
        self.ptr = self.rows.data_ptr()
        assert self.ptr % 16 == 0
        self.snap = self.buf.clone()

    def get(self, pad_zero_rows=None):
        assert bool((self.buf[:PAD] == SENT).all()) and bool((self.buf[PAD + self.R * self.ld:] == SENT).all()), "written outside the result"
        assert bool((self.rows[:, self.zero_to:] == SENT).all()), "written into a row's padding"
        z = self.rows[:, self.C:self.zero_to]
        if pad_zero_rows is not None:
            z = z[pad_zero_rows]
        assert bool((_bits(z) == 0).all()), "a padding channel of the 4-wide pixel is not +0"
        return self.rows[:, :self.C].cpu()

    def untouched(self):
        return _same(self.buf, self.snap)


class Ws:
    """Exactly nbytes of workspace inside a NaN-filled buffer."""

    def __init__(self, nbytes):
        assert nbytes % 16 == 0
        self.nbytes, self.n = nbytes, nbytes // 4
        self.buf = torch.full((2 * PAD + self.n,), NAN, dtype=F32, device=DEV)
        self.ptr = self.buf[PAD:].data_ptr()
        assert self.ptr % 16 == 0

    def check(self):
        assert bool(torch.isnan(self.buf[:PAD]).all()) and bool(torch.isnan(self.buf[PAD + self.n:]).all()), "written outside the workspace"

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def _ws_args(mode, need):
    """-> (Ws or None, pointer, bytes passed).  'short': the whole buffer is there, the call is told four bytes less."""
    if mode == "null":
        return None, None, 0
    ws = Ws(need)
    return ws, ws.ptr, need if mode == "full" else need - 4


def _check(tag, kind, got, ref, absref, T, bound, what="y"):
    """got: the result (cpu, fp32 or bf16); ref: float64 reference; absref: the same sum over |terms|; T: summed terms per element."""
    out16 = got.dtype == BF
    got, ref, absref = got.to(F64).reshape(-1), ref.reshape(-1), absref.reshape(-1)
    assert bool(torch.isfinite(got).all()), (tag, what, "non-finite")
    if kind == "int":
        want = ref.to(F32).to(BF).to(F64) if out16 else ref.to(F32).to(F64)
        bad = (got != want).nonzero().flatten()
        assert bad.numel() == 0, (tag, what, f"{bad.numel()} wrong elements, first at {int(bad[0])}: {float(got[bad[0]])} != {float(want[bad[0]])}")
        return
    e = O.rel(got, ref)
    el = (T + 2) * U * absref
    if out16:
        el = el + 2.0 ** -8 * (ref.abs() + el)
        bound = 4e-3
    worst = float(((got - ref).abs() / el.clamp_min(1e-300)).max())
    fam = tag.split(":")[0] + (" bf16" if out16 else "")
    _note(f"{fam} {what} rel-L2", e)
    _note(f"{fam} {what} element/bound", worst)
    assert e <= bound and worst <= 1.0, (tag, what, e, worst)


def _twice(tag, launch, exact=True):
    """launch() -> tuple of cpu tensors.  Two runs from the same start; exact: bit-equal."""
    a, b2 = launch(), launch()
    if exact:
        for i, (x, y) in enumerate(zip(a, b2)):
            assert _same(x, y), (tag, f"output {i} differs between two runs")
    return a


# ---------------------------------------------------------------------------------------------------- Cin <= 4: forward
class CinFwd:
    """One image / weight / bias set at a case's pitches, launched through any of the forward entry points."""

    def __init__(self, name, kind, ks, N, H, W, Cin, Cout, ldx, xoff, bias):
        self.g = (ks, N, H, W, Cin, Cout)
        self.ldx, self.M = ldx, N * H * W
        self.x = O.operand((N, H, W, Cin), kind, _seed(name, "x", kind))
        self.w = O.operand((ks, ks, Cin, Cout), kind, _seed(name, "w", ks, kind), amp=3, scale=0.2 if ks == 3 else 0.5)
        self.b = O.operand((Cout,), kind, _seed(name, "b", ks, kind)) if bias else None
        self.X, self.Wt = In(self.x, ldx, off=xoff // 4), In(self.w.reshape(-1, Cout))
        self.B = In(self.b.reshape(1, -1)) if bias else None
        self.ref = O.conv_fwd_ref(self.x, self.w, self.b, ks)
        self.absref = O.conv_fwd_ref(self.x.abs(), self.w.abs(), self.b.abs() if bias else None, ks)
        self.T = ks * ks * Cin + int(bias)

    def launch(self, lib, ldy, y16, entry="io"):
        ks, N, H, W, Cin, Cout = self.g
        y = Out(self.M, Cout, ldy, BF if y16 else F32)
        bp = self.B.ptr if self.B else None
        if entry == "io":
            rc = lib.mi_conv_small_cin_fwd_io(ks, N, H, W, Cin, Cout, self.X.ptr, self.ldx, self.Wt.ptr, bp, y.ptr, ldy, int(y16), _stream())
        elif entry == "v2":
            rc = lib.mi_conv_small_cin_fwd(ks, N, H, W, Cin, Cout, self.X.ptr, self.ldx, self.Wt.ptr, bp, y.ptr, ldy, _stream())
        else:
            rc = lib.mi_conv3x3_small_cin_fwd(N, H, W, Cin, Cout, self.X.ptr, self.ldx, self.Wt.ptr, bp, y.ptr, ldy, _stream())
        assert rc == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        return (y.get(),)

    def intact(self):
        return self.X.intact() and self.Wt.intact() and (self.B is None or self.B.intact())

    def check(self, tag, kind, y):
        _check(tag, kind, y, self.ref, self.absref, self.T, 2e-6 if self.g[0] == 1 else 1e-5)


def run_fwd(lib, c, kind):
    tag = ("fwd_tiled" if c.name.startswith("tiled") else "fwd") + ":" + c.name
    ldy = O.ldy_of(c.Cout, c.ldyk)
    f = CinFwd(c.name, kind, c.ks, c.N, c.H, c.W, c.Cin, c.Cout, c.ldx, c.xoff, c.bias)
    y, = _twice(tag, lambda: f.launch(lib, ldy, c.y16))
    f.check(tag, kind, y)
    if c.y16:                                   # the bf16 output is the fp32 instantiation's, rounded once
        y32, = f.launch(lib, ldy, False)
        f.check(tag, kind, y32)
        assert _same(y, y32.to(BF)), (tag, "bf16 output != fp32 output rounded")
    assert f.intact()


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.FWD_CASES, ids=repr)
def test_small_cin_fwd_untiled(case, kind):
    run_fwd(_lib(), case, kind)


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.TILED_CASES, ids=repr)
def test_small_cin_fwd_tiled(case, kind):
    run_fwd(_lib(), case, kind)


# ---------------------------------------------------------------------------------------------------- the dual launch and its chores
def run_dual(lib, c, kind):
    tag = "dual:" + c.name
    N, H, W, Cin, Cout = c.N, c.H, c.W, c.Cin, c.Cout
    ldy3, ldy1 = O.ldy_of(Cout, c.ldyk), O.ldy_of(Cout, (c.ldyk + 1) % 3)
    f3 = CinFwd(c.name, kind, 3, N, H, W, Cin, Cout, 4, 0, True)
    f1 = CinFwd(c.name, kind, 1, N, H, W, Cin, Cout, 4, 0, c.bias1)
    g = torch.Generator().manual_seed(_seed(c.name, "chores"))
    table = torch.randn(50, max(c.gather_row, 4), generator=g).to(DEV)
    idx = torch.tensor(([3, 49, 3, 0, 3, 17, 49] * 3)[:max(c.gather_n, 1)], dtype=torch.int64, device=DEV)
    nz = c.zero_bytes // 8

    def launch():
        y3, y1 = Out(f3.M, Cout, ldy3, BF if c.y16 else F32), Out(f3.M, Cout, ldy1)
        b1 = f1.B.ptr if f1.B else None
        pool = torch.full((nz + 32,), 7, dtype=torch.int64, device=DEV)
        rows = Out(max(c.gather_n, 1), max(c.gather_row, 4))
        if c.zero_bytes or c.gather_row:
            rc = lib.mi_conv_small_cin_fwd_dual_chores(N, H, W, Cin, Cout, f3.X.ptr, 4, f3.Wt.ptr, f3.B.ptr, y3.ptr, ldy3, int(c.y16), f1.Wt.ptr, b1, y1.ptr, ldy1,
                                                       pool[16:].data_ptr() if nz else None, c.zero_bytes, table.data_ptr() if c.gather_row else None,
                                                       idx.data_ptr() if c.gather_row else None, rows.ptr if c.gather_row else None, c.gather_row, c.gather_n, _stream())
        else:
            rc = lib.mi_conv_small_cin_fwd_dual(N, H, W, Cin, Cout, f3.X.ptr, 4, f3.Wt.ptr, f3.B.ptr, y3.ptr, ldy3, int(c.y16), f1.Wt.ptr, b1, y1.ptr, ldy1, _stream())
        assert rc == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        assert bool((pool[:16] == 7).all()) and bool((pool[16 + nz:] == 7).all()) and not bool(pool[16:16 + nz].any()), (tag, "zero fill")
        if c.gather_row:
            assert _same(rows.get(), table[idx].cpu()), (tag, "row gather")
        else:
            assert rows.untouched()
        return y3.get(), y1.get()
    y3, y1 = _twice(tag, launch)
    f3.check(tag, kind, y3)
    f1.check(tag, kind, y1)
    r3, = f3.launch(lib, ldy3, c.y16)
    r1, = f1.launch(lib, ldy1, False)
    assert _same(y3, r3), (tag, "y3 != the single 3x3 launch")
    assert _same(y1, r1) or O.rel(y1, r1) <= 2e-7, (tag, "y1 != the 1x1 launch", O.rel(y1, r1))
    assert f3.intact() and f1.intact()


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.DUAL_CASES, ids=repr)
def test_small_cin_fwd_dual_and_chores(case, kind):
    run_dual(_lib(), case, kind)


# ---------------------------------------------------------------------------------------------------- Cin <= 4: weight gradient
def run_wg(lib, c, kind):
    tag = ("wgrad_tiled" if c.name.startswith("wgt") else "wgrad") + ":" + c.name
    ks, N, H, W, Cin, Cout = c.ks, c.N, c.H, c.W, c.Cin, c.Cout
    M, na, lddy = N * H * W, ks * ks * Cin, Cout + 8 * c.lddyk
    x = O.operand((N, H, W, Cin), kind, _seed(c.name, "x", kind))
    dy = O.operand((N, H, W, Cout), kind, _seed(c.name, "dy", kind), bf16=c.dy16, amp=3)
    init = O.init_content((na * Cout,), _seed(c.name, "init"))
    X, DY = In(x, c.ldx, off=c.xoff // 4), In(dy, lddy, BF if c.dy16 else F32)
    ref = init + O.conv_wgrad_ref(x, dy, ks).reshape(-1)
    absref = init.abs() + O.conv_wgrad_ref(x.abs(), dy.abs(), ks).reshape(-1)
    need = lib.mi_conv_small_wgrad_workspace(na * Cout)
    assert need == O.small_wgrad_workspace(na * Cout)
    for mode in O.WS_MODES:
        plan = O.wg_plan(c, {"full": need, "null": 0, "short": need - 4}[mode])

        def launch():
            dW = Out(1, na * Cout, init64=init)
            ws, wp, wb = _ws_args(mode, need)
            rc = lib.mi_conv_small_cin_wgrad_io(ks, N, H, W, Cin, Cout, X.ptr, c.ldx, DY.ptr, lddy, int(c.dy16), dW.ptr, wp, wb, _stream())
            assert rc == 0, lib.mi_last_error()
            torch.cuda.synchronize()
            if ws:
                ws.check()
                assert mode == "full" or ws.untouched(), (tag, "a short workspace was written")
            return (dW.get(),)
        dW, = _twice(f"{tag}:{mode}", launch, exact=plan["reduce"] == "ws" or kind == "int")
        _check(tag, kind, dW, ref, absref, M + 1, 1e-5, "dW " + plan["reduce"])
    assert X.intact() and DY.intact()


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.WG_CASES, ids=repr)
def test_small_cin_wgrad_untiled(case, kind):
    run_wg(_lib(), case, kind)


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.WGT_CASES, ids=repr)
def test_small_cin_wgrad_tiled(case, kind):
    run_wg(_lib(), case, kind)


# ---------------------------------------------------------------------------------------------------- Cs <= 4: the three ops and the one-pass backward
def _cout_io(lib, op, M, C, Cs, a, lda, bp, ldb, wp, biasp, out, ldo, acc, wide16, wsp=None, wsb=0, entry="io"):
    if entry == "io":
        return lib.mi_conv1x1_small_cout_io(op, M, C, Cs, a, lda, bp, ldb, wp, biasp, out, ldo, int(acc), int(wide16), wsp, wsb, _stream())
    if entry == "ws":
        return lib.mi_conv1x1_small_cout_ws(op, M, C, Cs, a, lda, bp, ldb, wp, biasp, out, ldo, int(acc), wsp, wsb, _stream())
    return lib.mi_conv1x1_small_cout(op, M, C, Cs, a, lda, bp, ldb, wp, biasp, out, ldo, int(acc), _stream())


def run_c0(lib, c, kind):
    tag = "cout_fwd:" + c.name
    M, C, Cs = c.M, c.C, c.Cs
    x = O.operand((M, C), kind, _seed(c.name, "x", kind), bf16=c.x16)
    w = O.operand((C, Cs), kind, _seed(c.name, "w", kind), amp=3, scale=0.1)
    bias = O.operand((Cs,), kind, _seed(c.name, "b", kind)) if c.bias else None
    lda = C + 8 * c.ldak
    X, Wt, B = In(x, lda, BF if c.x16 else F32), In(w.reshape(1, -1)), In(bias.reshape(1, -1)) if c.bias else None

    def launch():
        y = Out(M, Cs, c.ldo, zero_to=min(c.ldo, 4))          # ldo >= 4 > Cs: channels Cs .. 3 come back 0; ldo == Cs: nothing behind the pixel
        rc = _cout_io(lib, 0, M, C, Cs, X.ptr, lda, None, 0, Wt.ptr, B.ptr if B else None, y.ptr, c.ldo, 0, c.x16)
        assert rc == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        return (y.get(),)
    y, = _twice(tag, launch)
    _check(tag, kind, y, O.cout_fwd_ref(x, w, bias), O.cout_fwd_ref(x.abs(), w.abs(), bias.abs() if c.bias else None), C + int(c.bias), 1e-5)
    assert X.intact() and Wt.intact() and (B is None or B.intact())
    if c.ldo >= 4 > Cs:
        # the padding channels are written as zeros, not as products with zero weights: an Inf in x reaches the pixel's Cs channels only
        m, x2 = M // 2, x.clone()
        x2[m, 5] = float("inf")
        X = In(x2, lda, BF if c.x16 else F32)
        y2, = launch()                              # (Out.get() holds channels Cs .. 3 of every pixel to +0)
        keep = torch.arange(M) != m
        assert _same(y2[keep], y[keep]) and not bool(torch.isfinite(y2[m][w[5] != 0]).any()), (tag, "Inf in x")


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.C0_CASES, ids=repr)
def test_small_cout_fwd(case, kind):
    run_c0(_lib(), case, kind)


def _dgrad(lib, M, C, Cs, DY, lddy, Wt, ldo, dx16, acc, init):
    dx = Out(M, C, ldo, BF if dx16 else F32, init64=init if acc else None)
    rc = _cout_io(lib, 1, M, C, Cs, DY.ptr, lddy, None, 0, Wt.ptr, None, dx.ptr, ldo, acc, dx16)
    assert rc == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    return (dx.get(),)


def run_c1(lib, c, kind):
    tag = "cout_dgrad:" + c.name
    M, C, Cs = c.M, c.C, c.Cs
    dy = O.operand((M, Cs), kind, _seed(c.name, "dy", kind), amp=3)
    w = O.operand((C, Cs), kind, _seed(c.name, "w", kind), amp=3, scale=0.1)
    init = O.init_content((M, C), _seed(c.name, "init"), bf16=True, kind=kind)       # (bf16-representable: both storages start from the same values)
    ldo = C + 8 * c.ldok
    DY, Wt = In(dy, c.lddy), In(w.reshape(1, -1))
    ref = O.cout_dgrad_ref(dy, w) + (init if c.acc else 0)
    absref = O.cout_dgrad_ref(dy.abs(), w.abs()) + (init.abs() if c.acc else 0)
    dx, = _twice(tag, lambda: _dgrad(lib, M, C, Cs, DY, c.lddy, Wt, ldo, c.dx16, c.acc, init))
    _check(tag, kind, dx, ref, absref, Cs + int(c.acc), 1e-5, "dx")
    if c.dx16:                                  # bf16 dx: the fp32 instantiation's result rounded once (accumulate: widen, add in fp32, round)
        dx32, = _dgrad(lib, M, C, Cs, DY, c.lddy, Wt, ldo, False, c.acc, init)
        _check(tag, kind, dx32, ref, absref, Cs + int(c.acc), 1e-5, "dx")
        assert _same(dx, dx32.to(BF)), (tag, "bf16 dx != fp32 dx rounded")
    assert DY.intact() and Wt.intact()


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.C1_CASES, ids=repr)
def test_small_cout_dgrad(case, kind):
    run_c1(_lib(), case, kind)


def run_c2(lib, c, kind):
    tag = "cout_wgrad:" + c.name
    M, C, Cs = c.M, c.C, c.Cs
    x = O.operand((M, C), kind, _seed(c.name, "x", kind), bf16=c.x16)
    dy = O.operand((M, Cs), kind, _seed(c.name, "dy", kind), amp=3)
    w = O.operand((C, Cs), kind, _seed(c.name, "w", kind), amp=3, scale=0.1)
    winit = O.init_content((C * Cs,), _seed(c.name, "winit"))
    xinit = O.init_content((M, C), _seed(c.name, "xinit"), bf16=True, kind=kind)
    ldx, lddx, lddy = C + 8 * c.ldak, C + 8 * (1 - c.ldak), 4
    X, DY, Wt = In(x, ldx, BF if c.x16 else F32), In(dy, lddy), In(w.reshape(1, -1))
    wref, wabs = winit + O.cout_wgrad_ref(x, dy).reshape(-1), winit.abs() + O.cout_wgrad_ref(x.abs(), dy.abs()).reshape(-1)
    dref = O.cout_dgrad_ref(dy, w) + (xinit if c.acc else 0)
    dabs = O.cout_dgrad_ref(dy.abs(), w.abs()) + (xinit.abs() if c.acc else 0)
    need = lib.mi_conv_small_wgrad_workspace(4 * C)
    assert need == O.small_wgrad_workspace(4 * C)
    dx1, = _dgrad(lib, M, C, Cs, DY, lddy, Wt, lddx, c.dx16, c.acc, xinit)
    _check(tag, kind, dx1, dref, dabs, Cs + int(c.acc), 1e-5, "dx")
    for mode in O.WS_MODES:
        reduce = O.plan_cout(2, M, C, Cs, c.x16, {"full": need, "null": 0, "short": need - 4}[mode])["reduce"]
        exact = reduce == "ws" or kind == "int"

        def op2():
            dW = Out(1, C * Cs, init64=winit)
            ws, wp, wb = _ws_args(mode, need)
            rc = _cout_io(lib, 2, M, C, Cs, X.ptr, ldx, DY.ptr, lddy, None, None, dW.ptr, Cs, 0, c.x16, wp, wb)
            assert rc == 0, lib.mi_last_error()
            torch.cuda.synchronize()
            if ws:
                ws.check()
                assert mode == "full" or ws.untouched(), (tag, "a short workspace was written")
            return (dW.get(),)

        def bwd():
            dW, dx = Out(1, C * Cs, init64=winit), Out(M, C, lddx, BF if c.dx16 else F32, init64=xinit if c.acc else None)
            ws, wp, wb = _ws_args(mode, need)
            rc = lib.mi_conv1x1_small_cout_bwd(M, C, Cs, X.ptr, ldx, int(c.x16), DY.ptr, lddy, Wt.ptr, dW.ptr, dx.ptr, lddx, int(c.dx16), int(c.acc), wp, wb, _stream())
            assert rc == 0, lib.mi_last_error()
            torch.cuda.synchronize()
            if ws:
                ws.check()
                assert mode == "full" or ws.untouched(), (tag, "a short workspace was written")
            return dW.get(), dx.get()
        dW2, = _twice(f"{tag}:op2:{mode}", op2, exact)
        _check(tag, kind, dW2, wref, wabs, M + 1, 1e-5, "dW " + reduce)
        a, b2 = bwd(), bwd()
        assert _same(a[1], b2[1]) and (not exact or _same(a[0], b2[0])), (tag, mode, "the one-pass backward differs between two runs")
        _check(tag, kind, a[0], wref, wabs, M + 1, 1e-5, "dW one-pass " + reduce)
        assert _same(a[1], dx1), (tag, mode, "one-pass dx != op 1")
        assert not exact or _same(a[0], dW2), (tag, mode, "one-pass dW != op 2")
    assert X.intact() and DY.intact() and Wt.intact()


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.C2_CASES, ids=repr)
def test_small_cout_wgrad_and_one_pass_backward(case, kind):
    run_c2(_lib(), case, kind)


# ---------------------------------------------------------------------------------------------------- GroupNorm + Mish in the final conv's load
def run_gn(lib, c):
    tag = "cout_gn:" + c.name
    N, HW, C, G, Cs = c.N, c.HW, c.C, c.G, c.Cs
    M, ldx = N * HW, C + 8 * c.ldxk
    x = O.bf16_round(O.randn((N, HW, C), _seed(c.name, "x")) * 1.3 + 0.2)
    if c.special == "const":
        x[1] = 0.75
    gamma, beta = O.randn((C,), _seed(c.name, "g")).abs() * 0.5 + 0.5, O.randn((C,), _seed(c.name, "be")) * 0.3
    w = O.randn((C, Cs), _seed(c.name, "w")) * 0.1
    bias = O.randn((Cs,), _seed(c.name, "b")) if c.bias else None
    sums = O.gn_sums(x)
    if c.special == "poison":
        sums[1, 2, 1] = 1 << 62
    X, Ga, Be, Wt = In(x, ldx, BF), In(gamma.reshape(1, -1)), In(beta.reshape(1, -1)), In(w.reshape(1, -1))
    B = In(bias.reshape(1, -1)) if c.bias else None
    sbuf = torch.full((sums.numel() + 32,), 1 << 62, dtype=torch.int64, device=DEV)
    sbuf[16:16 + sums.numel()].copy_(sums.view(-1))
    good = torch.ones(N, dtype=torch.bool)
    if c.special == "poison":
        good[1] = False
    good_px = good.repeat_interleave(HW)

    def launch():
        y = Out(M, Cs, 4, zero_to=4)
        rc = lib.mi_conv1x1_small_cout_gn_fwd(M, HW, C, Cs, X.ptr, ldx, sbuf[16:].data_ptr(), Ga.ptr, Be.ptr, G, 1e-5, Wt.ptr, B.ptr if B else None, y.ptr, 4, _stream())
        assert rc == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        return (y.get(pad_zero_rows=good_px.to(DEV)),)      # (a poisoned sample's padding channels are NaN x 0)
    y, = _twice(tag, launch)
    y = y.view(N, HW, Cs).to(F64)
    ref = O.gn_mish_conv_ref(x, sums, gamma, beta, G, 1e-5, w, bias)
    ab = O.gn_mish_conv_ref(x, sums, gamma, beta, G, 1e-5, w, bias, absolute=True)
    assert bool(torch.isnan(y[~good]).all()) and bool(torch.isfinite(y[good]).all()), (tag, "a poisoned sample is NaN, the others finite")
    e = O.rel(y[good], ref[good])
    ratio = (y - ref).abs() / ab
    plain = good.clone()
    if c.special == "const":
        plain[1] = False
        worst_c = float(ratio[1].max())
        _note("cout_gn constant sample pixel/scale", worst_c)
        assert worst_c <= 4 * GN_FIGURE_CONST, (tag, worst_c)
    worst = float(ratio[plain].max())
    _note("cout_gn rel-L2", e)
    _note("cout_gn pixel/scale", worst)
    assert e <= 2e-5 and worst <= 4 * GN_FIGURE, (tag, e, worst)
    assert X.intact() and Ga.intact() and Be.intact() and Wt.intact() and (B is None or B.intact())


@pytest.mark.parametrize("case", O.GN_CASES, ids=repr)
def test_small_cout_groupnorm_mish_in_the_load(case):
    run_gn(_lib(), case)


# ---------------------------------------------------------------------------------------------------- ABI-v1 wrappers
@pytest.mark.parametrize("kind", ["int", "randn"])
def test_abi_v1_wrappers_are_the_io_forms(kind):
    lib = _lib()
    f = CinFwd("abi", kind, 3, 2, 7, 7, 3, 64, 4, 0, True)
    y, = f.launch(lib, 68, False)
    assert _same(y, f.launch(lib, 68, False, "v2")[0]) and _same(y, f.launch(lib, 68, False, "v1")[0])
    f1 = CinFwd("abi", kind, 1, 2, 7, 7, 3, 64, 4, 0, True)
    assert _same(f1.launch(lib, 64, False)[0], f1.launch(lib, 64, False, "v2")[0])
    # weight gradients: v1 always takes the atomic path (bit-equal with integers; any order stays inside the derived bound)
    dy = O.operand((2, 7, 7, 64), kind, _seed("abi", "dy", kind), amp=3)
    DY = In(dy, 72)
    init = O.init_content((27 * 64,), 5)
    need = lib.mi_conv_small_wgrad_workspace(27 * 64)
    ref, ab = init + O.conv_wgrad_ref(f.x, dy, 3).reshape(-1), init.abs() + O.conv_wgrad_ref(f.x.abs(), dy.abs(), 3).reshape(-1)

    def wg(entry, mode):
        dW = Out(1, 27 * 64, init64=init)
        ws, wp, wb = _ws_args(mode, need)
        if entry == "io":
            rc = lib.mi_conv_small_cin_wgrad_io(3, 2, 7, 7, 3, 64, f.X.ptr, 4, DY.ptr, 72, 0, dW.ptr, wp, wb, _stream())
        elif entry == "v2":
            rc = lib.mi_conv_small_cin_wgrad(3, 2, 7, 7, 3, 64, f.X.ptr, 4, DY.ptr, 72, dW.ptr, wp, wb, _stream())
        else:
            rc = lib.mi_conv3x3_small_cin_wgrad(2, 7, 7, 3, 64, f.X.ptr, 4, DY.ptr, 72, dW.ptr, _stream())
        assert rc == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        return dW.get()
    assert _same(wg("io", "full"), wg("v2", "full"))
    a, v1 = wg("io", "null"), wg("v1", "null")
    _check("abi:v1", kind, v1, ref, ab, 99, 1e-5, "dW")
    assert kind != "int" or _same(a, v1)
    # mi_conv1x1_small_cout (no workspace) and mi_conv1x1_small_cout_ws
    M, C, Cs = 98, 64, 3
    x, d3 = O.operand((M, C), kind, 11), O.operand((M, Cs), kind, 12, amp=3)
    w, bias = O.operand((C, Cs), kind, 13, amp=3, scale=0.1), O.operand((Cs,), kind, 14)
    X, D3, Wt, B = In(x, C + 8), In(d3, 4), In(w.reshape(1, -1)), In(bias.reshape(1, -1))
    winit = O.init_content((C * Cs,), 15)
    need = lib.mi_conv_small_wgrad_workspace(4 * C)

    def call(entry, op, mode="null"):
        ws, wp, wb = _ws_args(mode, need)
        if op == 0:
            out = Out(M, Cs, 4, zero_to=4)
            rc = _cout_io(lib, 0, M, C, Cs, X.ptr, C + 8, None, 0, Wt.ptr, B.ptr, out.ptr, 4, 0, 0, wp, wb, entry)
        elif op == 1:
            out = Out(M, C, C + 8)
            rc = _cout_io(lib, 1, M, C, Cs, D3.ptr, 4, None, 0, Wt.ptr, None, out.ptr, C + 8, 0, 0, wp, wb, entry)
        else:
            out = Out(1, C * Cs, init64=winit)
            rc = _cout_io(lib, 2, M, C, Cs, X.ptr, C + 8, D3.ptr, 4, None, None, out.ptr, Cs, 0, 0, wp, wb, entry)
        assert rc == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        return out.get()
    for op in (0, 1):
        assert _same(call("io", op), call("ws", op)) and _same(call("io", op), call("v1", op))
    assert _same(call("io", 2, "full"), call("ws", 2, "full"))
    v1 = call("v1", 2)
    _check("abi:v1", kind, v1, winit + O.cout_wgrad_ref(x, d3).reshape(-1), winit.abs() + O.cout_wgrad_ref(x.abs(), d3.abs()).reshape(-1), M + 1, 1e-5, "dW")
    assert kind != "int" or (_same(call("io", 2), v1) and _same(call("ws", 2, "short"), v1))


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_everything_untouched():
    """Every condition of every MI_REQUIRE in the file and each reason of the three *_supported functions: a non-zero return, no launch,
    outputs and workspace as they were.  The oracle's *_accepts says beforehand that each call is one the host checks refuse."""
    lib = _lib()
    big = 1 << 18
    x = In(torch.zeros(big // 8, 8, dtype=F64))
    x16 = In(torch.zeros(big // 8, 8, dtype=F64), dtype=BF)
    w = In(torch.zeros(1, 27 * 1024, dtype=F64))
    bias = In(torch.zeros(1, 1024, dtype=F64))
    out, out2, ws = Out(1, big), Out(1, big), Ws(1 << 20)
    sums = torch.zeros(4096, dtype=torch.int64, device=DEV)
    idx = torch.zeros(16, dtype=torch.int64, device=DEV)
    n = [0]

    def refused(rc, what):
        n[0] += 1
        assert rc != 0, ("accepted", what)
        assert lib.mi_last_error(), what
        assert out.untouched() and out2.untouched() and ws.untouched(), ("written", what)

    # ---- mi_conv_small_cin_fwd_io
    ok = dict(ks=3, N=2, H=7, W=7, Cin=3, Cout=64, ldx=4, ldy=64, x_off=0, y_off=0, w_off=0, y_bf16=False)
    t16 = dict(ok, H=8, W=8, y_bf16=True)
    assert O.cin_fwd_accepts(**ok) and O.cin_fwd_accepts(**t16)
    bad = [dict(ok, ks=2), dict(ok, Cin=0), dict(ok, Cin=5), dict(ok, Cout=0), dict(ok, Cout=6), dict(ok, Cout=12), dict(ok, Cout=20), dict(ok, Cout=1028),
           dict(ok, ldy=66), dict(ok, y_off=8), dict(ok, w_off=8), dict(t16, y_off=4), dict(t16, H=28, W=28), dict(t16, ldx=3), dict(t16, Cout=512),
           dict(t16, N=3, H=4, W=8), dict(t16, x_off=4), dict(ok, y_bf16=True)]
    for a in bad:
        assert not O.cin_fwd_accepts(**a), a
        refused(lib.mi_conv_small_cin_fwd_io(a["ks"], a["N"], a["H"], a["W"], a["Cin"], a["Cout"], x.ptr + a["x_off"], a["ldx"], w.ptr + a["w_off"], bias.ptr,
                                             out.ptr + a["y_off"], a["ldy"], int(a["y_bf16"]), _stream()), ("fwd", a))
    for px, pw, py in ((None, w.ptr, out.ptr), (x.ptr, None, out.ptr), (x.ptr, w.ptr, None)):
        refused(lib.mi_conv_small_cin_fwd_io(3, 2, 7, 7, 3, 64, px, 4, pw, bias.ptr, py, 64, 0, _stream()), "fwd null pointer")
    # ---- mi_conv_small_cin_fwd_dual[_chores]
    dk = dict(N=2, H=8, W=8, Cin=3, Cout=64, ldx=4, ldy3=64, ldy1=64, x_off=0, y3_off=0, y1_off=0, w3_off=0, w1_off=0, y3_bf16=False)
    assert O.cin_dual_accepts(**dk)
    bad = [dict(dk, N=0), dict(dk, Cin=0), dict(dk, Cin=5), dict(dk, Cout=0), dict(dk, Cout=6), dict(dk, Cout=12), dict(dk, Cout=20), dict(dk, Cout=512), dict(dk, H=28, W=28),
           dict(dk, H=4), dict(dk, ldx=8), dict(dk, ldx=3), dict(dk, x_off=4), dict(dk, ldy3=66), dict(dk, ldy1=66), dict(dk, y3_off=8), dict(dk, y3_off=4, y3_bf16=True),
           dict(dk, y1_off=8), dict(dk, w3_off=8), dict(dk, w1_off=8)]
    for a in bad:
        assert not O.cin_dual_accepts(**a), a
        refused(lib.mi_conv_small_cin_fwd_dual(a["N"], a["H"], a["W"], a["Cin"], a["Cout"], x.ptr + a["x_off"], a["ldx"], w.ptr + a["w3_off"], bias.ptr, out.ptr + a["y3_off"],
                                               a["ldy3"], int(a["y3_bf16"]), w.ptr + a["w1_off"], bias.ptr, out2.ptr + a["y1_off"], a["ldy1"], _stream()), ("dual", a))
    assert not lib.mi_conv_small_cin_fwd_dual_supported(2, 8, 8, 3, 64, 8) and lib.mi_conv_small_cin_fwd_dual_supported(2, 8, 8, 3, 64, 4)
    zero = torch.full((64,), 7, dtype=torch.int64, device=DEV)
    zsnap = zero.clone()
    chores = [dict(zero=True, zero_bytes=12), dict(zero=True, zero_bytes=8, zero_off=4), dict(zero=False, gather=True, gather_row=6, gather_n=2),
              dict(zero=False, gather=True, gather_row=4, gather_n=0), dict(zero=False, gather=True, gather_row=4, gather_n=2, src_off=8),
              dict(zero=False, gather=True, gather_row=4, gather_n=2, dst_off=8), dict(zero=False, gather=True, gather_row=0, gather_n=2)]
    for a in chores:
        assert not O.chores_accept(**a), a
        g = a.get("gather", False)
        refused(lib.mi_conv_small_cin_fwd_dual_chores(2, 8, 8, 3, 64, x.ptr, 4, w.ptr, bias.ptr, out.ptr, 64, 0, w.ptr, bias.ptr, out2.ptr, 64,
                                                      zero.data_ptr() + a.get("zero_off", 0) if a["zero"] else None, a.get("zero_bytes", 0),
                                                      bias.ptr + a.get("src_off", 0) if g else None, idx.data_ptr() if g else None, ws.ptr + a.get("dst_off", 0) if g else None,
                                                      a.get("gather_row", 0), a.get("gather_n", 0), _stream()), ("chores", a))
    refused(lib.mi_conv_small_cin_fwd_dual_chores(2, 8, 8, 3, 64, x.ptr, 4, w.ptr, bias.ptr, out.ptr, 64, 0, w.ptr, bias.ptr, out2.ptr, 64, None, 0, None, idx.data_ptr(), ws.ptr,
                                                  4, 2, _stream()), "gather without a source")
    assert torch.equal(zero, zsnap)
    # ---- mi_conv_small_cin_wgrad_io
    wk = dict(ks=3, N=2, H=7, W=7, Cin=3, Cout=128, ldx=4, lddy=128, x_off=0, dy_off=0, dy_bf16=False)
    w16 = dict(wk, H=8, W=8, dy_bf16=True)
    assert O.cin_wgrad_accepts(**wk) and O.cin_wgrad_accepts(**w16)
    bad = [dict(wk, ks=2), dict(wk, Cin=0), dict(wk, Cin=5), dict(wk, Cout=32), dict(wk, Cout=512), dict(wk, Cout=256), dict(wk, Cin=4), dict(wk, lddy=130), dict(wk, dy_off=8),
           dict(w16, dy_off=4), dict(w16, H=28, W=28), dict(w16, ldx=3), dict(w16, N=3, H=4, W=8), dict(w16, x_off=4), dict(wk, dy_bf16=True)]
    for a in bad:
        assert not O.cin_wgrad_accepts(**a), a
        refused(lib.mi_conv_small_cin_wgrad_io(a["ks"], a["N"], a["H"], a["W"], a["Cin"], a["Cout"], x.ptr + a["x_off"], a["ldx"], x16.ptr + a["dy_off"], a["lddy"], int(a["dy_bf16"]),
                                               out.ptr, ws.ptr, ws.nbytes, _stream()), ("wgrad", a))
    refused(lib.mi_conv_small_cin_wgrad(3, 2, 7, 7, 3, 256, x.ptr, 4, w.ptr, 256, out.ptr, ws.ptr, ws.nbytes, _stream()), "wgrad v2 3x256")
    refused(lib.mi_conv3x3_small_cin_wgrad(2, 7, 7, 4, 128, x.ptr, 4, w.ptr, 128, out.ptr, _stream()), "wgrad v1 4x128")
    for px, pd, po in ((None, w.ptr, out.ptr), (x.ptr, None, out.ptr), (x.ptr, w.ptr, None)):
        refused(lib.mi_conv_small_cin_wgrad_io(3, 2, 7, 7, 3, 128, px, 4, pd, 128, 0, po, ws.ptr, ws.nbytes, _stream()), "wgrad null pointer")
    # ---- mi_conv1x1_small_cout_io / _bwd
    for op, M, C, Cs, lda, ldo, a_off, o_off, w16_, has_b in [(3, 5, 64, 3, 64, 4, 0, 0, 0, 1), (0, 5, 256, 3, 256, 4, 0, 0, 0, 1), (2, 5, 32, 3, 32, 3, 0, 0, 0, 1),
                                                              (0, 5, 64, 0, 64, 4, 0, 0, 0, 1), (0, 5, 64, 5, 64, 8, 0, 0, 0, 1), (0, 0, 64, 3, 64, 4, 0, 0, 0, 1),
                                                              (1, 0, 64, 3, 4, 64, 0, 0, 0, 1), (0, 5, 48, 3, 48, 4, 0, 0, 0, 1), (1, 5, 512, 3, 4, 512, 0, 0, 0, 1),
                                                              (0, 5, 64, 3, 66, 4, 0, 0, 0, 1), (0, 5, 64, 3, 64, 4, 8, 0, 0, 1), (0, 5, 64, 3, 64, 4, 4, 0, 1, 1),
                                                              (1, 5, 64, 3, 4, 66, 0, 0, 0, 1), (1, 5, 64, 3, 4, 64, 0, 8, 0, 1), (1, 5, 64, 3, 4, 64, 0, 4, 1, 1),
                                                              (2, 5, 64, 3, 66, 3, 0, 0, 0, 1), (2, 5, 64, 3, 64, 3, 8, 0, 0, 1), (2, 5, 64, 3, 64, 3, 0, 0, 0, 0)]:
        assert not O.cout_accepts(op, M, C, Cs, lda, ldo, a_off, o_off, bool(w16_), bool(has_b))
        refused(lib.mi_conv1x1_small_cout_io(op, M, C, Cs, x.ptr + a_off, lda, w.ptr if has_b else None, 4, w.ptr, bias.ptr, out.ptr + o_off, ldo, 0, w16_, ws.ptr, ws.nbytes,
                                             _stream()), ("cout", op, M, C, Cs, lda, ldo, a_off, o_off, w16_, has_b))
    refused(lib.mi_conv1x1_small_cout_io(0, 5, 64, 3, x.ptr, 64, None, 0, None, bias.ptr, out.ptr, 4, 0, 0, None, 0, _stream()), "cout forward without weights")
    refused(lib.mi_conv1x1_small_cout(3, 5, 64, 3, x.ptr, 64, None, 0, w.ptr, bias.ptr, out.ptr, 4, 0, _stream()), "cout v1 op 3")
    for M, C, Cs, ldx, lddx, x_off, dx_off, xb, db in [(5, 32, 3, 32, 32, 0, 0, 0, 0), (5, 64, 0, 64, 64, 0, 0, 0, 0), (5, 64, 5, 64, 64, 0, 0, 0, 0), (0, 64, 3, 64, 64, 0, 0, 0, 0),
                                                       (5, 64, 3, 66, 64, 0, 0, 0, 0), (5, 64, 3, 64, 66, 0, 0, 0, 0), (5, 64, 3, 64, 64, 8, 0, 0, 0), (5, 64, 3, 64, 64, 4, 0, 1, 0),
                                                       (5, 64, 3, 64, 64, 0, 8, 0, 0), (5, 64, 3, 64, 64, 0, 4, 0, 1)]:
        assert not O.cout_bwd_accepts(M, C, Cs, ldx, lddx, x_off, dx_off, bool(xb), bool(db))
        refused(lib.mi_conv1x1_small_cout_bwd(M, C, Cs, x.ptr + x_off, ldx, xb, w.ptr, 4, w.ptr, out.ptr, out2.ptr + dx_off, lddx, db, 0, ws.ptr, ws.nbytes, _stream()),
                ("bwd", M, C, Cs, ldx, lddx, x_off, dx_off, xb, db))
    # ---- mi_conv1x1_small_cout_gn_fwd
    gk = dict(M=72, HW=36, C=64, Cs=3, G=4, ldx=64, ldy=4, x_off=0, y_off=0)
    assert O.cout_gn_accepts(**gk)
    for a in [dict(gk, C=32), dict(gk, C=256), dict(gk, G=8), dict(gk, G=0), dict(gk, G=3), dict(gk, M=70), dict(gk, M=0), dict(gk, HW=0), dict(gk, ldy=8), dict(gk, ldy=3),
              dict(gk, ldx=66), dict(gk, x_off=4), dict(gk, y_off=8), dict(gk, Cs=0), dict(gk, Cs=5)]:
        assert not O.cout_gn_accepts(**a), a
        refused(lib.mi_conv1x1_small_cout_gn_fwd(a["M"], a["HW"], a["C"], a["Cs"], x16.ptr + a["x_off"], a["ldx"], sums.data_ptr(), bias.ptr, bias.ptr, a["G"], 1e-5, w.ptr, bias.ptr,
                                                 out.ptr + a["y_off"], a["ldy"], _stream()), ("gn", a))
    refused(lib.mi_conv1x1_small_cout_gn_fwd(72, 36, 64, 3, x16.ptr, 64, None, bias.ptr, bias.ptr, 4, 1e-5, w.ptr, bias.ptr, out.ptr, 4, _stream()), "gn without sums")
    refused(lib.mi_conv1x1_small_cout_gn_fwd(72, 36, 64, 3, x16.ptr, 64, sums.data_ptr() + 8, bias.ptr, bias.ptr, 4, 1e-5, w.ptr, bias.ptr, out.ptr, 4, _stream()), "gn sums 8 bytes off")
    refused(lib.mi_conv1x1_small_cout_gn_fwd(72, 36, 64, 3, x16.ptr, 64, sums.data_ptr(), bias.ptr + 8, bias.ptr, 4, 1e-5, w.ptr, bias.ptr, out.ptr, 4, _stream()), "gn gamma 8 bytes off")
    torch.cuda.synchronize()
    assert x.intact() and x16.intact() and w.intact() and bias.intact() and n[0] >= 100
