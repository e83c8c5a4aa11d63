"""conv1x1_pw_kernel, conv_gt_kernel and ln_conv1x1_pw_kernel (csrc/conv_pw.hip) on the MI355X against tests/_conv_stream_oracle.py, through
the C ABI (load_library(), ctypes, torch's current stream): every case of the oracle's lists (tests/test_conv_stream_cpu.py holds them to the
instantiations and edges they reach), fp32 and bf16 output where both exist, with integer-valued and with randn operands.

Buffers, as in tests/test_conv_pw_kernels_gpu.py (whose In / Out classes these are): x, x2, residual, bias, the LayerNorm's g / b, the
fragment-order weights and the per-sample weight batches are views at their pitch inside NaN-filled buffers -- NaN in front, behind and in
every row's padding (with ldx = 3 K the other two thirds of a row are NaN); bias, g and b are exactly their length.  y, the bf16 copy and
the normalised tensor sit between sentinels with sentinel padding inside every row; with accumulate y starts from non-zero content.  Every
launch runs twice from the same start and must be bit-equal; inputs must come back intact.

Integer operands (x in {-4..4}, w in {-3..3}, bias / residual / prior content small integers, T 12 < 2^24 asserted by the oracle): fp32 y
must be torch.equal to the float64 reference, bf16 y to the reference rounded to nearest even, bf16 accumulate is widen, add in fp32, round,
the bf16 copies equal bf16(y).  No tolerance, in bf16 mode, the fp32-input form and exact-fp32 mode.  randn operands: the project's
rel-L2 bounds (tests/test_kernels_gpu.py) -- 1x1: 1e-5 fp32 output, 6e-3 bf16 output, 2e-6 _f32; gather: 2e-5 bf16 mode, 4e-3 bf16 output,
3e-6 fp32 mode -- and per element |got - ref| <= (T + 2) 2^-24 sum |terms|, T the contraction length (the gather: that pixel's valid taps
x K; bias, residual and prior content count as terms), a bf16 output adding 2^-8 of its value.  Bit for bit: a bf16 output is the fp32
instantiation's output rounded once (the bias-in-registers path of a bf16 output without residual or accumulate included); _x32 is
mi_conv1x1_pw on bf16(x); the channel-tile loop is the 2-D grid; a batched launch is its samples launched with their own weights;
mi_conv_gt_dual's y is mi_conv_gt's; mi_conv_gt with k = 1, s = 1, p = 0 is mi_conv1x1_pw (integer operands).

LayerNorm + 1x1.  Exact family (eps = 0, pixel = 2^e x a balanced +-1 pattern, integer g / b / weights): ln_out torch.equal to
pattern g + b, y to the integer contraction + bias rounded to bf16.  x = 1.7 randn - 0.4 with ordinary and with wide (gamma, beta): at most
0.1 % of ln_out may differ from bf16(float64 LN), each by at most one bf16 ulp of the larger magnitude or, where the terms cancel,
2^-19 (|x-hat gamma| + |beta|); y against the conv of the kernel's own ln_out within (K + 2) 2^-24 sum |terms| + 2^-8 of the value; the plain
entry's y bit-equal to the dual's.  x = 100 + 0.1 randn: one bf16 ulp plus the oracle's change when the mean moves by 8 2^-24 |mean|.
Constant pixels with eps = 1e-5: ln_out = bf16(beta) exactly.

Measured on the MI355X (worst over the cases; figures, not bounds; the module prints them at its end).  1x1: fp32 output rel-L2 1.1e-7, worst
element 0.016 of its bound; bf16 output 1.7e-3 and 0.99 (its rounding, the half ulp); _f32 2.4e-7 and 0.081.  Gather: bf16 mode 2.7e-7 and
0.022; bf16 output 1.7e-3 and 0.99; fp32 mode 8.6e-7 and 0.058.  LayerNorm: 6.1e-5 (ordinary) / 6.9e-5 (wide parameters) of ln_out off the
bit model, every one by exactly one bf16 ulp; y 0.99 of its bound against the conv of the kernel's own ln_out (the half ulp) and rel-L2
2.4e-3 / 2.5e-3 against unrounded float64; x = 100 + 0.1 randn: 2.7 % of ln_out off the bit model, worst element 0.99 of its bound.  The
file's 425 tests take 14.8 s.

What the product library cannot reach: gt_plan's "dy or dx outside -8..7" (pad <= 7 and k <= 4 keep every offset inside -3..7); see
docs/kernels.md, "conv_pw.hip (1x1, tap-gather, LayerNorm + 1x1), tests"."""
import ctypes
import os
import sys
from contextlib import contextmanager

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_stream_oracle as O  # noqa: E402
from test_conv_pw_kernels_gpu import BF, DEV, F32, F64, NAN, PAD, In, Out, _cd, _K, _lib, _same, _stream, _twice  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
WORST = {}
REL = {("pw1", False): 1e-5, ("pw1", True): 6e-3, ("pw1f32", False): 2e-6, ("gt", False): 2e-5, ("gt", True): 4e-3, ("gtf32", False): 3e-6}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst measured: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


@contextmanager
def nloop(knob):
    """mi_debug_conv1x1_pw_nloop's state for the launches inside (0: 2-D grid, 1: the product's rule, 2: the loop from any grid); restored,
    with the 3x3 suite's tile hook and the query cache, on the way out."""
    lib, K = _lib(), _K()
    was = lib.mi_debug_conv1x1_pw_nloop(knob)
    K._QUERY_CACHE.clear()
    try:
        yield lib
    finally:
        lib.mi_debug_conv1x1_pw_nloop(was)
        lib.mi_debug_conv_pw_tile(0)
        K._QUERY_CACHE.clear()


class InAt(In):
    """In with the view starting col0 elements into every row (x in the second third of rows of 3 K): the columns in front are NaN too."""

    def __init__(self, t64, ld, dtype, col0):
        t64 = t64.reshape(-1, t64.shape[-1])
        R, C = t64.shape
        assert col0 + C <= ld
        self.buf = torch.full((2 * PAD + R * ld,), NAN, dtype=dtype, device=DEV)
        rows = self.buf[PAD:PAD + R * ld].view(R, ld)
        rows[:, col0:col0 + C].copy_(t64.to(dtype))
        self.ptr = rows[:, col0:].data_ptr()
        assert self.ptr % 16 == 0
        self.snap = self.buf.clone()


def _check(tag, fam, kind, got, ref, absref, T, what="y"):
    """got: the result (cpu, fp32 or bf16); ref: float64 reference; absref: the same sum over |terms|; T: summed terms per element."""
    out16 = got.dtype == BF
    got = got.to(F64).reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), (tag, what, "non-finite")
    if kind == "int":
        want = O.stored(ref, out16)
        bad = (got != want).reshape(-1).nonzero().flatten()
        assert bad.numel() == 0, (tag, what, f"{bad.numel()} wrong elements, first at {int(bad[0])}: "
                                  f"{float(got.reshape(-1)[bad[0]])} != {float(want.reshape(-1)[bad[0]])}")
        return
    e = O.rel(got, ref)
    el = (T + 2) * U * absref
    if out16:
        el = el + 2.0 ** -8 * (ref.abs() + el)
    worst = float(((got - ref).abs() / el.clamp_min(1e-300)).max())
    name = fam + (" bf16" if out16 else "")
    _note(f"{name} {what} rel-L2", e)
    _note(f"{name} {what} element/bound", worst)
    assert e <= REL[(fam, out16)] and worst <= 1.0, (tag, what, e, worst)


# ---------------------------------------------------------------------------------------------------- 1x1
class Pw1:
    def __init__(self, c, kind, ops=None):
        self.c, self.kind = c, kind
        ops = self.ops = ops or O.pw1_operands(c, kind)
        self.ref, self.absref = O.pw1_reference(ops, round_x=c.form == "x32")
        self.d = d = O.pw1_desc(c)
        xdt, wdt = (BF if c.form == "bf16" else F32), (F32 if c.form == "f32" else BF)
        self.X = InAt(ops["x"], d.ldx, xdt, c.xoff)
        self.X2 = In(ops["x2"], d.ldx2, xdt) if ops["x2"] is not None else None
        self.wbatch = O.pw1_wbatch(c)
        G = ops["G"] if c.hw else ops["G"][None]
        frags = torch.stack([O.wfq(g[None], c.form == "f32").reshape(-1) for g in G])
        self.Wt = In(frags, self.wbatch or None, wdt)
        self.B = In(ops["bias"].reshape(1, -1)) if ops["bias"] is not None else None
        self.R = In(ops["res"], d.ldr) if ops["res"] is not None else None
        self.M, self.T = c.M, c.K + len(c.epi)

    def launch(self, lib, out16, dual=False, sample=None, form=None):
        """sample: the whole batch through mi_conv1x1_pw with that sample's weights."""
        c, d = self.c, self.d
        y = Out(self.M, c.Nc, d.ldy, BF if out16 else F32, init64=self.ops["prior"])
        y16 = Out(self.M, c.Nc, c.Nc + c.ldy16, BF) if dual else None
        x2, b, r = (self.X2.ptr if self.X2 else None), (self.B.ptr if self.B else None), (self.R.ptr if self.R else None)
        y16a = (y16.ptr if dual else None, (c.Nc + c.ldy16) if dual else 0)
        form = form or c.form
        if form == "x32":
            rc = lib.mi_conv1x1_pw_x32(_cd(d), self.X.ptr, x2, self.Wt.ptr, b, r, y.ptr, int(out16), _stream())
        elif form == "f32":
            rc = lib.mi_conv1x1_pw_f32(_cd(d), self.X.ptr, x2, self.Wt.ptr, b, r, y.ptr, _stream())
        elif c.hw and sample is None:
            rc = lib.mi_conv1x1_pw_batched(_cd(d), self.X.ptr, self.Wt.ptr, self.wbatch, b, r, y.ptr, int(out16), *y16a, _stream())
        else:
            w = self.Wt.ptr + (sample or 0) * self.wbatch * 2
            rc = lib.mi_conv1x1_pw(_cd(d), self.X.ptr, x2, w, b, r, y.ptr, int(out16), *y16a, _stream())
        assert rc == 0, (c, lib.mi_last_error())
        torch.cuda.synchronize()
        return (y.get(), y16.get()) if dual else (y.get(),)

    def intact(self):
        return all(b is None or b.intact() for b in (self.X, self.X2, self.Wt, self.B, self.R))

    def check(self, tag, y):
        _check(tag, "pw1f32" if self.c.form == "f32" else "pw1", self.kind, y, self.ref, self.absref, self.T)


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.PW1_CASES, ids=repr)
def test_1x1_cases(case, kind):
    """Shapes, chunk counts, two sources, pitches, the eight epilogue forms on both outputs, the bf16 copy, both tiles with the plain and the
    flattened grid, the channel-tile loop and every condition that switches it off, per-sample weights, fp32 input, exact fp32."""
    c = case
    with nloop(c.knob) as lib:
        f = Pw1(c, kind)
        sup = {"bf16": lib.mi_conv1x1_pw_supported, "x32": lib.mi_conv1x1_pw_x32_supported, "f32": lib.mi_conv1x1_pw_f32_supported}[c.form]
        assert sup(_cd(f.d)) == 1
        tag = f"pw1:{c.name}:{kind}"
        y32, = _twice(tag, lambda: f.launch(lib, False))
        f.check(tag, y32)
        if c.form != "f32":
            y16, = _twice(tag, lambda: f.launch(lib, True))
            f.check(tag, y16)
            assert _same(y16, y32.to(BF)), (tag, "bf16 output != fp32 output rounded once")
        if c.ldy16 >= 0:
            yd, cp = _twice(tag, lambda: f.launch(lib, False, dual=True))
            assert _same(yd, y32), (tag, "y of the launch with a bf16 copy != y of the launch without")
            assert _same(cp, yd.to(BF)), (tag, "bf16 copy != bf16(y)")
        assert f.intact(), (tag, "an input changed")


@pytest.mark.parametrize("case", O.PW1_NLOOP_CASES, ids=repr)
def test_channel_tile_loop_equals_the_2d_grid(case):
    c = case
    f = Pw1(c, "randn")
    assert O.pw1_plan(f.d, "bf16", True, knob=2).nloop and not O.pw1_plan(f.d, "bf16", True, knob=0).nloop
    with nloop(2) as lib:
        a, = f.launch(lib, True)
    with nloop(0) as lib:
        b, = f.launch(lib, True)
    assert _same(a, b), c
    assert f.intact()


@pytest.mark.parametrize("case", O.PW1_X32_CASES, ids=repr)
def test_fp32_input_is_the_bf16_conv_on_rounded_x(case):
    c = case
    with nloop(1) as lib:
        f = Pw1(c, "randn")
        ops16 = dict(f.ops, x=O.bf16_round(f.ops["x"]), x2=None if f.ops["x2"] is None else O.bf16_round(f.ops["x2"]))
        g = Pw1(c._replace(form="bf16", ldx=2 * c.ldx, ldx2=2 * c.ldx2), "randn", ops=ops16)
        for out16 in (False, True):
            assert _same(f.launch(lib, out16)[0], g.launch(lib, out16)[0]), (c, out16, "_x32 != mi_conv1x1_pw on bf16(x)")
        assert f.intact() and g.intact()


@pytest.mark.parametrize("case", O.PW1_BATCHED_CASES, ids=repr)
def test_batched_launch_is_its_samples_with_their_own_weights(case):
    c = case
    S = c.M // c.hw
    with nloop(1) as lib:
        f = Pw1(c, "randn")
        for out16 in (False, True):
            y, = f.launch(lib, out16)
            y = y.view(S, c.hw, c.Nc)
            for s in sorted({0, 1, S // 2, S - 1}):
                one, = f.launch(lib, out16, sample=s)
                assert _same(one.view(S, c.hw, c.Nc)[s], y[s]), (c, out16, s)
        assert f.intact()


# ---------------------------------------------------------------------------------------------------- tap gather
class Gt:
    def __init__(self, c, kind, mode=1, one_tap=None):
        self.c, self.kind, self.mode = c, kind, mode
        ops = self.ops = O.gt_operands(c, kind, mode, one_tap)
        self.ref, self.absref, T = O.gt_reference(c, ops)
        self.T = T[None, :, :, None].to(F64)
        self.d = d = O.gt_desc(c, mode)
        dt = BF if mode == 1 else F32
        self.X = In(ops["x"], d.ldx, dt)
        self.Wt = In(O.wfq(ops["G"], mode == 0).reshape(1, -1), dtype=dt)
        self.B = In(ops["bias"].reshape(1, -1)) if ops["bias"] is not None else None
        self.R = In(ops["res"], d.ldr) if ops["res"] is not None else None
        self.rows = d.N * d.OH * d.OW

    def launch(self, lib, out16, dual=False):
        c, d = self.c, self.d
        y = Out(self.rows, c.Nc, d.ldy, BF if out16 else F32, init64=self.ops["prior"])
        b, r = (self.B.ptr if self.B else None), (self.R.ptr if self.R else None)
        if dual:
            y16 = Out(self.rows, c.Nc, c.Nc + c.ldy16, BF)
            rc = lib.mi_conv_gt_dual(_cd(d), self.X.ptr, self.Wt.ptr, b, r, y.ptr, y16.ptr, c.Nc + c.ldy16, _stream())
        else:
            rc = lib.mi_conv_gt(_cd(d), self.X.ptr, self.Wt.ptr, b, r, y.ptr, int(out16), _stream())
        assert rc == 0, (c, lib.mi_last_error())
        torch.cuda.synchronize()
        return (y.get(), y16.get()) if dual else (y.get(),)

    def intact(self):
        return all(b is None or b.intact() for b in (self.X, self.Wt, self.B, self.R))

    def check(self, tag, y):
        _check(tag, "gt" if self.mode else "gtf32", self.kind, y, self.ref, self.absref, self.T)


@pytest.mark.parametrize("mode", [1, 0], ids=["bf16mode", "fp32mode"])
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.GT_CASES, ids=repr)
def test_gather_cases(case, kind, mode):
    """The four shipped kinds on square and non-square grids, the generic forms gt_plan admits, odd and even half counts (the zero-padded last
    half), ragged channel tiles, one tile, M % 128 == 64, the 128-pixel tile, pitches, the eight epilogue forms for a strided and a
    parity-class layer (residual and prior content differ per produced pixel), the bf16 copy."""
    c = case
    lib = _lib()
    f = Gt(c, kind, mode)
    pl = O.gt_plan(f.d)
    pxt, ncls = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.mi_conv_gt_tile(_cd(f.d), ctypes.byref(pxt), ctypes.byref(ncls)) == 0 and (pxt.value, ncls.value) == (pl.pxt, pl.ncls)
    tag = f"gt:{c.name}:{kind}:mode{mode}"
    y32, = _twice(tag, lambda: f.launch(lib, False))
    f.check(tag, y32)
    if mode == 1:
        y16, = _twice(tag, lambda: f.launch(lib, True))
        f.check(tag, y16)
        assert _same(y16, y32.to(BF)), (tag, "bf16 output != fp32 output rounded once")
        if c.ldy16 >= 0 and "a" not in c.epi:
            yd, cp = _twice(tag, lambda: f.launch(lib, False, dual=True))
            assert _same(yd, y32), (tag, "mi_conv_gt_dual's y != mi_conv_gt's")
            assert _same(cp, yd.to(BF)), (tag, "bf16 copy != bf16(y)")
    assert f.intact(), (tag, "an input changed")


@pytest.mark.parametrize("out16", [False, True], ids=["f32", "bf16"])
def test_gather_k1_is_the_1x1_kernel(out16):
    """mi_conv_gt with k = 1, s = 1, p = 0 and mi_conv1x1_pw on the same buffers, integer operands: torch.equal."""
    lib = _lib()
    c = O.GT("k1_vs_pw1", 2, 8, 8, 256, 192, 1, 1, 0, 0, ldx=8, ldy=8, ldr=4, epi="br")
    f = Gt(c, "int")
    a, = f.launch(lib, out16)
    d = f.d
    d1 = O.desc1(d.N, d.OH, d.OW, d.K, d.Nc, ldx=d.ldx, ldy=d.ldy, ldr=d.ldr)
    y = Out(f.rows, c.Nc, d.ldy, BF if out16 else F32)
    assert lib.mi_conv1x1_pw(_cd(d1), f.X.ptr, None, f.Wt.ptr, f.B.ptr, f.R.ptr, y.ptr, int(out16), None, 0, _stream()) == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    assert torch.equal(a, y.get())
    f.check("gt:k1_vs_pw1", a)


_PROBES = [(O.GT("probe_down", 2, 8, 8, 64, 64, 3, 2, 1, 0, epi=""), (0, 1, 3, 4)), (O.GT("probe_dgrad", 2, 8, 8, 64, 64, 3, 2, 1, 1, epi=""), (0, 2, 6, 8, 4)),
           (O.GT("probe_up", 1, 8, 16, 64, 64, 4, 2, 1, 1, epi=""), (0, 3, 12, 15, 5)), (O.GT("probe_k3s1", 1, 8, 8, 64, 64, 3, 1, 1, 0, epi=""), (0, 2, 6, 8))]


@pytest.mark.parametrize("mode", [1, 0], ids=["bf16mode", "fp32mode"])
@pytest.mark.parametrize("case,taps", _PROBES, ids=lambda v: repr(v) if isinstance(v, O.GT) else "")
def test_gather_border_probe(case, taps, mode):
    """Weights that are non-zero on one tap only: exactly 0 wherever that tap falls outside the image (or, for a parity class, is not the
    class's tap), with integer and with randn operands."""
    lib = _lib()
    for tap in taps:
        for kind in ("int", "randn"):
            f = Gt(case, kind, mode, one_tap=tap)
            zero = f.absref.sum(-1) == 0                          # produced pixels the tap does not reach
            assert bool(zero.any()) or tap in (4, 5), (case, tap)
            assert bool((~zero).any())
            for out16 in ((False, True) if mode else (False,)):
                y, = f.launch(lib, out16)
                f.check(f"gt:{case.name}:tap{tap}", y)
                yv = y.to(F64).view(f.ref.shape)
                assert not bool(yv[zero].any()), (case, tap, kind, out16, "a tap outside the image contributed")


# ---------------------------------------------------------------------------------------------------- LayerNorm + 1x1
class Ln:
    def __init__(self, c, ops):
        self.c, self.ops = c, ops
        self.d = d = O.ln_desc(c)
        self.X = In(ops["x"], d.ldx, F32)
        self.Gm, self.Bt = In(ops["g"].reshape(1, -1)), In(ops["b"].reshape(1, -1))
        self.Wt = In(O.wfq(ops["G"][None]).reshape(1, -1), dtype=BF)
        self.B = In(ops["bias"].reshape(1, -1)) if ops["bias"] is not None else None

    def launch(self, lib, dual):
        c, d = self.c, self.d
        y = Out(c.M, c.Nc, d.ldy, BF)
        a = (_cd(d), self.X.ptr, self.Gm.ptr, self.Bt.ptr, self.ops["eps"], self.Wt.ptr, self.B.ptr if self.B else None, y.ptr)
        if dual:
            ln = Out(c.M, c.K, c.K + c.ldl, BF)
            rc = lib.mi_ln_conv1x1_pw_dual(*a, ln.ptr, c.K + c.ldl, _stream())
        else:
            rc = lib.mi_ln_conv1x1_pw(*a, _stream())
        assert rc == 0, (c, lib.mi_last_error())
        torch.cuda.synchronize()
        return (y.get(), ln.get()) if dual else (y.get(),)

    def both(self, lib, tag):
        """-> (y, ln_out as float64): dual and plain entry, each twice; the plain entry's y must be the dual's."""
        y, ln = _twice(tag, lambda: self.launch(lib, True))
        yp, = _twice(tag, lambda: self.launch(lib, False))
        assert _same(yp, y), (tag, "mi_ln_conv1x1_pw's y != mi_ln_conv1x1_pw_dual's")
        assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(ln.float()).all()), (tag, "non-finite")
        assert all(b is None or b.intact() for b in (self.X, self.Gm, self.Bt, self.Wt, self.B)), (tag, "an input changed")
        return y.to(F64), ln.to(F64)

    def check_conv(self, tag, y, ln, fam):
        """y against the conv of the kernel's own ln_out."""
        o = self.ops
        ref, ab = O.pw1_ref(ln, o["G"], bias=o["bias"]), O.pw1_ref(ln, o["G"], bias=o["bias"], absolute=True)
        el = (self.c.K + 2 + (o["bias"] is not None)) * U * ab
        el = el + 2.0 ** -8 * (ref.abs() + el)
        worst = float(((y - ref).abs() / el.clamp_min(1e-300)).max())
        _note(f"ln {fam} y element/bound", worst)
        assert worst <= 1.0, (tag, worst)


def _assert_pick(lib, c):
    d = O.ln_desc(c)
    assert lib.mi_ln_conv1x1_pw_supported(_cd(d)) == 1 and O.lnpw1_pick(d) is not None


@pytest.mark.parametrize("case", O.LN_CASES + O.LN_LOOP_CASES, ids=repr)
def test_layernorm_exact_family(case):
    c, lib = case, _lib()
    _assert_pick(lib, c)
    o = O.ln_operands(c, "exact")
    y, ln = Ln(c, o).both(lib, f"ln:{c.name}:exact")
    bad = (ln != o["ln"]).reshape(-1).nonzero().flatten()
    assert bad.numel() == 0, (c, f"ln_out: {bad.numel()} wrong elements, first at pixel {int(bad[0]) // c.K} channel {int(bad[0]) % c.K}")
    want = O.bf16_round(O.pw1_ref(o["ln"], o["G"], bias=o["bias"]))
    bad = (y != want).reshape(-1).nonzero().flatten()
    assert bad.numel() == 0, (c, f"y: {bad.numel()} wrong elements, first at pixel {int(bad[0]) // c.Nc} channel {int(bad[0]) % c.Nc}")


@pytest.mark.parametrize("params", ["plain", "wide"])
@pytest.mark.parametrize("case", O.LN_CASES + O.LN_LOOP_CASES[:1] + O.LN_LOOP_CASES[3:], ids=repr)
def test_layernorm_randn(case, params):
    c, lib = case, _lib()
    o = O.ln_operands(c, "randn", params)
    tag = f"ln:{c.name}:{params}"
    f = Ln(c, o)
    y, ln = f.both(lib, tag)
    share, worst = O.ln_model_check(ln, o["x"], o["g"], o["b"], o["eps"])
    _note(f"ln {params} share of ln_out off the bit model", share)
    _note(f"ln {params} differing element/allowed", worst)
    assert share <= O.LN_DIFFER_CAP and worst <= 1.0, (tag, share, worst)
    f.check_conv(tag, y, ln, params)
    e = O.rel(y, O.pw1_ref(O.ln64(o["x"], o["g"], o["b"], o["eps"])[0], o["G"], bias=o["bias"]))
    _note(f"ln {params} y rel-L2 vs float64", e)
    assert e <= 6e-3, (tag, e)


@pytest.mark.parametrize("case", O.LN_LOOP_CASES[1:3], ids=repr)
def test_layernorm_randn_loop_forms(case):
    test_layernorm_randn(case, "plain")


@pytest.mark.parametrize("case", [O.LN_CASES[0], O.LN_CASES[7], O.LN_CASES[5]], ids=repr)
def test_layernorm_large_mean(case):
    """x = 100 + 0.1 randn: the float32 mean alone flips a few per cent of the roundings, so the bit model does not apply; per element one bf16
    ulp plus the oracle's own change when the mean moves by 8 2^-24 |mean|."""
    c, lib = case, _lib()
    o = O.ln_operands(c, "offset")
    tag = f"ln:{c.name}:offset"
    f = Ln(c, o)
    y, ln = f.both(lib, tag)
    w = O.ln_offset_bound(ln, o["x"], o["g"], o["b"], o["eps"])
    share, _ = O.ln_model_check(ln, o["x"], o["g"], o["b"], o["eps"])
    _note("ln offset element/bound", w)
    _note("ln offset share of ln_out off the bit model", share)
    assert w <= 1.0, (tag, w)
    f.check_conv(tag, y, ln, "offset")


@pytest.mark.parametrize("case", [O.LN_CASES[1], O.LN_CASES[8]], ids=repr)
def test_layernorm_constant_pixels(case):
    c, lib = case, _lib()
    o = O.ln_operands(c, "const")
    f = Ln(c, o)
    y, ln = f.both(lib, f"ln:{c.name}:const")
    assert torch.equal(ln, O.bf16_round(o["b"]).expand(c.M, c.K)), c
    f.check_conv(f"ln:{c.name}:const", y, ln, "const")


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_everything_untouched():
    """Every reason of pw1_ok (three forms), gt_plan and lnpw1_ok and every MI_REQUIRE of the nine entry points: a non-zero return,
    mi_last_error set, y, the bf16 copy and the normalised tensor as they were, and the *_supported query in agreement with the oracle."""
    lib = _lib()
    big = 1 << 18
    x16, x32 = In(torch.zeros(big // 8, 8, dtype=F64), dtype=BF), In(torch.zeros(big // 8, 8, dtype=F64))
    w16, w32, f4 = In(torch.zeros(1, 1 << 16, dtype=F64), dtype=BF), In(torch.zeros(1, 1 << 16, dtype=F64)), In(torch.zeros(1, 1 << 12, dtype=F64))
    y, y16, ln = Out(1, big), Out(1, big, dtype=BF), Out(1, big, dtype=BF)
    n = [0]
    st = _stream()

    def refused(rc, what):
        n[0] += 1
        assert rc != 0, ("accepted", what)
        assert lib.mi_last_error(), what
        assert y.untouched() and y16.untouched() and ln.untouched(), ("written", what)

    # ---- 1x1, bf16 form
    ok = O.desc1(1, 8, 16, 128, 128)

    def pw(d, x=x16.ptr, x2=None, w=w16.ptr, res=None, yp=y.ptr, out16=0, c16=None, ld16=0, dp=True):
        return lib.mi_conv1x1_pw(_cd(d) if dp else None, x, x2, w, f4.ptr, res, yp, out16, c16, ld16, st)
    assert O.pw1_ok(ok) and lib.mi_conv1x1_pw_supported(_cd(ok)) == 1
    two = ok._replace(K=256, K1=128, ldx=128, ldx2=128)
    bad = [ok._replace(KH=3), ok._replace(KW=3), ok._replace(pad=1), ok._replace(stride=2), ok._replace(mode=0), ok._replace(IH=16), ok._replace(IW=8),
           ok._replace(K=192, K1=192, ldx=192), ok._replace(K1=64), ok._replace(K1=0), ok._replace(K1=256), ok._replace(Nc=96, ldy=96), ok._replace(ldx=132),
           two._replace(ldx2=132), ok._replace(OH=4, IH=4)]
    for d in bad:
        assert not O.pw1_ok(d) and lib.mi_conv1x1_pw_supported(_cd(d)) == 0, d
        refused(pw(d, x2=x16.ptr), ("pw1", d))
    assert O.pw1_ok(two) and lib.mi_conv1x1_pw_supported(_cd(two)) == 1
    for kw, what in [(dict(dp=False), "d"), (dict(x=None), "x"), (dict(w=None), "w"), (dict(yp=None), "y")]:
        refused(pw(ok, **kw), "pw1 null " + what)
    refused(pw(two), "two sources without x2")
    refused(pw(ok, x=x16.ptr + 8), "x 8 bytes off")
    refused(pw(two, x2=x16.ptr + 8), "x2 8 bytes off")
    refused(pw(ok, w=w16.ptr + 8), "w 8 bytes off")
    refused(pw(ok._replace(ldy=132)), "ldy % 8")
    refused(pw(ok._replace(ldr=130), res=f4.ptr), "ldr % 4")
    refused(pw(ok, c16=y16.ptr, ld16=132), "ldy16 % 8")
    refused(pw(ok, c16=y16.ptr, ld16=128, out16=1), "a bf16 copy of a bf16 output")
    refused(pw(ok._replace(accumulate=1), c16=y16.ptr, ld16=128), "a bf16 copy under accumulate")
    # ---- batched
    def pwb(d, wbatch):
        return lib.mi_conv1x1_pw_batched(_cd(d) if d else None, x16.ptr, w16.ptr, wbatch, None, None, y.ptr, 0, None, 0, st)
    refused(pwb(None, 128 * 128), "batched null d")
    refused(pwb(ok, 0), "wbatch 0")
    refused(pwb(ok, 128 * 128 + 4), "wbatch % 8")
    refused(pwb(O.desc1(4, 4, 8, 128, 128), 128 * 128), "hw % 64")
    refused(pwb(two, 256 * 128), "batched with two sources")
    # ---- 1x1, fp32 input
    def px(d, x=x32.ptr, x2=None, w=w16.ptr, res=None, yp=y.ptr, dp=True):
        return lib.mi_conv1x1_pw_x32(_cd(d) if dp else None, x, x2, w, None, res, yp, 0, st)
    for d in [ok._replace(ldx=130), two._replace(ldx2=130), ok._replace(mode=0), ok._replace(K1=64), ok._replace(Nc=32, ldy=32), ok._replace(pad=1)]:
        assert not O.pw1_ok(d, "x32") and lib.mi_conv1x1_pw_x32_supported(_cd(d)) == 0, d
        refused(px(d, x2=x32.ptr), ("x32", d))
    assert O.pw1_ok(ok._replace(ldx=132), "x32") and lib.mi_conv1x1_pw_x32_supported(_cd(ok._replace(ldx=132))) == 1
    for kw, what in [(dict(dp=False), "d"), (dict(x=None), "x"), (dict(w=None), "w"), (dict(yp=None), "y")]:
        refused(px(ok, **kw), "x32 null " + what)
    refused(px(two), "x32: two sources without x2")
    refused(px(ok, x=x32.ptr + 8), "x32: x 8 bytes off")
    refused(px(two, x2=x32.ptr + 8), "x32: x2 8 bytes off")
    refused(px(ok, w=w16.ptr + 8), "x32: w 8 bytes off")
    refused(px(ok._replace(ldy=132)), "x32: ldy % 8")
    refused(px(ok._replace(ldr=130), res=f4.ptr), "x32: ldr % 4")
    # ---- 1x1, exact fp32
    okf = O.desc1(1, 8, 16, 64, 64, mode=0)
    twof = okf._replace(K=128, K1=64, ldx=64, ldx2=64)

    def pf(d, x=x32.ptr, x2=None, w=w32.ptr, res=None, yp=y.ptr, dp=True):
        return lib.mi_conv1x1_pw_f32(_cd(d) if dp else None, x, x2, w, None, res, yp, st)
    assert O.pw1_ok(okf, "f32") and lib.mi_conv1x1_pw_f32_supported(_cd(okf)) == 1 and lib.mi_conv1x1_pw_f32_supported(_cd(twof)) == 1
    for d in [okf._replace(mode=1), okf._replace(K=96, K1=96, ldx=96), twof._replace(K1=32, ldx=32), okf._replace(ldx=66), twof._replace(ldx2=66),
              okf._replace(Nc=96, ldy=96), okf._replace(OH=4, IH=4), okf._replace(KH=3)]:
        assert not O.pw1_ok(d, "f32") and lib.mi_conv1x1_pw_f32_supported(_cd(d)) == 0, d
        refused(pf(d, x2=x32.ptr), ("f32", d))
    for kw, what in [(dict(dp=False), "d"), (dict(x=None), "x"), (dict(w=None), "w"), (dict(yp=None), "y")]:
        refused(pf(okf, **kw), "f32 null " + what)
    refused(pf(twof), "f32: two sources without x2")
    refused(pf(okf, x=x32.ptr + 8), "f32: x 8 bytes off")
    refused(pf(twof, x2=x32.ptr + 8), "f32: x2 8 bytes off")
    refused(pf(okf, w=w32.ptr + 8), "f32: w 8 bytes off")
    refused(pf(okf._replace(ldy=68)), "f32: ldy % 8")
    refused(pf(okf._replace(ldr=66), res=f4.ptr), "f32: ldr % 4")
    # ---- tap gather
    g = O.gt_desc(O.GT("ok", 2, 8, 8, 64, 64, 3, 2, 1, 0))
    gtr = O.gt_desc(O.GT("ok", 2, 8, 8, 64, 64, 4, 2, 1, 1))

    def gt(d, x=x16.ptr, w=w16.ptr, res=None, yp=y.ptr, out16=0, dp=True):
        return lib.mi_conv_gt(_cd(d) if dp else None, x, w, None, res, yp, out16, st)
    assert O.gt_plan(g) and O.gt_plan(gtr) and lib.mi_conv_gt_supported(_cd(g)) == 1 and lib.mi_conv_gt_supported(_cd(gtr)) == 1
    badg = [g._replace(mode=2), g._replace(K1=32), g._replace(K=96, K1=96, ldx=96), g._replace(Nc=96, ldy=96), g._replace(ldx=68), g._replace(mode=0, ldx=66),
            g._replace(KW=4), g._replace(KH=5, KW=5, pad=2), g._replace(KH=0, KW=0), g._replace(stride=3), g._replace(stride=0), g._replace(pad=-1),
            g._replace(pad=8, IH=1, IW=1), g._replace(OH=9), g._replace(OW=7), gtr._replace(OH=17), gtr._replace(OW=8),
            O.desc(8, 0, 0, 64, 64, IH=8, IW=6, OH=8, OW=6, KH=3, KW=3, stride=1, pad=1),              # GW = 6
            O.desc(8, 0, 0, 64, 64, IH=3, IW=8, OH=3, OW=8, KH=3, KW=3, stride=1, pad=1),              # GH GW = 24
            O.desc(1, 0, 0, 64, 64, IH=4, IW=4, OH=4, OW=4, KH=3, KW=3, stride=1, pad=1),              # 16 pixels
            O.desc(2, 0, 0, 64, 64, IH=8, IW=8, OH=16, OW=16, KH=1, KW=1, stride=2, pad=0, transposed=1),  # parity classes without a tap
            O.desc(2, 0, 0, 8192, 8192, IH=16, IW=16, OH=8, OW=8, KH=4, KW=4, stride=2, pad=1)]          # 2^31 bytes of weights
    for d in badg:
        assert O.gt_plan(d) is None and lib.mi_conv_gt_supported(_cd(d)) == 0, d
        refused(gt(d), ("gt", d))
    for kw, what in [(dict(dp=False), "d"), (dict(x=None), "x"), (dict(w=None), "w"), (dict(yp=None), "y")]:
        refused(gt(g, **kw), "gt null " + what)
    refused(gt(g, x=x16.ptr + 8), "gt: x 8 bytes off")
    refused(gt(g, w=w16.ptr + 8), "gt: w 8 bytes off")
    refused(gt(g._replace(ldy=68)), "gt: ldy % 8")
    refused(gt(g._replace(ldr=66), res=f4.ptr), "gt: ldr % 4")
    refused(gt(g._replace(mode=0), x=x32.ptr, w=w32.ptr, out16=1), "gt: out_bf16 in fp32 mode")

    def gd(d, c16=y16.ptr, ld16=64, dp=True):
        return lib.mi_conv_gt_dual(_cd(d) if dp else None, x16.ptr, w16.ptr, None, None, y.ptr, c16, ld16, st)
    refused(gd(g, dp=False), "gt_dual null d")
    refused(gd(g, c16=None), "gt_dual null copy")
    refused(gd(g, ld16=68), "gt_dual ldy16 % 8")
    refused(gd(g, c16=y16.ptr + 8), "gt_dual copy 8 bytes off")
    refused(gd(g._replace(accumulate=1)), "gt_dual under accumulate")
    refused(gd(g._replace(mode=0)), "gt_dual in fp32 mode")
    # ---- LayerNorm + 1x1
    lo = O.desc1(1, 8, 16, 128, 64)

    def lnf(d, x=x32.ptr, ga=f4.ptr, be=f4.ptr, w=w16.ptr, yp=y16.ptr, dp=True, dual=None):
        a = (_cd(d) if dp else None, x, ga, be, 1e-5, w, None, yp)
        return lib.mi_ln_conv1x1_pw_dual(*a, *dual, st) if dual else lib.mi_ln_conv1x1_pw(*a, st)
    assert O.lnpw1_ok(lo) and lib.mi_ln_conv1x1_pw_supported(_cd(lo)) == 1
    for d in [lo._replace(K=384, K1=384, ldx=384), lo._replace(K=64, K1=64, ldx=64), lo._replace(K=256, K1=128, ldx=256), lo._replace(Nc=96, ldy=96),
              lo._replace(ldx=130), lo._replace(ldy=68), lo._replace(accumulate=1), lo._replace(mode=0), lo._replace(OH=4, IH=4), lo._replace(KH=3),
              lo._replace(pad=1), lo._replace(stride=2), lo._replace(IW=8)]:
        assert not O.lnpw1_ok(d) and lib.mi_ln_conv1x1_pw_supported(_cd(d)) == 0, d
        refused(lnf(d), ("ln", d))
        refused(lnf(d, dual=(ln.ptr, 128)), ("ln dual", d))
    for kw, what in [(dict(dp=False), "d"), (dict(x=None), "x"), (dict(ga=None), "g"), (dict(be=None), "b"), (dict(w=None), "w"), (dict(yp=None), "y"),
                     (dict(x=x32.ptr + 8), "x off"), (dict(ga=f4.ptr + 8), "g off"), (dict(be=f4.ptr + 8), "b off"), (dict(w=w16.ptr + 8), "w off"),
                     (dict(yp=y16.ptr + 8), "y off")]:
        refused(lnf(lo, **kw), "ln " + what)
        refused(lnf(lo, dual=(ln.ptr, 128), **kw), "ln dual " + what)
    refused(lnf(lo, dual=(None, 128)), "ln dual: null normalised tensor")
    refused(lnf(lo, dual=(ln.ptr, 132)), "ln dual: ldl % 8")
    refused(lnf(lo, dual=(ln.ptr + 8, 128)), "ln dual: normalised tensor 8 bytes off")
    torch.cuda.synchronize()
    assert all(b.intact() for b in (x16, x32, w16, w32, f4)) and n[0] >= 150, n[0]
