"""conv3x3_halo_kernel's entry points (csrc/conv3x3_halo.hip) on the MI355X against tests/_halo_oracle.py, through the C ABI
(load_library(), ctypes, torch's current stream): every case of the oracle's lists (tests/test_halo_cpu.py holds them to the
instantiations and edges they reach), all four storage modes, forward and data gradient, integer-valued and randn operands.  After
every launch the library's tile query must name the plan the case is there for.

Buffers.  x, x2, residual, bias, the weights [tap][n][k], the coefficient tensor and gamma / beta / temb are views at their pitch inside
NaN-filled buffers: NaN in front, behind and in every row's padding (ldx = K1 + 8, ldx2 = K - K1 + 24, ldr = Nc + 4).  Outputs sit between
sentinels with sentinel padding inside every row (ldy = Nc + 8, ldy16 = Nc + 12); with accumulate they start from non-zero content.  The
GroupNorm sums start at zero between sentinels.  Every launch runs twice from the same start and every output must be bit-equal; inputs
must come back intact.

Integer operands (x in {-4..4}, w in {-3..3}, bias / residual / prior content small integers): 9 K 12 < 2^24, so every partial sum is
exact in fp32 under any order: fp32 y must be torch.equal to the float64 reference, bf16 y to the reference rounded to nearest even, bf16
accumulate follows widen, add in fp32, round once.  No tolerance.  A wrong zero at an image border, between the images of a multi-image
tile or at the seam of two row tiles is a wrong integer.  GroupNorm sums: x, w in {-1, 0, 1} at K = 64 plus a sparse residual of 300 (what a
bf16 output rounds) keep the per-workgroup fp32 reductions exact (the oracle asserts the condition), and the raw 64-bit words must equal
the sums of the STORED values times 2^20.

randn operands: the project's bounds rel-L2 <= 1e-5 (fp32 output) and <= 6e-3 (bf16 output) against float64 on the bf16-rounded operands;
per element |got - ref| <= (T + 2) 2^-24 sum |terms| with T = 9 K (K for 1x1; bias, residual and prior content count as terms), a bf16
output adding its rounding, 2^-8 of the value.

Fused entry points: per element |got - model| <= 4 f (sum |h| |w| + |bias|) against the rounding model h = bf16(mish(x scale + shift) + tb)
with f = 4.5e-4 the float32 emulation's figure (tests/test_halo_cpu.py), a bf16 output adding its own rounding; rel-L2 <= 5e-3 (fp32) /
6e-3 (bf16) against unrounded float64; the sums form against the coef form fed by mi_gn_coef_from_sums within the same bound.

Measured on the MI355X (worst over the cases; not used as bounds): 3x3 fp32 output rel-L2 1.9e-7, worst element 0.007 of its bound; 1x1
7.0e-8 and 0.05; bf16 outputs 1.7e-3 (their rounding; worst element 0.99 of the bound, the half ulp); the dual entry's y 9.1e-8; fused:
worst element 2.7e-4 of its scale (bound 1.8e-3), rel-L2 against float64 1.3e-3 / 2.1e-3, sums form against coef form 0.31 of the bound;
the file's 159 tests take 51 s, the slowest (k1_t256_qmap_nc384, 19.7 M outputs) 2 s.  The mutation check is in docs/kernels.md,
"conv3x3_halo.hip, tests"."""
import ctypes
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _halo_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -776.0                        # never-written sentinel (exact in bf16)
ISENT = -(1 << 40) - 12345           # ... of the 64-bit sums
PAD = 64                             # elements in front of and behind a view
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
U = 2.0 ** -24
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


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    T0[0] = time.time()
    yield
    print("\nworst measured: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())) + f"; the file took {time.time() - T0[0]:.1f} s")


def _tile(lib, d, io):
    bm, ck, sk = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.mi_conv3x3_bf16w_tile(_cd(d), io, ctypes.byref(bm), ctypes.byref(ck), ctypes.byref(sk))
    return None if rc else (bm.value, ck.value, sk.value)


def _fused_tile(lib, d):
    bm, ck = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.mi_conv3x3_gn_mish_tile(_cd(d), ctypes.byref(bm), ctypes.byref(ck))
    return None if rc else (bm.value, ck.value)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


class In:
    """Rows of t64 [..][C] at pitch ld inside a NaN-filled buffer: NaN in front, behind and in every row's padding."""

    def __init__(self, t64, ld=None, dtype=F32):
        t64 = t64.reshape(-1, t64.shape[-1])
        R, C = t64.shape
        ld = C if ld is None else ld
        assert ld >= C
        self.buf = torch.full((2 * PAD + R * ld,), NAN, dtype=dtype, device=DEV)
        rows = self.buf[PAD:PAD + R * ld].view(R, ld)
        rows[:, :C].copy_(t64.to(dtype))
        self.ptr = rows.data_ptr()
        assert self.ptr % 16 == 0
        self.snap = self.buf.clone()

    def intact(self):
        return _same(self.buf, self.snap)


class Out:
    """R rows of C results at pitch ld between PAD sentinels, sentinel padding inside every row; init64: what the rows hold before the
    launch (else sentinels)."""

    def __init__(self, R, C, ld=None, dtype=F32, init64=None):
        ld = C if ld is None else ld
        self.R, self.C, self.ld = R, C, ld
        self.buf = torch.full((2 * PAD + R * ld,), SENT, dtype=dtype, device=DEV)
        self.rows = self.buf[PAD:PAD + R * ld].view(R, ld)
        if init64 is not None:
            self.rows[:, :C].copy_(init64.reshape(R, C).to(dtype))
        self.ptr = self.rows.data_ptr()
        assert self.ptr % 16 == 0
        self.snap = self.buf.clone()

    def get(self):
        assert bool((self.buf[:PAD] == SENT).all()) and bool((self.buf[PAD + self.R * self.ld:] == SENT).all()), "written outside the result"
        assert bool((self.rows[:, self.C:] == SENT).all()), "written into a row's padding"
        return self.rows[:, :self.C].cpu()

    def untouched(self):
        return _same(self.buf, self.snap)


class Sums:
    """[N][Nc / 16][2] 64-bit fixed-point sums, zero, between sentinels (16-byte aligned)."""

    def __init__(self, N, Nc, init=None):
        self.n = N * (Nc // 16) * 2
        self.buf = torch.full((32 + self.n,), ISENT, dtype=torch.int64, device=DEV)
        self.buf[16:16 + self.n] = 0 if init is None else init.reshape(-1).to(DEV)
        self.ptr = self.buf[16:].data_ptr()
        assert self.ptr % 16 == 0
        self.shape = (N, Nc // 16, 2)
        self.snap = self.buf.clone()

    def get(self):
        assert bool((self.buf[:16] == ISENT).all()) and bool((self.buf[16 + self.n:] == ISENT).all()), "written outside the sums"
        return self.buf[16:16 + self.n].cpu().view(self.shape)

    def untouched(self):
        return _same(self.buf, self.snap)


def _check(tag, kind, got, ref, absref, T, what="y"):
    """got: the result (cpu, fp32 or bf16); ref: float64 reference; absref: the same sum over |terms|; T: summed terms per element."""
    out16 = got.dtype == BF
    got, ref = got.to(F64).reshape(-1), ref.reshape(-1)
    assert bool(torch.isfinite(got).all()), (tag, what, "non-finite")
    if kind in ("int", "unit"):
        want = O.stored(ref, out16)
        bad = (got != want).nonzero().flatten()
        assert bad.numel() == 0, (tag, what, f"{bad.numel()} wrong elements, first at {int(bad[0])}: {float(got[bad[0]])} != {float(want[bad[0]])}")
        return
    e = O.rel(got, ref)
    el = (T + 2) * U * absref.reshape(-1)
    bound = 1e-5
    if out16:
        el = el + 2.0 ** -8 * (ref.abs() + el)
        bound = 6e-3
    worst = float(((got - ref).abs() / el.clamp_min(1e-300)).max())
    fam = tag.split(":")[0] + (" bf16" if out16 else "")
    _note(f"{fam} {what} rel-L2", e)
    _note(f"{fam} {what} element/bound", worst)
    assert e <= bound and worst <= 1.0, (tag, what, e, worst)


def _twice(tag, launch):
    """launch() -> tuple of cpu tensors.  Two runs from the same start, bit-equal."""
    a, b2 = launch(), launch()
    for i, (x, y) in enumerate(zip(a, b2)):
        assert _same(x, y), (tag, f"output {i} differs between two runs")
    return a


# ---------------------------------------------------------------------------------------------------- the plain conv, 3x3 and 1x1
class Conv:
    """One operand set of a case at its pitches, x and x2 stored as fp32 and as bf16, with the convolution's float64 reference computed once
    for every storage mode and epilogue variant."""

    def __init__(self, c, kind, flip=False, ops=None):
        self.c, self.kind, self.flip = c, kind, flip
        self.ops = ops = ops or O.operands(c, kind, flip)
        self.base = O.base_reference(c, ops, flip)
        self.absbase = O.base_reference(c, ops, flip, absolute=True) if kind == "randn" else self.base
        d = O.case_desc(c, int(flip), "r")
        self.X = {dt: In(ops["x"], d.ldx, dt) for dt in (F32, BF)}
        self.X2 = {dt: In(ops["x2"], d.ldx2, dt) for dt in (F32, BF)} if ops["x2"] is not None else None
        self.Wt = In(O.halo_weights(ops["G"]).reshape(1, -1), dtype=BF)
        self.B = In(ops["bias"].reshape(1, -1))
        self.R = In(ops["res"], d.ldr)
        self.M = c.N * c.H * c.W
        self.taps = ops["G"].shape[0]

    def reference(self, epi):
        ref, ab = self.base, self.absbase
        for k, name in (("b", "bias"), ("r", "res"), ("a", "prior")):
            if k in epi:
                ref, ab = ref + self.ops[name], ab + self.ops[name].abs()
        return ref, ab

    def launch(self, lib, io, epi, entry="io", ldy16=None):
        c = self.c
        d = O.case_desc(c, int(self.flip), epi)
        y = Out(self.M, c.Nc, d.ldy, BF if io & 2 else F32, init64=self.ops["prior"] if "a" in epi else None)
        xdt = BF if io & 1 else F32
        a = (_cd(d), self.X[xdt].ptr, self.X2[xdt].ptr if self.X2 else None, self.Wt.ptr, self.B.ptr if "b" in epi else None,
             self.R.ptr if "r" in epi else None, y.ptr)
        extra = ()
        if entry == "plain":
            assert io == 0
            rc = lib.mi_conv3x3_bf16w(*a, _stream())
        elif entry == "gnsums":
            gs = Sums(c.N, c.Nc)
            rc = lib.mi_conv3x3_bf16w_io_gnsums(*a, io, gs.ptr, _stream())
            extra = (gs,)
        elif entry == "dual":
            y16 = Out(self.M, c.Nc, ldy16, BF)
            rc = lib.mi_conv3x3_bf16w_io_dual(*a, y16.ptr, ldy16, io, _stream())
            extra = (y16,)
        else:
            rc = lib.mi_conv3x3_bf16w_io(*a, io, _stream())
        assert rc == 0, (c, io, epi, entry, lib.mi_last_error())
        torch.cuda.synchronize()
        f = O.launch_facts(d)
        assert _tile(lib, d, io) == O.q_tile(d) == (f.BM, f.CK, 0) and O.plan_name(f) == c.plan, (c, _tile(lib, d, io))
        return (y.get(),) + tuple(e.get() for e in extra)

    def intact(self):
        bufs = list(self.X.values()) + (list(self.X2.values()) if self.X2 else []) + [self.Wt, self.B, self.R]
        return all(b.intact() for b in bufs)

    def check(self, tag, y, epi):
        ref, ab = self.reference(epi)
        _check(tag, self.kind, y, ref, ab, self.taps * self.c.K + len(epi))


# storage mode (bit 0: x and x2 are bf16, bit 1: y is bf16) with an epilogue form: b bias, r residual at ldr > Nc, a accumulate
VARIANTS = [(0, "br"), (1, "a"), (2, "ba"), (3, "r"), (1, "bra"), (3, "b")]


def _plain_params():
    out = []
    for c in O.CASES_3X3 + O.CASES_1X1:
        for kind in ("int", "randn"):
            for flip in (False, True):
                out.append(pytest.param(c, kind, flip, id=f"{c.name}-{kind}-{'dgrad' if flip else 'fwd'}"))
    return out


@pytest.mark.parametrize("case,kind,flip", _plain_params())
def test_conv_every_plan_storage_and_epilogue(case, kind, flip):
    """Every case of the 3x3 and 1x1 lists: the four storage modes, each with another epilogue form, at ldx != ldx2 and ldy, ldr > Nc; the
    fp32 entry point (mi_conv3x3_bf16w) without an epilogue.  flip: transposed = 1 over weights that differ per tap."""
    c = case
    lib = _lib()
    f = Conv(c, kind, flip)
    tag = f"{'conv1x1' if f.taps == 1 else 'conv3x3'}:{c.name}:{'dgrad' if flip else 'fwd'}"
    for io, epi in VARIANTS:
        y, = _twice(tag, lambda: f.launch(lib, io, epi))
        f.check(f"{tag}:io{io}:{epi}", y, epi)
    y0, = _twice(tag, lambda: f.launch(lib, 0, "", "plain"))
    f.check(tag + ":plain", y0, "")
    y1, = f.launch(lib, 1, "")
    assert _same(y0, y1), (tag, "bf16-stored x gives another result than the same values stored as fp32")
    assert f.intact(), (tag, "an input changed")


@pytest.mark.parametrize("tap", (1, 3, 5, 7))
@pytest.mark.parametrize("case", [c for c in O.CASES_3X3 if c.name in ("ti4_two_tiles_nc36", "w8_3chunks_nc132", "w16_nonsquare_1chunk", "w64_h4_xmap")], ids=repr)
def test_borders_and_seams(case, tap):
    """Positive x, positive weights on ONE border tap (ky 3 + kx: 1 top, 3 left, 5 right, 7 bottom): the image row / column that tap reaches
    past must be exactly 0 in every image -- also between the images of a multi-image tile, where the neighbour's row lies next to it in
    LDS -- and every other element positive and exact: at the seam of two row tiles it is the neighbour tile's data."""
    c = case
    lib = _lib()
    ops = O.operands(c, "int")
    ops["x"] = ops["x"].abs() + 1
    if ops["x2"] is not None:
        ops["x2"] = ops["x2"].abs() + 1
    G = torch.zeros_like(ops["G"])
    G[tap] = ops["G"][tap].abs() + 1
    ops["G"] = G
    f = Conv(c, "int", ops=ops)
    for io in (0, 3):
        y, = f.launch(lib, io, "")
        f.check(f"borders:{c.name}:{tap}", y, "")
        y = y.to(F64).view(c.N, c.H, c.W, c.Nc)
        edge = {1: y[:, 0], 7: y[:, -1], 3: y[:, :, 0], 5: y[:, :, -1]}[tap]
        inner = {1: y[:, 1:], 7: y[:, :-1], 3: y[:, :, 1:], 5: y[:, :, :-1]}[tap]
        assert not bool(edge.any()), (c, tap, "a padding pixel contributed")
        assert bool((inner > 0).all()), (c, tap, "a pixel inside the image was taken for padding")


# ---------------------------------------------------------------------------------------------------- dual output
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", [c for c in O.CASES_3X3 + O.CASES_1X1 if c.name in ("w8_3chunks_nc132", "ti4_two_tiles_nc36", "wide64_xmap", "t256",
                                                                                    "k1_m105_3stages_two", "k1_t256")], ids=repr)
def test_dual_output_is_y_rounded_once(case, kind):
    """mi_conv3x3_bf16w_io_dual: y is what mi_conv3x3_bf16w_io writes, bit for bit, and the copy at ldy16 > Nc is that y -- bias and
    residual included -- rounded once to bf16, bit for bit."""
    c = case
    lib = _lib()
    f = Conv(c, kind)
    for io in (0, 1):
        tag = f"dual:{c.name}:io{io}"
        y, y16 = _twice(tag, lambda: f.launch(lib, io, "br", "dual", c.Nc + O.LD["y16"]))
        f.check(tag, y, "br")
        assert _same(y, f.launch(lib, io, "br")[0]), (tag, "the dual entry's y != the plain entry's")
        assert y16.dtype == BF and _same(y16, y.to(BF)), (tag, "the bf16 copy is not y rounded once")
    assert f.intact()


# ---------------------------------------------------------------------------------------------------- GroupNorm sums from the epilogue
@pytest.mark.parametrize("case", O.CASES_SUMS, ids=repr)
def test_groupnorm_sums_epilogue_exact(case):
    """The per-workgroup path (TI = 1; four and eight waves, N64) and the per-32-pixel-block path (TI > 1): the raw 64-bit words are the sums of
    the stored values -- of the ROUNDED values under a bf16 y -- times 2^20, exactly."""
    c = case
    lib = _lib()
    f = Conv(c, "unit", ops=O.sums_operands(c, True))
    fa = O.launch_facts(O.case_desc(c))
    for io in range(4):
        tag = f"sums:{c.name}:io{io}"
        ref, _ = f.reference("br")
        st = O.stored(ref, bool(io & 2))
        assert O.unit_sums_exact(st, fa.BM, c.H, c.W)
        y, gs = _twice(tag, lambda: f.launch(lib, io, "br", "gnsums"))
        f.check(tag, y, "br")
        assert _same(y, f.launch(lib, io, "br")[0]), (tag, "the sums entry's y != the plain entry's")
        want = O.gn_sums(st)
        assert torch.equal(gs, want), (tag, "sums", int((gs != want).sum()))
        if io & 2:
            assert not torch.equal(want, O.gn_sums(ref)), (tag, "the case does not tell rounded from unrounded sums")
    assert f.intact()


@pytest.mark.parametrize("io", [0, 3])
def test_groupnorm_sums_poisoned_by_inf(io):
    """One Inf in x: every slot of that sample -- all its slabs see the Inf through some tap -- reads as poisoned (|slot| >= 2^60), every
    other sample's sums are exact, and y is exact wherever the Inf does not reach."""
    c = O.CASES_SUMS[0]
    lib = _lib()
    ops = O.sums_operands(c, True)
    clean = Conv(c, "unit", ops=dict(ops))
    ref, _ = clean.reference("br")
    ops["x"] = ops["x"].clone()
    ops["x"][1, 5, 7, 3] = float("inf")
    f = Conv(c, "unit", ops=ops)
    f.base = f.absbase = clean.base
    y, gs = f.launch(lib, io, "br", "gnsums")
    st = O.stored(ref, bool(io & 2)).view(c.N, c.H, c.W, c.Nc)
    want = O.gn_sums(st)
    yv = y.to(F64).view(c.N, c.H, c.W, c.Nc)
    reach = torch.zeros(c.N, c.H, c.W, dtype=torch.bool)
    reach[1, 4:7, 6:9] = True
    assert not bool(torch.isfinite(yv[reach]).any()) and torch.equal(yv[~reach], st[~reach])
    assert bool((gs[1].abs() >= 1 << 60).all()), "a slot of the sample with the Inf is not poisoned"
    keep = [n for n in range(c.N) if n != 1]
    assert torch.equal(gs[keep], want[keep])


# ---------------------------------------------------------------------------------------------------- fused GroupNorm + Mish
class Fused:
    def __init__(self, c, x_f32, border_tap=None):
        self.c, self.x_f32 = c, x_f32
        o = self.ops = O.fused_operands(c, x_f32, border_tap)
        K = c.K
        self.d = O.fused_desc(c)
        self.X = In(o["x"], self.d.ldx, F32 if x_f32 else BF)
        self.Wt = In(O.halo_weights(o["G"]).reshape(1, -1), dtype=BF)
        self.B = In(o["bias"].reshape(1, -1)) if o["bias"] is not None else None
        self.coef = In(torch.stack([o["sc"], o["sh"], o["tb"]]).reshape(3 * c.N, K))
        self.Ga, self.Be = In(o["gamma"].reshape(1, -1)), In(o["beta"].reshape(1, -1))
        self.ldt = K + max(c.ldt, 0)
        self.Te = In(o["temb"], self.ldt) if o["temb"] is not None else None
        self.S = Sums(c.N, K, init=o["sums"])
        hm = O.fused_h(o["x"], o["sc"], o["sh"], o["tb"])
        self.model = O.conv_ref(hm, o["G"], bias=o["bias"])
        self.scale = O.conv_ref(hm, o["G"], bias=o["bias"], absolute=True)
        self.ref64 = O.fused_reference64(o, c)
        self.M = c.N * c.H * c.W

    def launch(self, lib, form, coef_ptr=None):
        c, io = self.c, 0 if self.x_f32 else 3
        y = Out(self.M, c.Nc, self.d.ldy, BF if io else F32)
        bp = self.B.ptr if self.B else None
        if form == "coef":
            rc = lib.mi_conv3x3_gn_mish(_cd(self.d), self.X.ptr, coef_ptr or self.coef.ptr, self.Wt.ptr, bp, y.ptr, io, _stream())
        else:
            rc = lib.mi_conv3x3_gn_mish_sums(_cd(self.d), self.X.ptr, self.S.ptr, self.Ga.ptr, self.Be.ptr, self.Te.ptr if self.Te else None,
                                             self.ldt if self.Te else 0, c.G, O.GN_EPS, self.Wt.ptr, bp, y.ptr, io, _stream())
        assert rc == 0, (c, lib.mi_last_error())
        torch.cuda.synchronize()
        fa = O.launch_facts(self.d, True)
        assert _fused_tile(lib, self.d) == (fa.BM, fa.CK) and O.plan_name(fa) == c.plan, (c, _fused_tile(lib, self.d))
        return (y.get(),)

    def library_coef(self, lib):
        c = self.c
        coef = torch.full((3 * c.N * c.K + 2 * PAD,), NAN, device=DEV)
        rc = lib.mi_gn_coef_from_sums(c.N, c.K, c.G, c.H * c.W, O.GN_EPS, self.S.ptr, self.Ga.ptr, self.Be.ptr, self.Te.ptr if self.Te else None,
                                      self.ldt if self.Te else 0, None, coef[PAD:].data_ptr(), _stream())
        assert rc == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        return coef

    def bound(self, out16):
        b = 4 * O.FUSED_EMUL_FIGURE * self.scale
        return b + 2.0 ** -8 * (self.model.abs() + b) if out16 else b

    def check(self, tag, y):
        out16 = y.dtype == BF
        got = y.to(F64).view_as(self.model)
        assert bool(torch.isfinite(got).all()), (tag, "non-finite")
        worst = float(((got - self.model).abs() / self.bound(out16).clamp_min(1e-300)).max())
        fig = float(((got - self.model).abs() / self.scale.clamp_min(1e-300)).max())
        e = O.rel(got, self.ref64)
        if not out16:
            _note("fused element/scale", fig)
        _note("fused rel-L2 vs float64" + (" bf16" if out16 else ""), e)
        assert worst <= 1.0 and e <= (6e-3 if out16 else 5e-3), (tag, worst, fig, e)

    def intact(self):
        return all(b is None or b.intact() for b in (self.X, self.Wt, self.B, self.coef, self.Ga, self.Be, self.Te)) and self.S.untouched()


@pytest.mark.parametrize("x_f32", [False, True], ids=["io3", "io0"])
@pytest.mark.parametrize("case", O.FUSED_CASES, ids=repr)
def test_fused_groupnorm_mish_entries(case, x_f32):
    c = case
    lib = _lib()
    f = Fused(c, x_f32)
    tag = f"fused:{c.name}:{'io0' if x_f32 else 'io3'}"
    yc, = _twice(tag + ":coef", lambda: f.launch(lib, "coef"))
    ys, = _twice(tag + ":sums", lambda: f.launch(lib, "sums"))
    f.check(tag + ":coef", yc)
    f.check(tag + ":sums", ys)
    lc = f.library_coef(lib)
    yl, = f.launch(lib, "coef", lc[PAD:].data_ptr())
    f.check(tag + ":library coef", yl)
    diff = (ys.to(F64) - yl.to(F64)).abs().view_as(f.model) / f.bound(not x_f32).clamp_min(1e-300)
    _note("fused sums form vs coef form, of the bound", float(diff.max()))
    assert float(diff.max()) <= 1.0, (tag, "_gn_mish_sums against _gn_mish fed by mi_gn_coef_from_sums", float(diff.max()))
    assert f.intact()


@pytest.mark.parametrize("tap", (1, 3, 5, 7))
@pytest.mark.parametrize("case", O.FUSED_CASES[:3], ids=repr)
def test_fused_padding_is_zero_after_the_transform(case, tap):
    """Integer weights on one border tap only, non-zero shift and time bias: every output of the border row / column that tap reaches past must
    be exactly 0 -- a padding pixel transformed to mish(shift) + tb instead of left zero shows in all of them."""
    c = case
    lib = _lib()
    for x_f32 in (False, True):
        f = Fused(c, x_f32, border_tap=tap)
        for form in ("coef", "sums"):
            y, = f.launch(lib, form)
            y = y.to(F64).view(c.N, c.H, c.W, c.Nc)
            assert bool(torch.isfinite(y).all())
            edge = {1: y[:, 0], 7: y[:, -1], 3: y[:, :, 0], 5: y[:, :, -1]}[tap]
            assert not bool(edge.any()), (c, tap, form, "a padding pixel contributed")
            assert bool(y.any())
            e = O.rel(y, f.ref64)
            assert e <= (5e-3 if x_f32 else 6e-3), (c, tap, form, e)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched():
    """A handful of the host-side refusals with real buffers (tests/test_halo_cpu.py matches every one by its message): the non-zero return
    first -- nothing may have been launched -- then y, the bf16 copy and the sums exactly as they were."""
    lib = _lib()
    c = O.CASES_3X3[4]
    f = Conv(c, "int")
    ok = O.case_desc(c, 0, "r")
    y, y16, gs = Out(f.M, c.Nc, ok.ldy), Out(f.M, c.Nc, c.Nc + 12, BF), Sums(c.N, c.Nc)
    n = [0]

    def refused(rc, what):
        n[0] += 1
        assert rc != 0, ("accepted", what)
        assert lib.mi_last_error(), what
        torch.cuda.synchronize()
        assert y.untouched() and y16.untouched() and gs.untouched(), ("written", what)

    X, Wp, B, R = f.X[F32].ptr, f.Wt.ptr, f.B.ptr, f.R.ptr

    def io(d=ok, x=X, w=Wp, bias=B, res=R, yp=y.ptr, mode=0):
        return lib.mi_conv3x3_bf16w_io(_cd(d), x, None, w, bias, res, yp, mode, _stream())

    assert O.dispatch_accepts(ok, has_res=True) is None
    refused(io(ok._replace(ldy=ok.ldy + 2)), "ldy % 4")
    refused(io(ok._replace(ldr=ok.ldr + 2)), "ldr % 4")
    refused(io(yp=y.ptr + 8), "fp32 y 8 bytes off")
    refused(io(yp=y.ptr + 4, mode=2), "bf16 y 4 bytes off")
    refused(io(bias=B + 4), "bias 4 bytes off")
    refused(io(res=R + 8), "residual 8 bytes off")
    refused(io(x=X + 8), "x 8 bytes off")
    refused(io(ok._replace(ldx=ok.ldx + 2)), "ldx % 4")
    refused(io(mode=4), "io 4")
    refused(io(ok._replace(K1=32)), "two sources without x2")
    refused(io(ok._replace(OW=28, IW=28)), "W = 28")
    refused(lib.mi_conv3x3_bf16w_io_gnsums(_cd(ok), X, None, Wp, B, R, y.ptr, 0, gs.ptr + 4, _stream()), "sums 4 bytes off")
    refused(lib.mi_conv3x3_bf16w_io_dual(_cd(ok), X, None, Wp, B, R, y.ptr, y16.ptr, c.Nc + 14, 0, _stream()), "ldy16 % 4")
    refused(lib.mi_conv3x3_bf16w_io_dual(_cd(ok), X, None, Wp, B, R, y.ptr, y16.ptr, c.Nc + 12, 2, _stream()), "dual with a bf16 y")
    fd = ok._replace(ldr=0)
    refused(lib.mi_conv3x3_gn_mish(_cd(fd._replace(ldy=fd.ldy + 2)), X, B, Wp, B, y.ptr, 0, _stream()), "fused ldy % 4")
    refused(lib.mi_conv3x3_gn_mish(_cd(fd), X, B, Wp, B + 8, y.ptr, 0, _stream()), "fused bias 8 bytes off")
    refused(lib.mi_conv3x3_gn_mish(_cd(fd), X, B, Wp, B, y.ptr + 8, 0, _stream()), "fused y 8 bytes off")
    refused(lib.mi_conv3x3_gn_mish(_cd(fd._replace(transposed=1)), X, B, Wp, B, y.ptr, 0, _stream()), "fused transposed")
    refused(lib.mi_conv3x3_gn_mish(_cd(fd), X, B, Wp, B, y.ptr, 1, _stream()), "fused io 1")
    assert f.intact() and n[0] >= 19
