"""conv_pw_kernel's 3x3 entry points (csrc/conv_pw.hip) on the MI355X against tests/_conv_pw_oracle.py, through the C ABI (load_library(),
ctypes, torch's current stream): every case of the oracle's lists (tests/test_conv_pw_cpu.py holds them to the instantiations and edges
they reach), forward and data gradient, fp32 and bf16 output, with integer-valued and with randn operands.

Buffers.  x, x2, residual, the coefficient tensor, gamma / beta / temb and the fragment-order weights are views at their pitch inside
NaN-filled buffers: NaN in front, behind and in every row's padding (fp32 views for the fp32-input and exact-fp32 forms).  Outputs sit
between sentinels with sentinel padding inside every row; with accumulate they start from non-zero content.  The GroupNorm sums start at
zero between sentinels.  Every launch runs twice from the same start and every output, the sums included, must be bit-equal; inputs must
come back intact.  Split launches run on a workspace the test registers: 256-byte aligned, 64 KB of zero flags, the partial tiles NaN,
sentinels behind exactly the bytes the restated pw_split needs -- afterwards the flags are zero again and the sentinels intact.

Integer operands (x in {-4..4}, w in {-3..3}, bias / residual / prior content small integers): 9 K 12 < 2^24 for K <= 1024, so every
partial sum is exact in fp32 under any order, split-K and the per-tile rotation of the chunk order included: fp32 y must be torch.equal to
the float64 reference, bf16 y to the reference rounded to nearest even, bf16 accumulate follows widen, add in fp32, round.  No tolerance.
GroupNorm sums: with x, w in {-1, 0, 1} at K = 64 the per-workgroup fp32 reductions are exact as well (the oracle asserts the condition),
and the raw 64-bit words must equal the reference times 2^20.

randn operands: the project's bounds (tests/test_kernels_gpu.py) rel-L2 <= 1e-5 for an fp32 output, <= 6e-3 for a bf16 output, <= 3e-6
for the exact-fp32 form; and per element |got - ref| <= (T + 2) 2^-24 sum |terms| with T = 9 K (bias, residual and prior content count as
terms) -- a bf16 output adds its rounding, 2^-8 of the value.  Bit for bit: a bf16 output is the fp32 instantiation's output rounded once
(the tile16 path adds the bias before the same single rounding: no combination is exempt); _pw_x32 is _pw on bf16(x); _pw_gnsums' y is
_pw's y; _gn_mish_sums is _gn_mish fed by mi_gn_coef_from_sums; a split launch repeats itself.

Fused variants: per element |got - model| <= 4 f (sum |h| |w| + |bias|) against the rounding model h = bf16(mish(x scale + shift) + tb)
with f = 3.5e-5 the float32 emulation's figure (tests/test_conv_pw_cpu.py), a bf16 output adding its own rounding; and rel-L2 <= 5e-3 (fp32
output) / 6e-3 (bf16 output) against unrounded float64.

Measured on the MI355X (worst over the cases; not used as bounds): fp32 output rel-L2 4.0e-7, worst element 0.004 of its bound; bf16
outputs 1.7e-3 (their rounding; worst element 0.97 of the bound, the half ulp); exact-fp32 form 4.4e-7; randn sums 0.004 of their bound;
split against unsplit 3.4e-7; fused: worst element 7.6e-6 of its scale with ordinary parameters, 1.1e-5 with wide ones, 1.9e-5 under
split-K (bound 1.4e-4), rel-L2 against float64 1.8e-3 / 2.5e-3; the file's 199 tests take 4.9 s.

What the product library cannot reach: pw_geom's "TH not a power of two", "N % TI" and its pw_xp comparison cannot fail on their own (see
docs/kernels.md, "conv_pw.hip (3x3), tests")."""
import ctypes
import os
import sys
from contextlib import contextmanager

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_pw_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -776.0                        # never-written sentinel (exact in bf16)
ISENT = -(1 << 40) - 12345           # ... of the 64-bit sums
PAD = 64                             # elements in front of and behind a view
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
U = 2.0 ** -24
WORST = {}


def _lib():
    from src.ops.lib import load_library
    return load_library()


def _K():
    from src.ops import functional
    return functional


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cd(d):
    from src.ops.lib import MiConvDesc
    return ctypes.byref(MiConvDesc(**d._asdict()))


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst measured: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


@contextmanager
def knobs(pt=0, sk=0):
    """Force the pixel tile and the split mode (0: no split launches, whatever workspace the product registered); restored on the way out."""
    lib, K = _lib(), _K()
    was = lib.mi_debug_conv_pw_splitk(sk)
    assert lib.mi_debug_conv_pw_tile(pt) == 0
    K._QUERY_CACHE.clear()
    try:
        yield lib
    finally:
        lib.mi_debug_conv_pw_tile(0)
        lib.mi_debug_conv_pw_splitk(was)
        K._QUERY_CACHE.clear()


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


def _check(tag, kind, got, ref, absref, T, bound, what="y"):
    """got: the result (cpu, fp32 or bf16); ref: float64 reference; absref: the same sum over |terms|; T: summed terms per element."""
    out16 = got.dtype == BF
    got, ref, absref = got.to(F64).reshape(-1), ref.reshape(-1), absref.reshape(-1)
    assert bool(torch.isfinite(got).all()), (tag, what, "non-finite")
    if kind in ("int", "unit"):
        want = O.stored(ref, out16)
        bad = (got != want).nonzero().flatten()
        assert bad.numel() == 0, (tag, what, f"{bad.numel()} wrong elements, first at {int(bad[0])}: {float(got[bad[0]])} != {float(want[bad[0]])}")
        return
    e = O.rel(got, ref)
    el = (T + 2) * U * absref
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


# ---------------------------------------------------------------------------------------------------- the plain conv and its forms
class Conv:
    """One operand set of a Plain case at its pitches, launched through mi_conv3x3_pw / _gnsums / _x32 / _f32.  form: 'bf16' (bf16 x and
    weights), 'x32' (fp32 x, rounded once while staged; bf16 weights), 'f32' (exact fp32)."""

    def __init__(self, c, kind, flip=False, form="bf16", ops=None):
        self.c, self.kind, self.flip, self.form = c, kind, flip, form
        ops = ops or O.plain_operands(c, kind, flip, stored_f32=form != "bf16")
        if form == "x32":
            ops = dict(ops, G=O.bf16_round(ops["G"]))
        self.ops = ops
        self.ref, self.absref = O.plain_reference(ops, flip, round_x=form == "x32")
        self.d = O.plain_desc(c, int(flip), form == "x32", form == "f32")
        xdt, wdt = (BF if form == "bf16" else F32), (F32 if form == "f32" else BF)
        self.X = In(ops["x"], self.d.ldx, xdt)
        self.X2 = In(ops["x2"], self.d.ldx2, xdt) if ops["x2"] is not None else None
        self.Wt = In(O.frag_operand(ops["G"], flip, form == "f32").reshape(1, -1), dtype=wdt)
        self.B = In(ops["bias"].reshape(1, -1)) if ops["bias"] is not None else None
        self.R = In(ops["res"], self.d.ldr) if ops["res"] is not None else None
        self.M, self.T = O.case_pixels(c), O.term_count(c)

    def launch(self, lib, out16, entry=None, gsum=False):
        c, d = self.c, self.d
        y = Out(self.M, c.Nc, d.ldy, BF if out16 else F32, init64=self.ops["prior"])
        gs = Sums(c.N, c.Nc) if gsum else None
        a = (_cd(d), self.X.ptr, self.X2.ptr if self.X2 else None, self.Wt.ptr, self.B.ptr if self.B else None, self.R.ptr if self.R else None, y.ptr)
        entry = entry or {"bf16": "gnsums" if gsum else "pw", "x32": "x32", "f32": "f32"}[self.form]
        if entry == "pw":
            rc = lib.mi_conv3x3_pw(*a, int(out16), _stream())
        elif entry == "gnsums":
            rc = lib.mi_conv3x3_pw_gnsums(*a, int(out16), gs.ptr, _stream())
        elif entry == "x32":
            rc = lib.mi_conv3x3_pw_x32(*a, int(out16), gs.ptr if gs else None, _stream())
        else:
            rc = lib.mi_conv3x3_pw_f32(*a, _stream())
        assert rc == 0, (c, lib.mi_last_error())
        torch.cuda.synchronize()
        return (y.get(), gs.get()) if gsum else (y.get(),)

    def intact(self):
        return all(b is None or b.intact() for b in (self.X, self.X2, self.Wt, self.B, self.R))

    def check(self, tag, y, bound=1e-5):
        _check(tag, self.kind, y, self.ref, self.absref, self.T, bound)


def run_plain(c, kind, fam="plain"):
    with knobs(c.pt) as lib:
        for flip in (False, True):
            tag = f"{fam}:{c.name}:{'dgrad' if flip else 'fwd'}"
            f = Conv(c, kind, flip)
            assert lib.mi_conv3x3_pw_tile(_cd(f.d)) == O.q_tile(f.d, O.Knobs(c.pt, 0, 0)) != 0
            y32, = _twice(tag, lambda: f.launch(lib, False))
            y16, = _twice(tag, lambda: f.launch(lib, True))
            f.check(tag, y32)
            f.check(tag, y16)
            assert _same(y16, y32.to(BF)), (tag, "bf16 output != fp32 output rounded once")
            assert f.intact(), (tag, "an input changed")


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.GEOMETRY_CASES, ids=repr)
def test_tile_geometries(case, kind):
    """Every row of the geometry table (W 8 / 16 / 32 x tile 64 / 128 / 256, TI 1 and 2, one to six tiles per image, the forced 256-pixel
    tile at W = 8): a wrong, dropped or doubled tap at an image border, a band row or a tile seam is a wrong integer."""
    run_plain(case, kind, "geometry")


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.BATCH_CASES + O.CHANNEL_CASES, ids=repr)
def test_batches_and_channels(case, kind):
    run_plain(case, kind, "channels")


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.PITCH_CASES + O.EPILOGUE_CASES, ids=repr)
def test_pitches_and_epilogue_forms(case, kind):
    run_plain(case, kind, "epilogue")


@pytest.mark.parametrize("case", [c for c in O.BATCH_CASES if "xmap" in c.name], ids=repr)
def test_xmap_batch_equals_single_images(case):
    """N % 8 == 0 with several tiles per image remaps the workgroups (an image's row tiles on one XCD): bit-equal to the same images launched
    one at a time (one chunk: every tile walks the contraction in the same order)."""
    c = case
    assert c.K == 64
    with knobs(c.pt) as lib:
        f = Conv(c, "randn")
        assert O.launch_facts(f.d, 0, False, kn=O.Knobs(c.pt, 0, 0)).xmap
        y, = f.launch(lib, False)
        y = y.view(c.N, -1, c.Nc)
        for n in range(c.N):
            one = c._replace(N=1, name=c.name)
            ops = {k: (v[n:n + 1] if (v is not None and v.dim() == 4 and k != "G") else v) for k, v in f.ops.items()}
            g = Conv(one, "randn", ops=ops)
            assert not O.launch_facts(g.d, 0, False, kn=O.Knobs(c.pt, 0, 0)).xmap
            assert _same(g.launch(lib, False)[0], y[n]), (c, n)


# ---------------------------------------------------------------------------------------------------- GroupNorm sums from the epilogue
def _sums_check(tag, kind, c, y, gs, M_per_img):
    """gs against the stored y: exactly (integer operands), or within the fp32 reductions' error: (n + 2) 2^-24 of the sum over |terms| for
    the n = H W 16 values of a slab, plus half a unit of the 20 fraction bits per workgroup that adds."""
    yv = y.to(F64).view(c.N, M_per_img, c.Nc)
    want = O.gn_sums(yv.view(c.N, c.H, c.W, c.Nc))
    if kind == "unit":
        assert torch.equal(gs, want), (tag, "sums", int((gs != want).sum()))
        return
    n = M_per_img * 16
    v = yv.view(c.N, M_per_img, c.Nc // 16, 16)
    mag = torch.stack([v.abs().sum((1, 3)), (v * v).sum((1, 3))], -1)
    bound = (n + 2) * U * mag + (M_per_img // min(c.pt, M_per_img) + 1) * 2.0 ** -21
    worst = float(((gs.to(F64) - want.to(F64)).abs() / O.GSUM_SCALE / bound).max())
    _note("sums element/bound", worst)
    assert worst <= 1.0, (tag, worst)


@pytest.mark.parametrize("kind", ["unit", "randn"])
@pytest.mark.parametrize("case", O.GNS_CASES, ids=repr)
def test_groupnorm_sums_epilogue(case, kind):
    c = case
    with knobs(c.pt) as lib:
        f = Conv(c, kind)
        for out16 in (False, True):
            tag = f"sums:{c.name}:{'bf16' if out16 else 'f32'}"
            if kind == "unit":
                assert O.unit_sums_exact(O.stored(f.ref, out16), c.pt, c.H, c.W)
            y, gs = _twice(tag, lambda: f.launch(lib, out16, gsum=True))
            f.check(tag, y)
            assert _same(y, f.launch(lib, out16)[0]), (tag, "_pw_gnsums' y != _pw's y")
            _sums_check(tag, kind, c, y, gs, c.H * c.W)
        assert f.intact()


# ---------------------------------------------------------------------------------------------------- fp32 input, exact fp32
@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.X32_CASES, ids=repr)
def test_fp32_input_is_the_bf16_conv_on_rounded_x(case, kind):
    c = case
    with knobs(c.pt) as lib:
        for flip in (False, True):
            tag = f"x32:{c.name}:{'dgrad' if flip else 'fwd'}"
            f = Conv(c, kind, flip, "x32")
            assert lib.mi_conv3x3_pw_x32_tile(_cd(f.d)) == O.q_tile(f.d, O.Knobs(c.pt, 0, 0), in32=True) != 0
            ops16 = dict(f.ops, x=O.bf16_round(f.ops["x"]), x2=None if f.ops["x2"] is None else O.bf16_round(f.ops["x2"]))
            c16 = c._replace(ldx=2 * c.ldx, ldx2=2 * c.ldx2)              # (bf16 pitches in multiples of 8)
            g = Conv(c16, kind, flip, "bf16", ops=ops16)
            for out16 in (False, True):
                y, = _twice(tag, lambda: f.launch(lib, out16))
                f.check(tag, y)
                assert _same(y, g.launch(lib, out16, "pw")[0]), (tag, "_pw_x32 != _pw on bf16(x)")
                ys, gs = _twice(tag, lambda: f.launch(lib, out16, gsum=True))
                y2, gs2 = g.launch(lib, out16, "gnsums", gsum=True)
                assert _same(ys, y) and torch.equal(gs, gs2), (tag, "_pw_x32 with sums")
                _sums_check(tag, "randn", c, ys, gs, c.H * c.W)
            assert f.intact() and g.intact()


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.F32_CASES, ids=repr)
def test_exact_fp32_form(case, kind):
    c = case
    with knobs(c.pt) as lib:
        for flip in (False, True):
            tag = f"f32:{c.name}:{'dgrad' if flip else 'fwd'}"
            f = Conv(c, kind, flip, "f32")
            assert lib.mi_conv3x3_pw_f32_tile(_cd(f.d)) == O.q_tile(f.d, O.Knobs(c.pt, 0, 0), f32=True) != 0
            y, = _twice(tag, lambda: f.launch(lib, False))
            f.check(tag, y, 3e-6)
            assert f.intact()


# ---------------------------------------------------------------------------------------------------- fragment layouts of the pack kernels
@pytest.mark.parametrize("layout", ["wfq", "wdq", "wfq32", "wdq32"])
def test_pack_kernels_write_the_torch_layouts(layout):
    K = _K()
    ci, co = 192, 128
    Wm = O.randn((9, ci, co), 77)
    n = Wm.numel()
    flat = Wm.reshape(-1).to(F32).to(DEV)
    table, nent, tiles = K.pack_table([(0, 9, ci, co)], DEV)
    if layout.endswith("32"):
        dq, fq = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        K.pack_weights_f32frag(table, nent, tiles, flat, dq, fq)
        want = (O.wfq if layout == "wfq32" else O.wdq)(Wm, True).to(F32)
    else:
        wd, wf, dq, fq = (torch.zeros(n, device=DEV, dtype=BF) for _ in range(4))
        K.pack_weights_bf16(table, nent, tiles, flat, wd, wf, dq, fq)
        want = (O.wfq if layout == "wfq" else O.wdq)(O.bf16_round(Wm)).to(BF)
    torch.cuda.synchronize()
    got = (fq if layout.startswith("wfq") else dq).cpu()
    assert _same(got, want.reshape(-1)), layout


# ---------------------------------------------------------------------------------------------------- fused GroupNorm + Mish
class Fused:
    def __init__(self, c, x_f32, border_tap=None):
        self.c, self.x_f32 = c, x_f32
        o = self.ops = O.fused_operands(c, border_tap, x_f32)
        K = c.K
        self.ldx = K + (4 if x_f32 else 8) * (c.ldt > 0)
        self.d = O.desc(c.N, c.H, c.W, K, c.Nc, ldx=self.ldx, ldy=c.Nc + 8)
        self.X = In(o["x"], self.ldx, F32 if x_f32 else BF)
        self.Wt = In(O.wfq(o["G"]).reshape(1, -1), dtype=BF)
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
        self.M = O.case_pixels(c)

    def launch(self, lib, out16, var, coef_ptr=None):
        c = self.c
        y = Out(self.M, c.Nc, self.d.ldy, BF if out16 else F32)
        bp = self.B.ptr if self.B else None
        if var == 2:
            fn = lib.mi_conv3x3_pw_x32_gn_mish if self.x_f32 else lib.mi_conv3x3_pw_gn_mish
            rc = fn(_cd(self.d), self.X.ptr, coef_ptr or self.coef.ptr, self.Wt.ptr, bp, y.ptr, int(out16), _stream())
        else:
            fn = lib.mi_conv3x3_pw_x32_gn_mish_sums if self.x_f32 else lib.mi_conv3x3_pw_gn_mish_sums
            rc = fn(_cd(self.d), self.X.ptr, self.S.ptr, self.Ga.ptr, self.Be.ptr, self.Te.ptr if self.Te else None, self.ldt if self.Te else 0, c.G, O.GN_EPS,
                    self.Wt.ptr, bp, y.ptr, int(out16), _stream())
        assert rc == 0, (c, lib.mi_last_error())
        torch.cuda.synchronize()
        return (y.get(),)

    def library_coef(self, lib):
        c = self.c
        coef = torch.full((3 * c.N * c.K + 2 * PAD,), NAN, device=DEV)
        rc = lib.mi_gn_coef_from_sums(c.N, c.K, c.G, c.H * c.W, O.GN_EPS, self.S.ptr, self.Ga.ptr, self.Be.ptr, self.Te.ptr if self.Te else None,
                                      self.ldt if self.Te else 0, None, coef[PAD:].data_ptr(), _stream())
        assert rc == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        return coef

    def check(self, tag, y, rel=None):
        """rel: the share of sum |h| |w| + |bias| an element may be off the model (default: four times the emulation's figure)."""
        out16 = y.dtype == BF
        got = y.to(F64).view_as(self.model)
        assert bool(torch.isfinite(got).all()), (tag, "non-finite")
        bound = (4 * O.FUSED_EMUL_FIGURE if rel is None else rel) * self.scale
        if out16:
            bound = bound + 2.0 ** -8 * (self.model.abs() + bound)
        worst = float(((got - self.model).abs() / bound.clamp_min(1e-300)).max())
        fig = float(((got - self.model).abs() / self.scale.clamp_min(1e-300)).max())
        e = O.rel(got, self.ref64)
        fam = tag.split(":")[0]
        if not out16:
            _note(f"{fam} {self.c.params} element/scale", fig)
        _note(f"{fam} rel-L2 vs float64" + (" bf16" if out16 else ""), e)
        assert worst <= 1.0 and e <= (6e-3 if out16 else 5e-3), (tag, worst, fig, e)

    def intact(self):
        return all(b is None or b.intact() for b in (self.X, self.Wt, self.B, self.coef, self.Ga, self.Be, self.Te)) and self.S.untouched()


@pytest.mark.parametrize("x_f32", [False, True], ids=["bf16x", "f32x"])
@pytest.mark.parametrize("case", O.FUSED_CASES, ids=repr)
def test_fused_groupnorm_mish_variants(case, x_f32):
    c = case
    with knobs(c.pt) as lib:
        f = Fused(c, x_f32)
        q = (lib.mi_conv3x3_pw_x32_gn_mish_tile if x_f32 else lib.mi_conv3x3_pw_gn_mish_tile)(_cd(f.d))
        assert q == O.q_fused_tile(f.d, O.Knobs(c.pt, 0, 0), x_f32) == c.pt
        lc = f.library_coef(lib)
        mine = f.coef.buf[PAD:PAD + 3 * c.N * c.K]
        _note("fused coefficient model vs library (abs)", float((lc[PAD:PAD + 3 * c.N * c.K] - mine).abs().max()))
        for out16 in (False, True):
            tag = f"fused:{c.name}:{'f32x' if x_f32 else 'bf16x'}:{'bf16' if out16 else 'f32'}"
            y2, = _twice(tag + ":coef", lambda: f.launch(lib, out16, 2))
            y3, = _twice(tag + ":sums", lambda: f.launch(lib, out16, 3))
            f.check(tag + ":coef", y2)
            f.check(tag + ":sums", y3)
            yl, = f.launch(lib, out16, 2, lc[PAD:].data_ptr())
            assert _same(y3, yl), (tag, "_gn_mish_sums != _gn_mish fed by mi_gn_coef_from_sums", float((y3.double() - yl.double()).abs().max()))
        assert f.intact()


@pytest.mark.parametrize("x_f32", [False, True], ids=["bf16x", "f32x"])
@pytest.mark.parametrize("tap", O.BORDER_TAPS)
@pytest.mark.parametrize("case", [O.FUSED_CASES[0], O.FUSED_CASES[1], O.FUSED_CASES[3]], ids=repr)
def test_fused_padding_is_zero_not_transformed(case, tap, x_f32):
    """Integer weights on one border tap only: every output of the border row / column that tap reaches past must be exactly 0 -- a padding
    pixel transformed to mish(shift) + tb instead of left zero shows in all of them.  The weights are sparse (one in eight, about K / 8 terms
    per element), so the emulation's figure -- measured on dense randn weights, where a flipped h is one term in 9 K -- says nothing here; the
    other elements are held to what the number format allows when EVERY h is one bf16 ulp off its model: 2^-7 of sum |h| |w|, plus the fp32
    accumulation's (T + 2) 2^-24."""
    c = case
    with knobs(c.pt) as lib:
        f = Fused(c, x_f32, border_tap=tap)
        for var in (2, 3):
            for out16 in (False, True):
                y, = f.launch(lib, out16, var)
                f.check(f"fused_border:{c.name}:{tap}", y, rel=2.0 ** -7 + (c.K + 2) * U)
                y = y.to(F64).view(c.N, c.H, c.W, c.Nc)
                edge = {1: y[:, 0], 7: y[:, -1], 3: y[:, :, 0], 5: y[:, :, -1]}[tap]
                assert not bool(edge.any()), (c, tap, var, out16, "a padding pixel contributed")
                assert bool(y.any())


# ---------------------------------------------------------------------------------------------------- split-K
class Workspace:
    """Exactly `need` bytes a split launch may use inside a buffer: 64 KB of zero flags, NaN partial tiles, then sentinels (and sentinels in
    front).  `registered` bytes are announced to the library (>= 128 KB, the setter's minimum)."""

    def __init__(self, need, registered=None):
        self.need = need
        self.registered = max(need, 2 * O.SK_FLAG_BYTES) if registered is None else registered
        total = max(self.registered, need) + 4096
        self.raw = torch.full((total // 4 + 128,), SENT, dtype=F32, device=DEV)
        off = (-self.raw.data_ptr() // 4) % 64 + 64                       # 256-byte aligned, sentinels in front
        self.buf = self.raw[off:off + total // 4]
        self.ptr = self.buf.data_ptr()
        assert self.ptr % 256 == 0
        self.nf = O.SK_FLAG_BYTES // 4
        self.buf[:self.nf].view(torch.int32).zero_()
        if need > O.SK_FLAG_BYTES:
            self.buf[self.nf:need // 4] = NAN
        self.snap = self.raw.clone()

    def register(self, lib):
        assert lib.mi_conv_pw_set_splitk_workspace(self.ptr, self.registered) == 0, lib.mi_last_error()

    def check(self):
        assert not bool(self.buf[:self.nf].view(torch.int32).any()), "a flag stayed up"
        n = max(self.need, O.SK_FLAG_BYTES) // 4
        assert bool((self.buf[n:] == SENT).all()) and _same(self.raw[:self.raw.numel() - self.buf.numel() - 64], self.snap[:self.raw.numel() - self.buf.numel() - 64]), \
            "written outside the workspace's need"

    def untouched(self):
        return _same(self.raw, self.snap)


@contextmanager
def registered(ws, pt, mode):
    """The test's workspace instead of the product's; at the end whatever functional._SPLITK_WS holds for the device is registered again."""
    lib, K = _lib(), _K()
    idx = torch.cuda.current_device()
    try:
        with knobs(pt, mode):
            ws.register(lib)
            K._QUERY_CACHE.clear()
            yield lib
    finally:
        torch.cuda.synchronize()
        mine = K._SPLITK_WS.get(idx)
        if mine is not None:
            lib.mi_conv_pw_set_splitk_workspace(mine.data_ptr(), mine.numel())
        else:
            lib.mi_conv_pw_set_splitk_workspace(None, 0)
        K._QUERY_CACHE.clear()


_SPLIT_VAR = {"plain": 0, "sums": 1, "x32": 0, "fused": 2, "fused32": 2}


@pytest.mark.parametrize("case", O.SPLIT_CASES, ids=repr)
def test_split_k(case):
    c = case
    d = O.split_desc(c)
    var, in32 = _SPLIT_VAR[c.variant], c.variant in ("x32", "fused32")
    ks, pt, TH, TI, need = O.pw_split(d, var, in32, O.split_kn(c, 1 << 40))
    ws = Workspace(need if ks > 1 else 0, None if ks > 1 else 1 << 20)
    kn = O.Knobs(c.pt, c.mode, ws.registered)
    facts = O.launch_facts(d, var, False, False, in32, False, kn)
    assert facts.ks == ks and facts.grid <= 400
    tag = f"split:{c.name}"
    pc = O.Plain(c.name, c.N, c.H, c.W, c.K, c.Nc, c.pt, c.K1, epi="br")
    fusedc = O.Fused(c.name, c.N, c.H, c.W, c.K, c.K // 32, c.Nc, c.pt, 4)

    def run(lib, kind):
        if var == 2:
            f = Fused(fusedc, in32)
            outs = [f.launch(lib, o16, v)[0] for o16 in (False, True) for v in (2, 3)]
            return f, outs
        f = Conv(pc, kind, False, "x32" if in32 else "bf16")
        if c.variant == "sums":
            outs = [t for o16 in (False, True) for t in f.launch(lib, o16, gsum=True)]
        else:
            outs = [f.launch(lib, o16)[0] for o16 in (False, True)]
        return f, outs

    with knobs(c.pt, 0) as lib:                                # the unsplit launches of the same operands
        assert lib.mi_conv3x3_pw_splitk(_cd(d), var, int(in32)) & 15 == 1
        base = {k: run(lib, k)[1] for k in (("randn",) if var == 2 else ("unit" if c.variant == "sums" else "int", "randn"))}
    with registered(ws, c.pt, c.mode) as lib:
        q = lib.mi_conv3x3_pw_splitk(_cd(d), var, int(in32))
        assert q == O.q_splitk(d, var, in32, kn) and q & 15 == ks and (ks == 1 or q >> 4 == pt), (q, ks, pt)
        for kind, b in base.items():
            f, a = run(lib, kind)
            _, a2 = run(lib, kind)
            ws.check()
            if ks == 1:
                assert ws.untouched(), (tag, "an unsplit launch wrote the workspace")
            for i, (u, v, w0) in enumerate(zip(a, a2, b)):
                assert _same(u, v), (tag, kind, i, "a split launch differs between two runs")
                if u.dtype == torch.int64:
                    if kind == "unit":
                        assert torch.equal(u, w0), (tag, "sums")
                    continue
                if kind != "randn" or ks == 1:
                    assert _same(u, w0), (tag, kind, i, "split != unsplit on exact operands")
                elif u.dtype == F32:
                    e = O.rel(u, w0)
                    _note("split vs unsplit rel-L2", e)
                    assert e <= 3e-6, (tag, kind, i, e)
            if var == 2:
                for y in a:
                    f.check(tag, y)
            else:
                if c.variant == "sums":
                    assert kind != "unit" or O.unit_sums_exact(O.stored(f.ref, False), pt, c.H, c.W)
                    ys = [a[0], a[2]]
                    if kind == "unit":
                        for y, g in ((a[0], a[1]), (a[2], a[3])):
                            _sums_check(tag, "unit", pc, y, g, c.H * c.W)
                else:
                    ys = a
                for y in ys:
                    f.check(tag, y)
            assert f.intact()


def test_split_k_workspace_one_partial_tile_short():
    c = next(c for c in O.SPLIT_CASES if c.name == "sk4_k512")
    d = O.split_desc(c)
    ks, pt, _, _, need = O.pw_split(d, 0, False, O.split_kn(c, 1 << 40))
    assert ks == 4 and need - pt * 512 >= 2 * O.SK_FLAG_BYTES
    pc = O.Plain(c.name, c.N, c.H, c.W, c.K, c.Nc, c.pt, epi="b")
    f = Conv(pc, "randn")
    with knobs(c.pt, 0) as lib:
        base, = f.launch(lib, False)
    for short, want in ((0, 4), (pt * 512, 1)):
        ws = Workspace(need, need - short)
        with registered(ws, c.pt, c.mode) as lib:
            assert lib.mi_conv3x3_pw_splitk(_cd(d), 0, 0) & 15 == want == O.q_splitk(d, 0, False, O.Knobs(c.pt, c.mode, need - short)) & 15
            y, = f.launch(lib, False)
            if want == 1:
                assert ws.untouched() and _same(y, base), "a workspace one partial tile short must run unsplit and stay untouched"
            else:
                ws.check()
                f.check("split:short", y)


def test_split_k_flag_area_too_small():
    """(ks - 1) tiles 16 bytes of flags must fit 64 KB: 1 536 tiles under a split of 4 do not (the partial tiles would fit the workspace).
    The launch reports split 1, runs unsplit -- bit-equal to the launch with splits off -- and leaves the workspace untouched."""
    d = O.FLAG_EDGE
    need4 = O.SK_FLAG_BYTES + 3 * 1536 * 64 * 512
    assert O.pw_split(d, 0, False, O.Knobs(64, 4, need4))[0] == 1 and O.pw_split(d._replace(N=128), 0, False, O.Knobs(64, 4, need4))[0] == 4
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(d.N * 64, d.K, device=DEV, generator=g).to(BF)
    w = (torch.randn(9 * d.K * d.Nc, device=DEV, generator=g) * (9 * d.K) ** -0.5).to(BF)

    def run(lib):
        y = Out(d.N * 64, d.Nc, dtype=BF)
        assert lib.mi_conv3x3_pw(_cd(d), x.data_ptr(), None, w.data_ptr(), None, None, y.ptr, 1, _stream()) == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        return y.get()
    with knobs(64, 0) as lib:
        base = run(lib)
    ws = Workspace(need4)
    with registered(ws, 64, 4) as lib:
        assert lib.mi_conv3x3_pw_splitk(_cd(d), 0, 0) == (64 << 4) | 1
        y = run(lib)
        assert ws.untouched() and _same(y, base)
    assert bool(torch.isfinite(base.float()).all())


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_everything_untouched():
    """Every condition of pw_ok, pw_geom and pw_launch and of the workspace setter: a non-zero return, mi_last_error set, y, the sums and
    the workspace as they were, and the *_supported / *_tile query of the entry point in agreement.  The oracle says beforehand that
    each call is one the host checks refuse."""
    lib = _lib()
    big = 1 << 20
    x16, x32 = In(torch.zeros(big // 8, 8, dtype=F64), dtype=BF), In(torch.zeros(big // 8, 8, dtype=F64))
    w = In(torch.zeros(1, 9 * 256 * 128, dtype=F64), dtype=BF)
    f4 = In(torch.zeros(1, 1 << 16, dtype=F64))
    y, gs, sums = Out(1, big), Sums(64, 256), Sums(64, 256)
    ws = Workspace(1 << 20)
    n = [0]
    kn = O.Knobs(0, 0, 0)

    def refused(rc, what):
        n[0] += 1
        assert rc != 0, ("accepted", what)
        assert lib.mi_last_error(), what
        assert y.untouched() and gs.untouched() and ws.untouched(), ("written", what)

    ok = O.desc(2, 8, 16, 128, 128)

    def pw(d, x=x16.ptr, x2=None, wp=w.ptr, res=None, yp=y.ptr, out16=0, dp=True):
        return lib.mi_conv3x3_pw(_cd(d) if dp else None, x, x2, wp, f4.ptr, res, yp, out16, _stream())

    with registered(ws, 0, 0):
        assert O.launch_accepts(ok, 0, False, kn) and lib.mi_conv3x3_pw_supported(_cd(ok)) == 1
        # ---- pw_ok and pw_geom, through every entry point's query and mi_conv3x3_pw / _x32 / _f32
        bad = [ok._replace(KH=1), ok._replace(KW=5), ok._replace(pad=0), ok._replace(stride=2), ok._replace(mode=0), ok._replace(IH=16), ok._replace(IW=8),
               ok._replace(K=96, K1=96, ldx=96), ok._replace(K1=32, ldx2=96), ok._replace(Nc=96, ldy=96), ok._replace(ldx=132), ok._replace(K1=64, ldx=64, ldx2=68),
               ok._replace(N=1, OH=4, IH=4, OW=8, IW=8),                          # 32 pixels: no tile divides them
               ok._replace(OW=4, IW=4, OH=32, IH=32), ok._replace(OW=64, IW=64, OH=2, IH=2),          # W = 4, W = 64
               ok._replace(OH=6, IH=6, N=4),                                    # H % rows (128: 8 rows, 64: 4 rows)
               ok._replace(N=3, OH=4, IH=4, OW=8, IW=8),                          # N % TI: 96 pixels
               ok._replace(N=8, OH=2, IH=2, OW=8, IW=8)]                          # TI > 2: 16 pixels per image
        for d in bad:
            assert not O.launch_accepts(d, 0, False, kn), d
            assert lib.mi_conv3x3_pw_supported(_cd(d)) == 0 and lib.mi_conv3x3_pw_tile(_cd(d)) == 0, d
            refused(pw(d), ("pw", d))
        for pt, d in [(128, ok._replace(N=3, OH=8, IH=8, OW=8, IW=8)),            # 128-pixel tiles hold two 8 x 8 images: N % TI
                      (64, ok._replace(N=4, OH=2, IH=2, OW=8, IW=8)),             # TI = 4
                      (256, ok._replace(N=4, OH=8, IH=8, OW=16, IW=16)),          # 256 with TI > 1
                      (256, ok._replace(N=8, OH=4, IH=4, OW=32, IW=32)),
                      (128, ok._replace(N=2, OH=2, IH=2, OW=32, IW=32))]:         # TH = 2 is no multiple of the band's four rows
            with knobs(pt):
                assert not O.launch_accepts(d, 0, False, O.Knobs(pt, 0, 0)) and lib.mi_conv3x3_pw_tile(_cd(d)) == 0, (pt, d)
                refused(pw(d), ("pw forced", pt, d))
        with knobs(256):                                                          # 256-pixel tiles: the plain bf16 conv only
            d = ok._replace(N=2, OH=16, IH=16)
            assert lib.mi_conv3x3_pw_tile(_cd(d)) == 256 and lib.mi_conv3x3_pw_x32_tile(_cd(d)) == 0 and lib.mi_conv3x3_pw_gn_mish_tile(_cd(d)) == 0
            refused(lib.mi_conv3x3_pw_x32(_cd(d), x32.ptr, None, w.ptr, None, None, y.ptr, 0, None, _stream()), "x32 at 256")
            refused(lib.mi_conv3x3_pw_gn_mish(_cd(d), x16.ptr, f4.ptr, w.ptr, None, y.ptr, 0, _stream()), "fused at 256")
        assert lib.mi_debug_conv_pw_tile(96) != 0 and lib.mi_last_error()
        assert lib.mi_conv3x3_pw_tile(_cd(ok)) == 64                              # ... and the forced tile is still none
        # mode against entry point; granularity per storage
        f32d = ok._replace(mode=0)
        assert lib.mi_conv3x3_pw_f32_tile(_cd(f32d)) and not lib.mi_conv3x3_pw_f32_tile(_cd(ok))
        refused(lib.mi_conv3x3_pw_f32(_cd(ok), x32.ptr, None, f4.ptr, None, None, y.ptr, _stream()), "f32 entry, bf16 mode")
        refused(lib.mi_conv3x3_pw_x32(_cd(f32d), x32.ptr, None, w.ptr, None, None, y.ptr, 0, None, _stream()), "x32 entry, fp32 mode")
        for d in (f32d._replace(K1=48, ldx=48, ldx2=80), f32d._replace(ldx=130), f32d._replace(K1=64, ldx=64, ldx2=66)):
            assert not O.launch_accepts(d, 0, False, kn, f32=True, has_x2=True) and lib.mi_conv3x3_pw_f32_tile(_cd(d)) == 0
            refused(lib.mi_conv3x3_pw_f32(_cd(d), x32.ptr, x32.ptr, f4.ptr, None, None, y.ptr, _stream()), ("f32", d))
        assert lib.mi_conv3x3_pw_f32_tile(_cd(f32d._replace(K1=32, ldx=32, ldx2=96)))          # K1 % 32 is the exact-fp32 form's granularity
        for d in (ok._replace(ldx=130), ok._replace(K1=64, ldx=64, ldx2=66)):
            assert not O.launch_accepts(d, 0, False, kn, in32=True, has_x2=True) and lib.mi_conv3x3_pw_x32_supported(_cd(d)) == 0
            refused(lib.mi_conv3x3_pw_x32(_cd(d), x32.ptr, x32.ptr, w.ptr, None, None, y.ptr, 0, None, _stream()), ("x32", d))
        assert lib.mi_conv3x3_pw_x32_supported(_cd(ok._replace(ldx=132))) == 1 and lib.mi_conv3x3_pw_supported(_cd(ok._replace(ldx=132))) == 0
        # ---- pw_launch
        for kw, what in [(dict(dp=False), "d"), (dict(x=None), "x"), (dict(wp=None), "w"), (dict(yp=None), "y")]:
            assert not O.launch_accepts(ok, 0, False, kn, null=(what,))
            refused(pw(ok, **kw), "null " + what)
        two = ok._replace(K1=64, ldx=64, ldx2=64)
        assert O.launch_accepts(two, 0, False, kn, has_x2=True) and not O.launch_accepts(two, 0, False, kn)
        refused(pw(two), "two sources without x2")
        refused(pw(ok, x=x16.ptr + 8), "x 8 bytes off")
        refused(pw(two, x2=x16.ptr + 8), "x2 8 bytes off")
        refused(pw(ok, wp=w.ptr + 8), "w 8 bytes off")
        assert not O.launch_accepts(ok, 0, False, kn, x_off=8) and not O.launch_accepts(two, 0, False, kn, has_x2=True, x2_off=8) and not O.launch_accepts(ok, 0, False, kn, w_off=8)
        for d, res in [(ok._replace(ldy=132), None), (ok._replace(ldr=130), f4.ptr)]:
            assert not O.launch_accepts(d, 0, False, kn, has_res=res is not None)
            refused(pw(d, res=res), ("pitch", d))
        assert O.launch_accepts(ok._replace(ldr=130), 0, False, kn)               # (no residual: ldr is not looked at)
        refused(lib.mi_conv3x3_pw_gnsums(_cd(ok), x16.ptr, None, w.ptr, None, None, y.ptr, 0, None, _stream()), "sums without a buffer")
        assert not O.launch_accepts(ok, 1, False, kn, null=("gsum",))
        refused(lib.mi_conv3x3_pw_f32(_cd(f32d), x32.ptr, None, f4.ptr, None, None, None, _stream()), "f32 null y")
        # fused
        fd = O.desc(2, 8, 16, 128, 128)

        def fx(d=fd, coef=f4.ptr, x=x16.ptr):
            return lib.mi_conv3x3_pw_gn_mish(_cd(d), x, coef, w.ptr, None, y.ptr, 0, _stream())

        def fs(d=fd, s=sums.ptr, ga=f4.ptr, be=f4.ptr, te=None, ldt=0, G=4, x32_=False):
            fn = lib.mi_conv3x3_pw_x32_gn_mish_sums if x32_ else lib.mi_conv3x3_pw_gn_mish_sums
            return fn(_cd(d), x32.ptr if x32_ else x16.ptr, s, ga, be, te, ldt, G, 1e-5, w.ptr, None, y.ptr, 0, _stream())
        assert O.launch_accepts(fd, 2, False, kn) and O.launch_accepts(fd, 3, False, kn, G=4) and lib.mi_conv3x3_pw_gn_mish_supported(_cd(fd)) == 1
        d2 = fd._replace(K1=64, ldx=64, ldx2=64)
        assert lib.mi_conv3x3_pw_gn_mish_supported(_cd(d2)) == 0 and not O.launch_accepts(d2, 2, False, kn, has_x2=True)
        refused(fx(d2), "fused with two sources")
        ti2 = O.desc(2, 4, 8, 128, 128)                                           # 64-pixel tiles hold two 4 x 8 images
        assert lib.mi_conv3x3_pw_gn_mish_supported(_cd(ti2)) == 0 == lib.mi_conv3x3_pw_x32_gn_mish_supported(_cd(ti2)) and not O.launch_accepts(ti2, 2, False, kn)
        assert lib.mi_conv3x3_pw_supported(_cd(ti2)) == 1
        refused(fx(ti2), "fused with TI = 2")
        refused(fs(ti2), "fused (sums) with TI = 2")
        k1088 = O.desc(2, 8, 16, 1088, 64)
        assert lib.mi_conv3x3_pw_gn_mish_tile(_cd(k1088)) == 0 and lib.mi_conv3x3_pw_supported(_cd(k1088)) == 1 and not O.launch_accepts(k1088, 2, False, kn)
        refused(fx(k1088), "fused with K > 1024")
        refused(fx(coef=None), "coef null")
        refused(fx(coef=f4.ptr + 8), "coef 8 bytes off")
        assert not O.launch_accepts(fd, 2, False, kn, null=("coef",)) and not O.launch_accepts(fd, 2, False, kn, coef_off=8)
        for G in (0, -1, 3, 16, 1):                                               # G <= 0, K % G, K / G = 8 and 128 (48: K = 192 below)
            assert not O.launch_accepts(fd, 3, False, kn, G=G), G
            refused(fs(G=G), ("G", G))
        d192 = O.desc(2, 8, 16, 192, 64)
        assert not O.launch_accepts(d192, 3, False, kn, G=4) and O.launch_accepts(d192, 3, False, kn, G=6)
        refused(fs(d192, G=4), "K / G = 48")
        for kw, acc in [(dict(s=None), dict(null=("sums",))), (dict(ga=None), dict(null=("gamma",))), (dict(be=None), dict(null=("beta",))),
                        (dict(s=sums.ptr + 8), dict(gn_off=(8, 0, 0, 0))), (dict(ga=f4.ptr + 4), dict(gn_off=(0, 4, 0, 0))), (dict(be=f4.ptr + 4), dict(gn_off=(0, 0, 4, 0))),
                        (dict(te=f4.ptr + 8, ldt=128), dict(gn_off=(0, 0, 0, 8), has_temb=True, ldt=128)), (dict(te=f4.ptr, ldt=130), dict(has_temb=True, ldt=130))]:
            assert not O.launch_accepts(fd, 3, False, kn, G=4, **acc), acc
            refused(fs(**kw), ("fused sums", kw.keys()))
            refused(fs(x32_=True, **kw), ("fused sums x32", kw.keys()))
    # ---- the workspace setter
    assert lib.mi_conv_pw_set_splitk_workspace(ws.ptr, 2 * O.SK_FLAG_BYTES - 1) != 0 and lib.mi_last_error()
    assert lib.mi_conv_pw_set_splitk_workspace(ws.ptr + 128, 1 << 20) != 0 and lib.mi_last_error()
    torch.cuda.synchronize()
    assert ws.untouched() and y.untouched() and x16.intact() and x32.intact() and w.intact() and f4.intact() and sums.untouched() and n[0] >= 70
