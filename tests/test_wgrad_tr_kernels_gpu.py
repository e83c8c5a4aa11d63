"""csrc/wgrad_tr.hip, wgrad1x1_tr.hip and wgrad_s2_tr.hip on the MI355X against tests/_wgrad_oracle.py, through the C ABI
(load_library(), MiWgradDesc, torch's current stream): every case of the oracle's lists (tests/test_wgrad_tr_cpu.py holds them to the
edges they reach), each with integer-valued and with randn operands.

Buffers.  Operands are views at their pitch (P, P2 and Q all different) inside NaN-filled buffers: NaN in front, behind and in the
padding of every row.  dW and dbias start from non-zero integers inside sentinel-filled buffers with a sentinel tail.  The workspace
is exactly the bytes the *_workspace function reports (nothing, a null pointer, when no layer has k-slices) inside a NaN-filled
buffer whose front and tail must survive; a reduce that read a slice nobody wrote would add NaN.  Every launch runs twice from the
same start and dW must be bit-equal (fixed-order reduce); dbias, summed with atomics, is compared bit for bit only in the integer cases.

Integer operands (X in {-4..4}, dY in {-3..3}, initial content in {-3..3}): every product and partial sum is exact in fp32 and bf16
storage, so the result must be torch.equal to the float64 reference cast to fp32 under every plan, dbias included.  No tolerance.

randn operands, the project's bounds (tests/test_kernels_gpu.py): rel-L2 against float64 on the stored operands <= 2e-5 with bf16
operands, <= 3e-6 fp32 3x3, <= 2e-6 fp32 1x1 and fp32 stride 2, dbias <= 1e-5; and per element
|got - ref| <= N H W 2^-24 sum |x||dy|, the worst case of any fp32 summation order.

Measured on the MI355X (worst over the cases; not used as bounds): rel-L2 bf16 3x3 1.6e-7, fp32 3x3 5.0e-7, bf16 1x1 3.0e-7 (dbias
2.4e-7), fp32 1x1 3.2e-7 (dbias 1.6e-7), bf16 stride 2 1.0e-7, fp32 stride 2 1.9e-7; the worst element sits at 0.078 of its bound.

What the product library cannot reach: the MI_W* knobs (MI_WTR_BLOCKS, MI_WTR_XCD, MI_W1_NI, MI_W1_XCD, MI_WS2_BLOCKS,
MI_WS2_XCD) are constants outside -DMI_EXPERIMENT builds, so NI = 1
at Ci % 128 == 0, xcd_map off for a multi-tile split layer of the 1x1 / stride-2 kernels, and any stride-2 plan other than the one its
batch composition gives have no test here.  The stride-2 bf16 kernel has no blocks hook: its k-slices are one step long unless tiles x
steps exceed 256 workgroups, which the four sps2 / sps3 / sps4 cases arrange (2 to 4 steps per slice; longer slices need larger shapes)."""
import ctypes
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wgrad_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -776.0                        # never-written sentinel
PAD = 64                             # elements in front of and behind a view (a multiple of 16 bytes in both dtypes)
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
U = 2.0 ** -24
WORST = {}


def _lib():
    from src.ops.lib import load_library
    return load_library()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cdescs(ds):
    from src.ops.lib import MiWgradDesc
    return (MiWgradDesc * len(ds))(*[MiWgradDesc(**d) for d in ds])


def _parr(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst measured: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


class In:
    """Rows of t64 [..., C] at pitch ld inside a NaN-filled buffer: NaN in front, behind and in the padding of every row."""

    def __init__(self, t64, ld, dtype):
        t64 = t64.reshape(-1, t64.shape[-1])
        R, C = t64.shape
        assert ld >= C
        self.buf = torch.full((2 * PAD + R * ld,), NAN, dtype=dtype, device=DEV)
        rows = self.buf[PAD:PAD + R * ld].view(R, ld)
        rows[:, :C].copy_(t64.to(dtype))
        assert rows.data_ptr() % 16 == 0
        self.ptr = rows.data_ptr()
        self.snap = self.buf.clone()

    def intact(self):
        return bool(torch.equal(self.buf.view(torch.int16 if self.buf.dtype == BF else torch.int32),
                                self.snap.view(torch.int16 if self.buf.dtype == BF else torch.int32)))


class Out:
    """n fp32 results behind PAD sentinels, with a sentinel tail, starting from init."""

    def __init__(self, init64):
        self.n = init64.numel()
        self.buf = torch.full((PAD + self.n + 256,), SENT, dtype=F32, device=DEV)
        self.buf[PAD:PAD + self.n].copy_(init64.reshape(-1).to(F32))
        self.ptr = self.buf[PAD:].data_ptr()
        self.snap = self.buf.clone()

    def get(self):
        assert bool((self.buf[:PAD] == SENT).all()) and bool((self.buf[PAD + self.n:] == SENT).all()), "written outside the result"
        return self.buf[PAD:PAD + self.n].cpu()

    def untouched(self):
        return bool(torch.equal(self.buf, self.snap))


class Ws:
    """Exactly nbytes of workspace inside a NaN-filled buffer; nothing (a null pointer) when nbytes == 0."""

    def __init__(self, nbytes):
        assert nbytes % 4 == 0
        self.nbytes, self.n = nbytes, nbytes // 4
        self.buf = torch.full((PAD + self.n + 256,), NAN, dtype=F32, device=DEV)
        self.ptr = self.buf[PAD:].data_ptr() if nbytes else None
        assert not self.ptr or self.ptr % 16 == 0

    def check(self):
        assert bool(torch.isnan(self.buf[:PAD]).all()) and bool(torch.isnan(self.buf[PAD + self.n:]).all()), "written outside the workspace"

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def _ws_bytes(reported, plan):
    """The library's figure must be the oracle's; a plan without k-slices gets no workspace at all."""
    assert reported == plan["ws_bytes"], (reported, plan["ws_bytes"])
    return reported if plan["ws_floats"] else 0


def _check(tag, kind, got, init, grad, absgrad, npix, bound, what="dW"):
    """got: fp32 result (cpu); init + grad: the float64 reference; absgrad: the same contraction on |operands|."""
    init, grad, absgrad = init.reshape(-1), grad.reshape(-1), absgrad.reshape(-1)
    ref = init + grad
    assert bool(torch.isfinite(got).all()), (tag, "non-finite")
    if kind == "int":
        bad = (got != ref.to(F32)).nonzero().flatten()
        assert bad.numel() == 0, (tag, what, f"{bad.numel()} wrong elements, first at {int(bad[0])}: {float(got[bad[0]])} != {float(ref[bad[0]])}")
        return
    e = O.rel(got.to(F64) - init, grad)
    worst = float(((got.to(F64) - ref).abs() / (npix * U * absgrad).clamp_min(1e-300)).max())
    print(f"{tag} {what}: rel-L2 {e:.3g} (bound {bound:.0e}), worst element at {worst:.3g} of its bound")
    _note(f"{tag.split(':')[0]} {what}", e)
    _note(f"{tag.split(':')[0]} {what} element/bound", worst)
    assert e <= bound and worst <= 1.0, (tag, what, e, worst)


def _twice(tag, launch):
    """launch() -> (list of dW tensors, list of dbias tensors or None).  Two runs from the same start: dW bit-equal."""
    a, b = launch(), launch()
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (tag, "dW differs between two runs")
    return a


# ---------------------------------------------------------------------------------------------------- 3x3 stride 1
def run_tr(lib, c, kind):
    descs = O.tr_descs(c)
    dt, tag = (BF if c.mode else F32), ("tr" if c.mode else "tr32") + ":" + c.name
    L = []
    for i, (l, d) in enumerate(zip(c.layers, descs)):
        N, H, W, Ci, Cj = l[:5]
        x, dy = O.operands((N, H, W, Ci), (N, H, W, Cj), kind, _seed(c.name, i, kind), c.mode == 1, c.mode == 1)
        I1 = d["I1"]
        L.append(dict(P=In(x[..., :I1], d["ldp"], dt), P2=In(x[..., I1:], d["ldp2"], dt) if I1 != Ci else None, Q=In(dy, d["ldq"], dt),
                      grad=O.wgrad3x3_ref(x, dy), absg=O.wgrad3x3_ref(x.abs(), dy.abs()), init=O.init_content(9 * Ci * Cj), npix=N * H * W))
    n = len(L)
    try:
        lib.mi_debug_wgrad_tr_blocks(c.blocks)
        cd = _cdescs(descs)
        plan = O.tr_plan(descs, c.blocks)
        nbytes = _ws_bytes(lib.mi_conv3x3_wgrad_tr_batch_workspace(n, cd), plan)

        def launch():
            dW, ws = [Out(a["init"]) for a in L], Ws(nbytes)
            if n == 1:
                rc = lib.mi_conv3x3_wgrad_tr(ctypes.byref(cd[0]), L[0]["P"].ptr, L[0]["P2"].ptr if L[0]["P2"] else None, L[0]["Q"].ptr, dW[0].ptr,
                                             ws.ptr, ws.nbytes, _stream())
            else:
                rc = lib.mi_conv3x3_wgrad_tr_batch(n, cd, _parr([a["P"].ptr for a in L]), _parr([a["P2"].ptr if a["P2"] else None for a in L]),
                                                   _parr([a["Q"].ptr for a in L]), _parr([o.ptr for o in dW]), ws.ptr, ws.nbytes, _stream())
            assert rc == 0, lib.mi_last_error()
            torch.cuda.synchronize()
            ws.check()
            return [o.get() for o in dW], None
        got, _ = _twice(tag, launch)
    finally:
        lib.mi_debug_wgrad_tr_blocks(0)
    for i, (a, g) in enumerate(zip(L, got)):
        assert a["P"].intact() and a["Q"].intact() and (a.get("P2") is None or a["P2"].intact())
        _check(f"{tag}:{i}", kind, g, a["init"], a["grad"], a["absg"], a["npix"], 2e-5 if c.mode else 3e-6)


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.TR_CASES, ids=repr)
def test_wgrad3x3_tr(case, kind):
    run_tr(_lib(), case, kind)


# ---------------------------------------------------------------------------------------------------- 1x1
def run_w1(lib, c, kind):
    descs, q32 = O.w1_descs(c)
    xdt, tag = (BF if c.mode else F32), ("w1" if c.mode else "w1f32") + ":" + c.name
    L = []
    for i, (l, d) in enumerate(zip(c.layers, descs)):
        k, Ci, Cj, I1, q, bias = l
        x, dy = O.operands((64 * k, Ci), (64 * k, Cj), kind, _seed(c.name, i, kind), c.mode == 1, not q)
        dy_dw = O.bf16_round(dy) if (c.mode == 1 and q) else dy              # bf16 mode rounds an fp32 dY for the product, not for the bias sum
        grad, db = O.wgrad1x1_ref(x, dy, dy_dw=dy_dw)
        L.append(dict(P=In(x[:, :I1], d["ldp"], xdt), P2=In(x[:, I1:], d["ldp2"], xdt) if I1 != Ci else None, Q=In(dy, d["ldq"], F32 if q else BF),
                      grad=grad, absg=O.wgrad1x1_ref(x.abs(), dy_dw.abs())[0], db=db, absdb=dy.abs().sum(0), bias=bias,
                      init=O.init_content(Ci * Cj), binit=O.init_content(Cj) + 1, npix=64 * k))
    n = len(L)
    try:
        lib.mi_debug_wgrad1x1_tr_blocks(c.blocks)
        cd, cq = _cdescs(descs), (ctypes.c_int * n)(*q32)
        plan = O.w1_plan(descs, q32, c.blocks)
        nbytes = _ws_bytes(lib.mi_conv1x1_wgrad_tr_batch_workspace(n, cd, cq), plan)

        def launch():
            dW, ws = [Out(a["init"]) for a in L], Ws(nbytes)
            dB = [Out(a["binit"]) if a["bias"] else None for a in L]
            rc = lib.mi_conv1x1_wgrad_tr_batch(n, cd, cq, _parr([a["P"].ptr for a in L]), _parr([a["P2"].ptr if a["P2"] else None for a in L]),
                                               _parr([a["Q"].ptr for a in L]), _parr([o.ptr for o in dW]), _parr([o.ptr if o else None for o in dB]),
                                               ws.ptr, ws.nbytes, _stream())
            assert rc == 0, lib.mi_last_error()
            torch.cuda.synchronize()
            ws.check()
            return [o.get() for o in dW], [o.get() if o else None for o in dB]
        got, gotb = _twice(tag, launch)
    finally:
        lib.mi_debug_wgrad1x1_tr_blocks(0)
    for i, (a, g, gb) in enumerate(zip(L, got, gotb)):
        assert a["P"].intact() and a["Q"].intact() and (a.get("P2") is None or a["P2"].intact())
        _check(f"{tag}:{i}", kind, g, a["init"], a["grad"], a["absg"], a["npix"], 2e-5 if c.mode else 2e-6)
        if a["bias"]:
            _check(f"{tag}:{i}", kind, gb, a["binit"], a["db"], a["absdb"], a["npix"], 1e-5, "dbias")


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.W1_CASES, ids=repr)
def test_wgrad1x1_tr(case, kind):
    run_w1(_lib(), case, kind)


# ---------------------------------------------------------------------------------------------------- stride 2, bf16
def _s2_shapes(N, h, w, Ci, Cj, gather_i):
    return ((N, 2 * h, 2 * w, Ci), (N, h, w, Cj)) if gather_i else ((N, h, w, Ci), (N, 2 * h, 2 * w, Cj))


def run_s2(lib, c, kind):
    descs = O.s2_descs(c)
    tag = "s2:" + c.name
    L = []
    for i, (l, d) in enumerate(zip(c.layers, descs)):
        N, h, w, Ci, Cj, ks = l
        p, q = O.operands(*_s2_shapes(N, h, w, Ci, Cj, d["gather_i"]), kind, _seed(c.name, i, kind), True, True)
        L.append(dict(P=In(p, d["ldp"], BF), Q=In(q, d["ldq"], BF), grad=O.wgrad_s2_ref(p, q, ks, d["gather_i"]),
                      absg=O.wgrad_s2_ref(p.abs(), q.abs(), ks, d["gather_i"]), init=O.init_content(ks * ks * Ci * Cj), npix=N * h * w))
    n = len(L)
    cd = _cdescs(descs)
    nbytes = _ws_bytes(lib.mi_conv_s2_wgrad_tr_batch_workspace(n, cd), O.s2_plan(descs))

    def launch():
        dW, ws = [Out(a["init"]) for a in L], Ws(nbytes)
        rc = lib.mi_conv_s2_wgrad_tr_batch(n, cd, _parr([a["P"].ptr for a in L]), _parr([a["Q"].ptr for a in L]), _parr([o.ptr for o in dW]),
                                           ws.ptr, ws.nbytes, _stream())
        assert rc == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        ws.check()
        return [o.get() for o in dW], None
    got, _ = _twice(tag, launch)
    for i, (a, g) in enumerate(zip(L, got)):
        assert a["P"].intact() and a["Q"].intact() and (a.get("P2") is None or a["P2"].intact())
        _check(f"{tag}:{i}", kind, g, a["init"], a["grad"], a["absg"], a["npix"], 2e-5)


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.S2_CASES, ids=repr)
def test_wgrad_s2_tr(case, kind):
    run_s2(_lib(), case, kind)


# ---------------------------------------------------------------------------------------------------- stride 2, exact fp32
def run_s2f(lib, c, kind):
    d = O.s2f_desc(c)
    N, h, w, Ci, Cj, ks, g = c.layers[0]
    tag = "s2f32:" + c.name
    p, q = O.operands(*_s2_shapes(N, h, w, Ci, Cj, g), kind, _seed(c.name, kind), False, False)
    P, Q = In(p, d["ldp"], F32), In(q, d["ldq"], F32)
    grad, absg, init = O.wgrad_s2_ref(p, q, ks, g), O.wgrad_s2_ref(p.abs(), q.abs(), ks, g), O.init_content(ks * ks * Ci * Cj)
    cd = _cdescs([d])
    nbytes = _ws_bytes(lib.mi_conv_s2_wgrad_f32_workspace(ctypes.byref(cd[0])), O.s2f_plan(d))       # its two launches share this workspace

    def launch():
        dW, ws = Out(init), Ws(nbytes)
        rc = lib.mi_conv_s2_wgrad_f32(ctypes.byref(cd[0]), P.ptr, Q.ptr, dW.ptr, ws.ptr, ws.nbytes, _stream())
        assert rc == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        ws.check()
        return [dW.get()], None
    got, _ = _twice(tag, launch)
    assert P.intact() and Q.intact()
    _check(tag, kind, got[0], init, grad, absg, N * h * w, 2e-6)


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", O.S2F_CASES, ids=repr)
def test_wgrad_s2_f32(case, kind):
    run_s2f(_lib(), case, kind)


# ---------------------------------------------------------------------------------------------------- refusals
class Rig:
    """Buffers of one batch, large enough for every supported neighbour a refusal test passes; a refused call must leave all of them, the inputs included, alone."""

    def __init__(self, n, pdt, qdt, elems=1 << 18, out_elems=1 << 18):
        z = torch.ones(elems // 64, 64, dtype=F64)           # dense rows of ones: whatever pitch a descriptor names stays inside them
        self.n = n
        self.P, self.P2, self.Q = [In(z, 64, pdt) for _ in range(n)], [In(z, 64, pdt) for _ in range(n)], [In(z, 64, qdt) for _ in range(n)]
        self.dW, self.dB = [Out(O.init_content(out_elems)) for _ in range(n)], [Out(O.init_content(512)) for _ in range(n)]
        self.ws = Ws(64 << 20)

    def arrays(self, off=(0, 0, 0)):
        return (_parr([a.ptr + off[0] for a in self.P]), _parr([a.ptr + off[1] for a in self.P2]), _parr([a.ptr + off[2] for a in self.Q]),
                _parr([o.ptr for o in self.dW]), _parr([o.ptr for o in self.dB]))

    def untouched(self):
        torch.cuda.synchronize()
        return all(o.untouched() for o in self.dW + self.dB) and self.ws.untouched() and all(b.intact() for b in self.P + self.P2 + self.Q)


def _refused(lib, rig, rc, why):
    assert rc != 0, f"accepted: {why}"
    assert lib.mi_last_error(), why
    assert rig.untouched(), f"refused but wrote: {why}"


# a supported base per entry point, and one descriptor for each reason its *_supported check lists
def _bad(base, **kw):
    d = dict(base, **kw)
    if "DW" in kw:
        d["GW"] = kw["DW"] * (2 if base["stride"] == 2 else 1)
    if "DH" in kw:
        d["GH"] = kw["DH"] * (2 if base["stride"] == 2 else 1)
    return d


def test_refusals_3x3():
    lib = _lib()
    for mode in (1, 0):
        base = O.d3(4, 4, 16, 128, 96, 64, mode)          # 4 k-slices: a split plan
        assert O.tr_plan([base])["ws_floats"] > 0
        rig = Rig(2, BF if mode else F32, BF if mode else F32)
        P, P2, Q, dW, _ = rig.arrays()
        need = O.tr_plan([base, base])["ws_need"]

        def call(ds, n=None, arr=(P, P2, Q, dW), ws=rig.ws.ptr, nbytes=rig.ws.nbytes):
            return lib.mi_conv3x3_wgrad_tr_batch(len(ds) if n is None else n, _cdescs(ds), *arr, ws, nbytes, _stream())
        bads = [_bad(base, DW=24), _bad(base, DW=128), _bad(base, DH=3), _bad(base, N=1, DH=2, DW=16), _bad(base, Ci=96), _bad(base, I1=32), _bad(base, Cj=48),
                _bad(base, Cj=16), _bad(base, ldp=base["ldp"] + 2), _bad(base, ldp2=base["ldp2"] + 2), _bad(base, ldq=base["ldq"] + 2), _bad(base, KH=1, KW=1),
                _bad(base, stride=2), _bad(base, pad=0), _bad(base, gather_i=0), _bad(base, mode=2), _bad(base, GH=8)]
        for d in bads:
            assert not O.tr_ok(d), d
            _refused(lib, rig, call([base, d]), d)
            _refused(lib, rig, lib.mi_conv3x3_wgrad_tr(ctypes.byref(_cdescs([d])[0]), rig.P[0].ptr, rig.P2[0].ptr, rig.Q[0].ptr, rig.dW[0].ptr, rig.ws.ptr,
                                                       rig.ws.nbytes, _stream()), d)
        _refused(lib, rig, call([base, base], n=0), "n = 0")
        _refused(lib, rig, call([base] * 9, n=9, arr=[_parr(list(a) * 5) for a in (P, P2, Q, dW)]), "n = 9")
        for k in range(3):
            off = [0, 0, 0]
            off[k] = 8
            _refused(lib, rig, call([base, base], arr=rig.arrays(tuple(off))[:4]), f"pointer {k} 8 bytes off")
        _refused(lib, rig, call([base, base], ws=rig.ws.ptr + 8), "workspace 8 bytes off")
        _refused(lib, rig, call([base, base], ws=None, nbytes=0), "null workspace for a split plan")
        _refused(lib, rig, call([base, base], nbytes=need - 16), "workspace 16 bytes short of what the plan writes")
        _refused(lib, rig, call([base, dict(base, mode=1 - mode, ldp=72, ldp2=72, ldq=104)]), "mixed modes")
        _refused(lib, rig, call([base, base], arr=(P, _parr([None, None]), Q, dW)), "two sources without P2")
        assert call([base, base], nbytes=need) == 0, lib.mi_last_error()       # ... and exactly what the plan writes is enough
        torch.cuda.synchronize()
        assert not rig.dW[0].untouched() and not rig.dW[1].untouched()
    run_tr(lib, O.TR_CASES[0], "int")                     # a valid call after the refusals gives the exact result
    run_tr(lib, [c for c in O.TR_CASES if c.name == "batch3_unsplit_mid-bf16"][0], "int")


def test_refusals_1x1():
    lib = _lib()
    for mode in (1, 0):
        base = O.d1(4, 128, 96, 64, mode)
        assert O.w1_plan([base], [1])["ws_floats"] > 0
        rig = Rig(2, BF if mode else F32, F32)
        P, P2, Q, dW, dB = rig.arrays()
        need = O.w1_plan([base, base], [1, 1])["ws_need"]

        def call(ds, q32=(1, 1), n=None, arr=(P, P2, Q, dW, dB), ws=rig.ws.ptr, nbytes=rig.ws.nbytes):
            return lib.mi_conv1x1_wgrad_tr_batch(len(ds) if n is None else n, _cdescs(ds), (ctypes.c_int * len(q32))(*q32), *arr, ws, nbytes, _stream())
        bads = [_bad(base, N=1, DH=4, DW=8), _bad(base, Ci=96), _bad(base, I1=32), _bad(base, Cj=48), _bad(base, Cj=16), _bad(base, ldp=base["ldp"] + 2),
                _bad(base, ldp2=base["ldp2"] + 2), _bad(base, ldq=base["ldq"] + 2), _bad(base, KH=3, KW=3, pad=1), _bad(base, stride=2), _bad(base, pad=1),
                _bad(base, gather_i=0), _bad(base, mode=2), _bad(base, GW=16)]
        for d in bads:
            assert not O.w1_ok(d, 1), d
            _refused(lib, rig, call([base, d]), d)
        _refused(lib, rig, call([base, base], n=0), "n = 0")
        _refused(lib, rig, call([base] * 9, q32=(1,) * 9, n=9, arr=[_parr(list(a) * 5) for a in (P, P2, Q, dW, dB)]), "n = 9")
        for k in range(3):
            off = [0, 0, 0]
            off[k] = 8
            _refused(lib, rig, call([base, base], arr=rig.arrays(tuple(off))), f"pointer {k} 8 bytes off")
        _refused(lib, rig, call([base, base], ws=None, nbytes=0), "null workspace for a split plan")
        _refused(lib, rig, call([base, base], nbytes=need - 16), "workspace 16 bytes short of what the plan writes")
        _refused(lib, rig, call([base, dict(base, mode=1 - mode, ldp=72, ldp2=72, ldq=104)]), "mixed modes")
        if mode == 1:
            _refused(lib, rig, call([base, base], q32=(1, 0)), "dbias with bf16 dY")
            assert call([base, base], q32=(1, 0), arr=(P, P2, Q, dW, _parr([rig.dB[0].ptr, None]))) == 0, lib.mi_last_error()
        else:
            _refused(lib, rig, call([base, base], q32=(1, 0)), "bf16 dY in exact-fp32 mode")
            assert call([base, base], nbytes=need) == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        assert not rig.dW[0].untouched() and not rig.dW[1].untouched() and not rig.dB[0].untouched()
    run_w1(lib, O.W1_CASES[0], "int")
    run_w1(lib, [c for c in O.W1_CASES if c.name == "mix_b37"][0], "int")


def test_refusals_s2():
    lib = _lib()
    base = O.ds2(2, 6, 32, 64, 96, 3, 1)                  # 6 k-slices
    assert O.s2_plan([base])["ws_floats"] > 0
    rig = Rig(2, BF, BF)
    P, _, Q, dW, _ = rig.arrays()
    need = O.s2_plan([base, base])["ws_need"]

    def call(ds, n=None, arr=(P, Q, dW), ws=rig.ws.ptr, nbytes=rig.ws.nbytes):
        return lib.mi_conv_s2_wgrad_tr_batch(len(ds) if n is None else n, _cdescs(ds), *arr, ws, nbytes, _stream())
    bads = [_bad(base, DW=64), _bad(base, DW=4), _bad(base, DH=5), _bad(base, N=1, DH=1, DW=32), _bad(base, Ci=96), _bad(base, Cj=48), _bad(base, Cj=16), _bad(base, I1=0),
            _bad(base, ldp=base["ldp"] + 4), _bad(base, ldq=base["ldq"] + 4), _bad(base, KH=4, KW=4), _bad(base, KH=3, KW=4), _bad(base, gather_i=0),
            _bad(base, stride=1), _bad(base, pad=0), _bad(base, mode=0), _bad(base, GH=6)]
    for d in bads:
        assert not O.s2_ok(d), d
        _refused(lib, rig, call([base, d]), d)
    _refused(lib, rig, call([base, base], n=0), "n = 0")
    _refused(lib, rig, call([base] * 9, n=9, arr=[_parr(list(a) * 5) for a in (P, Q, dW)]), "n = 9")
    for k in (0, 2):
        off = [0, 0, 0]
        off[k] = 8
        a = rig.arrays(tuple(off))
        _refused(lib, rig, call([base, base], arr=(a[0], a[2], a[3])), f"pointer {k} 8 bytes off")
    _refused(lib, rig, call([base, base], ws=None, nbytes=0), "null workspace for a split plan")
    _refused(lib, rig, call([base, base], nbytes=need - 16), "workspace 16 bytes short of what the plan writes")
    assert call([base, base], nbytes=need) == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    assert not rig.dW[0].untouched() and not rig.dW[1].untouched()
    run_s2(lib, O.S2_CASES[0], "int")
    run_s2(lib, [c for c in O.S2_CASES if c.name == "batch3"][0], "int")


def test_refusals_s2_f32():
    lib = _lib()
    # 64 steps: the second tap group (4 taps, 64 k-slices each) needs more workspace than the first (5 taps, 32 each) -- a call that is
    # refused for the second group's sake must not have run the first
    base = O.s2f_desc([c for c in O.S2F_CASES if c.name == "n64_8x8_k3_g1"][0])
    plan = O.s2f_plan(base)
    assert plan["groups"][1]["ws_floats"] > plan["groups"][0]["ws_floats"] > 0
    rig = Rig(1, F32, F32, elems=1 << 21)
    need = plan["ws_need"]

    def call(d, P=rig.P[0].ptr, Q=rig.Q[0].ptr, ws=rig.ws.ptr, nbytes=rig.ws.nbytes):
        return lib.mi_conv_s2_wgrad_f32(ctypes.byref(_cdescs([d])[0]), P, Q, rig.dW[0].ptr, ws, nbytes, _stream())
    bads = [_bad(base, DH=6), _bad(base, DW=12), _bad(base, N=1, DH=4, DW=8), _bad(base, Ci=96), _bad(base, Cj=48), _bad(base, Cj=16), _bad(base, I1=0),
            _bad(base, ldp=base["ldp"] + 2), _bad(base, ldq=base["ldq"] + 2), _bad(base, KH=5, KW=5), _bad(base, KH=3, KW=4), _bad(base, stride=1), _bad(base, pad=0),
            _bad(base, mode=1), _bad(base, GH=8)]
    for d in bads:
        assert not O.s2f_ok(d), d
        _refused(lib, rig, call(d), d)
    _refused(lib, rig, call(base, P=rig.P[0].ptr + 8), "P 8 bytes off")
    _refused(lib, rig, call(base, Q=rig.Q[0].ptr + 8), "Q 8 bytes off")
    _refused(lib, rig, call(base, ws=None, nbytes=0), "null workspace for a split plan")
    _refused(lib, rig, call(base, nbytes=need - 16), "workspace 16 bytes short of what the second tap group writes")
    assert call(base, nbytes=need) == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    assert not rig.dW[0].untouched()
    run_s2f(lib, O.S2F_CASES[0], "int")                   # (the plan above runs for its values as O.S2F_CASES' n64_8x8_k3_g1)
