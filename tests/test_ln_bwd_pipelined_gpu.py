"""chan_ln_bwd_pipe_kernel: the channel LayerNorm's backward with U pixel groups of a wave in flight -- through the C ABI, against the
guarded kernel it replaces (mi_debug_ln_bwd_pipeline(0), bit for bit) and against the float64 restatement of tests/_norm_oracle.py.

Shapes: the smallest that reach every edge of the unrolled loop under the real cap of 512 workgroups, for U = 2 AND U = 4 at every width,
so that the edges stay covered whichever of the two ln_bwd_go instantiates for a width.  C = 128 (two pixels per wave, 8 per workgroup
and iteration, 4 096 per pass of the grid): M = 1 and 9 (single-group body only, dead lanes), 4 096 U + 5 (exactly one unrolled iteration
for the first waves, none for the others, a ragged last group), 4 096 (U + 1) + 13 (an unrolled iteration and then the single-group
remainder).  C = 256 and 512 (one pixel per wave, 2 048 per pass; one and two float4 per lane): M = 3, 2 048 U + 2, 2 048 (U + 1) + 7.
The largest tensor is 10 247 x (512 + 16) floats = 21.6 MB.

Every shape with fp32 and bf16 dy; dx written, accumulated in place and accumulated out of place (mi_chan_layernorm_bwd_out, dx_in in a
NaN-padded buffer and intact afterwards); dense and with four different pitches; parameter gradients as partial rows and as atomics onto
non-zero dg / db.  Inputs are views between NaN with NaN in their pitch padding, dx has a sentinel in its padding and behind it.

Checks: mi_chan_layernorm_bwd_pipelined is 1 for each of these launches; every launch runs twice, dx and the partial rows bit-equal; the
same launch with the hook off: dx (both variants) and the partial rows bit-equal, which is the claim that no sum changed its order; the
atomically added dg / db, whose order was never fixed, to 1e-5 of the float64 sum of the partial rows (tests/test_ln_bwd_out_of_place_gpu.py's
bound); against the float64 oracle the bounds of tests/test_norm_kernels_gpu.py: dx (the two sigma == 0 pixels measured apart), dg, db
<= 5e-5 rel-L2, the same for an fp32 dx from bf16 dy.  C = 132, 260 and 1 024, and a pointer 8 bytes off (4 for bf16 dy, whose rows need 8):
the query is 0 and the launch runs on the guarded kernel to the same bounds.  The hook is restored after every test."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _norm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -776.0
PAD = 64                              # elements of NaN in front of and behind an input
BF, F32 = torch.bfloat16, torch.float32
US = (2, 4)                           # pixel groups in flight: the edge shapes of both, at every width
PITCH = dict(x=4, dy=12, dx=16, dxin=8)
MODES = ["write", "inplace", "out"]


def _shapes():
    out = [(1, 128), (9, 128)] + [(M, 128) for U in US for M in (4096 * U + 5, 4096 * (U + 1) + 13)]
    for C in (256, 512):
        out += [(3, C)] + [(M, C) for U in US for M in (2048 * U + 2, 2048 * (U + 1) + 7)]
    return out


PARAMS = [pytest.param(case, dy16, mode, pitched, id=f"{case[0]}x{case[1]}-{'dy16' if dy16 else 'dy32'}-{mode}-{'pitched' if pitched else 'dense'}")
          for case in _shapes() for dy16 in (False, True) for mode in MODES for pitched in (False, True)]


def _lib():
    from src.ops.lib import load_library
    return load_library()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture
def hook():
    """mi_debug_ln_bwd_pipeline, put back to what it was."""
    lib = _lib()
    was = lib.mi_debug_ln_bwd_pipeline(1)
    try:
        yield lib
    finally:
        lib.mi_debug_ln_bwd_pipeline(was)


class In:
    """Rows of t [R][C] at pitch ld inside a NaN-filled buffer, `shift` elements off the 16-byte aligned position."""

    def __init__(self, t, ld=None, dtype=F32, shift=0):
        t = t.reshape(-1, t.shape[-1])
        R, C = t.shape
        self.ld = ld or C
        self.buf = torch.full((2 * PAD + R * self.ld,), float("nan"), dtype=dtype, device=DEV)
        self.rows = self.buf[PAD + shift:PAD + shift + R * self.ld].view(R, self.ld)
        self.rows[:, :C].copy_(t.to(dtype))
        self.buf0 = self.buf.clone()
        assert self.rows.data_ptr() % 16 == shift * self.buf.element_size()
        self.ptr = ctypes.c_void_p(self.rows.data_ptr())

    def intact(self):
        return torch.equal(self.buf.view(torch.int16), self.buf0.view(torch.int16))


class Out:
    """R rows of C floats at pitch ld in a sentinel-filled buffer with a sentinel tail, `shift` floats off the aligned position."""

    def __init__(self, R, C, ld=None, init=None, shift=0):
        self.R, self.C, self.ld, self.off = R, C, ld or C, PAD + shift
        self.buf = torch.full((self.off + R * self.ld + 256,), SENT, dtype=F32, device=DEV)
        self.rows = self.buf[self.off:self.off + R * self.ld].view(R, self.ld)
        if init is not None:
            self.rows[:, :C].copy_(init.reshape(R, C).to(F32))
        self.ptr = ctypes.c_void_p(self.rows.data_ptr())

    def get(self):
        assert bool((self.buf[:self.off] == SENT).all()) and bool((self.buf[self.off + self.R * self.ld:] == SENT).all()), "written outside"
        assert bool((self.rows[:, self.C:] == SENT).all()), "pitch padding written"
        got = self.rows[:, :self.C]
        assert bool(torch.isfinite(got).all()), "NaN in an output: a padding or a dead row was read into it"
        return got


@functools.lru_cache(maxsize=2)
def _reference(case, dy16):
    """The inputs of a case on the GPU (float64, holding the stored values) and the float64 gradients, once for all its variants."""
    inp = {k: v.to(DEV) for k, v in O.ln_inputs(case, bf16_dy=dy16).items()}
    return inp, O.ln_grads_ref(inp["x"], inp["g"], O.LN_EPS, inp["dy"])


def _launch(lib, case, inp, dy16, mode, pitched, kind, shift=None):
    """One launch on fresh buffers.  kind: 'part' or 'atomic'.  -> dict(dx buffer, part | dg, db, query)."""
    M, C = case
    shift = shift or {}
    ld = {k: C + (PITCH[k] if pitched else 0) for k in PITCH}
    x, g = In(inp["x"], ld["x"], shift=shift.get("x", 0)), In(inp["g"][None])
    dy = In(inp["dy"], ld["dy"], BF if dy16 else F32, shift=shift.get("dy", 0))
    dx = Out(M, C, ld["dx"], init=inp["prev"] if mode == "inplace" else None, shift=shift.get("dx", 0))
    dxin = In(inp["prev"], ld["dxin"], shift=shift.get("dxin", 0)) if mode == "out" else None
    rows = lib.mi_chan_layernorm_bwd_part_rows(M, C)
    part = Out(rows + 2, 2 * C) if kind == "part" else None
    dg, db = (Out(1, C, init=torch.full((C,), 0.25)), Out(1, C, init=torch.full((C,), -0.5))) if kind == "atomic" else (None, None)
    head = (M, C, x.ptr, x.ld, g.ptr, O.LN_EPS, dy.ptr, dy.ld)
    acc_from = dxin.ptr if mode == "out" else dx.ptr if mode == "inplace" else None
    query = lib.mi_chan_layernorm_bwd_pipelined(C, x.ptr, dy.ptr, dx.ptr, acc_from, x.ld, dy.ld, dx.ld, dxin.ld if dxin else dx.ld, int(dy16))
    if mode == "out":
        rc = lib.mi_chan_layernorm_bwd_out(*head, dxin.ptr, dxin.ld, dx.ptr, dx.ld, dg.ptr if dg else None, db.ptr if db else None,
                                           part.ptr if part else None, int(dy16), _stream())
    elif kind == "part":
        rc = lib.mi_chan_layernorm_bwd_part(*head, dx.ptr, dx.ld, int(mode == "inplace"), part.ptr, int(dy16), _stream())
    else:
        rc = lib.mi_chan_layernorm_bwd_io(*head, dx.ptr, dx.ld, int(mode == "inplace"), dg.ptr, db.ptr, int(dy16), _stream())
    assert rc == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    assert x.intact() and dy.intact() and g.intact() and (dxin is None or dxin.intact()), "an input was written"
    r = dict(dx=dx.get().clone(), query=query, rows=rows)
    if part:
        p = part.get()
        assert bool((p[:rows] != SENT).all()) and bool((p[rows:] == SENT).all()), "partial rows: not every row, or one too many"
        r["part"] = p[:rows].clone()
    else:
        r.update(dg=dg.get().view(C).double() - 0.25, db=db.get().view(C).double() + 0.5)
    return r


def _check(lib, case, dy16, mode, pitched, want_query, shift=None):
    M, C = case
    inp, (dxr, dgr, dbr) = _reference(case, dy16)
    tag = f"{case} {'dy16' if dy16 else 'dy32'} {mode} {'pitched' if pitched else 'dense'} {shift or ''}"
    go = functools.partial(_launch, lib, case, inp, dy16, mode, pitched, shift=shift)
    lib.mi_debug_ln_bwd_pipeline(1)
    p1, p2, a1 = go("part"), go("part"), go("atomic")
    assert p1["query"] == want_query and a1["query"] == want_query, (tag, p1["query"], a1["query"])
    lib.mi_debug_ln_bwd_pipeline(0)
    p0, a0 = go("part"), go("atomic")
    assert p0["query"] == 0 and a0["query"] == 0, "the query ignores the hook"
    lib.mi_debug_ln_bwd_pipeline(1)

    bits = lambda t: t.contiguous().view(torch.int32)      # noqa: E731
    assert torch.equal(bits(p1["dx"]), bits(p2["dx"])) and torch.equal(bits(p1["part"]), bits(p2["part"])), f"{tag}: not reproducible"
    assert torch.equal(bits(p1["dx"]), bits(p0["dx"])), f"{tag}: dx differs from the guarded kernel's"
    assert torch.equal(bits(p1["part"]), bits(p0["part"])), f"{tag}: partial rows of dg / db differ from the guarded kernel's"
    assert torch.equal(bits(a1["dx"]), bits(p1["dx"])) and torch.equal(bits(a0["dx"]), bits(p1["dx"])), f"{tag}: dx of the atomics variant differs"

    dg64, db64 = p1["part"][:, :C].double().sum(0), p1["part"][:, C:].double().sum(0)
    for name, a in (("on", a1), ("off", a0)):
        for k, want in (("dg", dg64), ("db", db64)):
            err = float((a[k] - want).norm() / want.norm().clamp_min(1e-30))
            assert err <= 1e-5, (tag, name, k, err)

    got = p1["dx"].double() - (inp["prev"] if mode != "write" else 0.0)
    mid, ends = slice(1, M - 1), [0, M - 1]
    e = dict(dx=O.rel(got[mid], dxr[mid]), dx_ends=O.rel(got[ends], dxr[ends]), dg=O.rel(dg64, dgr), db=O.rel(db64, dbr),
             dg_atomic=O.rel(a1["dg"], dgr), db_atomic=O.rel(a1["db"], dbr))
    print(f"LayerNorm backward {tag}: " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))
    assert max(e.values()) <= 5e-5, (tag, e)


@pytest.mark.parametrize("case,dy16,mode,pitched", PARAMS)
def test_pipelined_is_the_guarded_kernel_bit_for_bit(hook, case, dy16, mode, pitched):
    _check(hook, case, dy16, mode, pitched, want_query=1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dy16", [False, True], ids=["dy32", "dy16"])
@pytest.mark.parametrize("case", [(257, 132), (2051, 260), (37, 1024)], ids=lambda c: "x".join(map(str, c)))
def test_other_widths_stay_on_the_guarded_kernel(hook, case, dy16, mode):
    _check(hook, case, dy16, mode, True, want_query=0)


@pytest.mark.parametrize("which,dy16,mode", [("x", False, "write"), ("dx", True, "inplace"), ("dxin", True, "out"), ("dy", False, "out"),
                                             ("dy", True, "write")])
@pytest.mark.parametrize("case", [(4096 * 4 + 5, 128), (2048 * 4 + 2, 512)], ids=lambda c: "x".join(map(str, c)))
def test_misaligned_pointer_stays_on_the_guarded_kernel(hook, case, which, dy16, mode):
    """One pointer 8 bytes off 16-byte alignment (bf16 dy: 4 bytes off, its rows need 8)."""
    _check(hook, case, dy16, mode, True, want_query=0, shift={which: 2})
    _check(hook, case, dy16, mode, True, want_query=1)


def test_hook_returns_the_previous_value(hook):
    assert hook.mi_debug_ln_bwd_pipeline(0) == 1 and hook.mi_debug_ln_bwd_pipeline(1) == 0 and hook.mi_debug_ln_bwd_pipeline(1) == 1
