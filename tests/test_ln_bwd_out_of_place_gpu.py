"""mi_chan_layernorm_bwd_out: the channel LayerNorm's backward with dx_out = dx_in + gradient, dx_in read only -- through the C ABI,
against the accumulating in-place call (mi_chan_layernorm_bwd_io / _part, accumulate = 1) on a copy of dx_in.

Every shape with fp32 and bf16 dy and two pitches; dx_in sits in a NaN-padded buffer (a read past a row's C floats, or past the last
row, puts a NaN into the result), dx_out's rows are padded with and followed by a sentinel.  dx and the partial rows of dg / db (fixed
order) are compared bit for bit; the atomically added dg / db are bit-equal where one workgroup runs and otherwise held to 1e-5 of the
float64 sum of the partial rows (fp32 atomics in a varying order: a few ulp of the largest term over <= 512 addends).
Shapes: 5 x 4 (one wave, dead lanes), 257 x 132 (the 64-lane form, a ragged last workgroup), 2 051 x 260 (more pixels than one
pass of the capped grid covers: the pixel loop), 1 024 x 128 (the two-pixels-per-wave form at its widest)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -777.25
EPS = 1e-5
CASES = [(5, 4), (257, 132), (2051, 260), (1024, 128)]
PITCHES = [0, 12]                     # extra floats / elements per row (0: dense)


def _lib():
    from src.ops.lib import load_library
    return load_library()


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(M, Cc, pad, dy16):
    g = torch.Generator().manual_seed(1000 * M + Cc + pad)
    ld = Cc + pad
    x = torch.randn(M, ld, generator=g)
    x[0, :Cc] = 0.5                                     # sigma == 0 in the first and in the last pixel
    x[M - 1, :Cc] = -2.0
    gam = torch.randn(Cc, generator=g)
    dy = torch.randn(M, ld, generator=g)
    dxin = torch.full((M + 2, ld), float("nan"))        # one NaN row in front and behind, NaN padding in every row
    dxin[1:M + 1, :Cc] = torch.randn(M, Cc, generator=g)
    return (x.to(DEV), gam.to(DEV), dy.to(DEV, torch.bfloat16 if dy16 else torch.float32), dxin.to(DEV))


def _out(M, ld):
    return torch.full((M * ld + 64,), SENT, device=DEV)


@pytest.mark.parametrize("pad", PITCHES, ids=lambda p: f"pitch+{p}")
@pytest.mark.parametrize("dy16", [False, True], ids=["dy32", "dy16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_out_of_place_matches_in_place(case, dy16, pad):
    lib = _lib()
    M, Cc = case
    ld = Cc + pad
    ldo = Cc + (0 if pad == 0 else 20)                  # dx_out's pitch differs from dx_in's in the pitched case
    x, gam, dy, dxin = _inputs(M, Cc, pad, dy16)
    dxin0 = dxin.clone()
    rows = lib.mi_chan_layernorm_bwd_part_rows(M, Cc)
    assert rows >= 1
    head = (M, Cc, _ptr(x), ld, _ptr(gam), EPS, _ptr(dy), ld)

    # ---- the in-place reference: dx_in's values copied into a buffer of dx_out's layout, accumulate = 1
    def ref_buffer():
        r = _out(M, ldo)
        r[:M * ldo].view(M, ldo)[:, :Cc] = dxin0[1:M + 1, :Cc]
        return r
    ref_p, part_ref = ref_buffer(), torch.full((rows + 2, 2 * Cc), SENT, device=DEV)
    assert lib.mi_chan_layernorm_bwd_part(*head, _ptr(ref_p), ldo, 1, _ptr(part_ref), int(dy16), _stream()) == 0, lib.mi_last_error()
    ref_a, dg_ref, db_ref = ref_buffer(), torch.full((Cc,), 0.25, device=DEV), torch.full((Cc,), -0.5, device=DEV)
    assert lib.mi_chan_layernorm_bwd_io(*head, _ptr(ref_a), ldo, 1, _ptr(dg_ref), _ptr(db_ref), int(dy16), _stream()) == 0, lib.mi_last_error()

    # ---- out of place, partial rows
    out_p, part = _out(M, ldo), torch.full((rows + 2, 2 * Cc), SENT, device=DEV)
    rc = lib.mi_chan_layernorm_bwd_out(*head, _ptr(dxin, 4 * ld), ld, _ptr(out_p), ldo, None, None, _ptr(part), int(dy16), _stream())
    assert rc == 0, lib.mi_last_error()
    # ---- out of place, atomics
    out_a, dg, db = _out(M, ldo), torch.full((Cc,), 0.25, device=DEV), torch.full((Cc,), -0.5, device=DEV)
    rc = lib.mi_chan_layernorm_bwd_out(*head, _ptr(dxin, 4 * ld), ld, _ptr(out_a), ldo, _ptr(dg), _ptr(db), None, int(dy16), _stream())
    assert rc == 0, lib.mi_last_error()
    torch.cuda.synchronize()

    assert torch.equal(_bits(dxin), _bits(dxin0)), "dx_in was written"
    for tag, got, ref in (("part", out_p, ref_p), ("atomic", out_a, ref_a)):
        assert torch.equal(_bits(got), _bits(ref)), f"{tag}: dx_out differs from the in-place call (or a pad / sentinel was written)"
        body = got[:M * ldo].view(M, ldo)
        assert bool(torch.isfinite(body[:, :Cc]).all()), f"{tag}: NaN in dx_out: dx_in's padding was read"
        assert bool((body[:, Cc:] == SENT).all()) and bool((got[M * ldo:] == SENT).all()), f"{tag}: written outside dx_out's rows"
    assert torch.equal(_bits(part), _bits(part_ref)), "partial rows of dg / db differ from the in-place call"
    assert bool((part[rows:] == SENT).all()) and bool((part[:rows] != SENT).all())
    dg64, db64 = part[:rows, :Cc].double().sum(0), part[:rows, Cc:].double().sum(0)
    for tag, got, ref, init, want in (("dg", dg, dg_ref, 0.25, dg64), ("db", db, db_ref, -0.5, db64)):
        if rows == 1:
            assert torch.equal(_bits(got), _bits(ref)), f"{tag}: one workgroup, yet not the in-place call's bits"
        for v in (got, ref):
            err = float(((v.double() - init) - want).norm() / want.norm().clamp_min(1e-30))
            assert err <= 1e-5, (tag, err)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_same_pointer_is_the_in_place_call(case):
    lib = _lib()
    M, Cc = case
    x, gam, dy, dxin = _inputs(M, Cc, 0, False)
    rows = lib.mi_chan_layernorm_bwd_part_rows(M, Cc)
    head = (M, Cc, _ptr(x), Cc, _ptr(gam), EPS, _ptr(dy), Cc)
    a, b = dxin[1:M + 1].clone(), dxin[1:M + 1].clone()
    pa, pb = torch.empty(rows, 2 * Cc, device=DEV), torch.empty(rows, 2 * Cc, device=DEV)
    assert lib.mi_chan_layernorm_bwd_part(*head, _ptr(a), Cc, 1, _ptr(pa), 0, _stream()) == 0, lib.mi_last_error()
    assert lib.mi_chan_layernorm_bwd_out(*head, _ptr(b), Cc, _ptr(b), Cc, None, None, _ptr(pb), 0, _stream()) == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(pa), _bits(pb))
    assert bool(torch.isfinite(b).all())


@pytest.mark.parametrize("dy16", [False, True], ids=["dy32", "dy16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_overlap_is_refused(case, dy16):
    """dx_in / dx_out ranges that overlap without being the same pointer: refused before anything is launched."""
    lib = _lib()
    M, Cc = case
    x, gam, dy, _ = _inputs(M, Cc, 0, dy16)
    rows = lib.mi_chan_layernorm_bwd_part_rows(M, Cc)
    head = (M, Cc, _ptr(x), Cc, _ptr(gam), EPS, _ptr(dy), Cc)
    buf = torch.arange(2 * M * Cc + 8, device=DEV, dtype=torch.float32)
    buf0 = buf.clone()
    part, dg, db = torch.full((rows, 2 * Cc), SENT, device=DEV), torch.full((Cc,), SENT, device=DEV), torch.full((Cc,), SENT, device=DEV)
    last = 4 * ((M - 1) * Cc + Cc - 4)                                  # the two ranges share their last / first 16 bytes
    for off_in, off_out in ((0, 16), (16, 0), (0, last), (last, 0), (0, 4 * Cc)):
        rc = lib.mi_chan_layernorm_bwd_out(*head, _ptr(buf, off_in), Cc, _ptr(buf, off_out), Cc, None, None, _ptr(part), int(dy16), _stream())
        assert rc != 0, (off_in, off_out)
        rc = lib.mi_chan_layernorm_bwd_out(*head, _ptr(buf, off_in), Cc, _ptr(buf, off_out), Cc, _ptr(dg), _ptr(db), None, int(dy16), _stream())
        assert rc != 0, (off_in, off_out)
    # same pointer, two pitches: not the in-place call either
    assert lib.mi_chan_layernorm_bwd_out(*head, _ptr(buf), Cc, _ptr(buf), Cc + 4, None, None, _ptr(part), int(dy16), _stream()) != 0
    torch.cuda.synchronize()
    assert torch.equal(buf, buf0) and bool((part == SENT).all()) and bool((dg == SENT).all()) and bool((db == SENT).all())
    # adjacent ranges are fine
    rc = lib.mi_chan_layernorm_bwd_out(*head, _ptr(buf), Cc, _ptr(buf, 4 * M * Cc), Cc, None, None, _ptr(part), int(dy16), _stream())
    assert rc == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf[:M * Cc], buf0[:M * Cc]) and torch.equal(buf[2 * M * Cc:], buf0[2 * M * Cc:])
