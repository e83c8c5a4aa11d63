"""Store mode of the LDS-DMA weight-gradient kernels (csrc/wgrad_tr.hip, wgrad1x1_tr.hip, wgrad_s2_tr.hip: mi_conv3x3_wgrad_tr_batch_ex,
mi_conv1x1_wgrad_tr_batch_ex, mi_conv_s2_wgrad_tr_batch_ex with MI_WGRAD_STORE) and mi_zero_ranges (csrc/elementwise.hip), on the
MI355X through the C ABI.

Every case of tests/_wgrad_oracle.py's TR_CASES, W1_CASES and S2_CASES (the shapes tests/test_wgrad_tr_kernels_gpu.py runs, whose
buffer rig this file borrows): a case its *_supported query refuses FAILS.  They include the smallest plans (one step, one tile: the
direct store of a layer without k-slices), ragged Cj, and k-slices forced through the blocks hooks (both reduce instantiations, every
tail length).  Integer operands only -- every product and partial sum is exact in fp32 and in bf16 storage -- so there is no tolerance
anywhere in this file.

dW starts as NaN between sentinels.  The result must be torch.equal to the float64 reference cast to fp32 (one NaN left, or one
element added to instead of written, fails), bit-equal after `+ 0.0` to the plain entry point run on a zeroed dW (a stored -0.0 against
an accumulated +0.0 is the one permitted difference), bit-equal between two runs, and the sentinels in front of and behind dW and
around the workspace must survive.  dbias (1x1) is still added into its non-zero start.  flags = 0 through the _ex entry point is the
accumulating call; an unknown flag bit is refused before anything is written."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wgrad_oracle as O  # noqa: E402
from test_wgrad_tr_kernels_gpu import BF, DEV, F32, F64, NAN, SENT, In, Out, Ws, _cdescs, _lib, _parr, _s2_shapes, _seed, _stream, _ws_bytes  # noqa: E402

pytestmark = pytest.mark.gpu
STORE = 1
I32 = torch.int32


def _bits(t):
    return (t + 0.0).view(I32)


class Prep:
    """Operands (integer-valued), float64 references and the launcher of one case of the oracle's lists."""

    def __init__(self, kind, c):
        lib = _lib()
        self.kind, self.c, self.tag = kind, c, f"{kind}:{c.name}"
        self.q32 = None
        L = []
        if kind == "tr":
            self.descs = O.tr_descs(c)
            dt = BF if c.mode else F32
            for i, (l, d) in enumerate(zip(c.layers, self.descs)):
                N, H, W, Ci, Cj = l[:5]
                x, dy = O.operands((N, H, W, Ci), (N, H, W, Cj), "int", _seed(c.name, i, "store"), True, True)
                I1 = d["I1"]
                L.append(dict(P=In(x[..., :I1], d["ldp"], dt), P2=In(x[..., I1:], d["ldp2"], dt) if I1 != Ci else None, Q=In(dy, d["ldq"], dt),
                              grad=O.wgrad3x3_ref(x, dy), n=9 * Ci * Cj))
            self.plan = O.tr_plan(self.descs, c.blocks)
            self.hook = lib.mi_debug_wgrad_tr_blocks
        elif kind == "w1":
            self.descs, self.q32 = O.w1_descs(c)
            xdt = BF if c.mode else F32
            for i, (l, d) in enumerate(zip(c.layers, self.descs)):
                k, Ci, Cj, I1, q, bias = l
                x, dy = O.operands((64 * k, Ci), (64 * k, Cj), "int", _seed(c.name, i, "store"), True, True)
                grad, db = O.wgrad1x1_ref(x, dy)
                L.append(dict(P=In(x[:, :I1], d["ldp"], xdt), P2=In(x[:, I1:], d["ldp2"], xdt) if I1 != Ci else None, Q=In(dy, d["ldq"], F32 if q else BF),
                              grad=grad, db=db, bias=bias, binit=O.init_content(Cj) + 1, n=Ci * Cj))
            self.plan = O.w1_plan(self.descs, self.q32, c.blocks)
            self.hook = lib.mi_debug_wgrad1x1_tr_blocks
        else:
            self.descs = O.s2_descs(c)
            for i, (l, d) in enumerate(zip(c.layers, self.descs)):
                N, h, w, Ci, Cj, ks = l
                p, q = O.operands(*_s2_shapes(N, h, w, Ci, Cj, d["gather_i"]), "int", _seed(c.name, i, "store"), True, True)
                L.append(dict(P=In(p, d["ldp"], BF), P2=None, Q=In(q, d["ldq"], BF), grad=O.wgrad_s2_ref(p, q, ks, d["gather_i"]), n=ks * ks * Ci * Cj))
            self.plan = O.s2_plan(self.descs)
            self.hook = None
        self.L, self.n = L, len(L)
        self.cd = _cdescs(self.descs)
        self.cq = (ctypes.c_int * self.n)(*self.q32) if self.q32 is not None else None
        for i, d in enumerate(self.descs):          # the shapes the kernels already run: refused is a failure, never a skip
            ok = (lib.mi_conv3x3_wgrad_tr_supported(ctypes.byref(self.cd[i])) if kind == "tr" else
                  lib.mi_conv1x1_wgrad_tr_supported(ctypes.byref(self.cd[i]), self.q32[i]) if kind == "w1" else
                  lib.mi_conv_s2_wgrad_tr_supported(ctypes.byref(self.cd[i])))
            assert ok == 1, (self.tag, i, "refused by *_supported")
        self.split = [a["splits"] > 1 for a in self.plan["layers"]]

    def run(self, flags, init):
        """One launch on fresh result buffers; flags None: the entry point without flags.  init: a float, or None for the oracle's small
        integers.  -> (dW Outs, dbias Outs or Nones, the workspace); not synchronised."""
        lib, L, n, cd = _lib(), self.L, self.n, self.cd
        start = (lambda m: O.init_content(m)) if init is None else (lambda m: torch.full((m,), init, dtype=F64))
        dW = [Out(start(a["n"])) for a in L]
        dB = [Out(a["binit"]) if a.get("bias") else None for a in L]
        try:
            if self.hook is not None:
                self.hook(self.c.blocks)
            reported = (lib.mi_conv3x3_wgrad_tr_batch_workspace(n, cd) if self.kind == "tr" else
                        lib.mi_conv1x1_wgrad_tr_batch_workspace(n, cd, self.cq) if self.kind == "w1" else lib.mi_conv_s2_wgrad_tr_batch_workspace(n, cd))
            ws = Ws(_ws_bytes(reported, self.plan))
            P, P2, Q = _parr([a["P"].ptr for a in L]), _parr([a["P2"].ptr if a["P2"] else None for a in L]), _parr([a["Q"].ptr for a in L])
            pW, pB = _parr([o.ptr for o in dW]), _parr([o.ptr if o else None for o in dB])
            tail = () if flags is None else (flags,)
            sfx = "" if flags is None else "_ex"
            if self.kind == "tr":
                rc = getattr(lib, "mi_conv3x3_wgrad_tr_batch" + sfx)(n, cd, P, P2, Q, pW, ws.ptr, ws.nbytes, _stream(), *tail)
            elif self.kind == "w1":
                rc = getattr(lib, "mi_conv1x1_wgrad_tr_batch" + sfx)(n, cd, self.cq, P, P2, Q, pW, pB, ws.ptr, ws.nbytes, _stream(), *tail)
            else:
                rc = getattr(lib, "mi_conv_s2_wgrad_tr_batch" + sfx)(n, cd, P, Q, pW, ws.ptr, ws.nbytes, _stream(), *tail)
        finally:
            if self.hook is not None:
                self.hook(0)
        assert rc == 0, (self.tag, lib.mi_last_error())
        return dW, dB, ws

    def intact(self):
        return all(a["P"].intact() and a["Q"].intact() and (a["P2"] is None or a["P2"].intact()) for a in self.L)


def _finish(dW, dB, ws):
    torch.cuda.synchronize()
    ws.check()
    return [o.get() for o in dW], [o.get() if o else None for o in dB]


# ---------------------------------------------------------------------------------------------------- store mode
def run_store(kind, c):
    p = Prep(kind, c)
    a1, b1 = _finish(*p.run(STORE, NAN))
    a2, _ = _finish(*p.run(STORE, NAN))
    old, _ = _finish(*p.run(None, 0.0))
    ex0, _ = _finish(*p.run(0, None))                # flags = 0: the accumulating call, onto the oracle's non-zero start
    for i, (a, g, g2, o) in enumerate(zip(p.L, a1, a2, old)):
        ref = a["grad"].reshape(-1).to(F32)
        bad = (g != ref).nonzero().flatten()       # (NaN != anything)
        assert bad.numel() == 0, (p.tag, i, f"{bad.numel()} wrong elements, first at {int(bad[0])}: {float(g[bad[0]])} != {float(ref[bad[0]])}")
        assert torch.equal(g, ref)
        assert torch.equal(g.view(I32), g2.view(I32)), (p.tag, i, "two store runs differ")
        assert torch.equal(_bits(g), _bits(o)), (p.tag, i, "store differs from the accumulating entry point on a zeroed dW")
        assert torch.equal(ex0[i], (O.init_content(a["n"]) + a["grad"].reshape(-1)).to(F32)), (p.tag, i, "flags = 0 does not accumulate")
        if a.get("bias"):
            assert torch.equal(b1[i], (a["binit"] + a["db"]).to(F32)), (p.tag, i, "dbias is still added")
    assert p.intact()


@pytest.mark.parametrize("case", O.TR_CASES, ids=repr)
def test_store_3x3(case):
    run_store("tr", case)


@pytest.mark.parametrize("case", O.W1_CASES, ids=repr)
def test_store_1x1(case):
    run_store("w1", case)


@pytest.mark.parametrize("case", O.S2_CASES, ids=repr)
def test_store_s2(case):
    run_store("s2", case)


# ---------------------------------------------------------------------------------------------------- refusals
def _case(cases, name):
    return [c for c in cases if c.name == name][0]


def test_unknown_flag_bits_are_refused():
    lib = _lib()
    for kind, cases, name in (("tr", O.TR_CASES, "splits9-bf16"), ("w1", O.W1_CASES, "splits9"), ("s2", O.S2_CASES, "splits13_k3")):
        p = Prep(kind, _case(cases, name))
        L, n, cd = p.L, p.n, p.cd
        dW, ws = [Out(O.init_content(a["n"])) for a in L], Ws(p.plan["ws_bytes"])
        dB = [Out(a["binit"]) if a.get("bias") else None for a in L]
        P, P2, Q = _parr([a["P"].ptr for a in L]), _parr([None for a in L]), _parr([a["Q"].ptr for a in L])
        pW, pB = _parr([o.ptr for o in dW]), _parr([o.ptr if o else None for o in dB])
        for bad in (2, 8, STORE | 2, STORE | 16, 1 << 31):
            if kind == "tr":
                rc = lib.mi_conv3x3_wgrad_tr_batch_ex(n, cd, P, P2, Q, pW, ws.ptr, ws.nbytes, _stream(), bad)
            elif kind == "w1":
                rc = lib.mi_conv1x1_wgrad_tr_batch_ex(n, cd, p.cq, P, P2, Q, pW, pB, ws.ptr, ws.nbytes, _stream(), bad)
            else:
                rc = lib.mi_conv_s2_wgrad_tr_batch_ex(n, cd, P, Q, pW, ws.ptr, ws.nbytes, _stream(), bad)
            torch.cuda.synchronize()
            assert rc != 0 and lib.mi_last_error(), (kind, bad)
            assert all(o.untouched() for o in dW) and ws.untouched() and all(o.untouched() for o in dB if o), (kind, bad, "refused but wrote")
        run_store(kind, p.c)                             # a valid call after the refusals gives the exact result


# ---------------------------------------------------------------------------------------------------- mi_zero_ranges
@pytest.mark.parametrize("shift", [0, 1, 3])
def test_zero_ranges(shift):
    """(offset, count) ranges of every alignment, 0-length ones, one longer than a sweep of the grid (8 x 256 float4), one range alone;
    every float between the ranges, in front of the base and in the tail keeps its sentinel.  shift: base 4 * shift bytes off 16."""
    lib = _lib()
    ranges = [(0, 1), (2, 0), (3, 2), (7, 5), (13, 4), (32, 64), (97, 0), (101, 1000), (1101, 3), (2000, 40000), (42001, 1), (42010, 8193), (60000, 0)]
    n_all = 60000 + 300
    buf = torch.full((64 + n_all,), SENT, dtype=F32, device=DEV)
    base = buf[60 + shift:]
    assert base.data_ptr() % 16 == (4 * ((60 + shift) % 4)) % 16
    table = torch.tensor(ranges, dtype=torch.int64, device=DEV)
    for sel in (ranges[7:8], ranges):
        buf.fill_(SENT)
        t = table if sel is ranges else torch.tensor(sel, dtype=torch.int64, device=DEV)
        assert lib.mi_zero_ranges(t.data_ptr(), len(sel), base.data_ptr(), _stream()) == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        want = torch.full((64 + n_all,), SENT, dtype=F32)
        for off, cnt in sel:
            want[60 + shift + off:60 + shift + off + cnt] = 0.0
        assert torch.equal(buf.cpu(), want), (shift, len(sel))
    buf.fill_(SENT)
    assert lib.mi_zero_ranges(None, 3, base.data_ptr(), _stream()) != 0 and lib.mi_zero_ranges(table.data_ptr(), 0, base.data_ptr(), _stream()) != 0
    assert lib.mi_zero_ranges(table.data_ptr(), 3, None, _stream()) != 0
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
