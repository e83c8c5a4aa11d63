"""tests/_igemm_oracle.py against independent facts, without a GPU: the float64 references against torch (F.conv2d, F.conv_transpose2d
and autograd's weight gradients, in float64, to 1e-12) at every geometry of the case lists and both weight layouts; the restated
planners against the library's own queries (mi_conv_igemm_plan, mi_conv_igemm_tile, mi_conv_igemm_bf16w_io_supported,
mi_conv_wgrad_plan, mi_conv_wgrad_slabs_workspace; the library loads without a device) over every case and a few thousand random
descriptors, refused ones among them; the instantiations and edges the case lists must keep reaching, computed from the plans; every
host-side refusal of igemm_conv.hip's and wgrad.hip's entry points by the text mi_last_error carries (made-up pointers: every refusal
precedes the first dereference); and the exactness condition of the integer operand families."""
import ctypes
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _igemm_oracle as O  # noqa: E402

F64 = torch.float64


def _lib():
    from src.ops.lib import load_library
    return load_library()


def _cd(d):
    from src.ops.lib import MiConvDesc
    return ctypes.byref(MiConvDesc(**d._asdict()))


def _wd(d):
    from src.ops.lib import MiWgradDesc
    return ctypes.byref(MiWgradDesc(**d._asdict()))


def _iplan(lib, d, wb, i16, al):
    from src.ops.lib import MiIgemmPlan
    p = MiIgemmPlan()
    for f, _ in p._fields_[:6]:
        setattr(p, f, -7)
    rc = lib.mi_conv_igemm_plan(_cd(d), int(wb), int(i16), int(al), ctypes.byref(p))
    if rc:
        return lib.mi_last_error().decode()
    return O.IgemmPlan(p.kernel, p.bm, p.bn, p.classes, p.ragged, p.ksplit, tuple(p.ntap), tuple(p.stages))


def _wplan(lib, d, al, slab):
    from src.ops.lib import MiWgradPlan
    p = MiWgradPlan()
    rc = lib.mi_conv_wgrad_plan(_wd(d), int(al), int(slab), ctypes.byref(p))
    if rc:
        return lib.mi_last_error().decode()
    return O.WgradPlan(p.fast, p.big, p.splits, p.chunk, p.xcd_map, p.grid)


# ---------------------------------------------------------------------------------------------------- references against torch
def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _torch_conv(d, src, W):
    """W: logical [taps][K][Nc].  Conv2d's weight is [out][in][kh][kw], ConvTranspose2d's [in][out][kh][kw]."""
    w4 = W.view(d.KH, d.KW, d.K, d.Nc)
    if not d.transposed:
        y = F.conv2d(_nchw(src), w4.permute(3, 2, 0, 1).contiguous(), stride=d.stride, padding=d.pad)
    else:
        op = (d.OH - ((d.IH - 1) * d.stride - 2 * d.pad + d.KH), d.OW - ((d.IW - 1) * d.stride - 2 * d.pad + d.KW))
        assert 0 <= op[0] < max(d.stride, 2) and 0 <= op[1] < max(d.stride, 2), (d, op)
        if d.stride == 1:
            assert op == (0, 0)
        y = F.conv_transpose2d(_nchw(src), w4.permute(2, 3, 0, 1).contiguous(), stride=d.stride, padding=d.pad, output_padding=op)
    assert y.shape[2:] == (d.OH, d.OW), (d, y.shape)
    return y.permute(0, 2, 3, 1)


def test_conv_reference_is_torch():
    seen, worst = set(), 0.0
    for c in O.CONV_CASES:
        d = O.conv_desc(c, 0)
        key = (d.KH, d.KW, d.stride, d.pad, d.transposed, d.IH, d.IW, d.OH, d.OW, bool(c.K1), c.epi)
        if key in seen:
            continue
        seen.add(key)
        d = d._replace(N=min(d.N, 3), K=min(d.K, 12), K1=min(d.K, 12) if not c.K1 else 4, Nc=min(d.Nc, 9))
        g = torch.Generator().manual_seed(len(seen))
        src = torch.randn(d.N, d.IH, d.IW, d.K, dtype=F64, generator=g)
        W = torch.randn(d.KH * d.KW, d.K, d.Nc, dtype=F64, generator=g)
        bias, res, prior = (torch.randn(s, dtype=F64, generator=g) for s in ((d.Nc,), (d.N, d.OH, d.OW, d.Nc), (d.N, d.OH, d.OW, d.Nc)))
        x, x2 = (src[..., :d.K1], src[..., d.K1:]) if c.K1 else (src, None)
        want = _torch_conv(d, src, W)
        got = O.conv_ref(d, x, W, x2)
        worst = max(worst, float((got - want).abs().max()))
        # both weight layouts decode to the header's W(ky, kx, k, j)
        for kn in (0, 1):
            mem = O.w_memory(W, kn).reshape(-1)
            t, k, j = 1 % (d.KH * d.KW), d.K - 1, d.Nc // 2
            assert float(mem[(t * d.K + k) * d.Nc + j] if kn else mem[(t * d.Nc + j) * d.K + k]) == float(W[t, k, j])
        full = O.conv_ref(d, x, W, x2, bias, res, prior)
        assert float((full - (want + bias + res + prior)).abs().max()) <= 1e-12
        ab = O.conv_ref(d, x, W, x2, bias, absolute=True)
        assert float((ab - (_torch_conv(d, src.abs(), W.abs()) + bias.abs())).abs().max()) <= 1e-12
    assert len(seen) >= 40 and worst <= 1e-12, (len(seen), worst)


def _torch_wgrad(d, P, Q):
    """autograd's weight gradient of the layer the descriptor stands for."""
    if d.gather_i:        # Conv2d: input P on the gathered grid, output gradient Q on the direct grid
        w = torch.zeros(d.Cj, d.Ci, d.KH, d.KW, dtype=F64, requires_grad=True)
        y = F.conv2d(_nchw(P), w, stride=d.stride, padding=d.pad)
        if y.shape[2:] != (d.DH, d.DW):              # a direct grid larger than the natural output (k4 / s1 / p1 on 8 -> 8) has no torch layer
            return None
        (gw,) = torch.autograd.grad(y, w, _nchw(Q))
        return gw.permute(2, 3, 1, 0).reshape(d.KH * d.KW, d.Ci, d.Cj)
    w = torch.zeros(d.Ci, d.Cj, d.KH, d.KW, dtype=F64, requires_grad=True)   # ConvTranspose2d: input P direct, output gradient Q gathered
    op = (d.GH - ((d.DH - 1) * d.stride - 2 * d.pad + d.KH), d.GW - ((d.DW - 1) * d.stride - 2 * d.pad + d.KW))
    if not (0 <= op[0] < max(d.stride, 2) and 0 <= op[1] < max(d.stride, 2)) or (d.stride == 1 and op != (0, 0)):
        return None
    y = F.conv_transpose2d(_nchw(P), w, stride=d.stride, padding=d.pad, output_padding=op)
    (gw,) = torch.autograd.grad(y, w, _nchw(Q))
    return gw.permute(2, 3, 0, 1).reshape(d.KH * d.KW, d.Ci, d.Cj)


def test_wgrad_reference_is_torch():
    seen, worst, n = set(), 0.0, 0
    for c in O.WG_CASES:
        d = O.wg_desc(c, 0)
        key = (d.KH, d.KW, d.stride, d.pad, d.gather_i, d.GH, d.GW, d.DH, d.DW, bool(c.I1))
        if key in seen:
            continue
        seen.add(key)
        d = d._replace(N=min(d.N, 3), Ci=min(d.Ci, 8), Cj=min(d.Cj, 5))
        I1 = 4 if c.I1 else d.Ci
        g = torch.Generator().manual_seed(len(seen))
        gs, ds = (d.N, d.GH, d.GW), (d.N, d.DH, d.DW)
        P = torch.randn((gs if d.gather_i else ds) + (d.Ci,), dtype=F64, generator=g)
        Q = torch.randn((ds if d.gather_i else gs) + (d.Cj,), dtype=F64, generator=g)
        want = _torch_wgrad(d, P, Q)
        if want is None:
            continue
        got = O.wgrad_ref(d, P[..., :I1], Q, P[..., I1:] if c.I1 else None)
        worst = max(worst, float((got - want).abs().max()))
        n += 1
    assert n >= 14 and worst <= 1e-12, (n, worst)
    x = torch.randn(37, 5, dtype=F64)
    assert torch.equal(O.colsum_ref(x), x.sum(0))


# ---------------------------------------------------------------------------------------------------- planners
def _conv_case_descs():
    out = []
    for c in O.CONV_CASES:
        for mode, wb, i16 in O.conv_variants(c):
            out.append((O.conv_desc(c, mode), wb, i16, O.conv_aligned(c)))
    return out


def _wg_case_descs():
    return [(O.wg_desc(c, m), O.wg_aligned(c), slab) for c in O.WG_CASES for m in c.modes for slab in (0, 1)]


def test_restated_planner_is_the_library():
    lib = _lib()
    n_ok = n_ref = n_fast = 0
    for d, wb, i16, al in _conv_case_descs() + O.random_conv_descs(4000):
        want, got = O.igemm_plan(d, wb, i16, al), _iplan(lib, d, wb, i16, al)
        if isinstance(want, str):
            assert isinstance(got, str) and want in got, (d, wb, i16, al, want, got)
            n_ref += 1
        else:
            assert got == want, (d, wb, i16, al, want, got)
            n_ok += 1
            n_fast += want.kernel
        bm, bn = ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.mi_conv_igemm_tile(_cd(d), ctypes.byref(bm), ctypes.byref(bn)) == 0
        assert (bm.value, bn.value) == O.igemm_tile(d), d                      # (the tile query does not check the descriptor)
        assert isinstance(want, str) or (want.bm, want.bn) == (bm.value, bn.value)
        assert lib.mi_conv_igemm_bf16w_io_supported(_cd(d)) == O.io_supported(d), d
        if O.io_supported(d):                                                  # what _supported admits, the dispatch's plan places
            p = _iplan(lib, d, 1, 1, 1)
            assert not isinstance(p, str) and p.kernel == 1, (d, p)
    assert n_ok > 1000 and n_ref > 1000 and n_fast > 100, (n_ok, n_ref, n_fast)
    n_ok = n_ref = n_fast = 0
    for d, al, slab in _wg_case_descs() + O.random_wg_descs(3000):
        want, got = O.wgrad_plan(d, al, slab), _wplan(lib, d, al, slab)
        if isinstance(want, str):
            assert isinstance(got, str) and want in got, (d, al, slab, want, got)
            n_ref += 1
        else:
            assert got == want, (d, al, slab, want, got)
            n_ok += 1
            n_fast += want.fast
            assert want.chunk % 32 == 0 and (want.splits - 1) * want.chunk < d.N * d.DH * d.DW <= want.splits * want.chunk
        assert lib.mi_conv_wgrad_slabs_workspace(_wd(d)) == O.slabs_workspace(d), d
    assert n_ok > 1000 and n_ref > 300 and n_fast > 100, (n_ok, n_ref, n_fast)
    # the layer of the issue: _supported used to admit it, the dispatch requires KH >= stride
    d = O.ConvD(N=2, IH=4, IW=4, OH=8, OW=8, K=64, Nc=64, KH=1, KW=2, stride=2, pad=0, transposed=1, w_kn=0, mode=1, K1=64, ldx=64, ldx2=0, ldy=64, ldr=0, accumulate=0)
    assert O.io_supported(d) == 0 and lib.mi_conv_igemm_bf16w_io_supported(_cd(d)) == 0
    assert "kernel smaller than stride" in _iplan(lib, d, 1, 1, 1)
    assert lib.mi_conv_igemm_bf16w_io_supported(_cd(d._replace(KH=2))) == 1


def test_case_lists_reach_every_instantiation_and_edge():
    lib = _lib()
    e = O.conv_edges()
    missing = [k for k in O.CONV_REQUIRED if k not in e]
    assert not missing, missing
    assert {k[5:] for k in e if k.startswith("inst:")} == {repr(i) for i in O.all_igemm_instantiations()} and len(O.all_igemm_instantiations()) == 16
    names = [c.name for c in O.CONV_CASES]
    assert len(names) == len(set(names)) and set(O.CONV_PLANS) <= set(names)
    for c in O.CONV_CASES:
        mode, wb, i16 = O.conv_variants(c)[0]
        got = _iplan(lib, O.conv_desc(c, mode), wb, i16, O.conv_aligned(c))
        assert not isinstance(got, str) and O.igemm_plan_name(got, mode, i16) == c.plan, (c, got)       # the library's own answer
        assert O.CONV_PLANS.get(c.name, c.plan) == c.plan, (c, c.plan)                                   # ... and the written table
        for mode, wb, i16 in O.conv_variants(c):
            d = O.conv_desc(c, mode)
            if wb:
                assert d.K % 8 == 0
            if i16:
                assert O.io_supported(d)
            # in bounds: what the kernels read and write stays inside the case's tensors
            assert d.ldx >= d.K1 and (not c.K1 or d.ldx2 >= d.K - d.K1) and d.ldy >= d.Nc
    # most cases are small: under 10 k output pixels and K <= 64; those that reach a tile form use K <= 8 (generic) or one ring stage per tap
    big = [c for c in O.CONV_CASES if c.N * c.O[0] * c.O[1] > 10000]
    assert {c.name for c in big} == {"tile_128x128", "tile_128x64", "tile_64x128", "ring_128x128", "ring_128x64", "ring_64x128", "ring_128x128_x16",
                                     "ring_128x64_x16", "ring_64x128_x16"} and all(c.K <= 8 or c.wb for c in big)
    e = O.wg_edges()
    missing = [k for k in O.WG_REQUIRED if k not in e]
    assert not missing, missing
    names = [c.name for c in O.WG_CASES]
    assert len(names) == len(set(names)) and set(O.WG_PLANS) <= set(names)
    for c in O.WG_CASES:
        d = O.wg_desc(c, c.modes[0])
        got = _wplan(lib, d, O.wg_aligned(c), 0)
        assert not isinstance(got, str) and O.wgrad_plan_name(got, c.modes[0]) == c.plan and O.WG_PLANS.get(c.name, c.plan) == c.plan, (c, got)
        if got.xcd_map:      # the map covers every (slice, tile, tap) once, the surplus drops out
            B = 128 if got.big else 64
            inner = O._cdiv(d.Ci, B) * O._cdiv(d.Cj, B) * d.KH * d.KW
            assert sorted(O.xcd_ids(got, inner)) == [(s, i) for s in range(got.splits) for i in range(inner)], c
    for M, C, ld, off in O.COLSUM_CASES:
        assert O.colsum_own_kernel(M, C, ld, off) and ld >= C, (M, C, ld, off)
    assert not O.colsum_own_kernel(100, 64, 64, 0)


# ---------------------------------------------------------------------------------------------------- refusals
P0 = 0x7f0000001000          # a made-up, 4096-byte aligned address: never dereferenced


def test_refusals_name_the_requirement():
    lib = _lib()
    n = [0]

    def refused(rc, text, what):
        n[0] += 1
        assert rc != 0, ("accepted", what)
        msg = lib.mi_last_error().decode()
        assert text in msg, (what, msg)

    X, X2, Wp, B, R, Y, WS = (P0 + i * 0x100000 for i in range(7))
    ok = O.ConvD(N=2, IH=4, IW=4, OH=8, OW=8, K=64, Nc=64, KH=4, KW=4, stride=2, pad=1, transposed=1, w_kn=0, mode=1, K1=64, ldx=64, ldx2=0, ldy=64, ldr=0, accumulate=0)

    def ig(d, x=X, x2=None, w=Wp, res=None, y=Y):
        return lib.mi_conv_igemm(_cd(d) if d is not None else None, x, x2, w, B, res, y, None)

    def igw(d, x=X, x2=None, w=Wp, y=Y):
        return lib.mi_conv_igemm_bf16w(_cd(d) if d is not None else None, x, x2, w, B, None, y, None)

    def io(d, x=X, x2=None, w=Wp, y=Y):
        return lib.mi_conv_igemm_bf16w_io(_cd(d) if d is not None else None, x, x2, w, B, None, y, 1, None)

    for kw in (dict(d=None), dict(x=None), dict(w=None), dict(y=None)):
        refused(ig(kw.pop("d", ok), **kw), "null argument", kw)
    for f in ("N", "K", "Nc", "KH", "KW", "stride"):
        for v in (0, -1):
            refused(ig(ok._replace(**{f: v})), "bad sizes", (f, v))
    refused(ig(ok._replace(mode=2)), "mode must be 0 (fp32) or 1 (bf16)", "mode 2")
    for K1 in (6, 64 + 4, 0, -4):
        refused(ig(ok._replace(K1=K1, ldx2=64), x2=X2), "bad two-source split", K1)
    refused(ig(ok._replace(K1=32, ldx=32, ldx2=32)), "bad two-source split", "x2 null")
    refused(ig(ok._replace(ldx=66)), "ldx must be a multiple of 4, ldy >= Nc", "ldx")
    refused(ig(ok._replace(ldy=63)), "ldx must be a multiple of 4, ldy >= Nc", "ldy")
    refused(ig(ok._replace(ldr=63), res=R), "ldr < Nc", "ldr")
    refused(ig(ok._replace(KH=1, KW=2, pad=0)), "transposed: kernel smaller than stride", "KH < stride")
    refused(ig(ok._replace(KH=2, KW=1, pad=0)), "transposed: kernel smaller than stride", "KW < stride")
    text = "mi_conv_igemm_bf16w: needs mode 1, K % 8 == 0 and 16-byte aligned bf16 weights"
    for d, kw in ((ok._replace(mode=0), {}), (ok._replace(K=36, K1=36, ldx=36), {}), (ok, dict(w=Wp + 8)), (ok, dict(w=None)), (None, {})):
        refused(igw(d, **kw), text, (d, kw))
    text = "mi_conv_igemm_bf16w_io: bf16 activations need mode 1"
    two = ok._replace(K=128, K1=64, ldx2=64)
    for d, kw in ((ok._replace(mode=0), {}), (ok._replace(K=96, K1=96, ldx=96), {}), (two._replace(K1=32, ldx=32), dict(x2=X2)), (ok._replace(ldx=68), {}),
                  (two._replace(ldx2=68), dict(x2=X2)), (ok._replace(KH=5, KW=5), {}), (ok._replace(KH=1, KW=1, stride=1, transposed=0, pad=0, IH=8, IW=8), {}),
                  (ok._replace(OH=7, OW=7), {}), (ok._replace(stride=3, KH=3, KW=3, OH=12, OW=12), {}), (ok, dict(x=X + 8)), (two, dict(x2=X2 + 8)), (ok, dict(w=Wp + 8)),
                  (ok, dict(w=None)), (ok._replace(KH=1, KW=2, pad=0), {}), (ok._replace(N=0), {}), (ok._replace(ldy=60), {})):
        assert d is None or kw or O.io_supported(d) == 0, d
        refused(io(d, **kw), text, (d, kw))
    assert O.io_supported(ok) == 1 and O.io_supported(two) == 1
    # ---- weight gradient
    wok = O.WgD(N=2, GH=8, GW=8, DH=8, DW=8, Ci=64, Cj=64, KH=3, KW=3, stride=1, pad=1, gather_i=1, mode=1, I1=64, ldp=64, ldp2=0, ldq=64)
    Pp, P2, Q, DW_ = X, X2, Wp, Y

    def wg(d, p=Pp, p2=None, q=Q, dw=DW_):
        return lib.mi_conv_wgrad(_wd(d) if d is not None else None, p, p2, q, dw, None)

    def sl(d, ws=WS, nbytes=None, **kw):
        nbytes = O.slabs_workspace(d) if nbytes is None else nbytes
        return lib.mi_conv_wgrad_slabs(_wd(d), kw.get("p", Pp), None, Q, DW_, ws, nbytes, None)

    for kw in (dict(d=None), dict(p=None), dict(q=None), dict(dw=None)):
        refused(wg(kw.pop("d", wok), **kw), "null argument", kw)
    refused(wg(wok._replace(mode=2)), "mode must be 0 or 1", "mode 2")
    for I1 in (6, 68, 0):
        refused(wg(wok._replace(I1=I1, ldp2=64), p2=P2), "bad two-source split", I1)
    refused(wg(wok._replace(I1=32, ldp=32, ldp2=32)), "bad two-source split", "P2 null")
    for f in ("N", "DH", "DW", "Ci", "Cj", "KH", "KW"):
        refused(wg(wok._replace(**{f: 0})), "bad sizes", f)
    refused(sl(wok, ws=None), "needs a workspace", "null ws")
    refused(sl(wok, ws=WS + 2), "needs a workspace", "misaligned ws")
    refused(sl(wok, nbytes=O.slabs_workspace(wok) - 4), "workspace smaller than mi_conv_wgrad_slabs_workspace()", "4 bytes short")
    refused(sl(wok._replace(Ci=0)), "workspace smaller than mi_conv_wgrad_slabs_workspace()", "no plan")
    refused(sl(wok._replace(mode=2)), "mode must be 0 or 1", "slab mode 2")
    refused(sl(wok, p=None), "null argument", "slab null P")
    # ---- column sums
    for a in ((0, 4, X, 4, Y), (4, 0, X, 4, Y), (4, 4, None, 4, Y), (4, 4, X, 4, None)):
        refused(lib.mi_colsum(*a, None), "bad argument", a)
    need = lib.mi_colsum_ordered_workspace(300, 5)
    assert need == 2 * 5 * 4
    for a in ((300, 5, X, 4, Y, WS, need), (300, 5, X, 5, Y, None, need), (300, 5, X, 5, Y, WS, need - 4), (0, 5, X, 5, Y, WS, need), (300, 5, None, 5, Y, WS, need)):
        refused(lib.mi_colsum_ordered(*a, None), "bad argument or workspace", a)
    assert n[0] >= 70


# ---------------------------------------------------------------------------------------------------- operand families
def test_integer_families_are_exact_in_fp32():
    """|x| <= 4, |w| <= 3, bias / residual / prior content at most 3: the sum over |terms| of every case stays below 2^24, so every fp32
    partial sum is an exact integer under any order, atomics included."""
    worst = 0
    for c in O.CONV_CASES:
        d = O.conv_desc(c, 0)
        classes = O.igemm_geometry(d)[0]
        taps = max(len(O.class_taps(d, k)) for k in range(classes))
        worst = max(worst, taps * c.K * 12 + 9)
    assert O.int_exact(worst) and worst >= 4224 * 12
    for c in O.WG_CASES:
        assert O.int_exact(c.N * c.D[0] * c.D[1] * 12 + 3), c
    for M, C, ld, off in O.COLSUM_CASES:
        assert O.int_exact(M * 4 + 3)
    # on the operands themselves, for the heaviest contraction and a weight-gradient case
    c = O.conv_case("ks_k4224")
    ops = O.conv_operands(c, "int")
    ab = O.conv_reference(c, 1, ops, False)[1]
    assert O.int_exact(float(ab.max())) and bool((ab == ab.round()).all()) and float(ops["x"].abs().max()) == 4 and float(ops["W"].abs().max()) == 3
    c = O.wg_case("r_xcd16")
    ops = O.wg_operands(c, "int")
    ab = O.wg_reference(c, 1, ops, False)[1]
    assert O.int_exact(float(ab.max()) + 3) and bool((ops["prior"] != 0).all())
    # integers survive the rounding to bf16 that mode 1 applies, and truncation is another function than rounding on randn operands
    assert torch.equal(O.bf16_round(ops["P"]), ops["P"])
    x = O.randn((4096,), 3)
    trunc = (x.float().view(torch.int32) & -65536).view(torch.float32).double()
    assert not torch.equal(trunc, O.bf16_round(x))


def test_operand_builders_keep_nan_and_sentinels():
    t = O.ints((6, 3), -4, 4, 1)
    a = O.In(t, ld=4, off=1)
    assert bool(torch.isnan(a.buf[:O.PAD + 1]).all()) and bool(torch.isnan(a.rows[:, 3]).all()) and bool(torch.isnan(a.buf[O.PAD + 1 + 24:]).all())
    assert torch.equal(a.rows[:, :3].double(), t) and a.ptr % 16 == 4 and a.intact()
    o = O.Out(6, 3, ld=4, init64=O.init_content((6, 3), 5))
    assert bool((o.get() != 0).all()) and o.untouched()
    o.rows[0, 3] = 1.0
    try:
        o.get()
        raise RuntimeError("padding write not seen")
    except AssertionError:
        pass
    o.reset()
    assert o.untouched() and bool(torch.isnan(O.Out(2, 2, nan=True).get()).all())
