"""tests/_conv_stream_oracle.py against independent facts, without a GPU: the literal tap gather against F.conv2d / F.conv_transpose2d and
autograd's data gradients for the layer kinds the project ships and the generic ones gt_plan admits; the 1x1 reference; the restated
planners (pw1_ok in its three forms, gt_plan, lnpw1_ok) against the library's own *_supported / mi_conv_gt_tile answers (the library
loads without a device) over the case lists and random descriptors; the edges the case lists must keep reaching; the exactness of the
LayerNorm family that needs no tolerance, in float32 on the CPU; and the float32 emulation's share of flipped roundings that the GPU
test's 0.1 % cap is held against.

Measured here (float32 emulation in the kernel's order against bf16(float64 LN), x = 1.7 randn - 0.4, share of differing elements): K = 128
4.0e-5 / 2.7e-5 (ordinary / wide parameters), K = 256 5.0e-5 / 2.1e-5, K = 512 2.9e-5 / 2.5e-5 over 4 096 pixels each; every differing
element is off by exactly one bf16 ulp.  x = 100 + 0.1 randn: 2.6 % differ (the float32 mean), which is why that case has its own bound
(the emulation reaches 0.98 of it: one ulp beside a small allowance for the mean)."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_pw_oracle as P  # noqa: E402
import _conv_stream_oracle as O  # noqa: E402

F64, F32 = torch.float64, torch.float32


def _lib():
    from src.ops.lib import load_library
    return load_library()


def _cdesc(d):
    from src.ops.lib import MiConvDesc
    return ctypes.byref(MiConvDesc(**d._asdict()))


# ---------------------------------------------------------------------------------------------------- references
# (k, s, p): the shipped kinds and the generic forms of the case lists
_LAYERS = [(3, 2, 1), (4, 2, 1), (1, 1, 0), (1, 2, 0), (2, 2, 0), (3, 1, 1), (4, 2, 2), (2, 1, 0), (4, 1, 2), (3, 2, 3)]


@pytest.mark.parametrize("k,s,p", _LAYERS)
@pytest.mark.parametrize("IH,IW", [(6, 10), (9, 5)])
def test_forward_gather_is_conv2d_and_its_data_gradient_is_the_transposed_gather(k, s, p, IH, IW):
    g = torch.Generator().manual_seed(5)
    N, Ci, Co = 2, 5, 3
    OH, OW = (IH + 2 * p - k) // s + 1, (IW + 2 * p - k) // s + 1
    x = torch.randn(N, IH, IW, Ci, generator=g, dtype=F64).requires_grad_(True)
    Wm = torch.randn(k * k, Ci, Co, generator=g, dtype=F64)                # master layout [tap][ci][co]
    bias = torch.randn(Co, generator=g, dtype=F64)
    w4 = Wm.view(k, k, Ci, Co).permute(3, 2, 0, 1)
    y = Fn.conv2d(x.permute(0, 3, 1, 2), w4, bias, stride=s, padding=p).permute(0, 2, 3, 1)
    assert y.shape[1:3] == (OH, OW)
    res, prior = torch.randn(y.shape, generator=g, dtype=F64), torch.randn(y.shape, generator=g, dtype=F64)
    got, cnt = O.gather_ref(x.detach(), Wm, k, s, p, 0, OH, OW, bias, res, prior)
    assert P.rel(got, y + res + prior) <= 1e-12
    assert int(cnt.max()) <= k * k and int(cnt.min()) >= 0
    ab, _ = O.gather_ref(x.detach(), Wm, k, s, p, 0, OH, OW, bias, res, prior, absolute=True)
    assert bool((ab >= got.abs() - 1e-12).all())
    # the data gradient: the header's transposed form with the contraction over co, produced tensor = the conv's input
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    dx, = torch.autograd.grad(y, x, dy)
    gd, _ = O.gather_ref(dy, Wm.transpose(1, 2).contiguous(), k, s, p, 1, IH, IW)
    assert P.rel(gd, dx) <= 1e-12


@pytest.mark.parametrize("k,s,p", [(k, s, p) for k, s, p in _LAYERS if 0 <= s + 2 * p - k < s])
def test_transposed_gather_is_conv_transpose2d_and_its_data_gradient_is_the_forward_gather(k, s, p):
    g = torch.Generator().manual_seed(6)
    N, Ci, Co, IH, IW = 2, 4, 3, 5, 7
    op = s * IH - ((IH - 1) * s - 2 * p + k)                               # output_padding that makes the produced tensor s x the input
    assert 0 <= op < s
    u = torch.randn(N, IH, IW, Ci, generator=g, dtype=F64).requires_grad_(True)
    Wt = torch.randn(k * k, Ci, Co, generator=g, dtype=F64)                # [tap][in][out]
    w4 = Wt.view(k, k, Ci, Co).permute(2, 3, 0, 1)
    y = Fn.conv_transpose2d(u.permute(0, 3, 1, 2), w4, None, stride=s, padding=p, output_padding=op).permute(0, 2, 3, 1)
    assert y.shape[1:3] == (s * IH, s * IW)
    got, _ = O.gather_ref(u.detach(), Wt, k, s, p, 1, s * IH, s * IW)
    assert P.rel(got, y) <= 1e-12
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    du, = torch.autograd.grad(y, u, dy)
    gd, _ = O.gather_ref(dy, Wt.transpose(1, 2).contiguous(), k, s, p, 0, IH, IW)
    assert P.rel(gd, du) <= 1e-12


def test_gather_3x3_stride1_is_the_3x3_oracle():
    x, G = P.randn((2, 4, 8, 6), 1), P.randn((9, 6, 5), 2)
    assert P.rel(O.gather_ref(x, G, 3, 1, 1, 0, 4, 8)[0], P.conv_ref(x, G)) <= 1e-13
    assert P.rel(O.gather_ref(x, G, 3, 1, 1, 1, 4, 8)[0], P.conv_ref(x, G, flip=True)) <= 1e-13


def test_1x1_reference_and_gather_k1():
    x, x2, G = P.randn((2, 16, 6), 3), P.randn((2, 16, 4), 4), P.randn((10, 5), 5)
    b, r = P.randn((5,), 6), P.randn((2, 16, 5), 7)
    y = O.pw1_ref(x, G, x2, b, r)
    want = torch.einsum("spk,kj->spj", torch.cat([x, x2], -1), G) + b + r
    assert P.rel(y, want) <= 1e-13
    Gs = P.randn((2, 10, 5), 8)
    assert P.rel(O.pw1_ref(x, Gs, x2), torch.stack([torch.cat([x[i], x2[i]], -1) @ Gs[i] for i in range(2)])) <= 1e-13
    xx = torch.cat([x, x2], -1).view(2, 4, 4, 10)
    assert P.rel(O.gather_ref(xx, G[None], 1, 1, 0, 0, 4, 4, b)[0].view(2, 16, 5), O.pw1_ref(x, G, x2, b)) <= 1e-13


# ---------------------------------------------------------------------------------------------------- planners
def _pw1_queries(lib, d):
    c = _cdesc(d)
    return ((lib.mi_conv1x1_pw_supported(c), lib.mi_conv1x1_pw_x32_supported(c), lib.mi_conv1x1_pw_f32_supported(c), lib.mi_ln_conv1x1_pw_supported(c)),
            (int(O.pw1_ok(d, "bf16")), int(O.pw1_ok(d, "x32")), int(O.pw1_ok(d, "f32")), int(O.lnpw1_ok(d))))


def _gt_query(lib, d):
    pxt, ncls = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib.mi_conv_gt_tile(_cdesc(d), ctypes.byref(pxt), ctypes.byref(ncls))
    sup = lib.mi_conv_gt_supported(_cdesc(d))
    pl = O.gt_plan(d)
    assert sup == int(rc == 0)
    return (rc, pxt.value, ncls.value) if rc == 0 else (rc,), (0, pl.pxt, pl.ncls) if pl else (-1,)


def test_restated_planners_are_the_library():
    lib = _lib()
    descs = [O.pw1_desc(c) for c in O.PW1_CASES] + [O.ln_desc(c) for c in O.LN_CASES + O.LN_LOOP_CASES] + O.random_pw1_descs(400)
    n_ok = [0, 0, 0, 0]
    for d in descs:
        got, want = _pw1_queries(lib, d)
        assert got == want, (d, got, want)
        n_ok = [a + b for a, b in zip(n_ok, got)]
    assert min(n_ok) >= 20, n_ok                                 # the random descriptors are not all refused
    for c in O.PW1_CASES:
        assert O.pw1_ok(O.pw1_desc(c), c.form), c
    gts = [O.gt_desc(c, m) for c in O.GT_CASES for m in (1, 0)] + O.random_gt_descs(600)
    ok = 0
    for d in gts:
        got, want = _gt_query(lib, d)
        assert got == want, (d, got, want)
        ok += got[0] == 0
    assert 120 <= ok <= len(gts) - 100, ok
    assert lib.mi_conv1x1_pw_supported(None) == 0 and lib.mi_conv_gt_supported(None) == 0 and lib.mi_ln_conv1x1_pw_supported(None) == 0


def test_gt_plan_classes_of_the_shipped_layers():
    """The tap lists the kernel walks, by hand: Downsample's data gradient has parity classes of 1, 2, 2, 4 taps; every class's taps are the
    header's definition restricted to that parity, so summing the classes' one-tap gathers gives the literal reference."""
    d = O.gt_desc(O.GT("x", 4, 4, 4, 64, 64, 3, 2, 1, 1))
    pl = O.gt_plan(d)
    assert [(a, b, len(t)) for a, b, t in pl.classes] == [(0, 0, 1), (0, 1, 2), (1, 0, 2), (1, 1, 4)]
    assert pl.classes[0][2] == [(0, 0, 4)] and sorted(pl.classes[3][2]) == [(0, 0, 8), (0, 1, 6), (1, 0, 2), (1, 1, 0)]
    up = O.gt_plan(O.gt_desc(O.GT("x", 4, 4, 4, 64, 64, 4, 2, 1, 1)))
    assert [len(t) for _, _, t in up.classes] == [4, 4, 4, 4] and (up.si, up.so) == (1, 2)
    for c in O.GT_CASES[:20] + O.GT_GENERIC_CASES:
        pl = O.gt_plan(O.gt_desc(c))
        IH, IW, OH, OW = O.gt_geometry(c)
        x, G = P.ints((1, IH, IW, 2), -4, 4, 1), P.ints((c.k * c.k, 2, 3), -3, 3, 2)
        y = torch.zeros(1, OH, OW, 3, dtype=F64)
        for ao, bo, taps in pl.classes:                           # the kernel's walk: class grid, taps as (dy, dx, weight tap)
            for gy_ in range(pl.GH):
                for gx_ in range(pl.GW):
                    for dy, dx, wt in taps:
                        iy, ix = gy_ * pl.si + dy, gx_ * pl.si + dx
                        if 0 <= iy < IH and 0 <= ix < IW:
                            y[0, gy_ * pl.so + ao, gx_ * pl.so + bo] += x[0, iy, ix] @ G[wt]
        assert torch.equal(y, O.gather_ref(x, G, c.k, c.s, c.p, c.tr, OH, OW)[0]), c


def test_plans_of_named_cases():
    byname = {c.name: c for c in O.PW1_CASES}

    def plan(n, o16=True):
        c = byname[n]
        return O.pw1_plan(O.pw1_desc(c), c.form, o16, "r" in c.epi, False, O.pw1_wbatch(c), c.knob)
    assert plan("t128_gx43").pxt == 128 and plan("t128_gx43").gx == 43 and not plan("t128_gx44").flat and plan("t128_gx48_flat").flat
    assert plan("t128_nc128").pxt == 128 and O.pw1_plan(O.pw1_desc(byname["t128_nc128"]._replace(M=32640)), "bf16") .pxt == 64
    assert plan("nloop_nc768_gx44").nloop and plan("nloop_nc320_gx86").nloop and not plan("nloop_nc768_gx44", False).nloop
    assert all(not plan(c.name).nloop for c in O.PW1_NLOOP_OFF_CASES)
    assert not O.pw1_plan(O.pw1_desc(byname["nloop_nc768_gx44"]), "bf16", True, knob=1).nloop                # 44 tiles < 1 024
    assert O.pw1_plan(O.desc1(1, 8192, 16, 128, 384), "bf16", True, knob=1).nloop and not O.pw1_plan(O.desc1(1, 8192, 16, 128, 384), "bf16", True, knob=0).nloop
    assert plan("wb_hw192_t64").pxt == 64 and plan("wb_t128").pxt == 128
    gt = {c.name: O.gt_plan(O.gt_desc(c)) for c in O.GT_CASES}
    assert gt["t128_up_nc256"].pxt == 128 and gt["t128_up_nc256"].M == 4096
    assert O.gt_plan(O.gt_desc(O.GT("x", 8, 16, 16, 64, 256, 4, 2, 1, 1))).pxt == 64                          # half of it: 64-pixel tiles
    ln = {c.name: O.lnpw1_pick(O.ln_desc(c)) for c in O.LN_CASES + O.LN_LOOP_CASES}
    assert ln["loop64_k128"][:3] == (64, 1, False) and ln["loop128_k128"][:3] == (128, 1, False)
    assert O.lnpw1_pick(O.ln_desc(O.LN("x", 32640, 128, 64)))[:3] == (64, 1, True) and O.lnpw1_pick(O.ln_desc(O.LN("x", 65408, 128, 64)))[:3] == (64, 1, False)
    assert [O.lnpw1_lds(64, n) for n in (1, 2, 4)] == [33792, 51200, 86016] and O.lnpw1_lds(128, 1) == 66560


def test_case_lists_reach_every_named_edge():
    e = O.edges()
    missing = [k for k in O.REQUIRED_EDGES if k not in e]
    assert not missing, missing
    names = [c.name for c in O.PW1_CASES] + [c.name for c in O.GT_CASES] + [c.name for c in O.LN_CASES + O.LN_LOOP_CASES]
    assert len(names) == len(set(names))


# ---------------------------------------------------------------------------------------------------- LayerNorm models
@pytest.mark.parametrize("K", [128, 256, 512])
def test_exact_layernorm_family_needs_no_tolerance(K):
    """The kernel's arithmetic in float32 on this CPU: mean exactly 0, sqrt(var) the pixel's power of two, the normalised tensor exactly
    pattern g + b."""
    c = O.LN("x", 256, K, 64)
    o = O.ln_operands(c, "exact")
    assert torch.equal(O.ln_emul32(o["x"], o["g"], o["b"], 0.0), o["ln"])
    assert torch.equal(O.bf16_round(O.ln64(o["x"], o["g"], o["b"], 0.0)[0]), o["ln"])
    assert bool((o["x"].sum(1) == 0).all()) and float(o["ln"].abs().max()) <= 7
    k = O.ln_operands(c, "const")
    assert torch.equal(O.ln_emul32(k["x"], k["g"], k["b"], k["eps"]), O.bf16_round(k["b"]).expand(256, K))


@pytest.mark.parametrize("params", ["plain", "wide"])
@pytest.mark.parametrize("K", [128, 256, 512])
def test_float32_emulation_stays_under_a_quarter_of_the_cap(K, params):
    c = O.LN("emul", 4096, K, 64)
    o = O.ln_operands(c, "randn", params)
    share, worst = O.ln_model_check(O.ln_emul32(o["x"], o["g"], o["b"], o["eps"]), o["x"], o["g"], o["b"], o["eps"])
    print(f"K {K} {params}: share {share:.3g}, worst differing element / allowed {worst:.3g}")
    assert share <= O.LN_DIFFER_CAP / 4 and worst <= 1.0, (share, worst)


def test_offset_input_is_not_held_to_the_bit_model():
    c = O.LN("emul", 2048, 256, 64)
    o = O.ln_operands(c, "offset")
    em = O.ln_emul32(o["x"], o["g"], o["b"], o["eps"])
    share, _ = O.ln_model_check(em, o["x"], o["g"], o["b"], o["eps"])
    w = O.ln_offset_bound(em, o["x"], o["g"], o["b"], o["eps"])
    print(f"offset: share {share:.3g}, worst / bound {w:.3g}")
    assert share > O.LN_DIFFER_CAP and w <= 1.0, (share, w)


def test_integer_families_are_exact():
    for c in O.PW1_CASES[:3] + O.GT_CASES[:3]:
        ops = O.pw1_operands(c, "int") if isinstance(c, O.P1) else O.gt_operands(c, "int")
        for v in ops.values():
            assert v is None or bool((v == v.round()).all())
    with pytest.raises(AssertionError):
        O.assert_exact(1 << 21)
