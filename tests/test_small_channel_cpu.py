"""tests/_small_channel_oracle.py checked without a GPU: the float64 references against torch.autograd, the restated *_supported
predicates against an enumeration written another way and against the library (which loads without a device), the case lists of
tests/test_small_channel_kernels_gpu.py against the instantiations and edges they are there to reach (an edge lost in a later edit
fails here), and the float32 emulation figure the GroupNorm-fused kernel's per-pixel bound rests on."""
import itertools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _small_channel_oracle as O  # noqa: E402

F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    from src.ops.lib import load_library
    return load_library()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------- references against autograd
@pytest.mark.parametrize("shape", [(2, 5, 4, 3, 8, 3), (1, 1, 1, 1, 4, 3), (3, 2, 7, 4, 12, 1), (2, 3, 3, 2, 4, 1)])
def test_conv_refs_against_autograd(shape):
    N, H, W, Cin, Cout, ks = shape
    x, dy = torch.randn(N, H, W, Cin, dtype=F64), torch.randn(N, H, W, Cout, dtype=F64)
    w = torch.randn(Cout, Cin, ks, ks, dtype=F64, requires_grad=True)
    bias = torch.randn(Cout, dtype=F64)
    y = F.conv2d(_nchw(x), w, bias, padding=ks // 2)
    y.backward(_nchw(dy))
    wk = w.detach().permute(2, 3, 1, 0).contiguous()
    assert O.rel(O.conv_fwd_ref(x, wk, bias, ks), y.detach().permute(0, 2, 3, 1)) <= 1e-12
    assert O.rel(O.conv_fwd_ref(x, wk, None, ks) + bias, y.detach().permute(0, 2, 3, 1)) <= 1e-12
    assert O.rel(O.conv_wgrad_ref(x, dy, ks), w.grad.permute(2, 3, 1, 0)) <= 1e-12


@pytest.mark.parametrize("C,Cs", [(32, 1), (64, 3), (8, 4)])
def test_small_cout_refs_against_autograd(C, Cs):
    x = torch.randn(2, 3, 5, C, dtype=F64, requires_grad=True)
    dy = torch.randn(2, 3, 5, Cs, dtype=F64)
    w = torch.randn(Cs, C, 1, 1, dtype=F64, requires_grad=True)
    bias = torch.randn(Cs, dtype=F64)
    xn = _nchw(x)
    y = F.conv2d(xn, w, bias)
    y.backward(_nchw(dy))
    wk = w.detach()[:, :, 0, 0].t().contiguous()
    xm, dym = x.detach().reshape(-1, C), dy.reshape(-1, Cs)
    assert O.rel(O.cout_fwd_ref(xm, wk, bias), y.detach().permute(0, 2, 3, 1).reshape(-1, Cs)) <= 1e-12
    assert O.rel(O.cout_dgrad_ref(dym, wk), x.grad.reshape(-1, C)) <= 1e-12
    assert O.rel(O.cout_wgrad_ref(xm, dym), w.grad[:, :, 0, 0].t()) <= 1e-12


@pytest.mark.parametrize("N,HW,C,G,Cs", [(2, 36, 64, 4, 3), (3, 7, 128, 8, 1), (1, 1, 64, 1, 4)])
def test_groupnorm_mish_conv_ref_against_torch(N, HW, C, G, Cs):
    x = torch.round((torch.randn(N, HW, C, dtype=F64) * 1.3 + 0.2) * 1024) / 1024      # multiples of 2^-10: the 20-fraction-bit sums are exact
    gamma, beta = torch.rand(C, dtype=F64) + 0.5, torch.randn(C, dtype=F64) * 0.3
    w, bias = torch.randn(C, Cs, dtype=F64) * 0.1, torch.randn(Cs, dtype=F64)
    sums = O.gn_sums(x)
    assert sums.shape == (N, C // 16, 2) and sums.dtype == torch.int64
    from src.ops.functional import gn_sums_encode
    xd = x.view(N, HW, C // 16, 16)
    assert torch.equal(sums.view(-1), gn_sums_encode(torch.stack([xd.sum((1, 3)), (xd * xd).sum((1, 3))], dim=-1)))
    hn = F.group_norm(x.permute(0, 2, 1).reshape(N, C, HW, 1), G, gamma, beta, 1e-5)
    hn = hn * torch.tanh(F.softplus(hn))
    ref = F.conv2d(hn, w.t().reshape(Cs, C, 1, 1), bias).reshape(N, Cs, HW).permute(0, 2, 1)
    got = O.gn_mish_conv_ref(x, sums, gamma, beta, G, 1e-5, w, bias)
    assert O.rel(got, ref) <= 1e-12
    ab = O.gn_mish_conv_ref(x, sums, gamma, beta, G, 1e-5, w, bias, absolute=True)
    assert bool((ab >= got.abs() - 1e-12).all())


def test_groupnorm_ref_constant_slab_and_poison():
    x = torch.full((2, 36, 64), 0.75, dtype=F64)
    sums = O.gn_sums(x)
    mean, var = O.gn_stats_from_sums(sums, 36, 64, 2)
    assert torch.equal(mean, torch.full((2, 2), 0.75, dtype=F64)) and torch.equal(var, torch.zeros(2, 2, dtype=F64))
    sums[1, 3, 1] = 1 << 62
    y = O.gn_mish_conv_ref(x, sums, torch.ones(64), torch.zeros(64), 2, 1e-5, torch.ones(64, 2, dtype=F64), None)
    assert bool(torch.isfinite(y[0]).all()) and bool(torch.isnan(y[1]).all())


# ---------------------------------------------------------------------------------------------------- truth tables
TILED_HW = {(64 // W * k, W) for W in (1, 2, 4, 8, 16, 32, 64) for k in (1, 2, 4, 8, 16, 32, 64, 128)}     # whole 64-pixel row tiles, H W a power of two
WGRAD_3X3 = {(1, 64), (1, 128), (1, 256), (2, 64), (2, 128), (3, 64), (3, 128), (4, 64)}                   # 108 Cin Cout <= 49 152


def test_tiled_geometry_and_lds_rule_enumerated():
    for H, W in itertools.product(range(1, 130), range(1, 130)):
        assert O.cin_tiled_geom(3, H, W, 4) == ((H, W) in TILED_HW), (H, W)
    assert not O.cin_tiled_geom(1, 8, 8, 4) and not O.cin_tiled_geom(3, 8, 8, 8) and not O.cin_tiled_geom(3, 8, 8, 4, False)
    for Cin, Cout in itertools.product(range(1, 5), (64, 128, 256)):
        assert O.cin_lds_rule(3, Cin, Cout) == ((Cin, Cout) in WGRAD_3X3)
        assert O.cin_lds_rule(1, Cin, Cout)


def test_supported_predicates_against_the_library_and_functional(lib):
    from src.ops import functional as K
    geoms = [(1, 8, 8), (3, 8, 8), (2, 28, 28), (1, 4, 4), (4, 4, 8), (1, 1, 64), (1, 64, 1), (2, 64, 64), (1, 128, 128), (0, 8, 8), (3, 4, 8), (1, 2, 32), (1, 16, 2)]
    for (N, H, W), ks, Cin, Cout, ldx in itertools.product(geoms, (1, 2, 3), range(0, 6), (4, 32, 64, 128, 256, 512), (3, 4, 8)):
        assert bool(lib.mi_conv_small_cin_bf16_supported(ks, N, H, W, Cin, Cout, ldx)) == O.cin_bf16_supported(ks, N, H, W, Cin, Cout, ldx), (ks, N, H, W, Cin, Cout, ldx)
        exp = ks == 3 and ldx == 4 and N > 0 and (H, W) in TILED_HW and (N * H * W) % 64 == 0 and (Cin, Cout) in WGRAD_3X3
        assert O.cin_bf16_supported(ks, N, H, W, Cin, Cout, ldx) == exp
    for (N, H, W), Cin, Cout, ldx in itertools.product(geoms, range(0, 6), (0, 4, 6, 8, 12, 16, 20, 64, 128, 256, 260, 512), (3, 4, 8)):
        assert bool(lib.mi_conv_small_cin_fwd_dual_supported(N, H, W, Cin, Cout, ldx)) == O.cin_dual_supported(N, H, W, Cin, Cout, ldx), (N, H, W, Cin, Cout, ldx)
    for C, Cs, G in itertools.product((16, 32, 64, 96, 128, 256), range(0, 6), range(0, 17)):
        assert bool(lib.mi_conv1x1_small_cout_gn_supported(C, Cs, G)) == O.cout_gn_supported(C, Cs, G), (C, Cs, G)
        assert O.cout_gn_supported(C, Cs, G) == ((C, G) in {(64, 1), (64, 2), (64, 4), (128, 1), (128, 2), (128, 4), (128, 8)} and 1 <= Cs <= 4)
    for ks, Cin, Cout in itertools.product((1, 2, 3, 5), range(0, 6), (0, 4, 6, 8, 12, 16, 20, 32, 64, 128, 256, 512, 1024, 1028)):
        assert K.small_cin_supported(ks, Cin, Cout) == O.cin_fwd_accepts(ks, 1, 7, 7, Cin, Cout, 4, Cout), (ks, Cin, Cout)
        assert K.small_cin_supported(ks, Cin, Cout, wgrad=True) == O.cin_wgrad_accepts(ks, 1, 7, 7, Cin, Cout, 4, Cout), (ks, Cin, Cout)
    for op, C, Cs in itertools.product((0, 1, 2), (16, 32, 64, 96, 128, 256, 512), range(0, 6)):
        assert K.small_cout_supported(op, C, Cs) == O.cout_accepts(op, 5, C, Cs, C, C if op == 1 else 4), (op, C, Cs)
    for outputs in (4, 27 * 128, 4 * 256):
        assert lib.mi_conv_small_wgrad_workspace(outputs) == O.small_wgrad_workspace(outputs)


def test_plans_by_hand():
    # the shipped MNIST configuration: 28x28, one channel -> the untiled kernels with divisions, never bf16
    p = O.plan_cin_fwd(3, 128, 28, 28, 1, 128, 4)
    assert p["kernel"] == "small_cin_fwd_kernel<1, 3, false, true>" and p["grid"] == 4096 and p["iters"] == 2
    assert O.plan_cin_fwd(3, 128, 28, 28, 1, 128, 4, y_bf16=True)["kernel"] is None
    assert O.plan_cin_wgrad(3, 128, 28, 28, 1, 128, 4, ws_bytes=768 * 9 * 128 * 4)["reduce"] == "ws"
    assert O.plan_cin_wgrad(3, 128, 28, 28, 1, 128, 4, ws_bytes=768 * 9 * 128 * 4 - 4)["reduce"] == "atomic"
    # CelebA 64x64: one image row per tile
    p = O.plan_cin_fwd(3, 14, 64, 64, 3, 8, 4)
    assert p == dict(kernel="small_cin3x3_fwd_tiled_kernel<3, false>", tiled=True, grid=768, iters=2, ntiles=896, wrap=True)
    p = O.plan_cin_wgrad(3, 14, 64, 64, 3, 128, 4)
    assert (p["per"], p["owners"], p["idle"], p["ragged"]) == (2, 448, 320, False)
    p = O.plan_cin_wgrad(3, 769, 8, 8, 3, 128, 4)
    assert (p["per"], p["owners"], p["idle"], p["ragged"]) == (2, 385, 383, True)
    assert O.plan_cin_wgrad(3, 3, 8, 8, 3, 64, 4)["kernel"] == "small_cin_wgrad_kernel<3, 3, true, true>"
    assert O.plan_cin_wgrad(3, 3, 8, 8, 3, 64, 4, dy_bf16=True)["kernel"] == "small_cin3x3_wgrad_tiled_kernel<3, true>"
    assert O.plan_cout(0, 32805, 128, 3) == dict(kernel="small_cout_fwd_kernel<4, false>", grid=1024, iters=2, capped=True, ragged=True)
    assert O.plan_cout(1, 16421, 256, 3, True) == dict(kernel="small_cout_dgrad_kernel<true>", grid=4096, iters=2, capped=True, ragged=True)
    p = O.plan_cout_gn(7 * 4096, 4096, 128)
    assert (p["ppw"], p["grid"], p["iters"], p["straddle"]) == (64, 448, 2, False)
    p = O.plan_cout_gn(3 * 36, 36, 64)
    assert (p["ppw"], p["grid"], p["straddle"], p["ragged"]) == (32, 4, True, True)


def test_argument_conditions_by_hand():
    ok = dict(ks=3, N=2, H=7, W=7, Cin=3, Cout=64, ldx=4, ldy=64)
    assert O.cin_fwd_accepts(**ok)
    for bad in (dict(ks=2), dict(Cin=0), dict(Cin=5), dict(Cout=6), dict(Cout=12), dict(Cout=20), dict(Cout=1028), dict(Cout=0), dict(ldy=66), dict(y_off=8),
                dict(w_off=8), dict(y_bf16=True), dict(y_bf16=True, y_off=4)):
        assert not O.cin_fwd_accepts(**{**ok, **bad}), bad
    t = dict(ks=3, N=2, H=8, W=8, Cin=3, Cout=64, ldx=4, ldy=64, y_bf16=True)
    assert O.cin_fwd_accepts(**t)
    for bad in (dict(H=28, W=28), dict(ldx=3), dict(Cout=512), dict(N=3, H=4, W=8), dict(x_off=4), dict(y_off=4)):
        assert not O.cin_fwd_accepts(**{**t, **bad}), bad
    w = dict(ks=3, N=2, H=7, W=7, Cin=3, Cout=128, ldx=4, lddy=128)
    assert O.cin_wgrad_accepts(**w)
    for bad in (dict(Cout=32), dict(Cout=256), dict(Cin=4), dict(ks=2), dict(lddy=130), dict(dy_off=8), dict(dy_bf16=True), dict(Cin=0), dict(Cin=5)):
        assert not O.cin_wgrad_accepts(**{**w, **bad}), bad
    assert O.cin_wgrad_accepts(**{**w, **dict(Cin=1, Cout=256)}) and O.cin_wgrad_accepts(**{**w, **dict(Cin=4, Cout=64)})
    assert not O.cout_accepts(3, 5, 64, 3, 64, 4) and not O.cout_accepts(0, 5, 256, 3, 256, 4) and not O.cout_accepts(2, 5, 32, 3, 32, 4)
    assert not O.cout_accepts(0, 0, 64, 3, 64, 4) and not O.cout_accepts(0, 5, 64, 0, 64, 4) and not O.cout_accepts(0, 5, 64, 5, 64, 4)
    assert O.cout_accepts(0, 5, 64, 3, 64, 3) and not O.cout_accepts(0, 5, 64, 3, 66, 4) and not O.cout_accepts(0, 5, 64, 3, 64, 4, a_off=8)
    assert O.cout_accepts(0, 5, 64, 3, 64, 4, a_off=8, wide_bf16=True) and not O.cout_accepts(0, 5, 64, 3, 64, 4, a_off=4, wide_bf16=True)
    assert not O.cout_accepts(1, 5, 64, 3, 4, 66) and not O.cout_accepts(2, 5, 64, 3, 64, 3, has_b=False)
    assert O.cout_bwd_accepts(5, 64, 3, 64, 64) and not O.cout_bwd_accepts(5, 32, 3, 32, 32) and not O.cout_bwd_accepts(5, 64, 3, 64, 66)
    assert O.cout_gn_accepts(72, 36, 64, 3, 4, 64, 4)
    for bad in (dict(C=32), dict(C=256), dict(G=8), dict(M=70), dict(ldy=8), dict(ldx=66), dict(x_off=4), dict(y_off=8), dict(Cs=0), dict(Cs=5), dict(M=0)):
        assert not O.cout_gn_accepts(**{**dict(M=72, HW=36, C=64, Cs=3, G=4, ldx=64, ldy=4), **bad}), bad
    assert O.chores_accept(True, 8008) and not O.chores_accept(True, 12) and not O.chores_accept(True, 8, zero_off=4)
    assert O.chores_accept(False, 12) and O.chores_accept(False, gather=True, gather_row=132, gather_n=3)
    assert not O.chores_accept(False, gather=True, gather_row=6, gather_n=3) and not O.chores_accept(False, gather=True, gather_row=4, gather_n=0)


# ---------------------------------------------------------------------------------------------------- the audit
def test_every_instantiation_is_reached_by_a_named_case():
    e = O.edges()
    missing = sorted(k for k in O.all_instantiations() - O.UNREACHABLE if k not in e)
    assert not missing, missing
    # out of reach in the product library: Cin 4 admits 64 output channels only, and fp32 dy at 64 channels goes to the untiled kernel
    for k in O.UNREACHABLE:
        assert k not in e
    assert len(O.all_instantiations()) == 24 + 24 + 8 + 8 + 8 + 6 + 2 + 2 + 4 + 2


def test_every_edge_is_reached_by_a_named_case():
    e = O.edges()
    missing = [k for k in O.REQUIRED_EDGES if k not in e]
    assert not missing, missing


def test_case_lists_are_well_formed_and_small():
    lists = [O.FWD_CASES, O.TILED_CASES, O.DUAL_CASES, O.WG_CASES, O.WGT_CASES, O.C0_CASES, O.C1_CASES, O.C2_CASES, O.GN_CASES]
    names = [c.name for li in lists for c in li]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    small = 0
    for li in lists:
        for c in li:
            px, wide = O.case_sizes(c)
            assert px <= O.MAX_PIXELS and wide <= O.MAX_WIDE_BYTES, (c.name, px, wide)
            small += px <= 10000
    assert small >= 0.8 * len(names)
    for c in O.FWD_CASES:
        assert not O.fwd_plan(c)["tiled"] and O.cin_fwd_accepts(c.ks, c.N, c.H, c.W, c.Cin, c.Cout, c.ldx, O.ldy_of(c.Cout, c.ldyk), c.xoff), c.name
    for c in O.TILED_CASES:
        assert O.fwd_plan(c)["tiled"] and O.cin_fwd_accepts(c.ks, c.N, c.H, c.W, c.Cin, c.Cout, 4, O.ldy_of(c.Cout, c.ldyk), y_bf16=c.y16), c.name
    for c in O.DUAL_CASES:
        assert O.cin_dual_supported(c.N, c.H, c.W, c.Cin, c.Cout, 4) and O.chores_accept(c.zero_bytes > 0, c.zero_bytes, 0, c.gather_row > 0, c.gather_row, c.gather_n), c.name
    for c in O.WG_CASES:
        assert not O.wg_plan(c)["tiled"] and O.cin_wgrad_accepts(c.ks, c.N, c.H, c.W, c.Cin, c.Cout, c.ldx, c.Cout + 8 * c.lddyk, c.xoff), c.name
    for c in O.WGT_CASES:
        assert O.wg_plan(c)["tiled"] and O.cin_wgrad_accepts(c.ks, c.N, c.H, c.W, c.Cin, c.Cout, 4, c.Cout + 8 * c.lddyk, dy_bf16=c.dy16), c.name
    for c in O.C0_CASES:
        assert O.cout_accepts(0, c.M, c.C, c.Cs, c.C + 8 * c.ldak, c.ldo) and c.ldo >= c.Cs, c.name
    for c in O.C1_CASES:
        assert O.cout_accepts(1, c.M, c.C, c.Cs, c.lddy, c.C + 8 * c.ldok) and c.lddy >= c.Cs, c.name
    for c in O.C2_CASES:
        assert O.cout_accepts(2, c.M, c.C, c.Cs, c.C + 8 * c.ldak, c.Cs) and O.cout_bwd_accepts(c.M, c.C, c.Cs, c.C + 8 * c.ldak, c.C + 8), c.name
    for c in O.GN_CASES:
        assert O.cout_gn_accepts(c.N * c.HW, c.HW, c.C, c.Cs, c.G, c.C + 8 * c.ldxk, 4), c.name


def test_integer_operands_are_exact_in_fp32():
    """The largest partial sum of any case stays below 2^24 with operands in {-4..4} and initial content in {-3..3}."""
    worst = max(max(O.case_sizes(c)[0] for c in O.WG_CASES + O.WGT_CASES + O.C2_CASES) * 16 + 3, 27 * 16 + 4, 256 * 16 + 4)
    assert worst < 2 ** 24


# ---------------------------------------------------------------------------------------------------- the emulation figure
def _emul_worst(x, G, Cs, i, rows=None):
    N, HW, C = x.shape
    gamma, beta = O.randn((C,), 200 + i).abs() * 0.5 + 0.5, O.randn((C,), 300 + i) * 0.3
    w, bias = O.randn((C, Cs), 400 + i) * 0.1, O.randn((Cs,), 500 + i)
    sums = O.gn_sums(x)
    ref = O.gn_mish_conv_ref(x, sums, gamma, beta, G, 1e-5, w, bias)
    ab = O.gn_mish_conv_ref(x, sums, gamma, beta, G, 1e-5, w, bias, absolute=True)
    worst = 0.0
    for seed in (0, 1):
        em = O.gn_mish_conv_emul32(x, sums, gamma.float(), beta.float(), G, 1e-5, w.float(), bias.float(), seed)
        r = (em.to(F64) - ref).abs() / ab
        worst = max(worst, float((r if rows is None else r[rows]).max()))
    return worst


def test_groupnorm_fused_float32_emulation_figures():
    """What a float32 evaluation in the kernel's form costs against float64 true Mish on the same inputs, per pixel and relative to
    sum_c |mish(z_c)| |w_c| + |bias|: the GPU test allows the kernel four times O.GN_EMUL_FIGURE (O.GN_EMUL_FIGURE_CONST for a sample of
    constant x: variance 0, x sc + sh cancels at rstd = 1 / sqrt(eps) = 316)."""
    worst = 0.0
    for i, (N, HW, C, G, Cs) in enumerate([(3, 36, 64, 1, 3), (2, 49, 64, 4, 1), (2, 256, 128, 8, 4), (3, 36, 128, 2, 2), (1, 1024, 128, 1, 3)]):
        worst = max(worst, _emul_worst(O.bf16_round(O.randn((N, HW, C), 100 + i) * 1.3 + 0.2), G, Cs, i))
    worst_c = 0.0
    for i, (C, G, Cs) in enumerate([(128, 4, 3), (64, 2, 2), (128, 8, 4), (64, 1, 1)]):
        x = O.bf16_round(O.randn((3, 36, C), 600 + i) * 1.3 + 0.2)
        x[1] = 0.75
        worst_c = max(worst_c, _emul_worst(x, G, Cs, 10 + i, rows=1))
    print(f"float32 emulation of the GroupNorm-fused final conv: worst per-pixel error {worst:.3g} of sum |mish| |w| + |bias|, constant sample {worst_c:.3g}")
    assert 0.5 * O.GN_EMUL_FIGURE <= worst <= O.GN_EMUL_FIGURE, worst
    assert 0.5 * O.GN_EMUL_FIGURE_CONST <= worst_c <= O.GN_EMUL_FIGURE_CONST, worst_c
