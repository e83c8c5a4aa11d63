"""tests/_conv_pw_oracle.py against independent facts, without a GPU: the float64 references against torch.autograd; the fragment layouts
as permutations of the master layout; the restated planner against the library's own queries (the library loads without a device, and
with no split-K workspace registered pw_split answers 1) over every case of the lists and a few thousand random descriptors, under every
forced tile; the edges the case lists must keep reaching; the exactness conditions of the integer operand families; and the float32
emulation's figures that the fused variants' GPU bound is four times of.

Measured here (float32 emulation of the fused staging against the rounding model, relative to sum |h| |w| + |bias|, worst over the fused
cases, both storages of x and eight seeds; not used as a bound beyond the rounded-up figure in the oracle): 3.1e-5 with ordinary
parameters, 2.1e-5 with wide ones, 1.4e-5 on the other samples of the case with a sample of constant x and 0 on that sample (one value
per channel: whole channels flip or none); the oracle keeps 3.5e-5 for all."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_pw_oracle as O  # noqa: E402

F64 = torch.float64


def _lib():
    from src.ops.lib import load_library
    return load_library()


def _cdesc(d):
    from src.ops.lib import MiConvDesc
    return ctypes.byref(MiConvDesc(**d._asdict()))


# ---------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("N,H,W,Ci,Co,K1", [(2, 5, 8, 6, 4, 0), (1, 4, 3, 8, 5, 3), (3, 2, 2, 4, 4, 0)])
def test_references_against_autograd(N, H, W, Ci, Co, K1):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, H, W, Ci, generator=g, dtype=F64).requires_grad_(True)
    Wm = torch.randn(9, Ci, Co, generator=g, dtype=F64)             # master layout [tap][ci][co]
    bias, res, prior = torch.randn(Co, generator=g, dtype=F64), torch.randn(N, H, W, Co, generator=g, dtype=F64), torch.randn(N, H, W, Co, generator=g, dtype=F64)
    w4 = Wm.view(3, 3, Ci, Co).permute(3, 2, 0, 1)
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w4, bias, padding=1).permute(0, 2, 3, 1)
    dy = torch.randn(N, H, W, Co, generator=g, dtype=F64)
    dx, = torch.autograd.grad(y, x, dy)
    xa, xb = (x.detach()[..., :K1], x.detach()[..., K1:]) if K1 else (x.detach(), None)
    assert O.rel(O.conv_ref(xa, Wm, False, xb, bias), y) <= 1e-12
    assert O.rel(O.conv_ref(xa, Wm, False, xb, bias, res, prior), y + res + prior) <= 1e-12
    assert O.rel(O.conv_ref(dy, O.dgrad_operand(Wm), True), dx) <= 1e-12
    # two sources on the gradient's side: the contraction over co split in two
    c1 = Co // 2
    assert O.rel(O.conv_ref(dy[..., :c1], O.dgrad_operand(Wm), True, dy[..., c1:], prior=x.detach()), dx + x.detach()) <= 1e-12
    ab = O.conv_ref(xa, Wm, False, xb, bias, res, prior, absolute=True)
    assert bool((ab >= (y + res + prior).abs() - 1e-12).all())


# ---------------------------------------------------------------------------------------------------- fragment layouts
@pytest.mark.parametrize("f32", [False, True])
def test_fragment_layouts_are_permutations_of_the_master_layout(f32):
    ci, co = 128, 64
    Wm = torch.arange(9 * ci * co, dtype=F64).view(9, ci, co)
    step, e = (8, 4) if f32 else (16, 8)
    fq, dq = O.wfq(Wm, f32), O.wdq(Wm, f32)
    assert fq.shape == (9, co // 32, ci // step, 64, e) and dq.shape == (9, ci // 32, co // step, 64, e)
    for t in (fq, dq):
        assert torch.equal(t.reshape(-1).sort().values, Wm.reshape(-1))                  # every master element exactly once
        assert torch.equal(t.reshape(9, -1).sort(1).values, Wm.reshape(9, -1))           # ... and inside its own tap
    # spot values straight from the header's formulas
    for tap, nb, kq, lane, j in [(0, 0, 0, 0, 0), (4, 1, 3, 37, 2), (8, co // 32 - 1, ci // step - 1, 63, e - 1)]:
        assert fq[tap, nb, kq, lane, j] == Wm[tap, step * kq + e * (lane >> 5) + j, 32 * nb + (lane & 31)]
    for tap, nb, kq, lane, j in [(0, 0, 0, 0, 0), (5, 2, 1, 44, 3), (8, ci // 32 - 1, co // step - 1, 63, e - 1)]:
        assert dq[tap, nb, kq, lane, j] == Wm[tap, 32 * nb + (lane & 31), step * kq + e * (lane >> 5) + j]
    assert torch.equal(dq, O.wfq(Wm.transpose(1, 2).contiguous(), f32))                   # the data gradient contracts over co
    G = torch.arange(9 * ci * co, dtype=F64).view(9, ci, co)
    assert torch.equal(O.frag_operand(G, False, f32), fq) and torch.equal(O.frag_operand(G, True, f32), O.wfq(G, f32))


# ---------------------------------------------------------------------------------------------------- planner
def _queries(lib, d, kn):
    c = _cdesc(d)
    got = (lib.mi_conv3x3_pw_supported(c), lib.mi_conv3x3_pw_tile(c), lib.mi_conv3x3_pw_x32_supported(c), lib.mi_conv3x3_pw_x32_tile(c),
           lib.mi_conv3x3_pw_f32_tile(c), lib.mi_conv3x3_pw_gn_mish_supported(c), lib.mi_conv3x3_pw_gn_mish_tile(c),
           lib.mi_conv3x3_pw_x32_gn_mish_supported(c), lib.mi_conv3x3_pw_x32_gn_mish_tile(c)) + tuple(
        lib.mi_conv3x3_pw_splitk(c, var, in32) for var in (0, 1, 2, 3) for in32 in (0, 1))
    want = (O.q_supported(d, kn), O.q_tile(d, kn), O.q_supported(d, kn, True), O.q_tile(d, kn, True), O.q_tile(d, kn, f32=True),
            int(O.q_fused_tile(d, kn) != 0), O.q_fused_tile(d, kn), int(O.q_fused_tile(d, kn, True) != 0), O.q_fused_tile(d, kn, True)) + tuple(
        O.q_splitk(d, var, in32, kn) for var in (0, 1, 2, 3) for in32 in (0, 1))
    return got, want


def _all_case_descs():
    out = []
    for c in O.PLAIN_CASES + O.GNS_CASES + O.X32_CASES:
        out += [O.plain_desc(c, 0), O.plain_desc(c, 1)]
    out += [O.plain_desc(c, 0, f32=True) for c in O.F32_CASES]
    out += [O.desc(c.N, c.H, c.W, c.K, c.Nc) for c in O.FUSED_CASES] + [O.split_desc(c) for c in O.SPLIT_CASES]
    return out


def test_restated_planner_is_the_library():
    lib = _lib()
    descs = _all_case_descs() + O.random_descs(3000)
    n_ok = 0
    on_gpu = torch.cuda.is_available()                     # run beside the GPU tests: no split-K workspace while the plans are compared
    if on_gpu:
        lib.mi_conv_pw_set_splitk_workspace(None, 0)
    try:
        for force in (0, 64, 128, 256):
            assert lib.mi_debug_conv_pw_tile(force) == 0
            for mode in (1, 2):
                was = lib.mi_debug_conv_pw_splitk(mode)
                kn = O.Knobs(force, mode, 0)
                for d in descs:
                    got, want = _queries(lib, d, kn)
                    assert got == want, (d, force, got, want)
                    n_ok += got[0]
                lib.mi_debug_conv_pw_splitk(was)
    finally:
        lib.mi_debug_conv_pw_tile(0)
        lib.mi_debug_conv_pw_splitk(1)
        if on_gpu:
            from src.ops import functional as K
            mine = K._SPLITK_WS.get(torch.cuda.current_device())
            if mine is not None:
                lib.mi_conv_pw_set_splitk_workspace(mine.data_ptr(), mine.numel())
            K._QUERY_CACHE.clear()
    assert n_ok > 1000                                     # the enumeration is not all refusals
    assert lib.mi_debug_conv_pw_tile(96) != 0 and b"mi_debug_conv_pw_tile" in lib.mi_last_error()
    # the 2^31 fragment-offset limit needs nothing allocated: Nc K 2 9 bytes
    big = O.desc(2, 8, 8, 1024 * 128, 1024)
    assert O.pw_ok(big, 128) is None and O.pw_ok(O.desc(2, 8, 8, 1024, 1024), 128) is not None
    assert lib.mi_conv3x3_pw_supported(_cdesc(big)) == 0 and lib.mi_conv3x3_pw_tile(_cdesc(big)) == 0


def test_split_plans_of_the_restated_planner():
    """pw_split needs a registered workspace, which needs a device: here the restatement is held to the arithmetic of every split
    case (the GPU test compares it with mi_conv3x3_pw_splitk on registered workspaces)."""
    for c in O.SPLIT_CASES:
        d, kn = O.split_desc(c), O.split_kn(c)
        var = {"plain": 0, "sums": 1, "x32": 0, "fused": 2, "fused32": 2}[c.variant]
        ks, pt, TH, TI, need = O.pw_split(d, var, c.variant in ("x32", "fused32"), kn)
        if ks == 1:
            assert c.name == "rule_off_k960"
            continue
        tiles = (d.N * d.OH * d.OW // pt) * ((d.Nc + 127) // 128)
        assert need == 65536 + (ks - 1) * tiles * pt * 512 and (d.K // 64) % ks == 0 and d.K // 64 // ks >= 2
        assert O.pw_split(d, var, False, kn._replace(ws_bytes=need))[0] == ks
        assert O.pw_split(d, var, False, kn._replace(ws_bytes=need - pt * 512))[0] == 1          # one partial tile short
        assert tiles * ks <= 400
    # the flag area: (ks - 1) tiles 16 bytes must fit 64 KB
    wide = O.desc(1032, 8, 8, 256, 512)                    # 4 128 tiles: 16 bytes each is 512 bytes too many
    assert O.pw_split(wide, 0, False, O.Knobs(64, 2, 1 << 40))[0] == 1 and O.pw_split(O.desc(1024, 8, 8, 256, 512), 0, False, O.Knobs(64, 2, 1 << 40))[0] == 2
    assert O.pw_split(O.FLAG_EDGE, 0, False, O.Knobs(64, 4, 1 << 40))[0] == 1 and O.pw_split(O.FLAG_EDGE, 0, False, O.Knobs(64, 2, 1 << 40))[0] == 2
    assert O.pw_split(wide, 0, False, O.Knobs(256, 2, 1 << 40))[0] == 1 and O.pw_split(wide, 0, False, O.Knobs(64, 0, 1 << 40))[0] == 1


def test_case_lists_reach_every_edge():
    e = O.edges()
    missing = [k for k in O.REQUIRED_EDGES if k not in e]
    assert not missing, missing
    assert {k[5:] for k in e if k.startswith("inst:")} == {repr(i) for i in O.all_instantiations()}
    names = [c.name for c in O.PLAIN_CASES + O.GNS_CASES + O.X32_CASES + O.F32_CASES + O.FUSED_CASES + O.SPLIT_CASES]
    assert len(names) == len(set(names))
    for c in O.PLAIN_CASES + O.GNS_CASES + O.X32_CASES + O.F32_CASES + O.FUSED_CASES + O.SPLIT_CASES:
        assert O.case_pixels(c) <= 4096 and c.K <= 1024 and c.Nc <= 768, c
    # the geometry table of the issue, row by row: (W, tile, H) -> (TH, TI)
    table = {(32, 64, 2): (2, 1), (32, 128, 4): (4, 1), (32, 128, 8): (4, 1), (32, 256, 8): (8, 1), (32, 256, 16): (8, 1), (16, 64, 2): (2, 2),
             (16, 64, 4): (4, 1), (16, 64, 12): (4, 1), (16, 128, 4): (4, 2), (16, 128, 8): (8, 1), (16, 128, 48): (8, 1), (16, 256, 16): (16, 1),
             (8, 64, 4): (4, 2), (8, 64, 8): (8, 1), (8, 64, 24): (8, 1), (8, 128, 8): (8, 2), (8, 128, 16): (16, 1), (8, 128, 32): (16, 1), (8, 256, 32): (32, 1)}
    seen = {(c.W, c.pt, c.H): O.pw_geom(O.plain_desc(c), c.pt) for c in O.GEOMETRY_CASES}
    assert seen == table


# ---------------------------------------------------------------------------------------------------- integer families
def test_integer_families_are_exact_in_fp32():
    """|x| <= 4, |w| <= 3: every partial sum of 9 K products (and bias, residual, prior content of at most 4) is an integer below 2^24 in
    magnitude whatever the order -- split-K included; checked on the sums over |terms| of the heaviest cases."""
    assert 9 * 1024 * 12 + 3 * 4 < 2 ** 24
    for c in [c for c in O.PLAIN_CASES if c.K >= 320] + O.F32_CASES[:1]:
        x = O.operand((c.N, c.H, c.W, c.K), "int", 1)
        G = O.operand((9, c.K, c.Nc), "int", 2, amp=3)
        ab = O.conv_ref(x, G, absolute=True)
        assert float(ab.max()) + 12 < 2 ** 24 and bool((ab == ab.round()).all())


@pytest.mark.parametrize("case", O.GNS_CASES, ids=repr)
def test_unit_family_keeps_the_groupnorm_sums_exact(case):
    c = case
    for out16 in (False, True):
        y = O.stored(O.plain_reference(O.plain_operands(c, "unit"))[0], out16)
        assert O.unit_sums_exact(y, c.pt, c.H, c.W), c
        s = O.gn_sums(y)
        assert s.dtype == torch.int64 and bool((s % (1 << 20) == 0).all())


# ---------------------------------------------------------------------------------------------------- the fused variants' figure
def fused_figures(c, seed=0, x_f32=False):
    """-> (figure of the float32 emulation, the same on the other samples of a 'const' case, share of h elements off the model)."""
    ops = O.fused_operands(c, x_f32=x_f32)
    hm = O.fused_h(ops["x"], ops["sc"], ops["sh"], ops["tb"])
    he = O.fused_h_emul32(ops["x"], ops["sc"], ops["sh"], ops["tb"], seed)
    ym, ye = O.conv_ref(hm, ops["G"], bias=ops["bias"]), O.conv_ref(he, ops["G"], bias=ops["bias"])
    scale = O.conv_ref(hm, ops["G"], bias=ops["bias"], absolute=True)
    ratio = (ye - ym).abs() / scale.clamp_min(1e-300)
    share = float((he != hm).double().mean())
    if c.params == "const":
        return float(ratio[1].max()), float(ratio[0].max()), share
    return float(ratio.max()), 0.0, share


def test_fused_emulation_figures():
    """Re-measures, over both storages of x and eight seeds of the emulation's exp / rcp errors each, the figures the GPU test's per-element bound is four times of.  An
    h element the emulation stores differently from the model is one bf16 ulp off, or (without a time bias, far down mish's left tail, where
    ln 2 - 2 ln 2 r cancels) tiny against the other terms of its sums: the share is printed, the figure is what counts."""
    worst = {"plain": 0.0, "wide": 0.0, "const": 0.0}
    for c in O.FUSED_CASES:
        for seed, x_f32 in [(s_, f_) for f_ in (False, True) for s_ in range(8)]:
            fig, other, share = fused_figures(c, seed, x_f32)
            print(f"{c.name} seed {seed} {'fp32' if x_f32 else 'bf16'} x: figure {fig:.3g} (other samples {other:.3g}), h elements off the model {share:.3g}")
            worst[c.params] = max(worst[c.params], fig)
            if c.params == "const":
                worst["plain"] = max(worst["plain"], other)
    print("worst figures:", worst)
    fig = max(worst.values())
    assert fig <= O.FUSED_EMUL_FIGURE, worst              # the constant the GPU bound is four times of is not below the emulation
    assert fig >= O.FUSED_EMUL_FIGURE / 2, worst          # ... nor left far above it
