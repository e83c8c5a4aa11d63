"""CPU oracle of conv3x3_halo_kernel (csrc/conv3x3_halo.hip): the LDS halo-tile 3x3 convolution and data gradient, its 1x1 form, the
dual-output and GroupNorm-sums epilogues and the register-staged fused GroupNorm + Mish entry points.

Shared by tests/test_halo_cpu.py and tests/test_halo_kernels_gpu.py:
  * a restatement of the host planner (halo_geom, halo_ok, halo_w8, halo_wide64, the N64 condition, fused_plan) and of the launch facts of
    launch_halo that select code paths in the kernel (TH, TI, HP, xmap, qmap with its P x Q, the LDS skew, the grid).  The product library
    is built without MI_EXPERIMENT, so every mi_knob is its default: no split-K, no forced ksplit, no PIPE, no row epilogue;
  * all_instantiations(): the 46 instantiations those rules can reach;
  * the case lists -- each case names the plan it is there for -- and edges(): which instantiations and dispatch edges they reach;
  * the operand families (integer: every fp32 partial sum exact; randn), the 1x1 reference, and a float32 emulation of the fused staging
    (z = fma(x, scale, shift), mish_fast_f: e = exp(min(z, 20)), w = e (e + 2), z w rcp(w + 2), + tb, one rounding to bf16; the sums form
    takes rstd from an approximate reciprocal square root).
References, rounding models and number helpers come from tests/_conv_pw_oracle.py.  The rules are read from the .hip file and written again
here; nothing is imported from the package."""
import os
import sys
from collections import namedtuple

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _norm_oracle as NO  # noqa: E402
from _conv_pw_oracle import (F32, F64, GN_EPS, GSUM_SCALE, bf16_round, coef_from_sums, conv_ref, desc, dgrad_operand, fused_h,  # noqa: E402,F401
                             fused_h_emul32, gn_sums, init_content, ints, mish64, operand, randn, rel, seed, stored, term_count, unit_sums_exact)

# worst per-element distance of conv(h of the float32 emulation below) from conv(h of the rounding model), relative to sum |h| |w| + |bias|,
# over the fused cases, both forms (coef / sums), both storages of x and eight seeds (two for the large cases; re-measured and held in
# tests/test_halo_cpu.py: 3.9e-4, rounded up).  It is ten times conv_pw's figure because these cases have K = 32 .. 96: an h element
# stored one bf16 ulp off the model moves an output by 2^-8 of ONE of its 9 K terms, and with 288 terms one term can be a tenth of the sum.
# mish_fast_f is not conv_pw's mish_tb2 sequence either, so this is the halo's own figure.
FUSED_EMUL_FIGURE = 4.5e-4
LARGE_GRID = 200                  # workgroups from which the planner takes 256-pixel tiles


# ------------------------------------------------------------------------------------------------------------ planner, restated
def desc1(N, H, W, K, Nc, **kw):
    """A 1x1 descriptor (pad 0)."""
    return desc(N, H, W, K, Nc, **kw)._replace(KH=1, KW=1, pad=0)


def _cdiv(a, b):
    return (a + b - 1) // b


def halo_maxhp(BM):
    return 400 if BM == 256 else 288 if BM == 128 else 160


def halo_geom(d, BM):
    """-> (TH, TI) or None: whole image rows (TH rows of one image) or TI whole images per tile."""
    W, H = d.OW, d.OH
    if BM % W:
        return None
    rows = BM // W
    if rows <= H:
        if H % rows:
            return None
        TH, TI = rows, 1
    else:
        if rows % H:
            return None
        TH, TI = H, rows // H
        if d.N % TI:
            return None
    return (TH, TI) if TI * (TH + 2) * (W + 2) <= halo_maxhp(BM) else None


def halo_ok(d):
    """-> (BM, CK) or None."""
    k3 = d.KH == 3 and d.KW == 3 and d.pad == 1
    k1 = d.KH == 1 and d.KW == 1 and d.pad == 0
    if not (k3 or k1) or d.stride != 1 or d.mode != 1:
        return None
    if d.IH != d.OH or d.IW != d.OW:
        return None
    if d.K % 32 or d.K1 % 32 or d.Nc % 4:
        return None
    M, nt = d.N * d.OH * d.OW, _cdiv(d.Nc, 128)
    if k1:
        return (256 if _cdiv(M, 256) * nt >= 200 else 128 if _cdiv(M, 128) * nt >= 400 else 64), 32
    if d.OW < 4 or d.OW > 64:
        return None
    best = 0
    for BM, need in ((256, 200), (128, 400), (64, 0)):
        if halo_geom(d, BM) is None:
            continue
        best = BM
        if _cdiv(M, BM) * nt >= need:
            break
    if not best:
        return None
    return best, (64 if best == 256 and d.K % 64 == 0 and d.K1 % 64 == 0 else 32)


def halo_w8(d, BM):
    """-> (TH, TI) of the 8-wave 128-pixel tile, or None."""
    b128 = _cdiv(d.N * d.OH * d.OW, 128) * _cdiv(d.Nc, 128)
    if d.KH == 3 and BM == 64 and d.K % 64 == 0 and d.K1 % 64 == 0 and b128 >= 200:
        return halo_geom(d, 128)
    return None


def halo_wide64(d, BM):
    return d.KH == 3 and BM == 64 and d.K % 64 == 0 and d.K1 % 64 == 0 and _cdiv(d.N * d.OH * d.OW, 64) * _cdiv(d.Nc, 128) <= 256


def fused_plan(d):
    """-> (BM, CK, TH) or None."""
    if d.KH != 3 or d.KW != 3 or d.pad != 1 or d.stride != 1 or d.mode != 1 or d.transposed:
        return None
    if d.IH != d.OH or d.IW != d.OW or d.K1 != d.K or d.K % 32 or d.Nc % 4 or d.OW < 4 or d.OW > 64:
        return None
    M, nt = d.N * d.OH * d.OW, _cdiv(d.Nc, 128)
    best = bth = 0
    for BM, need in ((256, 200), (128, 400), (64, 0)):
        g = halo_geom(d, BM)
        if g is None or g[1] != 1:
            continue
        best, bth = BM, g[0]
        if _cdiv(M, BM) * nt >= need:
            break
    if not best:
        return None
    ck = 64 if (d.K % 64 == 0 and (best == 256 or (best == 64 and _cdiv(M, 64) * nt <= 256))) else 32
    return best, ck, bth


def q_supported(d):
    return int(halo_ok(d) is not None)


def q_tile(d, io=0):
    """mi_conv3x3_bf16w_tile -> (BM, CK, sk) or None."""
    p = halo_ok(d)
    if p is None:
        return None
    BM, CK = p
    if halo_w8(d, BM):
        return 128, 64, 0
    return BM, (64 if halo_wide64(d, BM) else CK), 0


def q_fused_tile(d):
    p = fused_plan(d)
    return None if p is None else p[:2]


# ks: 3 or 1; inst: (ks, BM, CK, WAVES, N64, FUSE) -- IO is the seventh template argument a launch adds
Facts = namedtuple("Facts", "ks BM CK WAVES N64 FUSE TH TI HP tiles_per_img xmap qmap P Q skew gx gy grid nchunks")


def _skew(W, CK, BM, HP, TH, TI):
    if W not in (8, 16):
        return 0
    el, pitch = (14 if CK == 64 else 22) * 8, CK + 8
    return el if HP * pitch + TI * (TH + 2) * el <= halo_maxhp(BM) * pitch else 0


def _grid(d, ks, BM, TH, xmap):
    gx, gy = _cdiv(d.N * d.OH * d.OW, BM), _cdiv(d.Nc, 128)
    qmap = 0
    if ks == 3 and not xmap and gy > 1 and TH == d.OH and gy % 2 == 0 and gx % 4 == 0:
        qmap = 2
    if ks == 1 and gy > 1 and gx % 8 == 0:
        qmap = 1
    return gx, gy, qmap, ((gx * gy, 1, 1) if qmap else (gx, gy, 1))


def launch_facts(d, fused=False):
    """What halo_dispatch / fused_go and launch_halo derive for a descriptor the planner takes (None otherwise)."""
    if fused:
        p = fused_plan(d)
        if p is None:
            return None
        BM, CK, TH = p
        tpi = d.OH // TH
        xmap = tpi > 1 and d.N % 8 == 0
        HP = (TH + 2) * (d.OW + 2)
        gx, gy, qmap, grid = _grid(d, 3, BM, TH, xmap)
        return Facts(3, BM, CK, 8 if BM == 256 else 4, False, True, TH, 1, HP, tpi, xmap, qmap, 8 // qmap if qmap else 0, qmap, _skew(d.OW, CK, BM, HP, TH, 1),
                     gx, gy, grid, d.K // CK)
    p = halo_ok(d)
    if p is None:
        return None
    BM, CK = p
    if d.KH == 1:
        gx, gy, qmap, grid = _grid(d, 1, BM, 1, False)
        return Facts(1, BM, 32, 8 if BM == 256 else 4, False, False, 1, 1, BM, 1, False, qmap, 8 if qmap else 0, qmap, 0, gx, gy, grid, d.K // 32)
    TH, TI = halo_geom(d, BM)
    tpi = 1 if TI > 1 else d.OH // TH
    xmap = TI == 1 and tpi > 1 and d.N % 8 == 0
    WAVES, N64 = (8 if BM == 256 else 4), False
    w8 = halo_w8(d, BM)
    if w8:
        TH, TI = w8
        tpi = 1 if TI > 1 else d.OH // TH
        xmap = xmap and TI == 1 and tpi > 1
        BM, CK, WAVES = 128, 64, 8
    else:
        if halo_wide64(d, BM):
            CK = 64
        N64 = BM == 256 and CK == 64 and d.Nc <= 64
    HP = TI * (TH + 2) * (d.OW + 2)
    gx, gy, qmap, grid = _grid(d, 3, BM, TH, xmap)
    return Facts(3, BM, CK, WAVES, N64, False, TH, TI, HP, tpi, xmap, qmap, 8 // qmap if qmap else 0, qmap, _skew(d.OW, CK, BM, HP, TH, TI), gx, gy, grid,
                 d.K // CK)


def inst(f, io):
    return (f.ks, f.BM, f.CK, f.WAVES, f.N64, f.FUSE, io)


def plan_name(f):
    if f.ks == 1:
        return f"1x1<{f.BM}>"
    return ("FUSE" if f.FUSE else "") + f"<{f.BM},{f.CK}>" + ("w8" if f.WAVES == 8 and f.BM == 128 else "") + ("N64" if f.N64 else "")


def all_instantiations():
    """Every conv3x3_halo_kernel<BM, CK, KS, false, IO, WAVES, FUSE, false, N64> the product library can launch: seven 3x3 plans and two 1x1
    tiles times four storage modes, five fused tiles times two.  The 1x1 path never picks BM = 128: that needs b256 < 200 and b128 >= 400,
    but b128 = ceil(M / 128) nt <= 2 ceil(M / 256) nt = 2 b256 < 400."""
    s = set()
    for io in range(4):
        for BM, CK, WV, N64 in ((64, 32, 4, False), (64, 64, 4, False), (128, 32, 4, False), (128, 64, 8, False), (256, 64, 8, False), (256, 32, 8, False),
                                (256, 64, 8, True)):
            s.add((3, BM, CK, WV, N64, False, io))
        for BM in (64, 256):
            s.add((1, BM, 32, 8 if BM == 256 else 4, False, False, io))
    for io in (0, 3):
        for BM, CK in ((256, 64), (256, 32), (128, 32), (64, 64), (64, 32)):
            s.add((3, BM, CK, 8 if BM == 256 else 4, False, True, io))
    return s


for _M in range(1, 60000, 97):        # the arithmetic fact behind the missing 1x1 BM = 128, on a sweep
    for _nt in (1, 2, 3, 7):
        assert not (_cdiv(_M, 256) * _nt < 200 and _cdiv(_M, 128) * _nt >= 400)


def dispatch_accepts(d, io=0, has_x2=False, has_res=False, off=None, entry="io", ldy16=0, null=()):
    """halo_dispatch's argument conditions behind its entry points -> None when accepted, else a fragment of the message the refusal
    carries.  off: byte offsets from 16-byte alignment of x, x2, w, y, residual, bias, gsum, y16."""
    off = off or {}
    o = lambda k: off.get(k, 0)  # noqa: E731
    if entry == "io" and ("d" in null or d.KH not in (3, 1) or io & ~3):
        return "io in 0..3"
    if entry == "gnsums" and ("d" in null or d.KH != 3 or io & ~3 or "gsum" in null or d.Nc % 16 or (d.OH * d.OW) % 32):
        return "mi_conv3x3_bf16w_io_gnsums"
    if entry == "dual" and ("d" in null or d.KH not in (3, 1) or io & ~1 or "y16" in null or ldy16 % 4 or o("y16") % 8):
        return "mi_conv3x3_bf16w_io_dual"
    if {"d", "x", "w", "y"} & set(null):
        return "null argument"
    if halo_ok(d) is None:
        return "descriptor not supported by the halo kernel"
    if d.K1 != d.K and not has_x2:
        return "two-source split without x2"
    if d.ldx % 4 or (has_x2 and d.ldx2 % 4) or o("x") % 16 or (has_x2 and o("x2") % 16) or o("w") % 16:
        return "16-byte aligned with ld % 4 == 0"
    if d.ldy % 4 or (has_res and d.ldr % 4):
        return "ldy % 4 == 0"
    if o("y") % (8 if io & 2 else 16):
        return "y must be 16-byte aligned"
    if (has_res and o("res") % 16) or o("bias") % 16:
        return "residual and bias must be 16-byte aligned"
    if o("gsum") % 8:
        return "gsum must be 8-byte aligned"
    if d.KH == 3 and halo_geom(d, halo_ok(d)[0]) is None:
        return "halo tile geometry"
    return None


# ------------------------------------------------------------------------------------------------------------ cases
class _Case:
    def __repr__(self):
        return self.name


def _nt(name, fields, defaults):
    base = namedtuple(name, fields, defaults=defaults)
    return type(name, (_Case, base), {"__slots__": ()})


# plan: plan_name() of the launch this case is there for (held by tests/test_halo_cpu.py against the library); K1: channels of the first
# source (0: one source).  Pitches are fixed per family: ldx = K1 + 8, ldx2 = K - K1 + 24, ldy = Nc + 8, ldr = Nc + 4, ldy16 = Nc + 12.
Case = _nt("Case", "name plan N H W K Nc K1", (0,))
CASES_3X3 = [
    Case("w16_nonsquare_1chunk", "<64,32>", 2, 48, 16, 32, 64),              # non-square, one chunk, skew at W = 16
    Case("w8_3chunks_nc132", "<64,32>", 6, 8, 8, 96, 132, 32),               # three chunks, K1 at an odd chunk, a channel tile with 4 live columns, skew W = 8
    Case("ti4_one_tile", "<64,32>", 4, 4, 4, 32, 32),                        # four 4x4 images in the only tile
    Case("ti4_two_tiles_nc36", "<64,32>", 8, 4, 4, 32, 36),                  # two multi-image tiles, ragged Nc
    Case("wide64_xmap", "<64,64>", 8, 16, 16, 64, 64),
    Case("wide64_qmap_2chunks", "<64,64>", 16, 8, 8, 128, 256),              # whole-image tiles, (P, Q) = (4, 2)
    Case("w64_h4_xmap", "<128,32>", 8, 4, 64, 32, 64),
    Case("w64_h64_3chunks_nc68", "<128,32>", 1, 64, 64, 96, 68),
    Case("w64_h2_qmap", "<128,32>", 4, 2, 64, 32, 256),                      # whole-image 128-pixel tiles: (P, Q) = (4, 2) over 4 x 2 tiles
    Case("w8tile_th8", "<128,64>w8", 100, 16, 16, 64, 128),
    Case("w8tile_th4_xmap_two", "<128,64>w8", 32, 32, 32, 128, 128, 64),
    Case("w8tile_ti2", "<128,64>w8", 400, 8, 8, 64, 128),
    Case("t256", "<256,64>", 50, 32, 32, 64, 128),
    Case("t256_xmap_two", "<256,64>", 56, 32, 32, 128, 128, 64),
    Case("t256_qmap_w16", "<256,64>", 52, 16, 16, 64, 512),                  # TH = H, skew W = 16 at BM = 256
    Case("t256_ck32_1chunk", "<256,32>", 25, 32, 32, 32, 256),
    Case("t256_ck32_3chunks_two", "<256,32>", 25, 32, 32, 96, 256, 32),      # K1 = 32 of 96: the source switch at an odd chunk
    Case("n64", "<256,64>N64", 50, 32, 32, 64, 64),
    Case("n64_nc36_xmap", "<256,64>N64", 56, 32, 32, 64, 36),
    Case("t256_ti4", "<256,64>", 800, 8, 8, 64, 128),                        # four 8x8 images per tile
]
CASES_1X1 = [
    Case("k1_m105_1stage", "1x1<64>", 3, 7, 5, 32, 36),                      # M tail 105 % 64; stages 2..4 of the only group are zero-masked
    Case("k1_m105_3stages_two", "1x1<64>", 3, 7, 5, 96, 36, 32),
    Case("k1_m105_5stages_two", "1x1<64>", 3, 7, 5, 160, 36, 96),            # a partial second group
    Case("k1_t256", "1x1<256>", 200, 16, 16, 64, 128),
    Case("k1_t256_qmap_nc384", "1x1<256>", 200, 16, 16, 64, 384),
]
# the epilogue-sum entry: TI = 1 per-workgroup path (4- and 8-wave tiles), TI > 1 per-block path, N64; unit operands at K = 64
CASES_SUMS = [
    Case("sums_wide64", "<64,64>", 8, 16, 16, 64, 64), Case("sums_ti2_w4", "<64,64>", 4, 8, 4, 64, 48), Case("sums_t256", "<256,64>", 50, 32, 32, 64, 128),
    Case("sums_w8tile_ti2", "<128,64>w8", 400, 8, 8, 64, 128), Case("sums_n64", "<256,64>N64", 50, 32, 32, 64, 64), Case("sums_t256_ti4", "<256,64>", 800, 8, 8, 64, 128),
]
# fused: G groups; ldt elements added to K (-1: no time bias)
Fused = _nt("Fused", "name plan N H W K Nc G ldt", ())
FUSED_CASES = [
    Fused("fx_64x64_cg16", "FUSE<64,64>", 4, 16, 16, 64, 64, 4, 4), Fused("fx_64x32_cg32_xmap", "FUSE<64,32>", 8, 32, 32, 32, 64, 1, -1),
    Fused("fx_128x32_w64_cg16", "FUSE<128,32>", 8, 4, 64, 32, 64, 2, 4), Fused("fx_256x64_cg64", "FUSE<256,64>", 50, 32, 32, 64, 128, 1, 0),
    Fused("fx_256x32_cg32_nc256", "FUSE<256,32>", 25, 32, 32, 96, 256, 3, 4),
]
LD = dict(x=8, x2=24, y=8, r=4, y16=12)


def case_desc(c, flip=0, epi="", dense=False):
    """The descriptor of a case's launch: pitches of LD (dense: none), ldr only with a residual ('r' in epi), accumulate with 'a'."""
    K1 = c.K1 or c.K
    p = (lambda k: 0) if dense else LD.get
    mk = desc1 if c.plan.startswith("1x1") else desc
    return mk(c.N, c.H, c.W, c.K, c.Nc, K1=K1, ldx=K1 + p("x"), ldx2=(c.K - K1 + p("x2")) if c.K1 else 0, ldy=c.Nc + p("y"),
              ldr=(c.Nc + p("r")) if "r" in epi else 0, transposed=flip, accumulate=int("a" in epi))


def fused_desc(c):
    return desc(c.N, c.H, c.W, c.K, c.Nc, ldx=c.K + LD["x"], ldy=c.Nc + LD["y"])


def is_large(c):
    f = launch_facts(fused_desc(c), True) if isinstance(c, Fused) else launch_facts(case_desc(c))
    return f.grid[0] * f.grid[1] >= LARGE_GRID


def edges():
    """name -> the case names that reach it."""
    e = {}

    def hit(k, c):
        e.setdefault(k, []).append(c.name)

    for c in CASES_3X3 + CASES_1X1 + CASES_SUMS:
        d = case_desc(c)
        f = launch_facts(d)
        assert f is not None, c
        hit("plan:" + plan_name(f), c)
        for io in range(4):
            hit("inst:" + repr(inst(f, io)), c)
        if f.ks == 1:
            hit(f"k1:stages:{f.nchunks}", c)
            hit(f"k1:qmap:{f.qmap}", c)
            if (d.N * d.OH * d.OW) % f.BM:
                hit("k1:m_tail", c)
            if f.nchunks % 4:
                hit("k1:masked_stages", c)
            continue
        hit(f"map:{f.BM}:" + ("xmap" if f.xmap else "qmap" if f.qmap else "none"), c)
        hit("skew:" + (f"w{d.OW}" if f.skew else "off"), c)
        if f.TI > 1:
            hit("ti>1:" + ("one_tile" if f.gx == 1 else "tiles"), c)
        hit("chunks:" + ("1" if f.nchunks == 1 else "2" if f.nchunks == 2 else "odd" if f.nchunks % 2 else "even"), c)
        if c.K1 and (c.K1 // f.CK) % 2:
            hit("k1_odd_chunk", c)
        if d.Nc % 128 and d.Nc % 128 < 32:
            hit("nc_tile_under_32", c)
        if f.N64 and d.Nc < 64:
            hit("n64_nc_under_64", c)
        if f.tiles_per_img > 1:
            hit("row_tiles", c)
        if c in CASES_SUMS:
            hit("sums:" + ("n64" if f.N64 else f"ti{'1' if f.TI == 1 else '>1'}:waves{f.WAVES}"), c)
    for c in FUSED_CASES:
        f = launch_facts(fused_desc(c), True)
        assert f is not None, c
        hit("plan:" + plan_name(f), c)
        for io in (0, 3):
            hit("inst:" + repr(inst(f, io)), c)
        hit(f"fused:cg{c.K // c.G}", c)
        hit("fused:temb:" + ("none" if c.ldt < 0 else "dense" if c.ldt == 0 else "pitched"), c)
        hit("fused:map:" + ("xmap" if f.xmap else "qmap" if f.qmap else "none"), c)
    return e


REQUIRED_EDGES = tuple(
    ["inst:" + repr(i) for i in sorted(all_instantiations())]
    + [f"map:{bm}:{m}" for bm in (64, 128, 256) for m in ("xmap", "qmap", "none")]
    + ["skew:w8", "skew:w16", "skew:off", "ti>1:one_tile", "ti>1:tiles", "chunks:1", "chunks:2", "chunks:odd", "k1_odd_chunk", "nc_tile_under_32",
       "n64_nc_under_64", "row_tiles", "k1:stages:1", "k1:stages:3", "k1:stages:5", "k1:m_tail", "k1:masked_stages", "k1:qmap:0", "k1:qmap:1",
       "sums:ti1:waves4", "sums:ti1:waves8", "sums:ti>1:waves4", "sums:ti>1:waves8", "sums:n64",
       "fused:cg16", "fused:cg32", "fused:cg64", "fused:temb:none", "fused:temb:dense", "fused:temb:pitched", "fused:map:xmap", "fused:map:none"])


def random_descs(n, seed=11):
    """Descriptors around the planner's conditions: mostly valid values with off ones mixed in."""
    g = torch.Generator().manual_seed(seed)

    def pick(vals):
        return vals[int(torch.randint(0, len(vals), (1,), generator=g))]
    out = []
    for _ in range(n):
        W = pick([4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 3, 28, 65, 5])
        H = pick([1, 2, 3, 4, 6, 7, 8, 12, 16, 24, 32, 48, 64])
        N = pick([1, 2, 3, 4, 5, 6, 8, 16, 25, 50, 56, 64, 100, 128, 200, 400, 512, 800])
        K = pick([32, 64, 64, 96, 128, 128, 160, 192, 256, 512, 48])
        Nc = pick([4, 32, 36, 64, 64, 68, 128, 128, 132, 192, 256, 384, 512, 768, 30])
        K1 = pick([K, K, K, K, K, 32, 64, max(K - 32, 0), 96, 16])
        over = {}
        r = pick(list(range(40)))
        if r == 0:
            over["KH"] = pick([1, 5])
        elif r == 1:
            over["pad"] = 0
        elif r == 2:
            over["stride"] = 2
        elif r == 3:
            over["IH"] = H * 2
        elif r == 4:
            over["KW"] = 1
        elif r == 5:
            over["IW"] = W + 1
        elif r == 6:
            over["transposed"] = 1
        mode = pick([1, 1, 1, 1, 1, 1, 1, 0])
        mk = desc1 if pick([0, 0, 0, 1]) else desc
        out.append(mk(N, H, W, K, Nc, K1=K1, mode=mode, **over))
    # the refusals the issue names, always present
    out += [desc(2, 8, 3, 32, 32), desc(2, 8, 28, 32, 32), desc(2, 8, 65, 32, 32), desc(3, 6, 8, 32, 32), desc(3, 4, 4, 32, 32), desc(2, 8, 8, 48, 32),
            desc(2, 8, 8, 64, 32, K1=16), desc(2, 8, 8, 32, 30), desc(2, 8, 8, 32, 32, stride=2), desc(2, 8, 8, 32, 32, mode=0), desc(2, 8, 8, 32, 32, IH=16)]
    return out


# ------------------------------------------------------------------------------------------------------------ operands and references
def conv1_ref(x, G, x2=None, absolute=False):
    """The 1x1 form: y[m][j] = sum_k src[m][k] G[0][k][j] over one or two sources; absolute: over the absolute values of the terms."""
    a = (lambda t: t.to(F64).abs()) if absolute else (lambda t: t.to(F64))
    src = a(x) if x2 is None else torch.cat([a(x), a(x2)], dim=-1)
    N, H, W, K = src.shape
    return (src.reshape(-1, K) @ a(G[0])).view(N, H, W, -1)


def operands(c, kind, flip=False):
    """x (and x2), the contraction-first weights G [taps][K][Nc] (asymmetric: independent values per tap), and the epilogue's operands:
    bias, residual, prior content.  kind 'int': x in {-4..4}, w in {-3..3}; 'unit': {-1, 0, 1}; 'randn': bf16-representable normals."""
    K1 = c.K1 or c.K
    taps = 1 if c.plan.startswith("1x1") else 9
    key = (c.name, kind, bool(flip))
    sh = (c.N, c.H, c.W)
    return dict(x=operand(sh + (K1,), kind, seed(key, "x"), bf16=True),
                x2=operand(sh + (c.K - K1,), kind, seed(key, "x2"), bf16=True) if c.K1 else None,
                G=operand((taps, c.K, c.Nc), kind, seed(key, "w"), bf16=True, amp=3, scale=(taps * c.K) ** -0.5),
                bias=operand((c.Nc,), kind, seed(key, "b")), res=operand(sh + (c.Nc,), kind, seed(key, "r")),
                prior=init_content(sh + (c.Nc,), seed(key, "p"), kind))


def base_reference(c, ops, flip=False, absolute=False):
    """The convolution alone, float64 (bias, residual and prior content are added per variant by the caller)."""
    if c.plan.startswith("1x1"):
        return conv1_ref(ops["x"], ops["G"], ops["x2"], absolute)
    return conv_ref(ops["x"], ops["G"], flip, ops["x2"], absolute=absolute)


def halo_weights(G):
    """Contraction-first G [taps][K][Nc] -> the kernel's operand [tap][n][k] (what mi_pack_weights_bf16 writes as Wf, or Wd for the data
    gradient, whose contraction-first operand is dgrad_operand(master))."""
    return G.transpose(1, 2).contiguous()


def int_family_exact(K, taps=9):
    """|x| <= 4, |w| <= 3: every partial sum of taps K products plus bias, residual and prior content (at most 4 each) is an integer below 2^24."""
    return taps * K * 12 + 12 < 2 ** 24


def sums_operands(c, out16):
    """Unit operands at K = 64 plus a sparse large residual (300 on one pixel in sixteen of each slab's first channel): values above 256 are
    what a bf16 output rounds, so sums taken before the rounding differ from sums of the stored values."""
    assert c.K == 64
    ops = operands(c, "unit")
    big = torch.zeros(c.N, c.H * c.W, c.Nc, dtype=F64)
    big[:, ::16, ::16] = 300.0
    ops["res"] = ops["res"] + big.view(c.N, c.H, c.W, c.Nc)
    return ops


def fused_operands(c, x_f32=False, border_tap=None):
    """x: the raw conv output the kernel normalises, its fixed-point slab sums, gamma / beta, temb [N][K] or None, the coefficients
    (sc, sh, tb) of the rounding model (non-zero shift and time bias), G, bias.  border_tap: integer weights in {-3..3}, one in eight
    non-zero, on that tap alone and no bias (tap = ky 3 + kx: 1 top, 3 left, 5 right, 7 bottom)."""
    N, H, W, K = c.N, c.H, c.W, c.K
    x = (randn((N, H, W, K), seed(c.name, "x", x_f32)) * 1.3 + 0.2).to(F32).to(F64)
    x = x if x_f32 else bf16_round(x)
    gamma, beta = randn((K,), seed(c.name, "g")) * 0.5 + 1, randn((K,), seed(c.name, "be")) * 0.2 + 0.3
    temb = (randn((N, K), seed(c.name, "t")) * 0.3 + 0.5) if c.ldt >= 0 else None
    sums = gn_sums(x)
    sc, sh, tb = coef_from_sums(sums, H * W, K, c.G, GN_EPS, gamma, beta, temb)
    if border_tap is None:
        G = randn((9, K, c.Nc), seed(c.name, "w"), bf16=True, scale=(9 * K) ** -0.5)
        bias = randn((c.Nc,), seed(c.name, "b"))
    else:
        G = torch.zeros(9, K, c.Nc, dtype=F64)
        G[border_tap] = ints((K, c.Nc), -3, 3, seed(c.name, "wb", border_tap)) * (ints((K, c.Nc), 0, 7, seed(c.name, "thin")) == 0)
        bias = None
    return dict(x=x, sums=sums, gamma=gamma, beta=beta, temb=temb, sc=sc, sh=sh, tb=tb, G=G, bias=bias)


def fused_reference64(ops, c):
    """Unrounded float64: conv(mish(groupnorm(x) gamma + beta) + temb) + bias, statistics from the same sums."""
    N, K, cg = ops["x"].shape[0], c.K, c.K // c.G
    tot = ops["sums"].view(N, c.G, cg // 16, 2).sum(2).to(F64) / (GSUM_SCALE * c.H * c.W * cg)
    mean = tot[..., 0]
    rstd = 1.0 / torch.sqrt((tot[..., 1] - mean * mean).clamp_min(0.0) + GN_EPS)
    sc = rstd.repeat_interleave(cg, 1) * ops["gamma"][None]
    sh = ops["beta"][None] - mean.repeat_interleave(cg, 1) * sc
    tb = ops["temb"] if ops["temb"] is not None else torch.zeros_like(sc)
    return conv_ref(fused_h(ops["x"], sc, sh, tb, rounded=False), ops["G"], bias=ops["bias"])


def halo_h_emul32(x, sc, sh, tb, emu_seed=0, beta=None, G=1):
    """The halo kernel's staging in float32: z = fma(x, scale, shift), mish_fast_f (exp and rcp with a 2^-21 relative error), + tb, one
    rounding to bf16.  beta given: the sums form, whose rstd comes from the approximate reciprocal square root -- 2^-21 off per sample and
    group, so scale' = scale (1 + e) and shift' = beta - mean scale' = shift + e (shift - beta)."""
    em = NO._Emu(emu_seed)
    scf, shf = sc.to(F32), sh.to(F32)
    if beta is not None:
        N, K = sc.shape
        e = 2.0 ** -21 * (2.0 * torch.rand((N, G), generator=em.g, dtype=F64) - 1.0)
        e = e.repeat_interleave(K // G, 1)
        scf, shf = (sc * (1.0 + e)).float(), (sh + e * (sh - beta.to(F64)[None])).float()
    z = NO._fma(x.to(F32), scf[:, None, None, :].expand_as(x), shf[:, None, None, :].expand_as(x))
    o = em.mish_fast(z) + tb.to(F32)[:, None, None, :]
    return bf16_round(o)
