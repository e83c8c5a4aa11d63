"""CPU oracle of conv_pw_kernel's 3x3 entry points (csrc/conv_pw.hip): the default 3x3 convolution and data gradient of every
bf16-stored layer, its GroupNorm-sums epilogue, its fp32-input and exact-fp32 forms, the fused GroupNorm + Mish variants and split-K.

Shared by tests/test_conv_pw_cpu.py and tests/test_conv_pw_kernels_gpu.py:
  * float64 references on NHWC tensors: the forward conv over one or two sources, the data gradient (flipped taps against the wdq-order
    operand), then bias, fp32 residual and accumulate; the same sums over |terms| for the per-element bound;
  * the four fragment layouts of include/mi_ddpm.h (wfq, wdq, wfq32, wdq32) built in torch from the master layout [tap][ci][co];
  * a restatement of the host planner (pw_geom, pw_ok, pw_split, pw_pick_tile) and of the launch facts that select code paths;
  * the rounding models (bf16 round to nearest even; x rounded once for the fp32-input form; h = bf16(mish(x scale + shift) + tb) per
    staged element for the fused variants, coefficients given or resolved from the 20-fraction-bit sums) and a float32 emulation of the
    kernel's form of Mish (e = 2^t, q = e (e + 2) + 2, r = 1 / q with a 2^-21 relative error on exp and rcp);
  * the case lists, and edges(): which instantiations and dispatch edges those lists reach, by name.
The rules are read from the .hip file and written again here; nothing is imported from the package."""
import math
import os
import sys
import zlib
from collections import namedtuple

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _norm_oracle as NO  # noqa: E402

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
GSUM_SCALE = 1048576.0            # csrc/common.h MI_GSUM_SCALE: 20 fraction bits
SK_FLAG_BYTES = 64 * 1024         # PW_SK_FLAG_BYTES
# worst per-element distance of conv(h of the float32 emulation) from conv(h of the rounding model), relative to sum |h| |w| + |bias|, over
# the fused cases, both storages of x and eight seeds (re-measured and held in tests/test_conv_pw_cpu.py: 3.1e-5, rounded up for another
# CPU's exp.  The GPU test allows the kernel four times as much, whatever the parameters)
FUSED_EMUL_FIGURE = 3.5e-5
LOG2E_F32 = 1.44269504            # the constants of coef_landed / mish_tb2, as float32 literals
LN2_F32, M2LN2_F32 = 0.693147182, -1.38629436


# ------------------------------------------------------------------------------------------------------------ numbers, operands
def bf16_round(t):
    """Round to nearest even onto bf16, returned as float64 (t holds float32-representable values)."""
    return t.to(F32).to(BF).to(F64)


def rel(got, ref):
    got, ref = got.detach().to(F64).cpu().reshape(-1), ref.detach().to(F64).cpu().reshape(-1)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).to(F64)


def randn(shape, seed, bf16=False, scale=1.0):
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F32) * scale
    return bf16_round(t) if bf16 else t.to(F64)


def operand(shape, kind, seed, bf16=False, amp=4, scale=1.0):
    """kind 'int': integers in {-amp..amp} (exact in fp32 and bf16); 'unit': {-1, 0, 1}; 'randn': normal values (bf16 when stored so)."""
    if kind == "int":
        return ints(shape, -amp, amp, seed)
    if kind == "unit":
        return ints(shape, -1, 1, seed)
    return randn(shape, seed, bf16, scale)


def init_content(shape, seed, kind="int"):
    """What a += output holds before the launch: non-zero small integers ({-3..3} \\ {0}), or bf16-representable normal values (both
    storages then start from the same numbers)."""
    if kind in ("int", "unit"):
        return ints(shape, 1, 3, seed) * (ints(shape, 0, 1, seed + 1) * 2 - 1)
    return randn(shape, seed, bf16=True)


# ------------------------------------------------------------------------------------------------------------ references
def _padded(x):
    N, H, W, C = x.shape
    xp = torch.zeros(N, H + 2, W + 2, C, dtype=F64)
    xp[:, 1:1 + H, 1:1 + W] = x
    return xp


def conv_ref(x, G, flip=False, x2=None, bias=None, res=None, prior=None, absolute=False):
    """y[n][oy][ox][j] = bias[j] + res + prior + sum_{ky,kx,k} src[n][oy + ky - 1][ox + kx - 1][k] G[tap'][k][j], tap' = ky 3 + kx, or
    8 - (ky 3 + kx) with flip (the data gradient: G is then the wdq-order operand, [tap][co][ci] of the master weights).  src channel k
    comes from x for k < K1 and from x2 at k - K1.  absolute: the same sum over the absolute values of its terms."""
    a = (lambda t: t.to(F64).abs()) if absolute else (lambda t: t.to(F64))
    src = a(x) if x2 is None else torch.cat([a(x), a(x2)], dim=-1)
    N, H, W, K = src.shape
    assert G.shape[0] == 9 and G.shape[1] == K
    xp = _padded(src)
    y = torch.zeros(N * H * W, G.shape[2], dtype=F64)
    for ky in range(3):
        for kx in range(3):
            t = ky * 3 + kx
            y += xp[:, ky:ky + H, kx:kx + W].reshape(N * H * W, K) @ a(G[8 - t if flip else t])
    y = y.view(N, H, W, -1)
    for extra in (bias, res, prior):
        if extra is not None:
            y = y + a(extra)
    return y


def dgrad_operand(Wm):
    """Master weights [tap][ci][co] -> the contraction-first operand [tap][co][ci] of the data gradient (conv_ref(..., flip=True))."""
    return Wm.transpose(1, 2).contiguous()


# ------------------------------------------------------------------------------------------------------------ fragment layouts
def _lanes(step, half):
    lane = torch.arange(64)
    return lane & 31, half * (lane >> 5), torch.arange(half), step


def wfq(Wm, f32=False):
    """include/mi_ddpm.h: wfq[tap][co/32][ci/16][lane][8] = W[tap][ci = 16 kq + 8 (lane >> 5) + e][co = 32 nb + (lane & 31)]; f32:
    wfq32[tap][co/32][ci/8][lane][4] = W[tap][ci = 8 ko + 4 (lane >> 5) + j][co = 32 nb + (lane & 31)].  Wm: [tap][ci][co]."""
    T, ci, co = Wm.shape
    lo, hi, e, step = _lanes(8 if f32 else 16, 4 if f32 else 8)
    kq, nb = torch.arange(ci // step), torch.arange(co // 32)
    ci_idx = step * kq[None, :, None, None] + hi[None, None, :, None] + e[None, None, None, :]
    co_idx = 32 * nb[:, None, None, None] + lo[None, None, :, None]
    return Wm[:, ci_idx, co_idx].contiguous()


def wdq(Wm, f32=False):
    """wdq[tap][ci/32][co/16][lane][8] = W[tap][ci = 32 nb + (lane & 31)][co = 16 kq + 8 (lane >> 5) + e]; f32:
    wdq32[tap][ci/32][co/8][lane][4] = W[tap][ci = 32 nb + (lane & 31)][co = 8 ko + 4 (lane >> 5) + j]."""
    T, ci, co = Wm.shape
    lo, hi, e, step = _lanes(8 if f32 else 16, 4 if f32 else 8)
    kq, nb = torch.arange(co // step), torch.arange(ci // 32)
    ci_idx = 32 * nb[:, None, None, None] + lo[None, None, :, None]
    co_idx = step * kq[None, :, None, None] + hi[None, None, :, None] + e[None, None, None, :]
    return Wm[:, ci_idx, co_idx].contiguous()


def frag_operand(G, flip, f32=False):
    """The fragment-order tensor a launch with contraction-first operand G [tap][K][Nc] reads: wfq of the master weights G for the forward
    conv, wdq of the master weights G^T for the data gradient."""
    return wdq(G.transpose(1, 2).contiguous(), f32) if flip else wfq(G, f32)


# ------------------------------------------------------------------------------------------------------------ planner, restated
_DESC = ("N", "IH", "IW", "OH", "OW", "K", "Nc", "KH", "KW", "stride", "pad", "transposed", "w_kn", "mode", "K1", "ldx", "ldx2", "ldy", "ldr",
         "accumulate")
Desc = namedtuple("Desc", _DESC)


def desc(N, H, W, K, Nc, K1=None, ldx=None, ldx2=None, ldy=None, ldr=0, transposed=0, accumulate=0, mode=1, **over):
    K1 = K if K1 is None else K1
    d = dict(N=N, IH=H, IW=W, OH=H, OW=W, K=K, Nc=Nc, KH=3, KW=3, stride=1, pad=1, transposed=transposed, w_kn=0, mode=mode, K1=K1,
             ldx=K1 if ldx is None else ldx, ldx2=(K - K1 if K1 != K else 0) if ldx2 is None else ldx2, ldy=Nc if ldy is None else ldy, ldr=ldr,
             accumulate=accumulate)
    d.update(over)
    return Desc(**d)


def pw_xp(pt):
    return 320 if pt == 256 else 192 if pt == 128 else 128


def pw_lds(pt, raw=False):
    return (128 if pt == 256 else (72 if raw else 64) if pt == 128 else (48 if raw else 32)) * 1024 + 2048


def pw_geom(d, pt):
    """-> (TH, TI) or None."""
    W, H = d.OW, d.OH
    if W not in (8, 16, 32):
        return None
    rows, bh = pt // W, pt // 32
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
    if (TH & (TH - 1)) or TH % bh or TI > 2:
        return None
    if pt == 256 and TI > 1:
        return None
    return (TH, TI) if TI * (TH + 2) * W <= pw_xp(pt) else None


def pw_ok(d, pt, in32=False, f32=False):
    if d.KH != 3 or d.KW != 3 or d.pad != 1 or d.stride != 1 or d.mode != (0 if f32 else 1):
        return None
    if d.IH != d.OH or d.IW != d.OW:
        return None
    lda, ck = (4 if (in32 or f32) else 8), (32 if f32 else 64)
    if d.K % 64 or d.K1 % ck or d.Nc % 64 or d.ldx % lda or (d.K1 != d.K and d.ldx2 % lda):
        return None
    if (d.N * d.OH * d.OW) % pt:
        return None
    if d.Nc * d.K * (4 if f32 else 2) * 9 >= 1 << 31:
        return None
    return pw_geom(d, pt)


class Knobs(namedtuple("Knobs", "force sk_mode ws_bytes")):
    """The library's state a plan depends on: the forced tile (mi_debug_conv_pw_tile), the split mode (mi_debug_conv_pw_splitk) and the
    bytes of the registered split-K workspace (0: none -- what a process without a device sees)."""


DEFAULT = Knobs(0, 1, 0)


def pw_split(d, var, in32, kn):
    """-> (ks, pt, TH, TI, need bytes); ks == 1: no split (the other fields are then meaningless)."""
    none = (1, 0, 0, 0, 0)
    if not kn.sk_mode or not kn.ws_bytes:
        return none
    cand = kn.force
    if cand == 256:
        return none
    if not cand:
        g = pw_ok(d, 128, in32)
        cand = 128 if (g and (var < 2 or g[1] == 1)) else 64
    g = pw_ok(d, cand, in32)
    if not g or (var >= 2 and g[1] != 1):
        return none
    tiles = (d.N * d.OH * d.OW // cand) * ((d.Nc + 127) // 128)
    nch = d.K // 64
    ks = 1
    if kn.sk_mode >= 2:
        ks = kn.sk_mode
    elif tiles < 200 and nch >= 16:
        ks = 2 if tiles * 2 >= 256 else 4
    while ks > 1 and (nch % ks or nch // ks < 2):
        ks >>= 1
    if ks <= 1:
        return none
    need = SK_FLAG_BYTES + (ks - 1) * tiles * cand * 128 * 4
    if (ks - 1) * tiles * 4 * 4 > SK_FLAG_BYTES or need > kn.ws_bytes:
        return none
    return ks, cand, g[0], g[1], need


def pw_pick_tile(d, var, in32=False, f32=False, kn=DEFAULT, split=False):
    """-> (pt, TH, TI, ks); pt == 0: not supported.  split: the caller asks for a split plan (launches and mi_conv3x3_pw_splitk do)."""
    no = (0, 0, 0, 1)
    if f32 and var != 0:
        return no
    if var >= 2 and d.K > 1024:
        return no
    if not f32 and split:
        ks, pts, TH, TI, _ = pw_split(d, var, in32, kn)
        if ks > 1:
            return pts, TH, TI, ks
    if kn.force in (64, 128):
        g = pw_ok(d, kn.force, in32, f32)
        return (kn.force, g[0], g[1], 1) if g else no
    if kn.force == 256:
        g = pw_ok(d, 256) if (var < 2 and not in32 and not f32) else None
        return (256, g[0], g[1], 1) if g else no
    t128 = (d.N * d.OH * d.OW // 128) * ((d.Nc + 127) // 128)
    g = pw_ok(d, 64, in32, f32)
    if t128 < 200 and g and (var < 2 or g[1] == 1):
        return 64, g[0], g[1], 1
    g = pw_ok(d, 128, in32, f32)
    return (128, g[0], g[1], 1) if g else no


def q_supported(d, kn=DEFAULT, in32=False):
    return int(pw_pick_tile(d, 0, in32, False, kn)[0] != 0)


def q_tile(d, kn=DEFAULT, in32=False, f32=False):
    return pw_pick_tile(d, 0, in32, f32, kn)[0]


def q_fused_tile(d, kn=DEFAULT, in32=False):
    pt, _, TI, _ = pw_pick_tile(d, 2, in32, False, kn)
    return pt if (pt and TI == 1 and d.K1 == d.K) else 0


def q_splitk(d, var, in32, kn=DEFAULT):
    pt, _, _, ks = pw_pick_tile(d, var, bool(in32), False, kn, split=True)
    return (pt << 4) | ks if pt else 1


Facts = namedtuple("Facts", "pt TH TI ks tiles_per_img XP xmap qmap gx gy cpq nch chunks tile16 idle grid inst lds")


def launch_facts(d, var, out16, has_res=False, in32=False, f32=False, kn=DEFAULT):
    """What pw_launch derives for a descriptor the planner takes (None otherwise): the facts that select code paths in the kernel."""
    pt, TH, TI, ks = pw_pick_tile(d, var, in32, f32, kn, split=True)
    if not pt:
        return None
    tpi = 1 if TI > 1 else d.OH // TH
    xmap = TI == 1 and tpi > 1 and d.N % 8 == 0
    gx, gy = d.N * d.OH * d.OW // pt, (d.Nc + 127) // 128
    qmap = (not xmap) and gy > 1 and gy % 2 == 0 and gx % 4 == 0
    nch = d.K // (32 if f32 else 64)
    lds = pw_lds(pt, in32 and var < 2)
    if var >= 2:
        lds = max(lds, 2 * pw_xp(pt) * 128 + 2048 + 12 * d.K)
    return Facts(pt, TH, TI, ks, tpi, TI * (TH + 2) * d.OW, xmap, qmap, gx, gy, gy // 2, nch, nch // ks,
                 bool(out16) and not has_res and not d.accumulate, d.Nc % 128 == 64, gx * gy * ks,
                 (bool(out16), var, pt, bool(in32), bool(f32)), lds)


def all_instantiations():
    """Every <OUT16, VAR, PT, IN32, F32> pw_launch's switch can reach."""
    s = {(False, 0, pt, False, True) for pt in (64, 128)}
    for o16 in (False, True):
        for var in (0, 1, 2, 3):
            for pt in (64, 128):
                s.add((o16, var, pt, False, False))
                s.add((o16, var, pt, True, False))
        for var in (0, 1):
            s.add((o16, var, 256, False, False))
    return s


def launch_accepts(d, var, out16, kn=DEFAULT, in32=False, f32=False, x_off=0, x2_off=0, w_off=0, null=(), coef_off=0, G=0, gn_off=(0, 0, 0, 0),
                   ldt=0, has_temb=False, has_x2=False, has_res=False):
    """pw_launch's argument conditions, in its order.  null: names of null arguments among d, x, w, y, coef, gsum, sums, gamma, beta."""
    if {"d", "x", "w", "y"} & set(null):
        return False
    pt, TH, TI, ks = pw_pick_tile(d, var, in32, f32, kn, split=True)
    if not pt:
        return False
    if d.K1 != d.K and not has_x2:
        return False
    if x_off % 16 or w_off % 16 or (has_x2 and x2_off % 16):
        return False
    if d.ldy % 8 or (has_res and d.ldr % 4):
        return False
    if var >= 2 and (TI != 1 or d.K1 != d.K):
        return False
    if var == 2 and ("coef" in null or coef_off % 16):
        return False
    if var == 3:
        if {"sums", "gamma", "beta"} & set(null) or G <= 0 or d.K % G or d.K // G not in (16, 32, 64):
            return False
        so, go, bo, to = gn_off
        if go % 8 or bo % 8 or so % 16 or (has_temb and (to % 16 or ldt % 4)):
            return False
    if var == 1 and ("gsum" in null or d.Nc % 16):
        return False
    if f32 and out16:
        return False
    return True


# ------------------------------------------------------------------------------------------------------------ rounding models
def mish64(z):
    return NO.mish(z.to(F64))


def f32r(t):
    return t.to(F32).to(F64)


def coef_from_sums(sums, HW, K, G, eps, gamma, beta, temb=None):
    """mi_gn_coef_from_sums' arithmetic, as conv_pw_kernel's prologue (stats_landed, coef_landed) restates it: integer slab sums, mean and
    var = E[x^2] - mean^2 in double (clamped at 0), rstd = 1 / sqrtf((float)var + eps), scale = gamma rstd, shift = beta - (float)mean scale
    in float32.  sums: int64 [N][K / 16][2].  -> scale, shift, tb [N][K] (float32 values as float64)."""
    N = sums.shape[0]
    cg = K // G
    tot = sums.view(N, G, cg // 16, 2).sum(2).to(F64) * (1.0 / (GSUM_SCALE * HW * cg))
    mean = tot[..., 0]
    var = (tot[..., 1] - mean * mean).clamp_min(0.0)
    rstd = (1.0 / torch.sqrt(var.to(F32) + torch.tensor(eps, dtype=F32))).to(F32)
    sc = gamma.to(F32)[None] * rstd.repeat_interleave(cg, 1)
    sh = NO._fma(-mean.to(F32).repeat_interleave(cg, 1), sc, beta.to(F32)[None].expand_as(sc))
    tb = temb.to(F32) if temb is not None else torch.zeros(N, K, dtype=F32)
    return sc.to(F64), sh.to(F64), tb.to(F64)


def gn_sums(x):
    """x [N][H][W][C] (stored values) -> the epilogue's fixed-point sums [N][C / 16][2] int64."""
    N, C = x.shape[0], x.shape[-1]
    xd = x.to(F64).reshape(N, -1, C // 16, 16)
    s = torch.stack([xd.sum((1, 3)), (xd * xd).sum((1, 3))], dim=-1)
    return torch.round(s * GSUM_SCALE).to(torch.int64)


def fused_h(x, sc, sh, tb, rounded=True):
    """h = bf16(mish(x scale + shift) + tb) per element of x [N][H][W][K] (coefficients [N][K]); rounded False: unrounded float64."""
    z = x.to(F64) * sc[:, None, None, :] + sh[:, None, None, :]
    h = mish64(z) + tb[:, None, None, :]
    return bf16_round(h) if rounded else h


def fused_h_emul32(x, sc, sh, tb, seed=0):
    """The kernel's float32 arithmetic (coef_landed, mish_tb2): scale and shift times log2(e), t = fma(x, sc, sh), e = 2^t, q = fma(e, e + 2, 2),
    r = 1 / q, s = fma(r, -2 ln 2, ln 2), o = fma(t, s, tb); exp and rcp carry a 2^-21 relative error; then one rounding to bf16."""
    em = NO._Emu(seed)
    l2 = torch.tensor(LOG2E_F32, dtype=F32)
    scl, shl = (sc.to(F32) * l2)[:, None, None, :], (sh.to(F32) * l2)[:, None, None, :]
    t = NO._fma(x.to(F32), scl.expand_as(x), shl.expand_as(x))
    e = NO._pert(torch.exp2(t.double()), em.g)
    e = torch.where(torch.isinf(e), torch.full_like(e, float("inf")), e)
    two = torch.full_like(e, 2.0)
    q = NO._fma(e, e + 2.0, two)
    r = NO._pert(1.0 / q.double(), em.g)
    s = NO._fma(r, torch.full_like(r, M2LN2_F32), torch.full_like(r, LN2_F32))
    o = NO._fma(t, s, tb.to(F32)[:, None, None, :].expand_as(t))
    return bf16_round(o)


# ------------------------------------------------------------------------------------------------------------ cases
class _Case:
    def __repr__(self):
        return self.name


def _nt(name, fields, defaults):
    base = namedtuple(name, fields, defaults=defaults)
    return type(name, (_Case, base), {"__slots__": ()})


# pt: the tile forced with mi_debug_conv_pw_tile (0: the automatic pick); K1: channels of the first source (0: one source);
# ldx / ldx2 / ldy / ldr: elements ADDED to the dense pitch; epi: "", "b", "br", "a", "ba", "ra", "bra" (bias, residual, accumulate)
Plain = _nt("Plain", "name N H W K Nc pt K1 ldx ldx2 ldy ldr epi", (0, 0, 0, 0, 0, "b"))


def _geometry_cases():
    rows = [(32, 64, 2), (32, 128, 4), (32, 128, 8), (32, 256, 8), (32, 256, 16), (16, 64, 2), (16, 64, 4), (16, 64, 12), (16, 128, 4), (16, 128, 8),
            (16, 128, 48), (16, 256, 16), (8, 64, 4), (8, 64, 8), (8, 64, 24), (8, 128, 8), (8, 128, 16), (8, 128, 32), (8, 256, 32)]
    out = []
    for W, pt, H in rows:
        N = 2                                                # (two images: TI == 2 tiles hold both, TI == 1 tiles cross an image border)
        while (N * H * W) % pt:
            N += 2
        out.append(Plain(f"geo_w{W}_t{pt}_h{H}", N, H, W, 64, 64, pt))
    return out


GEOMETRY_CASES = _geometry_cases()
BATCH_CASES = [
    Plain("batch_ti2_n2", 2, 8, 8, 64, 64, 128), Plain("batch_ti2_n6", 6, 8, 8, 64, 64, 128), Plain("batch_ti2_w16_n6", 6, 2, 16, 64, 64, 64),
    Plain("batch_xmap_n8", 8, 16, 16, 64, 64, 128), Plain("batch_xmap_n8_t64", 8, 8, 16, 64, 128, 64),
    Plain("batch_n3", 3, 16, 16, 64, 64, 128), Plain("batch_n5", 5, 8, 32, 64, 64, 64),
]
CHANNEL_CASES = [
    Plain("ch_k128", 2, 8, 8, 128, 64, 128), Plain("ch_k192", 2, 8, 8, 192, 64, 64), Plain("ch_k320", 2, 8, 8, 320, 128, 128),
    Plain("ch_k1024", 2, 8, 8, 1024, 64, 128),
    Plain("ch_two_k1_64", 2, 8, 8, 192, 64, 128, 64), Plain("ch_two_k1_k_64", 2, 8, 8, 192, 64, 64, 128), Plain("ch_two_k320", 4, 4, 16, 320, 128, 128, 256),
    Plain("ch_nc128", 2, 8, 8, 64, 128, 128), Plain("ch_nc192", 2, 8, 8, 64, 192, 128), Plain("ch_nc192_t64", 2, 8, 8, 128, 192, 64),
    Plain("ch_nc256_qmap", 8, 8, 8, 64, 256, 128), Plain("ch_nc768_qmap", 4, 8, 8, 64, 768, 64), Plain("ch_nc256_gx2", 4, 8, 8, 64, 256, 128),
    Plain("ch_nc256_gx6", 6, 8, 8, 64, 256, 64), Plain("ch_nc384", 8, 8, 8, 64, 384, 128),
]
PITCH_CASES = [
    Plain("pitch_ldx", 2, 8, 16, 128, 64, 128, 0, 8), Plain("pitch_ldx2", 2, 8, 16, 192, 64, 128, 64, 8, 24),
    Plain("pitch_ldy8", 2, 8, 16, 64, 192, 64, 0, 0, 0, 8), Plain("pitch_ldy64_ldr", 2, 8, 16, 64, 64, 128, 0, 0, 0, 64, 4, "br"),
    Plain("pitch_all", 2, 4, 32, 128, 128, 128, 64, 8, 24, 8, 4, "bra"),
]
EPILOGUE_CASES = [Plain(f"epi_{e or 'none'}", 2, 8, 16, 128, 192, 128, 0, 0, 0, 8, 4, e) for e in ("", "b", "r", "br", "a", "ba", "ra", "bra")]
PLAIN_CASES = GEOMETRY_CASES + BATCH_CASES + CHANNEL_CASES + PITCH_CASES + EPILOGUE_CASES

# GroupNorm sums from the epilogue: TI 1 / 2, 256-pixel tiles, Nc 192 (the slab guard) and 64, fp32 and bf16 output; through _pw_x32 too
def Gns(name, N, H, W, K, Nc, pt, epi="b"):
    return Plain(name, N, H, W, K, Nc, pt, epi=epi)


GNS_CASES = [
    Gns("gns_ti1_t128", 2, 8, 16, 64, 128, 128), Gns("gns_ti1_t64", 2, 8, 16, 64, 64, 64, "br"), Gns("gns_ti2_t128", 4, 8, 8, 64, 192, 128),
    Gns("gns_ti2_t64_w16", 4, 2, 16, 64, 128, 64), Gns("gns_ti2_t64_w8", 4, 4, 8, 64, 192, 64, ""), Gns("gns_t256", 2, 16, 16, 64, 192, 256),
    Gns("gns_t256_w32", 1, 16, 32, 64, 64, 256, "ba"), Gns("gns_tiles3", 2, 12, 16, 64, 128, 64),
]

# the fp32-input and exact-fp32 forms: ldx in floats (+ 4)
X32_CASES = [
    Plain("x32_t128", 2, 8, 16, 128, 128, 128, 0, 4), Plain("x32_t64_two", 2, 8, 8, 192, 64, 64, 64, 4, 4, 8, 4, "br"),
    Plain("x32_ti2", 2, 8, 8, 64, 192, 128, 0, 0, 0, 0, 0, "ba"), Plain("x32_w32", 2, 4, 32, 64, 64, 64, 0, 4),
]
F32_CASES = [
    Plain("f32_t128", 2, 8, 16, 128, 128, 128, 0, 4), Plain("f32_t64_two", 2, 8, 8, 192, 64, 64, 96, 4, 4, 8, 4, "br"),
    Plain("f32_ti2", 2, 8, 8, 64, 192, 128, 0, 0, 0, 0, 0, "ba"), Plain("f32_w32_k1_32", 2, 4, 32, 128, 64, 64, 32, 0, 4),
]

# fused GroupNorm + Mish: params "plain" (gamma = randn 0.5 + 1, beta = randn 0.2), "wide" (gamma = 4 randn + 1, beta = 10 randn),
# "const" (plain with sample 1 constant: rstd = 1 / sqrt(eps)); ldt: elements added to K (-1: no time bias)
Fused = _nt("Fused", "name N H W K G Nc pt ldt params bias", (0, "plain", True))
FUSED_CASES = [
    Fused("fx_w16_t64_cg16", 2, 8, 16, 64, 4, 64, 64), Fused("fx_w16_t128_cg32", 2, 8, 16, 128, 4, 128, 128, 4),
    Fused("fx_w32_t64_cg64", 2, 4, 32, 128, 2, 64, 64, -1), Fused("fx_w32_t128_wide", 2, 8, 32, 64, 4, 192, 128, 0, "wide"),
    Fused("fx_w8_t64_const", 2, 8, 8, 128, 8, 64, 64, 4, "const", False), Fused("fx_k1024", 1, 8, 16, 1024, 16, 64, 128, 0, "plain"),
    Fused("fx_w8_t128_h16", 2, 16, 8, 64, 2, 128, 128, -1, "wide", False),
]
# integer weights that are zero except one border tap: a padding pixel that was transformed instead of left zero shows in every border
# output element (tap = ky 3 + kx: 1 top, 3 left, 5 right, 7 bottom)
BORDER_TAPS = (1, 3, 5, 7)

# split-K: forced modes 2 and 4 over chunk counts 4, 6, 8 (the while that halves ks), every variant; and the rule itself (mode 1)
Split = _nt("Split", "name N H W K Nc pt mode variant K1", ("plain", 0))
SPLIT_CASES = [
    Split("sk2_k256", 2, 8, 8, 256, 128, 128, 2), Split("sk4_k256_halved", 2, 8, 8, 256, 128, 64, 4), Split("sk2_k384", 2, 8, 8, 384, 64, 128, 2),
    Split("sk4_k384_halved", 2, 8, 8, 384, 64, 128, 4), Split("sk4_k512", 2, 8, 8, 512, 192, 64, 4), Split("sk2_k512_sums", 4, 8, 8, 512, 128, 128, 2, "sums"),
    Split("sk4_k512_x32", 2, 8, 16, 512, 64, 128, 4, "x32"), Split("sk2_k256_two", 2, 8, 16, 256, 64, 64, 2, "plain", 64),
    Split("sk2_k256_fused", 2, 8, 16, 256, 64, 128, 2, "fused"), Split("sk4_k512_fused32", 2, 8, 16, 512, 64, 64, 4, "fused32"),
    Split("rule_on", 2, 8, 8, 1024, 64, 0, 1), Split("rule_off_k960", 2, 8, 8, 960, 64, 0, 1),
]
# the flag-area limit: (ks - 1) tiles 16 bytes > 64 KB needs more tiles than 4 096 pixels give -- 1 536 tiles under a split of 4 (no reference:
# the launch must report split 1 and equal the unsplit launch bit for bit)
FLAG_EDGE = desc(256, 8, 8, 512, 768)
SPLIT_WS_BYTES = 8 << 20      # the workspace the GPU test registers unless a case needs an exact size


def split_kn(c, ws_bytes=SPLIT_WS_BYTES):
    return Knobs(c.pt, c.mode, ws_bytes)


def split_desc(c):
    return desc(c.N, c.H, c.W, c.K, c.Nc, K1=c.K1 or None, ldx=(c.K1 or c.K))


def plain_desc(c, flip=0, in32=False, f32=False):
    K1 = c.K1 or c.K
    return desc(c.N, c.H, c.W, c.K, c.Nc, K1=K1, ldx=K1 + c.ldx, ldx2=(c.K - K1 + c.ldx2) if c.K1 else 0, ldy=c.Nc + c.ldy,
                ldr=(c.Nc + c.ldr) if "r" in c.epi else 0, transposed=flip, accumulate=int("a" in c.epi), mode=0 if f32 else 1)


def case_pixels(c):
    return c.N * c.H * c.W


def unit_sums_exact(y, pt, H, W):
    """The GroupNorm-sums exactness condition for integer-valued stored y [N][H][W][Nc]: per workgroup (pt pixels), image and 16-channel slab,
    sum |y| and sum y^2 stay below 2^24 -- the kernel reduces them in fp32 before the fixed-point add, so every partial sum is exact."""
    N, Nc = y.shape[0], y.shape[-1]
    px = min(pt, H * W)                                       # a tile's share of one image
    v = y.to(F64).reshape(N * H * W // px, px, Nc // 16, 16)
    return bool((v == v.round()).all()) and float(v.abs().sum((1, 3)).max()) < 2 ** 24 and float((v * v).sum((1, 3)).max()) < 2 ** 24


# ------------------------------------------------------------------------------------------------------------ operands of a case
def seed(*key):
    return zlib.crc32(repr(key).encode())


def plain_operands(c, kind, flip=False, stored_f32=False):
    """The operands of a plain / sums / fp32-input / exact-fp32 case, float64: x (and x2), the contraction-first weights G [tap][K][Nc], bias,
    residual, prior content.  stored_f32: x and G keep float32 values (else they are bf16-representable).  flip draws other values."""
    K1 = c.K1 or c.K
    b16 = not stored_f32
    key = (c.name, kind, bool(flip))
    x = operand((c.N, c.H, c.W, K1), kind, seed(key, "x"), bf16=b16)
    x2 = operand((c.N, c.H, c.W, c.K - K1), kind, seed(key, "x2"), bf16=b16) if c.K1 else None
    G = operand((9, c.K, c.Nc), kind, seed(key, "w"), bf16=b16, amp=3, scale=(9 * c.K) ** -0.5)
    bias = operand((c.Nc,), kind, seed(key, "b")) if "b" in c.epi else None
    res = operand((c.N, c.H, c.W, c.Nc), kind, seed(key, "r")) if "r" in c.epi else None
    prior = init_content((c.N, c.H, c.W, c.Nc), seed(key, "p"), kind) if "a" in c.epi else None
    return dict(x=x, x2=x2, G=G, bias=bias, res=res, prior=prior)


def plain_reference(ops, flip=False, round_x=False):
    """-> (float64 reference, the same sum over |terms|).  round_x: x and x2 rounded once to bf16 (the fp32-input form)."""
    r = (lambda t: None if t is None else bf16_round(t)) if round_x else (lambda t: t)
    args = (r(ops["x"]), ops["G"], flip, r(ops["x2"]), ops["bias"], ops["res"], ops["prior"])
    return conv_ref(*args), conv_ref(*args, absolute=True)


def stored(ref, out16):
    """The value a correct kernel stores for an exactly representable reference: fp32, or rounded to nearest even onto bf16."""
    return bf16_round(ref) if out16 else ref.to(F32).to(F64)


GN_EPS = 1e-5


def fused_operands(c, border_tap=None, x_f32=False):
    """Operands of a fused case.  x: the raw bf16 conv output the kernel normalises (N, H, W, K), sums: its fixed-point slab sums, gamma / beta
    by c.params, temb [N][K] or None, the coefficients (sc, sh, tb) of the rounding model, G, bias.  border_tap: integer weights in {-3..3}, one
    in eight non-zero, on that tap alone and no bias (see BORDER_TAPS)."""
    N, H, W, K = c.N, c.H, c.W, c.K
    x = f32r(randn((N, H, W, K), seed(c.name, "x", x_f32)) * 1.3 + 0.2)       # x_f32: fp32-stored activations keep every mantissa bit
    x = x if x_f32 else bf16_round(x)
    if c.params == "const":
        x[1] = 0.75
    if c.params == "wide":
        gamma, beta = randn((K,), seed(c.name, "g")) * 4 + 1, randn((K,), seed(c.name, "be")) * 10
    else:
        gamma, beta = randn((K,), seed(c.name, "g")) * 0.5 + 1, randn((K,), seed(c.name, "be")) * 0.2
    temb = (randn((N, K), seed(c.name, "t")) * 0.3 + 0.5) if c.ldt >= 0 else None
    sums = gn_sums(x)
    sc, sh, tb = coef_from_sums(sums, H * W, K, c.G, GN_EPS, gamma, beta, temb)
    if border_tap is None:
        G = randn((9, K, c.Nc), seed(c.name, "w"), bf16=True, scale=(9 * K) ** -0.5)
    else:
        G = torch.zeros(9, K, c.Nc, dtype=F64)
        G[border_tap] = ints((K, c.Nc), -3, 3, seed(c.name, "wb", border_tap)) * (ints((K, c.Nc), 0, 7, seed(c.name, "thin")) == 0)
    bias = randn((c.Nc,), seed(c.name, "b")) if (c.bias and border_tap is None) else None
    return dict(x=x, sums=sums, gamma=gamma, beta=beta, temb=temb, sc=sc, sh=sh, tb=tb, G=G, bias=bias)


def fused_exact_stats(ops, c):
    """(mean, rstd) [N][G] in float64 from the same sums: what the unrounded float64 reference of the old bound normalises with."""
    N, K = ops["x"].shape[0], c.K
    cg = K // c.G
    tot = ops["sums"].view(N, c.G, cg // 16, 2).sum(2).to(F64) / (GSUM_SCALE * c.H * c.W * cg)
    mean = tot[..., 0]
    return mean, 1.0 / torch.sqrt((tot[..., 1] - mean * mean).clamp_min(0.0) + GN_EPS)


def fused_reference64(ops, c):
    """Unrounded float64: conv(mish(groupnorm(x) gamma + beta) + temb) + bias."""
    mean, rstd = fused_exact_stats(ops, c)
    cg = c.K // c.G
    sc = rstd.repeat_interleave(cg, 1) * ops["gamma"][None]
    sh = ops["beta"][None] - mean.repeat_interleave(cg, 1) * sc
    tb = ops["temb"] if ops["temb"] is not None else torch.zeros_like(sc)
    return conv_ref(fused_h(ops["x"], sc, sh, tb, rounded=False), ops["G"], bias=ops["bias"])


# ------------------------------------------------------------------------------------------------------------ which edges the lists reach
def edges():
    """name -> the case names that reach it."""
    e = {}

    def hit(k, c):
        e.setdefault(k, []).append(c.name)

    def plain(c, var, in32=False, f32=False, outs=(False, True)):
        for o16 in outs:
            d = plain_desc(c, 0, in32, f32)
            f = launch_facts(d, var, o16, "r" in c.epi, in32, f32, Knobs(c.pt, 0, 0))
            assert f is not None, c
            hit("inst:" + repr(f.inst), c)
            hit(f"xmap:{int(f.xmap)}", c)
            hit(f"qmap:{int(f.qmap)}", c)
            if f.qmap:
                hit(f"cpq:{f.cpq}", c)
            hit(f"w{d.OW}:ti{f.TI}", c)
            hit(f"w{d.OW}:t{f.pt}:th{f.TH}", c)
            if f.XP == pw_xp(f.pt):
                hit(f"xp_equal:{f.pt}:ti{f.TI}", c)
            hit(f"tile16:{int(f.tile16)}", c)
            hit(f"idle_waves:{int(f.idle)}", c)
            hit(f"chunks:{f.nch}", c)
            hit(f"gy_odd:{int(f.gy % 2)}", c)
            hit(f"tiles_per_img:{min(f.tiles_per_img, 3)}", c)
            if var == 1:
                hit(f"gns:t{f.pt}:ti{f.TI}", c)
                if d.Nc % 128:
                    hit(f"gns:slab_guard:ti{f.TI}", c)
    for c in PLAIN_CASES:
        plain(c, 0)
    for c in GNS_CASES:
        plain(c, 1)
    for c in X32_CASES:
        plain(c, 0, in32=True)
        plain(c, 1, in32=True)
    for c in F32_CASES:
        plain(c, 0, f32=True, outs=(False,))
    for c in FUSED_CASES:
        for var in (2, 3):
            for in32 in (False, True):
                for o16 in (False, True):
                    d = desc(c.N, c.H, c.W, c.K, c.Nc)
                    f = launch_facts(d, var, o16, False, in32, False, Knobs(c.pt, 0, 0))
                    assert f is not None and f.TI == 1, c
                    hit("inst:" + repr(f.inst), c)
        hit(f"fused:cg{c.K // c.G}", c)
        hit(f"fused:w{c.W}:t{c.pt}", c)
        hit("fused:temb:" + ("none" if c.ldt < 0 else "dense" if c.ldt == 0 else "pitched"), c)
        hit("fused:params:" + c.params, c)
        if c.K == 1024:
            hit("fused:k1024", c)
    for c in SPLIT_CASES:
        var = {"plain": 0, "sums": 1, "x32": 0, "fused": 2, "fused32": 2}[c.variant]
        f = launch_facts(split_desc(c), var, False, False, c.variant in ("x32", "fused32"), False, split_kn(c))
        assert f is not None and f.grid <= 400, c
        hit(f"split:{f.ks}", c)
        hit(f"split:mode{c.mode}:chunks{f.nch}:ks{f.ks}", c)
        hit("split:variant:" + c.variant + (":two" if c.K1 else ""), c)
    return e


REQUIRED_EDGES = tuple(
    ["inst:" + repr(i) for i in sorted(all_instantiations())]
    + ["xmap:0", "xmap:1", "qmap:0", "qmap:1", "cpq:1", "cpq:3", "gy_odd:1", "tile16:0", "tile16:1", "idle_waves:0", "idle_waves:1"]
    + [f"w{w}:ti{ti}" for w in (8, 16) for ti in (1, 2)] + ["w32:ti1", "xp_equal:64:ti2", "xp_equal:128:ti2", "xp_equal:64:ti1", "xp_equal:128:ti1",
                                                           "xp_equal:256:ti1"]
    + ["w32:t64:th2", "w32:t128:th4", "w32:t256:th8", "w16:t64:th2", "w16:t64:th4", "w16:t128:th4", "w16:t128:th8", "w16:t256:th16", "w8:t64:th4",
       "w8:t64:th8", "w8:t128:th8", "w8:t128:th16", "w8:t256:th32"]
    + [f"chunks:{n}" for n in (1, 2, 3, 5, 16)] + ["tiles_per_img:1", "tiles_per_img:2", "tiles_per_img:3"]
    + ["gns:t64:ti1", "gns:t64:ti2", "gns:t128:ti1", "gns:t128:ti2", "gns:t256:ti1", "gns:slab_guard:ti1", "gns:slab_guard:ti2"]
    + ["fused:cg16", "fused:cg32", "fused:cg64", "fused:k1024", "fused:temb:none", "fused:temb:dense", "fused:temb:pitched", "fused:params:plain",
       "fused:params:wide", "fused:params:const", "fused:w16:t64", "fused:w16:t128", "fused:w32:t64", "fused:w32:t128"]
    + ["split:1", "split:2", "split:4", "split:mode2:chunks4:ks2", "split:mode4:chunks4:ks2", "split:mode2:chunks6:ks2", "split:mode4:chunks6:ks2",
       "split:mode4:chunks8:ks4", "split:mode1:chunks16:ks4", "split:mode1:chunks15:ks1", "split:variant:plain", "split:variant:sums",
       "split:variant:x32", "split:variant:plain:two", "split:variant:fused", "split:variant:fused32"])


def random_descs(n, seed=7):
    """Descriptors around the planner's conditions: mostly valid values with a few off ones mixed in."""
    g = torch.Generator().manual_seed(seed)

    def pick(vals):
        return vals[int(torch.randint(0, len(vals), (1,), generator=g))]
    out = []
    for _ in range(n):
        W = pick([8, 8, 16, 16, 32, 32, 4, 64, 24])
        H = pick([1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64])
        N = pick([1, 2, 3, 4, 5, 6, 8, 16, 64, 128, 512])
        K = pick([64, 128, 192, 256, 320, 512, 1024, 1088, 96, 32])
        Nc = pick([64, 128, 192, 256, 384, 768, 96, 32, 1024])
        K1 = pick([K, K, K, 64, 32, max(K - 64, 0), 96])
        over = {}
        r = pick(list(range(24)))
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
        mode = pick([1, 1, 1, 0])
        ldx = K1 + pick([0, 0, 8, 4, 2])
        ldx2 = max(K - K1, 0) + pick([0, 0, 24, 4, 2])
        out.append(desc(N, H, W, K, Nc, K1=K1, ldx=ldx, ldx2=ldx2, mode=mode, **over))
    return out


def term_count(c):
    """Summed terms per output element: 9 K products + bias, residual, prior content."""
    return 9 * c.K + len(c.epi)


assert math.isclose(LOG2E_F32, 1.0 / math.log(2.0), rel_tol=1e-7)
