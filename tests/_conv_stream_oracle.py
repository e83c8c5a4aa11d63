"""CPU oracle of the three streaming kernels of csrc/conv_pw.hip: conv1x1_pw_kernel (mi_conv1x1_pw, _batched, _x32, _f32), conv_gt_kernel
(mi_conv_gt, _dual, _tile, _supported) and ln_conv1x1_pw_kernel (mi_ln_conv1x1_pw, _dual).

Shared by tests/test_conv_stream_cpu.py and tests/test_conv_stream_kernels_gpu.py:
  * float64 references: y = [x | x2] @ G + bias + res + prior for the 1x1 conv (per-sample G for the batched entry); the tap gather taken
    literally from include/mi_ddpm.h for any k, stride, pad and H != W (transposed = 0: iy = oy s - p + ky; transposed = 1:
    iy = (oy + p - ky) / s where divisible; tap ky KW + kx of the contraction-first operand G[tap][K][Nc]) with the number of valid taps per
    produced pixel; each with the same sum over |terms|;
  * the channel LayerNorm of the reference model, (x - mean) / (sqrt(var) + eps) g + b in float64, its bf16 rounding model, and a float32
    emulation in the kernel's order (per-lane octet sums, the 1-2-4 xor tree, two-pass variance);
  * the host planners restated: pw1_ok in its three forms and what pw1_go derives (tile, grid, flattened ids, the channel-tile loop and
    the instantiation), gt_plan (classes with their tap lists, tile, refusals), lnpw1_ok with its PXT / NCH / G2 pick and lnpw1_lds;
  * the case lists, and edges(): which instantiations and dispatch edges those lists reach, by name.
The fragment layouts, descriptors and operand generators are tests/_conv_pw_oracle.py's (they take any tap count).  The rules are read from
the .hip file and the header and written again here; nothing is imported from the package."""
import os
import sys
from collections import namedtuple

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_pw_oracle as P  # noqa: E402
from _conv_pw_oracle import BF, F32, F64, bf16_round, desc, frag_operand, init_content, ints, operand, randn, rel, seed, stored, wdq, wfq  # noqa: E402,F401

U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------ references
def pw1_ref(x, G, x2=None, bias=None, res=None, prior=None, absolute=False):
    """x [S][hw][K1] (x2 [S][hw][K - K1]), G [K][Nc] or per sample [S][K][Nc] -> y [S][hw][Nc]; absolute: the sum over |terms|."""
    a = (lambda t: t.to(F64).abs()) if absolute else (lambda t: t.to(F64))
    src = a(x) if x2 is None else torch.cat([a(x), a(x2)], dim=-1)
    y = src @ a(G)
    for extra in (bias, res, prior):
        if extra is not None:
            y = y + a(extra)
    return y


def gather_ref(x, G, k, s, p, tr, OH, OW, bias=None, res=None, prior=None, absolute=False):
    """The header's definition: y[n][oy][ox][j] = bias + res + prior + sum_{ky,kx,c} x[n][iy][ix][c] G[ky k + kx][c][j] over the taps whose
    (iy, ix) exists.  x [N][IH][IW][K], G [k k][K][Nc].  -> (y [N][OH][OW][Nc], valid taps per produced pixel [OH][OW])."""
    a = (lambda t: t.to(F64).abs()) if absolute else (lambda t: t.to(F64))
    xa, Ga = a(x), a(G)
    N, IH, IW, K = x.shape
    assert G.shape[0] == k * k and G.shape[1] == K
    y = torch.zeros(N, OH, OW, G.shape[2], dtype=F64)
    cnt = torch.zeros(OH, OW, dtype=torch.int64)

    def axis(n_out, n_in, kk):
        o = torch.arange(n_out)
        if tr:
            num = o + p - kk
            ok, i = (num % s == 0), torch.div(num, s, rounding_mode="floor")
        else:
            i = o * s - p + kk
            ok = torch.ones_like(o, dtype=torch.bool)
        ok = ok & (i >= 0) & (i < n_in)
        return o[ok], i[ok]
    for ky in range(k):
        oy, iy = axis(OH, IH, ky)
        for kx in range(k):
            ox, ix = axis(OW, IW, kx)
            if oy.numel() == 0 or ox.numel() == 0:
                continue
            y[:, oy[:, None], ox[None, :]] += xa[:, iy[:, None], ix[None, :]] @ Ga[ky * k + kx]
            cnt[oy[:, None], ox[None, :]] += 1
    for extra in (bias, res, prior):
        if extra is not None:
            y = y + a(extra)
    return y, cnt


def ln64(x, g, b, eps):
    """Channel LayerNorm of the reference model in float64: (x - mean) / (sqrt(var) + eps) g + b, biased variance.  -> (out, xhat g)."""
    x = x.to(F64)
    mean = x.mean(-1, keepdim=True)
    std = ((x - mean) ** 2).mean(-1, keepdim=True).sqrt()
    xg = (x - mean) / (std + eps) * g.to(F64)
    return xg + b.to(F64), xg


def ln_emul32(x, g, b, eps):
    """float32 in ln_conv1x1_pw_kernel's order.  A pixel's K channels live in 8 lanes: lane o holds octet o of every 64-channel half
    (chunk ch, half h: channels 128 ch + 64 h + 8 o .. + 7, as two quads).  s = sum over (ch, h, quad) of (x0 + x1) + (x2 + x3), then
    s += s[o ^ 1], s[o ^ 2], s[o ^ 4]; mean = s / K; the same walk over (x - mean)^2; inv = 1 / (sqrt(s2 / K) + eps);
    out = (x - mean) inv g + b, rounded to bf16 once."""
    M, K = x.shape
    xs = x.to(F32).view(M, K // 64, 8, 2, 4)                               # [pixel][half][octet][quad][4]

    def lanes(v):
        s = torch.zeros(M, 8, dtype=F32)
        for hh in range(K // 64):
            for q in range(2):
                s = s + ((v[:, hh, :, q, 0] + v[:, hh, :, q, 1]) + (v[:, hh, :, q, 2] + v[:, hh, :, q, 3]))
        o = torch.arange(8)
        for st in (1, 2, 4):
            s = s + s[:, o ^ st]
        return s[:, :1]
    invc = torch.tensor(1.0 / K, dtype=F32)
    mean = lanes(xs) * invc
    dv = xs - mean.view(M, 1, 1, 1, 1)
    s2 = lanes(dv * dv)
    inv = 1.0 / (torch.sqrt(s2 * invc) + torch.tensor(eps, dtype=F32))
    out = (x.to(F32) - mean) * inv * g.to(F32) + b.to(F32)
    return bf16_round(out)


def bf16_ulp(v):
    """One unit in the last place of bf16 at magnitude v (float64 tensor; 0 -> the smallest normal's)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - 7)


# ------------------------------------------------------------------------------------------------------------ planners, restated
def desc1(N, H, W, K, Nc, **kw):
    return desc(N, H, W, K, Nc, **dict(dict(KH=1, KW=1, pad=0), **kw))


def pw1_ok(d, form="bf16"):
    """pw1_ok(d, f32, in32): form 'bf16', 'x32' (fp32 x, bf16 MFMA mode) or 'f32' (exact fp32)."""
    if d.KH != 1 or d.KW != 1 or d.pad != 0 or d.stride != 1 or d.mode != (0 if form == "f32" else 1) or d.IH != d.OH or d.IW != d.OW:
        return False
    ck, lda = (64 if form == "f32" else 128), (8 if form == "bf16" else 4)
    if d.K % ck or d.K1 % ck or d.K1 <= 0 or d.K1 > d.K or d.Nc % 64 or d.ldx % lda or (d.K1 != d.K and d.ldx2 % lda):
        return False
    return (d.N * d.OH * d.OW) % 128 == 0


Pw1Facts = namedtuple("Pw1Facts", "small pxt gx gy flat nloop inst chunks idle fast16")


def pw1_plan(d, form="bf16", out16=False, has_res=False, dual=False, wbatch=0, knob=1):
    """What the entry points derive for a descriptor pw1_ok takes (None otherwise).  knob: mi_debug_conv1x1_pw_nloop's state (0 off,
    1 the channel-tile loop from 1 024 pixel tiles up, 2 from any grid).  inst = <OUT16, DUAL, PXT, F32, IN32, NLOOP>."""
    if not pw1_ok(d, form):
        return None
    M, gy = d.N * d.OH * d.OW, (d.Nc + 127) // 128
    hw = d.OH * d.OW
    if form == "x32":
        small = True
    else:
        small = (M // 128) * gy < 256 or bool(form == "bf16" and wbatch and hw % 128 != 0)
    pxt = 64 if small else 128
    gx = M // pxt
    nloop = bool(form == "bf16" and out16 and not has_res and not d.accumulate and not small and not wbatch and d.K == 128 and d.K1 == d.K
                 and gy > 1 and knob and gx >= (0 if knob == 2 else 1024))
    flat = (not nloop) and gy > 1 and gx % 8 == 0
    o16 = bool(out16) and form != "f32"
    inst = (o16, bool(dual) and not o16 and form == "bf16", pxt, form == "f32", form == "x32", nloop)
    return Pw1Facts(small, pxt, gx, gy, flat, nloop, inst, d.K // (64 if form == "f32" else 128), d.Nc % 128 == 64,
                    o16 and not has_res and not d.accumulate)


def pw1_instantiations():
    s = {(o16, du, px, False, False, False) for px in (64, 128) for o16, du in ((True, False), (False, True), (False, False))}
    s |= {(True, False, 128, False, False, True), (True, False, 64, False, True, False), (False, False, 64, False, True, False),
          (False, False, 64, True, False, False), (False, False, 128, True, False, False)}
    return s


GtPlan = namedtuple("GtPlan", "classes ncls pxt gx gy M GH GW si so flat")


def ilog2_exact(v):
    return v.bit_length() - 1 if v > 0 and v & (v - 1) == 0 else -1


def gt_plan(d):
    """gt_plan: None when refused; classes = [(ao, bo, [(dy, dx, weight tap), ...]), ...] in blockIdx.z order."""
    if d.mode not in (0, 1) or d.K1 != d.K or d.K % 64 or d.Nc % 64 or d.ldx % (8 if d.mode == 1 else 4):
        return None
    k, s, p = d.KH, d.stride, d.pad
    if d.KW != k or k * k > 16 or k < 1 or s not in (1, 2) or p < 0 or p > 7:
        return None
    if d.Nc * d.K * (2 if d.mode == 1 else 4) * k * k >= 1 << 31:
        return None
    classes = []
    if not d.transposed:
        if d.OH != (d.IH + 2 * p - k) // s + 1 or d.OW != (d.IW + 2 * p - k) // s + 1:
            return None
        GH, GW, si, so = d.OH, d.OW, s, 1
        classes.append((0, 0, [(ky - p, kx - p, ky * k + kx) for ky in range(k) for kx in range(k)]))
    else:
        if d.OH != s * d.IH or d.OW != s * d.IW:
            return None
        GH, GW, si, so = d.OH // s, d.OW // s, 1, s
        for cy in range(s):
            for cx in range(s):
                taps = []
                for ky in range((cy + p) % s, k, s):
                    for kx in range((cx + p) % s, k, s):
                        dy, dx = (cy + p - ky) // s, (cx + p - kx) // s
                        if not (-8 <= dy <= 7 and -8 <= dx <= 7):
                            return None
                        taps.append((dy, dx, ky * k + kx))
                if not taps:
                    return None
                classes.append((cy, cx, taps))
    if ilog2_exact(GW) < 0 or ilog2_exact(GH * GW) < 0:
        return None
    M = d.N * GH * GW
    if M % 64:
        return None
    gy = (d.Nc + 127) // 128
    small = M % 128 != 0 or (M // 128) * gy * len(classes) < 256
    pxt = 64 if small else 128
    gx = M // pxt
    return GtPlan(classes, len(classes), pxt, gx, gy, M, GH, GW, si, so, gy > 1 and gx % 8 == 0)


def lnpw1_ok(d):
    if d.KH != 1 or d.KW != 1 or d.pad != 0 or d.stride != 1 or d.mode != 1 or d.IH != d.OH or d.IW != d.OW:
        return False
    if d.K not in (128, 256, 512) or d.K1 != d.K or d.Nc % 64 or d.ldx % 4 or d.ldy % 8 or d.accumulate:
        return False
    return (d.N * d.OH * d.OW) % 128 == 0


def lnpw1_pick(d):
    """-> (PXT, NCH, G2, gx, gy) of a descriptor lnpw1_ok takes (None otherwise)."""
    if not lnpw1_ok(d):
        return None
    M, nch, gy = d.N * d.OH * d.OW, d.K // 128, (d.Nc + 127) // 128
    if d.K == 128 and M // 128 >= 512:
        return 128, 1, False, M // 128, gy
    return 64, nch, M // 64 < 512, M // 64, gy


def lnpw1_lds(pxt, nch):
    return nch * pxt * 256 + pxt * 256 + nch * 1024


def ln_instantiations():
    return {(128, 1, False)} | {(64, n, g2) for n in (1, 2, 4) for g2 in (False, True)}


# ------------------------------------------------------------------------------------------------------------ cases
_nt = P._nt
# 1x1.  M pixels (hw = 0: one sample; hw > 0: the batched entry, samples of hw pixels with their own weights, wb elements added to one
# layer's fragments); K1: channels of the first source (0: one source); ldx / ldx2 / ldy / ldr / ldy16: elements ADDED to the dense pitch
# (ldy16 < 0: no bf16 copy is launched); xoff: columns in front of x inside its row (ldx = 3 K, x in the second third); epi as in the 3x3
# oracle; form 'bf16', 'x32', 'f32'; knob: mi_debug_conv1x1_pw_nloop's state for the case
P1 = _nt("P1", "name M K Nc K1 ldx ldx2 ldy ldr ldy16 epi form hw wb xoff knob", (0, 0, 0, 0, 0, -1, "b", "bf16", 0, 0, 0, 1))


def _p1(name, M, K, Nc, **kw):
    return P1(name, M, K, Nc, **kw)


PW1_SHAPE_CASES = [
    _p1("m128_nc64", 128, 128, 64), _p1("m256_nc64", 256, 128, 64, epi=""), _p1("nc128", 256, 128, 128), _p1("nc192", 256, 128, 192, epi="br"),
    _p1("nc320", 128, 128, 320, epi=""), _p1("nc768", 256, 128, 768), _p1("k256", 256, 256, 64), _p1("k384", 128, 384, 192, epi="r"),
    _p1("k1024", 256, 1024, 128, epi="ba"),
    _p1("two_k1_128", 256, 384, 64, K1=128, ldx=8, ldx2=24), _p1("two_k1_256", 128, 384, 192, K1=256, ldx=16, ldx2=8, epi="bra"),
]
PW1_PITCH_CASES = [
    _p1("ldx8", 256, 128, 64, ldx=8), _p1("ldx3k_second_third", 256, 128, 192, ldx=256, xoff=128, epi="br", ldr=4),
    _p1("ldy8", 256, 128, 192, ldy=8), _p1("ldy64_ldr4", 128, 256, 64, ldy=64, ldr=4, epi="br"), _p1("ldy16_8", 256, 128, 192, ldy=8, ldy16=8, epi="b"),
]
PW1_EPILOGUE_CASES = [_p1(f"epi_{e or 'none'}", 256, 128, 192, ldy=8, ldr=4, ldy16=(-1 if "a" in e else 24), epi=e)
                      for e in ("", "b", "r", "br", "a", "ba", "ra", "bra")]
PW1_GRID_CASES = [
    _p1("t64_gx8_flat", 512, 128, 192, epi="br"), _p1("t64_gx6", 384, 128, 192, epi="br"), _p1("t64_gx10", 640, 128, 192),
    _p1("t64_gx16_gy3_flat", 1024, 128, 320, ldy16=8),
    _p1("t128_gx43", 5504, 128, 768), _p1("t128_gx44", 5632, 128, 768, epi="br", ldy16=8), _p1("t128_gx48_flat", 6144, 128, 768, epi="br", ldy16=8),
    _p1("t128_nc128", 32768, 128, 128, epi=""),
]
# the channel-tile loop (knob 2).  Nc = 320 at M = 5 632 / 6 144 has (M / 128) gy = 132 / 144 < 256: 64-pixel tiles, so the loop stays
# off there (one of its conditions); Nc = 320 reaches it from M = 11 008 on (gx = 86; 11 264: gx = 88)
PW1_NLOOP_CASES = [
    _p1("nloop_nc768_gx44", 5632, 128, 768, knob=2), _p1("nloop_nc768_gx48", 6144, 128, 768, knob=2, epi=""),
    _p1("nloop_nc320_gx86", 11008, 128, 320, knob=2, ldy=8), _p1("nloop_nc320_gx88", 11264, 128, 320, knob=2, epi=""),
]
PW1_NLOOP_OFF_CASES = [      # each switches the loop off although the knob asks for it (fp32 output: every case's second launch)
    _p1("nloop_off_small_5632", 5632, 128, 320, knob=2), _p1("nloop_off_small_6144", 6144, 128, 320, knob=2),
    _p1("nloop_off_res", 5632, 128, 768, knob=2, epi="br"), _p1("nloop_off_acc", 5632, 128, 768, knob=2, epi="a"),
    _p1("nloop_off_k256", 5632, 256, 768, knob=2), _p1("nloop_off_wbatch", 5632, 128, 768, knob=2, hw=256, wb=64),
    _p1("nloop_off_gy1", 32768, 128, 128, knob=2, epi=""),
]
PW1_BATCHED_CASES = [
    _p1("wb_hw64", 128, 128, 64, hw=64, wb=64), _p1("wb_hw192_t64", 384, 128, 192, hw=192, wb=8, epi="br", ldr=4),
    _p1("wb_hw256", 512, 256, 128, hw=256, wb=128, ldy16=8), _p1("wb_ldx3k", 256, 128, 128, hw=64, wb=64, ldx=256, xoff=128, epi="ba"),
    _p1("wb_t128", 5632, 128, 768, hw=256, wb=64),
]
PW1_X32_CASES = [
    _p1("x32_ldx4", 256, 128, 192, ldx=4, form="x32"), _p1("x32_two", 128, 384, 64, K1=128, ldx=4, ldx2=12, form="x32", epi="br", ldr=4),
    _p1("x32_acc", 256, 256, 128, ldx=4, form="x32", epi="ba", ldy=8), _p1("x32_flat", 512, 128, 192, form="x32", epi=""),
]
PW1_F32_CASES = [
    _p1("f32_k64", 128, 64, 64, form="f32"), _p1("f32_k192", 256, 192, 192, form="f32", ldx=4, epi="br", ldr=4),
    _p1("f32_k512", 128, 512, 128, form="f32", epi="ba"), _p1("f32_two_k1_64", 256, 192, 64, K1=64, ldx=4, ldx2=4, form="f32"),
    _p1("f32_t128", 5632, 64, 768, form="f32", epi="br"), _p1("f32_t128_flat", 6144, 64, 768, form="f32", ldy=8),
]
PW1_CASES = (PW1_SHAPE_CASES + PW1_PITCH_CASES + PW1_EPILOGUE_CASES + PW1_GRID_CASES + PW1_NLOOP_CASES + PW1_NLOOP_OFF_CASES
             + PW1_BATCHED_CASES + PW1_X32_CASES + PW1_F32_CASES)


def pw1_desc(c):
    K1 = c.K1 or c.K
    if c.hw:
        N, H, W = c.M // c.hw, c.hw // 8, 8
    else:
        N, H, W = 1, c.M // 16, 16
    return desc1(N, H, W, c.K, c.Nc, K1=K1, ldx=K1 + c.ldx, ldx2=(c.K - K1 + c.ldx2) if c.K1 else 0, ldy=c.Nc + c.ldy,
                 ldr=(c.Nc + c.ldr) if "r" in c.epi else 0, accumulate=int("a" in c.epi), mode=0 if c.form == "f32" else 1)


def pw1_wbatch(c):
    return c.K * c.Nc + c.wb if c.hw else 0


def assert_exact(T):
    """Integer operands: every term is at most 4 x 3 = 12 in magnitude, so T of them stay below 2^24 and every fp32 partial sum is exact."""
    assert T * 12 < 2 ** 24, T


def pw1_operands(c, kind):
    """float64 operands of a 1x1 case: x [S][hw][K1] (and x2), G [K][Nc] or [S][K][Nc], bias, res, prior.  bf16-representable where the
    kernel reads bf16 (x for the bf16 form, G unless exact fp32)."""
    K1 = c.K1 or c.K
    S, hw = (c.M // c.hw, c.hw) if c.hw else (1, c.M)
    key = (c.name, kind)
    x = operand((S, hw, K1), kind, seed(key, "x"), bf16=c.form == "bf16")
    x2 = operand((S, hw, c.K - K1), kind, seed(key, "x2"), bf16=c.form == "bf16") if c.K1 else None
    G = operand(((S,) if c.hw else ()) + (c.K, c.Nc), kind, seed(key, "w"), bf16=c.form != "f32", amp=3, scale=c.K ** -0.5)
    bias = operand((c.Nc,), kind, seed(key, "b")) if "b" in c.epi else None
    res = operand((S, hw, c.Nc), kind, seed(key, "r")) if "r" in c.epi else None
    prior = init_content((S, hw, c.Nc), seed(key, "p"), kind) if "a" in c.epi else None
    if kind == "int":
        assert_exact(c.K + 3)
    return dict(x=x, x2=x2, G=G, bias=bias, res=res, prior=prior)


def pw1_reference(ops, round_x=False):
    r = (lambda t: None if t is None else bf16_round(t)) if round_x else (lambda t: t)
    args = (r(ops["x"]), ops["G"], r(ops["x2"]), ops["bias"], ops["res"], ops["prior"])
    return pw1_ref(*args), pw1_ref(*args, absolute=True)


# Gather.  (N, GH, GW): the gathered class grid; k, s, p, tr: the layer; pitches added to the dense ones (ldx in elements of x's storage);
# ldy16 < 0: no mi_conv_gt_dual launch
GT = _nt("GT", "name N GH GW K Nc k s p tr ldx ldy ldr ldy16 epi", (0, 0, 0, -1, "b"))
_KINDS = {"down": (3, 2, 1, 0), "down_dgrad": (3, 2, 1, 1), "up": (4, 2, 1, 1), "up_dgrad": (4, 2, 1, 0)}
_GRIDS = [(1, 8, 8), (2, 4, 16), (4, 2, 8), (3, 8, 8), (1, 16, 4)]
GT_SHIPPED_CASES = [GT(f"{kn}_n{N}_{GH}x{GW}", N, GH, GW, 64 if i % 2 else 128, 64, *ksp, epi="b" if i % 2 else "br", ldr=4 * (i % 2 == 0))
                    for kn, ksp in _KINDS.items() for i, (N, GH, GW) in enumerate(_GRIDS)]
GT_GENERIC_CASES = [
    GT("k1_s1", 1, 8, 8, 128, 64, 1, 1, 0, 0), GT("k1_s1_tr", 2, 4, 16, 64, 64, 1, 1, 0, 1), GT("k1_s2", 1, 8, 16, 64, 128, 1, 2, 0, 0),
    GT("k2_s2", 2, 8, 4, 128, 64, 2, 2, 0, 0), GT("k2_s2_tr", 2, 4, 8, 64, 64, 2, 2, 0, 1, epi="br"),
    GT("k3_s1", 1, 8, 8, 64, 64, 3, 1, 1, 0), GT("k3_s1_tr", 1, 4, 16, 64, 64, 3, 1, 1, 1), GT("k2_s1", 1, 8, 8, 64, 64, 2, 1, 0, 0),
    GT("k4_s2_p2", 1, 8, 8, 64, 64, 4, 2, 2, 0), GT("k4_s1_p2_tr", 1, 8, 8, 64, 64, 4, 1, 2, 1), GT("k3_s2_p3", 2, 8, 4, 64, 64, 3, 2, 3, 0),
]
GT_CHANNEL_CASES = [
    GT("ch_k64_up", 1, 8, 8, 64, 64, 4, 2, 1, 1), GT("ch_k128_down", 1, 8, 8, 128, 192, 3, 2, 1, 0), GT("ch_k192_dgrad", 2, 8, 8, 192, 256, 3, 2, 1, 1),
    GT("ch_k512_up", 1, 8, 8, 512, 64, 4, 2, 1, 1), GT("ch_k192_k1", 1, 8, 8, 192, 192, 1, 1, 0, 0), GT("ch_k512_down", 1, 8, 8, 512, 64, 3, 2, 1, 0),
    GT("m64_one_tile", 1, 8, 8, 64, 256, 3, 2, 1, 0), GT("m192_t64", 3, 8, 8, 64, 192, 4, 2, 1, 1), GT("flat_gx8_gy2", 8, 8, 8, 64, 256, 3, 2, 1, 0),
    GT("t128_up_nc256", 16, 16, 16, 64, 256, 4, 2, 1, 1, epi="br", ldy16=8),
]
GT_PITCH_CASES = [
    GT("pitch_down", 2, 8, 8, 128, 64, 3, 2, 1, 0, ldx=8, ldy=8, ldr=4, ldy16=24, epi="br"),
    GT("pitch_dgrad", 2, 8, 8, 64, 192, 3, 2, 1, 1, ldx=8, ldy=8, ldr=4, ldy16=24, epi="br"),
    GT("pitch_up", 1, 4, 16, 128, 64, 4, 2, 1, 1, ldx=8, ldy=8, ldr=4, ldy16=24, epi="r"),
]
GT_EPILOGUE_CASES = [GT(f"epi_{nm}_{e or 'none'}", 2, 8, 8, 64, 192, *ksp, ldy=8, ldr=4, epi=e)
                     for nm, ksp in (("down", (3, 2, 1, 0)), ("up", (4, 2, 1, 1))) for e in ("", "b", "r", "br", "a", "ba", "ra", "bra")]
GT_CASES = GT_SHIPPED_CASES + GT_GENERIC_CASES + GT_CHANNEL_CASES + GT_PITCH_CASES + GT_EPILOGUE_CASES


def gt_geometry(c):
    """-> (IH, IW, OH, OW): the produced tensor is s x the gathered one (transposed), or the gathered grid is the produced one and the input
    the shipped s x GH where the size rule takes it, else the smallest input that gives GH rows."""
    if c.tr:
        return c.GH, c.GW, c.s * c.GH, c.s * c.GW

    def inp(g):
        i = c.s * g
        return i if (i + 2 * c.p - c.k) // c.s + 1 == g else (g - 1) * c.s + c.k - 2 * c.p
    return inp(c.GH), inp(c.GW), c.GH, c.GW


def gt_desc(c, mode=1):
    IH, IW, OH, OW = gt_geometry(c)
    xadd = c.ldx if mode == 1 else c.ldx // 2
    return desc(c.N, 0, 0, c.K, c.Nc, IH=IH, IW=IW, OH=OH, OW=OW, KH=c.k, KW=c.k, stride=c.s, pad=c.p, transposed=c.tr, ldx=c.K + xadd,
                ldy=c.Nc + c.ldy, ldr=(c.Nc + c.ldr) if "r" in c.epi else 0, accumulate=int("a" in c.epi), mode=mode)


def gt_operands(c, kind, mode=1, one_tap=None):
    IH, IW, OH, OW = gt_geometry(c)
    key = (c.name, kind, mode)
    b16 = mode == 1
    x = operand((c.N, IH, IW, c.K), kind, seed(key, "x"), bf16=b16)
    G = operand((c.k * c.k, c.K, c.Nc), kind, seed(key, "w"), bf16=b16, amp=3, scale=(c.k * c.k * c.K) ** -0.5)
    if one_tap is not None:
        keep = torch.zeros(c.k * c.k, 1, 1, dtype=F64)
        keep[one_tap] = 1
        G = G * keep
    bias = operand((c.Nc,), kind, seed(key, "b")) if "b" in c.epi and one_tap is None else None
    res = operand((c.N, OH, OW, c.Nc), kind, seed(key, "r")) if "r" in c.epi and one_tap is None else None
    prior = init_content((c.N, OH, OW, c.Nc), seed(key, "p"), kind) if "a" in c.epi else None
    if kind == "int":
        assert_exact(c.k * c.k * c.K + 3)
    return dict(x=x, G=G, bias=bias, res=res, prior=prior)


def gt_reference(c, ops):
    """-> (reference, sum over |terms|, summed terms per element [OH][OW])."""
    IH, IW, OH, OW = gt_geometry(c)
    args = (ops["x"], ops["G"], c.k, c.s, c.p, c.tr, OH, OW, ops["bias"], ops["res"], ops["prior"])
    y, cnt = gather_ref(*args)
    ab, _ = gather_ref(*args, absolute=True)
    return y, ab, cnt * c.K + sum(ops[n] is not None for n in ("bias", "res", "prior"))


# LayerNorm + 1x1.  pitches added to the dense ones
LN = _nt("LN", "name M K Nc ldx ldy ldl bias", (0, 0, 0, False))
LN_CASES = [
    LN("k128_m128", 128, 128, 64), LN("k256_m128", 128, 256, 192, bias=True), LN("k512_m128", 128, 512, 384),
    LN("k128_m1024", 1024, 128, 192, bias=True), LN("k256_m1024", 1024, 256, 384), LN("k512_m1024", 1024, 512, 64, bias=True),
    LN("k128_gx6", 384, 128, 384), LN("pitched_k256", 256, 256, 192, 4, 8, 8, True), LN("pitched_k128", 640, 128, 64, 4, 8, 8),
    LN("pitched_k512", 128, 512, 192, 4, 8, 8, True),
]
LN_LOOP_CASES = [LN("loop64_k128", 32768, 128, 192, bias=True), LN("loop64_k256", 32768, 256, 64), LN("loop64_k512", 32768, 512, 64),
                 LN("loop128_k128", 65536, 128, 64)]
LN_PARAMS = {"plain": (0.3, 1.0, 0.2), "wide": (4.0, 1.0, 10.0)}       # gamma = a randn + b, beta = c randn
LN_DIFFER_CAP = 1e-3           # share of ln_out elements that may differ from bf16(float64 LN)
LN_EMUL_FIGURE = 5e-5          # the float32 emulation's worst share on the randn inputs (re-measured in tests/test_conv_stream_cpu.py)


def ln_desc(c):
    return desc1(1, c.M // 16, 16, c.K, c.Nc, ldx=c.K + c.ldx, ldy=c.Nc + c.ldy)


def ln_operands(c, family, params="plain"):
    """family 'exact': pixel p holds 2^e pattern_p (e in -3..3, pattern a balanced +-1 vector), g in {-3..3}, b in {-4..4}, integer weights,
    eps = 0; 'randn': x = 1.7 randn - 0.4; 'offset': x = 100 + 0.1 randn; 'const': every pixel one dyadic constant, eps = 1e-5."""
    M, K, Nc = c.M, c.K, c.Nc
    key = (c.name, family, params)
    if family == "exact":
        gen = torch.Generator().manual_seed(seed(key, "perm"))
        order = torch.rand(M, K, generator=gen).argsort(1)
        pattern = torch.where(order < K // 2, 1.0, -1.0).to(F64)
        scale = torch.pow(torch.tensor(2.0, dtype=F64), ints((M, 1), -3, 3, seed(key, "e")))
        x, g, b = scale * pattern, ints((K,), -3, 3, seed(key, "g")), ints((K,), -4, 4, seed(key, "b"))
        G, bias, eps = ints((K, Nc), -3, 3, seed(key, "w")), (ints((Nc,), -4, 4, seed(key, "bias")) if c.bias else None), 0.0
        assert_exact(K * 7 // 4 + 2)                       # |ln| <= 3 + 4 = 7, |w| <= 3: 21 per term
        return dict(x=x, g=g, b=b, G=G, bias=bias, eps=eps, ln=pattern * g + b)
    ga, gb, bc = LN_PARAMS[params]
    g, b = randn((K,), seed(key, "g")) * ga + gb, randn((K,), seed(key, "b")) * bc
    if family == "randn":
        x = randn((M, K), seed(key, "x")) * 1.7 - 0.4
    elif family == "offset":
        x = randn((M, K), seed(key, "x")) * 0.1 + 100.0
    else:
        x = (ints((M, 1), -6, 6, seed(key, "c")) * 0.25).expand(M, K).contiguous()
    x = x.to(F32).to(F64)
    G = randn((K, Nc), seed(key, "w"), bf16=True, scale=K ** -0.5)
    bias = randn((Nc,), seed(key, "bias")) if c.bias else None
    return dict(x=x, g=g.to(F32).to(F64), b=b.to(F32).to(F64), G=G, bias=bias, eps=1e-5)


def ln_model_check(got, x, g, b, eps):
    """ln_out (float64 values of the bf16 result) against bf16(float64 LN): -> (share of differing elements, worst differing element over what it
    may be off).  A differing element may be off one bf16 ulp of the larger magnitude, or, where x-hat gamma and beta cancel, 2^-19 of
    |x-hat gamma| + |beta| (the fp32 error of the terms, which then exceeds the result's ulp)."""
    out, xg = ln64(x, g, b, eps)
    model = bf16_round(out)
    diff = (got - model).abs()
    allow = torch.maximum(bf16_ulp(torch.maximum(got.abs(), model.abs())), 2.0 ** -19 * (xg.abs() + b.to(F64).abs()))
    bad = diff > 0
    share = float(bad.sum()) / got.numel()
    worst = float((diff / allow)[bad].max()) if bool(bad.any()) else 0.0
    return share, worst


def ln_offset_bound(got, x, g, b, eps):
    """x = 100 + 0.1 randn: |got - bf16(float64 LN)| over one bf16 ulp plus the oracle's own change when the mean moves by 8 2^-24 |mean|
    (the float32 sum of K values near 100): d out = d mean / (std + eps) |g|."""
    x = x.to(F64)
    out, _ = ln64(x, g, b, eps)
    model = bf16_round(out)
    mean = x.mean(-1, keepdim=True)
    std = ((x - mean) ** 2).mean(-1, keepdim=True).sqrt()
    move = 8 * U * mean.abs() / (std + eps) * g.to(F64).abs()
    allow = bf16_ulp(torch.maximum(got.abs(), model.abs())) + move
    return float(((got - model).abs() / allow).max())


# ------------------------------------------------------------------------------------------------------------ which edges the lists reach
def edges():
    """name -> the case names that reach it."""
    e = {}

    def hit(k, c):
        e.setdefault(k, []).append(c.name)
    for c in PW1_CASES:
        d = pw1_desc(c)
        for o16 in ((False,) if c.form == "f32" else (False, True)):
            for dual in ((False, True) if (c.ldy16 >= 0 and not o16) else (False,)):
                f = pw1_plan(d, c.form, o16, "r" in c.epi, dual, pw1_wbatch(c), c.knob)
                assert f is not None, c
                hit("pw1:inst:" + repr(f.inst), c)
                hit(f"pw1:t{f.pxt}:flat{int(f.flat)}", c)
                if f.pxt == 64 and f.gy > 1 and f.gx % 8:
                    hit(f"pw1:t64:gx{f.gx}", c)
                hit(f"pw1:chunks:{f.chunks}:{c.form}", c)
                hit(f"pw1:idle:{int(f.idle)}", c)
                hit(f"pw1:idle:{int(f.idle)}:fast16:{int(f.fast16)}", c)
                if f.nloop:
                    hit(f"pw1:nloop:gy{f.gy}:flatgrid{int(f.gx % 8 == 0)}:idle{int(f.idle)}", c)
                if c.knob == 2 and o16 and not f.nloop:
                    why = ("small" if f.small and not c.hw else "res" if "r" in c.epi else "acc" if "a" in c.epi else "k256" if c.K != 128
                           else "wbatch" if c.hw else "gy1" if f.gy == 1 else "?")
                    hit("pw1:nloop_off:" + why, c)
                if c.knob == 2 and not o16:
                    hit("pw1:nloop_off:fp32", c)
                hit(f"pw1:epi:{c.epi or 'none'}:{'bf16' if o16 else 'f32'}", c)
                if dual:
                    hit(f"pw1:dual:{c.epi or 'none'}:t{f.pxt}", c)
        if c.K1:
            hit(f"pw1:two:{c.K1}of{c.K}:{c.form}", c)
        if c.hw:
            hit(f"pw1:batched:hw{c.hw}:t{f.pxt}", c)
        if c.xoff:
            hit("pw1:ldx3k" + (":batched" if c.hw else ""), c)
        for n in ("ldx", "ldx2", "ldy", "ldr"):
            if getattr(c, n):
                hit(f"pw1:pitch:{n}+{getattr(c, n)}:{c.form}", c)
        if c.ldy16 > 0:
            hit(f"pw1:pitch:ldy16+{c.ldy16}", c)
    for c in GT_CASES:
        for mode in (1, 0):
            d = gt_desc(c, mode)
            pl = gt_plan(d)
            assert pl is not None, (c, mode)
            for o16 in ((False, True) if mode else (False,)):
                hit("gt:inst:" + repr((o16, pl.pxt, mode == 0)), c)
            hit(f"gt:k{c.k}s{c.s}p{c.p}tr{c.tr}", c)
            hit("gt:taps:" + "-".join(str(len(t)) for _, _, t in pl.classes), c)
            hch = 64 if mode else 32
            for _, _, taps in pl.classes:
                nhc = len(taps) * c.K // hch
                hit(f"gt:pad_half:{nhc % 2}:mode{mode}", c)
                hit(f"gt:chunks:{min((nhc + 1) // 2, 3)}", c)
            hit(f"gt:flat:{int(pl.flat)}", c)
            hit(f"gt:idle:{int(c.Nc % 128 == 64)}", c)
            if pl.GH != pl.GW:
                hit("gt:nonsquare:" + ("wide" if pl.GW > pl.GH else "tall"), c)
            if pl.M % 128 == 64:
                hit("gt:m%128=64", c)
            if pl.gx == 1:
                hit("gt:one_tile", c)
            hit(f"gt:epi:{c.epi or 'none'}:tr{c.tr}", c)
            if c.ldy16 >= 0 and mode == 1 and "a" not in c.epi:
                hit(f"gt:dual:tr{c.tr}:t{pl.pxt}", c)
            for n in ("ldx", "ldy", "ldr"):
                if getattr(c, n):
                    hit(f"gt:pitch:{n}:tr{c.tr}", c)
    for c in LN_CASES + LN_LOOP_CASES:
        pxt, nch, g2, gx, gy = lnpw1_pick(ln_desc(c))
        hit("ln:inst:" + repr((pxt, nch, g2)), c)
        if g2:
            hit(f"ln:g2:gx%8:{'zero' if gx % 8 == 0 else 'nonzero'}", c)
        hit(f"ln:idle:{int(c.Nc % 128 == 64)}", c)
        hit(f"ln:gy:{min(gy, 3)}", c)
        hit(f"ln:bias:{int(c.bias)}", c)
        for n in ("ldx", "ldy", "ldl"):
            if getattr(c, n):
                hit(f"ln:pitch:{n}:k{c.K}", c)
    return e


REQUIRED_EDGES = tuple(
    ["pw1:inst:" + repr(i) for i in sorted(pw1_instantiations())]
    + ["pw1:t64:flat0", "pw1:t64:flat1", "pw1:t128:flat0", "pw1:t128:flat1", "pw1:t64:gx6", "pw1:t64:gx10"]
    + [f"pw1:chunks:{n}:bf16" for n in (1, 2, 3, 8)] + [f"pw1:chunks:{n}:f32" for n in (1, 3, 8)] + ["pw1:chunks:1:x32", "pw1:chunks:2:x32", "pw1:chunks:3:x32"]
    + ["pw1:idle:1:fast16:1", "pw1:idle:1:fast16:0", "pw1:idle:0:fast16:1", "pw1:idle:0:fast16:0"]
    + ["pw1:nloop:gy6:flatgrid0:idle0", "pw1:nloop:gy6:flatgrid1:idle0", "pw1:nloop:gy3:flatgrid0:idle1", "pw1:nloop:gy3:flatgrid1:idle1"]
    + ["pw1:nloop_off:" + w for w in ("small", "res", "acc", "k256", "wbatch", "gy1", "fp32")]
    + [f"pw1:epi:{e or 'none'}:{o}" for e in ("", "b", "r", "br", "a", "ba", "ra", "bra") for o in ("f32", "bf16")]
    + ["pw1:dual:br:t64", "pw1:dual:br:t128", "pw1:dual:none:t64", "pw1:dual:r:t64"]
    + ["pw1:two:128of384:bf16", "pw1:two:256of384:bf16", "pw1:two:128of384:x32", "pw1:two:64of192:f32"]
    + ["pw1:batched:hw64:t64", "pw1:batched:hw192:t64", "pw1:batched:hw256:t64", "pw1:batched:hw256:t128", "pw1:ldx3k", "pw1:ldx3k:batched"]
    + ["pw1:pitch:ldx+8:bf16", "pw1:pitch:ldy+8:bf16", "pw1:pitch:ldy+64:bf16", "pw1:pitch:ldr+4:bf16", "pw1:pitch:ldy16+8", "pw1:pitch:ldx+4:x32",
       "pw1:pitch:ldx2+12:x32", "pw1:pitch:ldx+4:f32", "pw1:pitch:ldx2+24:bf16"]
    + ["gt:inst:" + repr((o16, pxt, f32)) for o16, pxt, f32 in ((False, 64, False), (True, 64, False), (False, 128, False), (True, 128, False),
                                                                 (False, 64, True), (False, 128, True))]
    + ["gt:k3s2p1tr0", "gt:k3s2p1tr1", "gt:k4s2p1tr1", "gt:k4s2p1tr0", "gt:k1s1p0tr0", "gt:k1s1p0tr1", "gt:k1s2p0tr0", "gt:k2s2p0tr0", "gt:k2s2p0tr1",
       "gt:k3s1p1tr0", "gt:k3s1p1tr1", "gt:k4s2p2tr0", "gt:k2s1p0tr0", "gt:k4s1p2tr1", "gt:k3s2p3tr0"]
    + ["gt:taps:1-2-2-4", "gt:taps:4-4-4-4", "gt:taps:9", "gt:taps:16", "gt:taps:1", "gt:taps:1-1-1-1"]
    + ["gt:pad_half:0:mode1", "gt:pad_half:1:mode1", "gt:pad_half:0:mode0", "gt:chunks:1", "gt:chunks:2", "gt:chunks:3"]
    + ["gt:flat:0", "gt:flat:1", "gt:idle:0", "gt:idle:1", "gt:nonsquare:wide", "gt:nonsquare:tall", "gt:m%128=64", "gt:one_tile"]
    + [f"gt:epi:{e or 'none'}:tr{t}" for e in ("", "b", "r", "br", "a", "ba", "ra", "bra") for t in (0, 1)]
    + ["gt:dual:tr0:t64", "gt:dual:tr1:t64", "gt:dual:tr1:t128"] + [f"gt:pitch:{n}:tr{t}" for n in ("ldx", "ldy", "ldr") for t in (0, 1)]
    + ["ln:inst:" + repr(i) for i in sorted(ln_instantiations())]
    + ["ln:g2:gx%8:zero", "ln:g2:gx%8:nonzero", "ln:idle:0", "ln:idle:1", "ln:gy:1", "ln:gy:2", "ln:gy:3", "ln:bias:0", "ln:bias:1"]
    + [f"ln:pitch:{n}:k{k}" for n in ("ldx", "ldy", "ldl") for k in (128, 256, 512)])


# ------------------------------------------------------------------------------------------------------------ random descriptors
def _picker(sd):
    g = torch.Generator().manual_seed(sd)
    return lambda vals: vals[int(torch.randint(0, len(vals), (1,), generator=g))]


def random_pw1_descs(n, sd=11):
    pick = _picker(sd)
    out = []
    for _ in range(n):
        N, H, W = pick([1, 2, 3, 4, 22, 44, 64]), pick([1, 2, 4, 8, 12, 16, 32]), pick([4, 8, 16, 32, 24])
        K = pick([64, 128, 192, 256, 384, 512, 1024, 96, 32])
        Nc = pick([64, 128, 192, 320, 768, 96, 32])
        K1 = pick([K, K, K, 64, 128, max(K - 128, 0), K + 128, 0])
        over = {}
        r = pick(list(range(20)))
        if r == 0:
            over["KH"] = 3
        elif r == 1:
            over["pad"] = 1
        elif r == 2:
            over["stride"] = 2
        elif r == 3:
            over["IH"] = H * 2
        elif r == 4:
            over["KW"] = 3
        elif r == 5:
            over["IW"] = W + 1
        elif r == 6:
            over["accumulate"] = 1
        out.append(desc1(N, H, W, K, Nc, K1=K1, ldx=max(K1, 0) + pick([0, 0, 8, 4, 2]), ldx2=max(K - K1, 0) + pick([0, 0, 8, 4, 2]),
                         ldy=Nc + pick([0, 0, 8, 4]), mode=pick([1, 1, 1, 0]), **over))
    return out


def random_gt_descs(n, sd=13):
    pick = _picker(sd)
    out = []
    for _ in range(n):
        k, s, p, tr = pick([1, 2, 3, 3, 4, 4, 5]), pick([1, 2, 2, 3]), pick([0, 1, 1, 2, 3, 7, 8, -1]), pick([0, 1])
        GH, GW, N = pick([1, 2, 4, 8, 16, 6]), pick([2, 4, 8, 16, 12]), pick([1, 2, 3, 4, 8, 16, 64])
        K, Nc = pick([64, 128, 192, 512, 96]), pick([64, 192, 256, 96])
        if tr:
            IH, IW, OH, OW = GH, GW, s * GH, s * GW
        else:
            OH, OW = GH, GW
            IH, IW = (GH - 1) * s + k - 2 * p + pick([0, 0, s - 1]), (GW - 1) * s + k - 2 * p + pick([0, 0, s - 1])
        over = {}
        r = pick(list(range(16)))
        if r == 0:
            over["KW"] = k + 1
        elif r == 1:
            over["OH"] = OH + 1
        elif r == 2:
            over["K1"] = 64 if K != 64 else 128
        elif r == 3:
            over["mode"] = 2
        mode = over.pop("mode", pick([1, 1, 0]))
        d = dict(IH=IH, IW=IW, OH=OH, OW=OW, KH=k, KW=k, stride=s, pad=p, transposed=tr, ldx=K + pick([0, 0, 8, 4, 2]), mode=mode)
        d.update(over)
        out.append(desc(N, 0, 0, K, Nc, **d))
    return out
