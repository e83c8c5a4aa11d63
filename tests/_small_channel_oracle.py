"""CPU oracle of the small-channel ends of the U-Net (csrc/small_channel.hip): Conv2d(Cin <= 4, C, 3|1), Conv2d(C, Cs <= 4, 1), their
gradients, the dual 3x3 + 1x1 launch with its chores and the final conv with GroupNorm + Mish in its load.

Three things live here, shared by tests/test_small_channel_cpu.py and tests/test_small_channel_kernels_gpu.py:
  * float64 references on NHWC tensors with the weights in the kernels' layouts ([ks][ks][Cin][Cout] and [C][Cs]), and a float32
    emulation of the GroupNorm-fused kernel's arithmetic (what its per-pixel bound rests on);
  * a restatement of the host dispatch (plan_*: which kernel instantiation a call reaches, its grid and the iterations of its busiest
    workgroup), of the three *_supported predicates and of the argument conditions of every entry point (*_accepts);
  * the case lists, and edges(): which instantiations and dispatch edges those lists reach, by name.
The rules are read from the .hip file and written again here; nothing is imported from the package."""
from collections import namedtuple

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
GSUM_SCALE = 1048576.0            # csrc/common.h MI_GSUM_SCALE: 20 fraction bits
GSUM_POISON = 1 << 60             # |slot| >= 2^60: the reader returns NaN
WG_BLOCKS = 768                   # weight-gradient workgroups = partial tiles in the workspace
MAX_PIXELS, MAX_WIDE_BYTES = 57344, 35 << 20
# worst per-pixel error of the float32 emulation of the GroupNorm-fused final conv against float64, relative to sum_c |mish| |w| + |bias|
# (re-measured and held in tests/test_small_channel_cpu.py: 2.94e-7 and 3.23e-6, rounded up for another CPU's exp; the GPU test allows the
# kernel four times as much): ordinary samples, and a sample of constant x, where x sc + sh cancels at rstd = 1 / sqrt(eps)
GN_EMUL_FIGURE, GN_EMUL_FIGURE_CONST = 3.5e-7, 4.0e-6


# ------------------------------------------------------------------------------------------------------------ references
def bf16_round(t):
    """Round to nearest even onto bf16, returned as float64 (t holds float32-representable values)."""
    return t.to(F32).to(BF).to(F64)


def rel(got, ref):
    got, ref = got.detach().to(F64).cpu(), ref.detach().to(F64).cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def _padded(x, ks):
    N, H, W, C = x.shape
    p = ks // 2
    xp = torch.zeros(N, H + 2 * p, W + 2 * p, C, dtype=F64)
    xp[:, p:p + H, p:p + W] = x
    return xp


def conv_fwd_ref(x, w, bias, ks):
    """x [N][H][W][Cin], w [ks][ks][Cin][Cout], pad ks // 2 -> y [N][H][W][Cout]."""
    N, H, W, _ = x.shape
    xp = _padded(x.to(F64), ks)
    y = torch.zeros(N, H, W, w.shape[-1], dtype=F64)
    for ky in range(ks):
        for kx in range(ks):
            y += torch.einsum("nhwi,io->nhwo", xp[:, ky:ky + H, kx:kx + W], w[ky, kx].to(F64))
    return y if bias is None else y + bias.to(F64)


def conv_wgrad_ref(x, dy, ks):
    """dW[ky][kx][ci][co] = sum_px x[px + (ky, kx) - pad][ci] dy[px][co] as shifted contractions."""
    N, H, W, Cin = x.shape
    xp = _padded(x.to(F64), ks)
    dW = torch.zeros(ks, ks, Cin, dy.shape[-1], dtype=F64)
    for ky in range(ks):
        for kx in range(ks):
            dW[ky, kx] = torch.einsum("nhwi,nhwo->io", xp[:, ky:ky + H, kx:kx + W], dy.to(F64))
    return dW


def cout_fwd_ref(x, w, bias):
    """x [M][C], w [C][Cs] -> y [M][Cs]."""
    y = x.to(F64) @ w.to(F64)
    return y if bias is None else y + bias.to(F64)


def cout_dgrad_ref(dy, w):
    return dy.to(F64) @ w.to(F64).t()


def cout_wgrad_ref(x, dy):
    return x.to(F64).t() @ dy.to(F64)


def mish64(z):
    return z * torch.tanh(torch.nn.functional.softplus(z, threshold=1e9))


def gn_sums(x):
    """x [N][HW][C] -> the epilogue's fixed-point sums [N][C / 16][2] int64 (the layout of functional.gn_sums_encode)."""
    N, HW, C = x.shape
    xd = x.to(F64).view(N, HW, C // 16, 16)
    s = torch.stack([xd.sum((1, 3)), (xd * xd).sum((1, 3))], dim=-1)
    return torch.round(s * GSUM_SCALE).to(torch.int64)


def gn_stats_from_sums(sums, HW, C, G):
    """-> (mean, var) [N][G] float64 decoded from the 20-fraction-bit sums; NaN for a sample with a poisoned slot."""
    N = sums.shape[0]
    Cg = C // G
    grp = sums.view(N, G, Cg // 16, 2)
    poisoned = (grp.abs() >= GSUM_POISON).any(3).any(2)
    tot = grp.sum(2).to(F64) / (GSUM_SCALE * HW * Cg)
    mean = tot[..., 0]
    var = (tot[..., 1] - mean * mean).clamp_min(0.0)
    nan = torch.full_like(mean, float("nan"))
    return torch.where(poisoned, nan, mean), torch.where(poisoned, nan, var)


def gn_mish_conv_ref(x, sums, gamma, beta, G, eps, w, bias, absolute=False):
    """y[n][p][j] = bias[j] + sum_c mish(groupnorm(x)[n][p][c]) w[c][j], statistics from the sums.  absolute: sum_c |mish| |w| + |bias|."""
    N, HW, C = x.shape
    mean, var = gn_stats_from_sums(sums, HW, C, G)
    rstd = 1.0 / torch.sqrt(var + eps)
    Cg = C // G
    z = (x.to(F64).view(N, HW, G, Cg) - mean[:, None, :, None]) * rstd[:, None, :, None]
    z = z.reshape(N, HW, C) * gamma.to(F64) + beta.to(F64)
    m = mish64(z)
    if absolute:
        y = m.abs() @ w.to(F64).abs()
        return y if bias is None else y + bias.to(F64).abs()
    y = m @ w.to(F64)
    return y if bias is None else y + bias.to(F64)


def gn_mish_conv_emul32(x, sums, gamma, beta, G, eps, w, bias, seed=0):
    """The kernel's arithmetic in float32: coefficients resolved in double then float (rstd = 1 / sqrtf((float)var + eps), sc = gamma rstd,
    sh = beta - mean sc), z = x sc + sh, mish_fast_f's form x * w / (w + 2) with w = e (e + 2), e = exp(min(x, 20)), exp and the reciprocal
    each carrying a 2^-21 relative error of random sign; a lane's 4 CK channels summed in order, the 8 lanes by a tree, bias last."""
    N, HW, C = x.shape
    g = torch.Generator().manual_seed(seed)
    mean, var = gn_stats_from_sums(sums, HW, C, G)
    rstd = (1.0 / torch.sqrt(var.to(F32) + torch.tensor(eps, dtype=F32))).to(F32)
    Cg = C // G
    sc = gamma.to(F32) * rstd.repeat_interleave(Cg, 1)                        # [N][C]
    sh = beta.to(F32) - mean.to(F32).repeat_interleave(Cg, 1) * sc
    z = x.to(F32) * sc[:, None, :] + sh[:, None, :]

    def wobble(t):
        s = torch.randint(0, 2, t.shape, generator=g).to(F32) * 2 - 1
        return t * (1 + s * 2.0 ** -21)
    e = wobble(torch.exp(z.clamp_max(20.0)))
    ww = e * (e + 2.0)
    m = z * ww * wobble(1.0 / (ww + 2.0))
    CK = C // 32
    terms = m[..., None] * w.to(F32)                                          # [N][HW][C][Cs]
    lanes = []
    for sub in range(8):
        a = torch.zeros(N, HW, w.shape[1], dtype=F32)
        for k in range(CK):
            for e4 in range(4):
                a = a + terms[:, :, 4 * (sub + 8 * k) + e4]
        lanes.append(a)
    for o in (1, 2, 4):
        lanes = [lanes[i] + lanes[i ^ o] for i in range(8)]
    y = lanes[0]
    return y if bias is None else y + bias.to(F32)


# ------------------------------------------------------------------------------------------------------------ operands
def ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).to(F64)


def randn(shape, seed, bf16=False, scale=1.0):
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F32) * scale
    return bf16_round(t) if bf16 else t.to(F64)


def operand(shape, kind, seed, bf16=False, amp=4, scale=1.0):
    """kind 'int': integers in {-amp..amp} (exact in fp32 and bf16); 'randn': float32 (bf16 when stored so) normal values."""
    return ints(shape, -amp, amp, seed) if kind == "int" else randn(shape, seed, bf16, scale)


def init_content(shape, seed, bf16=False, kind="int"):
    """What a += output holds before the launch: non-zero small integers ({-3..3} \\ {0}), or rounded normal values."""
    if kind == "int":
        t = ints(shape, 1, 3, seed) * (ints(shape, 0, 1, seed + 1) * 2 - 1)
        return t
    return randn(shape, seed, bf16)


# ------------------------------------------------------------------------------------------------------------ dispatch, restated
def log2_exact(v):
    return v.bit_length() - 1 if v > 0 and v & (v - 1) == 0 else -1


def cdiv(a, b):
    return -(-a // b)


def b(v):
    return "true" if v else "false"


def cin_tiled_geom(ks, H, W, ldx, x_aligned=True):
    w_sh, hw_sh = log2_exact(W), log2_exact(H * W)
    rows = 64 // W if w_sh >= 0 and W <= 64 else 0
    return bool(ks == 3 and w_sh >= 0 and hw_sh >= 0 and ldx == 4 and x_aligned and rows >= 1 and H % rows == 0 and (rows + 2) * (W + 2) <= 256)


def cin_lds_rule(ks, Cin, Cout):
    """The weight gradient's reduce area, 3 partial sets of ks ks Cin (Cout / 4) float4, must fit 48 KiB."""
    return 3 * ks * ks * Cin * (Cout // 4) * 16 <= 48 * 1024


def cin_bf16_supported(ks, N, H, W, Cin, Cout, ldx):
    return bool(N > 0 and 1 <= Cin <= 4 and Cout in (64, 128, 256) and (N * H * W) % 64 == 0 and cin_tiled_geom(ks, H, W, ldx) and cin_lds_rule(3, Cin, Cout))


def cin_dual_supported(N, H, W, Cin, Cout, ldx):
    return bool(N > 0 and 1 <= Cin <= 4 and Cout >= 4 and Cout % 4 == 0 and Cout <= 256 and 256 % (Cout // 4) == 0 and (N * H * W) % 64 == 0
                and cin_tiled_geom(3, H, W, ldx))


def cout_gn_supported(C, Cs, G):
    return bool(C in (64, 128) and 1 <= Cs <= 4 and G > 0 and C % G == 0 and (C // G) % 16 == 0)


def _form(H, W, ldx, x_aligned):
    pow2 = log2_exact(W) >= 0 and log2_exact(H * W) >= 0
    vec = ldx % 4 == 0 and x_aligned
    return (True, True) if pow2 and vec else (False, True) if vec else (False, False)


def plan_cin_fwd(ks, N, H, W, Cin, Cout, ldx, x_aligned=True, y_bf16=False):
    """mi_conv_small_cin_fwd_io -> dict(kernel, grid, iters, ...); kernel None: refused (bf16 output off the tiled kernel)."""
    M = N * H * W
    if cin_tiled_geom(ks, H, W, ldx, x_aligned) and Cout <= 256 and M % 64 == 0:
        nt = M // 64
        grid = min(nt, 768)
        return dict(kernel=f"small_cin3x3_fwd_tiled_kernel<{Cin}, {b(y_bf16)}>", tiled=True, grid=grid, iters=cdiv(nt, grid), ntiles=nt,
                    wrap=nt > 768)
    if y_bf16:
        return dict(kernel=None)
    pp = 256 // (Cout // 4)
    blocks = min(cdiv(M, 2 * pp), 4096)
    step = blocks * pp
    iters = cdiv(M, 2 * step)
    p2, v = _form(H, W, ldx, x_aligned)
    return dict(kernel=f"small_cin_fwd_kernel<{Cin}, {ks}, {b(p2)}, {b(v)}>", tiled=False, grid=blocks, iters=iters, capped=cdiv(M, 2 * pp) > 4096,
                masked=M - (iters - 1) * 2 * step < 2 * step, form=(p2, v))


def plan_cin_dual(N, H, W, Cin, Cout, y_bf16=False):
    nt = N * H * W // 64
    grid = min(nt, 768)
    return dict(kernel=f"small_cin3x3_fwd_tiled_kernel<{Cin}, {b(y_bf16)}, true>", tiled=True, grid=grid, iters=cdiv(nt, grid), ntiles=nt, wrap=nt > 768)


def small_wgrad_workspace(outputs):
    return WG_BLOCKS * outputs * 4


def plan_cin_wgrad(ks, N, H, W, Cin, Cout, ldx, x_aligned=True, dy_bf16=False, ws_bytes=0):
    """mi_conv_small_cin_wgrad_io -> dict(kernel, grid, per, owners, idle, ragged, reduce = 'ws' | 'atomic')."""
    M = N * H * W
    reduce = "ws" if ws_bytes >= small_wgrad_workspace(ks * ks * Cin * Cout) else "atomic"
    if cin_tiled_geom(ks, H, W, ldx, x_aligned) and (Cout >= 128 or dy_bf16) and M % 64 == 0:
        nt = M // 64
        per = cdiv(nt, WG_BLOCKS)
        owners = cdiv(nt, per)
        return dict(kernel=f"small_cin3x3_wgrad_tiled_kernel<{Cin}, {b(dy_bf16)}>", tiled=True, grid=WG_BLOCKS, per=per, iters=per, owners=owners,
                    idle=WG_BLOCKS - owners, ragged=nt % per != 0, ntiles=nt, reduce=reduce)
    if dy_bf16:
        return dict(kernel=None)
    pp = 256 // (Cout // 4)
    per = cdiv(M, WG_BLOCKS)
    owners = cdiv(M, per)
    p2, v = _form(H, W, ldx, x_aligned)
    return dict(kernel=f"small_cin_wgrad_kernel<{Cin}, {ks}, {b(p2)}, {b(v)}>", tiled=False, grid=WG_BLOCKS, per=per, iters=cdiv(per, pp), owners=owners,
                idle=WG_BLOCKS - owners, ragged=M % per != 0, form=(p2, v), reduce=reduce)


def plan_cout(op, M, C, Cs, wide_bf16=False, ws_bytes=0):
    """mi_conv1x1_small_cout_io."""
    if op == 0:
        groups = cdiv(M, 32)
        blocks = min(groups, 1024)
        return dict(kernel=f"small_cout_fwd_kernel<{C // 32}, {b(wide_bf16)}>", grid=blocks, iters=cdiv(groups, blocks), capped=groups > 1024, ragged=M % 32 != 0)
    if op == 1:
        pp = 256 // (C // 4)
        blocks = min(cdiv(M, pp), 4096)
        return dict(kernel=f"small_cout_dgrad_kernel<{b(wide_bf16)}>", grid=blocks, iters=cdiv(M, blocks * pp), capped=cdiv(M, pp) > 4096, ragged=M % pp != 0)
    per = cdiv(M, WG_BLOCKS)
    owners = cdiv(M, per)
    return dict(kernel=f"small_cout_wgrad_kernel<{b(wide_bf16)}>", grid=WG_BLOCKS, per=per, iters=cdiv(per, 256 // (C // 4)), owners=owners, idle=WG_BLOCKS - owners,
                ragged=M % per != 0, reduce="ws" if ws_bytes >= small_wgrad_workspace(4 * C) else "atomic")


def plan_cout_bwd(M, C, Cs, x_bf16=False, dx_bf16=False, ws_bytes=0):
    p = plan_cout(2, M, C, Cs, x_bf16, ws_bytes)
    p["kernel"] = f"small_cout_wgrad_kernel<{b(x_bf16)}, true, {b(dx_bf16)}>"
    return p


def plan_cout_gn(M, HW, C):
    """mi_conv1x1_small_cout_gn_fwd: contiguous runs of ppw pixels per workgroup, 32 pixels per iteration."""
    ppw = 32
    while M // ppw > 768 and HW % (2 * ppw) == 0:
        ppw *= 2
    blocks = cdiv(M, ppw)
    straddle = any(g0 // HW != min(g0 + 31, min(M, (g0 // ppw + 1) * ppw) - 1) // HW for g0 in range(0, M, 32))
    return dict(kernel=f"small_cout_fwd_gn_kernel<{C // 32}>", grid=blocks, ppw=ppw, iters=cdiv(ppw, 32), straddle=straddle, ragged=M % 32 != 0)


# ---- argument conditions of the entry points (the MI_REQUIREs); *_off: bytes past a 16-byte boundary
def cin_fwd_accepts(ks, N, H, W, Cin, Cout, ldx, ldy, x_off=0, y_off=0, w_off=0, y_bf16=False):
    if not (ks in (1, 3) and 1 <= Cin <= 4 and Cout >= 4 and Cout % 4 == 0 and Cout <= 1024 and 256 % (Cout // 4) == 0 and ldy % 4 == 0
            and y_off % (8 if y_bf16 else 16) == 0 and w_off % 16 == 0):
        return False
    return plan_cin_fwd(ks, N, H, W, Cin, Cout, ldx, x_off % 16 == 0, y_bf16)["kernel"] is not None


def cin_dual_accepts(N, H, W, Cin, Cout, ldx, ldy3, ldy1, x_off=0, y3_off=0, y1_off=0, w3_off=0, w1_off=0, y3_bf16=False):
    return bool(cin_dual_supported(N, H, W, Cin, Cout, ldx) and x_off % 16 == 0 and ldy3 % 4 == 0 and ldy1 % 4 == 0
                and y3_off % (8 if y3_bf16 else 16) == 0 and y1_off % 16 == 0 and w3_off % 16 == 0 and w1_off % 16 == 0)


def chores_accept(zero, zero_bytes=0, zero_off=0, gather=False, gather_row=0, gather_n=0, src_off=0, dst_off=0):
    if zero and not (zero_bytes % 8 == 0 and zero_off % 8 == 0 and zero_bytes < (1 << 30)):
        return False
    if gather and not (gather_row > 0 and gather_row % 4 == 0 and gather_n > 0 and gather_row * gather_n < (1 << 30) and src_off % 16 == 0 and dst_off % 16 == 0):
        return False
    return True


def cin_wgrad_accepts(ks, N, H, W, Cin, Cout, ldx, lddy, x_off=0, dy_off=0, dy_bf16=False):
    if not (ks in (1, 3) and 1 <= Cin <= 4 and Cout in (64, 128, 256) and lddy % 4 == 0 and dy_off % (8 if dy_bf16 else 16) == 0
            and cin_lds_rule(ks, Cin, Cout)):
        return False
    return plan_cin_wgrad(ks, N, H, W, Cin, Cout, ldx, x_off % 16 == 0, dy_bf16)["kernel"] is not None


def cout_accepts(op, M, C, Cs, lda, ldo, a_off=0, out_off=0, wide_bf16=False, has_b=True):
    if not (1 <= Cs <= 4 and C in (32, 64, 128, 256) and M > 0):
        return False
    wal = 8 if wide_bf16 else 16
    if op == 0:
        return C <= 128 and lda % 4 == 0 and a_off % wal == 0
    if op == 1:
        return ldo % 4 == 0 and out_off % wal == 0
    if op == 2:
        return has_b and C >= 64 and lda % 4 == 0 and a_off % wal == 0
    return False


def cout_bwd_accepts(M, C, Cs, ldx, lddx, x_off=0, dx_off=0, x_bf16=False, dx_bf16=False):
    return bool(1 <= Cs <= 4 and C in (64, 128, 256) and M > 0 and ldx % 4 == 0 and lddx % 4 == 0 and x_off % (8 if x_bf16 else 16) == 0
                and dx_off % (8 if dx_bf16 else 16) == 0)


def cout_gn_accepts(M, HW, C, Cs, G, ldx, ldy, x_off=0, y_off=0):
    return bool(M > 0 and HW > 0 and M % HW == 0 and cout_gn_supported(C, Cs, G) and ldx % 4 == 0 and ldy == 4 and x_off % 8 == 0 and y_off % 16 == 0)


# ------------------------------------------------------------------------------------------------------------ cases
class _Case:
    def __repr__(self):
        return self.name


def _nt(name, fields):
    base = namedtuple(name, ["name"] + fields.split())
    return type(name, (_Case, base), {"__slots__": ()})


# ldx classes: 'dense' (= Cin), 5, 8, 4, 'off4' (ldx 4, x four bytes past a 16-byte boundary); ldy classes 0: Cout, 1: Cout + 4, 2: 2 Cout + 8
Fwd = _nt("Fwd", "ks N H W Cin Cout ldx xoff bias ldyk y16")
Dual = _nt("Dual", "N H W Cin Cout y16 bias1 zero_bytes gather_row gather_n ldyk")
Wg = _nt("Wg", "ks N H W Cin Cout ldx xoff lddyk dy16")
C0 = _nt("C0", "M C Cs x16 ldak ldo bias")
C1 = _nt("C1", "M C Cs dx16 acc lddy ldok")
C2 = _nt("C2", "M C Cs x16 dx16 acc ldak")
Gn = _nt("Gn", "N HW C G Cs ldxk bias special")


def ldy_of(Cout, k):
    return (Cout, Cout + 4, 2 * Cout + 8)[k]


def _fwd_cases():
    out = []

    def add(ks, shp, cin, cout, ldx, xoff, bias, ldyk, y16=False, tag=""):
        N, H, W = shp
        ld = cin if ldx == "dense" else ldx
        out.append(Fwd(f"k{ks}-{N}x{H}x{W}-{cin}to{cout}-ldx{ld}{'+4B' if xoff else ''}-{'b' if bias else 'nb'}-ldy{ldy_of(cout, ldyk)}{'-y16' if y16 else ''}{tag}",
                       ks, N, H, W, cin, cout, ld, xoff, bias, ldyk, y16))
    couts = (4, 8, 64, 128, 512, 1024)
    pv_shapes = ((1, 1, 1), (1, 4, 4), (4, 4, 8))
    v_shapes = ((2, 28, 28), (3, 14, 14), (5, 7, 7), (1, 3, 5))
    s_shapes = ((2, 28, 28), (3, 14, 14), (5, 7, 7), (1, 1, 1), (1, 3, 5), (1, 4, 4), (4, 4, 8))
    i = 0
    for cin in (1, 2, 3, 4):
        for ks in (1, 3):
            # POW2 and VEC: power-of-two images the tiled kernel does not take (fewer rows than a tile, M % 64 != 0), or ldx 8
            for r in range(2):
                add(ks, pv_shapes[i % 3], cin, couts[i % 6], (4, 8)[r], 0, i % 2 == 0, i % 3)
                i += 1
            # VEC only: 28x28, 14x14, 7x7, 3x5
            for r in range(2):
                add(ks, v_shapes[i % 4], cin, couts[(i + r) % 6], (4, 8)[(i + r) % 2], 0, i % 2 == 1, (i + 1) % 3)
                i += 1
            # scalar loads: dense ldx = Cin < 4, ldx 5, x four bytes off
            dense = ("dense", 5) if cin < 4 else (5, 5)
            for r, (ldx, xoff) in enumerate(((dense[0], 0), (5, 0), (4, 4))):
                add(ks, s_shapes[(i + r) % 7], cin, couts[(i + 2 * r) % 6], ldx, xoff, (i + r) % 2 == 0, (i + r) % 3)
            i += 1
    # 512 / 1024 channels on a geometry the tiled kernel would take: never tiled
    add(3, (3, 8, 8), 3, 512, 4, 0, True, 1)
    add(3, (1, 2, 32), 1, 1024, 4, 0, False, 0)
    add(3, (2, 4, 16), 2, 64, 8, 0, True, 0, tag="-tiledgeom-ldx8")
    # the 4 096-workgroup cap's second round with an odd M, and an odd M below the cap (the masked second pixel)
    add(3, (1, 91, 91), 1, 1024, 4, 0, True, 0, tag="-cap")
    add(1, (1, 91, 91), 3, 1024, 3, 0, False, 0, tag="-cap")
    add(3, (5, 7, 7), 3, 128, 4, 0, True, 0, tag="-oddM")
    return out


def _tiled_cases():
    out = []
    shapes = ((1, 1, 64), (1, 2, 32), (2, 4, 16), (3, 8, 8), (1, 16, 4), (1, 32, 2), (1, 64, 1), (2, 64, 64), (1, 16, 64))
    couts = (4, 16, 64, 128, 256)
    i = 0
    for y16 in (False, True):
        for N, H, W in shapes:
            cin, cout = i % 4 + 1, couts[i % 5]
            out.append(Fwd(f"tiled-{N}x{H}x{W}-{cin}to{cout}-{'b' if i % 3 else 'nb'}-ldy{ldy_of(cout, i % 3)}{'-y16' if y16 else ''}",
                           3, N, H, W, cin, cout, 4, 0, i % 3 != 0, i % 3, y16))
            i += 1
    for y16 in (False, True):   # 896 tiles > 768 workgroups: a second tile for some while the others prefetch past the end
        out.append(Fwd(f"tiled-14x64x64-3to8-b-ldy12-wrap{'-y16' if y16 else ''}", 3, 14, 64, 64, 3, 8, 4, 0, True, 1, y16))
    return out


def _dual_cases():
    out = []
    shapes = ((1, 1, 64), (2, 4, 16), (3, 8, 8), (1, 32, 2), (1, 64, 1), (2, 64, 64), (1, 16, 64), (1, 2, 32))
    couts = (64, 4, 128, 16, 256)
    chores = ((0, 0, 0), (8, 0, 0), (0, 4, 1), (8 * 1001, 132, -1), (8 * 1001, 0, 0), (0, 132, -1), (8, 4, -1), (8, 132, 1))
    i = 0
    for y16 in (False, True):
        for N, H, W in shapes:
            cin, cout = (i + i // 4) % 4 + 1, couts[i % 5]
            zb, gr, gn = chores[(i + i // 8) % 8]
            gn = N if gn < 0 else gn
            out.append(Dual(f"dual-{N}x{H}x{W}-{cin}to{cout}{'-y16' if y16 else ''}-{'b1' if i % 2 else 'nb1'}-z{zb}-g{gr}x{gn}",
                            N, H, W, cin, cout, y16, i % 2 == 1, zb, gr, gn, i % 3))
            i += 1
    out.append(Dual("dual-14x64x64-2to8-y16-b1-z8008-g132x14-wrap", 14, 64, 64, 2, 8, True, True, 8 * 1001, 132, 14, 1))
    return out


def _wg_cases():
    out = []

    def add(ks, shp, cin, cout, ldx, xoff, lddyk, dy16=False, tag=""):
        N, H, W = shp
        ld = cin if ldx == "dense" else ldx
        out.append(Wg(f"wg-k{ks}-{N}x{H}x{W}-{cin}to{cout}-ldx{ld}{'+4B' if xoff else ''}-lddy{cout + 8 * lddyk}{'-dy16' if dy16 else ''}{tag}",
                      ks, N, H, W, cin, cout, ld, xoff, lddyk, dy16))
    # the Cout the 48 KiB rule admits, per (ks, Cin)
    admit = {(1, c): (64, 128, 256) for c in (1, 2, 3, 4)}
    admit.update({(3, 1): (64, 128, 256), (3, 2): (64, 128), (3, 3): (64, 128), (3, 4): (64,)})
    pv_shapes = ((1, 1, 1), (1, 4, 4), (4, 4, 8))
    v_shapes = ((2, 7, 7), (1, 1, 769), (2, 28, 28), (4, 28, 28))
    s_shapes = ((1, 1, 1), (2, 7, 7), (1, 1, 769), (2, 28, 28), (4, 28, 28), (1, 4, 4))
    i = 0
    for cin in (1, 2, 3, 4):
        for ks in (1, 3):
            co = admit[(ks, cin)]
            add(ks, pv_shapes[i % 3], cin, co[i % len(co)], (4, 8)[i % 2], 0, i % 2)
            add(ks, v_shapes[i % 4], cin, co[(i + 1) % len(co)], (4, 8)[(i + 1) % 2], 0, (i + 1) % 2)
            add(ks, v_shapes[(i + 2) % 4], cin, co[(i + 2) % len(co)], 4, 0, i % 2)
            dense = "dense" if cin < 4 else 5
            add(ks, s_shapes[i % 6], cin, co[i % len(co)], dense, 0, i % 2)
            add(ks, s_shapes[(i + 3) % 6], cin, co[(i + 1) % len(co)], 4 if i % 2 else 5, 4 if i % 2 else 0, (i + 1) % 2)
            i += 1
    add(3, (1, 1, 1), 1, 256, 4, 0, 0, tag="-lds-edge")
    add(3, (4, 28, 28), 1, 256, 4, 0, 1, tag="-lds-edge")
    add(3, (2, 28, 28), 4, 64, 4, 0, 0, tag="-lds-edge")
    # fp32 dy at 64 channels on the tiled geometry: the untiled kernel, POW2 and VEC
    add(3, (3, 8, 8), 4, 64, 4, 0, 1, tag="-tiledgeom")
    add(3, (2, 64, 64), 2, 64, 4, 0, 0, tag="-tiledgeom")
    return out


def _wgt_cases():
    out = []
    shapes = {1: (1, 1, 64), 3: (3, 8, 8), 767: (767, 8, 8), 768: (12, 64, 64), 769: (769, 2, 32), 896: (14, 64, 64)}
    i = 0
    for dy16 in (False, True):
        for nt in (1, 3, 767, 768, 769, 896):
            cin = i % 4 + 1
            if cin == 4 and not dy16:
                cin = 3                       # (Cin 4 admits Cout 64 only, which fp32 dy sends to the untiled kernel: <4, false> is out of reach)
            cout = 64 if cin == 4 else (64 if dy16 and i % 3 == 0 else 128)
            N, H, W = shapes[nt]
            out.append(Wg(f"wgt-{nt}tiles-{N}x{H}x{W}-{cin}to{cout}-lddy{cout + 8 * (i % 2)}{'-dy16' if dy16 else ''}", 3, N, H, W, cin, cout, 4, 0, i % 2, dy16))
            i += 1
    out.append(Wg("wgt-3tiles-3x8x8-1to256-lddy256", 3, 3, 8, 8, 1, 256, 4, 0, 0, False))
    out.append(Wg("wgt-769tiles-769x8x8-1to256-lddy264-dy16", 3, 769, 8, 8, 1, 256, 4, 0, 1, True))
    out.append(Wg("wgt-1tiles-1x64x1-4to64-lddy64-dy16", 3, 1, 64, 1, 4, 64, 4, 0, 0, True))
    return out


def _c0_cases():
    out = []
    Ms = (1, 31, 33, 1568, 32805)
    i = 0
    for C in (32, 64, 128):
        for Cs in (1, 2, 3, 4):
            for x16 in (False, True):
                for r in range(2):
                    M = Ms[(i + r) % 5]
                    ldo = (Cs, 4, 8)[(i + r) % 3]
                    out.append(C0(f"c0-M{M}-{C}to{Cs}{'-x16' if x16 else ''}-lda{C + 8 * ((i + r) % 2)}-ldo{ldo}-{'b' if (i // 2 + r) % 2 else 'nb'}",
                                  M, C, Cs, x16, (i + r) % 2, ldo, (i // 2 + r) % 2 == 1))
                i += 1
    return out


def _c1_cases():
    out = []
    Ms = (1, 7, 1568)
    i = 0
    for C in (32, 64, 128, 256):
        for Cs in (1, 2, 3, 4):
            for dx16 in (False, True):
                for acc in (False, True):
                    M = Ms[i % 3]
                    lddy = (Cs, 4)[(i // 2) % 2]
                    out.append(C1(f"c1-M{M}-{Cs}to{C}{'-dx16' if dx16 else ''}{'-acc' if acc else ''}-lddy{lddy}-ldo{C + 8 * (i % 2)}", M, C, Cs, dx16, acc, lddy, i % 2))
                    i += 1
    for dx16 in (False, True):      # 16 421 pixels at 4 per workgroup: past the 4 096-workgroup cap, ragged
        out.append(C1(f"c1-M16421-3to256{'-dx16' if dx16 else ''}-acc-lddy4-ldo264-cap", 16421, 256, 3, dx16, True, 4, 1))
    return out


def _c2_cases():
    out = []
    Ms = (1, 98, 769, 3136)
    i = 0
    for C in (64, 128, 256):
        for Cs in (1, 2, 3, 4):
            for x16 in (False, True):
                for dx16 in (False, True):
                    M = Ms[(i + i // 4) % 4]
                    out.append(C2(f"c2-M{M}-{C}x{Cs}{'-x16' if x16 else ''}{'-dx16' if dx16 else ''}{'-acc' if i % 3 == 0 else ''}-ldx{C + 8 * (i % 2)}",
                                  M, C, Cs, x16, dx16, i % 3 == 0, i % 2))
                    i += 1
    return out


def _gn_cases():
    out = []
    shapes = ((1, 36), (3, 36), (2, 49), (1, 1), (8, 1024), (7, 4096))
    i = 0
    for C, G in ((64, 1), (64, 2), (64, 4), (128, 1), (128, 2), (128, 4), (128, 8)):
        for N, HW in shapes:
            if HW == 4096 and (i // 6) % 2:          # the 28 672-pixel slab once per two (C, G)
                N, HW = 3, 36
            Cs = (i + i // 4) % 4 + 1
            out.append(Gn(f"gn-{N}x{HW}-{C}g{G}to{Cs}-ldx{C + 8 * (i % 2)}-{'b' if (i // 2) % 2 else 'nb'}-{i}", N, HW, C, G, Cs, i % 2, (i // 2) % 2 == 1, ""))
            i += 1
    out.append(Gn("gn-3x36-128g4to3-const", 3, 36, 128, 4, 3, 0, True, "const"))
    out.append(Gn("gn-3x36-64g2to2-poison", 3, 36, 64, 2, 2, 1, True, "poison"))
    return out


FWD_CASES, TILED_CASES, DUAL_CASES = _fwd_cases(), _tiled_cases(), _dual_cases()
WG_CASES, WGT_CASES = _wg_cases(), _wgt_cases()
C0_CASES, C1_CASES, C2_CASES, GN_CASES = _c0_cases(), _c1_cases(), _c2_cases(), _gn_cases()
WS_MODES = ("full", "null", "short")
# instantiations the product library cannot reach (see edges())
UNREACHABLE = {"small_cin3x3_wgrad_tiled_kernel<4, false>"}


def all_instantiations():
    """Every kernel symbol the dispatch rules name."""
    k = set()
    for cin in (1, 2, 3, 4):
        for ks in (1, 3):
            for p2, v in ((True, True), (False, True), (False, False)):
                k.add(f"small_cin_fwd_kernel<{cin}, {ks}, {b(p2)}, {b(v)}>")
                k.add(f"small_cin_wgrad_kernel<{cin}, {ks}, {b(p2)}, {b(v)}>")
        for h in (False, True):
            k.add(f"small_cin3x3_fwd_tiled_kernel<{cin}, {b(h)}>")
            k.add(f"small_cin3x3_fwd_tiled_kernel<{cin}, {b(h)}, true>")
            k.add(f"small_cin3x3_wgrad_tiled_kernel<{cin}, {b(h)}>")
    for h in (False, True):
        for ck in (1, 2, 4):
            k.add(f"small_cout_fwd_kernel<{ck}, {b(h)}>")
        k.add(f"small_cout_dgrad_kernel<{b(h)}>")
        k.add(f"small_cout_wgrad_kernel<{b(h)}>")
        for d in (False, True):
            k.add(f"small_cout_wgrad_kernel<{b(h)}, true, {b(d)}>")
    k.update({"small_cout_fwd_gn_kernel<2>", "small_cout_fwd_gn_kernel<4>"})
    return k


def fwd_plan(c):
    return plan_cin_fwd(c.ks, c.N, c.H, c.W, c.Cin, c.Cout, c.ldx, c.xoff == 0, c.y16)


def wg_plan(c, ws_bytes=0):
    return plan_cin_wgrad(c.ks, c.N, c.H, c.W, c.Cin, c.Cout, c.ldx, c.xoff == 0, c.dy16, ws_bytes)


def case_sizes(c):
    """(pixels, bytes of the wide tensor) of a case."""
    if isinstance(c, (Fwd, Wg)):
        M = c.N * c.H * c.W
        wide = ldy_of(c.Cout, c.ldyk) if isinstance(c, Fwd) else c.Cout + 8 * c.lddyk
        return M, M * wide * (2 if (c.y16 if isinstance(c, Fwd) else c.dy16) else 4)
    if isinstance(c, Dual):
        M = c.N * c.H * c.W
        return M, M * ldy_of(c.Cout, c.ldyk) * 4
    if isinstance(c, Gn):
        return c.N * c.HW, c.N * c.HW * (c.C + 8) * 2
    return c.M, c.M * (c.C + 8) * 4


def edges():
    """name -> the cases that reach it.  Instantiations by their symbol, dispatch edges by a word."""
    e = {}

    def hit(key, c):
        e.setdefault(key, []).append(c.name)
    for c in FWD_CASES + TILED_CASES:
        p = fwd_plan(c)
        hit(p["kernel"], c)
        hit(f"fwd shape {c.N}x{c.H}x{c.W}", c)
        hit(f"fwd Cout {c.Cout}", c)
        hit(f"fwd ldy class {c.ldyk}", c)
        hit("fwd bias" if c.bias else "fwd no bias", c)
        if p["tiled"]:
            if p["wrap"]:
                hit("fwd tiled second tile (ntiles > 768)", c)
        else:
            hit("fwd ldx " + ("4+4B" if c.xoff else "dense" if c.ldx == c.Cin and c.Cin < 4 else str(c.ldx)), c)
            if p["capped"] and p["iters"] >= 2 and (c.N * c.H * c.W) % 2:
                hit("fwd 4096 cap second round odd M", c)
            if not p["capped"] and p["masked"] and (c.N * c.H * c.W) % 2:
                hit("fwd masked second pixel odd M", c)
            if cin_tiled_geom(3, c.H, c.W, 4) and c.ks == 3 and (c.N * c.H * c.W) % 64 == 0:
                hit("fwd untiled on the tiled geometry", c)
            if c.ks == 3 and log2_exact(c.W) >= 0 and log2_exact(c.H * c.W) >= 0 and c.ldx == 4 and not c.xoff and c.Cout <= 256:
                hit("fwd power of two but not tiled (rows / M % 64)", c)
    for c in DUAL_CASES:
        p = plan_cin_dual(c.N, c.H, c.W, c.Cin, c.Cout, c.y16)
        hit(p["kernel"], c)
        hit("dual bias1" if c.bias1 else "dual no bias1", c)
        hit("dual chores " + ("both" if c.zero_bytes and c.gather_row else "zero" if c.zero_bytes else "gather" if c.gather_row else "none"), c)
        if c.zero_bytes:
            hit(f"dual zero {c.zero_bytes} bytes", c)
        if c.gather_row:
            hit(f"dual gather row {c.gather_row}", c)
            hit("dual gather n 1" if c.gather_n == 1 else "dual gather n N", c)
        if p["wrap"]:
            hit("dual second tile (ntiles > 768)", c)
    for c in WG_CASES + WGT_CASES:
        for mode in WS_MODES:
            full = small_wgrad_workspace(c.ks * c.ks * c.Cin * c.Cout)
            p = wg_plan(c, {"full": full, "null": 0, "short": full - 4}[mode])
            hit(p["kernel"], c)
            hit(f"wgrad {'tiled' if p['tiled'] else 'untiled'} {mode} -> {p['reduce']}", c)
        hit(f"wgrad lddy class {c.lddyk}", c)
        if p["tiled"]:
            hit(f"wgrad tiled ntiles {p['ntiles']}", c)
            hit(f"wgrad tiled Cout {c.Cout}{' dy16' if c.dy16 else ''}", c)
            if p["per"] == 1 and p["idle"]:
                hit("wgrad tiled per 1 idle workgroups", c)
            if p["per"] == 2 and p["ragged"]:
                hit("wgrad tiled per 2 ragged last owner", c)
        else:
            hit(f"wgrad M {c.N * c.H * c.W}", c)
            hit("wgrad ldx " + ("4+4B" if c.xoff else "dense" if c.ldx == c.Cin and c.Cin < 4 else str(c.ldx)), c)
            if p["idle"] > WG_BLOCKS // 2:
                hit("wgrad most workgroups own no pixel", c)
            if (c.ks, c.Cin, c.Cout) in ((3, 1, 256), (3, 4, 64)):
                hit(f"wgrad LDS edge {c.Cin}x{c.Cout}", c)
            if cin_tiled_geom(c.ks, c.H, c.W, c.ldx, not c.xoff) and (c.N * c.H * c.W) % 64 == 0:
                hit("wgrad untiled on the tiled geometry (fp32 dy, 64 channels)", c)
    for c in C0_CASES:
        p = plan_cout(0, c.M, c.C, c.Cs, c.x16)
        hit(p["kernel"], c)
        hit(f"c0 M {c.M}", c)
        hit(f"c0 Cs {c.Cs}", c)
        hit(f"c0 lda class {c.ldak}", c)
        hit("c0 ldo " + ("dense" if c.ldo == c.Cs else str(c.ldo)) + (" padding zeros" if c.ldo >= 4 > c.Cs else ""), c)
        hit("c0 bias" if c.bias else "c0 no bias", c)
        if p["capped"] and p["iters"] >= 2 and p["ragged"]:
            hit("c0 1024 cap second round ragged", c)
    for c in C1_CASES:
        p = plan_cout(1, c.M, c.C, c.Cs, c.dx16)
        hit(p["kernel"], c)
        hit(f"c1 M {c.M}", c)
        hit(f"c1 C {c.C} Cs {c.Cs}", c)
        hit(f"c1 {'dx16' if c.dx16 else 'dx32'} {'acc' if c.acc else 'store'}", c)
        hit("c1 lddy " + ("dense" if c.lddy == c.Cs else "4"), c)
        hit(f"c1 ldo class {c.ldok}", c)
        if p["capped"] and p["iters"] >= 2:
            hit("c1 4096 cap second round", c)
    for c in C2_CASES:
        for mode in WS_MODES:
            full = small_wgrad_workspace(4 * c.C)
            nb = {"full": full, "null": 0, "short": full - 4}[mode]
            hit(plan_cout(2, c.M, c.C, c.Cs, c.x16, nb)["kernel"], c)
            p = plan_cout_bwd(c.M, c.C, c.Cs, c.x16, c.dx16, nb)
            hit(p["kernel"], c)
            hit(f"c2 {mode} -> {p['reduce']}", c)
        hit(f"c2 M {c.M}", c)
        hit(f"c2 C {c.C} Cs {c.Cs}", c)
        if p["idle"] > WG_BLOCKS // 2:
            hit("c2 most workgroups own no pixel", c)
    for c in GN_CASES:
        p = plan_cout_gn(c.N * c.HW, c.HW, c.C)
        hit(p["kernel"], c)
        hit(f"gn C {c.C} G {c.G}", c)
        hit(f"gn Cs {c.Cs}", c)
        hit(f"gn shape {c.N}x{c.HW}", c)
        hit(f"gn ldx class {c.ldxk}", c)
        hit("gn bias" if c.bias else "gn no bias", c)
        if p["straddle"]:
            hit("gn 32-pixel group straddles samples", c)
        if p["ppw"] > 32:
            hit("gn ppw doubled", c)
        if p["ragged"]:
            hit("gn ragged last group", c)
        if c.special:
            hit("gn " + c.special, c)
    return e


REQUIRED_EDGES = (
    [f"fwd shape {s}" for s in ("2x28x28", "3x14x14", "5x7x7", "1x1x1", "1x3x5", "1x4x4", "4x4x8", "1x91x91", "1x1x64", "1x2x32", "2x4x16", "3x8x8", "1x16x4",
                                "1x32x2", "1x64x1", "2x64x64", "1x16x64", "14x64x64")]
    + [f"fwd Cout {c}" for c in (4, 8, 16, 64, 128, 256, 512, 1024)] + [f"fwd ldy class {k}" for k in (0, 1, 2)] + ["fwd bias", "fwd no bias"]
    + [f"fwd ldx {k}" for k in ("dense", "5", "8", "4", "4+4B")]
    + ["fwd 4096 cap second round odd M", "fwd masked second pixel odd M", "fwd untiled on the tiled geometry", "fwd power of two but not tiled (rows / M % 64)",
       "fwd tiled second tile (ntiles > 768)"]
    + ["dual bias1", "dual no bias1", "dual chores none", "dual chores zero", "dual chores gather", "dual chores both", "dual zero 8 bytes", "dual zero 8008 bytes",
       "dual gather row 4", "dual gather row 132", "dual gather n 1", "dual gather n N", "dual second tile (ntiles > 768)"]
    + [f"wgrad {t} {m} -> {r}" for t in ("tiled", "untiled") for m, r in (("full", "ws"), ("null", "atomic"), ("short", "atomic"))]
    + [f"wgrad M {m}" for m in (1, 98, 769, 1568, 3136)] + [f"wgrad ldx {k}" for k in ("dense", "5", "8", "4", "4+4B")] + ["wgrad lddy class 0", "wgrad lddy class 1"]
    + ["wgrad most workgroups own no pixel", "wgrad LDS edge 1x256", "wgrad LDS edge 4x64", "wgrad untiled on the tiled geometry (fp32 dy, 64 channels)"]
    + [f"wgrad tiled ntiles {n}" for n in (1, 3, 767, 768, 769, 896)] + ["wgrad tiled per 1 idle workgroups", "wgrad tiled per 2 ragged last owner"]
    + ["wgrad tiled Cout 64 dy16", "wgrad tiled Cout 128", "wgrad tiled Cout 128 dy16", "wgrad tiled Cout 256", "wgrad tiled Cout 256 dy16"]
    + [f"c0 M {m}" for m in (1, 31, 33, 1568, 32805)] + [f"c0 Cs {s}" for s in (1, 2, 3, 4)] + ["c0 lda class 0", "c0 lda class 1", "c0 bias", "c0 no bias"]
    + ["c0 ldo dense", "c0 ldo 4 padding zeros", "c0 ldo 8", "c0 ldo 8 padding zeros", "c0 1024 cap second round ragged"]
    + [f"c1 M {m}" for m in (1, 7, 1568, 16421)] + [f"c1 C {c} Cs {s}" for c in (32, 64, 128, 256) for s in (1, 2, 3, 4)]
    + [f"c1 {d} {a}" for d in ("dx16", "dx32") for a in ("acc", "store")] + ["c1 lddy dense", "c1 lddy 4", "c1 ldo class 0", "c1 ldo class 1", "c1 4096 cap second round"]
    + [f"c2 {m} -> {r}" for m, r in (("full", "ws"), ("null", "atomic"), ("short", "atomic"))] + [f"c2 M {m}" for m in (1, 98, 769, 3136)]
    + [f"c2 C {c} Cs {s}" for c in (64, 128, 256) for s in (1, 2, 3, 4)] + ["c2 most workgroups own no pixel"]
    + [f"gn C {c} G {g}" for c, g in ((64, 1), (64, 2), (64, 4), (128, 1), (128, 2), (128, 4), (128, 8))] + [f"gn Cs {s}" for s in (1, 2, 3, 4)]
    + [f"gn shape {s}" for s in ("1x36", "3x36", "2x49", "1x1", "8x1024", "7x4096")] + ["gn ldx class 0", "gn ldx class 1", "gn bias", "gn no bias"]
    + ["gn 32-pixel group straddles samples", "gn ppw doubled", "gn ragged last group", "gn const", "gn poison"]
)
