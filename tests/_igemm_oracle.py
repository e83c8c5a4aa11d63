"""CPU oracle of the generic convolution and weight-gradient kernels (csrc/igemm_conv.hip: igemm_kernel, igemm_fast_kernel;
csrc/wgrad.hip: wgrad_kernel, wgrad_fast_kernel, slab_sum_kernel, colsum_kernel).

Shared by tests/test_igemm_cpu.py, tests/test_igemm_kernels_gpu.py and tests/test_wgrad_generic_kernels_gpu.py:
  * float64 references written from the contract in include/mi_ddpm.h: shifted contractions over (tap, channel) for MiConvDesc (both
    directions, both weight layouts, two sources, bias, residual, accumulate) and over pixels for MiWgradDesc (both gather sides, two
    sources), and column sums;
  * a restatement of both host planners (igemm: tile rule, ring-kernel predicate, k-split rule, the taps of a parity class; wgrad:
    the pixel slices, the ring-kernel predicate, the XCD map).  The product library is built without MI_EXPERIMENT, so MI_IGEMM_FAST,
    MI_IGEMM_TILE, MI_WGRAD_FAST and MI_WGRAD_XCD are their defaults;
  * operand builders: views at a given pitch inside NaN-filled buffers (inputs) and between sentinels (outputs);
  * the case lists -- each case names the plan it is there for -- and edges(): which instantiations and kernel edges they reach.
The rules are read from the .hip files and written again here; nothing is imported from the package."""
import os
import sys
from collections import namedtuple

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _conv_pw_oracle import F32, F64, BF, bf16_round, init_content, ints, operand, randn, rel, seed  # noqa: E402,F401

NAN = float("nan")
SENT = -776.0                        # never-written sentinel
PAD = 64                             # elements in front of and behind a view
U = 2.0 ** -24
PLAN_CLASSES = 16                    # MI_IGEMM_PLAN_CLASSES

_CONV = ("N", "IH", "IW", "OH", "OW", "K", "Nc", "KH", "KW", "stride", "pad", "transposed", "w_kn", "mode", "K1", "ldx", "ldx2", "ldy", "ldr",
         "accumulate")
ConvD = namedtuple("ConvD", _CONV)
_WG = ("N", "GH", "GW", "DH", "DW", "Ci", "Cj", "KH", "KW", "stride", "pad", "gather_i", "mode", "I1", "ldp", "ldp2", "ldq")
WgD = namedtuple("WgD", _WG)


def _cdiv(a, b):
    return (a + b - 1) // b


def _up(a, b):
    return _cdiv(a, b) * b


# ------------------------------------------------------------------------------------------------------------ igemm planner, restated
IgemmPlan = namedtuple("IgemmPlan", "kernel bm bn classes ragged ksplit ntap stages")


def class_taps(d, cls):
    """The taps that contribute to parity class cls: [(tap index, dy, dx)], input pixel = base + (dy, dx)."""
    s = d.stride
    py, px = (cls // s, cls % s) if d.transposed else (0, 0)
    out = []
    for ky in range(d.KH):
        for kx in range(d.KW):
            if d.transposed:
                ny, nx = py + d.pad - ky, px + d.pad - kx
                if ny % s or nx % s:
                    continue
                out.append((ky * d.KW + kx, ny // s, nx // s))                       # (exact divisions)
            else:
                out.append((ky * d.KW + kx, ky - d.pad, kx - d.pad))
    return out


def igemm_geometry(d):
    """-> (classes, OHc, OWc, Mc, ragged)."""
    if d.transposed and d.stride > 1:
        s = d.stride
        OHc, OWc = _cdiv(d.OH, s), _cdiv(d.OW, s)
        return s * s, OHc, OWc, d.N * OHc * OWc, bool(d.OH % s or d.OW % s)
    return 1, d.OH, d.OW, d.N * d.OH * d.OW, False


def igemm_tile(d):
    """mi_conv_igemm_tile (no checks)."""
    classes, _, _, Mc, _ = igemm_geometry(d)
    bn64 = d.Nc <= 64
    bm64 = _cdiv(Mc, 128) * _cdiv(d.Nc, 128) * classes < 384 or Mc <= 64
    if not bn64 and bm64 and _cdiv(Mc, 64) * _cdiv(d.Nc, 128) * classes < 384:
        bn64 = True
    return (64 if bm64 else 128), (64 if bn64 else 128)


def igemm_plan(d, has_wb=False, in16=False, aligned=True):
    """mi_conv_igemm_plan -> IgemmPlan, or the fragment of mi_last_error that the refusal carries."""
    if d.N <= 0 or d.K <= 0 or d.Nc <= 0 or d.KH <= 0 or d.KW <= 0 or d.stride <= 0:
        return "bad sizes"
    if d.mode not in (0, 1):
        return "mode must be 0 (fp32) or 1 (bf16)"
    if d.K1 != d.K and not (0 < d.K1 < d.K and d.K1 % 4 == 0):
        return "bad two-source split"
    if d.ldx % 4 or d.ldy < d.Nc:
        return "ldx must be a multiple of 4, ldy >= Nc"
    if in16 and d.K1 != d.K and d.K1 % 64:
        return "bf16 activations: K1 % 64 == 0"
    if d.transposed and d.stride > 1 and (d.KH < d.stride or d.KW < d.stride):
        return "transposed: kernel smaller than stride"
    classes, _, _, Mc, ragged = igemm_geometry(d)
    ksplit = 1
    if _cdiv(Mc, 64) * _cdiv(d.Nc, 64) * classes <= 16 and d.K >= 1024 and d.KH * d.KW == 1 and (d.accumulate or d.ldy == d.Nc):
        ksplit = min(d.K // 128, 32)
    bm, bn = igemm_tile(d)
    ntap = [len(class_taps(d, c)) for c in range(classes)]
    vecA = aligned and d.ldx % 4 == 0 and (d.K1 == d.K or d.ldx2 % 4 == 0)
    table_ok = classes <= 4 and d.KH * d.KW <= 16 and all(ntap)
    fast = (not ragged and d.mode == 1 and has_wb and ksplit == 1 and d.K % 32 == 0 and d.K1 % 32 == 0 and vecA and table_ok)
    if in16 and not fast:
        return "bf16 activations: the layer does not fit the ring kernel"
    ck = 64 if fast and in16 else 32
    nt = tuple((ntap + [0] * PLAN_CLASSES)[:PLAN_CLASSES])
    return IgemmPlan(int(fast), bm, bn, classes, int(ragged), ksplit, nt, tuple(n * _cdiv(d.K, ck) for n in nt))


def io_supported(d):
    """mi_conv_igemm_bf16w_io_supported."""
    if d.mode != 1 or d.K % 64 or d.K1 % 64 or d.ldx % 8 or (d.K1 != d.K and d.ldx2 % 8):
        return 0
    if d.KH * d.KW > 16 or d.KH * d.KW == 1:
        return 0
    if d.transposed and d.stride > 1 and (d.OH % d.stride or d.OW % d.stride or d.stride != 2):
        return 0
    p = igemm_plan(d, True, True, True)
    return int(not isinstance(p, str) and p.kernel == 1)


def igemm_plan_name(p, mode, in16=False):
    """'gen0<64,64>', 'gen1<128,64>/ks8', 'fast<64,128>', 'fast16<64,64>', 'gen1<64,64>/ragged'."""
    s = (("fast16" if in16 else "fast") if p.kernel else f"gen{mode}") + f"<{p.bm},{p.bn}>"
    return s + (f"/ks{p.ksplit}" if p.ksplit > 1 else "") + ("/ragged" if p.ragged else "")


def all_igemm_instantiations():
    """igemm_kernel<MODE, BM, BN> (8) and igemm_fast_kernel<BM, BN, IN16> (8)."""
    t = [(128, 128), (128, 64), (64, 128), (64, 64)]
    return {("gen", m, bm, bn) for m in (0, 1) for bm, bn in t} | {("fast", bm, bn, i) for i in (0, 1) for bm, bn in t}


# ------------------------------------------------------------------------------------------------------------ wgrad planner, restated
WgradPlan = namedtuple("WgradPlan", "fast big splits chunk xcd_map grid")


def wgrad_plan_splits(d):
    """-> (splits, chunk)."""
    B = 128 if (d.Ci >= 128 and d.Cj >= 128) else 64
    Mtot = d.N * d.DH * d.DW
    base = d.KH * d.KW * _cdiv(d.Ci, B) * _cdiv(d.Cj, B)
    splits = max(1, min(_cdiv(1024, base), _cdiv(Mtot, 64)))
    chunk = _up(_cdiv(Mtot, splits), 32)
    return _cdiv(Mtot, chunk), chunk


def _pow2(v):
    return v > 0 and v & (v - 1) == 0


def wgrad_plan(d, aligned=True, slab=False):
    """mi_conv_wgrad_plan -> WgradPlan, or the fragment of mi_last_error that the refusal carries."""
    if min(d.N, d.DH, d.DW, d.Ci, d.Cj, d.KH, d.KW) <= 0:
        return "bad sizes"
    if d.mode not in (0, 1):
        return "mode must be 0 or 1"
    if d.I1 != d.Ci and not (0 < d.I1 < d.Ci and d.I1 % 4 == 0):
        return "bad two-source split"
    big = d.Ci >= 128 and d.Cj >= 128
    B = 128 if big else 64
    splits, chunk = wgrad_plan_splits(d)
    inner = _cdiv(d.Ci, B) * _cdiv(d.Cj, B) * d.KH * d.KW
    vec = aligned and d.ldp % 4 == 0 and (d.I1 == d.Ci or d.ldp2 % 4 == 0) and d.ldq % 4 == 0
    fast = (not slab and d.mode == 1 and vec and _pow2(d.DW) and _pow2(d.DH * d.DW) and d.Ci % 4 == 0 and d.Cj % 4 == 0 and d.I1 % 4 == 0
            and d.Ci >= 4 and d.Cj >= 4)
    xcd = fast and splits >= 8
    return WgradPlan(int(fast), int(big), splits, chunk, int(xcd), inner * (_up(splits, 8) if xcd else splits))


def slabs_workspace(d):
    if min(d.N, d.DH, d.DW, d.Ci, d.Cj, d.KH, d.KW) <= 0:
        return 0
    return wgrad_plan_splits(d)[0] * d.KH * d.KW * d.Ci * d.Cj * 4


def wgrad_plan_name(p, mode):
    B = 128 if p.big else 64
    return ("fast" if p.fast else f"gen{mode}") + f"<{B},{B}>" + ("/xcd" if p.xcd_map else "")


def xcd_ids(p, inner):
    """The (split, inner index) pairs wgrad_fast_kernel's XCD map gives the launch's workgroups, surplus ones dropped."""
    out = []
    for b in range(p.grid):
        split = (b & 7) + 8 * ((b >> 3) // inner)
        if split < p.splits:
            out.append((split, (b >> 3) % inner))
    return out


# ------------------------------------------------------------------------------------------------------------ references
def _axis(O, I, k, s, p, transposed):
    """Pairs (o, i) of one axis that tap offset k joins."""
    oo, ii = [], []
    for o in range(O):
        if transposed:
            n = o + p - k
            if n % s:
                continue
            i = n // s
        else:
            i = o * s - p + k
        if 0 <= i < I:
            oo.append(o)
            ii.append(i)
    return torch.tensor(oo, dtype=torch.long), torch.tensor(ii, dtype=torch.long)


def conv_ref(d, x, W, x2=None, bias=None, res=None, prior=None, absolute=False):
    """include/mi_ddpm.h: y[n,oy,ox,j] = bias[j] + res + prior + sum_{ky,kx,k} src[n,iy,ix,k] W[tap][k][j]; transposed = 0:
    iy = oy stride - pad + ky; transposed = 1: iy = (oy + pad - ky) / stride where divisible.  W: the logical [taps][K][Nc] operand.
    absolute: the same sum over the absolute values of its terms."""
    a = (lambda t: t.to(F64).abs()) if absolute else (lambda t: t.to(F64))
    src = a(x) if x2 is None else torch.cat([a(x), a(x2)], dim=-1)
    assert src.shape == (d.N, d.IH, d.IW, d.K) and W.shape == (d.KH * d.KW, d.K, d.Nc)
    y = torch.zeros(d.N, d.OH, d.OW, d.Nc, dtype=F64)
    for ky in range(d.KH):
        oy, iy = _axis(d.OH, d.IH, ky, d.stride, d.pad, d.transposed)
        for kx in range(d.KW):
            ox, ix = _axis(d.OW, d.IW, kx, d.stride, d.pad, d.transposed)
            if oy.numel() == 0 or ox.numel() == 0:
                continue
            g = src[:, iy[:, None], ix[None, :]]                                   # [N][oy][ox][K]
            y[:, oy[:, None], ox[None, :]] += g @ a(W[ky * d.KW + kx])
    for extra in (bias, res, prior):
        if extra is not None:
            y = y + a(extra)
    return y


def wgrad_ref(d, P, Q, P2=None, absolute=False):
    """dW[tap][i][j] = sum_{n,y,x} P[n,py,px,i] Q[n,qy,qx,j]: (y, x) over the DH x DW grid of the direct operand, the gathered operand
    read at (y stride - pad + ky, x stride - pad + kx) of its GH x GW grid.  gather_i = 1: P gathered."""
    a = (lambda t: t.to(F64).abs()) if absolute else (lambda t: t.to(F64))
    Pc = a(P) if P2 is None else torch.cat([a(P), a(P2)], dim=-1)
    Qc = a(Q)
    dW = torch.zeros(d.KH * d.KW, d.Ci, d.Cj, dtype=F64)
    for ky in range(d.KH):
        dy, gy = _axis(d.DH, d.GH, ky, d.stride, d.pad, 0)
        for kx in range(d.KW):
            dx, gx = _axis(d.DW, d.GW, kx, d.stride, d.pad, 0)
            if dy.numel() == 0 or dx.numel() == 0:
                continue
            pi = (gy, gx) if d.gather_i else (dy, dx)
            qi = (dy, dx) if d.gather_i else (gy, gx)
            Pg = Pc[:, pi[0][:, None], pi[1][None, :]].reshape(-1, d.Ci)
            Qg = Qc[:, qi[0][:, None], qi[1][None, :]].reshape(-1, d.Cj)
            dW[ky * d.KW + kx] = Pg.t() @ Qg
    return dW


def colsum_ref(x, absolute=False):
    x = x.to(F64)
    return (x.abs() if absolute else x).sum(0)


def w_memory(W, w_kn):
    """The logical [tap][K][Nc] operand as the fp32 tensor in memory: [tap][K][Nc] (w_kn) or [tap][Nc][K]."""
    return W.contiguous() if w_kn else W.transpose(1, 2).contiguous()


# ------------------------------------------------------------------------------------------------------------ operand builders
def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


class In:
    """Rows of t64 [..][C] at pitch ld inside a NaN-filled buffer: NaN in front, behind and in every row's padding.  off: elements the
    view starts past 16-byte alignment."""

    def __init__(self, t64, ld=None, dtype=F32, off=0, device="cpu"):
        t64 = t64.reshape(-1, t64.shape[-1])
        R, C = t64.shape
        ld = C if ld is None else ld
        assert ld >= C
        self.buf = torch.full((2 * PAD + R * ld,), NAN, dtype=dtype, device=device)
        self.rows = self.buf[PAD + off:PAD + off + R * ld].view(R, ld)
        self.rows[:, :C].copy_(t64.to(dtype))
        self.ptr = self.rows.data_ptr()
        assert self.ptr % 16 == off * self.buf.element_size()
        self.snap = self.buf.clone()

    def intact(self):
        return same_bits(self.buf, self.snap)


class Out:
    """R rows of C results at pitch ld between PAD sentinels, sentinel padding inside every row; init64: what the rows hold before the
    launch (else NaN when nan, else sentinels)."""

    def __init__(self, R, C, ld=None, init64=None, nan=False, device="cpu"):
        ld = C if ld is None else ld
        assert ld >= C
        self.R, self.C, self.ld = R, C, ld
        self.buf = torch.full((2 * PAD + R * ld,), SENT, dtype=F32, device=device)
        self.rows = self.buf[PAD:PAD + R * ld].view(R, ld)
        if init64 is not None:
            self.rows[:, :C].copy_(init64.reshape(R, C).to(F32))
        elif nan:
            self.rows[:, :C] = NAN
        self.ptr = self.rows.data_ptr()
        assert self.ptr % 16 == 0
        self.snap = self.buf.clone()

    def get(self):
        assert bool((self.buf[:PAD] == SENT).all()) and bool((self.buf[PAD + self.R * self.ld:] == SENT).all()), "written outside the result"
        assert bool((self.rows[:, self.C:] == SENT).all()), "written into a row's padding"
        return self.rows[:, :self.C].cpu()

    def reset(self):
        self.buf.copy_(self.snap)

    def untouched(self):
        return same_bits(self.buf, self.snap)


# ------------------------------------------------------------------------------------------------------------ conv cases
class _Case:
    def __repr__(self):
        return self.name


def _nt(name, fields, defaults):
    base = namedtuple(name, fields, defaults=defaults)
    return type(name, (_Case, base), {"__slots__": ()})


# plan: igemm_plan_name() for the case's first variant (tests/test_igemm_cpu.py holds it against the library).  I, O: (H, W) of the
# gathered and of the produced tensor; k: (KH, KW); T: transposed; kn: w_kn; K1: channels of the first source (0: one source);
# epi: 'b' bias, 'r' residual, 'a' accumulate; wb: the bf16 weight copy (mode 1 only); in16: bf16-stored activations;
# xoff / woff: floats the x / w view starts past 16-byte alignment; ldx, ldx2, ldy: pitches (0: the family's default below);
# modes: the modes a case without wb runs in.
Conv = _nt("Conv", "name plan N I O K Nc k s p T kn K1 epi wb in16 xoff woff ldx ldx2 ldy modes",
           (1, 0, "", False, False, 0, 0, 0, 0, 0, (0, 1)))


def conv_variants(c):
    """[(mode, wb, in16)] a case runs as."""
    return [(1, True, c.in16)] if c.wb else [(m, False, False) for m in c.modes]


def conv_desc(c, mode):
    K1 = c.K1 or c.K
    q = 8 if c.in16 else 4
    ldx = c.ldx or _up(K1, q) + q
    ldx2 = (c.ldx2 or _up(c.K - K1, q) + 3 * q) if c.K1 else 0
    ldy = c.ldy or c.Nc + 3
    return ConvD(N=c.N, IH=c.I[0], IW=c.I[1], OH=c.O[0], OW=c.O[1], K=c.K, Nc=c.Nc, KH=c.k[0], KW=c.k[1], stride=c.s, pad=c.p, transposed=c.T,
                 w_kn=c.kn, mode=mode, K1=K1, ldx=ldx, ldx2=ldx2, ldy=ldy, ldr=(c.Nc + 5) if "r" in c.epi else 0, accumulate=int("a" in c.epi))


def conv_aligned(c):
    return c.xoff == 0


def _layer(name, kind, k, s, p, I, O, Cin, Cout, N=2, **kw):
    """A layer of the nets and its data gradient: kind 'conv' (I -> O) or 'convT'.  The gradient reads the same weights [tap][Cin][Cout]
    with w_kn = 0 and transposed flipped."""
    T = int(kind == "convT")
    gkw = dict(kw)
    if "ldx" in gkw:                       # the input's pitch is the gradient's output pitch
        gkw["ldy"] = gkw.pop("ldx")
    return [Conv(name, "", N, I, O, Cin, Cout, (k, k) if isinstance(k, int) else k, s, p, T, 1, **kw),
            Conv(name + "_dgrad", "", N, O, I, Cout, Cin, (k, k) if isinstance(k, int) else k, s, p, 1 - T, 0, **gkw)]


def _conv_cases():
    L = []
    T44 = dict(k=(4, 4), s=2, p=1, T=1)
    # ---- the generic kernel's four tiles (two modes each), K = 8 keeps them off the ring kernel
    L += [Conv("tile_128x128", "", 24, (16, 16), (32, 32), 8, 136, kn=1, **T44), Conv("tile_128x64", "", 48, (16, 16), (32, 32), 8, 40, kn=0, **T44),
          Conv("tile_64x128", "", 12, (16, 16), (32, 32), 8, 136, kn=0, **T44)]
    # ---- K edges on 3x3 / 3x5 (chunk tails, ragged quads, the scalar paths of both weight layouts)
    for K in (1, 3, 5, 8, 24, 33, 34, 36, 40, 64):
        L.append(Conv(f"k{K}", "", 2, (3, 5), (3, 5), K, 12, (3, 3), 1, 1, 0, K % 2, ldx=4 if K < 4 else 0))
    # ---- Nc edges (Nc = 1, 3 at ldy = 4)
    for Nc in (1, 3, 40, 65, 129, 136):
        L.append(Conv(f"nc{Nc}", "", 2, (7, 7), (7, 7), 8, Nc, (3, 3), 1, 1, 0, Nc % 2, ldy=4 if Nc < 4 else 0, epi="b"))
    L += [Conv("nc65_nk", "", 2, (7, 7), (7, 7), 8, 65, (1, 1), 1, 0, 0, 0), Conv("k5_nk", "", 2, (3, 5), (3, 5), 5, 12, (3, 3), 1, 1, 0, 0),
          Conv("vecA_off", "", 2, (7, 7), (7, 7), 40, 24, (3, 3), 1, 1, 0, 1, xoff=1), Conv("vecB_off_kn", "", 2, (7, 7), (7, 7), 40, 24, (3, 3), 1, 1, 0, 1, woff=1),
          Conv("vecB_off_nk", "", 2, (7, 7), (7, 7), 40, 24, (3, 3), 1, 1, 0, 0, woff=1)]
    # ---- two sources: K1 = 4 and 36 (a 32-channel chunk straddles the split), ldx2 != ldx
    L += [Conv("two_k1_4", "", 2, (7, 7), (7, 7), 40, 24, (3, 3), 1, 1, 0, 1, K1=4, epi="b"),
          Conv("two_k1_36", "", 2, (7, 7), (7, 7), 64, 24, (3, 3), 1, 1, 0, 0, K1=36, epi="r"),
          Conv("two_k1_36_vecA_off", "", 2, (3, 5), (3, 5), 64, 24, (3, 3), 1, 1, 0, 1, K1=36, xoff=1)]
    # ---- Mc = 1, 63, 65 (98 is the 7x7 cases'); Linear with both layouts
    L += [Conv("linear_kn_m1", "", 1, (1, 1), (1, 1), 40, 24, (1, 1), 1, 0, 0, 1, epi="b"), Conv("linear_nk_m63", "", 63, (1, 1), (1, 1), 24, 40, (1, 1), 1, 0, 0, 0, epi="b"),
          Conv("linear_kn_m65", "", 65, (1, 1), (1, 1), 33, 65, (1, 1), 1, 0, 0, 1, epi="ba")]
    # ---- the geometries the nets run, each with its data gradient
    L += _layer("c4s2p1_28to14", "conv", 4, 2, 1, (28, 28), (14, 14), 1, 8, ldx=4) + _layer("c4s2p1_14to7", "conv", 4, 2, 1, (14, 14), (7, 7), 8, 16)
    L += _layer("c3s2p1_7to4", "conv", 3, 2, 1, (7, 7), (4, 4), 16, 24) + _layer("c3s2p1_7x8to4x4", "conv", 3, 2, 1, (7, 8), (4, 4), 8, 16)
    L += _layer("c4s1p0_4to1", "conv", 4, 1, 0, (4, 4), (1, 1), 24, 40, N=5) + _layer("c2s1p0_2to1", "conv", 2, 1, 0, (2, 2), (1, 1), 24, 8, N=5)
    L += _layer("t4s1p0_1to4", "convT", 4, 1, 0, (1, 1), (4, 4), 40, 24, N=5) + _layer("t3s2p1_4to7", "convT", 3, 2, 1, (4, 4), (7, 7), 24, 16)
    L += _layer("t4s2p1_7to14", "convT", 4, 2, 1, (7, 7), (14, 14), 16, 8) + _layer("c3s1p1_7x7", "conv", 3, 1, 1, (7, 7), (7, 7), 16, 24)
    L += _layer("c3s1p1_3x5", "conv", 3, 1, 1, (3, 5), (3, 5), 8, 8) + _layer("c1_7x7", "conv", 1, 1, 0, (7, 7), (7, 7), 24, 16)
    L += _layer("t3s3p0_2to6", "convT", 3, 3, 0, (2, 2), (6, 6), 8, 8) + _layer("c1x3p0", "conv", (1, 3), 1, 0, (5, 7), (5, 5), 8, 8)
    # ---- bias x residual (own pitch) x accumulate
    for e in ("r", "a", "br", "ra", "bra"):
        L.append(Conv(f"epi_{e}", "", 2, (4, 4), (7, 7), 24, 20, (3, 3), 2, 1, 1, 1, epi=e))
    # ---- the bf16 weight copy on the generic kernel: K % 32, vecA off, ragged, k-slices
    L += [Conv("wb_k8", "", 2, (7, 7), (14, 14), 8, 24, epi="b", wb=True, **T44), Conv("wb_k40_two", "", 2, (7, 7), (7, 7), 40, 24, (3, 3), 1, 1, 0, 0, K1=8, wb=True),
          Conv("wb_vecA_off", "", 2, (7, 7), (14, 14), 32, 24, xoff=1, wb=True, **T44),
          Conv("wb_ragged_4to7", "", 3, (4, 4), (7, 7), 32, 40, (3, 3), 2, 1, 1, 0, epi="br", wb=True),
          Conv("wb_ragged_4x4to7x8", "", 3, (4, 4), (7, 8), 64, 24, (3, 3), 2, 1, 1, 0, wb=True)]
    # ---- k-slices: 1x1, at most 16 64-tiles, K >= 1024
    lin = dict(I=(2, 2), O=(2, 2), k=(1, 1), s=1, p=0, T=0)
    L += [Conv("ks_k1024", "", 4, K=1024, Nc=24, kn=1, ldy=24, epi="br", **lin), Conv("ks_k1056_two", "", 4, K=1056, Nc=24, kn=0, K1=516, ldy=24, epi="b", **lin),
          Conv("ks_k4224", "", 4, K=4224, Nc=40, kn=1, ldy=40, modes=(1,), **lin), Conv("ks_k1024_acc_pitched", "", 4, K=1024, Nc=24, kn=1, epi="bra", **lin),
          Conv("ks_off_pitched", "", 4, K=1024, Nc=24, kn=1, epi="b", **lin), Conv("ks_k1024_wb", "", 4, K=1024, Nc=24, ldy=24, epi="br", wb=True, **lin),
          Conv("ks_k1056_wb_acc", "", 4, K=1056, Nc=24, epi="a", wb=True, **lin)]
    # ---- the ring kernel: four tiles x (fp32 x at K = 32, bf16 x at K = 64)
    for i16, K in ((False, 32), (True, 64)):
        sfx = "_x16" if i16 else ""
        L += [Conv("ring_128x128" + sfx, "", 24, (16, 16), (32, 32), K, 136, wb=True, in16=i16, **T44),
              Conv("ring_128x64" + sfx, "", 48, (16, 16), (32, 32), K, 40, wb=True, in16=i16, epi="b", **T44),
              Conv("ring_64x128" + sfx, "", 12, (16, 16), (32, 32), K, 136, wb=True, in16=i16, epi="r", **T44)]
    # stage counts 1 / 2 / 2 / 4 times K / 32 (ConvT(3, 2, 1) with output padding, 4 -> 8), 9 and 18 (3x3 stride 1); Mc ragged; Nc = 40, 72
    T33 = dict(I=(4, 4), O=(8, 8), k=(3, 3), s=2, p=1, T=1)
    L += [Conv("ring_t3_k32", "", 3, K=32, Nc=40, wb=True, **T33), Conv("ring_t3_k64", "", 3, K=64, Nc=72, wb=True, epi="b", **T33),
          Conv("ring_t3_k96", "", 3, K=96, Nc=40, wb=True, epi="a", **T33), Conv("ring_t3_k128_two", "", 3, K=128, Nc=72, K1=64, wb=True, epi="bra", **T33),
          Conv("ring_t3_k64_x16", "", 3, K=64, Nc=40, wb=True, in16=True, **T33), Conv("ring_t3_k128_two_x16", "", 3, K=128, Nc=72, K1=64, wb=True, in16=True, epi="br", **T33),
          Conv("ring_c3_k32", "", 5, (3, 5), (3, 5), 32, 40, (3, 3), 1, 1, 0, 0, wb=True), Conv("ring_c3_k64_two", "", 5, (3, 5), (3, 5), 64, 72, (3, 3), 1, 1, 0, 0, K1=32, wb=True, epi="r"),
          Conv("ring_c3_dgrad_k32", "", 5, (3, 5), (3, 5), 32, 24, (3, 3), 1, 1, 1, 0, wb=True)]
    # non-transposed stride 2 on odd grids (the bit masks), fp32 and bf16 x
    L += [Conv("ring_c3s2_7to4", "", 3, (7, 7), (4, 4), 32, 40, (3, 3), 2, 1, 0, 0, wb=True, epi="b"), Conv("ring_c4s2_14to7", "", 3, (14, 14), (7, 7), 32, 24, (4, 4), 2, 1, 0, 0, wb=True),
          Conv("ring_c4s2_14to7_x16", "", 3, (14, 14), (7, 7), 64, 24, (4, 4), 2, 1, 0, 0, wb=True, in16=True, epi="a"),
          Conv("ring_t4_7to14", "", 3, (7, 7), (14, 14), 32, 24, wb=True, epi="r", **T44)]
    out = []
    for c in L:
        mode, wb, i16 = conv_variants(c)[0]
        p = igemm_plan(conv_desc(c, mode), wb, i16, conv_aligned(c))
        assert not isinstance(p, str), (c.name, p)
        out.append(c._replace(plan=igemm_plan_name(p, mode, i16)))
    return out


# the plan every case is there for, written out; _conv_cases() fills the field from the restated planner and the CPU test holds both
# this table and the library's answer against it
CONV_PLANS = {
    "tile_128x128": "gen0<128,128>", "tile_128x64": "gen0<128,64>", "tile_64x128": "gen0<64,128>",
    "ks_k1024": "gen0<64,64>/ks8", "ks_k1056_two": "gen0<64,64>/ks8", "ks_k4224": "gen1<64,64>/ks32", "ks_k1024_acc_pitched": "gen0<64,64>/ks8",
    "ks_off_pitched": "gen0<64,64>", "ks_k1024_wb": "gen1<64,64>/ks8", "ks_k1056_wb_acc": "gen1<64,64>/ks8",
    "wb_k8": "gen1<64,64>", "wb_k40_two": "gen1<64,64>", "wb_vecA_off": "gen1<64,64>", "wb_ragged_4to7": "gen1<64,64>/ragged",
    "wb_ragged_4x4to7x8": "gen1<64,64>/ragged", "t3s2p1_4to7": "gen0<64,64>/ragged", "c3s2p1_7x8to4x4_dgrad": "gen0<64,64>/ragged",
    "ring_128x128": "fast<128,128>", "ring_128x64": "fast<128,64>", "ring_64x128": "fast<64,128>",
    "ring_128x128_x16": "fast16<128,128>", "ring_128x64_x16": "fast16<128,64>", "ring_64x128_x16": "fast16<64,128>",
    "ring_t3_k32": "fast<64,64>", "ring_t3_k64_x16": "fast16<64,64>", "ring_c3s2_7to4": "fast<64,64>", "ring_c4s2_14to7_x16": "fast16<64,64>",
    "nc129": "gen0<64,64>", "nc136": "gen0<64,64>",
}
CONV_CASES = _conv_cases()


def conv_case(name):
    return next(c for c in CONV_CASES if c.name == name)


def conv_terms(c, mode):
    """Summed terms per output element: the most taps of a class times K, plus the epilogue's operands."""
    d = conv_desc(c, mode)
    classes = igemm_geometry(d)[0]
    return max(len(class_taps(d, k)) for k in range(classes)) * c.K + len(c.epi)


def conv_operands(c, kind):
    """float64 operands of a case: x (and x2), the logical weights W [taps][K][Nc], bias, residual, prior content.  kind 'int': x in
    {-4..4}, w in {-3..3}, bias / residual in {-3..3}, prior content non-zero in {-3..3}; 'randn': normal values (fp32)."""
    K1 = c.K1 or c.K
    key = (c.name, kind)
    taps = c.k[0] * c.k[1]
    sh_i, sh_o = (c.N,) + tuple(c.I), (c.N,) + tuple(c.O)
    return dict(x=operand(sh_i + (K1,), kind, seed(key, "x")), x2=operand(sh_i + (c.K - K1,), kind, seed(key, "x2")) if c.K1 else None,
                W=operand((taps, c.K, c.Nc), kind, seed(key, "w"), amp=3, scale=(taps * c.K) ** -0.5),
                bias=operand((c.Nc,), kind, seed(key, "b"), amp=3) if "b" in c.epi else None,
                res=operand(sh_o + (c.Nc,), kind, seed(key, "r"), amp=3) if "r" in c.epi else None,
                prior=init_content(sh_o + (c.Nc,), seed(key, "p"), kind) if "a" in c.epi else None)


def conv_reference(c, mode, ops, rounded):
    """-> (float64 reference, the same sum over |terms|).  rounded: x, x2 and W rounded once to bf16, to nearest even (what mode 1 stages)."""
    r = (lambda t: None if t is None else bf16_round(t)) if rounded else (lambda t: t)
    d = conv_desc(c, mode)
    args = (d, r(ops["x"]), r(ops["W"]), r(ops["x2"]), ops["bias"], ops["res"], ops["prior"])
    return conv_ref(*args), conv_ref(*args, absolute=True)


def conv_edges():
    """edge name -> the case names that reach it (from the restated plans: the coverage claim is computed, not written)."""
    e = {}

    def hit(k, c):
        e.setdefault(k, []).append(c.name)

    for c in CONV_CASES:
        for mode, wb, i16 in conv_variants(c):
            d = conv_desc(c, mode)
            p = igemm_plan(d, wb, i16, conv_aligned(c))
            classes, OHc, OWc, Mc, ragged = igemm_geometry(d)
            if p.kernel:
                hit("inst:" + repr(("fast", p.bm, p.bn, int(i16))), c)
                ck = 64 if i16 else 32
                for n in p.stages[:classes]:
                    hit(f"ring:stages:{n}", c)
                    hit(f"ring:stages%3:{n % 3}", c)
                if d.Nc % p.bn and c.Nc in (40, 72, 136):
                    hit(f"ring:nc{c.Nc}", c)
                if Mc % p.bm:
                    hit("ring:m_tail", c)
                if c.K1:
                    hit(f"ring:two:k1_{c.K1}" + ("_x16" if i16 else ""), c)
                if not d.transposed and d.stride == 2 and d.IH % 2 and d.IW % 2:          # 7 -> 4: the last tap column / row leaves the input
                    hit("ring:s2:odd_input", c)
                if not d.transposed and d.stride == 2 and d.OH % 2 and d.OW % 2:          # 14 -> 7
                    hit("ring:s2:odd_output", c)
                for f in c.epi:
                    hit("ring:epi:" + f, c)
                assert d.K % ck == 0
                continue
            hit("inst:" + repr(("gen", mode, p.bm, p.bn)), c)
            if wb:
                why = "ks" if p.ksplit > 1 else "ragged" if ragged else "vecA" if c.xoff else "k%32" if d.K % 32 or d.K1 % 32 else "?"
                hit("gen:wb:" + why, c)
            if p.ksplit > 1:
                kper = _cdiv(_cdiv(d.K, 32), p.ksplit) * 32                      # channels per slice
                hit(f"ks:{p.ksplit}:mode{mode}" + (":wb" if wb else ""), c)
                if (p.ksplit - 1) * kper >= d.K:
                    hit("ks:empty_slice", c)
                if d.K // 128 > 32:
                    hit("ks:cap", c)
                hit("ks:" + ("acc_pitched" if d.accumulate and d.ldy > d.Nc else "acc" if d.accumulate else "zeroed"), c)
                if c.K1:
                    hit("ks:two", c)
                for f in "br":
                    if f in c.epi:
                        hit("ks:epi:" + f, c)
            elif d.K >= 1024 and d.KH * d.KW == 1:
                hit("ks:off_pitched", c)
            hit(f"gen:K{d.K}", c)
            hit(f"gen:Nc{d.Nc}", c)
            hit(f"gen:Mc{Mc}", c)
            if d.K % 32 and d.K % 4:
                hit("gen:k_ragged_quad", c)
            if c.xoff:
                hit("gen:vecA_off", c)
            if c.woff:
                hit("gen:vecB_off:ptr:" + ("kn" if d.w_kn else "nk"), c)
            if not wb and d.w_kn and d.Nc % 4:
                hit("gen:vecB_off:kn_nc%4", c)
            if not wb and not d.w_kn and d.K % 4:
                hit("gen:vecB_off:nk_k%4", c)
            if c.K1:
                hit(f"gen:two:k1_{c.K1}", c)
            if ragged:
                hit("gen:ragged:" + ("both" if d.OH % d.stride and d.OW % d.stride else "one"), c)
            if classes > 1:
                hit(f"gen:classes:{classes}", c)
            if d.KH != d.KW:
                hit("gen:kh!=kw", c)
            hit(f"gen:w_kn{d.w_kn}:T{d.transposed}", c)
            hit("gen:epi:" + (c.epi or "none"), c)
            hit(f"geom:k{d.KH}s{d.stride}p{d.pad}T{d.transposed}:{d.IH}x{d.IW}->{d.OH}x{d.OW}", c)
    return e


CONV_REQUIRED = tuple(
    ["inst:" + repr(i) for i in sorted(all_igemm_instantiations(), key=repr)]
    + [f"gen:K{k}" for k in (1, 3, 5, 8, 24, 33, 34, 36, 40, 64)] + [f"gen:Nc{n}" for n in (1, 3, 40, 65, 129, 136)] + [f"gen:Mc{m}" for m in (1, 63, 65, 98)]
    + ["gen:k_ragged_quad", "gen:vecA_off", "gen:vecB_off:ptr:kn", "gen:vecB_off:ptr:nk", "gen:vecB_off:kn_nc%4", "gen:vecB_off:nk_k%4", "gen:two:k1_4", "gen:two:k1_36",
       "gen:ragged:both", "gen:ragged:one", "gen:classes:4", "gen:classes:9", "gen:kh!=kw", "gen:w_kn0:T0", "gen:w_kn0:T1", "gen:w_kn1:T0", "gen:w_kn1:T1",
       "gen:epi:none", "gen:epi:b", "gen:epi:r", "gen:epi:a", "gen:epi:br", "gen:epi:ra", "gen:epi:bra",
       "gen:wb:ks", "gen:wb:ragged", "gen:wb:vecA", "gen:wb:k%32",
       "ks:8:mode0", "ks:8:mode1", "ks:8:mode1:wb", "ks:32:mode1", "ks:empty_slice", "ks:cap", "ks:acc_pitched", "ks:zeroed", "ks:two", "ks:epi:b", "ks:epi:r", "ks:off_pitched"]
    + [f"ring:stages:{n}" for n in (1, 2, 3, 4, 6, 8, 9, 12, 16, 18)] + [f"ring:stages%3:{n}" for n in (0, 1, 2)]
    + ["ring:nc40", "ring:nc72", "ring:nc136", "ring:m_tail", "ring:two:k1_32", "ring:two:k1_64", "ring:two:k1_64_x16", "ring:s2:odd_input", "ring:s2:odd_output", "ring:epi:b", "ring:epi:r",
       "ring:epi:a"]
    + [f"geom:{g}" for g in (
        "k4s2p1T0:28x28->14x14", "k4s2p1T1:14x14->28x28", "k4s2p1T0:14x14->7x7", "k4s2p1T1:7x7->14x14", "k3s2p1T0:7x7->4x4", "k3s2p1T1:4x4->7x7", "k3s2p1T1:4x4->7x8",
        "k4s1p0T0:4x4->1x1", "k4s1p0T1:1x1->4x4", "k2s1p0T0:2x2->1x1", "k2s1p0T1:1x1->2x2", "k3s1p1T0:7x7->7x7", "k3s1p1T1:7x7->7x7", "k3s1p1T0:3x5->3x5", "k3s1p1T1:3x5->3x5",
        "k1s1p0T0:7x7->7x7", "k1s1p0T0:1x1->1x1", "k3s3p0T1:2x2->6x6", "k3s3p0T0:6x6->2x2", "k1s1p0T1:7x7->7x7")])


def random_conv_descs(n, seed_=5):
    """Descriptors around the planner's conditions, refused ones among them -> [(d, has_wb, in16, aligned)]."""
    g = torch.Generator().manual_seed(seed_)

    def pick(v):
        return v[int(torch.randint(0, len(v), (1,), generator=g))]
    out = []
    for _ in range(n):
        kh, kw = pick([(1, 1), (1, 1), (1, 1), (3, 3), (3, 3), (3, 3), (4, 4), (4, 4), (4, 4), (2, 2), (2, 2), (1, 3), (5, 5), (1, 2), (2, 1), (0, 3)])
        s = pick([1, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 0])
        T = pick([0, 1])
        K = pick([1, 3, 8, 24, 32, 32, 64, 64, 96, 128, 40, 1024, 1024, 1056, 4224, 64, 128, 32, 8, 0])
        K1 = pick([K, K, K, K, K, K, K, K, K, K, 4, 32, 64, 36, 6, K + 4])
        Nc = pick([1, 3, 24, 40, 64, 65, 72, 128, 136, 256, 24, 64, 136, 40, 0])
        N = pick([1, 2, 3, 12, 24, 48, 64, 200, 4, 4, 2, 2, 0])
        O = pick([(1, 1), (2, 2), (4, 4), (7, 7), (7, 8), (8, 8), (14, 14), (16, 16), (32, 32), (3, 5)])
        I = pick([O, (_cdiv(O[0], 2), _cdiv(O[1], 2)), (O[0] * 2, O[1] * 2)])
        ldx = pick([_up(max(K1, 1), 4), _up(max(K1, 1), 4), _up(max(K1, 1), 4) + 4, _up(max(K1, 1), 8) + 8, _up(max(K1, 1), 8) + 8, K1 + 2])
        ldy = pick([Nc, Nc, Nc, Nc, Nc + 3, Nc + 3, Nc + 3, Nc - 1])
        d = ConvD(N=N, IH=I[0], IW=I[1], OH=O[0], OW=O[1], K=K, Nc=Nc, KH=kh, KW=kw, stride=s, pad=pick([0, 1, 1]), transposed=T, w_kn=pick([0, 1]),
                  mode=pick([0, 0, 1, 1, 1, 1, 1, 1, 1, 2]), K1=K1, ldx=ldx, ldx2=pick([0, 8, 12, 40, 6, 72]), ldy=ldy, ldr=0, accumulate=pick([0, 0, 1]))
        out.append((d, pick([0, 1, 1]), pick([0, 0, 1]), pick([0, 1, 1, 1])))
    return out


# ------------------------------------------------------------------------------------------------------------ wgrad cases
# plan: wgrad_plan_name() in the case's first mode.  G, D: (H, W) of the gathered and of the direct grid; gi: gather_i; I1: channels
# of the first source (0: one); poff: floats the P view starts past alignment; ldp: pitch of P (0: default); modes.
Wg = _nt("Wg", "name plan N G D Ci Cj k s p gi I1 poff ldp modes", (0, 0, 0, (0, 1)))


def wg_desc(c, mode):
    I1 = c.I1 or c.Ci
    return WgD(N=c.N, GH=c.G[0], GW=c.G[1], DH=c.D[0], DW=c.D[1], Ci=c.Ci, Cj=c.Cj, KH=c.k[0], KW=c.k[1], stride=c.s, pad=c.p, gather_i=c.gi, mode=mode,
               I1=I1, ldp=c.ldp or _up(I1, 4) + 4, ldp2=(_up(c.Ci - I1, 4) + 12) if c.I1 else 0, ldq=_up(c.Cj, 4) + 8)


def wg_aligned(c):
    return c.poff == 0


def _wg_cases():
    L = []
    # ---- the generic kernel: channel edges (both tiles), two sources, the nets' geometries on both gather sides, Mtot edges, vec off
    for Ci, Cj in ((1, 3), (3, 1), (24, 40), (40, 129), (129, 24), (136, 132)):
        L.append(Wg(f"g_c{Ci}x{Cj}", "", 2, (7, 7), (7, 7), Ci, Cj, (3, 3), 1, 1, Ci % 2))
    L += [Wg("g_two_i1_4", "", 2, (7, 7), (7, 7), 40, 24, (3, 3), 1, 1, 1, I1=4), Wg("g_two_i1_36", "", 2, (7, 7), (7, 7), 40, 24, (3, 3), 1, 1, 0, I1=36),
          Wg("g_two_i1_128_big", "", 2, (3, 5), (3, 5), 136, 132, (3, 3), 1, 1, 1, I1=128)]
    for gi in (1, 0):
        s = f"_gi{gi}"
        L += [Wg("g_c4s2_28to14" + s, "", 2, (28, 28), (14, 14), 3 if gi else 8, 8 if gi else 3, (4, 4), 2, 1, gi),
              Wg("g_c4s2_14to7" + s, "", 3, (14, 14), (7, 7), 8, 16, (4, 4), 2, 1, gi), Wg("g_c3s2_7to4" + s, "", 3, (7, 7), (4, 4), 16, 24, (3, 3), 2, 1, gi),
              Wg("g_c3s1_7x7" + s, "", 5, (7, 7), (7, 7), 16, 24, (3, 3), 1, 1, gi), Wg("g_c3s1_3x5" + s, "", 3, (3, 5), (3, 5), 8, 8, (3, 3), 1, 1, gi)]
    # Mtot = 1, 31, 33, 245 (slices that cross images, a ragged last slice)
    L += [Wg("g_m1", "", 1, (1, 1), (1, 1), 24, 40, (1, 1), 1, 0, 1), Wg("g_m31", "", 31, (1, 1), (1, 1), 24, 40, (1, 1), 1, 0, 0),
          Wg("g_m33", "", 33, (1, 1), (1, 1), 24, 8, (1, 1), 1, 0, 1), Wg("g_m245", "", 5, (7, 7), (7, 7), 8, 8, (3, 3), 1, 1, 1)]
    L += [Wg("g_vec_off_ptr", "", 2, (7, 7), (7, 7), 24, 40, (3, 3), 1, 1, 1, poff=1), Wg("g_vec_off_ldp5", "", 2, (7, 7), (7, 7), 5, 40, (3, 3), 1, 1, 0, ldp=5),
          Wg("g_splits_many", "", 160, (28, 28), (14, 14), 4, 4, (1, 1), 2, 0, 1, poff=1)]          # 490 slices
    # ---- the ring kernel (mode 1, power-of-two direct grid, aligned): both tiles, clamped quads, two sources, steps per slice, XCD map
    r = dict(modes=(1,))
    L += [Wg("r_c4", "", 2, (8, 8), (8, 8), 4, 4, (3, 3), 1, 1, 1, **r), Wg("r_c36x68", "", 2, (8, 8), (8, 8), 36, 68, (3, 3), 1, 1, 0, **r),
          Wg("r_c68_two_i1_4", "", 2, (16, 16), (8, 8), 68, 36, (4, 4), 2, 1, 1, I1=4, **r), Wg("r_c136_two_i1_68_big", "", 2, (8, 8), (8, 8), 136, 128, (3, 3), 1, 1, 1, I1=68, **r),
          Wg("r_c128_big_gi0", "", 2, (16, 16), (8, 8), 128, 136, (4, 4), 2, 1, 0, **r), Wg("r_k1_m48", "", 3, (4, 4), (4, 4), 36, 24, (1, 1), 1, 0, 1, **r)]
    # steps per slice through the plan: 4x4 taps, Ci = 1024 x Cj = 64 -> 4 slices
    L.append(Wg("r_steps1", "", 2, (8, 8), (4, 4), 1024, 64, (4, 4), 2, 1, 1, **r))            # 32 pixels: the only slice is one step
    for steps, N in ((2, 4), (3, 6), (4, 8), (5, 10), (7, 14)):
        L.append(Wg(f"r_steps{steps}", "", N, (16, 16), (8, 8), 1024, 64, (4, 4), 2, 1, 1, **r))
    # XCD map: splits = 8, 11, 16; below 8 without it
    L += [Wg("r_xcd8", "", 8, (8, 8), (8, 8), 64, 64, (4, 4), 1, 1, 1, **r), Wg("r_xcd11", "", 11, (8, 8), (8, 8), 64, 64, (3, 3), 1, 1, 0, **r),
          Wg("r_xcd16", "", 16, (8, 8), (8, 8), 36, 64, (3, 3), 1, 1, 1, **r)]
    # what the ring predicate refuses, in mode 1: DW = 7, Ci % 4, a misaligned operand
    L += [Wg("rx_dw7", "", 2, (7, 7), (7, 7), 36, 24, (3, 3), 1, 1, 1, **r), Wg("rx_ci6", "", 2, (8, 8), (8, 8), 6, 24, (3, 3), 1, 1, 1, **r),
          Wg("rx_ptr", "", 2, (8, 8), (8, 8), 36, 24, (3, 3), 1, 1, 1, poff=1, **r)]
    out = []
    for c in L:
        p = wgrad_plan(wg_desc(c, c.modes[0]), wg_aligned(c))
        assert not isinstance(p, str), (c.name, p)
        out.append(c._replace(plan=wgrad_plan_name(p, c.modes[0])))
    return out


WG_PLANS = {
    "g_c136x132": "gen0<128,128>", "g_two_i1_128_big": "gen0<128,128>", "g_c24x40": "gen0<64,64>", "g_c40x129": "gen0<64,64>",
    "r_c4": "fast<64,64>", "r_c136_two_i1_68_big": "fast<128,128>", "r_c128_big_gi0": "fast<128,128>", "r_xcd8": "fast<64,64>/xcd", "r_xcd11": "fast<64,64>/xcd",
    "r_xcd16": "fast<64,64>/xcd", "r_steps4": "fast<64,64>", "rx_dw7": "gen1<64,64>", "rx_ci6": "gen1<64,64>", "rx_ptr": "gen1<64,64>",
}
WG_CASES = _wg_cases()


def wg_case(name):
    return next(c for c in WG_CASES if c.name == name)


def wg_operands(c, kind):
    I1 = c.I1 or c.Ci
    key = (c.name, kind)
    gsh, dsh = (c.N,) + tuple(c.G), (c.N,) + tuple(c.D)
    psh, qsh = (gsh, dsh) if c.gi else (dsh, gsh)
    M = c.N * c.D[0] * c.D[1]
    return dict(P=operand(psh + (I1,), kind, seed(key, "p")), P2=operand(psh + (c.Ci - I1,), kind, seed(key, "p2")) if c.I1 else None,
                Q=operand(qsh + (c.Cj,), kind, seed(key, "q"), amp=3, scale=M ** -0.5),
                prior=init_content((c.k[0] * c.k[1], c.Ci, c.Cj), seed(key, "dw"), "int"))       # non-zero integers in both families


def wg_reference(c, mode, ops, rounded):
    r = (lambda t: None if t is None else bf16_round(t)) if rounded else (lambda t: t)
    d = wg_desc(c, mode)
    return wgrad_ref(d, r(ops["P"]), r(ops["Q"]), r(ops["P2"])), wgrad_ref(d, r(ops["P"]), r(ops["Q"]), r(ops["P2"]), absolute=True)


def wg_edges():
    e = {}

    def hit(k, c):
        e.setdefault(k, []).append(c.name)

    for c in WG_CASES:
        for mode in c.modes:
            d = wg_desc(c, mode)
            for slab in (False, True):
                p = wgrad_plan(d, wg_aligned(c), slab)
                Mtot = d.N * d.DH * d.DW
                if p.fast:
                    hit("inst:" + repr(("fast", 128 if p.big else 64)), c)
                    last = Mtot - (p.splits - 1) * p.chunk
                    hit(f"ring:steps:{p.chunk // 32}", c)
                    hit(f"ring:steps%3:{(p.chunk // 32) % 3}", c)
                    hit(f"ring:splits:{p.splits if p.splits in (8, 11, 16) else '<8' if p.splits < 8 else 'other'}", c)
                    if p.xcd_map and p.grid > d.KH * d.KW * _cdiv(d.Ci, 128 if p.big else 64) * _cdiv(d.Cj, 128 if p.big else 64) * p.splits:
                        hit("ring:xcd_surplus", c)
                    if last % 32:
                        hit("ring:half_step", c)
                    for C_, nm in ((d.Ci, "ci"), (d.Cj, "cj")):
                        if C_ % (128 if p.big else 64):                        # the last tile's quads past the extent read at C - 4
                            hit(f"ring:clamped_{nm}", c)
                    if c.I1:
                        hit(f"ring:two:i1_{c.I1}", c)
                    hit(f"ring:k{d.KH}s{d.stride}gi{d.gather_i}", c)
                    continue
                hit("inst:" + repr(("gen", mode, 128 if p.big else 64)) + (":slab" if slab else ""), c)
                if slab:
                    continue
                hit(f"gen:Ci{d.Ci}", c)
                hit(f"gen:Cj{d.Cj}", c)
                hit(f"gen:Mtot{Mtot}", c)
                if c.I1:
                    hit(f"gen:two:i1_{c.I1}", c)
                hit(f"gen:gi{d.gather_i}:{d.GH}x{d.GW}->{d.DH}x{d.DW}", c)
                if c.poff:
                    hit("gen:vec_off:ptr", c)
                if d.ldp % 4:
                    hit("gen:vec_off:ldp", c)
                hit("gen:splits:" + ("1" if p.splits == 1 else ">=300" if p.splits >= 300 else "some"), c)
                if Mtot % p.chunk:
                    hit("gen:ragged_last_slice", c)
                if p.splits > 1 and p.chunk % (d.DH * d.DW):
                    hit("gen:slice_crosses_images", c)
                if mode == 1 and c.name.startswith("rx_"):
                    hit("gen:ring_refused:" + c.name[3:], c)
    return e


WG_REQUIRED = tuple(
    ["inst:" + repr(("gen", m, b)) + s for m in (0, 1) for b in (64, 128) for s in ("", ":slab")] + ["inst:" + repr(("fast", b)) for b in (64, 128)]
    + [f"gen:Ci{c}" for c in (1, 3, 24, 40, 129, 136)] + [f"gen:Cj{c}" for c in (1, 3, 24, 40, 129, 132)] + [f"gen:Mtot{m}" for m in (1, 31, 33, 245)]
    + ["gen:two:i1_4", "gen:two:i1_36", "gen:two:i1_128", "gen:vec_off:ptr", "gen:vec_off:ldp", "gen:splits:1", "gen:splits:some", "gen:splits:>=300",
       "gen:ragged_last_slice", "gen:slice_crosses_images", "gen:ring_refused:dw7", "gen:ring_refused:ci6", "gen:ring_refused:ptr"]
    + [f"gen:gi{gi}:{g}" for gi in (0, 1) for g in ("28x28->14x14", "14x14->7x7", "7x7->4x4", "7x7->7x7", "3x5->3x5")]
    + [f"ring:steps:{n}" for n in (1, 2, 3, 4, 5, 7)] + [f"ring:steps%3:{n}" for n in (0, 1, 2)]
    + ["ring:splits:8", "ring:splits:11", "ring:splits:16", "ring:splits:<8", "ring:xcd_surplus", "ring:half_step", "ring:clamped_ci", "ring:clamped_cj", "ring:two:i1_4",
       "ring:two:i1_68", "ring:k1s1gi1", "ring:k3s1gi1", "ring:k3s1gi0", "ring:k4s2gi1", "ring:k4s2gi0"])


def random_wg_descs(n, seed_=9):
    g = torch.Generator().manual_seed(seed_)

    def pick(v):
        return v[int(torch.randint(0, len(v), (1,), generator=g))]
    out = []
    for _ in range(n):
        D = pick([(1, 1), (4, 4), (7, 7), (8, 8), (8, 8), (8, 4), (16, 16), (16, 16), (3, 5), (14, 14), (32, 32), (4, 4), (2, 8), (0, 4)])
        s = pick([1, 1, 2])
        Ci = pick([1, 3, 4, 24, 36, 64, 68, 128, 136, 256, 1024, 6, 64, 128, 36, 4, 0])
        Cj = pick([1, 3, 4, 24, 40, 64, 128, 132, 256, 6])
        I1 = pick([Ci, Ci, Ci, Ci, Ci, Ci, Ci, Ci, Ci, Ci, 4, 36, 68, 128, 6, Ci + 4])
        k = pick([(1, 1), (3, 3), (4, 4), (1, 3), (3, 3), (4, 4), (1, 1), (0, 1)])
        d = WgD(N=pick([1, 2, 3, 8, 11, 16, 40, 128, 4, 8, 16, 0]), GH=D[0] * s, GW=D[1] * s, DH=D[0], DW=D[1], Ci=Ci, Cj=Cj, KH=k[0], KW=k[1], stride=s, pad=pick([0, 1]),
                gather_i=pick([0, 1]), mode=pick([0, 1, 1, 1, 0, 1, 1, 1, 2]), I1=I1, ldp=pick([_up(max(I1, 1), 4), _up(max(I1, 1), 4) + 4, _up(max(I1, 1), 4) + 4, 5, I1 + 1]), ldp2=pick([0, 8, 72, 5]),
                ldq=pick([_up(Cj, 4), _up(Cj, 4) + 8, _up(Cj, 4) + 8, Cj + 1]))
        out.append((d, pick([0, 1, 1, 1]), pick([0, 0, 1])))
    return out


# ------------------------------------------------------------------------------------------------------------ column sums
# (M, C, ld, off): mi_colsum's own kernel runs where C % 4, C > 1024, ld % 4 or x is 4 bytes off; mi_colsum_ordered always
COLSUM_CASES = [(1, 1, 1, 0), (255, 3, 3, 0), (256, 5, 7, 0), (257, 63, 64, 0), (1000, 65, 65, 0), (257, 130, 132, 0), (255, 1028, 1028, 0), (256, 64, 64, 1),
                (1000, 24, 26, 0), (33, 1028, 1032, 0)]


def colsum_own_kernel(M, C, ld, off):
    return bool(C % 4 or C < 4 or C > 1024 or ld % 4 or off)


def int_exact(max_abs_sum):
    """Integer operands: every partial sum is an integer below 2^24 in magnitude whatever the order when the sum over |terms| is."""
    return max_abs_sum < 2 ** 24
