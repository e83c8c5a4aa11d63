"""Float64 oracle, rounding model, float32 emulation and dispatch model of csrc/norm_act.hip (GroupNorm + Mish and the channel
LayerNorm).  CPU only: nothing here imports the library or touches a GPU.

Layout.  GroupNorm tensors are [N][HW][C] (channels last), gamma / beta [C], temb [N][C], statistics [N][G] pairs (mean, rstd);
LayerNorm tensors are [M][C].

Oracle (float64).  y = mish(xhat gamma + beta) + temb + res with the TRUE Mish z tanh(softplus(z)) (no threshold), xhat = (x - mean) rstd,
rstd = 1 / sqrt(var + eps), biased variance over the (HW, C / G) slice.  The gradients are the closed form of the kernel's header:
    dz = dout mish'(z),  dbeta = sum dz,  dgamma = sum dz xhat,  dtemb[n] = sum_p dout,
    s1 = sum_slice gamma dz,  s2 = sum_slice gamma dz xhat,  dx = rstd (dz gamma - (s1 + xhat s2) / cnt),  dbias = sum_(n, p) dx.
LayerNorm: y = xc inv g + b, xc = x - mean, inv = 1 / (sqrt(var) + eps) (eps is added to the standard deviation),
    dh = dy g,  S = sum dh xc,  dx = inv (dh - mean(dh)) - k2 xc,  k2 = inv^2 S / (sigma C),  dg = sum_m dy xc inv,  db = sum_m dy.
A pixel whose channels are all equal has sigma == 0; there d sigma / d x is not defined and the kernel's convention is k2 = 0 (the
subgradient that ignores the sqrt): ln_grads_ref does the same, and the autograd check leaves that pixel out.

Rounding model of bf16 storage.  Inputs are taken as stored (the caller passes the rounded values).  Outputs are rounded once, at the
store.  The one inner rounding: gn_mish_bwd_kernel keeps dz as bf16 between its two passes where it has PKC (bf16 x, MAXU > 4,
VEC >= 4 -- dz_is_rounded()); dx is then formed from bf16(dz), while every sum (dgamma, dbeta, dbias, s1, s2) saw the unrounded dz.

Float32 emulation.  gn_fwd_emulated / gn_bwd_emulated evaluate the kernels' own float32 arithmetic on the CPU -- h = fma(x, rstd, -mean rstd),
the closed forms of mish_fast_f, mish_tb_pk, mish_grad_fast_f, mish_grad_pk, mish_f, mish_grad_f, sums accumulated per thread and unit
-- with v_exp_f32 / v_rcp_f32 modelled as the exact function times (1 + 2^-21 u), u uniform in [-1, 1] (both are 1 ulp instructions).
It is used only by tests/test_norm_cpu.py to set the figures below; the GPU tests compare the kernels with the oracle and the
rounding model, never with the emulation.

Figures (measured by tests/test_norm_cpu.py::test_emulation_sets_the_bounds over every case below, asserted there):
    bf16 flip share, emulation against bf16(rounding model): y <= 0.022 %, dx <= 0.048 %   (EMU_FLIPS = 0.125 %; the GPU cap FLIP_CAP = 0.5 %)
        one exception: the uncached <4,0,IO> backward with gamma = 4 randn + 1, beta = 10 randn: 0.22 %.  mish_grad_fast_f forms
        1 - tanh^2 from a float32 tanh; for z in (8.7, 20] that tanh is a * rcp(a), i.e. 1 + the reciprocal's own error, and the gradient
        is off by 2 z times it (2^-21 here; v_rcp_f32 itself is good to about 2^-23).  The packed forms (e w / n^2) have no such term.
    every differing element: one bf16 ulp off, or within ALLOW = 2^-19 of the magnitude of its terms (largest excess seen: 1.5e-6 = 0.76 ALLOW)
    dbias against the oracle, per channel relative to sum |dx|: fp32 x <= 2.2e-7 (EMU_DBIAS_F32 = 3e-7), bf16 x <= 7.5e-6 (EMU_DBIAS_BF16 = 8e-6)
    dgamma, dbeta rel-L2: fp32 x <= 4.3e-7 (the project's 5e-5 is the bound there), bf16 x <= 5.9e-6 (EMU_DPARAM_BF16 = 6.5e-6)
The GPU tests allow 4 x EMU_DBIAS_* and 4 x EMU_DPARAM_BF16.
"""
import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16

# ---------------------------------------------------------------------------------------------------- cases
# GroupNorm, fp32 storage: (N, HW, C, G) -> (forward, backward) instantiation <VEC, MAXU>
GN_F32_CASES = [
    ((8, 64, 8, 8), ((1, 16), (1, 16))),          # C/G = 1, remap
    ((3, 130, 6, 3), ((1, 16), (1, 16))),         # C/G = 2, ragged last unit
    ((1, 2209, 4, 2), ((1, 0), (1, 0))),          # uncached both ways, ragged batch of MI_GN_UB0 rows
    ((16, 49, 48, 3), ((4, 4), (4, 4))),          # remap with G = 3
    ((2, 1000, 20, 5), ((4, 4), (4, 4))),         # ragged, prefetched residual rows
    ((2, 600, 64, 4), ((4, 16), (4, 16))),        # ragged
    ((2, 1025, 32, 2), ((4, 32), (4, 0))),
    ((1, 2100, 32, 2), ((4, 0), (4, 0))),
    ((2, 20, 256, 2), ((4, 4), (4, 4))),          # C/G = 128: two passes of the channel totals
    ((8, 136, 128, 1), ((4, 32), (4, 0))),        # G = 1, remap
]
GN_F32_PITCHED = [(3, 130, 6, 3), (1, 2209, 4, 2), (2, 1000, 20, 5), (2, 600, 64, 4), (2, 1025, 32, 2), (2, 20, 256, 2), (8, 136, 128, 1)]
GN_F32_EDGE_SHAPES = [(2, 600, 64, 4), (2, 20, 256, 2)]
GN_F32_IO_BWD = [(2, 600, 64, 4), (2, 1025, 32, 2)]          # backward io = 2, 4, 6 (fp32 x)
EDGES = ["constant_slice", "mean100", "threshold_even", "threshold_odd"]

# GroupNorm, bf16 storage: (N, HW, C, G), variant -> backward instantiation <VEC, MAXU, FULL> for io = 1, 3, 5, 7
GN_BF16_CASES = [
    ((3, 49, 64, 8), "", (4, 4, False)),          # small packed path with dead rows
    ((2, 150, 256, 8), "", (4, 16, False)),       # guarded packed cache
    ((2, 1000, 128, 8), "", (4, 16, False)),
    ((2, 64, 1024, 8), "", (4, 8, True)),         # pipelined
    ((8, 256, 256, 8), "", (4, 8, True)),
    ((1, 2048, 8, 2), "", (4, 8, True)),
    ((2, 143, 256, 2), "", (8, 16, False)),       # wide, ragged
    ((1, 2500, 16, 2), "", (8, 16, False)),
    ((2, 143, 256, 2), "lddo4", (4, 0, False)),   # lddo % 8 == 4: gn_wide16 refuses the pitch
    ((2, 143, 256, 2), "dx8", (4, 0, False)),     # dx 8 bytes off a 16-byte boundary: gn_wide16 refuses the pointer (bf16 dx only)
    ((2, 289, 512, 4), "", (4, 0, False)),
]
GN_BF16_FWD = {(2, 143, 256, 2): (4, 32), (2, 289, 512, 4): (4, 0)}
BWD_IO16 = (1, 3, 5, 7)

LN_CASES = [(5, 4), (9, 128), (7, 132), (5, 516), (6, 1024), (4101, 64), (2051, 260)]
LN_FWD_ONLY = [(16389, 132)]

SUMS_CASES = [(2, 16, 128, 8), (2, 32, 128, 8), (2, 48, 128, 8), (2, 64, 128, 8), (2, 128, 128, 8), (2, 8, 1024, 64)]   # (N, HW, C, G)
SUMS_UNR = {16: (1, 1), 32: (2, 2), 48: (1, 1), 64: (4, 4), 128: (8, 4), 8: (4, 4)}      # HW -> UNR (plain, with a residual)

FLIP_CAP = 0.005          # the condition the GPU tests hold a stored bf16 tensor to (share of elements one bf16 ulp off)
EMU_FLIPS = 0.00125       # what the CPU test asserts of the emulation (measured: see the header)
ALLOW = 2.0 ** -19        # float32 evaluation error of a term, relative to the term: 4 x the 2^-21 of v_exp_f32 / v_rcp_f32 (flips())
EMU_DBIAS_F32 = 3e-7
EMU_DBIAS_BF16 = 8e-6
EMU_DPARAM_BF16 = 6.5e-6
GN_EPS = 1e-5
LN_EPS = 1e-5
UB0 = 4                   # MI_GN_UB0


# ---------------------------------------------------------------------------------------------------- numbers
def rb(x):
    """x rounded to bf16 (round to nearest even), in x's dtype."""
    return x.float().bfloat16().to(x.dtype)


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-300))


def rel_max(a, b):
    """max |a - b| / max |b|: the statistics' measure."""
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).abs().max() / b.abs().max())


def _ordered(x):
    """bf16(x) as integers ordered like the values (what is below the smallest normal float32 counts as +0)."""
    x = x.detach().cpu().float()
    x = torch.where(x.abs() < 2.0 ** -126, torch.zeros_like(x), x)
    v = x.bfloat16().view(torch.int16).int() & 0xFFFF
    return torch.where((v & 0x8000) != 0, -(v & 0x7FFF), v)


def _ulp16(r):
    return torch.exp2(torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -126))) - 7)


def flips(got_bf16, model, scale=None, alts=()):
    """A stored bf16 tensor against bf16(model): (share of elements whose bits differ, excess).  excess is the largest distance of an
    element beyond ONE bf16 ulp of bf16(model), in units of `scale` (0 where every differing element is exactly one ulp off).  scale: the
    magnitude of the terms the element is the sum of -- where they cancel, the float32 evaluation error of the terms (ALLOW x scale) is
    more than an ulp of the result, and no rounding model can say which bf16 value is stored.  alts: further models an element may be
    measured against (the bf16 neighbours of an inner rounding, see gn_mish_grads_ref); the share is against `model` alone."""
    got = got_bf16.detach().cpu().double()
    share = float((_ordered(got) != _ordered(model)).double().mean())
    best = None
    for m in (model,) + tuple(alts):
        r = rb(m.double())
        ex = ((got - r).abs() - _ulp16(r)).clamp_min(0.0)
        best = ex if best is None else torch.minimum(best, ex)
    if scale is None:
        scale = torch.ones_like(best)
    return share, float((best / scale.double().clamp_min(2.0 ** -126)).max())


def bf16_neighbours(v):
    """The bf16 values one ulp below and above the bf16 values v (float64)."""
    u = _ulp16(v)
    return v - u, v + u


def mish(z):
    return z * torch.tanh(torch.logaddexp(z, torch.zeros_like(z)))


def mish_grad(z):
    th = torch.tanh(torch.logaddexp(z, torch.zeros_like(z)))
    return th + z * (1 - th * th) * torch.sigmoid(z)


# ---------------------------------------------------------------------------------------------------- GroupNorm oracle
def _grp(t, G):
    N, HW, C = t.shape
    return t.reshape(N, HW, G, C // G)


def gn_stats_ref(x, G, eps):
    xg = _grp(x.double(), G)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    return mean, 1.0 / torch.sqrt(var + eps)


def _gn_z(x, gamma, beta, G, eps, stats):
    N, HW, C = x.shape
    mean, rstd = stats if stats is not None else gn_stats_ref(x, G, eps)
    mean, rstd = mean.double()[:, None, :, None], rstd.double()[:, None, :, None]
    h = (_grp(x.double(), G) - mean) * rstd
    ga, be = gamma.double().reshape(1, 1, G, C // G), beta.double().reshape(1, 1, G, C // G)
    return h, h * ga + be, ga, rstd


def gn_y_scale(x, gamma, beta, G, eps, temb=None, res=None, stats=None):
    """|mish(z)| + |temb| + |res|: the magnitude of y's terms (for flips())."""
    N, HW, C = x.shape
    s = mish(_gn_z(x, gamma, beta, G, eps, stats)[1]).abs().reshape(N, HW, C)
    if temb is not None:
        s = s + temb.double().abs()[:, None, :]
    return s + res.double().abs() if res is not None else s


def gn_mish_ref(x, gamma, beta, G, eps, temb=None, res=None, stats=None):
    """-> y [N][HW][C], mean [N][G], rstd [N][G] (float64).  stats: evaluate with these (mean, rstd) instead of the slice's own."""
    N, HW, C = x.shape
    mean, rstd = stats if stats is not None else gn_stats_ref(x, G, eps)
    _, z, _, _ = _gn_z(x, gamma, beta, G, eps, (mean, rstd))
    y = mish(z).reshape(N, HW, C)
    if temb is not None:
        y = y + temb.double()[:, None, :]
    if res is not None:
        y = y + res.double()
    return y, mean.double(), rstd.double()


def gn_mish_grads_ref(x, gamma, beta, G, eps, dout, stats=None, round_dz=False):
    """-> dict of dx, dgamma, dbeta, dtemb, dbias, scale (the magnitude of dx's terms, for flips()), dx_plain, alts (float64).  round_dz: dx
    is formed from bf16(dz) (the rounding model of the packed cache; dx_plain is without), and alts holds two more models: dx formed from
    the bf16 neighbours of bf16(dz) below and above (see flips(): where float32 arithmetic puts dz
    on the other side of a rounding boundary, the stored dz is one bf16 ulp off, which is more than one ulp of dx where dx's two terms cancel)."""
    N, HW, C = x.shape
    h, z, ga, rstd = _gn_z(x, gamma, beta, G, eps, stats)
    dog = _grp(dout.double(), G)
    dz = dog * mish_grad(z)
    dbeta, dgamma = dz.sum((0, 1)).reshape(C), (dz * h).sum((0, 1)).reshape(C)
    dtemb = dout.double().sum(1)
    s1, s2 = (dz * ga).sum((1, 3), keepdim=True), (dz * ga * h).sum((1, 3), keepdim=True)
    cnt = float(HW * (C // G))
    dx_plain = rstd * (dz * ga - (s1 + h * s2) / cnt)
    dx = rstd * (rb(dz) * ga - (s1 + h * s2) / cnt) if round_dz else dx_plain
    # |mish'| <= 1.1; mish_grad_fast_f forms 1 - tanh^2 from a float32 tanh next to 1: an error of 2 z_c (z_c = z clamped to [0, 20]) times tanh's
    scale = rstd * ((1.1 + 2.0 * z.clamp(0.0, 20.0)) * dog.abs() * ga.abs() + (s1.abs() + (h * s2).abs()) / cnt)
    alts = tuple((rstd * (v * ga - (s1 + h * s2) / cnt)).reshape(N, HW, C) for v in bf16_neighbours(rb(dz))) if round_dz else ()
    return dict(dx=dx.reshape(N, HW, C), dgamma=dgamma, dbeta=dbeta, dtemb=dtemb, dbias=dx_plain.sum((0, 1)).reshape(C),
                scale=scale.reshape(N, HW, C), dx_plain=dx_plain.reshape(N, HW, C), alts=alts)


def coef_ref(x, gamma, beta, G, eps, temb=None, stats=None):
    """-> scale = rstd gamma, shift = beta - mean scale, tbias = temb (0 without one), each [N][C]."""
    N, HW, C = x.shape
    mean, rstd = stats if stats is not None else gn_stats_ref(x, G, eps)
    cg = C // G
    scale = rstd.double().repeat_interleave(cg, 1) * gamma.double()[None]
    shift = beta.double()[None] - mean.double().repeat_interleave(cg, 1) * scale
    return scale, shift, temb.double() if temb is not None else torch.zeros(N, C, dtype=F64)


def sums_ref(x):
    """(sum, sum of squares) per sample and 16-channel slab of the stored values: [N][C / 16][2], float64 (exact for bf16 x)."""
    N, HW, C = x.shape
    xs = x.double().reshape(N, HW, C // 16, 16)
    return torch.stack([xs.sum((1, 3)), (xs * xs).sum((1, 3))], -1)


def stats_from_sums_ref(x, G):
    """The statistics as the sum-fed kernels form them: var = E[x^2] - mean^2 clamped at 0 (in double)."""
    N, HW, C = x.shape
    s = sums_ref(x).reshape(N, G, C // 16 // G, 2).sum(2)
    cnt = HW * (C // G)
    mean = s[..., 0] / cnt
    return mean, (s[..., 1] / cnt - mean * mean).clamp_min(0.0)


def dz_is_rounded(io, vec, maxu):
    """Where gn_mish_bwd_kernel has PKC."""
    return bool(io & 1) and maxu > 4 and vec >= 4


# ---------------------------------------------------------------------------------------------------- LayerNorm oracle
def ln_ref(x, g, b, eps):
    x = x.double()
    xc = x - x.mean(1, keepdim=True)
    inv = 1.0 / (torch.sqrt((xc * xc).mean(1, keepdim=True)) + eps)
    return xc * inv * g.double()[None] + b.double()[None]


def ln_grads_ref(x, g, eps, dy):
    """-> dx, dg, db (float64); k2 = 0 for a pixel with sigma == 0 (the kernel's convention, see the header)."""
    x, dy = x.double(), dy.double()
    C = x.shape[1]
    xc = x - x.mean(1, keepdim=True)
    sigma = torch.sqrt((xc * xc).mean(1, keepdim=True))
    inv = 1.0 / (sigma + eps)
    dh = dy * g.double()[None]
    S = (dh * xc).sum(1, keepdim=True)
    k2 = torch.where(sigma > 0, inv * inv * S / (sigma.clamp_min(1e-300) * C), torch.zeros_like(S))
    dx = inv * (dh - dh.mean(1, keepdim=True)) - k2 * xc
    return dx, (dy * xc * inv).sum(0), dy.sum(0)


# ---------------------------------------------------------------------------------------------------- dispatch model
def _cdiv(a, b):
    return (a + b - 1) // b


def gn_prepare(HW, C, G):
    """gn_prepare(): -> (vec, units, vec8_units, PP) or None where the entry point refuses the shape."""
    if C % G:
        return None
    cg = C // G
    if cg & (cg - 1) or cg > 128:
        return None
    vec = 4 if cg % 4 == 0 else 1
    if vec == 1 and cg > 2:
        return None
    PP = 256 // (cg // vec)
    v8 = _cdiv(HW, 256 // (cg // 8)) if cg % 8 == 0 else 0
    return vec, _cdiv(HW, PP), v8, PP


def _all16(pitches, alignments, need_ld=8):
    return all(p % need_ld == 0 for p in pitches) and all(a % 16 == 0 for a in alignments)


def launch_plan(N, HW, C, G, io=0, pitches=(), alignments=(), direction="bwd", knobs=None):
    """The instantiation a GroupNorm launch lands on: dict(kernel=(VEC, MAXU, IO, FULL), units, PP, ragged_unit, dead_rows, remap,
    ragged_ub, rounds_dz).  pitches: the pixel strides the dispatch looks at (backward: ldx, lddo, lddx); alignments: the byte addresses
    modulo 16 of the pointers it looks at (backward: x, dout, dx, gamma, beta).  knobs: MI_GN_VEC8 / MI_GN_FULL / MI_GN_WIDE16 / MI_GN_XCD as
    an experiment build reads them; the product library has the defaults compiled in (mi_knob is a constant there)."""
    k = dict(MI_GN_VEC8=0, MI_GN_FULL=1, MI_GN_WIDE16=1, MI_GN_XCD=1)
    k.update(knobs or {})
    prep = gn_prepare(HW, C, G)
    assert prep is not None, "refused by gn_prepare"
    vec, units, v8, PP = prep
    fwd = direction == "fwd"
    assert (vec >= 4 or io == 0) and (vec == 1 or all(p % 4 == 0 for p in pitches))
    full = False
    if k["MI_GN_VEC8"] and (io & 1) and 4 < v8 <= 8 and _all16([p for p in pitches if p], alignments):      # gn_vec8
        vec = 8
    if not fwd and (io & 1) and vec == 4 and k["MI_GN_FULL"] and HW == 8 * PP:                               # GN_DISPATCH_BWD16
        kern, full = (4, 8), True
    elif not fwd and (io & 1) and vec == 4 and k["MI_GN_WIDE16"] and units > 16 and 8 < v8 <= 16 and _all16(pitches, alignments):
        vec, kern = 8, (8, 16)
    elif vec == 8:
        kern = (8, 4) if v8 <= 4 else (8, 8)
    elif vec == 4:
        kern = (4, 4) if units <= 4 else (4, 16) if units <= 16 else (4, 32) if (units <= 32 and fwd) else (4, 0)
    else:
        kern = (1, 16) if units <= 16 else (1, 0)
    if kern[0] == 8:
        PP = 256 // (C // G // 8)
        units = _cdiv(HW, PP)
    maxu = kern[1]
    return dict(kernel=(kern[0], maxu, io, full), units=units, PP=PP, ragged_unit=HW % PP != 0,
                dead_rows=maxu > 0 and units * PP > HW, remap=N % 8 == 0 and bool(k["MI_GN_XCD"]),
                ragged_ub=maxu == 0 and not fwd and HW % (UB0 * PP) != 0, rounds_dz=(not fwd) and dz_is_rounded(io, kern[0], maxu))


def ln_plan(M, C, direction="fwd", cap_env=0):
    """ln_fwd_go / ln_bwd_blocks: dict(LPX, MAXV, blocks, iterations of the busiest wave, capped)."""
    assert C % 4 == 0 and 0 < C <= 1024
    half = C <= 128
    per = 8 if half else 4
    want = _cdiv(M, per)
    cap = 4096 if direction == "fwd" else (cap_env or 512)
    blocks = min(want, cap)
    return dict(LPX=32 if half else 64, MAXV=1 if half else 4, blocks=blocks, iterations=_cdiv(want, blocks), capped=want > cap, nq=C // 4)


def apply_sums_plan(HW, C, G, residual=False, pitches=(), alignments=()):
    """mi_gn_mish_apply_sums: the unroll it picks, or None where it returns 1."""
    if C <= 0 or G <= 0 or G > 64 or C % G or (C // G) % 16 or C % 8 or C // 8 > 256 or (C // 8) & (C // 8 - 1):
        return None
    if any(p % 8 for p in pitches) or any(a % 16 for a in alignments):
        return None
    PP = 256 // (C // 8)
    unr = 4 if residual else 8
    while unr > 1 and HW % (PP * unr):
        unr >>= 1
    return None if HW % (PP * unr) else dict(UNR=unr, chunks=HW // (PP * unr), PP=PP)


# ---------------------------------------------------------------------------------------------------- inputs
def gn_inputs(case, seed=0, bf16_x=False, bf16_dout=False, edge=None, wide_params=False):
    """Deterministic inputs of one case (float64 tensors holding exactly the values that are stored)."""
    N, HW, C, G = case
    g = torch.Generator().manual_seed(1000 + seed + 7 * N + HW + 13 * C + G)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)      # noqa: E731
    x = r(N, HW, C) * 1.5 + 0.3
    gamma, beta = r(C) + 1.0, r(C)
    if wide_params:
        gamma, beta = 4.0 * r(C) + 1.0, 10.0 * r(C)
    temb, res, dout = r(N, C), r(N, HW, C), r(N, HW, C)
    cg = C // G
    if edge == "constant_slice":
        x[N - 1, :, C - cg:] = 0.75                                # the last (sample, group) slice
    elif edge == "mean100":
        x = r(N, HW, C) * 0.1 + 100.0
    elif edge in ("threshold_even", "threshold_odd"):
        hi = torch.arange(C) % 2 == (0 if edge == "threshold_even" else 1)
        gamma = torch.full((C,), 0.5, dtype=F64)
        beta = torch.where(hi, torch.full((C,), 30.0, dtype=F64), torch.full((C,), -40.0, dtype=F64))
    st = lambda t, b16: rb(t) if b16 else t.float().double()    # noqa: E731
    return dict(x=st(x, bf16_x), gamma=st(gamma, False), beta=st(beta, False), temb=st(temb, False), res=st(res, False),
                dout=st(dout, bf16_dout))


def ln_inputs(case, seed=0, bf16_dy=False):
    M, C = case
    g = torch.Generator().manual_seed(2000 + seed + M + 3 * C)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)      # noqa: E731
    x = r(M, C) * 1.7 - 0.3
    x[0] = 0.5                                                   # an all-equal pixel in the first wave ...
    x[M - 1] = -3.0                                              # ... and in the last (sums of these are exact in float32: sigma == 0 exactly)
    gg, bb, dy, prev = r(C) + 1.0, r(C), r(M, C), r(M, C)
    st = lambda t: t.float().double()                           # noqa: E731
    return dict(x=st(x), g=st(gg), b=st(bb), dy=rb(dy) if bf16_dy else st(dy), prev=st(prev))


# ---------------------------------------------------------------------------------------------------- float32 emulation
_U = 2.0 ** -21


def _pert(t64, gen):
    return (t64 * (1.0 + _U * (2.0 * torch.rand(t64.shape, generator=gen, dtype=F64) - 1.0))).float()


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


class _Emu:
    """v_exp_f32 / v_rcp_f32 with a 2^-21 relative perturbation; everything else is float32 torch arithmetic."""

    def __init__(self, seed=0):
        self.g = torch.Generator().manual_seed(seed)

    def exp(self, x):
        return _pert(torch.exp(x.double()), self.g)

    def rcp(self, x):
        return _pert(1.0 / x.double(), self.g)

    def mish_fast(self, z):                         # mish_fast_f
        e = self.exp(z.clamp_max(20.0))
        w = e * (e + 2.0)
        return z * w * self.rcp(w + 2.0)

    def mish_tb_pk(self, z, tb):                    # mish_tb_pk
        e = self.exp(z.clamp_max(20.0))
        w = e * (e + 2.0)
        return _fma(z * w, self.rcp(w + 2.0), tb)

    def mish_grad_fast(self, z):                    # mish_grad_fast_f
        e = self.exp(z.clamp_max(20.0))
        w = e * (e + 2.0)
        r = self.rcp((w + 2.0) * (1.0 + e))
        th, sg = w * (1.0 + e) * r, e * (w + 2.0) * r
        return th + z * (1.0 - th * th) * sg

    def mish_grad_pk(self, z):                      # mish_grad_pk: e w / n^2
        zc = z.clamp_max(20.0)
        e = self.exp(zc)
        ep = e + 2.0
        n = _fma(e, ep, torch.full_like(e, 2.0))
        r = self.rcp(n)
        t1 = _fma(zc, torch.full_like(zc, 4.0), torch.full_like(zc, 6.0))
        p1 = _fma(ep + 2.0, e, t1)
        om = _fma(p1, e, t1 - 2.0)
        return (e * r) * om * r

    def mish(self, z):                              # mish_f (fp32 x): true division, tanhf above the threshold
        e = self.exp(z.clamp_max(20.0))
        w = e * (e + 2.0)
        return torch.where(z > 20.0, z * torch.tanh(z.double()).float(), z * (w / (w + 2.0)))

    def mish_grad(self, z):                         # mish_grad_f
        e = self.exp(z.clamp_max(20.0))
        w = e * (e + 2.0)
        th, sg = w / (w + 2.0), e / (1.0 + e)
        tz = torch.tanh(z.double()).float()
        return torch.where(z > 20.0, tz + z * (1.0 - tz * tz), th + z * (1.0 - th * th) * sg)


def _units_sum(t, PP):
    """Sum over the pixel axis (dim 1) the way a thread does: unit after unit in float32, then across the PP rows."""
    N, HW = t.shape[:2]
    units = _cdiv(HW, PP)
    pad = torch.zeros((N, units * PP - HW) + tuple(t.shape[2:]), dtype=t.dtype)
    u = torch.cat([t, pad], 1).reshape((N, units, PP) + tuple(t.shape[2:]))
    acc = torch.zeros_like(u[:, 0])
    for k in range(units):
        acc = acc + u[:, k]
    return acc.sum(1)


def gn_fwd_emulated(inp, case, stats32, x_bf16, use_temb=True, use_res=True, apply_sums=False, seed=0):
    """y in float32 before the store, with the given float32 statistics (mean, rstd [N][G])."""
    N, HW, C, G = case
    em = _Emu(seed)
    cg = C // G
    mean, rstd = (t.float().repeat_interleave(cg, 1)[:, None, :] for t in stats32)
    ga = inp["gamma"].float()[None, None] * rstd
    be = inp["beta"].float()[None, None] - mean * ga
    z = _fma(inp["x"].float(), ga, be)
    tb = inp["temb"].float()[:, None, :] if use_temb else torch.zeros(1, 1, C)
    if apply_sums:
        y = em.mish_tb_pk(z, tb.expand_as(z))
    else:
        y = (em.mish_fast(z) if x_bf16 else em.mish(z)) + tb
    return y + inp["res"].float() if use_res else y


def gn_bwd_emulated(inp, case, stats32, io, plan, init=None, seed=0):
    """dx (float32 before the store), dgamma, dbeta, dtemb, dbias as the backward kernel of `plan` evaluates them in float32."""
    N, HW, C, G = case
    vec, maxu, _, _ = plan["kernel"]
    PP = plan["PP"]
    em = _Emu(seed)
    cg = C // G
    mean, rstd = (t.float().repeat_interleave(cg, 1)[:, None, :] for t in stats32)
    x, d = inp["x"].float(), inp["dout"].float()
    ga, be = inp["gamma"].float()[None, None], inp["beta"].float()[None, None]
    packed = bool(io & 1) and vec >= 2 and maxu > 0            # pair1q: the small packed path, the packed cache, the pipelined form
    if packed:
        h = _fma(x, rstd, -mean * rstd)
        dz = d * em.mish_grad_pk(_fma(h, ga, be))
    else:
        h = (x - mean) * rstd
        z = _fma(h, ga, be)
        dz = d * (em.mish_grad_fast(z) if io & 1 else em.mish_grad(z))
    cA, cD, cT, cB = (_units_sum(t, PP) for t in (dz, _fma(dz, h, torch.zeros_like(h)), d, h))       # [N][C]: chs[0..3]
    gm = inp["gamma"].float()[None]
    s1 = (gm * cA).reshape(N, G, cg).sum(2).repeat_interleave(cg, 1)
    s2 = (gm * cD).reshape(N, G, cg).sum(2).repeat_interleave(cg, 1)
    cnt = float(HW * cg)
    r1 = rstd[:, 0]
    dbias_n = r1 * (gm * cA - (float(HW) * s1 + s2 * cB) / cnt)
    zero = torch.zeros(C)
    i_g, i_b, i_bias = (init[k].float() if init else zero for k in ("dgamma", "dbeta", "dbias"))
    acc = lambda i, t: i + t.sum(0) if N > 1 else i + t[0]     # noqa: E731
    dzs = rb(dz) if dz_is_rounded(io, vec, maxu) else dz
    icnt = torch.tensor(1.0 / cnt).float()
    if dz_is_rounded(io, vec, maxu):
        u2 = _fma(h, s2[:, None, :], s1[:, None, :])
        dx = _fma(u2, (-rstd * icnt).expand_as(u2), dzs * (rstd * ga))
    else:
        dx = rstd * (dzs * ga - (s1[:, None, :] + h * s2[:, None, :]) * icnt)
    return dict(dx=dx, dgamma=acc(i_g, cD), dbeta=acc(i_b, cA), dtemb=cT, dbias=acc(i_bias, dbias_n))


def dbias_err(got, ref, dx_ref):
    """max over channels of |dbias - ref| / sum_(n, p) |dx|."""
    den = dx_ref.double().abs().sum((0, 1))
    return float(((got.detach().double().cpu() - ref).abs() / den).max())
