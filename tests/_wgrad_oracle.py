"""CPU oracle of the LDS-DMA weight-gradient family (csrc/wgrad_tr.hip, wgrad1x1_tr.hip, wgrad_s2_tr.hip, csrc/tr_common.h).

Three things live here, shared by tests/test_wgrad_tr_cpu.py and tests/test_wgrad_tr_kernels_gpu.py:
  * float64 reference weight gradients, written as explicit shifted contractions over NHWC tensors in the library's
    dW[KH][KW][Ci][Cj] layout (two sources are the channel concatenation of P and P2);
  * a restatement of the host planners (tr_common.h's balance_shares, kslices and batch_layout, the per-kind work measures and xcd_map
    rules of tr_plan / w1_plan / s2_plan, the workgroup -> (slice, tile) maps, which reduce instantiation is launched) and of the
    *_supported predicates;
  * the case lists, and edges(): which planner / geometry edges those lists reach, by name.
A descriptor is a plain dict with the fields of MiWgradDesc (FIELDS)."""
import torch

F64 = torch.float64
MAXP = 8
FIELDS = ("N", "GH", "GW", "DH", "DW", "Ci", "Cj", "KH", "KW", "stride", "pad", "gather_i", "mode", "I1", "ldp", "ldp2", "ldq")
PITCH_P, PITCH_P2, PITCH_Q = 8, 16, 24       # elements added to the channel count: all different, multiples of 16 bytes in both dtypes


# ------------------------------------------------------------------------------------------------------------ references
def bf16_round(t):
    """Round to nearest even onto bf16, returned as float64 (t holds float32-representable values)."""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def wgrad3x3_ref(x, dy, x2=None):
    """3x3 / stride 1 / pad 1.  x [N][H][W][I1] (x2 [N][H][W][Ci - I1] behind it), dy [N][H][W][Cj] -> dW [3][3][Ci][Cj]."""
    if x2 is not None:
        x = torch.cat([x, x2], -1)
    N, H, W, _ = x.shape
    xp = torch.zeros(N, H + 2, W + 2, x.shape[-1], dtype=F64)
    xp[:, 1:H + 1, 1:W + 1] = x
    dW = torch.zeros(3, 3, x.shape[-1], dy.shape[-1], dtype=F64)
    for ky in range(3):
        for kx in range(3):
            dW[ky, kx] = torch.einsum("nhwi,nhwj->ij", xp[:, ky:ky + H, kx:kx + W], dy.to(F64))
    return dW


def wgrad1x1_ref(x, dy, x2=None, dy_dw=None):
    """1x1.  x [M][I1] (x2 behind it), dy [M][Cj] -> (dW [Ci][Cj], dbias [Cj]).  dy_dw: the dY the matrix product sees when it differs from
    the one the bias sum sees (fp32 dY in bf16 mode: rounded for dW, unrounded for dbias)."""
    if x2 is not None:
        x = torch.cat([x, x2], -1)
    x = x.reshape(-1, x.shape[-1]).to(F64)
    dy = dy.reshape(-1, dy.shape[-1]).to(F64)
    q = dy if dy_dw is None else dy_dw.reshape(dy.shape).to(F64)
    return x.t() @ q, dy.sum(0)


def wgrad_s2_ref(p, q, ks, gather_i):
    """Stride 2 / pad 1, ks = 3 or 4.  The small tensor [N][h][w][.] meets the big one [N][2h][2w][.] at (2y + ky - 1, 2x + kx - 1), zero
    outside.  gather_i: p (the ci side) is the big one -- the weight gradient of Conv2d(ks, 2, 1); else q is -- ConvTranspose2d(ks, 2, 1).
    -> dW [ks][ks][Ci][Cj]."""
    big, small = (p, q) if gather_i else (q, p)
    N, h, w, _ = small.shape
    assert big.shape[:3] == (N, 2 * h, 2 * w)
    bp = torch.zeros(N, 2 * h + 2, 2 * w + 2, big.shape[-1], dtype=F64)
    bp[:, 1:2 * h + 1, 1:2 * w + 1] = big
    dW = torch.zeros(ks, ks, p.shape[-1], q.shape[-1], dtype=F64)
    for ky in range(ks):
        for kx in range(ks):
            g = bp[:, ky:ky + 2 * h:2, kx:kx + 2 * w:2]
            dW[ky, kx] = torch.einsum("nhwi,nhwj->ij", g, small.to(F64)) if gather_i else torch.einsum("nhwi,nhwj->ij", small.to(F64), g)
    return dW


def rel(got, ref):
    got, ref = got.detach().to(F64).cpu(), ref.detach().to(F64).cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------ descriptors
def d3(N, H, W, Ci, Cj, I1=None, mode=1):
    I1 = Ci if I1 is None else I1
    return dict(N=N, GH=H, GW=W, DH=H, DW=W, Ci=Ci, Cj=Cj, KH=3, KW=3, stride=1, pad=1, gather_i=1, mode=mode, I1=I1,
                ldp=I1 + PITCH_P, ldp2=(Ci - I1 + PITCH_P2) if I1 != Ci else 0, ldq=Cj + PITCH_Q)


def d1(k, Ci, Cj, I1=None, mode=1):
    """1x1 over 64 k pixels ([k][8][8])."""
    d = d3(k, 8, 8, Ci, Cj, I1, mode)
    d.update(KH=1, KW=1, pad=0)
    return d


def ds2(N, h, w, Ci, Cj, ks, gather_i, mode=1):
    return dict(N=N, GH=2 * h, GW=2 * w, DH=h, DW=w, Ci=Ci, Cj=Cj, KH=ks, KW=ks, stride=2, pad=1, gather_i=gather_i, mode=mode, I1=Ci,
                ldp=Ci + PITCH_P, ldp2=0, ldq=Cj + PITCH_Q)


# ------------------------------------------------------------------------------------------------------------ *_supported
def tr_ok(d):
    if d["KH"] != 3 or d["KW"] != 3 or d["pad"] != 1 or d["stride"] != 1 or not d["gather_i"] or d["mode"] not in (0, 1):
        return False
    if d["GH"] != d["DH"] or d["GW"] != d["DW"]:
        return False
    W, H = d["DW"], d["DH"]
    if W not in (8, 16, 32, 64) or H % (64 // W) or (d["N"] * H * W) % 64:
        return False
    if d["Ci"] % 64 or d["I1"] % 64 or d["Cj"] % 32 or d["Cj"] < 32:
        return False
    a = 8 if d["mode"] == 1 else 4
    return not (d["ldp"] % a or d["ldq"] % a or (d["I1"] != d["Ci"] and d["ldp2"] % a))


def w1_ok(d, q32):
    if d["KH"] != 1 or d["KW"] != 1 or d["pad"] != 0 or d["stride"] != 1 or not d["gather_i"] or d["mode"] not in (0, 1):
        return False
    if d["GH"] != d["DH"] or d["GW"] != d["DW"] or (d["N"] * d["DH"] * d["DW"]) % 64:
        return False
    if d["Ci"] % 64 or d["I1"] % 64 or d["Cj"] % 32 or d["Cj"] < 32:
        return False
    two = d["I1"] != d["Ci"]
    if d["mode"] == 0:
        return bool(q32) and d["ldp"] % 4 == 0 and (not two or d["ldp2"] % 4 == 0) and d["ldq"] % 4 == 0
    if d["ldp"] % 8 or (two and d["ldp2"] % 8):
        return False
    return d["ldq"] % 4 == 0 if q32 else d["ldq"] % 8 == 0


def s2_ok(d):
    if d["stride"] != 2 or d["pad"] != 1 or d["mode"] != 1 or d["KH"] != d["KW"]:
        return False
    if not ((d["KH"] == 3 and d["gather_i"]) or (d["KH"] == 4 and not d["gather_i"])):
        return False
    if d["GH"] != 2 * d["DH"] or d["GW"] != 2 * d["DW"] or d["I1"] != d["Ci"]:
        return False
    w, h = d["DW"], d["DH"]
    if w not in (8, 16, 32) or h % (64 // w) or (d["N"] * h * w) % 64:
        return False
    Cb, Cs = (d["Ci"], d["Cj"]) if d["gather_i"] else (d["Cj"], d["Ci"])
    if Cb % 64 or Cs % 32 or Cs < 32:
        return False
    return not (d["ldp"] % 8 or d["ldq"] % 8)


def s2f_ok(d):
    if d["mode"] != 0 or d["stride"] != 2 or d["pad"] != 1 or d["KH"] != d["KW"] or d["KH"] not in (3, 4):
        return False
    if d["I1"] != d["Ci"] or d["Ci"] % 64 or d["Cj"] % 32 or d["Cj"] < 32 or d["ldp"] % 4 or d["ldq"] % 4:
        return False
    if d["GH"] != 2 * d["DH"] or d["GW"] != 2 * d["DW"] or (d["DH"] & (d["DH"] - 1)) or (d["DW"] & (d["DW"] - 1)):
        return False
    return (d["N"] * d["DH"] * d["DW"]) % 64 == 0


# ------------------------------------------------------------------------------------------------------------ planners
def balance_shares(work, tiles, target):
    """tr_common.h: whole k-slices, handed greedily to the problem whose workgroups carry the most work each."""
    n = len(tiles)
    wgs, total = list(tiles), sum(tiles)
    while True:
        best, worst = -1, 0.0
        for i in range(n):
            per = work[i] / wgs[i]
            if per > worst and total + tiles[i] <= target:
                worst, best = per, i
        if best < 0:
            break
        top = 0.0
        for i in range(n):
            top = max(top, work[i] / wgs[i])
        if worst < top:
            break
        wgs[best] += tiles[best]
        total += tiles[best]
    return wgs


def kslices(total, ntiles, wgs):
    """tr_common.h kslices: (sps, splits) of one problem that is given wgs workgroups."""
    s = max(1, min(wgs // ntiles, total))
    sps = -(-total // s)
    return sps, -(-total // sps)


def _steps(d):
    return d["N"] * d["DH"] * d["DW"] // 64


def tr_tiles(d):
    return (d["Ci"] // 64) * ((d["Cj"] + 127) // 128)


def tr_shares(descs, blocks=0):
    work = [float(d["N"] * d["DH"] * d["DW"] * d["Ci"] * ((d["Cj"] + 127) // 128 * 128)) for d in descs]
    return balance_shares(work, [tr_tiles(d) for d in descs], blocks if blocks > 0 else 256)


def _finish(layers, slot_floats, g8_from):
    """tr_common.h batch_layout, and what the entry points derive from it: wg0, tile0, workspace, reduce instantiation (nimax: w1_launch)."""
    wg = tile = fl = 0
    max_splits, nimax = 1, 1
    for a in layers:
        a["wg0"], a["tile0"] = wg, tile
        wg += a["ntiles"] * a["splits"]
        a["ws_off"] = fl
        a["ws_floats"] = a["splits"] * a["ntiles"] * slot_floats(a) if a["splits"] > 1 else 0
        fl += a["ws_floats"]
        if a["splits"] > 1:
            tile += a["ntiles"]
            nimax = max(nimax, a.get("ni", 1))
        max_splits = max(max_splits, a["splits"])
    return dict(layers=layers, wgs=wg, red_tiles=tile, reduce=None if tile == 0 else (8 if max_splits >= g8_from else 2), nimax=nimax,
                ws_floats=fl, ws_need=fl * 4, ws_bytes=fl * 4 + 256)


def tr_plan(descs, blocks=0):
    """wgrad_tr.hip tr_plan: mi_conv3x3_wgrad_tr_batch's plan."""
    layers = []
    wg = 0
    for d, w in zip(descs, tr_shares(descs, blocks)):
        nt, total = tr_tiles(d), _steps(d)
        sps, splits = kslices(total, nt, w)
        xcd = 0
        if nt > 1 and wg % 8 == 0:
            if splits % 8 == 0:
                xcd = 1
            elif splits < 8 and 8 % splits == 0 and nt % (8 // splits) == 0:
                xcd = 2
        layers.append(dict(ntiles=nt, gx=d["Ci"] // 64, gy=(d["Cj"] + 127) // 128, total=total, sps=sps, splits=splits, xcd_map=xcd, share=w))
        wg += nt * splits
    return _finish(layers, lambda a: 36 * 2048, 64)


def tr_wg_map(a, wg):
    """wgrad_tr_body: workgroup of the problem -> (k-slice, tile)."""
    nt = a["ntiles"]
    if a["xcd_map"] == 1:
        xcd, slot = wg & 7, wg >> 3
        return xcd + 8 * (slot // nt), slot % nt
    if a["xcd_map"] == 2:
        xcd, slot, g = wg & 7, wg >> 3, 8 // a["splits"]
        return xcd // g, (xcd % g) * (nt // g) + slot
    return wg // nt, wg % nt


def w1_ni(d):
    return 2 if d["Ci"] % 128 == 0 and d["mode"] != 0 else 1


def w1_tiles(d):
    return (d["Ci"] // (64 * w1_ni(d))) * ((d["Cj"] + 127) // 128)


def w1_shares(descs, q32, blocks=0):
    by = []
    for d, q in zip(descs, q32):
        tiles_ci, tiles_co = float(d["Ci"] // (64 * w1_ni(d))), float((d["Cj"] + 127) // 128)
        by.append(float(d["N"]) * d["DH"] * d["DW"] * (tiles_co * d["Ci"] * (4.0 if d["mode"] == 0 else 2.0) + tiles_ci * d["Cj"] * (4.0 if q else 2.0)))
    return balance_shares(by, [w1_tiles(d) for d in descs], blocks if blocks > 0 else 256)


def w1_plan(descs, q32, blocks=0):
    """wgrad1x1_tr.hip w1_plan: mi_conv1x1_wgrad_tr_batch's plan (and, per tap group, s2f_group_plan: mi_conv_s2_wgrad_f32's)."""
    layers = []
    for d, w in zip(descs, w1_shares(descs, q32, blocks)):
        nt, total = w1_tiles(d), _steps(d)
        sps, splits = kslices(total, nt, w)
        layers.append(dict(ntiles=nt, ni=w1_ni(d), gx=d["Ci"] // (64 * w1_ni(d)), gy=(d["Cj"] + 127) // 128, total=total, sps=sps, splits=splits,
                           xcd_map=int(nt > 1 and splits > 1), share=w))
    return _finish(layers, lambda a: a["ni"] * 4 * 2048, 32)


def rank_map(wg0, W, wg):
    """tr_common.h xcd_rank (wgrad1_body, wgrad1_f32_body, wgrad_s2_body under xcd_map): workgroup wg of a problem of W workgroups that
    starts at wg0 -> rank by (XCD, order on it)."""
    x = (wg0 + wg) & 7
    rank = (wg - ((x - wg0) & 7)) >> 3
    for xx in range(x):
        rank += (W - ((xx - wg0) & 7) + 7) >> 3
    return rank


def s2_tiles(d):
    Cb, Cs = (d["Ci"], d["Cj"]) if d["gather_i"] else (d["Cj"], d["Ci"])
    return (Cb // 64) * ((Cs + 127) // 128) * (2 if d["KH"] == 4 else 1)


def s2_shares(descs):
    work = [float(d["N"]) * d["DH"] * d["DW"] * d["Ci"] * d["Cj"] * d["KH"] * d["KW"] for d in descs]
    return balance_shares(work, [s2_tiles(d) for d in descs], 256)


def s2_plan(descs):
    """wgrad_s2_tr.hip s2_plan: mi_conv_s2_wgrad_tr_batch's plan."""
    layers = []
    for d, w in zip(descs, s2_shares(descs)):
        nt, total = s2_tiles(d), _steps(d)
        sps, splits = kslices(total, nt, w)
        layers.append(dict(ntiles=nt, KS=d["KH"], total=total, sps=sps, splits=splits, xcd_map=int(nt > 1 and splits > 1), share=w))
    return _finish(layers, lambda a: (36 if a["KS"] == 3 else 32) * 2048, 64)


def s2f_groups(ntap):
    """Taps per launch of mi_conv_s2_wgrad_f32: 9 -> 5 + 4, 16 -> 8 + 8.  -> [(first, count)]"""
    ng = (ntap + MAXP - 1) // MAXP
    out, t0 = [], 0
    for g in range(ng):
        c = (ntap - t0 + (ng - g) - 1) // (ng - g)
        out.append((t0, c))
        t0 += c
    return out


def s2f_plan(d):
    """mi_conv_s2_wgrad_f32: one w1 plan per tap group, on one workspace (the largest group's)."""
    t = dict(d, KH=1, KW=1, pad=0, stride=1, gather_i=1, GH=d["DH"], GW=d["DW"])
    groups = [w1_plan([t] * c, [1] * c) for _, c in s2f_groups(d["KH"] * d["KW"])]
    fl = max(g["ws_floats"] for g in groups)
    return dict(groups=groups, ws_floats=fl, ws_need=fl * 4, ws_bytes=fl * 4 + 256)


def reduce_tails(splits, G):
    """tr_common.h slice_sum, per slice group: (ran the 8-wide main loop, slices left to the tail)."""
    out = set()
    for grp in range(G):
        cnt = len(range(grp, splits, G))
        out.add((cnt >= 8, cnt % 8))
    return out


# ------------------------------------------------------------------------------------------------------------ case lists
class Case:
    def __init__(self, name, layers, blocks=0, mode=1):
        self.name, self.layers, self.blocks, self.mode = name, layers, blocks, mode

    def __repr__(self):
        return self.name


def _both(name, layers, blocks=0, modes=(1, 0)):
    return [Case(f"{name}-{'bf16' if m else 'fp32'}", layers, blocks, m) for m in modes]


# 3x3 stride 1: layers are (N, H, W, Ci, Cj[, I1]); blocks = mi_debug_wgrad_tr_blocks (0: one workgroup per CU)
L_H24, L_H3, L_W8, L_ONE, L_H4 = (2, 24, 32, 64, 128), (5, 3, 64, 64, 64), (3, 16, 8, 128, 160, 64), (1, 8, 8, 64, 32), (4, 4, 16, 64, 96)
TR_CASES = (
    _both("one_step", [L_ONE])                                   # one step, added straight into dW, a co tile three quarters empty
    + _both("h1_w64", [(2, 1, 64, 64, 32)])                      # both zero rows in every step
    + _both("h2_w32", [(1, 2, 32, 64, 64)]) + _both("h4_w16", [L_H4])          # the step is the image
    + _both("w8_two_src", [L_W8]) + _both("w8_two_src_b8", [L_W8], 8) + _both("w8_two_src_b17", [L_W8], 17)
    + _both("h24_b24", [L_H24], 24) + _both("h24_b12", [L_H24], 12) + _both("h24_b8", [L_H24], 8) + _both("h24_b5", [L_H24], 5)
    + _both("h3_w64_b15", [L_H3], 15) + _both("h3_w64_b7", [L_H3], 7) + _both("h3_w64_b2", [L_H3], 2) + _both("h3_w64_b1", [L_H3], 1)
    + _both("h8_w32_sps7", [(5, 8, 32, 64, 64)], 3)
    + _both("xcd1_s8", [(2, 16, 16, 128, 64)], 16) + _both("xcd1_s16", [(4, 16, 16, 128, 160)], 64)
    + _both("xcd2_unsplit", [(1, 8, 8, 256, 256, 192)])
    # the reduce: <2> below 64 k-slices, <8> from 64; every tail length behind the 8-wide main loop (one 8x8 image per step)
    + [c for s in (9, 13, 16, 17, 63, 64, 77, 94, 111, 127) for c in _both(f"splits{s}", [(s, 8, 8, 64, 32)], s)]
    + _both("batch2", [L_H24, L_H4]) + _both("batch3_unsplit_mid", [L_H24, L_ONE, L_W8])
    + _both("batch3_g8", [(64, 8, 8, 64, 32), L_ONE, (2, 16, 16, 128, 64)])
    + _both("batch8", [L_H24, L_ONE, L_W8, L_H3, (1, 2, 32, 64, 64), L_H4, (2, 16, 16, 128, 64), (2, 1, 64, 64, 32)])
    + _both("batch8_b37", [L_W8, L_H24, L_ONE, L_H3, (1, 2, 32, 64, 64), L_H4, (2, 16, 16, 128, 64), (2, 1, 64, 64, 32)], 37)
)

# 1x1: layers are (k, Ci, Cj, I1, q32, bias) over 64 k pixels; blocks = mi_debug_wgrad1x1_tr_blocks
W1_MIX = [(1, 64, 32, 64, 0, 0), (37, 128, 160, 128, 1, 1), (4, 192, 96, 64, 1, 0), (5, 256, 416, 192, 0, 0), (2, 64, 160, 64, 1, 1),
          (3, 128, 32, 64, 1, 1)]
W1_CASES = (
    [Case("k1_q16_ni1", [(1, 64, 32, 64, 0, 0)]), Case("k2_q16_ni2", [(2, 128, 96, 128, 0, 0)]),
     Case("k3_q32_ni1_bias_gx3", [(3, 192, 160, 192, 1, 1)]), Case("k4_q32_ni2_bias_i64", [(4, 256, 416, 64, 1, 1)]),
     Case("k5_q16_ni2_i192", [(5, 256, 96, 192, 0, 0)]), Case("k5_q32_ni1_i64", [(5, 192, 32, 64, 1, 1)]),
     Case("k4_q16_ni1_unsplit", [(4, 192, 160, 128, 0, 0)], 3), Case("k4_q32_ni2_unsplit_bias", [(4, 256, 160, 192, 1, 1)], 4)]
    + [Case(f"k37_b{b}", [(37, 128, 160, 128, 1, 1)], b) for b in (9, 37, 62, 66, 203)]
    + [Case(f"k37_q16_b{b}", [(37, 192, 416, 128, 0, 0)], b) for b in (37, 203)]
    + [Case(f"splits{s}", [(s, 64, 32, 64, 1, 1)], s) for s in (2, 3, 5, 9, 13, 16, 17, 31, 32, 77, 94, 111, 127)]
    + [Case("unsplit_mid", [(5, 64, 96, 64, 0, 0), (1, 256, 160, 64, 1, 1), (37, 128, 160, 128, 1, 1)]), Case("mix", W1_MIX), Case("mix_b9", W1_MIX, 9), Case("mix_b37", W1_MIX, 37), Case("mix_b203", W1_MIX[::-1], 203),
       Case("mix8", W1_MIX + [(5, 64, 96, 64, 0, 0), (2, 256, 32, 256, 1, 0)], 101)]
    + [Case("f32_k1", [(1, 64, 32, 64, 1, 1)], 0, 0), Case("f32_k3_i64_bias", [(3, 192, 160, 64, 1, 1)], 0, 0),
       Case("f32_k5", [(5, 128, 416, 128, 1, 0)], 0, 0), Case("f32_k37_i192_b37", [(37, 256, 96, 192, 1, 1)], 37, 0),
       Case("f32_k37_b203", [(37, 128, 160, 128, 1, 1)], 203, 0), Case("f32_splits77", [(77, 64, 32, 64, 1, 1)], 77, 0),
       Case("f32_mix_b37", [(2, 64, 96, 64, 1, 1), (37, 128, 160, 64, 1, 0), (1, 256, 32, 256, 1, 1)], 37, 0)]
)

# stride 2, bf16: layers are (N, h, w, Ci, Cj, ks); ks = 3: Conv2d (gather_i = 1), ks = 4: ConvTranspose2d (gather_i = 0)
S2_A, S2_B, S2_C = (1, 8, 8, 64, 32, 3), (2, 6, 32, 192, 96, 3), (1, 16, 8, 160, 128, 4)
S2_CASES = [
    Case("one_step_w8_k3", [S2_A]), Case("one_step_w8_k4", [(1, 8, 8, 32, 64, 4)]),
    Case("one_step_w32_k3", [(2, 2, 32, 64, 96, 3)]), Case("one_step_w32_k4", [(2, 2, 32, 96, 64, 4)]),
    Case("one_step_w16_k3", [(1, 4, 16, 128, 160, 3)]), Case("one_step_w16_k4", [(1, 4, 16, 160, 128, 4)]),
    Case("h16_w8_k3", [(1, 16, 8, 128, 32, 3)]), Case("h16_w8_k4", [S2_C]),
    Case("h6_w32_k3", [S2_B]), Case("h6_w32_k4", [(2, 6, 32, 32, 192, 4)]),
    Case("h12_w16_k3", [(3, 12, 16, 64, 160, 3)]), Case("h12_w16_k4", [(3, 12, 16, 96, 64, 4)]),
    Case("g8_k3", [(4, 32, 32, 64, 64, 3)]), Case("g8_k4", [(8, 16, 32, 64, 64, 4)]),
    # the reduce: one 8x8 small image per step and k-slice; <8> from 64 k-slices, every tail length
    *[Case(f"splits{t}_k3", [(t, 8, 8, 64, 32, 3)]) for t in (13, 17, 77, 111)],
    *[Case(f"splits{t}_k4", [(t, 8, 8, 32, 64, 4)]) for t in (5, 16, 63, 94, 127)],
    # no blocks hook: k-slices of several steps (the ring slots rotate inside a slice) need more tiles x steps than one round of the chip
    Case("sps2_w32_k3", [(8, 12, 32, 192, 160, 3)]), Case("sps4_w32_k4", [(11, 12, 32, 160, 192, 4)]),
    Case("sps2_w8_k3", [(48, 8, 8, 192, 160, 3)]), Case("sps3_w16_k4", [(12, 16, 16, 160, 192, 4)]),
    Case("batch2", [S2_A, S2_B]), Case("batch3", [S2_B, S2_A, S2_C]),
    Case("batch8", [S2_A, S2_B, S2_C, (2, 2, 32, 96, 64, 4), (1, 4, 16, 128, 160, 3), (3, 12, 16, 96, 64, 4), (1, 16, 8, 128, 32, 3),
                    (2, 16, 16, 64, 96, 3)]),
]

# stride 2, exact fp32: (N, DH, DW, Ci, Cj, ks, gather_i)
S2F_CASES = [Case(f"n{N}_{h}x{w}_k{ks}_g{g}", [(N, h, w, Ci, Cj, ks, g)], 0, 0)
             for (N, h, w), chans in (((1, 8, 8), ((64, 32), (64, 96))), ((4, 2, 8), ((64, 160), (128, 32))),
                                      ((2, 4, 16), ((128, 96), (64, 32))), ((3, 8, 8), ((64, 96), (128, 160))))
             for ks in (3, 4) for g, (Ci, Cj) in zip((1, 0), chans)]
# 64 steps: the second tap group (4 taps, 64 k-slices each) needs more workspace than the first (5 taps, 32 each); both reduce instantiations
S2F_CASES.append(Case("n64_8x8_k3_g1", [(64, 8, 8, 64, 32, 3, 1)], 0, 0))


def tr_descs(c):
    return [d3(*l, mode=c.mode) for l in c.layers]


def w1_descs(c):
    return [d1(k, Ci, Cj, I1, c.mode) for (k, Ci, Cj, I1, _, _) in c.layers], [l[4] for l in c.layers]


def s2_descs(c):
    return [ds2(N, h, w, Ci, Cj, ks, 1 if ks == 3 else 0) for (N, h, w, Ci, Cj, ks) in c.layers]


def s2f_desc(c):
    N, h, w, Ci, Cj, ks, g = c.layers[0]
    return ds2(N, h, w, Ci, Cj, ks, g, mode=0)


def case_plan(kind, c):
    if kind == "tr":
        return tr_plan(tr_descs(c), c.blocks)
    if kind == "w1":
        return w1_plan(*w1_descs(c), c.blocks)
    if kind == "s2":
        return s2_plan(s2_descs(c))
    return s2f_plan(s2f_desc(c))


def _slice_edges(tag, a, H, TR, out):
    """Edges of one problem's k-slices.  H, TR: image height and rows per step (None for the 1x1 kernels)."""
    out.add(f"{tag}:sps{a['sps']}")
    if a["splits"] == 1:
        out.add(f"{tag}:direct")
    if a["total"] % a["sps"]:
        out.add(f"{tag}:short_last_slice")
    if H is not None:
        for s in range(1, a["splits"]):
            y0 = (s * a["sps"] * TR) % H
            if y0:
                out.add(f"{tag}:slice_starts_inside_image")
                out.add(f"{tag}:row_phase_{y0 // TR}of{H // TR}")
        if a["sps"] * TR > H and a["splits"] > 1:
            out.add(f"{tag}:slice_crosses_images")


def _batch_edges(tag, p, out):
    L = p["layers"]
    out.add(f"{tag}:batch{len(L)}")
    if p["reduce"]:
        out.add(f"{tag}:reduce<{p['reduce']}>")
        for a in L:
            if a["splits"] > 1:
                for main, tail in reduce_tails(a["splits"], p["reduce"]):
                    out.add(f"{tag}:reduce<{p['reduce']}>:tail{tail}{'+main' if main else ''}")
    for i, a in enumerate(L):
        out.add(f"{tag}:xcd_map{a['xcd_map']}")
        if a["xcd_map"] and not tag.startswith("tr"):
            if a["wg0"] % 8:
                out.add(f"{tag}:rank_wg0_not_8")
            if (a["ntiles"] * a["splits"]) % 8:
                out.add(f"{tag}:rank_wgs_not_8")
        if a["splits"] == 1 and any(b["splits"] > 1 for b in L[:i]) and any(b["splits"] > 1 for b in L[i + 1:]):
            out.add(f"{tag}:unsplit_between_split")


def edges():
    """Every named edge the case lists reach."""
    out = set()
    for c in TR_CASES:
        t = "tr" if c.mode else "tr32"
        p = tr_plan(tr_descs(c), c.blocks)
        _batch_edges(t, p, out)
        for l, a in zip(c.layers, p["layers"]):
            N, H, W, Ci, Cj = l[:5]
            _slice_edges(t, a, H, 64 // W, out)
            out.add(f"{t}:W{W}")
            out.add(f"{t}:H{H}_W{W}")
            if H & (H - 1):
                out.add(f"{t}:H_not_pow2")
            if N * H * W == 64:
                out.add(f"{t}:one_step")
            if len(l) > 5 and l[5] != Ci:
                out.add(f"{t}:two_sources")
            if Cj % 128:
                out.add(f"{t}:ragged_co_{Cj % 128}")
            if t == "tr32" and W == 64 and any((s * a["sps"]) % H for s in range(1, a["splits"])):
                out.add("tr32:W64_halo_prefetch_inside_image")
        if len({l[2] for l in c.layers}) > 1:
            out.add(f"{t}:mixed_W")
        two = [len(l) > 5 and l[5] != l[3] for l in c.layers]
        if any(two) and not all(two):
            out.add(f"{t}:P2_null_for_some")
    for c in W1_CASES:
        ds, q32 = w1_descs(c)
        p = w1_plan(ds, q32, c.blocks)
        _batch_edges("w1", p, out)
        for (k, Ci, Cj, I1, q, bias), a in zip(c.layers, p["layers"]):
            kern = "f32" if c.mode == 0 else f"<Q32={q},NI={a['ni']}>"
            out.add(f"w1:{kern}")
            out.add(f"w1:{kern}:k{k}")
            _slice_edges(f"w1:{kern}", a, None, None, out)
            out.add(f"w1:Cj{Cj}")
            out.add(f"w1:Ci{Ci}_I1_{I1}")
            if a["ni"] == 2 and (I1 // 64) % 2:
                out.add("w1:tile_straddles_sources")
            if bias:
                out.add("w1:dbias")
                if a["gx"] > 1:
                    out.add(f"w1:{kern}:dbias_gx>1")
                if a["splits"] > 1:
                    out.add(f"w1:{kern}:dbias_split")
        nis = {a["ni"] for a in p["layers"] if a["splits"] > 1}
        if nis == {1, 2}:
            out.add("w1:reduce_mixed_ni")
        if len(c.layers) > 1:
            if len({l[4] for l in c.layers}) > 1:
                out.add("w1:batch_mixed_dY_types")
            if len({l[5] for l in c.layers}) > 1:
                out.add("w1:batch_null_and_set_dbias")
            if len({a["splits"] > 1 for a in p["layers"]}) > 1:
                out.add("w1:batch_split_and_unsplit")
    for c in S2_CASES:
        p = s2_plan(s2_descs(c))
        _batch_edges("s2", p, out)
        for (N, h, w, Ci, Cj, ks), a in zip(c.layers, p["layers"]):
            t = f"s2:k{ks}"
            _slice_edges(t, a, h, 64 // w, out)
            out.add(f"{t}:w{w}")
            if N * h * w == 64:
                out.add(f"{t}:one_step_w{w}")
            if h & (h - 1):
                out.add(f"{t}:h_not_pow2")
            if w == 8 and h == 16:
                out.add(f"{t}:h16_w8")
            small, big = (Cj, Ci) if ks == 3 else (Ci, Cj)
            out.add(f"s2:small{small}")
            out.add(f"s2:big{big}")
    for c in S2F_CASES:
        N, h, w, Ci, Cj, ks, g = c.layers[0]
        out.add(f"s2f:k{ks}_gather{g}")
        out.add(f"s2f:grid{N}x{h}x{w}")
        if Cj % 128:
            out.add("s2f:ragged_Cj")
        p = s2f_plan(s2f_desc(c))
        if any(a["splits"] > 1 for gp in p["groups"] for a in gp["layers"]):
            out.add("s2f:split")
        if len({gp["ws_floats"] for gp in p["groups"]}) > 1:
            out.add("s2f:groups_differ_in_workspace")
        if p["groups"][1]["ws_floats"] > p["groups"][0]["ws_floats"]:
            out.add("s2f:second_group_needs_more")
    return out


# ------------------------------------------------------------------------------------------------------------ operands
def operands(shape_p, shape_q, kind, seed, p16, q16):
    """(P, Q) as float64 holding exactly the values the kernel is given.  kind "int": X in {-4..4}, dY in {-3..3} (exact in bf16, every
    product and partial sum exact in fp32); "randn": float32 normals, rounded to bf16 where the operand is stored as bf16."""
    g = torch.Generator().manual_seed(seed)
    if kind == "int":
        return (torch.randint(-4, 5, shape_p, generator=g).to(F64), torch.randint(-3, 4, shape_q, generator=g).to(F64))
    p, q = torch.randn(shape_p, generator=g).to(F64), torch.randn(shape_q, generator=g).to(F64)
    return (bf16_round(p) if p16 else p), (bf16_round(q) if q16 else q)


def init_content(n):
    """Small integers a result buffer starts from (the kernels accumulate)."""
    return ((torch.arange(n, dtype=F64) * 5) % 7) - 3
