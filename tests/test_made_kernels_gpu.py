"""MADE's kernels (csrc/made.hip) one by one on the MI355X against the float64 helpers of tests/_made_oracle.py: ragged and
multi-block shapes, pitched operands, both compute modes, the fused head with its per-row log-sum-exp, the sampler's head rows,
non-finite inputs, and the sampling step driven directly with given logits.

Bounds.  fp32 mode: <= 1e-5 of max |ref|, the project's bound.  bf16 mode: the SAME 1e-5, against the reference whose matrix-core
operands are rounded to bf16 as the kernel rounds them (bf16 x bf16 products are exact in fp32, which leaves fp32 accumulation
order and expf; tests/test_made_cpu.py::test_rounded_operands_leave_only_fp32_accumulation measures <= 4e-7 for that on the CPU),
and the old <= 2e-2 against the unrounded reference beside it."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _made_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -777.25                       # padding / never-written sentinel (finite, so torch.equal compares it bit for bit)
MODES = ["fp32", "bf16"]


def _K():
    from src.ops import functional as K
    return K


def _md(K, mode):
    return K.MODE_FP32 if mode == "fp32" else K.MODE_BF16


def _rel(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max()) / max(float(b.abs().max()), 1e-30)


def _degrees(fin, fout, first):
    din = torch.arange(fin) if first else torch.randint(0, 97, (fin,))
    dout = torch.randint(int(din.min()), int(din.max()) + 1, (fout,))
    return din.int(), dout.int()


def _off(pitch):
    return {0: 0, 3: 1, 4: 3}[pitch]


def _pitched(t, pitch, fill=None):
    """(buffer, view): the CPU matrix t (or, with fill, a matrix of t's shape filled with it) as columns [off, off + width) of a
    device buffer of row pitch width + pitch whose other columns hold SENT.  pitch 0: contiguous."""
    n, wd = t.shape
    buf = torch.full((n, wd + pitch), SENT, device=DEV)
    view = buf[:, _off(pitch):_off(pitch) + wd]
    if fill is None:
        view.copy_(t)
    else:
        view.fill_(fill)
    assert view.stride(0) == wd + pitch and (pitch == 0 or not view.is_contiguous() or n == 1)
    return buf, view


def _padding_intact(buf, wd, pitch):
    pad = torch.cat([buf[:, :_off(pitch)], buf[:, _off(pitch) + wd:]], 1)
    return bool((pad == SENT).all())


# ------------------------------------------------------------------ 1. masked linear: forward, data gradient, weight gradient
# (N, in, out, first layer, pitch).  What the three launches make of a triple:
#   forward  : rows N in 32-row blocks, contraction `in` (x rows and W rows both k-contiguous: 16-byte loads where a lane's 8 values
#              are aligned, scalar loads elsewhere and in the K tail), columns `out` in 128-column workgroups;
#   data grad: rows N in 32-row blocks (N <= 64, RM = 1) or 128-row blocks (N > 64, RM = 4), contraction `out` in splits of
#              DGRAD_KSPAN = 2048 (gy rows k-contiguous), columns `in`;
#   wgt grad : rows `out`, columns `in` in 512-column workgroups, contraction N (tail N % 16: 1..7 lower half-wave, 9..15 upper).
# K tail below means in % 16 (forward) / out % 16 (data gradient); "upper" = the tail ends in the half-wave that owns k = 8..15.
LINEAR = [
    (1, 27, 40, True, 0),        # one row; odd pitch 27: every row on the scalar path; K tail 11 (upper, 3 values); out < 128
    (31, 105, 36, False, 0),     # row tail 31; 105 % 4 = 1: rows cycle through the 4 alignments (1 in 4 aligned); K tail 9 (upper, 1)
    (33, 786, 1028, True, 0),    # 2 forward row blocks, tail 1; 786 % 4 = 2: rows alternate aligned / scalar; K tail 2 (lower);
                                 #   column tail 4 in a 9th workgroup; data-gradient K tail 4
    (64, 1000, 36, False, 0),    # no row tail; K tail 8: the lower half-wave full, the upper one empty; RM = 1 at its largest N
    (64, 1024, 1024, False, 0),  # no tail anywhere (rows, K, columns), both for the forward and the data gradient
    (64, 27, 128, True, 0),      # no row tail, K tail, no column tail
    (33, 105, 128, False, 0),    # row tail, K tail, no column tail
    (65, 1024, 1024, False, 0),  # RM = 4 at its smallest N (row tail 65 of 128); forward: 3 row blocks, tail 1; no K / column tail
    (96, 16, 4, False, 0),       # MNIST's last batch: RM = 4 with a row tail, forward without; one exact chunk; data-gradient K = 4
    (1, 16, 4, False, 0),        # row tail, no K tail, column tail
    (127, 8, 2052, True, 0),     # K = 8: the upper half-wave loads nothing; out > DGRAD_KSPAN: 2 splits, the last 4 long
    (257, 8, 2052, True, 0),     # the same splits over 3 data-gradient row blocks (tail 1), 9 forward row blocks
    (130, 27, 40, True, 3),      # pitched; 2 data-gradient row blocks (tail 2); weight-gradient K tail 2
    (257, 105, 36, False, 4),    # pitched; 3 row blocks, tail 1; weight-gradient K tail 1
    (96, 786, 1028, True, 3),    # pitched, odd pitch 789 / 1031 at the real widths: x and gy rows cycle through the alignments
    (33, 1000, 36, False, 4),    # pitched, pitch % 4 = 0 at a column offset of 3: no row aligned although the width is
    (130, 8, 2052, True, 3),     # pitched with 2 splits: the split sum reads its workspace with pitch `in`, s_in / dx with theirs
    (257, 1024, 1024, False, 0), # 3 / 9 row blocks at the hidden layers' real widths
    (127, 786, 1028, True, 0),   # row tail 127 of 128 (RM = 4), 31 of 32 (forward); weight-gradient K tail 15 (upper, 7)
    (31, 1024, 1024, False, 4),  # pitched at the aligned widths: pitch 1028, offset 3
    (65, 1000, 36, False, 0),    # RM = 4 with K tail 4 and column tail 104 of 128
    (256, 52, 77, False, 0),     # RM = 4 without a row tail; out = 77: gy rows cycle through the alignments, K tail 13 (upper, 5)
    (130, 52, 77, False, 4),     # the same widths pitched, with a row tail
    (256, 128, 77, False, 0),    # data gradient: no row tail, K tail, no column tail
    (96, 1024, 36, False, 0),    # data gradient: row tail, K tail, no column tail
]


def test_linear_matrix_covers_the_issue():
    """The matrix above holds every N and width pair it was asked to, at least four pitched triples and both pitches."""
    assert {t[0] for t in LINEAR} >= {1, 31, 33, 64, 65, 96, 127, 130, 257}
    assert {t[1:3] for t in LINEAR} >= {(27, 40), (105, 36), (786, 1028), (1000, 36), (1024, 1024), (16, 4), (8, 2052)}
    assert sum(1 for t in LINEAR if t[4]) >= 4 and {t[4] for t in LINEAR} == {0, 3, 4}
    fwd = {(t[0] % 32 != 0, t[1] % 16 != 0, t[2] % 128 != 0) for t in LINEAR}
    assert len(fwd) == 8                                  # row tail x K tail x column tail, forward
    dg = {((t[0] % (128 if t[0] > 64 else 32)) != 0, t[2] % 16 != 0, t[1] % 128 != 0) for t in LINEAR}
    assert len(dg) == 8                                   # and the data gradient


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,fin,fout,first,pitch", LINEAR)
def test_masked_linear_matrix(n, fin, fout, first, pitch, mode):
    K = _K()
    md, rb = _md(K, mode), mode == "bf16"
    torch.manual_seed(1000 * n + fin + fout)
    din, dout = _degrees(fin, fout, first)
    mask = O.live_mask(din, dout)
    w = torch.randn(fout, fin) / math.sqrt(fin)
    b = torch.randn(fout) * 0.1
    x, gy, s_in = torch.rand(n, fin), torch.randn(n, fout), torch.rand(n, fin)
    dd = [t.to(DEV) for t in (din, dout)]
    wd, bd = w.to(DEV), b.to(DEV)
    xb, xv = _pitched(x, pitch)
    gb, gv = _pitched(gy, pitch)
    sb, sv = _pitched(s_in, pitch)

    # forward, with and without the sigmoid; written into a NaN-filled view, twice
    for act in (True, False):
        yb, yv = _pitched(gy, pitch, fill=float("nan"))
        K.made_linear(xv, wd, bd, *dd, act, out=yv, mode=md)
        err = _rel(yv, O.masked_linear_ref(x, w, b, din, dout, act, rb))
        err0 = _rel(yv, O.masked_linear_ref(x, w, b, din, dout, act, False))
        print(f"forward act={act}: {err:.3g} (unrounded ref {err0:.3g})")
        assert err <= 1e-5 and err0 <= (2e-2 if rb else 1e-5)
        assert _padding_intact(yb, fout, pitch)
        y2b, y2v = _pitched(gy, pitch, fill=float("nan"))
        K.made_linear(xv, wd, bd, *dd, act, out=y2v, mode=md)
        assert torch.equal(yv, y2v)                       # documented as bit-reproducible
    assert _padding_intact(xb, fin, pitch)

    # data gradient
    db_, dv = _pitched(x, pitch, fill=float("nan"))
    K.made_dgrad(gv, wd, *dd, s_in=sv, out=dv, mode=md)
    err = _rel(dv, O.masked_dgrad_ref(gy, w, din, dout, s_in, rb))
    err0 = _rel(dv, O.masked_dgrad_ref(gy, w, din, dout, s_in, False))
    print(f"data gradient: {err:.3g} (unrounded ref {err0:.3g})")
    assert err <= 1e-5 and err0 <= (2e-2 if rb else 1e-5)
    d2b, d2v = _pitched(x, pitch, fill=float("nan"))
    K.made_dgrad(gv, wd, *dd, s_in=sv, out=d2v, mode=md)
    assert torch.equal(dv, d2v)                           # the splits are summed in a fixed order
    assert _padding_intact(db_, fin, pitch) and _padding_intact(sb, fin, pitch) and _padding_intact(gb, fout, pitch)
    if pitch:                                             # and without the s (1 - s) factor
        K.made_dgrad(gv, wd, *dd, out=d2v, mode=md)
        assert _rel(d2v, O.masked_dgrad_ref(gy, w, din, dout, None, rb)) <= 1e-5 and _padding_intact(d2b, fin, pitch)

    # weight gradient: live entries written, masked ones never, the bias gradient written over NaN
    dw = torch.full((fout, fin), SENT, device=DEV)
    db = torch.full((fout,), float("nan"), device=DEV)
    K.made_wgrad(gv, xv, *dd, dw, db, mode=md)
    dw_ref, db_ref = O.masked_wgrad_ref(gy, x, din, dout, rb)
    dwc = dw.cpu()
    assert torch.equal(dwc[~mask], torch.full_like(dwc[~mask], SENT))
    scale = max(float(dw_ref.abs().max()), 1e-30)
    err = float((dwc.double() - dw_ref)[mask].abs().max()) / scale if mask.any() else 0.0
    err0 = float((dwc.double() - O.masked_wgrad_ref(gy, x, din, dout, False)[0])[mask].abs().max()) / scale if mask.any() else 0.0
    print(f"weight gradient: {err:.3g} (unrounded ref {err0:.3g})")
    assert err <= 1e-5 and err0 <= (2e-2 if rb else 1e-5)
    assert torch.isfinite(db).all() and _rel(db, db_ref) <= 1e-5
    assert _padding_intact(xb, fin, pitch) and _padding_intact(gb, fout, pitch)


# ------------------------------------------------------------------ 2. fused head: loss, lse, dlogits; ragged row blocks
# (N, Hd, C, H, W, normalize, pitch of h).  The head runs 128-row blocks (HEAD_ROWS) and one workgroup per pixel; its loss is the sum
# of ceil(N / 128) * D partials written at [blockIdx.y * D + d].
HEAD = [
    (1, 4, 3, 4, 4, False, 0),          # one row: 127 of 128 rows out of range; Hd = 4: the upper half-wave never loads
    (96, 36, 3, 4, 4, True, 3),         # MNIST's last batch; Hd = 36: K tail 4; h pitched; normalize: targets 1..63 truncate one low
    (129, 64, 1, 5, 7, False, 0),       # two row blocks, the second with one row
    (200, 36, 1, 5, 7, True, 0),        # two row blocks, tail 72
    (257, 4, 3, 4, 4, True, 0),         # three row blocks, tail 1
    (257, 64, 1, 5, 7, False, 4),       # three row blocks, h pitched at offset 3
    (200, 1024, 1, 28, 28, False, 0),   # the real size: 2 row blocks x 784 pixels, 98 data-gradient splits behind it
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,hd,C,H,W,normalize,pitch", HEAD)
def test_fused_head_matrix(n, hd, C, H, W, normalize, pitch, mode):
    """loss <= 1e-5 relative, lse <= 1e-5 of max |lse|, dlogits <= 1e-4 of max |ref|, all against the float64 head (operands
    rounded in bf16 mode).  Every pixel's 256 dlogits sum to zero within 4 x 6.3e-7 = 2.52e-6 of their scale factor: 6.3e-7 is what
    an fp32 torch evaluation of exp(v - lse) - onehot leaves on the CPU (tests/test_made_cpu.py::test_dlogits_zero_sum_fp32_floor),
    4 x is the margin for the GPU's expf and summation order.  lse and dlogits come from the same mode: the recomputation in
    mi_made_head_dlogits must reproduce the logits mi_made_head_fwd reduced, or the sum leaves zero."""
    K = _K()
    md, rb = _md(K, mode), mode == "bf16"
    torch.manual_seed(n + hd)
    D = C * H * W
    din = torch.randint(0, D, (hd,)).int()
    dout = (torch.arange(D).repeat_interleave(256) - 1).int()
    w = torch.randn(256 * D, hd) / math.sqrt(hd)
    b = torch.randn(256 * D) * 0.1
    h = torch.rand(n, hd)
    k = torch.randint(0, 256, (n, D))
    special = torch.tensor([0, 255, 1] + list(range(1, 64)))[:k.numel()]
    k.view(-1)[:special.numel()] = special
    k[-1, -1], k[-1, 0] = 255, 0                          # and in the last row of the last row block
    img = k.float() * 2 / 255 - 1 if normalize else k.float() / 255
    if normalize:
        assert int((O.target(img, True) != k).sum()) > 0 or n * D < 4      # the truncating target differs from k somewhere
    _, lse_ref, bpd_ref, dl_ref = O.head_ref(h, w, b, din, dout, img, normalize, rb, gscale=0.75)
    dd = [t.to(DEV) for t in (din, dout)]
    wd, bd, xd = w.to(DEV), b.to(DEV), img.to(DEV)
    hb, hv = _pitched(h, pitch)
    lse = torch.full((n, D), float("nan"), device=DEV)
    loss, lse = K.made_head_fwd(hv, wd, bd, *dd, xd, normalize, lse=lse, mode=md)
    e_loss = abs(float(loss) - float(bpd_ref)) / float(bpd_ref)
    e_lse = float((lse.cpu().double() - lse_ref).abs().max()) / float(lse_ref.abs().max())
    dl = torch.full((n, 256 * D), float("nan"), device=DEV)
    K.made_head_dlogits(hv, wd, bd, *dd, xd, normalize, lse, gscale=torch.full((1,), 0.75, device=DEV), out=dl, mode=md)
    dlc = dl.cpu().double()
    e_dl = float((dlc - dl_ref).abs().max()) / float(dl_ref.abs().max())
    gs = 0.75 / (n * D * O.LN2)
    zs = float(dlc.reshape(n, D, 256).sum(-1).abs().max()) / gs
    print(f"loss {e_loss:.3g}, lse {e_lse:.3g}, dlogits {e_dl:.3g}, zero sum {zs:.3g}")
    assert e_loss <= 1e-5
    assert e_lse <= 1e-5
    assert e_dl <= 1e-4
    assert zs <= 4 * O.ZERO_SUM_FP32
    assert _padding_intact(hb, hd, pitch)


# ------------------------------------------------------------------ 3. the sampler's head rows
# (N, C, HW, Hd, pitch of h): column c of the launch is head row ((c >> 8) * HW + *pos) * 256 + (c & 255).  The same instantiation and
# reduction order as mi_made_linear, so the rows are the matching columns of the full logits bit for bit.
ROWS = [
    (1, 1, 1, 4, 0),             # the smallest everything: the remap is the identity
    (33, 3, 6, 36, 0),           # row tail 1, three channels: columns 256..767 jump by HW pixels
    (130, 4, 35, 1024, 0),       # C = 4: 1024 columns in 8 workgroups, the real hidden width, 5 row blocks
    (130, 1, 6, 1024, 3),        # h pitched
    (33, 4, 1, 36, 0),           # HW = 1 with C = 4: the channel stride of the remap is 1 pixel
    (1, 3, 35, 4, 0),            # one row, Hd = 4
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,C,HW,hd,pitch", ROWS)
def test_head_rows_are_columns_of_the_full_logits(n, C, HW, hd, pitch, mode):
    K = _K()
    md = _md(K, mode)
    torch.manual_seed(n + C + HW)
    D = C * HW
    din = torch.randint(0, D, (hd,)).int().to(DEV)
    dout = (torch.arange(D).repeat_interleave(256) - 1).int().to(DEV)
    w = (torch.randn(256 * D, hd) / math.sqrt(hd)).to(DEV)
    b = (torch.randn(256 * D) * 0.1).to(DEV)
    hb, hv = _pitched(torch.rand(n, hd), pitch)
    full = K.made_linear(hv, w, b, din, dout, False, mode=md).reshape(n, C, HW, 256)
    assert torch.isfinite(full).all()
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    for p in (range(HW) if HW <= 6 else (0, HW // 2, HW - 1)):
        pos.fill_(p)                                      # a device value, as the replayed sampler's counter is
        out = torch.full((n, 256 * C), float("nan"), device=DEV)
        K.made_head_rows(hv, w, b, din, dout, pos, C, HW, out, mode=md)
        assert torch.equal(out, full[:, :, p].reshape(n, 256 * C)), p
    assert _padding_intact(hb, hd, pitch)


# ------------------------------------------------------------------ 4. non-finite inputs at kernel level
def _seen_sum(x, w, b, din, dout):
    """float64 y[n][o] = sum over the LIVE i only of x[n][i] W[o][i] + b[o]: what `W * mask` means for a non-finite x (a plain
    matmul with W * mask would meet NaN * 0 and Inf * 0 at the masked entries)."""
    live = O.live_mask(din, dout)
    prod = x.double()[:, None, :] * w.double()[None]
    return torch.where(live[None], prod, torch.zeros((), dtype=torch.float64)).sum(-1) + b.double()


def _poison(x):
    """NaN and +-Inf at index 0, at an index with k % 16 >= 8, at the last index (in the K tail), and over a whole row.  Rows 0..31
    and 32..63 (one row block each) are poisoned only in part, rows from 64 on are clean."""
    last = x.shape[1] - 1
    nan, inf = float("nan"), float("inf")
    cells = [(2, 0, nan), (5, 12, inf), (7, last, nan), (33, last, -inf), (41, 12, inf), (41, last, -inf), (44, 0, -inf), (45, 12, nan)]
    xp = x.clone()
    for r, i, v in cells:
        xp[r, i] = v
    xp[40] = nan
    return xp


def _check_nonfinite(got, clean, ref, touched):
    got, clean = got.cpu(), clean.cpu()
    assert torch.equal(got[~touched], clean[~touched])    # a unit whose degree excludes every poisoned input: bit-identical
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(torch.isposinf(got), torch.isposinf(ref))
    assert torch.equal(torch.isneginf(got), torch.isneginf(ref))
    fin = torch.isfinite(ref)
    assert fin.any() and float((got.double() - ref)[fin].abs().max()) <= 1e-5 * float(ref[fin].abs().max())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fin", [43, 100])                # K tail 11 (last index in the upper half-wave) and 4 (in the lower one)
def test_linear_nonfinite_inputs_meet_live_weights_only(fin, mode):
    K = _K()
    md, rb = _md(K, mode), mode == "bf16"
    torch.manual_seed(fin)
    n, fout = 70, 200
    din = (torch.arange(fin) + 1).int()                   # degree-0 units see no input at all
    dout = torch.randint(0, fin + 1, (fout,)).int()
    dout[:4] = torch.tensor([0, fin, 13, 1])              # sees nothing / everything / index 12 but not the last / index 0 only
    w = torch.randn(fout, fin) / math.sqrt(fin)
    b = torch.randn(fout) * 0.1
    x = torch.rand(n, fin)
    xp = _poison(x)
    touched = ((~torch.isfinite(xp)).double() @ O.live_mask(din, dout).double().t()) > 0
    assert touched.any() and (~touched[40]).any() and touched[:64].any(1).sum() == 8 and not touched[64:].any()
    dd = [t.to(DEV) for t in (din, dout)]
    for act in (False, True):
        clean = K.made_linear(x.to(DEV), w.to(DEV), b.to(DEV), *dd, act, mode=md)
        got = K.made_linear(xp.to(DEV), w.to(DEV), b.to(DEV), *dd, act, mode=md)
        xr, wr = (xp.bfloat16().float(), w.bfloat16().float()) if rb else (xp, w)
        ref = _seen_sum(xr, wr, b, din, dout)
        _check_nonfinite(got, clean, torch.sigmoid(ref) if act else ref, touched)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hd", [44, 100])
def test_head_rows_nonfinite_inputs_meet_live_weights_only(hd, mode):
    K = _K()
    md, rb = _md(K, mode), mode == "bf16"
    torch.manual_seed(hd)
    n, C, HW = 70, 3, 6
    D = C * HW
    din = torch.randint(0, D, (hd,)).int()
    dout = (torch.arange(D).repeat_interleave(256) - 1).int()   # pixel 0 sees nothing
    w = torch.randn(256 * D, hd) / math.sqrt(hd)
    b = torch.randn(256 * D) * 0.1
    h = torch.rand(n, hd)
    hp = _poison(h)
    dd = [t.to(DEV) for t in (din, dout)]
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    hr, wr = (hp.bfloat16().float(), w.bfloat16().float()) if rb else (hp, w)
    for p in (0, 3, 5):
        sel = torch.cat([torch.arange(256) + (c * HW + p) * 256 for c in range(C)])
        pos.fill_(p)
        clean = torch.full((n, 256 * C), float("nan"), device=DEV)
        got = torch.full((n, 256 * C), float("nan"), device=DEV)
        K.made_head_rows(h.to(DEV), w.to(DEV), b.to(DEV), *dd, pos, C, HW, clean, mode=md)
        K.made_head_rows(hp.to(DEV), w.to(DEV), b.to(DEV), *dd, pos, C, HW, got, mode=md)
        touched = ((~torch.isfinite(hp)).double() @ O.live_mask(din, dout[sel]).double().t()) > 0
        assert torch.isfinite(clean).all() and (p > 0 or not touched[:, :256].any())
        _check_nonfinite(got, clean, _seen_sum(hr, wr[sel], b[sel], din, dout[sel]), touched)


# ------------------------------------------------------------------ 5. mi_made_sample_step on its own
def _step(logits, cnt, tape, img, normalize):
    _K().made_sample_step(logits, cnt, tape, img, normalize)


def _grid(k, normalize):
    v = k.float() / 255
    return v * 2 - 1 if normalize else v


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n,C", [(1, 1), (5, 3), (64, 4), (300, 1)])      # 1, 1, 16 and 19 passes of the 16-wave loop
def test_sample_step_exact_picks(n, C, normalize):
    """Given logits (16 randn: peaked, so few uniforms fall near a CDF boundary) and a uniform tape, the written value is k / 255
    (2k / 255 - 1) with k from the float64 softmax.  Draws within 1e-5 of a bracketing CDF boundary are left out: at most 1 in
    1 000 (measured on the CPU with the reference alone: 1.3e-4 of the draws at this logit scale)."""
    torch.manual_seed(17 * n + C)
    H, W = 1, 7
    U = n * C
    tape = torch.rand(H * W, U)
    td = tape.to(DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    left_out = draws = 0
    for pix in (0, 3, 6, 2):
        logits = 16 * torch.randn(U, 256)
        before = _grid(torch.randint(0, 256, (n, C, H, W)), normalize)
        before[..., pix] = -1.0
        img = before.to(DEV)
        cnt.fill_(pix)
        _step(logits.to(DEV), cnt, td, img, normalize)
        assert int(cnt) == pix + 1                        # the counter advances by exactly 1
        after = img.cpu()
        k, dist = O.pick(F.softmax(logits.double(), -1), tape[pix].double())
        near = dist < 1e-5
        left_out += int(near.sum())
        draws += U
        got, want = after[..., pix].reshape(-1), _grid(k, normalize)
        assert torch.equal(got[~near], want[~near]), pix
        assert ((got >= (-1.0 if normalize else 0.0)) & (got <= 1.0)).all()
        after[..., pix] = -1.0
        assert torch.equal(after, before)                 # only column pix of each (n, c) row changes
    assert left_out * 1000 <= draws, (left_out, draws)


def test_sample_step_distribution():
    """One fixed row of logits shared by 4096 units (N = 1024, C = 4) over 245 positions, 1 003 520 draws: every class count within
    5 sigma of n p (the statistic and bound of PixelCNN's test)."""
    torch.manual_seed(3)
    row = torch.randn(256) * 2
    n, C, H, W = 1024, 4, 5, 49
    logits = row.expand(n * C, 256).contiguous().to(DEV)
    tape = torch.rand(H * W, n * C).to(DEV)
    img = torch.full((n, C, H, W), -1.0, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(H * W):
        _step(logits, cnt, tape, img, False)
    assert int(cnt) == H * W
    v = img.cpu().reshape(-1) * 255
    k = torch.round(v).long()
    assert float((v - k).abs().max()) <= 1e-4 and int(k.min()) >= 0 and int(k.max()) <= 255
    prob = F.softmax(row.double(), 0)
    count = torch.bincount(k, minlength=256).double()
    sig = (k.numel() * prob * (1 - prob)).sqrt()
    assert float(((count - k.numel() * prob).abs() / sig.clamp(min=1e-9)).max()) <= 5.0


def test_sample_step_degenerate_cases():
    n = 64
    one = torch.full((256,), -1e4)
    one[77] = 0
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    img = torch.full((n, 1, 1, 2), -1.0, device=DEV)
    for _ in range(2):
        _step(one.expand(n, 256).contiguous().to(DEV), cnt, torch.rand(2, n).to(DEV), img, False)
    assert torch.equal(img.cpu(), torch.full((n, 1, 1, 2), 77.0) / 255)
    u = torch.tensor([[0.0, 1 - 2 ** -24, 0.5, 0.25] * (n // 4)])
    for normalize in (False, True):
        img = torch.full((n, 1, 1, 1), -1.0, device=DEV)
        cnt.zero_()
        _step(torch.zeros(n, 256, device=DEV), cnt, u.to(DEV), img, normalize)
        want = _grid(torch.tensor([0, 255, 128, 64] * (n // 4)), normalize)
        assert torch.equal(img.cpu().reshape(-1), want)


def test_sample_step_skip_rule_and_counter_past_the_raster():
    """A position where no unit holds -1 is left bit-identical; one unit holding -1 (past the first 1024, the width of the scan)
    gives every unit a draw; at *counter = HW and HW + 1 nothing is written.  The counter advances each time."""
    torch.manual_seed(9)
    n, C, H, W = 300, 4, 1, 7
    U, HW = n * C, H * W
    logits = 16 * torch.randn(U, 256)
    tape = torch.rand(HW, U)
    ld, td = logits.to(DEV), tape.to(DEV)
    cnt = torch.full((1,), 4, dtype=torch.int32, device=DEV)
    given = torch.full((n, C, H, W), 0.3)                 # off the k / 255 grid: a rewrite is visible
    img = given.to(DEV)
    _step(ld, cnt, td, img, False)
    assert torch.equal(img.cpu(), given) and int(cnt) == 5
    given.view(U, HW)[1100, 5] = -1.0
    img = given.to(DEV)
    _step(ld, cnt, td, img, False)
    assert int(cnt) == 6
    after = img.cpu()
    k, dist = O.pick(F.softmax(logits.double(), -1), tape[5].double())
    ok = dist >= 1e-5
    assert int((~ok).sum()) * 1000 <= U
    assert torch.equal(after.view(U, HW)[:, 5][ok], _grid(k, False)[ok])
    col = after.view(U, HW)[:, 5]
    assert torch.equal(col, torch.round(col * 255) / 255)           # every unit got a draw, the given ones too
    after.view(U, HW)[:, 5] = given.view(U, HW)[:, 5]
    assert torch.equal(after, given)
    blank = torch.full((n, C, H, W), -1.0)
    img = blank.to(DEV)
    for c0 in (HW, HW + 1):
        cnt.fill_(c0)
        _step(ld, cnt, td, img, False)
        assert int(cnt) == c0 + 1 and torch.equal(img.cpu(), blank)


def test_sample_step_tape_is_indexed_by_position_then_unit():
    """Two whole-raster runs whose tapes differ only in row 3 differ only at position 3; and the draw of unit u reads tape[pix][u]:
    swapping two units' uniforms swaps nothing but what the reference predicts (covered by the exact picks above)."""
    torch.manual_seed(21)
    n, C, H, W = 40, 3, 1, 7
    U, HW = n * C, H * W
    logits = (2 * torch.randn(U, 256)).to(DEV)            # flat enough that a new uniform nearly always moves the pick
    ta = torch.rand(HW, U)
    tb = ta.clone()
    tb[3] = torch.rand(U)
    out = []
    for t in (ta, tb):
        img = torch.full((n, C, H, W), -1.0, device=DEV)
        cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
        for _ in range(HW):
            _step(logits, cnt, t.to(DEV), img, False)
        assert int(cnt) == HW
        out.append(img.cpu().view(U, HW))
    diff = out[0] != out[1]
    assert diff[:, 3].sum() > U // 2
    diff[:, 3] = False
    assert not diff.any()
