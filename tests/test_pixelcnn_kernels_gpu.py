"""PixelCNN's kernels (csrc/pixelcnn.hip) one by one on the MI355X against the float64 helpers of tests/_pixelcnn_oracle.py, at the
shapes the tiny nets of the fixture (hidden size 8) never reach: more than one row tile, column tile and reduction block, ragged
last tiles, 16-deep chunks that straddle the two sources, pitched NHWC channel slices with sentinels around them, both compute modes,
the head's saved log-sum-exp, the sampling step with its own dot product, and the conditioning helpers.

Bounds.  fp32 mode: <= 1e-5 of max |ref|, the project's bound.  bf16 mode: the SAME 1e-5 against the reference whose matrix-core
operands are rounded to bf16 where the kernel rounds them (bf16 x bf16 products are exact in fp32, which leaves fp32 accumulation
order), and the old <= 2e-2 against the unrounded reference beside it.  The one other bound (the head's dlogits) is derived in its
test's docstring from an fp32 evaluation on the CPU."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pixelcnn_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -777.25                       # padding / never-written sentinel (finite, so torch.equal compares it bit for bit)
MODES = ["fp32", "bf16"]
NAN = float("nan")
ONE = [(0, 0, 0)]                    # the single tap of a 1x1 convolution


def _K():
    from src.ops import functional as K
    return K


def _md(K, mode):
    return K.MODE_FP32 if mode == "fp32" else K.MODE_BF16


def _rel(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max()) / max(float(b.abs().max()), 1e-30)


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.detach().permute(0, 3, 1, 2).cpu()


def _off(pitch):
    return {0: 0, 3: 1, 4: 3, 7: 2}[pitch]


def _pitched(t, pitch, fill=None):
    """(buffer, view): the CPU NHWC tensor t (or, with fill, a tensor of t's shape filled with it) as channels [off, off + C) of a
    device buffer of pixel pitch C + pitch whose other channels hold SENT.  pitch 0: contiguous."""
    n, h, w, c = t.shape
    buf = torch.full((n, h, w, c + pitch), SENT, device=DEV)
    view = buf[..., _off(pitch):_off(pitch) + c]
    if fill is None:
        view.copy_(t)
    else:
        view.fill_(fill)
    assert view.stride(2) == c + pitch or n * h * w == 1
    return buf, view


def _rows(t, pitch, fill=None):
    """_pitched for a [N, J] matrix of per-sample rows."""
    buf, view = _pitched(t[:, None, None, :], pitch, fill)
    return buf[:, 0, 0], view[:, 0, 0]


def _padding_intact(buf, c, pitch):
    pad = torch.cat([buf[..., :_off(pitch)], buf[..., _off(pitch) + c:]], -1)
    return bool((pad == SENT).all())


def _check(what, got, ref_r, ref_0, rb):
    """got against the (operand-rounded, in bf16 mode) reference at 1e-5 and against the unrounded one at 2e-2 (1e-5 in fp32 mode)."""
    err, err0 = _rel(got, ref_r), _rel(got, ref_0)
    print(f"{what}: {err:.3g} (unrounded ref {err0:.3g})")
    assert err <= 1e-5, (what, err)
    assert err0 <= (2e-2 if rb else 1e-5), (what, err0)


def _mask(kind, k):
    from src.models.pixelcnn import horizontal_mask, vertical_mask
    if kind == "1":
        return torch.ones(1, 1)
    return (vertical_mask if kind[0] == "v" else horizontal_mask)(k, kind.endswith("c"))


# ------------------------------------------------------------------ 1. conv: forward, data gradient, weight gradient
# (N, H, W, Cin, Cout, kind, k, dilation, pitch); kind "1": 1x1, "v" / "h": vertical / horizontal mask, "vc" / "hc": mask-centre.
# What the three launches make of a case (P = N H W pixels, T live taps):
#   forward  : 64-pixel row tiles over P, 64-column tiles over Cout, contraction T * Cin in 16-deep chunks;
#   data grad: the same kernel with the weight strides swapped and the taps negated: columns Cin, contraction T * Cout;
#   wgt grad : per live tap, 64 x 64 blocks of (Cin, Cout), contraction over the pixels in splits of 2 048, 16 deep.
CONV = [
    (1, 5, 7, 128, 128, "1", 1, 1, 0),    # conv1x1_1 at the real hidden size: 2 weight-gradient row tiles (blockIdx.x > 0) x 2 column
                                          #   tiles; P = 35: one ragged pixel tile, weight-gradient pixel tail 3 of 16
    (1, 5, 7, 65, 130, "v", 3, 2, 0),     # ragged 2nd / 3rd tiles on both sides (65 = 64 + 1, 130 = 128 + 2); 6 * 65 % 16 = 6: chunks
                                          #   straddle taps and end in a K tail; the data gradient's 6 * 130 % 16 = 12
    (2, 7, 5, 20, 40, "h", 3, 4, 0),      # W = 5 under dilation 4: the tap at dx = -4 is inside at x = 4 only; 2 * 20 % 16 = 8
    (1, 33, 63, 3, 5, "vc", 5, 1, 0),     # P = 2 079 = 2 048 + 31: the 2nd weight-gradient split is 31 pixels (% 16 = 15, < 64); 10 taps
    (1, 5, 7, 128, 128, "1", 1, 1, 3),    # the same four pitched: x, dy and y are channel slices of wider buffers
    (2, 5, 7, 65, 130, "v", 3, 2, 4),     #   two samples: the taps must not reach across the sample boundary
    (2, 7, 5, 20, 40, "h", 3, 4, 3),
    (1, 33, 63, 3, 5, "vc", 5, 1, 4),
    (3, 7, 5, 8, 70, "hc", 5, 1, 3),      # mask-centre horizontal (2 of 5 taps), 2 column tiles (64 + 6), P = 105: 2 pixel tiles
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,H,W,cin,cout,kind,k,dil,pitch", CONV)
def test_conv_matrix(n, H, W, cin, cout, kind, k, dil, pitch, mode):
    """Masked taps of the weight hold SENT on the device: a kernel that read one would show it.  dW starts from non-zero live
    entries (the kernel adds onto them) and zero masked ones, which must stay exactly 0."""
    from src.models.pixelcnn import live_taps
    K = _K()
    md, rb = _md(K, mode), mode == "bf16"
    torch.manual_seed(100 * cin + cout + n)
    mask = _mask(kind, k)
    T = mask.numel()
    taps = live_taps(mask, dil)
    w = torch.randn(cout, cin, *mask.shape) * 0.2
    b = torch.randn(cout)
    x, dy = torch.randn(n, cin, H, W), torch.randn(n, cout, H, W)
    wd = torch.where(mask > 0, w, torch.full_like(w, SENT)).to(DEV)
    xb, xv = _pitched(_nhwc(x), pitch)
    gb, gv = _pitched(_nhwc(dy), pitch)

    yb, yv = _pitched(_nhwc(dy), pitch, fill=NAN)
    K.pcnn_conv(xv, wd, taps, (T, cin * T), cout, bias=b.to(DEV), out=yv, mode=md)
    _check("forward", _nchw(yv), O.conv_ref(x, w, mask, b, dil, rb), O.conv_ref(x, w, mask, b, dil), rb)
    assert _padding_intact(yb, cout, pitch)

    db, dv = _pitched(_nhwc(x), pitch, fill=NAN)
    K.pcnn_conv(gv, wd, [(-a, -c, t) for a, c, t in taps], (cin * T, T), cin, out=dv, mode=md)
    dx_r, dw_r = O.conv_grads_ref(x, w, mask, dy, dil, rb)
    dx_0, dw_0 = O.conv_grads_ref(x, w, mask, dy, dil) if rb else (dx_r, dw_r)
    _check("data gradient", _nchw(dv), dx_r, dx_0, rb)
    assert _padding_intact(db, cin, pitch)

    dw0 = torch.randn_like(w) * 0.5 * mask
    dw = dw0.to(DEV)
    K.pcnn_wgrad(xv, gv, dw, taps, (T, cin * T), mode=md)
    dwc = dw.cpu()
    assert float((dwc * (1 - mask)).abs().max()) == 0.0               # masked taps: never written
    scale = float(dw_r.abs().max())
    err = float((dwc.double() - dw0.double() - dw_r).abs().max()) / scale
    err0 = float((dwc.double() - dw0.double() - dw_0).abs().max()) / scale
    print(f"weight gradient: {err:.3g} (unrounded ref {err0:.3g})")
    assert err <= 1e-5 and err0 <= (2e-2 if rb else 1e-5)
    assert _padding_intact(xb, cin, pitch) and _padding_intact(gb, cout, pitch)


# ------------------------------------------------------------------ 2. plain epilogues at more than one column tile
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", ["bias_res", "accumulate", "accumulate_res", "elu_grad", "elu_grad_res"])
def test_plain_epilogues_two_column_tiles(variant, mode):
    """Cout = 70 (one full column tile and one of 6), P = 100 (2 pixel tiles), Cin = 20; y, res and aux each with a pitch of its own
    (73, 74 and 77 floats).  y = (conv + bias [+ res]) [* ELU'(aux)] [+ y]."""
    K = _K()
    md, rb = _md(K, mode), mode == "bf16"
    n, H, W, cin, cout = 2, 5, 10, 20, 70
    one = torch.ones(1, 1)
    w = torch.randn(cout, cin, 1, 1) * 0.3
    b = torch.randn(cout)
    x = torch.randn(n, cin, H, W)
    res, y0, aux = torch.randn(n, cout, H, W), torch.randn(n, cout, H, W), torch.randn(n, cout, H, W)
    aux.view(-1)[::7] = 0.0                                             # exactly zero: ELU' = exp(0) = 1 on the `else` branch
    assert (aux > 0).any() and (aux < 0).any() and (aux == 0).any()
    xb, xv = _pitched(_nhwc(x), 4)
    rbuf, rv = _pitched(_nhwc(res), 4)
    abuf, av = _pitched(_nhwc(aux), 7)
    acc = variant.startswith("accumulate")
    yb, yv = _pitched(_nhwc(y0), 3, fill=None if acc else NAN)
    use_res = variant.endswith("res")
    eg = variant.startswith("elu_grad")
    K.pcnn_conv(xv, w.to(DEV), ONE, (1, cin), cout, bias=b.to(DEV), res=rv if use_res else None, aux=av if eg else None,
                epi=K.PCNN_ELU_GRAD if eg else K.PCNN_PLAIN, accumulate=acc, out=yv, mode=md)

    def ref(r):
        y = O.conv_ref(x, w, one, b, 1, r)
        if use_res:
            y = y + res.double()
        if eg:
            y = y * O.elu_d(aux)
        return y + y0.double() if acc else y
    _check(variant, _nchw(yv), ref(rb), ref(False), rb)
    assert _padding_intact(yb, cout, 3) and _padding_intact(rbuf, cout, 4) and _padding_intact(abuf, cout, 7) and _padding_intact(xb, cin, 4)


@pytest.mark.parametrize("mode", MODES)
def test_elu_in_forward_twelve_column_tiles(mode):
    """The CIFAR logits path: ELU on load, Cout = 768 (12 column tiles), Cin = 20, P = 30.  bf16 mode rounds x after the ELU."""
    K = _K()
    md, rb = _md(K, mode), mode == "bf16"
    n, H, W, cin, cout = 1, 5, 6, 20, 768
    w = torch.randn(cout, cin, 1, 1) * 0.3
    b = torch.randn(cout)
    x = torch.randn(n, cin, H, W) * 2
    xb, xv = _pitched(_nhwc(x), 3)
    yb, yv = _pitched(torch.empty(n, H, W, cout), 4, fill=NAN)
    K.pcnn_conv(xv, w.to(DEV), ONE, (1, cin), cout, bias=b.to(DEV), elu_in=True, out=yv, mode=md)
    one = torch.ones(1, 1)
    _check("elu_in", _nchw(yv), O.conv_ref(x, w, one, b, 1, rb, elu_in=True), O.conv_ref(x, w, one, b, 1, False, elu_in=True), rb)
    assert _padding_intact(yb, cout, 4) and _padding_intact(xb, cin, 3)
    if rb:                                                              # rounding x before the ELU instead is a visible error
        wrong = O.conv_ref(F.elu(x.bfloat16().double()), O.op(w, True), one, b, 1, False)
        assert _rel(wrong, O.conv_ref(x, w, one, b, 1, True, elu_in=True)) > 1e-4


# ------------------------------------------------------------------ 3. gated layers, both modes
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cond", [False, True])
@pytest.mark.parametrize("C", [20, 33, 40])
def test_gated_layers_ragged_pair_tiles(C, cond, mode):
    """The vertical gate (3x3, dilation 2, tanh * sigmoid) and the horizontal gate (1x3, dilation 2, plus the 1x1 second source of 2C
    channels, tanh * tanh).  C = 20: K1 = 2 * 20 = 40, the chunk k = 32..47 straddles x and x2; C = 33: a full tile of 32 pairs and
    a tile of one pair; C = 40: a full tile and a tile of 8 pairs.  Weights are scaled by 1 / sqrt(fan-in), so the pre-activations
    have unit scale and the gates are not saturated.  The second source is the float32 of the reference's own vertical
    pre-activation, so the horizontal check does not lean on the vertical launch."""
    from src.models.pixelcnn import horizontal_mask, live_taps, vertical_mask
    K = _K()
    md, rb = _md(K, mode), mode == "bf16"
    torch.manual_seed(C + 7)
    n, H, W = 3, 9, 11                                                  # P = 297: 5 pixel tiles, the last of 41
    vx, hx = torch.randn(n, C, H, W), torch.randn(n, C, H, W)
    Wv, bv = torch.randn(2 * C, C, 3, 3) / math.sqrt(6 * C), torch.randn(2 * C) * 0.1
    Wh, bh = torch.randn(2 * C, C, 1, 3) / math.sqrt(4 * C), torch.randn(2 * C) * 0.1
    W11, b11 = torch.randn(2 * C, 2 * C, 1, 1) / math.sqrt(4 * C), torch.randn(2 * C) * 0.1
    cb = torch.randn(n, 4 * C) * 0.5 if cond else None
    vm, hm, one = vertical_mask(3), horizontal_mask(3), torch.ones(1, 1)
    cbuf, cv = _rows(cb, 3) if cond else (None, None)
    cond_v, cond_h = (cv[:, :2 * C], cv[:, 2 * C:]) if cond else (None, None)

    vpre = {r: O.conv_ref(vx, Wv, vm, bv, 2, r) for r in {rb, False}}
    x2 = vpre[False].float()
    hpre = {r: O.conv_ref(hx, Wh, hm, bh, 2, r) + O.conv_ref(x2, W11, one, b11, 1, r) for r in {rb, False}}
    vout = {r: O.gate(vpre[r], cb[:, :2 * C] if cond else None, True) for r in vpre}
    hout = {r: O.gate(hpre[r], cb[:, 2 * C:] if cond else None, False) for r in hpre}

    xb, xv = _pitched(_nhwc(vx), 3)
    ob, ov = _pitched(torch.empty(n, H, W, C), 4, fill=NAN)
    pb, pv = _pitched(torch.empty(n, H, W, 2 * C), 3, fill=NAN)
    wvd = torch.where(vm > 0, Wv, torch.full_like(Wv, SENT)).to(DEV)
    K.pcnn_conv(xv, wvd, live_taps(vm, 2), (9, 9 * C), 2 * C, bias=bv.to(DEV), epi=K.PCNN_GATE_TS, cond=cond_v, out=ov, pre=pv, mode=md)
    _check("vertical pre", _nchw(pv), vpre[rb], vpre[False], rb)
    _check("vertical gate", _nchw(ov), vout[rb], vout[False], rb)
    assert _padding_intact(ob, C, 4) and _padding_intact(pb, 2 * C, 3) and _padding_intact(xb, C, 3)

    hb, hv = _pitched(_nhwc(hx), 4)
    x2b, x2v = _pitched(_nhwc(x2), 3)
    ob, ov = _pitched(torch.empty(n, H, W, C), 3, fill=NAN)
    pb, pv = _pitched(torch.empty(n, H, W, 2 * C), 4, fill=NAN)
    whd = torch.where(hm > 0, Wh, torch.full_like(Wh, SENT)).to(DEV)
    K.pcnn_conv(hv, whd, live_taps(hm, 2), (3, 3 * C), 2 * C, bias=bh.to(DEV), x2=x2v, w2=W11.to(DEV), w2_strides=(1, 2 * C),
                bias2=b11.to(DEV), epi=K.PCNN_GATE_TT, cond=cond_h, out=ov, pre=pv, mode=md)
    _check("horizontal pre", _nchw(pv), hpre[rb], hpre[False], rb)
    _check("horizontal gate", _nchw(ov), hout[rb], hout[False], rb)
    assert _padding_intact(ob, C, 3) and _padding_intact(pb, 2 * C, 4) and _padding_intact(hb, C, 4) and _padding_intact(x2b, 2 * C, 3)
    assert not cond or _padding_intact(cbuf[:, None, None, :], 4 * C, 3)


# ------------------------------------------------------------------ 4. gate backward with several pixel blocks per sample
# (N, H, W, C): a workgroup takes ppb = 8192 / C pixels of one sample and adds its sums into dcond once.
GATE_BWD = [
    (2, 10, 20, 64),                      # HW = 200, ppb = 128: blocks of 128 + 72
    (2, 20, 25, 20),                      # HW = 500, ppb = 409: blocks of 409 + 91
    (2, 1, 5, 4096),                      # the supported maximum: ppb = 2, blocks of 2 + 2 + 1, 32 KB of LDS
]


@pytest.mark.parametrize("n,H,W,C", GATE_BWD)
def test_gate_backward_several_pixel_blocks(n, H, W, C):
    K = _K()
    from src.ops.lib import load_library
    assert load_library().mi_pcnn_gate_bwd_supported(4096) == 1 and load_library().mi_pcnn_gate_bwd_supported(4097) == 0
    torch.manual_seed(C)
    cb = torch.randn(n, 4 * C) * 0.5
    dc0 = torch.randn(n, 4 * C)
    cbuf, cv = _rows(cb, 3)
    dbuf, dv = _rows(dc0, 3)
    want = dc0.double().clone()
    for kind, ts, sl in ((K.PCNN_GATE_TS, True, slice(0, 2 * C)), (K.PCNN_GATE_TT, False, slice(2 * C, 4 * C))):
        pre, dout = torch.randn(n, 2 * C, H, W), torch.randn(n, C, H, W)
        pb, pv = _pitched(_nhwc(pre), 3)
        gb, gv = _pitched(_nhwc(dout), 4)
        ob, ov = _pitched(_nhwc(pre), 4, fill=NAN)
        K.pcnn_gate_bwd(pv, gv, kind, cond=cv[:, sl], dcond=dv[:, sl], dpre=ov)
        dp_ref, sums = O.gate_bwd_ref(pre, cb[:, sl], dout, ts)
        err = _rel(_nchw(ov), dp_ref)
        want[:, sl] += sums
        e_dc = float((dv[:, sl].cpu().double() - want[:, sl]).abs().max()) / float(sums.abs().max())
        print(f"kind {kind}: dpre {err:.3g}, dcond {e_dc:.3g}")
        assert err <= 1e-5 and e_dc <= 1e-5
        assert _padding_intact(pb, 2 * C, 3) and _padding_intact(gb, C, 4) and _padding_intact(ob, 2 * C, 4)
    assert _padding_intact(cbuf[:, None, None, :], 4 * C, 3) and _padding_intact(dbuf[:, None, None, :], 4 * C, 3)


# ------------------------------------------------------------------ 5. column sums
COLSUM = [(1, 1, 1), (1023, 3, 3), (1025, 65, 70), (2049, 130, 130)]      # (M, C, ld): one row span is 1 024 rows, one column tile 64


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("M,C,ld", COLSUM)
def test_column_sums_row_spans(M, C, ld, both):
    """out (and out2) += column sums, onto non-zero content.  Against float64 at 1e-5 of the largest sum: an fp32 evaluation of the
    2 049-row sums in the kernel's order on the CPU is 3.7e-7 off (tests/test_pixelcnn_cpu.py::test_column_sum_fp32_floor), so the
    project's bound holds as it is."""
    K = _K()
    torch.manual_seed(M + C)
    g = torch.randn(1, 1, M, C)
    buf = torch.full((1, 1, M, ld), SENT, device=DEV)
    gv = buf[..., :C]
    gv.copy_(g)
    sums = g.double().sum((0, 1, 2))
    assert float(sums.abs().max()) >= 0.05
    o1, o2 = torch.randn(C), torch.randn(C)
    d1, d2 = o1.to(DEV), o2.to(DEV)
    K.pcnn_colsum(gv, d1, d2 if both else None)
    scale = float(sums.abs().max())
    e1 = float((d1.cpu().double() - o1.double() - sums).abs().max()) / scale
    e2 = float((d2.cpu().double() - o2.double() - sums).abs().max()) / scale if both else 0.0
    print(f"colsum {e1:.3g} {e2:.3g}")
    assert e1 <= 1e-5 and e2 <= 1e-5
    assert both or torch.equal(d2.cpu(), o2)
    assert bool((buf[..., C:] == SENT).all())


# ------------------------------------------------------------------ 6. head: loss, lse, dlogits
# (N, H, W, Cc, Ch, normalize, pitch of h).  64 (pixel, colour) units per workgroup, one partial each, one 256-thread reduce.
HEAD = [
    (1, 3, 3, 1, 254, False, 0),          # the LDS limit: 64 rows of 255 floats
    (2, 3, 5, 3, 1, True, 0),             # one hidden unit; 90 units: the second workgroup holds 26
    (1, 5, 7, 2, 20, True, 0),            # Cc = 2, 70 units
    (3, 3, 5, 4, 8, False, 0),            # Cc = 4, 180 units
    (2, 46, 60, 3, 8, False, 0),          # 16 560 units, 259 partials: the reduce loop runs twice for threads 0..2
    (2, 5, 7, 3, 20, True, 3),            # h pitched; 210 units
]


def _head_case(n, H, W, Cc, Ch, normalize):
    h = torch.randn(n, H, W, Ch)
    w, b = torch.randn(256 * Cc, Ch), torch.randn(256 * Cc)
    s = 20.0 / float(O.head_logits(h.reshape(-1, Ch), w, b).std())      # logits of standard deviation 20: they span about +-60
    w, b = (w * s).float(), (b * s).float()
    k = torch.randint(0, 256, (n, Cc, H, W))
    special = torch.tensor([0, 255] + list(range(1, 64)))[:k.numel() - 2]
    k.view(-1)[:special.numel()] = special
    k.view(-1)[-2:] = torch.tensor([255, 0])                            # and in the last workgroup
    img = k.float() * 2 / 255 - 1 if normalize else k.float() / 255
    return h, w, b, k, img


@pytest.mark.parametrize("n,H,W,Cc,Ch,normalize,pitch", HEAD)
def test_head_matrix(n, H, W, Cc, Ch, normalize, pitch):
    """loss <= 1e-5 relative and the saved lse <= 1e-5 of max |lse|, both against float64.  dlogits against
    (softmax - onehot) g / (N Cc H W ln 2) with g = 0.75: <= max(1e-5, 4 x floor) of max |ref|, where floor is what the same head
    evaluated in fp32 on the CPU (O.head_ref(dtype=float32): the kernel's sequential chain over the hidden units, each step rounded)
    leaves against float64 for this test's seeded input.  The logits reach +-70 to +-170, where one fp32 ulp is 7.6e-6 to 1.5e-5,
    so exp(l - lse) of a class of probability near 1 cannot be better than that.  Measured on the CPU for the six cases in order:
    3.8e-6, 3.5e-6, 3.5e-6, 3.6e-6, 6.3e-6, 3.6e-6 (bounds 1.5e-5, 1.4e-5, 1.4e-5, 1.4e-5, 2.5e-5, 1.4e-5); the factor 4 allows for
    the GPU's expf and another summation order."""
    K = _K()
    from src.ops.lib import load_library
    assert load_library().mi_pcnn_head_supported(1, 254) == 1 and load_library().mi_pcnn_head_supported(1, 255) == 0
    torch.manual_seed(n * H * W + Ch)
    h, w, b, k, img = _head_case(n, H, W, Cc, Ch, normalize)
    assert {0, 255} <= set(k.view(-1).tolist())
    if normalize:
        assert set(range(1, 64)) <= set(k.view(-1).tolist()) and int((O.target(img, True) != k).sum()) >= 63
    assert (n * H * W * Cc) % 64 != 0
    lse_ref, bpd_ref, dl_ref = O.head_ref(h, w, b, img, normalize, gscale=0.75)
    floor = _rel(O.head_ref(h, w, b, img, normalize, gscale=0.75, dtype=torch.float32)[2], dl_ref)
    hb, hv = _pitched(h, pitch)
    wd, bd, xd = w.to(DEV), b.to(DEV), img.to(DEV)
    lse = torch.full((n * H * W * Cc,), NAN, device=DEV)
    loss, lse = K.pcnn_head_fwd(hv, wd, bd, xd, normalize, lse=lse)
    e_loss = abs(float(loss) - float(bpd_ref)) / float(bpd_ref)
    e_lse = _rel(lse.reshape(n, H, W, Cc), lse_ref)
    dl = torch.full((n, H, W, 256 * Cc), NAN, device=DEV)
    K.pcnn_head_dlogits(hv, wd, bd, xd, normalize, lse, gscale=torch.full((1,), 0.75, device=DEV), out=dl)
    e_dl = _rel(dl, dl_ref)
    span = float(O.head_logits(h.reshape(-1, Ch), w, b).abs().max())
    print(f"loss {e_loss:.3g}, lse {e_lse:.3g}, dlogits {e_dl:.3g} (fp32 floor on the CPU {floor:.3g}), max |logit| {span:.3g}")
    assert span >= 50                                                    # the peaked regime of a trained net
    assert e_loss <= 1e-5
    assert e_lse <= 1e-5
    assert e_dl <= max(1e-5, 4 * floor)
    assert _padding_intact(hb, Ch, pitch)


# ------------------------------------------------------------------ 7. the sampling step, driven directly
def _sample_buffers(n, cc, before):
    """(img NCHW, xin buffer, xin view): the network input is a channel slice of pitch cc + 1 whose spare channel holds SENT."""
    H, W = O.SAMPLE_HW
    xbuf = torch.full((n, H, W, cc + 1), SENT, device=DEV)
    xbuf[..., :cc] = _nhwc(before).to(DEV)
    return before.to(DEV), xbuf, xbuf[..., :cc]


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n,cc", O.SAMPLE_UNITS)
def test_sample_step_exact_picks(n, cc, normalize):
    """Non-zero h (pitched), weights and bias: the written value is bit-equal to k / 255 (2k / 255 - 1) with k from the float64 softmax
    of the float64 logits, in the NCHW image and in the NHWC input (ldx = Cc + 1), and nothing else changes.  Draws within 1e-5 of a
    CDF boundary are left out; tests/test_pixelcnn_cpu.py::test_sample_scenarios_stay_inside_the_skip_cap counts them on the CPU."""
    K = _K()
    H, W = O.SAMPLE_HW
    h, w, b, tape, logits = O.sample_scenario(n, cc, normalize)
    hb, hv = _pitched(h, 3)
    wd, bd, td = w.to(DEV), b.to(DEV), tape.to(DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    for pix in O.SAMPLE_PIXELS:
        before = O.grid(torch.randint(0, 256, (n, cc, H, W)), normalize)
        before.view(n, cc, -1)[..., pix] = -1.0
        img, xbuf, xv = _sample_buffers(n, cc, before)
        cnt.fill_(pix)
        K.pcnn_sample_step(hv, wd, bd, cnt, td, img, xv, normalize)
        assert int(cnt) == pix + 1
        k, near = O.sample_picks(logits, tape, pix)
        want = O.grid(k, normalize)
        after, xafter = img.cpu().view(n, cc, -1), xbuf.cpu().view(n, H * W, cc + 1)
        got, gotx = after[..., pix].reshape(-1), xafter[:, pix, :cc].reshape(-1)
        assert torch.equal(got[~near], want[~near]) and torch.equal(gotx, got), pix
        after[..., pix] = -1.0
        xafter[:, pix, :cc] = -1.0
        assert torch.equal(after.view_as(before), before)               # only pixel pix changes, in both layouts
        assert torch.equal(xafter[..., :cc], _nhwc(before).view(n, H * W, cc)) and bool((xafter[..., cc] == SENT).all())
    assert _padding_intact(hb, O.SAMPLE_CH, 3)


def test_sample_step_skip_rule_and_counter_past_the_raster():
    """A pixel no sample has at -1 is left bit-identical (the counter still advances); one sample holding -1 there gives the whole
    batch a draw; with the counter at H W and past it nothing is written and the counter becomes pix + 1."""
    K = _K()
    n, cc = 100, 3
    H, W = O.SAMPLE_HW
    HW = H * W
    h, w, b, tape, logits = O.sample_scenario(n, cc, False)
    hb, hv = _pitched(h, 3)
    wd, bd, td = w.to(DEV), b.to(DEV), tape.to(DEV)
    given = torch.full((n, cc, H, W), 0.3)                              # off the k / 255 grid: a rewrite is visible
    img, xbuf, xv = _sample_buffers(n, cc, given)
    cnt = torch.full((1,), 4, dtype=torch.int32, device=DEV)
    K.pcnn_sample_step(hv, wd, bd, cnt, td, img, xv, False)
    assert int(cnt) == 5 and torch.equal(img.cpu(), given) and torch.equal(xv.cpu(), _nhwc(given))
    given[97, 1].view(-1)[5] = -1.0                                     # unit 292 alone, in the last pass of the 16-wave loop
    img, xbuf, xv = _sample_buffers(n, cc, given)
    K.pcnn_sample_step(hv, wd, bd, cnt, td, img, xv, False)
    assert int(cnt) == 6
    k, near = O.sample_picks(logits, tape, 5)
    after = img.cpu().view(n, cc, HW)
    col = after[..., 5].reshape(-1)
    assert torch.equal(col[~near], O.grid(k, False)[~near])
    assert torch.equal(col, torch.round(col * 255) / 255)               # every unit got a draw, the given ones too
    assert torch.equal(xbuf.cpu().view(n, HW, cc + 1)[:, 5, :cc].reshape(-1), col)
    after[..., 5] = given.view(n, cc, HW)[..., 5]
    assert torch.equal(after.view_as(given), given)
    blank = torch.full((n, cc, H, W), -1.0)
    img, xbuf, xv = _sample_buffers(n, cc, blank)
    for c0 in (HW, HW + 1, HW + 1000):
        cnt.fill_(c0)
        K.pcnn_sample_step(hv, wd, bd, cnt, td, img, xv, False)
        assert int(cnt) == c0 + 1 and torch.equal(img.cpu(), blank) and torch.equal(xv.cpu(), _nhwc(blank))
    assert bool((xbuf[..., cc] == SENT).all())


# ------------------------------------------------------------------ 8. conditioning helpers
def test_conditioning_rows_and_weight_gradient():
    """mi_pcnn_cond_rows / mi_pcnn_cond_wgrad against index-select and against the one-hot mi_pcnn_small_mm path (accumulate
    included): duplicate labels are summed, labels -1 and ncls give zero rows and no gradient, out / dcond are pitched rows."""
    K = _K()
    J, ncls = 50, 6                                                     # N J = 450: two workgroups
    lab = torch.tensor([1, 4, 1, -1, 5, 6, 0, 4, 1])
    N = lab.numel()
    ok = (lab >= 0) & (lab < ncls)
    oh = torch.zeros(N, ncls)
    oh[ok] = F.one_hot(lab[ok], ncls).float()
    w = torch.randn(J, ncls)
    wd, ohd, labd = w.to(DEV), oh.to(DEV), lab.to(DEV)
    want = torch.where(ok[:, None], w.t()[lab.clamp(0, ncls - 1)], torch.zeros(N, J))
    ob, ov = _rows(want, 3, fill=NAN)
    K.pcnn_cond_rows(labd, wd, ov)
    assert torch.equal(ov.cpu(), want) and _padding_intact(ob[:, None, None, :], J, 3)
    mb, mv = _rows(want, 4, fill=NAN)
    K.pcnn_small_mm(N, J, ncls, ohd, ncls, 1, wd, 1, ncls, mv, mv.stride(0))
    assert torch.equal(mv.cpu(), want) and _padding_intact(mb[:, None, None, :], J, 4)
    K.pcnn_small_mm(N, J, ncls, ohd, ncls, 1, wd, 1, ncls, mv, mv.stride(0), accumulate=True)
    assert torch.equal(mv.cpu(), want * 2) and _padding_intact(mb[:, None, None, :], J, 4)

    dc = torch.randn(N, J)
    dbuf, dv = _rows(dc, 3)
    g0 = torch.randn(J, ncls)
    ref = g0.double() + dc.double().t() @ oh.double()
    scale = float((dc.double().t() @ oh.double()).abs().max())
    ga, gb = g0.to(DEV), g0.to(DEV)
    K.pcnn_cond_wgrad(labd, dv, ga)
    K.pcnn_small_mm(J, ncls, N, dv, 1, dv.stride(0), ohd, ncls, 1, gb, ncls, accumulate=True)
    ea, eb = (float((t.cpu().double() - ref).abs().max()) / scale for t in (ga, gb))
    print(f"cond_wgrad {ea:.3g}, one-hot small_mm {eb:.3g}")
    assert ea <= 1e-5 and eb <= 1e-5
    assert _padding_intact(dbuf[:, None, None, :], J, 3)
