"""Per-kernel parity: every C-ABI entry point against a float64 CPU evaluation of the same
reference op (torch CPU = the reference's own arithmetic, ddpm.py line cited per test).
Tolerances (rel-L2): 2e-5 in exact-fp32 mode, 2e-2 in bf16-MFMA mode (CPU bf16
autocast of the reference differs from fp64 by 1.6e-2)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import DEV, TOL, conv_w_storage, from_nhwc, max_err, rel_err, to_nhwc_gpu, w_from_storage

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from src.ops import functional
    return functional


def _conv_case(K, mode, N, H, W, Ci, Co, k, s, p, seed=0, bias=True, split=None, residual=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, k, k, generator=g) / math.sqrt(Ci * k * k)
    b = torch.randn(Co, generator=g) if bias else None
    ref = F.conv2d(x.double(), w.double(), b.double() if bias else None, stride=s, padding=p)
    OH, OW = ref.shape[2], ref.shape[3]
    r = torch.randn(N, Co, OH, OW, generator=g) if residual else None
    if residual:
        ref = ref + r.double()
    ws = conv_w_storage(w)
    if split:
        xa, xb = to_nhwc_gpu(x[:, :split]), to_nhwc_gpu(x[:, split:])
    else:
        xa, xb = to_nhwc_gpu(x), None
    y = K.conv_igemm(xa, ws, kh=k, kw=k, stride=s, pad=p, transposed=False, w_kn=True, K=Ci, Nc=Co, out_hw=(OH, OW),
                     mode=mode, x2=xb, bias=b.to(DEV) if bias else None,
                     residual=to_nhwc_gpu(r) if residual else None)
    torch.cuda.synchronize()
    return rel_err(from_nhwc(y), ref), (x, w, b, ref, xa, xb, ws)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cfg", [
    dict(N=2, H=8, W=8, Ci=32, Co=32, k=3, s=1, p=1),
    dict(N=2, H=16, W=16, Ci=128, Co=128, k=3, s=1, p=1),
    dict(N=3, H=8, W=8, Ci=24, Co=40, k=3, s=1, p=1),                 # ragged K and N tiles
    dict(N=2, H=8, W=8, Ci=3, Co=16, k=3, s=1, p=1),                  # image input, Cin=3
    dict(N=2, H=8, W=8, Ci=16, Co=3, k=1, s=1, p=0),                  # final conv, Cout=3
    dict(N=2, H=16, W=16, Ci=64, Co=64, k=3, s=2, p=1),               # Downsample (ddpm.py:79)
    dict(N=2, H=8, W=8, Ci=64, Co=384, k=1, s=1, p=0, bias=False),    # to_qkv (ddpm.py:151)
    dict(N=2, H=8, W=8, Ci=64, Co=32, k=3, s=1, p=1, split=32),       # skip concat read in place (ddpm.py:255)
    dict(N=2, H=8, W=8, Ci=128, Co=64, k=1, s=1, p=0, residual=True), # to_out + Residual (ddpm.py:45,152)
    dict(N=5, H=7, W=7, Ci=16, Co=16, k=3, s=1, p=1),                 # odd spatial size (MNIST 7x7 level)
    dict(N=16, H=32, W=32, Ci=128, Co=128, k=3, s=1, p=1),            # 128x128 tiles, many blocks
])
def test_conv_forward(K, mode, cfg):
    err, _ = _conv_case(K, mode, **cfg)
    assert err < TOL[mode], err


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cfg", [
    dict(N=2, H=8, W=8, Ci=32, Co=48, k=3, s=1, p=1),
    dict(N=2, H=16, W=16, Ci=64, Co=64, k=3, s=2, p=1),
    dict(N=2, H=8, W=8, Ci=64, Co=24, k=1, s=1, p=0),
    dict(N=2, H=8, W=8, Ci=16, Co=3, k=1, s=1, p=0),
    dict(N=4, H=16, W=16, Ci=128, Co=128, k=3, s=1, p=1),
])
def test_conv_dgrad_and_wgrad(K, mode, cfg):
    """aten::convolution_backward (input, weight, bias) for Conv2d."""
    N, H, W, Ci, Co, k, s, p = (cfg[q] for q in ("N", "H", "W", "Ci", "Co", "k", "s", "p"))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(Co, Ci, k, k, generator=g, dtype=torch.float64) / math.sqrt(Ci * k * k)).requires_grad_(True)
    b = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, b, stride=s, padding=p)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    ws = conv_w_storage(w.detach())
    dyg = to_nhwc_gpu(dy.float())
    dx = K.conv_igemm(dyg, ws, kh=k, kw=k, stride=s, pad=p, transposed=True, w_kn=False, K=Co, Nc=Ci, out_hw=(H, W), mode=mode)
    dW = torch.zeros(k * k * Ci * Co, device=DEV)
    xg = to_nhwc_gpu(x.detach().float())
    K.conv_wgrad(xg, dyg, dW, kh=k, kw=k, stride=s, pad=p, gather_i=True, Ci=Ci, Cj=Co, grid_g=(H, W),
                 grid_d=(y.shape[2], y.shape[3]), mode=mode)
    db = torch.zeros(Co, device=DEV)
    K.colsum(dyg, db)
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(dx), x.grad) < TOL[mode]
    assert rel_err(w_from_storage(dW.view(k, k, Ci, Co)), w.grad) < TOL[mode]
    assert rel_err(db, b.grad) < 2e-5
    # accumulate=True adds onto an existing gradient
    dx2 = K.conv_igemm(dyg, ws, kh=k, kw=k, stride=s, pad=p, transposed=True, w_kn=False, K=Co, Nc=Ci, out_hw=(H, W),
                       mode=mode, out=dx.clone(), accumulate=True)
    assert rel_err(from_nhwc(dx2), 2 * x.grad) < TOL[mode]


@pytest.mark.parametrize("cfg", [dict(N=4, h=16, C=128), dict(N=8, h=8, C=256), dict(N=2, h=32, C=64), dict(N=3, h=8, C=64, Co=192)])
def test_stride2_family_reads_bf16_activations(K, cfg):
    """mi_conv_igemm_bf16w_io: Downsample (3x3 / stride 2), Upsample (4x4 / stride 2 transposed) and both data gradients with
    bf16-STORED activations (64-channel ring stages) against fp64 on the same bf16-rounded operands; accumulate and bias."""
    g = torch.Generator().manual_seed(61)
    N, h, Ci = cfg["N"], cfg["h"], cfg["C"]
    Co = cfg.get("Co", Ci)
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
    # Downsample forward + its data gradient
    x = torch.randn(N, Ci, 2 * h, 2 * h, generator=g).bfloat16()
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(Ci * 9)).bfloat16()
    b = torch.randn(Co, generator=g)
    xd = x.double().requires_grad_(True)
    y = F.conv2d(xd, w.double(), b.double(), stride=2, padding=1)
    dy = torch.randn(y.shape, generator=g).bfloat16()
    y.backward(dy.double())
    ws = conv_w_storage(w.float())                                      # [kh][kw][ci][co]
    wf, wd = ws.permute(0, 1, 3, 2).contiguous().bfloat16(), ws.bfloat16()
    assert K.igemm_bf16_in_supported(Ci, Co, 3, 2, False, 1, (h, h))
    yg = K.conv_igemm(nh(x), ws, kh=3, kw=3, stride=2, pad=1, transposed=False, w_kn=True, K=Ci, Nc=Co, out_hw=(h, h), mode=1,
                      bias=b.to(DEV), wb=wf)
    dxg = K.conv_igemm(nh(dy), ws, kh=3, kw=3, stride=2, pad=1, transposed=True, w_kn=False, K=Co, Nc=Ci, out_hw=(2 * h, 2 * h), mode=1, wb=wd)
    dx2 = K.conv_igemm(nh(dy), ws, kh=3, kw=3, stride=2, pad=1, transposed=True, w_kn=False, K=Co, Nc=Ci, out_hw=(2 * h, 2 * h), mode=1, wb=wd,
                       out=dxg.clone(), accumulate=True)
    torch.cuda.synchronize()
    assert yg.dtype == torch.float32 and rel_err(from_nhwc(yg), y) < 2e-5
    assert rel_err(from_nhwc(dxg), xd.grad) < 2e-5 and rel_err(from_nhwc(dx2), 2 * xd.grad) < 2e-5
    # Upsample forward + its data gradient
    x = torch.randn(N, Ci, h, h, generator=g).bfloat16()
    w = (torch.randn(Ci, Co, 4, 4, generator=g) / math.sqrt(Ci * 4)).bfloat16()
    xd = x.double().requires_grad_(True)
    y = F.conv_transpose2d(xd, w.double(), b.double(), stride=2, padding=1)
    dy = torch.randn(y.shape, generator=g).bfloat16()
    y.backward(dy.double())
    ws = conv_w_storage(w.float(), transposed=True)
    wf, wd = ws.permute(0, 1, 3, 2).contiguous().bfloat16(), ws.bfloat16()
    yg = K.conv_igemm(nh(x), ws, kh=4, kw=4, stride=2, pad=1, transposed=True, w_kn=True, K=Ci, Nc=Co, out_hw=(2 * h, 2 * h), mode=1,
                      bias=b.to(DEV), wb=wf)
    dxg = K.conv_igemm(nh(dy), ws, kh=4, kw=4, stride=2, pad=1, transposed=False, w_kn=False, K=Co, Nc=Ci, out_hw=(h, h), mode=1, wb=wd)
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(yg), y) < 2e-5 and rel_err(from_nhwc(dxg), xd.grad) < 2e-5
    # a layer the ring kernel does not take is refused, not silently converted
    with pytest.raises(RuntimeError):
        K.conv_igemm(torch.zeros(2, 8, 8, 32, device=DEV).bfloat16(), torch.zeros(3, 3, 32, 32, device=DEV), kh=3, kw=3, stride=2, pad=1,
                     transposed=False, w_kn=True, K=32, Nc=32, out_hw=(4, 4), mode=1, wb=torch.zeros(9 * 32 * 32, device=DEV).bfloat16())


@pytest.mark.parametrize("cfg", [dict(N=4, h=16, C=128), dict(N=8, h=8, C=256), dict(N=2, h=32, C=64), dict(N=4, h=8, C=64, Co=192),
                                 dict(N=64, h=16, C=128), dict(N=1, h=8, C=64)])
def test_stride2_family_tap_gather_kernel(K, cfg):
    """mi_conv_gt (round 4): Downsample (3x3 / stride 2; reference ddpm.py:76-82), Upsample (ConvTranspose2d(4, 2, 1); ddpm.py:67-73)
    and both data gradients for bf16-stored activations on the private-weight-stream machinery -- per tap a DMA gather of the strided
    pixel rows, the transposed forms as four parity classes.  Against fp64 on the same bf16-rounded operands; bias, accumulate,
    fp32 and bf16 outputs, 128- and 64-pixel tiles, a channel count that is not a multiple of 128."""
    g = torch.Generator().manual_seed(97)
    N, h, Ci = cfg["N"], cfg["h"], cfg["C"]
    Co = cfg.get("Co", Ci)
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
    K.PROBE = []
    try:
        # Downsample forward + its data gradient
        x = torch.randn(N, Ci, 2 * h, 2 * h, generator=g).bfloat16()
        w = (torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(Ci * 9)).bfloat16()
        b = torch.randn(Co, generator=g)
        xd = x.double().requires_grad_(True)
        y = F.conv2d(xd, w.double(), b.double(), stride=2, padding=1)
        dy = torch.randn(y.shape, generator=g).bfloat16()
        y.backward(dy.double())
        flat, wd, wf, offs, wdq, wfq = _pack(K, [conv_w_storage(w.float())], frag=True)
        yg = K.conv_gt(nh(x), wfq, kh=3, kw=3, stride=2, pad=1, transposed=False, K=Ci, Nc=Co, out_hw=(h, h), bias=b.to(DEV))
        y16 = K.conv_gt(nh(x), wfq, kh=3, kw=3, stride=2, pad=1, transposed=False, K=Ci, Nc=Co, out_hw=(h, h), bias=b.to(DEV),
                        out_dtype=torch.bfloat16)
        yd, yd16 = K.conv_gt(nh(x), wfq, kh=3, kw=3, stride=2, pad=1, transposed=False, K=Ci, Nc=Co, out_hw=(h, h), bias=b.to(DEV), want16=True)
        assert torch.equal(yd, yg) and torch.equal(yd16, yg.bfloat16())          # the bf16 copy from the same epilogue
        dxg = K.conv_gt(nh(dy), wdq, kh=3, kw=3, stride=2, pad=1, transposed=True, K=Co, Nc=Ci, out_hw=(2 * h, 2 * h))
        dx2 = K.conv_gt(nh(dy), wdq, kh=3, kw=3, stride=2, pad=1, transposed=True, K=Co, Nc=Ci, out_hw=(2 * h, 2 * h), out=dxg.clone(),
                        accumulate=True)
        torch.cuda.synchronize()
        assert yg is not None and yg.dtype == torch.float32 and rel_err(from_nhwc(yg), y) < 2e-5
        assert y16.dtype == torch.bfloat16 and rel_err(from_nhwc(y16.float()), y) < 4e-3
        assert rel_err(from_nhwc(dxg), xd.grad) < 2e-5 and rel_err(from_nhwc(dx2), 2 * xd.grad) < 2e-5
        # Upsample forward + its data gradient
        x = torch.randn(N, Ci, h, h, generator=g).bfloat16()
        w = (torch.randn(Ci, Co, 4, 4, generator=g) / math.sqrt(Ci * 4)).bfloat16()
        xd = x.double().requires_grad_(True)
        y = F.conv_transpose2d(xd, w.double(), b.double(), stride=2, padding=1)
        dy = torch.randn(y.shape, generator=g).bfloat16()
        y.backward(dy.double())
        flat, wd, wf, offs, wdq, wfq = _pack(K, [conv_w_storage(w.float(), transposed=True)], frag=True)
        yg = K.conv_gt(nh(x), wfq, kh=4, kw=4, stride=2, pad=1, transposed=True, K=Ci, Nc=Co, out_hw=(2 * h, 2 * h), bias=b.to(DEV))
        dxg = K.conv_gt(nh(dy), wdq, kh=4, kw=4, stride=2, pad=1, transposed=False, K=Co, Nc=Ci, out_hw=(h, h))
        torch.cuda.synchronize()
        assert rel_err(from_nhwc(yg), y) < 2e-5 and rel_err(from_nhwc(dxg), xd.grad) < 2e-5
        syms = {q[0] for q in K.PROBE if q[0].startswith(("conv", "igemm"))}
        assert syms and all(sy.startswith("conv_gt_kernel<") for sy in syms), syms
    finally:
        K.PROBE = None
    # refused (-> None, the caller falls back): fp32 input, channels not a multiple of 64, odd grids
    assert K.conv_gt(torch.zeros(2, 8, 8, 64, device=DEV), wfq, kh=3, kw=3, stride=2, pad=1, transposed=False, K=64, Nc=64, out_hw=(4, 4)) is None
    assert K.conv_gt(torch.zeros(2, 8, 8, 32, device=DEV).bfloat16(), wfq, kh=3, kw=3, stride=2, pad=1, transposed=False, K=32, Nc=64,
                     out_hw=(4, 4)) is None
    assert K.conv_gt(torch.zeros(4, 14, 14, 64, device=DEV).bfloat16(), wfq, kh=3, kw=3, stride=2, pad=1, transposed=False, K=64, Nc=64,
                     out_hw=(7, 7)) is None


@pytest.mark.parametrize("cfg", [dict(N=4, h=16, C=128), dict(N=8, h=8, C=256), dict(N=2, h=16, C=64, Co=192)])
def test_stride2_family_tap_gather_kernel_fp32_mode(K, cfg):
    """The exact-fp32 instantiation of mi_conv_gt (Unet.compute_mode = "fp32": v_mfma_f32_32x32x2_f32, fp32 tensors, weights from
    mi_pack_weights_f32frag): the four stride-2 layer kinds against fp64 on the same fp32 operands, <= 3e-6."""
    g = torch.Generator().manual_seed(101)
    N, h, Ci = cfg["N"], cfg["h"], cfg["C"]
    Co = cfg.get("Co", Ci)
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731

    def frag32(ws):
        n = (ws.numel() + 63) // 64 * 64
        flat = torch.zeros(n, device=DEV); flat[:ws.numel()] = ws.reshape(-1)
        table, nent, tiles = K.pack_table([(0, ws.shape[0] * ws.shape[1], ws.shape[2], ws.shape[3])], DEV)
        wdq32, wfq32 = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        K.pack_weights_f32frag(table, nent, tiles, flat, wdq32, wfq32)
        return wdq32, wfq32
    x = torch.randn(N, Ci, 2 * h, 2 * h, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(Ci * 9)
    b = torch.randn(Co, generator=g)
    xd = x.double().requires_grad_(True)
    y = F.conv2d(xd, w.double(), b.double(), stride=2, padding=1)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.double())
    wdq32, wfq32 = frag32(conv_w_storage(w))
    yg = K.conv_gt(nh(x), wfq32, kh=3, kw=3, stride=2, pad=1, transposed=False, K=Ci, Nc=Co, out_hw=(h, h), bias=b.to(DEV), mode=K.MODE_FP32)
    dxg = K.conv_gt(nh(dy), wdq32, kh=3, kw=3, stride=2, pad=1, transposed=True, K=Co, Nc=Ci, out_hw=(2 * h, 2 * h), mode=K.MODE_FP32)
    torch.cuda.synchronize()
    assert yg is not None and dxg is not None
    assert rel_err(from_nhwc(yg), y) < 3e-6 and rel_err(from_nhwc(dxg), xd.grad) < 3e-6
    x = torch.randn(N, Ci, h, h, generator=g)
    w = torch.randn(Ci, Co, 4, 4, generator=g) / math.sqrt(Ci * 4)
    xd = x.double().requires_grad_(True)
    y = F.conv_transpose2d(xd, w.double(), b.double(), stride=2, padding=1)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.double())
    wdq32, wfq32 = frag32(conv_w_storage(w, transposed=True))
    yg = K.conv_gt(nh(x), wfq32, kh=4, kw=4, stride=2, pad=1, transposed=True, K=Ci, Nc=Co, out_hw=(2 * h, 2 * h), bias=b.to(DEV), mode=K.MODE_FP32)
    dxg = K.conv_gt(nh(dy), wdq32, kh=4, kw=4, stride=2, pad=1, transposed=False, K=Co, Nc=Ci, out_hw=(h, h), mode=K.MODE_FP32)
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(yg), y) < 3e-6 and rel_err(from_nhwc(dxg), xd.grad) < 3e-6


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("C", [32, 128])
def test_conv_transpose_all(K, mode, C):
    """ConvTranspose2d(C, C, 4, 2, 1) (ddpm.py:70): forward, dgrad, wgrad."""
    g = torch.Generator().manual_seed(5)
    N, H = 2, 8
    x = torch.randn(N, C, H, H, generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(C, C, 4, 4, generator=g, dtype=torch.float64) / math.sqrt(C * 4)).requires_grad_(True)
    b = torch.randn(C, generator=g, dtype=torch.float64)
    y = F.conv_transpose2d(x, w, b, stride=2, padding=1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    ws = conv_w_storage(w.detach(), transposed=True)
    xg, dyg = to_nhwc_gpu(x.detach().float()), to_nhwc_gpu(dy.float())
    yg = K.conv_igemm(xg, ws, kh=4, kw=4, stride=2, pad=1, transposed=True, w_kn=True, K=C, Nc=C, out_hw=(2 * H, 2 * H),
                      mode=mode, bias=b.float().to(DEV))
    dx = K.conv_igemm(dyg, ws, kh=4, kw=4, stride=2, pad=1, transposed=False, w_kn=False, K=C, Nc=C, out_hw=(H, H), mode=mode)
    dW = torch.zeros(16 * C * C, device=DEV)
    K.conv_wgrad(xg, dyg, dW, kh=4, kw=4, stride=2, pad=1, gather_i=False, Ci=C, Cj=C, grid_g=(2 * H, 2 * H),
                 grid_d=(H, H), mode=mode)
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(yg), y) < TOL[mode]
    assert rel_err(from_nhwc(dx), x.grad) < TOL[mode]
    assert rel_err(w_from_storage(dW.view(4, 4, C, C), transposed=True), w.grad) < TOL[mode]


def test_wgrad_two_sources(K):
    g = torch.Generator().manual_seed(6)
    N, H, C1, C2, Co = 2, 8, 32, 16, 24
    x = torch.randn(N, C1 + C2, H, H, generator=g, dtype=torch.float64)
    w = torch.zeros(Co, C1 + C2, 3, 3, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(N, Co, H, H, generator=g, dtype=torch.float64)
    F.conv2d(x, w, None, padding=1).backward(dy)
    dW = torch.zeros(9 * (C1 + C2) * Co, device=DEV)
    K.conv_wgrad(to_nhwc_gpu(x[:, :C1].float()), to_nhwc_gpu(dy.float()), dW, kh=3, kw=3, stride=1, pad=1, gather_i=True,
                 Ci=C1 + C2, Cj=Co, grid_g=(H, H), grid_d=(H, H), mode=0, P2=to_nhwc_gpu(x[:, C1:].float()))
    torch.cuda.synchronize()
    assert rel_err(w_from_storage(dW.view(3, 3, C1 + C2, Co)), w.grad) < 2e-5


def test_linear_via_igemm(K):
    """nn.Linear (ddpm.py:127,190-192) as a 1x1 'conv' over a 1x1 image, weights [out,in]."""
    g = torch.Generator().manual_seed(7)
    B, I, O = 6, 32, 80
    x = torch.randn(B, I, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(O, I, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(O, generator=g, dtype=torch.float64)
    y = F.linear(x, w, b)
    dy = torch.randn(B, O, generator=g, dtype=torch.float64)
    y.backward(dy)
    xg, wg, dyg = x.detach().float().to(DEV), w.detach().float().to(DEV), dy.float().to(DEV)
    yg = K.conv_igemm(xg.view(B, 1, 1, I), wg, kh=1, kw=1, stride=1, pad=0, transposed=False, w_kn=False, K=I, Nc=O,
                      out_hw=(1, 1), mode=0, bias=b.float().to(DEV)).view(B, O)
    dxg = K.conv_igemm(dyg.view(B, 1, 1, O), wg, kh=1, kw=1, stride=1, pad=0, transposed=False, w_kn=True, K=O, Nc=I,
                       out_hw=(1, 1), mode=0).view(B, I)
    dW = torch.zeros(O * I, device=DEV)
    K.conv_wgrad(dyg.view(B, 1, 1, O), xg.view(B, 1, 1, I), dW, kh=1, kw=1, stride=1, pad=0, gather_i=True, Ci=O, Cj=I,
                 grid_g=(1, 1), grid_d=(1, 1), mode=0)
    torch.cuda.synchronize()
    assert rel_err(yg, y) < 2e-5 and rel_err(dxg, x.grad) < 2e-5 and rel_err(dW.view(O, I), w.grad) < 2e-5


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("cfg", [(16, 32, 32, 128, 128), (8, 16, 16, 128, 256), (16, 8, 8, 256, 512), (3, 32, 32, 64, 160), (8, 64, 64, 64, 64)])
def test_conv_epilogue_groupnorm_sums(K, cfg, storage):
    """mi_conv3x3_bf16w_io_gnsums + mi_gn_coef_from_sums: the next GroupNorm's statistics and coefficients from the conv's epilogue
    equal what mi_gn_stats_coef computes with a pass over the stored tensor (fp32 summation order aside), and the conv's output is
    unchanged (bitwise)."""
    N, H, W, Ci, Co = cfg
    g = torch.Generator().manual_seed(67)
    dt = torch.float32 if storage == "fp32" else torch.bfloat16
    x = torch.randn(N, H, W, Ci, generator=g).to(DEV).to(dt)
    wsh = (torch.randn(9 * Co * Ci, generator=g) / math.sqrt(9 * Ci)).to(DEV).bfloat16()
    bias = torch.randn(Co, generator=g).to(DEV)
    gamma, beta = (torch.rand(Co, generator=g) + 0.5).to(DEV), torch.randn(Co, generator=g).to(DEV)
    temb = torch.randn(N, Co, generator=g).to(DEV)
    auto, K.CONV_AUTO = K.CONV_AUTO, False          # the same (halo) kernel with and without the sums: bitwise comparison below
    try:
        y0 = K.conv3x3_bf16w(x, wsh, K=Ci, Nc=Co, flip=False, bias=bias, out_dtype=dt)
    finally:
        K.CONV_AUTO = auto
    sums = K.gn_sums_buffer(N, Co, DEV)
    y1 = K.conv3x3_bf16w(x, wsh, K=Ci, Nc=Co, flip=False, bias=bias, out_dtype=dt, gn_sums=sums)
    assert torch.equal(y0, y1)
    if (Co // 8) % 16:                              # 160 / 8 = 20 channels per group: slabs do not tile the groups -> refused
        with pytest.raises(RuntimeError):
            K.gn_coef_from_sums(sums, N, H * W, gamma, beta, temb=temb)
        return
    st1, cf1 = K.gn_coef_from_sums(sums, N, H * W, gamma, beta, temb=temb)
    st0, cf0 = K.gn_stats_coef(y0, gamma, beta, temb=temb)
    torch.cuda.synchronize()
    assert float((st1[..., 0] - st0[..., 0]).abs().max()) < 2e-5
    assert float(((st1[..., 1] - st0[..., 1]) / st0[..., 1]).abs().max()) < 2e-5
    assert float((cf1 - cf0).abs().max()) < 1e-4 * float(cf0.abs().max())


@pytest.mark.parametrize("cfg", [(16, 32, 32, 128, 128, 1), (8, 16, 16, 256, 256, 1), (4, 8, 8, 512, 512, 1), (4, 32, 32, 128, 128, 3),
                                 (3, 32, 32, 64, 160, 1)])
def test_conv_dual_output(K, cfg):
    """mi_conv3x3_bf16w_io_dual (to_out + Residual, reference ddpm.py:45,152): the fp32 output is the one the plain entry point
    writes (bitwise) and the second output is that tensor rounded to bf16 (bitwise)."""
    N, H, W, Ci, Co, ks = cfg
    g = torch.Generator().manual_seed(71)
    x = torch.randn(N, H, W, Ci, generator=g).to(DEV).bfloat16()
    wsh = (torch.randn(ks * ks * Co * Ci, generator=g) / math.sqrt(ks * ks * Ci)).to(DEV).bfloat16()
    bias = torch.randn(Co, generator=g).to(DEV)
    res = torch.randn(N, H, W, Co, generator=g).to(DEV)
    auto, K.CONV_AUTO = K.CONV_AUTO, False          # the dual-output entry point belongs to the halo kernel: compare with that kernel
    try:
        y0 = K.conv3x3_bf16w(x, wsh, K=Ci, Nc=Co, flip=False, ksize=ks, bias=bias, residual=res)
    finally:
        K.CONV_AUTO = auto
    y1, y16 = K.conv3x3_bf16w(x, wsh, K=Ci, Nc=Co, flip=False, ksize=ks, bias=bias, residual=res, want16=True)
    torch.cuda.synchronize()
    assert y16.dtype == torch.bfloat16 and y16.shape == y0.shape
    assert torch.equal(y0, y1) and torch.equal(y16, y0.bfloat16())


def _mish64(x):
    return x * torch.tanh(F.softplus(x))


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("cfg", [(16, 32, 32, 128, 128), (8, 16, 16, 256, 256), (16, 8, 8, 512, 512), (8, 16, 16, 128, 256),
                                 (2, 64, 64, 64, 64), (3, 32, 32, 128, 96)])
def test_fused_gn_mish_conv3x3(K, cfg, storage):
    """BASELINE.json's named kernel: GroupNorm-apply + Mish (+ time bias) folded into the 3x3 conv's input staging
    (mi_gn_stats_coef + mi_conv3x3_gn_mish; reference ddpm.py:112-120,139-140 Block -> time bias -> Block's conv) against
    (a) an fp64 evaluation of GroupNorm -> Mish -> + temb -> Conv2d on the same stored c1 and bf16-rounded weights, and
    (b) the two-pass path of this library (gn_mish_fwd, then the plain conv): the fused kernel must agree with it to bf16 rounding."""
    N, H, W, Cc, Co = cfg
    g = torch.Generator().manual_seed(61)
    dt = torch.bfloat16 if storage == "bf16" else torch.float32
    c1 = (torch.randn(N, Cc, H, W, generator=g) * 1.7 + 0.3).to(dt)
    gamma, beta = torch.randn(Cc, generator=g) * 0.5 + 1, torch.randn(Cc, generator=g) * 0.2
    temb = torch.randn(N, Cc, generator=g) * 0.3
    w = torch.randn(Co, Cc, 3, 3, generator=g) / math.sqrt(9 * Cc)
    bias = torch.randn(Co, generator=g) * 0.1
    wq = w.bfloat16()
    x64 = c1.double()
    hn = F.group_norm(x64, 8, gamma.double(), beta.double(), 1e-5)
    h = _mish64(hn) + temb.double()[:, :, None, None]
    ref = F.conv2d(h, wq.double(), bias.double(), padding=1)
    xg = c1.permute(0, 2, 3, 1).contiguous().to(DEV)
    wsh = wq.permute(2, 3, 0, 1).contiguous().to(DEV).reshape(-1)            # [ky][kx][Co][Ci]
    assert K.conv3x3_gn_mish_supported(N, H, W, Cc, Co)
    stats, coef = K.gn_stats_coef(xg, gamma.to(DEV), beta.to(DEV), temb=temb.to(DEV))
    y = K.conv3x3_gn_mish(xg, coef, wsh, K=Cc, Nc=Co, bias=bias.to(DEV))
    assert y is not None and y.dtype == dt
    h1, st2 = K.gn_mish_fwd(xg, gamma.to(DEV), beta.to(DEV), temb=temb.to(DEV), out_dtype=dt)
    y2 = K.conv3x3_bf16w(h1, wsh, K=Cc, Nc=Co, flip=False, bias=bias.to(DEV), out_dtype=dt)
    torch.cuda.synchronize()
    assert torch.allclose(stats, st2, rtol=1e-6, atol=1e-7)                  # same statistics kernel
    mean = x64.view(N, 8, -1).mean(-1)
    assert torch.allclose(stats[..., 0].cpu().double(), mean, atol=2e-5)
    got = y.float().cpu().permute(0, 3, 1, 2).double()
    two = y2.float().cpu().permute(0, 3, 1, 2).double()
    # h is rounded to bf16 before the MFMA in both paths (2^-9 relative per element, averaged over 9*C products)
    assert rel_err(got, ref) < (4e-3 if storage == "fp32" else 6e-3)
    assert rel_err(got, two) < (2e-3 if storage == "fp32" else 5e-3)
    if storage == "fp32":
        # the two paths round the same h values (the two-pass path stores h in fp32 and rounds it in the conv's staging; only the
        # reciprocal-based Mish of the fused path differs): nearly identical
        assert rel_err(got, two) < 1e-3


@pytest.mark.parametrize("cfg", [(2, 8, 8, 8), (2, 8, 8, 16), (3, 16, 16, 32), (2, 32, 32, 128), (2, 8, 8, 512),
                                 (2, 7, 7, 64), (1, 64, 64, 64), (2, 16, 16, 1024)])
def test_gn_mish_fwd_bwd(K, cfg):
    """Block's GroupNorm(8)+Mish (ddpm.py:116), + time bias (ddpm.py:140), + residual (ddpm.py:143)."""
    N, H, W, C = cfg
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    gamma = (torch.randn(C, generator=g, dtype=torch.float64) + 1).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_(True)
    temb = torch.randn(N, C, generator=g, dtype=torch.float64).requires_grad_(True)
    res = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    y = _mish64(F.group_norm(x, 8, gamma, beta, eps=1e-5)) + temb[:, :, None, None] + res
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    xg = to_nhwc_gpu(x.detach().float())
    ga, be = gamma.detach().float().to(DEV), beta.detach().float().to(DEV)
    yg, st = K.gn_mish_fwd(xg, ga, be, temb=temb.detach().float().to(DEV), residual=to_nhwc_gpu(res.float()))
    dga, dbe, dbias = (torch.zeros(C, device=DEV) for _ in range(3))
    dtemb = torch.zeros(N, C, device=DEV)
    dx = K.gn_mish_bwd(xg, st, ga, be, to_nhwc_gpu(dy.float()), dgamma=dga, dbeta=dbe, dtemb=dtemb, dbias=dbias)
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(yg), y) < 1e-5
    assert rel_err(from_nhwc(dx), x.grad) < 5e-5
    assert rel_err(dga, gamma.grad) < 5e-5 and rel_err(dbe, beta.grad) < 5e-5
    assert rel_err(dtemb, temb.grad) < 5e-5
    assert max_err(dbias, x.grad.sum((0, 2, 3))) < 1e-3 * float(x.grad.abs().sum((0, 2, 3)).max())


def test_mish_edges(K, golden_dir):
    """Mish KATs captured from the reference incl. the softplus threshold at 20 (ddpm.py:62-64)."""
    import os
    g = dict(np.load(os.path.join(golden_dir, "leaf_kats.npz")))
    x = torch.from_numpy(g["mish_x"])
    y = K.mish_fwd(x.to(DEV))
    ref = torch.from_numpy(g["mish_y"])
    assert torch.allclose(y.cpu(), ref, rtol=2e-6, atol=1e-12)
    xd = x.double().requires_grad_(True)
    _mish64(xd).sum().backward()
    dx = K.mish_bwd(x.to(DEV), torch.ones_like(x).to(DEV))
    assert torch.allclose(dx.cpu().double(), xd.grad, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("cfg", [(2, 4, 4, 16), (2, 8, 8, 128), (3, 7, 7, 256), (2, 8, 8, 512), (1, 4, 4, 1024)])
def test_chan_layernorm(K, cfg):
    """LayerNorm over channels with eps added to the std (ddpm.py:92-95)."""
    N, H, W, C = cfg
    g = torch.Generator().manual_seed(13)
    x = (torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 1.7 - 0.3).requires_grad_(True)
    gg = (torch.randn(1, C, 1, 1, generator=g, dtype=torch.float64) + 1).requires_grad_(True)
    bb = torch.randn(1, C, 1, 1, generator=g, dtype=torch.float64).requires_grad_(True)
    std = torch.var(x, dim=1, unbiased=False, keepdim=True).sqrt()
    y = (x - x.mean(1, keepdim=True)) / (std + 1e-5) * gg + bb
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    xg = to_nhwc_gpu(x.detach().float())
    g_, b_ = gg.detach().float().reshape(-1).to(DEV), bb.detach().float().reshape(-1).to(DEV)
    yg = K.chan_layernorm_fwd(xg, g_, b_)
    dx = torch.empty_like(xg.contiguous())
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    K.chan_layernorm_bwd(xg, g_, to_nhwc_gpu(dy.float()), dx, False, dg, db)
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(yg), y) < 1e-5
    assert rel_err(from_nhwc(dx), x.grad) < 5e-5
    assert rel_err(dg, gg.grad.reshape(-1)) < 5e-5 and rel_err(db, bb.grad.reshape(-1)) < 5e-5
    # the parameter gradients as per-workgroup partial rows + the batched row sum (what Unet's backward uses): dx bitwise the same,
    # dg / db added onto what the destination already holds
    wq = K.WgradQueue()
    dx2 = torch.empty_like(dx)
    dg2, db2 = torch.full((C,), 0.5, device=DEV), torch.full((C,), -2.0, device=DEV)
    K.chan_layernorm_bwd(xg, g_, to_nhwc_gpu(dy.float()), dx2, False, dg2, db2, defer=wq)
    assert wq.flushed == 0 and wq.pushed == 2
    wq.flush()
    torch.cuda.synchronize()
    assert wq.flushed == 2 and torch.equal(dx2, dx)
    assert rel_err(dg2 - 0.5, gg.grad.reshape(-1)) < 5e-5 and rel_err(db2 + 2.0, bb.grad.reshape(-1)) < 5e-5


@pytest.mark.parametrize("rows,cols,ld", [(1, 1, 1), (3, 5, 7), (64, 64, 64), (65, 130, 192), (512, 1024, 1024), (700, 96, 200)])
def test_rowsum_batch(K, rows, cols, ld):
    """mi_rowsum_batch: dst[c] += sum_r src[r * ld + c] for several items in one launch (ragged rows / columns, row stride > cols,
    more than MI_ROWSUM_MAX items -> several launches)."""
    g = torch.Generator().manual_seed(rows * 131 + cols)
    wq = K.WgradQueue()
    items = []
    for i in range(19 if rows < 100 else 3):
        src = torch.randn(rows + i, ld, generator=g).to(DEV)
        dst = torch.randn(cols, generator=g).to(DEV)
        ref = dst.double() + src[:, :cols].double().sum(0)
        wq.push_rowsum(src, rows + i, cols, ld, dst)
        items.append((src, dst, ref))
    wq.flush(kinds=(4,))
    torch.cuda.synchronize()
    for src, dst, ref in items:
        assert float((dst.double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("cfg", [(2, 4, 4), (2, 8, 8), (3, 7, 7), (2, 32, 32), (1, 64, 64), (2, 24, 24), (16, 16, 16)])
def test_linear_attention_core(K, cfg):
    """softmax over pixels of k, ctx = k v^T, out = ctx^T q (ddpm.py:157-165).  Images with >= 256 pixels per (batch, head) run as
    pixel slices when there are fewer than two workgroups per CU otherwise (three launches forward, two backward, partial results
    combined in a fixed order): 32x32 -> 8 slices, 64x64 -> 32, 24x24 -> 4 ragged ones, 16 x 16x16 -> 2; bitwise reproducible."""
    N, H, W = cfg
    n, heads = H * W, 4
    g = torch.Generator().manual_seed(17)
    qkv = (torch.randn(N, 384, H, W, generator=g, dtype=torch.float64) * 1.5).requires_grad_(True)
    q, k, v = qkv.reshape(N, 3, heads, 32, n).unbind(1)
    ks = k.softmax(dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", ks, v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(N, 128, H, W)
    dout = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(dout)
    qg = to_nhwc_gpu(qkv.detach().float()).contiguous()
    og, cg, sg = K.linattn_fwd(qg, heads)
    dq = K.linattn_bwd(qg, cg, sg, to_nhwc_gpu(dout.float()).contiguous(), heads)
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(og), out) < 1e-5
    assert rel_err(cg, ctx) < 1e-5
    assert rel_err(from_nhwc(dq), qkv.grad) < 5e-5
    og2, cg2, sg2 = K.linattn_fwd(qg, heads)
    dq2 = K.linattn_bwd(qg, cg2, sg2, to_nhwc_gpu(dout.float()).contiguous(), heads)
    assert torch.equal(og, og2) and torch.equal(cg, cg2) and torch.equal(dq, dq2)
    assert (K.load_library().mi_linattn_workspace(N, n, heads) > 0) == (n >= 256 and N * heads < 256)


def test_time_embed_and_layouts(K, golden_dir):
    import os
    g = dict(np.load(os.path.join(golden_dir, "leaf_kats.npz")))
    for d in (8, 32, 128):
        t = torch.from_numpy(g[f"posemb{d}_t"]).to(DEV)
        y = K.time_embed(t, d).cpu()
        assert torch.allclose(y, torch.from_numpy(g[f"posemb{d}_y"]), atol=2e-4, rtol=0)   # |arg| up to 999 rad
    x = torch.randn(3, 3, 5, 7)
    xh = K.nchw_to_nhwc(x.to(DEV))
    assert xh.shape == (3, 5, 7, 3) and xh.stride(2) == 4
    assert torch.equal(K.nhwc_to_nchw(xh).cpu(), x)


def test_diffusion_elementwise(K, golden_dir):
    """q_sample (ddpm.py:441-444), L1/L2 loss (:453-456), posterior update (:359-397), Adam."""
    from oracle import ddpm_oracle as O
    tab = O.schedule_tables(1000)
    tg = {k: v.to(DEV) for k, v in tab.items()}
    g = torch.Generator().manual_seed(19)
    B = 5
    x0 = torch.rand(B, 3, 8, 8, generator=g) * 2 - 1
    noise = torch.randn(B, 3, 8, 8, generator=g)
    t = torch.tensor([0, 1, 500, 998, 999])
    xt_ref = O.q_sample(tab, x0, t, noise)
    xt_nhwc, xt_nchw = K.q_sample(x0.to(DEV), noise.to(DEV), t.to(DEV), tg["sqrt_alphas_cumprod"],
                                  tg["sqrt_one_minus_alphas_cumprod"], want_nchw=True)
    assert torch.allclose(xt_nchw.cpu(), xt_ref, atol=1e-6) and torch.allclose(from_nhwc(xt_nhwc), xt_ref, atol=1e-6)
    pred = torch.randn(B, 3, 8, 8, generator=g)
    pred[0, 0, 0, 0] = noise[0, 0, 0, 0]                      # a tie: sign(0) = 0
    for lt, name in ((0, "l1"), (1, "l2")):
        pr = pred.clone().requires_grad_(True)
        ref = (noise - pr).abs().mean() if lt == 0 else F.mse_loss(noise, pr)
        ref.backward()
        loss, dpred = K.eps_loss(to_nhwc_gpu(pred), noise.to(DEV), lt)
        assert abs(float(loss) - float(ref)) < 1e-6
        assert torch.allclose(from_nhwc(dpred), pr.grad, atol=1e-9)
    z = torch.randn(B, 3, 8, 8, generator=g)
    xp_ref = O.p_sample_update(tab, xt_ref, t, pred, z)
    xp, xp_nhwc = K.p_sample_update(xt_ref.to(DEV), to_nhwc_gpu(pred), z.to(DEV), t.to(DEV), tg)
    assert torch.allclose(xp.cpu(), xp_ref, atol=2e-5, rtol=1e-5)
    assert torch.allclose(from_nhwc(xp_nhwc), xp_ref, atol=2e-5, rtol=1e-5)
    # the graph sampler's form: the image updated in place, the NHWC copy into a caller-owned buffer whose padding channel stays zero
    x_io = xt_ref.to(DEV).clone()
    nh = torch.zeros(B, 8, 8, 4, device=DEV)
    got, got_nhwc = K.p_sample_update(x_io, to_nhwc_gpu(pred), z.to(DEV), t.to(DEV), tg, out=x_io, out_nhwc=nh)
    assert got.data_ptr() == x_io.data_ptr() and torch.equal(x_io, xp)
    assert got_nhwc.data_ptr() == nh.data_ptr() and torch.equal(nh[..., :3], xp_nhwc) and float(nh[..., 3].abs().max()) == 0.0
    # Adam: 3 steps against torch.optim.Adam
    p = torch.randn(1003, generator=g)
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=1e-3, betas=(0.9, 0.999))
    pg, m, v = torch.zeros(1004, device=DEV), torch.zeros(1004, device=DEV), torch.zeros(1004, device=DEV)
    pg[:1003] = p.to(DEV)
    for step in range(1, 4):
        gr = torch.randn(1003, generator=g)
        pr.grad = gr.clone(); opt.step()
        gg = torch.zeros(1004, device=DEV); gg[:1003] = gr.to(DEV)
        K.adam_step(pg[:1003], gg[:1003], m[:1003], v[:1003], 1e-3, 0.9, 0.999, 1e-8, step)
    assert torch.allclose(pg[:1003].cpu(), pr.detach(), atol=1e-6)


def _pack(K, w_storage_list, frag=False):
    """fp32 tap-major weights -> (flat master, bf16 wd, bf16 wf, offsets) through mi_pack_weights_bf16; frag: -> (..., wdq, wfq), the
    MFMA-fragment-order copies as well."""
    offs, off = [], 0
    for w in w_storage_list:
        offs.append(off); off += (w.numel() + 63) // 64 * 64
    flat = torch.zeros(off, device=DEV)
    ents = []
    for w, o in zip(w_storage_list, offs):
        kh, kw, ci, co = w.shape
        flat[o:o + w.numel()] = w.reshape(-1)
        ents.append((o, kh * kw, ci, co))
    table, nent, tile = K.pack_table(ents, DEV)
    wd = torch.zeros(off, device=DEV, dtype=torch.bfloat16)
    wf = torch.zeros(off, device=DEV, dtype=torch.bfloat16)
    if not frag:
        K.pack_weights_bf16(table, nent, tile, flat, wd, wf)
        return flat, wd, wf, offs
    wdq, wfq = torch.zeros_like(wd), torch.zeros_like(wf)
    K.pack_weights_bf16(table, nent, tile, flat, wd, wf, wdq, wfq)
    return flat, wd, wf, offs, wdq, wfq


def test_pack_weights_bf16(K):
    g = torch.Generator().manual_seed(23)
    ws = [torch.randn(3, 3, 40, 24, generator=g).to(DEV), torch.randn(1, 1, 16, 3, generator=g).to(DEV),
          torch.randn(4, 4, 32, 32, generator=g).to(DEV), torch.randn(3, 3, 3, 128, generator=g).to(DEV),
          torch.randn(3, 3, 192, 100, generator=g).to(DEV), torch.randn(1, 1, 128, 384, generator=g).to(DEV)]
    flat, wd, wf, offs = _pack(K, ws)
    torch.cuda.synchronize()
    for w, o in zip(ws, offs):
        n = w.numel()
        assert torch.equal(wd[o:o + n].view(w.shape), w.to(torch.bfloat16))
        assert torch.equal(wf[o:o + n].view(w.shape[0], w.shape[1], w.shape[3], w.shape[2]),
                           w.permute(0, 1, 3, 2).contiguous().to(torch.bfloat16))


@pytest.fixture
def pw_always(K):
    """Route every supported layer to the private-weight-stream kernel (the default takes it only from ~one tile per CU up) and
    record the launches (functional.PROBE) so that a test can assert which kernel it exercised."""
    was, was_on, K.PW_MIN_TILES, K.USE_CONV_PW, K.PROBE = K.PW_MIN_TILES, K.USE_CONV_PW, 0, True, []
    yield K.PROBE
    K.PW_MIN_TILES, K.USE_CONV_PW, K.PROBE = was, was_on, None


@pytest.fixture(params=[128, 64])
def pw_tile(K, request):
    """Force conv_pw's pixel tile (mi_debug_conv_pw_tile): 128 = four MFMA blocks per wave, 64 = two (what small grids get)."""
    lib = K.load_library()
    lib.mi_debug_conv_pw_tile(request.param); K._QUERY_CACHE.clear()
    yield request.param
    lib.mi_debug_conv_pw_tile(0); K._QUERY_CACHE.clear()


def _conv_launches(probe):
    return [q[0] for q in probe if q[0].startswith("conv")]


def _frag_weights(K, w):
    """[Co][Ci][3][3] fp32 -> (plain bf16 [ky][kx][Co][Ci] flat, fragment-order forward operand) via the pack kernel."""
    flat, wd, wf, offs, wdq, wfq = _pack(K, [conv_w_storage(w.double())], frag=True)
    return wf, wfq


@pytest.fixture
def pw_tile256(K):
    """Force conv_pw's 256-pixel tiles (round 5: eight MFMA blocks per wave, one workgroup per CU; 32- and 16-pixel-wide images)."""
    lib = K.load_library()
    lib.mi_debug_conv_pw_tile(256); K._QUERY_CACHE.clear()
    yield 256
    lib.mi_debug_conv_pw_tile(0); K._QUERY_CACHE.clear()


@pytest.mark.parametrize("out16", [True, False])
@pytest.mark.parametrize("cfg", [(16, 32, 32, 128, 128), (8, 16, 16, 256, 256), (4, 8, 8, 512, 512), (16, 16, 16, 128, 384)])
def test_conv_pw_epilogue_groupnorm_sums(K, cfg, out16, pw_always, pw_tile):
    _pw_gnsums_case(K, cfg, out16, pw_always, pw_tile)


@pytest.mark.parametrize("out16", [True, False])
@pytest.mark.parametrize("cfg", [(16, 32, 32, 128, 128), (8, 16, 16, 256, 256), (3, 16, 16, 128, 384)])
def test_conv_pw_epilogue_groupnorm_sums_tile256(K, cfg, out16, pw_always, pw_tile256):
    _pw_gnsums_case(K, cfg, out16, pw_always, pw_tile256)


def _pw_gnsums_case(K, cfg, out16, pw_always, pw_tile):
    """mi_conv3x3_pw_gnsums + mi_gn_coef_from_sums: the next GroupNorm's statistics and coefficients out of the conv's row-contiguous
    epilogue (one image per tile at 32 / 16 pixels width, TWO at 8x8) equal what mi_gn_stats_coef computes with a pass over the
    stored tensor, and the conv's output is the plain entry point's (bitwise)."""
    N, H, W, Ci, Co = cfg
    g = torch.Generator().manual_seed(73)
    x = torch.randn(N, H, W, Ci, generator=g).to(DEV).bfloat16()
    w = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)
    wf, wfq = _frag_weights(K, w)
    bias = torch.randn(Co, generator=g).to(DEV)
    gamma, beta = (torch.rand(Co, generator=g) + 0.5).to(DEV), torch.randn(Co, generator=g).to(DEV)
    temb = torch.randn(N, Co, generator=g).to(DEV)
    dt = torch.bfloat16 if out16 else torch.float32
    y0 = K.conv3x3_bf16w(x, wf, K=Ci, Nc=Co, flip=False, bias=bias, out_dtype=dt, wq=wfq)
    sums = K.gn_sums_buffer(N, Co, DEV)
    y1 = K.conv3x3_bf16w(x, wf, K=Ci, Nc=Co, flip=False, bias=bias, out_dtype=dt, gn_sums=sums, wq=wfq)
    assert torch.equal(y0, y1)
    ls = _conv_launches(pw_always)
    o16 = "true" if out16 else "false"
    assert ls == [f"conv_pw_kernel<{o16}, 0, 0, {pw_tile}>", f"conv_pw_kernel<{o16}, 1, 0, {pw_tile}>"], ls
    # the raw sums: per sample and 16-channel slab, of the STORED values
    yd = y0.double().view(N, H * W, Co // 16, 16)
    want = torch.stack([yd.sum((1, 3)), (yd * yd).sum((1, 3))], dim=-1)             # [N][Co/16][2]
    got = K.gn_sums_decode(sums).view(N, Co // 16, 2)
    assert float((got - want).abs().max()) < 2e-5 * float(want.abs().max())
    if (Co // 8) % 16 or (Co // 8) & (Co // 8 - 1):
        return                                      # (384 channels: 48 per group -- the GroupNorm kernels do not take it)
    st1, cf1 = K.gn_coef_from_sums(sums, N, H * W, gamma, beta, temb=temb)
    st0, cf0 = K.gn_stats_coef(y0, gamma, beta, temb=temb)
    torch.cuda.synchronize()
    assert float((st1[..., 0] - st0[..., 0]).abs().max()) < 2e-5
    assert float(((st1[..., 1] - st0[..., 1]) / st0[..., 1]).abs().max()) < 2e-5
    assert float((cf1 - cf0).abs().max()) < 1e-4 * float(cf0.abs().max())


@pytest.mark.parametrize("out16", [True, False])
@pytest.mark.parametrize("cfg", [(16, 32, 32, 128, 128), (8, 16, 16, 256, 256), (8, 16, 16, 128, 256), (3, 32, 32, 128, 96), (2, 32, 32, 64, 64),
                                 (2, 16, 16, 512, 128)])
def test_fused_gn_mish_conv3x3_pw(K, cfg, out16, pw_always, pw_tile):
    """BASELINE.json's named kernel on the private-weight-stream structure (mi_conv3x3_pw_gn_mish; reference ddpm.py:112-120,139-140
    Block -> time bias -> Block's conv): the transform is applied once per staged element, in place in LDS.  Against (a) an fp64
    evaluation of GroupNorm -> Mish -> + temb -> Conv2d on the same stored bf16 c1 and bf16-rounded weights and (b) the two-pass path
    (gn_mish_fwd writing h1 as bf16, then the plain conv): same rounding points, so the two agree to a bf16 ulp of h1 here and there.
    Image borders (zero padding must stay zero after the transform), one to eight chunks, a ragged channel tile; 128- and 64-pixel tiles."""
    N, H, W, Cc, Co = cfg
    g = torch.Generator().manual_seed(79)
    c1 = (torch.randn(N, Cc, H, W, generator=g) * 1.7 + 0.3).bfloat16()
    gamma, beta = torch.randn(Cc, generator=g) * 0.5 + 1, torch.randn(Cc, generator=g) * 0.2
    temb = torch.randn(N, Cc, generator=g) * 0.3 + 0.5          # a non-zero time bias: padding must NOT become mish(shift) + tb
    w = torch.randn(Co, Cc, 3, 3, generator=g) / math.sqrt(9 * Cc)
    bias = torch.randn(Co, generator=g) * 0.1
    Cop = (Co + 63) // 64 * 64
    wp = torch.zeros(Cop, Cc, 3, 3); wp[:Co] = w
    bp = torch.zeros(Cop); bp[:Co] = bias
    x64 = c1.double()
    hn = F.group_norm(x64, 8, gamma.double(), beta.double(), 1e-5)
    h = _mish64(hn) + temb.double()[:, :, None, None]
    ref = F.conv2d(h, w.bfloat16().double(), bias.double(), padding=1)
    xg = c1.permute(0, 2, 3, 1).contiguous().to(DEV)
    wf, wfq = _frag_weights(K, wp)
    dt = torch.bfloat16 if out16 else torch.float32
    stats, coef = K.gn_stats_coef(xg, gamma.to(DEV), beta.to(DEV), temb=temb.to(DEV))
    y = K.conv3x3_gn_mish(xg, coef, wf, K=Cc, Nc=Cop, bias=bp.to(DEV), out_dtype=dt, wq=wfq)
    assert y is not None and y.dtype == dt
    ls = _conv_launches(pw_always)
    assert ls[-1].startswith("conv_pw_kernel") and ls[-1].endswith(f", 2, 0, {pw_tile}>"), ls
    h1, _ = K.gn_mish_fwd(xg, gamma.to(DEV), beta.to(DEV), temb=temb.to(DEV), out_dtype=torch.bfloat16)
    y2 = K.conv3x3_bf16w(h1, wf, K=Cc, Nc=Cop, flip=False, bias=bp.to(DEV), out_dtype=dt, wq=wfq)
    torch.cuda.synchronize()
    got = y.float().cpu().permute(0, 3, 1, 2).double()[:, :Co]
    two = y2.float().cpu().permute(0, 3, 1, 2).double()[:, :Co]
    assert rel_err(got, ref) < 6e-3
    assert rel_err(got, two) < (5e-3 if out16 else 1.5e-3)
    assert not y[..., Co:].any()
    if (Cc // 8) % 16 == 0:
        # the variant that resolves the coefficients itself from the producer's sums (mi_conv3x3_pw_gn_mish_sums) does
        # mi_gn_coef_from_sums' arithmetic: bitwise the output of the coefficient-tensor variant fed by that kernel
        xd = xg.double().view(N, H * W, Cc // 16, 16)
        sums = K.gn_sums_encode(torch.stack([xd.sum((1, 3)), (xd * xd).sum((1, 3))], dim=-1))
        _, coef2 = K.gn_coef_from_sums(sums, N, H * W, gamma.to(DEV), beta.to(DEV), temb=temb.to(DEV))
        ya = K.conv3x3_gn_mish(xg, coef2, wf, K=Cc, Nc=Cop, bias=bp.to(DEV), out_dtype=dt, wq=wfq)
        yb = K.conv3x3_gn_mish(xg, None, wf, K=Cc, Nc=Cop, bias=bp.to(DEV), out_dtype=dt, wq=wfq,
                               gn=(sums, gamma.to(DEV), beta.to(DEV), temb.to(DEV), 8, 1e-5))
        ls = _conv_launches(pw_always)
        assert ls[-1].endswith(f", 3, 0, {pw_tile}>") and ls[-2].endswith(f", 2, 0, {pw_tile}>"), ls
        assert torch.equal(ya, yb)
        assert rel_err(yb.float().cpu().permute(0, 3, 1, 2).double()[:, :Co], ref) < 6e-3


@pytest.mark.parametrize("out16", [True, False])
@pytest.mark.parametrize("cfg", [(16, 32, 32, 128, 128), (8, 16, 16, 256, 256), (8, 16, 16, 128, 256), (3, 32, 32, 128, 96), (2, 32, 32, 64, 64),
                                 (2, 16, 16, 512, 128)])
def test_fused_gn_mish_conv3x3_pw_fp32_storage(K, cfg, out16, pw_always, pw_tile):
    """The named kernel for fp32-STORED activations on the private-weight-stream structure (mi_conv3x3_pw_x32_gn_mish[_sums], round 4):
    c1 is read as fp32, GroupNorm-apply + Mish + time bias run on the fp32 values in registers, ONE rounding to bf16 at the LDS store.
    Against fp64 GroupNorm -> Mish -> + temb -> Conv2d on the same fp32 c1 and bf16-rounded weights, and against the two-pass path
    (gn_mish_fwd writing h1 as bf16, the plain conv): same single rounding point, so the two differ by exp / rcp approximations only."""
    N, H, W, Cc, Co = cfg
    g = torch.Generator().manual_seed(89)
    c1 = torch.randn(N, Cc, H, W, generator=g) * 1.7 + 0.3
    gamma, beta = torch.randn(Cc, generator=g) * 0.5 + 1, torch.randn(Cc, generator=g) * 0.2
    temb = torch.randn(N, Cc, generator=g) * 0.3 + 0.5
    w = torch.randn(Co, Cc, 3, 3, generator=g) / math.sqrt(9 * Cc)
    bias = torch.randn(Co, generator=g) * 0.1
    Cop = (Co + 63) // 64 * 64
    wp = torch.zeros(Cop, Cc, 3, 3); wp[:Co] = w
    bp = torch.zeros(Cop); bp[:Co] = bias
    hn = F.group_norm(c1.double(), 8, gamma.double(), beta.double(), 1e-5)
    h = _mish64(hn) + temb.double()[:, :, None, None]
    ref = F.conv2d(h, w.bfloat16().double(), bias.double(), padding=1)
    xg = c1.permute(0, 2, 3, 1).contiguous().to(DEV)
    wf, wfq = _frag_weights(K, wp)
    dt = torch.bfloat16 if out16 else torch.float32
    stats, coef = K.gn_stats_coef(xg, gamma.to(DEV), beta.to(DEV), temb=temb.to(DEV))
    y = K.conv3x3_gn_mish(xg, coef, wf, K=Cc, Nc=Cop, bias=bp.to(DEV), out_dtype=dt, wq=wfq)
    assert y is not None and y.dtype == dt
    ls = _conv_launches(pw_always)
    assert ls[-1].startswith("conv_pw_kernel") and ls[-1].endswith(f", 2, 0, {pw_tile}, true>"), ls
    h1, _ = K.gn_mish_fwd(xg, gamma.to(DEV), beta.to(DEV), temb=temb.to(DEV), out_dtype=torch.bfloat16)
    y2 = K.conv3x3_bf16w(h1, wf, K=Cc, Nc=Cop, flip=False, bias=bp.to(DEV), out_dtype=dt, wq=wfq)
    torch.cuda.synchronize()
    got = y.float().cpu().permute(0, 3, 1, 2).double()[:, :Co]
    two = y2.float().cpu().permute(0, 3, 1, 2).double()[:, :Co]
    assert rel_err(got, ref) < 5e-3
    assert rel_err(got, two) < (5e-3 if out16 else 1.5e-3)
    assert not y[..., Co:].any()
    if (Cc // 8) % 16 == 0:
        xd = xg.double().view(N, H * W, Cc // 16, 16)
        sums = K.gn_sums_encode(torch.stack([xd.sum((1, 3)), (xd * xd).sum((1, 3))], dim=-1))
        _, coef2 = K.gn_coef_from_sums(sums, N, H * W, gamma.to(DEV), beta.to(DEV), temb=temb.to(DEV))
        ya = K.conv3x3_gn_mish(xg, coef2, wf, K=Cc, Nc=Cop, bias=bp.to(DEV), out_dtype=dt, wq=wfq)
        yb = K.conv3x3_gn_mish(xg, None, wf, K=Cc, Nc=Cop, bias=bp.to(DEV), out_dtype=dt, wq=wfq,
                               gn=(sums, gamma.to(DEV), beta.to(DEV), temb.to(DEV), 8, 1e-5))
        ls = _conv_launches(pw_always)
        assert ls[-1].endswith(f", 3, 0, {pw_tile}, true>") and ls[-2].endswith(f", 2, 0, {pw_tile}, true>"), ls
        assert torch.equal(ya, yb)
        assert rel_err(yb.float().cpu().permute(0, 3, 1, 2).double()[:, :Co], ref) < 5e-3


@pytest.mark.parametrize("cfg", [dict(N=8, H=32, Co=384, kind="qkv"), dict(N=4, H=16, Co=128, kind="out"), dict(N=16, H=8, Co=256, kind="res"),
                                 dict(N=2, H=16, Co=96, kind="res"), dict(N=8, H=16, Co=128, kind="dgrad"),
                                 dict(N=32, H=16, Co=384, kind="qkv", Ci=256),                 # two chunks, 128-pixel tiles
                                 dict(N=16, H=8, Co=384, kind="qkv", Ci=512),                  # four chunks, 64-pixel tiles
                                 dict(N=8, H=8, Co=256, kind="res", Ci=1024, split=512),       # res_conv over the skip concat
                                 dict(N=8, H=16, Co=128, kind="res", Ci=512, split=256),
                                 dict(N=64, H=16, Co=128, kind="out", Ci=384),                 # odd chunk count
                                 dict(N=8, H=16, Co=256, kind="dgrad", Ci=384)])               # to_qkv's data gradient (K = 384)
def test_conv1x1_pw(K, cfg, pw_always):
    """The 1x1 convs with K % 128 == 0 input channels through mi_conv1x1_pw (reference ddpm.py:134,151-152): to_qkv (no bias, bf16 out),
    to_out (bias + fp32 residual, fp32 out AND its bf16 copy from the same epilogue), res_conv (bias, fp32 out, a ragged channel tile),
    and the data gradient of to_out (transposed weights, accumulate into an fp32 buffer); against fp64 on the bf16-rounded operands."""
    N, H, Co, kind = cfg["N"], cfg["H"], cfg["Co"], cfg["kind"]
    Ci, split = cfg.get("Ci", 128), cfg.get("split")
    g = torch.Generator().manual_seed(83)
    x = torch.randn(N, Ci, H, H, generator=g).bfloat16()
    Cop = (Co + 63) // 64 * 64
    w = torch.zeros(Cop, Ci, 1, 1)
    w[:Co] = torch.randn(Co, Ci, 1, 1, generator=g) / math.sqrt(Ci)
    b = torch.zeros(Cop); b[:Co] = torch.randn(Co, generator=g)
    r = torch.randn(N, Cop, H, H, generator=g)
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
    wq64 = w.bfloat16().double()
    if kind == "dgrad":
        # data gradient of a Cop -> 128 conv... here: dX[p][ci] = sum_co dY[p][co] W[co][ci] with co = the 128 "input" channels
        wt = torch.randn(Ci, Cop, 1, 1, generator=g) / math.sqrt(Ci)          # forward weight [co = 128][ci = Cop]
        flat, wd, wf, offs, wdq, wfq = _pack(K, [conv_w_storage(wt.double())], frag=True)
        dy = x                                                                 # [N][128][H][H] bf16
        prev = torch.randn(N, H, H, Cop, generator=g).to(DEV)
        ref = F.conv_transpose2d(dy.double(), wt.bfloat16().double()) + prev.cpu().permute(0, 3, 1, 2).double()
        out = K.conv3x3_bf16w(nh(dy), wd, K=Ci, Nc=Cop, flip=True, ksize=1, out=prev.clone(), accumulate=True, wq=wdq)
        torch.cuda.synchronize()
        assert _conv_launches(pw_always)[-1].startswith("conv1x1_pw_kernel")
        assert rel_err(from_nhwc(out), ref) < 1e-5
        return
    flat, wd, wf, offs, wdq, wfq = _pack(K, [conv_w_storage(w.double())], frag=True)
    y64 = F.conv2d(x.double(), wq64)
    if kind == "qkv":
        y = K.conv3x3_bf16w(nh(x), wf, K=Ci, Nc=Cop, flip=False, ksize=1, out_dtype=torch.bfloat16, wq=wfq)
        torch.cuda.synchronize()
        assert y.dtype == torch.bfloat16 and rel_err(from_nhwc(y.float()), y64) < 6e-3
    elif kind == "out":
        ref = y64 + b.double()[None, :, None, None] + r.double()
        y, y16 = K.conv3x3_bf16w(nh(x), wf, K=Ci, Nc=Cop, flip=False, ksize=1, bias=b.to(DEV), residual=to_nhwc_gpu(r), want16=True, wq=wfq)
        torch.cuda.synchronize()
        assert rel_err(from_nhwc(y), ref) < 1e-5 and torch.equal(y16, y.bfloat16())
    else:
        ref = y64 + b.double()[None, :, None, None]
        xa, xb = (nh(x[:, :split]), nh(x[:, split:])) if split else (nh(x), None)
        y = K.conv3x3_bf16w(xa, wf, K=Ci, Nc=Cop, flip=False, ksize=1, bias=b.to(DEV), wq=wfq, x2=xb)
        torch.cuda.synchronize()
        assert rel_err(from_nhwc(y)[:, :Co], ref[:, :Co]) < 1e-5 and not y[..., Co:].any()
    assert _conv_launches(pw_always)[-1].startswith("conv1x1_pw_kernel"), _conv_launches(pw_always)


@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("cfg", [dict(N=2, H=32, Ci=128, Co=128), dict(N=4, H=16, Ci=256, Co=128, split=128), dict(N=16, H=8, Ci=512, Co=256),
                                 dict(N=6, H=8, Ci=192, Co=96)])
def test_conv3x3_pw_fp32_input(K, cfg, out16, pw_always, pw_tile):
    """mi_conv3x3_pw_x32: the private-weight-stream conv reading the fp32 residual stream directly (the sampler's block1 convs; pieces
    loaded into registers, rounded to bf16 once, written to the tile): bitwise the result of mi_f32_to_bf16 + mi_conv3x3_pw on both
    tile sizes, with two sources, bias, residual, accumulate, and with the GroupNorm sums in the epilogue."""
    N, H, Ci, Co = cfg["N"], cfg["H"], cfg["Ci"], cfg["Co"]
    split = cfg.get("split")
    g = torch.Generator().manual_seed(97)
    x = torch.randn(N, H, H, Ci, generator=g).to(DEV)
    Cop = (Co + 63) // 64 * 64
    w = torch.zeros(Cop, Ci, 3, 3); w[:Co] = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)
    wf, wfq = _frag_weights(K, w)
    bias = torch.randn(Cop, generator=g).to(DEV)
    res = torch.randn(N, H, H, Cop, generator=g).to(DEV)
    dt = torch.bfloat16 if out16 else torch.float32
    xa, xb = (x[..., :split].contiguous(), x[..., split:].contiguous()) if split else (x, None)
    y32 = K.conv3x3_bf16w(xa, wf, K=Ci, Nc=Cop, flip=False, x2=xb, bias=bias, residual=res, out_dtype=dt, wq=wfq)
    y16 = K.conv3x3_bf16w(xa.bfloat16(), wf, K=Ci, Nc=Cop, flip=False, x2=xb.bfloat16() if split else None, bias=bias, residual=res,
                          out_dtype=dt, wq=wfq)
    ls = _conv_launches(pw_always)
    o16 = "true" if out16 else "false"
    assert ls[-2:] == [f"conv_pw_kernel<{o16}, 0, 0, {pw_tile}, true>", f"conv_pw_kernel<{o16}, 0, 0, {pw_tile}>"], ls
    assert torch.equal(y32, y16)
    y2 = K.conv3x3_bf16w(xa, wf, K=Ci, Nc=Cop, flip=False, x2=xb, out=y32.clone(), accumulate=True, wq=wfq)
    y3 = K.conv3x3_bf16w(xa.bfloat16(), wf, K=Ci, Nc=Cop, flip=False, x2=xb.bfloat16() if split else None, out=y16.clone(), accumulate=True, wq=wfq)
    assert torch.equal(y2, y3)
    if Cop % 16 == 0:
        s32, s16 = K.gn_sums_buffer(N, Cop, DEV), K.gn_sums_buffer(N, Cop, DEV)
        ya = K.conv3x3_bf16w(xa, wf, K=Ci, Nc=Cop, flip=False, x2=xb, bias=bias, out_dtype=dt, gn_sums=s32, wq=wfq)
        yb = K.conv3x3_bf16w(xa.bfloat16(), wf, K=Ci, Nc=Cop, flip=False, x2=xb.bfloat16() if split else None, bias=bias, out_dtype=dt,
                             gn_sums=s16, wq=wfq)
        torch.cuda.synchronize()
        assert _conv_launches(pw_always)[-2] == f"conv_pw_kernel<{o16}, 1, 0, {pw_tile}, true>"
        assert torch.equal(ya, yb)
        # fixed-point sums, integer atomics: independent of the arrival order; the two instantiations may contract the squares into FMAs
        # differently (one float ulp of a workgroup's partial sum)
        assert int((s32 - s16).abs().max()) <= 1e-6 * int(s16.abs().max())
        s32b = K.gn_sums_buffer(N, Cop, DEV)
        K.conv3x3_bf16w(xa, wf, K=Ci, Nc=Cop, flip=False, x2=xb, bias=bias, out_dtype=dt, gn_sums=s32b, wq=wfq)
        assert torch.equal(s32, s32b)                                      # the same kernel twice: bitwise


@pytest.mark.parametrize("cfg", [dict(N=2, H=32, Ci=128, Co=128), dict(N=4, H=16, Ci=256, Co=128, split=128), dict(N=16, H=8, Ci=512, Co=256),
                                 dict(N=6, H=8, Ci=192, Co=320), dict(N=8, H=32, Ci=64, Co=64), dict(N=2, H=16, Ci=96, Co=64)])
def test_conv3x3_pw_f32_fwd_and_dgrad(K, cfg, pw_always, pw_tile):
    """Exact-fp32 mode of the private-weight-stream conv (mi_conv3x3_pw_f32 on v_mfma_f32_32x32x2_f32, fp32 fragment-order weights from
    mi_pack_weights_f32frag): Block's 3x3 conv (ddpm.py:116) and its data gradient, two sources, bias, residual, accumulate, both tile
    sizes, against fp64 -- the fp32 mode's bar (<= 1e-5; the contraction is an fp32 fma chain) -- and the fragment layout itself."""
    N, H, Ci, Co = cfg["N"], cfg["H"], cfg["Ci"], cfg["Co"]
    split = cfg.get("split")
    g = torch.Generator().manual_seed(101)
    x = torch.randn(N, Ci, H, H, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)
    b = torch.randn(Co, generator=g); r = torch.randn(N, Co, H, H, generator=g); dy = torch.randn(N, Co, H, H, generator=g)
    xq = x.double().requires_grad_(True)
    yq = F.conv2d(xq, w.double(), b.double(), padding=1) + r.double()
    yq.backward(dy.double())
    ws = conv_w_storage(w.double()).float().to(DEV)                    # [3][3][Ci][Co]
    flat = torch.zeros((ws.numel() + 63) // 64 * 64, device=DEV); flat[:ws.numel()] = ws.reshape(-1)
    table, nent, tiles = K.pack_table([(0, 9, Ci, Co)], DEV)
    wdq32, wfq32 = torch.zeros_like(flat), torch.zeros_like(flat)
    K.pack_weights_f32frag(table, nent, tiles, flat, wdq32, wfq32)
    if Ci % 64 == 0 and Co % 64 == 0:
        wb = ws.view(9, Ci, Co)
        fq = wfq32[:ws.numel()].view(9, Co // 32, Ci // 8, 2, 32, 4)       # [tap][nb][ko][l >> 5][l & 31][j]
        assert torch.equal(fq, wb.permute(0, 2, 1).reshape(9, Co // 32, 32, Ci // 8, 2, 4).permute(0, 1, 3, 4, 2, 5).contiguous())
        dq = wdq32[:ws.numel()].view(9, Ci // 32, Co // 8, 2, 32, 4)
        assert torch.equal(dq, wb.reshape(9, Ci // 32, 32, Co // 8, 2, 4).permute(0, 1, 3, 4, 2, 5).contiguous())
    else:
        assert not wfq32.any()                                              # not flagged: no fragment copy, and the host layer refuses
        assert K.conv3x3_f32(torch.zeros(N, H, H, Ci, device=DEV), wfq32, K=Ci, Nc=Co, flip=False) is None
        return
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
    xa, xb = (nh(x[:, :split]), nh(x[:, split:])) if split else (nh(x), None)
    yg = K.conv3x3_f32(xa, wfq32, K=Ci, Nc=Co, flip=False, x2=xb, bias=b.to(DEV), residual=to_nhwc_gpu(r))
    dxg = K.conv3x3_f32(nh(dy), wdq32, K=Co, Nc=Ci, flip=True)
    assert yg is not None and dxg is not None
    assert _conv_launches(pw_always)[-2:] == [f"conv_pw_kernel<false, 0, 0, {pw_tile}, false, true>"] * 2
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(yg), yq) < 2e-6 and rel_err(from_nhwc(dxg), xq.grad) < 2e-6
    dx2 = K.conv3x3_f32(nh(dy), wdq32, K=Co, Nc=Ci, flip=True, out=dxg.clone(), accumulate=True)
    assert rel_err(from_nhwc(dx2), 2 * xq.grad) < 2e-6


@pytest.mark.parametrize("cfg", [dict(N=8, H=32, Ci=128, Co=384), dict(N=16, H=8, Ci=512, Co=384), dict(N=8, H=8, Ci=1024, Co=256, split=512),
                                 dict(N=4, H=16, Ci=64, Co=128), dict(N=64, H=16, Ci=384, Co=128, dgrad=True), dict(N=2, H=16, Ci=192, Co=64)])
def test_conv1x1_pw_f32(K, cfg, pw_always):
    """The 1x1 convs in exact-fp32 mode (mi_conv1x1_pw_f32): to_qkv / to_out / res_conv shapes (reference ddpm.py:134,151-152), two
    sources, bias + residual, the data gradient with accumulate; against fp64 at the fp32 mode's bar."""
    N, H, Ci, Co = cfg["N"], cfg["H"], cfg["Ci"], cfg["Co"]
    split = cfg.get("split")
    g = torch.Generator().manual_seed(103)
    x = torch.randn(N, Ci, H, H, generator=g)
    w = torch.randn(Co, Ci, 1, 1, generator=g) / math.sqrt(Ci)
    b = torch.randn(Co, generator=g); r = torch.randn(N, Co, H, H, generator=g)
    ws = conv_w_storage(w.double()).float().to(DEV)                    # [1][1][Ci][Co]
    flat = torch.zeros((ws.numel() + 63) // 64 * 64, device=DEV); flat[:ws.numel()] = ws.reshape(-1)
    table, nent, tiles = K.pack_table([(0, 1, Ci, Co)], DEV)
    wdq32, wfq32 = torch.zeros_like(flat), torch.zeros_like(flat)
    K.pack_weights_f32frag(table, nent, tiles, flat, wdq32, wfq32)
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
    if cfg.get("dgrad"):
        dy = torch.randn(N, Co, H, H, generator=g)
        prev = torch.randn(N, H, H, Ci, generator=g).to(DEV)
        ref = F.conv_transpose2d(dy.double(), w.double()) + prev.cpu().permute(0, 3, 1, 2).double()
        out = K.conv1x1_f32(nh(dy), wdq32, K=Co, Nc=Ci, flip=True, out=prev.clone(), accumulate=True)
        torch.cuda.synchronize()
        assert out is not None and rel_err(from_nhwc(out), ref) < 2e-6
    else:
        ref = F.conv2d(x.double(), w.double(), b.double()) + r.double()
        xa, xb = (nh(x[:, :split]), nh(x[:, split:])) if split else (nh(x), None)
        y = K.conv1x1_f32(xa, wfq32, K=Ci, Nc=Co, flip=False, x2=xb, bias=b.to(DEV), residual=to_nhwc_gpu(r))
        torch.cuda.synchronize()
        assert y is not None and rel_err(from_nhwc(y), ref) < 2e-6
    assert _conv_launches(pw_always)[-1].startswith("conv1x1_pw_kernel<false, false,") and _conv_launches(pw_always)[-1].endswith(", true>")


@pytest.mark.parametrize("N,H,Co,bias", [(32, 32, 384, False), (64, 16, 384, True), (32, 32, 320, True), (256, 8, 256, False), (128, 32, 384, False)])
def test_conv1x1_pw_channel_tile_loop(K, N, H, Co, bias, pw_always):
    """to_qkv at the 128-channel level (bf16 in, bf16 out, K = 128, 128-pixel tiles): one workgroup per pixel tile walks the channel
    tiles (conv1x1_pw_kernel's NLOOP).  Against fp64 on the bf16-rounded operands, and bit-equal to the 2-D-grid form of the same kernel
    (same contraction order, same rounding); a ragged last channel tile (320 = 2.5 tiles) and a bias ride along."""
    g = torch.Generator().manual_seed(97)
    Ci = 128
    x = torch.randn(N, Ci, H, H, generator=g).bfloat16()
    w = torch.randn(Co, Ci, 1, 1, generator=g) / math.sqrt(Ci)
    b = torch.randn(Co, generator=g) if bias else None
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
    flat, wd, wf, offs, wdq, wfq = _pack(K, [conv_w_storage(w.double())], frag=True)
    ref = F.conv2d(x.double(), w.bfloat16().double()) + (b.double()[None, :, None, None] if bias else 0.0)
    kw = dict(K=Ci, Nc=Co, flip=False, ksize=1, out_dtype=torch.bfloat16, wq=wfq, bias=b.to(DEV) if bias else None)
    lib = K.load_library()
    was = lib.mi_debug_conv1x1_pw_nloop(2)          # the loop form whatever the grid (the default takes it from 1 024 pixel tiles up)
    try:
        y = K.conv3x3_bf16w(nh(x), wf, **kw)
        torch.cuda.synchronize()
        assert _conv_launches(pw_always)[-1] == "conv1x1_pw_kernel<true, false, 128, false, false, true>", _conv_launches(pw_always)
        assert y.dtype == torch.bfloat16 and rel_err(from_nhwc(y.float()), ref) < 6e-3
        lib.mi_debug_conv1x1_pw_nloop(0)
        y2 = K.conv3x3_bf16w(nh(x), wf, **kw)
        torch.cuda.synchronize()
        assert _conv_launches(pw_always)[-1] == "conv1x1_pw_kernel<true, false, 128>", _conv_launches(pw_always)
    finally:
        lib.mi_debug_conv1x1_pw_nloop(was)
    assert torch.equal(y, y2)


@pytest.mark.parametrize("cfg", [dict(N=8, H=32, Ci=128, Co=128), dict(N=16, H=8, Ci=512, Co=128), dict(N=8, H=8, Ci=1024, Co=256, split=512),
                                 dict(N=4, H=16, Ci=128, Co=256), dict(N=64, H=16, Ci=384, Co=128, acc=True)])
@pytest.mark.parametrize("out16", [False, True])
def test_conv1x1_pw_fp32_input(K, cfg, out16, pw_always):
    """mi_conv1x1_pw_x32: the streaming 1x1 kernel reading fp32 activations (the fp32 residual-stream gradient in the data gradients of
    to_out / res_conv, res_conv's input in inference): bitwise mi_f32_to_bf16 + mi_conv1x1_pw (same rounding, same contraction order)."""
    N, H, Ci, Co = cfg["N"], cfg["H"], cfg["Ci"], cfg["Co"]
    split = cfg.get("split")
    g = torch.Generator().manual_seed(109)
    x = torch.randn(N, H, H, Ci, generator=g).to(DEV)
    w = torch.randn(Co, Ci, 1, 1, generator=g) / math.sqrt(Ci)
    flat, wd, wf, offs, wdq, wfq = _pack(K, [conv_w_storage(w.double())], frag=True)
    bias = torch.randn(Co, generator=g).to(DEV); res = torch.randn(N, H, H, Co, generator=g).to(DEV)
    dt = torch.bfloat16 if out16 else torch.float32
    xa, xb = (x[..., :split].contiguous(), x[..., split:].contiguous()) if split else (x, None)
    kw = dict(K=Ci, Nc=Co, flip=False, ksize=1, bias=bias, residual=res)
    if cfg.get("acc") and not out16:
        prev = torch.randn(N, H, H, Co, generator=g).to(DEV)
        y32 = K.conv3x3_bf16w(xa, wf, x2=xb, out=prev.clone(), accumulate=True, wq=wfq, **kw)
        y16 = K.conv3x3_bf16w(xa.bfloat16(), wf, x2=None, out=prev.clone(), accumulate=True, wq=wfq, **kw)
    else:
        y32 = K.conv3x3_bf16w(xa, wf, x2=xb, out_dtype=dt, wq=wfq, **kw)
        y16 = K.conv3x3_bf16w(xa.bfloat16(), wf, x2=xb.bfloat16() if split else None, out_dtype=dt, wq=wfq, **kw)
    torch.cuda.synchronize()
    ls = _conv_launches(pw_always)
    assert ls[-2].endswith(", 64, false, true>") and ls[-2].startswith("conv1x1_pw_kernel") and ls[-1].startswith("conv1x1_pw_kernel"), ls
    assert torch.equal(y32, y16)


@pytest.mark.parametrize("split", [2, 4])
@pytest.mark.parametrize("cfg", [(16, 8, 8, 512, 512), (8, 16, 16, 256, 256), (4, 16, 16, 256, 320), (2, 32, 32, 256, 128), (4, 8, 8, 1024, 256, 512)])
def test_conv3x3_pw_split_k(K, cfg, split, pw_always, pw_tile):
    """Split-K launches of conv_pw_kernel (the layers whose tiles would leave CUs without a workgroup): slices 1 .. S-1 of the contraction
    leave their fp32 accumulators in the registered workspace, slice 0 adds them and runs the unchanged epilogue.  Every variant the
    sampler and cfg 3 launch that way -- plain conv (bf16 / fp32 out, bias + residual, accumulate), GroupNorm sums from the epilogue,
    fp32 input, two sources, the fused GroupNorm + Mish forms -- against the unsplit launch of the same kernel (fp32 summation order
    is all that differs) and fp64; twice in a row (the flags are lowered for the next launch) and from a replayed graph."""
    N, H, W, Ci, Co = cfg[:5]
    K1 = cfg[5] if len(cfg) > 5 else None
    if Ci // 64 % split or Ci // 64 // split < 2:
        pytest.skip("fewer than two chunks per slice")
    lib = K.load_library()
    dev = torch.device(DEV, torch.cuda.current_device())
    had_ws = K._SPLITK_WS.get(dev.index) is not None
    if not had_ws:                                 # MI_CONV_AUTO=0 runs (the halo-only subprocess): no workspace was registered
        K._splitk_workspace(dev)
    g = torch.Generator().manual_seed(131 + split)
    x = torch.randn(N, H, W, Ci, generator=g).to(DEV)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)
    Cop = (Co + 63) // 64 * 64
    wp = torch.zeros(Cop, Ci, 3, 3); wp[:Co] = w
    wf, wfq = _frag_weights(K, wp)
    bias = torch.randn(Cop, generator=g).to(DEV); res = torch.randn(N, H, W, Cop, generator=g).to(DEV)
    xb = x.bfloat16()
    xa, x2 = (xb[..., :K1].contiguous(), xb[..., K1:].contiguous()) if K1 else (xb, None)
    ref = F.conv2d(xb.double().cpu().permute(0, 3, 1, 2), w.bfloat16().double(), padding=1).permute(0, 2, 3, 1)
    gamma, beta = (torch.rand(Ci, generator=g) + 0.5).to(DEV), torch.randn(Ci, generator=g).to(DEV)
    temb = torch.randn(N, Ci, generator=g).to(DEV)

    def run_all():
        out = {}
        out["bf16"] = K.conv3x3_bf16w(xa, wf, K=Ci, Nc=Cop, flip=False, x2=x2, bias=bias, out_dtype=torch.bfloat16, wq=wfq)
        out["f32"] = K.conv3x3_bf16w(xa, wf, K=Ci, Nc=Cop, flip=False, x2=x2, bias=bias, residual=res, wq=wfq)
        out["acc"] = K.conv3x3_bf16w(xa, wf, K=Ci, Nc=Cop, flip=False, x2=x2, out=res.clone(), accumulate=True, wq=wfq)
        if K1 is None:
            sums = K.gn_sums_buffer(N, Cop, DEV)
            out["gns"] = K.conv3x3_bf16w(xb, wf, K=Ci, Nc=Cop, flip=False, bias=bias, out_dtype=torch.bfloat16, gn_sums=sums, wq=wfq)
            out["sums"] = K.gn_sums_decode(sums).clone()
            out["x32"] = K.conv3x3_bf16w(x, wf, K=Ci, Nc=Cop, flip=False, bias=bias, out_dtype=torch.bfloat16, wq=wfq)
            if (Ci // 8) % 16 == 0 and Ci // 8 <= 64 and H * W >= 128:         # (one image per tile: the fused forms)
                st, coef = K.gn_stats_coef(xb, gamma, beta, temb=temb)
                out["fused"] = K.conv3x3_gn_mish(xb, coef, wf, K=Ci, Nc=Cop, bias=bias, out_dtype=torch.bfloat16, wq=wfq)
                st32, coef32 = K.gn_stats_coef(x, gamma, beta, temb=temb)
                out["fused32"] = K.conv3x3_gn_mish(x, coef32, wf, K=Ci, Nc=Cop, bias=bias, out_dtype=torch.bfloat16, wq=wfq)
        torch.cuda.synchronize()
        return out

    was = lib.mi_debug_conv_pw_splitk(0); K._QUERY_CACHE.clear()
    try:
        base = run_all()
        assert all(lib.mi_conv3x3_pw_splitk(C_byref(K, N, H, W, Ci, Cop, K1), v, 0) & 15 == 1 for v in (0, 2))
        lib.mi_debug_conv_pw_splitk(split); K._QUERY_CACHE.clear()
        q = lib.mi_conv3x3_pw_splitk(C_byref(K, N, H, W, Ci, Cop, K1), 0, 0)
        assert q & 15 == split and q >> 4 == pw_tile, (q, split, pw_tile)
        a = run_all()
        b = run_all()                              # the flags were lowered: a second launch waits for ITS partial tiles
        gph = torch.cuda.CUDAGraph(); st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            with torch.cuda.graph(gph, stream=st):
                yg = K.conv3x3_bf16w(xa, wf, K=Ci, Nc=Cop, flip=False, x2=x2, bias=bias, residual=res, wq=wfq)
        for _ in range(3):
            gph.replay()
        torch.cuda.synchronize()
    finally:
        lib.mi_debug_conv_pw_splitk(was); K._QUERY_CACHE.clear()
        if not had_ws:
            lib.mi_conv_pw_set_splitk_workspace(None, 0); K._SPLITK_WS[dev.index] = None
    for k, v in a.items():
        if v is None:
            continue
        assert torch.equal(v, b[k]), k                                         # deterministic: the slices are added in a fixed order
        d0 = (v.double() - base[k].double()).abs().max()
        scale = float(base[k].double().abs().max())
        if k == "sums":                                                        # of the stored bf16 values: a flipped rounding moves a sum
            assert float(d0) <= 1e-3 * scale, (k, float(d0), scale)
        elif v.dtype == torch.bfloat16:
            assert float(d0) <= 2 ** -7 * scale and float((v != base[k]).float().mean()) < 0.05, (k, float(d0), scale)
        else:
            assert float(d0) <= 3e-6 * scale, (k, float(d0), scale)
    assert torch.equal(yg, a["f32"])
    got = a["f32"].double().cpu() - bias.double().cpu() - res.double().cpu()
    assert rel_err(got[..., :Co], ref) < 1e-5


def C_byref(K, N, H, W, Ci, Co, K1):
    import ctypes
    d = K.MiConvDesc(N=N, IH=H, IW=W, OH=H, OW=W, K=Ci, Nc=Co, KH=3, KW=3, stride=1, pad=1, transposed=0, w_kn=0, mode=K.MODE_BF16,
                     K1=K1 or Ci, ldx=K1 or Ci, ldx2=(Ci - K1) if K1 else 0, ldy=Co, ldr=0, accumulate=0)
    return ctypes.byref(d)


@pytest.mark.parametrize("N,H,Ci,Co,bias", [(64, 32, 128, 384, False), (32, 32, 128, 384, False), (8, 32, 128, 384, False), (64, 16, 256, 384, False),
                                            (128, 16, 256, 384, True), (64, 8, 512, 384, True), (512, 8, 512, 384, False), (2, 8, 512, 320, False),
                                            (8, 16, 256, 128, True), (2, 8, 128, 64, False)])
def test_layernorm_conv1x1_fused(K, N, H, Ci, Co, bias, pw_always):
    """mi_ln_conv1x1_pw (inference): PreNorm's channel LayerNorm (reference ddpm.py:85-95: eps added to the std) applied while to_qkv's
    input is staged -- every tile form (128 pixels x one chunk, 64 pixels x 1 / 2 / 4 chunks; channel-tile loop from 512 pixel tiles up, a
    workgroup per channel tile below), ragged last channel tile, bias.  Against
    fp64 on the operands the two-launch path rounds (bf16 LayerNorm output, bf16 weights), and against that path itself: the two differ only
    where the LayerNorm's summation order moves a value across a bf16 rounding boundary."""
    g = torch.Generator().manual_seed(211 + Ci + H)
    x = (torch.randn(N, H, H, Ci, generator=g) * 1.7 - 0.4).to(DEV)
    gg = (torch.randn(Ci, generator=g) * 0.3 + 1).to(DEV); bb = (torch.randn(Ci, generator=g) * 0.2).to(DEV)
    w = torch.randn(Co, Ci, 1, 1, generator=g) / math.sqrt(Ci)
    b = torch.randn(Co, generator=g).to(DEV) if bias else None
    flat, wd, wf, offs, wdq, wfq = _pack(K, [conv_w_storage(w.double())], frag=True)
    assert K.ln_conv1x1_supported(N, H, H, Ci, Co)
    y = K.ln_conv1x1(x, gg, bb, wfq, Nc=Co, bias=b)
    yt, lnt = K.ln_conv1x1(x, gg, bb, wfq, Nc=Co, bias=b, want_ln=True)      # training's form: the normalised tensor written along
    ln = K.chan_layernorm_fwd(x, gg, bb, out_dtype=torch.bfloat16)
    y2 = K.conv3x3_bf16w(ln, wf, K=Ci, Nc=Co, flip=False, ksize=1, out_dtype=torch.bfloat16, wq=wfq, bias=b)
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and y.shape == (N, H, H, Co)
    xd = x.double().cpu()
    std = xd.var(dim=3, unbiased=False, keepdim=True).sqrt()
    lnd = (xd - xd.mean(3, keepdim=True)) / (std + 1e-5) * gg.double().cpu() + bb.double().cpu()
    assert rel_err(ln.float().cpu(), lnd) < 4e-3
    ref = torch.einsum("nhwc,oc->nhwo", ln.double().cpu(), w[:, :, 0, 0].bfloat16().double()) + (b.double().cpu() if bias else 0.0)
    e_fused, e_two = rel_err(y.float().cpu(), ref), rel_err(y2.float().cpu(), ref)
    assert e_two < 6e-3 and e_fused < 6e-3, (e_fused, e_two)
    # the dual form: the same y, and the tensor the MFMAs read -- the LayerNorm kernel's output up to summation-order flips of a bf16 ulp
    assert torch.equal(yt, y) and lnt.dtype == torch.bfloat16 and lnt.shape == x.shape
    assert rel_err(lnt.float().cpu(), lnd) < 4e-3
    dl = (lnt.float() - ln.float()).abs()
    assert float((dl > 0).float().mean()) < 0.02 and float(dl.max()) <= 2 ** -7 * float(ln.float().abs().max())
    ref_t = torch.einsum("nhwc,oc->nhwo", lnt.double().cpu(), w[:, :, 0, 0].bfloat16().double()) + (b.double().cpu() if bias else 0.0)
    assert rel_err(yt.float().cpu(), ref_t) < 4e-3                         # y IS the conv of the tensor written along (bf16 output rounding only)
    # the two paths against each other: a handful of bf16 ulps where the LayerNorm output crossed a rounding boundary
    diff = (y.float() - y2.float()).abs()
    assert float(diff.max()) <= 0.05 * float(y2.float().abs().max()) and float((diff > 0).float().mean()) < 0.2, (float(diff.max()), float((diff > 0).float().mean()))


def test_pack_weights_fragment_order(K):
    """The MFMA-fragment-order copies mi_conv3x3_pw streams (include/mi_ddpm.h): wfq[tap][co/32][ci/16][lane][8] and
    wdq[tap][ci/32][co/16][lane][8] for the 3x3, 1x1 and (round 4: the tap-gather kernel's Upsample) 4x4 layers with 64-multiples on
    both sides; the others get none (zero slice)."""
    g = torch.Generator().manual_seed(29)
    ws = [torch.randn(3, 3, 128, 64, generator=g).to(DEV), torch.randn(1, 1, 128, 384, generator=g).to(DEV),
          torch.randn(3, 3, 192, 256, generator=g).to(DEV), torch.randn(3, 3, 40, 64, generator=g).to(DEV),
          torch.randn(4, 4, 64, 64, generator=g).to(DEV), torch.randn(4, 4, 40, 64, generator=g).to(DEV)]
    flat, wd, wf, offs, wdq, wfq = _pack(K, ws, frag=True)
    torch.cuda.synchronize()
    for w, o in zip(ws, offs):
        kh, kw, ci, co = w.shape
        n = w.numel()
        assert torch.equal(wd[o:o + n].view(w.shape), w.to(torch.bfloat16))            # the plain copies are unchanged
        if kh * kw not in (1, 9, 16) or ci % 64 or co % 64:
            assert not wdq[o:o + n].any() and not wfq[o:o + n].any()
            continue
        T = kh * kw
        wb = w.to(torch.bfloat16).view(T, ci, co)
        # lane l, element e of fragment (nb, kq): row 32 nb + (l & 31), column 16 kq + 8 (l >> 5) + e
        fq = wfq[o:o + n].view(T, co // 32, ci // 16, 2, 32, 8)          # [tap][nb][kq][l >> 5][l & 31][e]
        ref_f = wb.permute(0, 2, 1).reshape(T, co // 32, 32, ci // 16, 2, 8).permute(0, 1, 3, 4, 2, 5)
        assert torch.equal(fq, ref_f.contiguous())
        dq = wdq[o:o + n].view(T, ci // 32, co // 16, 2, 32, 8)
        ref_d = wb.reshape(T, ci // 32, 32, co // 16, 2, 8).permute(0, 1, 3, 4, 2, 5)
        assert torch.equal(dq, ref_d.contiguous())


@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("cfg", [
    dict(N=2, H=32, Ci=128, Co=128),             # level 0: 4 rows of 32 per tile, 2 chunks
    dict(N=8, H=32, Ci=64, Co=256),              # XCD-grouped tile order, one chunk, 2 channel tiles
    dict(N=4, H=16, Ci=256, Co=128, split=128),  # skip concat (two sources), 8 rows of 16
    dict(N=16, H=8, Ci=512, Co=512),             # two 8x8 images per tile, 8 chunks, (pixel, channel) XCD groups
    dict(N=2, H=16, Ci=64, Co=96),               # ragged channel tile: one idle wave
    dict(N=4, H=8, Ci=1024, Co=64, split=512),   # long K, half-empty channel tile
    dict(N=6, H=8, Ci=192, Co=320),              # odd chunk count, ragged channel tile
])
def test_conv3x3_pw_fwd_and_dgrad(K, cfg, out16, pw_always, pw_tile):
    _pw_fwd_dgrad_case(K, cfg, out16, pw_always, pw_tile)


@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("cfg", [
    dict(N=2, H=32, Ci=128, Co=128),             # level 0: 8 rows of 32 per tile, 2 chunks
    dict(N=8, H=32, Ci=64, Co=256),              # XCD-grouped tile order, one chunk, 2 channel tiles
    dict(N=4, H=16, Ci=256, Co=128, split=128),  # skip concat (two sources), one 16x16 image per tile
    dict(N=3, H=16, Ci=64, Co=96),               # ragged channel tile: one idle wave
    dict(N=2, H=16, Ci=192, Co=320),             # odd chunk count, ragged channel tile
    dict(N=1, H=32, Ci=512, Co=64, split=256),   # long K, half-empty channel tile
])
def test_conv3x3_pw_fwd_and_dgrad_tile256(K, cfg, out16, pw_always, pw_tile256):
    """The same checks on the 256-pixel tiles (round 5): wave = 256 pixels x 32 channels, one workgroup per CU."""
    _pw_fwd_dgrad_case(K, cfg, out16, pw_always, pw_tile256)


@pytest.mark.parametrize("cfg", [dict(N=8, H=48, W=16, Ci=128, Co=256),     # six row tiles per image (not a power of two), image-per-XCD order
                                 dict(N=4, H=48, W=16, Ci=192, Co=768),     # (pixel, channel) XCD groups with three channel tiles per group
                                 dict(N=2, H=24, W=8, Ci=64, Co=128)])      # three 64-pixel row tiles per image
def test_conv3x3_pw_non_power_of_two_tile_counts(K, cfg, pw_always):
    """Round 5: the prologue's integer divisions (row tiles per image, channel tiles per XCD group, chunks per workgroup rotation) are
    multiplications by host-computed reciprocals -- images with 6 / 3 row tiles and layers with 3 channel tiles per group and 3 chunks
    take every one of them off the power-of-two path; forward and data gradient against fp64 on the same bf16-rounded operands."""
    N, H, W, Ci, Co = cfg["N"], cfg["H"], cfg["W"], cfg["Ci"], cfg["Co"]
    g = torch.Generator().manual_seed(613)
    x = torch.randn(N, Ci, H, W, generator=g).bfloat16()
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(Ci * 9))
    b = torch.randn(Co, generator=g)
    dy = torch.randn(N, Co, H, W, generator=g).bfloat16()
    xq = x.double().requires_grad_(True)
    yq = F.conv2d(xq, w.bfloat16().double(), b.double(), padding=1)
    yq.backward(dy.double())
    flat, wd, wf, offs, wdq, wfq = _pack(K, [conv_w_storage(w.double())], frag=True)
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
    yg = K.conv3x3_bf16w(nh(x), wf, K=Ci, Nc=Co, flip=False, bias=b.to(DEV), out_dtype=torch.float32, wq=wfq)
    dxg = K.conv3x3_bf16w(nh(dy), wd, K=Co, Nc=Ci, flip=True, out_dtype=torch.float32, wq=wdq)
    ls = _conv_launches(pw_always)
    assert len(ls) == 2 and all(q.startswith("conv_pw_kernel") for q in ls), ls
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(yg), yq) < 1e-5
    assert rel_err(from_nhwc(dxg), xq.grad) < 1e-5


def _pw_fwd_dgrad_case(K, cfg, out16, pw_always, pw_tile):
    """Block's 3x3 conv (ddpm.py:116) and its data gradient for bf16-stored activations through the private-weight-stream kernel
    (mi_conv3x3_pw: fragment-order weights by LDS-DMA per wave, one barrier per 64-channel chunk): bias, residual, fp32 and bf16
    output, accumulate; against fp64 on the same bf16-rounded operands and against the halo kernel."""
    from src.ops.lib import MiConvDesc, load_library
    import ctypes
    N, H, Ci, Co = cfg["N"], cfg["H"], cfg["Ci"], cfg["Co"]
    split = cfg.get("split")
    g = torch.Generator().manual_seed(61)
    x = torch.randn(N, Ci, H, H, generator=g).bfloat16()
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(Ci * 9))
    b = torch.randn(Co, generator=g)
    r = torch.randn(N, Co, H, H, generator=g)
    dy = torch.randn(N, Co, H, H, generator=g).bfloat16()
    xq = x.double().requires_grad_(True)
    wq = w.bfloat16().double()
    yq = F.conv2d(xq, wq, b.double(), padding=1) + r.double()
    yq.backward(dy.double())
    # weights padded to 64-multiples on both sides (the fragment copies need them; the extra rows / columns are zero)
    Cip, Cop = (Ci + 63) // 64 * 64, (Co + 63) // 64 * 64
    wp = torch.zeros(Cop, Cip, 3, 3, dtype=torch.float64)
    wp[:Co, :Ci] = w.double()
    flat, wd, wf, offs, wdq, wfq = _pack(K, [conv_w_storage(wp)], frag=True)
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
    xa, xb = (nh(x[:, :split]), nh(x[:, split:])) if split else (nh(x), None)
    d = MiConvDesc(N=N, IH=H, IW=H, OH=H, OW=H, K=Ci, Nc=Cop, KH=3, KW=3, stride=1, pad=1, transposed=0, w_kn=0, mode=1, K1=split or Ci,
                   ldx=xa.shape[3], ldx2=xb.shape[3] if xb is not None else 0, ldy=Cop, ldr=Cop, accumulate=0)
    assert load_library().mi_conv3x3_pw_supported(ctypes.byref(d)) == 1
    assert K.USE_CONV_PW
    odt = torch.bfloat16 if out16 else torch.float32
    tol = 6e-3 if out16 else 1e-5                                        # bf16 output: one more rounding
    bp = torch.zeros(Cop); bp[:Co] = b
    rp = torch.zeros(N, Cop, H, H); rp[:, :Co] = r
    dyp = torch.zeros(N, Cop, H, H); dyp[:, :Co] = dy.float()
    yg = K.conv3x3_bf16w(xa, wf, K=Ci, Nc=Cop, flip=False, x2=xb, bias=bp.to(DEV), residual=to_nhwc_gpu(rp), out_dtype=odt, wq=wfq)
    assert yg is not None and yg.dtype == odt
    dxg = K.conv3x3_bf16w(nh(dyp.bfloat16()), wd, K=Cop, Nc=Cip, flip=True, out_dtype=odt, wq=wdq)
    ls = _conv_launches(pw_always)
    assert len(ls) == 2 and all(q.startswith("conv_pw_kernel") and q.endswith(f", {pw_tile}>") for q in ls), ls
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(yg.float())[:, :Co], yq) < tol
    assert not yg[..., Co:].any()
    assert rel_err(from_nhwc(dxg.float())[:, :Ci], xq.grad) < tol
    dx2 = K.conv3x3_bf16w(nh(dyp.bfloat16()), wd, K=Cop, Nc=Cip, flip=True, out=dxg.clone(), accumulate=True, wq=wdq)
    assert rel_err(from_nhwc(dx2.float())[:, :Ci], 2 * xq.grad) < 2 * tol
    # the halo / shift kernels on the same operands (no fragment-order weights passed: the default pick of round 2)
    y2 = K.conv3x3_bf16w(xa, wf, K=Ci, Nc=Cop, flip=False, x2=xb, bias=bp.to(DEV), residual=to_nhwc_gpu(rp), out_dtype=odt)
    assert rel_err(yg.float(), y2.float()) < tol




@pytest.mark.parametrize("cfg", [
    # (the tile is what mi_conv3x3_bf16w_tile answers; tests/test_halo_kernels_gpu.py asserts it per launch and reaches the 256-pixel tiles)
    dict(N=2, H=32, Ci=128, Co=128),             # level 0: <64,64>, 2 rows x 32 cols per tile
    dict(N=4, H=16, Ci=256, Co=128, split=128),  # skip concat: <64,64>, 4 x 16 tiles
    dict(N=2, H=8, Ci=64, Co=192),               # <64,64>: 64-pixel tiles (one 8x8 image), ragged N tile
    dict(N=16, H=8, Ci=512, Co=512),             # <64,64>: one 8x8 image per tile, tiles in (P, Q) = (4, 2) order over the XCDs
    dict(N=4, H=4, Ci=32, Co=32),                # <64,32>: CK=32 path, 4 images per tile
    dict(N=40, H=32, Ci=64, Co=128),             # <128,64> with 8 waves: 320 tiles of 4 rows, an image's tiles on one XCD
    dict(N=1, H=64, Ci=64, Co=64),               # cfg-3 level 0: <128,32>, 2 rows x 64 cols
    dict(N=8, H=64, Ci=64, Co=64),               # ... <128,32> again (256 tiles of 2 rows: below the 400 a 128-pixel plan asks, 64-pixel tiles do not fit W = 64)
    dict(N=8, H=64, Ci=128, Co=64, split=64),    # ... the up path's skip concat into 64 channels, <128,32>; its data gradient has 128 outputs
])
def test_conv3x3_halo_fwd_and_dgrad(K, cfg):
    """Block's 3x3 conv (ddpm.py:116) and its data gradient through the LDS halo-tile kernel."""
    N, H, Ci, Co = cfg["N"], cfg["H"], cfg["Ci"], cfg["Co"]
    split = cfg.get("split")
    g = torch.Generator().manual_seed(29)
    x = torch.randn(N, Ci, H, H, generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(Co, Ci, 3, 3, generator=g, dtype=torch.float64) / math.sqrt(Ci * 9)).requires_grad_(True)
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    r = torch.randn(N, Co, H, H, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, b, padding=1) + r
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    flat, wd, wf, offs = _pack(K, [conv_w_storage(w.detach())])
    if split:
        xa, xb = to_nhwc_gpu(x.detach()[:, :split].float()), to_nhwc_gpu(x.detach()[:, split:].float())
    else:
        xa, xb = to_nhwc_gpu(x.detach().float()), None
    yg = K.conv3x3_bf16w(xa, wf, K=Ci, Nc=Co, flip=False, x2=xb, bias=b.float().to(DEV), residual=to_nhwc_gpu(r.float()))
    assert yg is not None, "shape should be supported by the halo kernel"
    dxg = K.conv3x3_bf16w(to_nhwc_gpu(dy.float()), wd, K=Co, Nc=Ci, flip=True)
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(yg), y) < 2e-2
    assert rel_err(from_nhwc(dxg), x.grad) < 2e-2
    # against the same bf16-rounded operands the error is only fp32 accumulation order
    xq, wq = x.detach().float().bfloat16().double(), w.detach().float().bfloat16().double()
    yq = F.conv2d(xq, wq, b, padding=1) + r
    assert rel_err(from_nhwc(yg), yq) < 1e-5
    dx2 = K.conv3x3_bf16w(to_nhwc_gpu(dy.float()), wd, K=Co, Nc=Ci, flip=True, out=dxg.clone(), accumulate=True)
    assert rel_err(from_nhwc(dx2), 2 * x.grad) < 2e-2


@pytest.mark.parametrize("cfg", [
    dict(N=8, H=32, Ci=128, Co=128),
    dict(N=16, H=16, Ci=256, Co=128, split=128),
    dict(N=8, H=8, Ci=64, Co=192),
    dict(N=16, H=8, Ci=512, Co=256),
    dict(N=8, H=4, Ci=32, Co=32),
    dict(N=8, H=4, Ci=128, Co=128),              # 4x4 images: 25 X slots per channel, LDS forces 64-wide co tiles
    dict(N=8, H=64, Ci=64, Co=64),
])
def test_conv3x3_wgrad_fast(K, cfg):
    """aten::convolution_backward (weight) of Block's 3x3 conv through the image-major MFMA kernel."""
    N, H, Ci, Co = cfg["N"], cfg["H"], cfg["Ci"], cfg["Co"]
    split = cfg.get("split")
    g = torch.Generator().manual_seed(31)
    x = torch.randn(N, Ci, H, H, generator=g, dtype=torch.float64)
    w = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(N, Co, H, H, generator=g, dtype=torch.float64)
    F.conv2d(x, w, None, padding=1).backward(dy)
    dW = torch.zeros(9 * Ci * Co, device=DEV)
    if split:
        P, P2 = to_nhwc_gpu(x[:, :split].float()), to_nhwc_gpu(x[:, split:].float())
    else:
        P, P2 = to_nhwc_gpu(x.float()), None
    from src.ops.lib import MiWgradDesc, load_library
    import ctypes
    d = MiWgradDesc(N=N, GH=H, GW=H, DH=H, DW=H, Ci=Ci, Cj=Co, KH=3, KW=3, stride=1, pad=1, gather_i=1, mode=1,
                    I1=split or Ci, ldp=4, ldp2=4, ldq=4)
    assert load_library().mi_conv3x3_wgrad_supported(ctypes.byref(d)) == 1
    db = torch.zeros(Co, device=DEV)
    K.conv_wgrad(P, to_nhwc_gpu(dy.float()), dW, kh=3, kw=3, stride=1, pad=1, gather_i=True, Ci=Ci, Cj=Co,
                 grid_g=(H, H), grid_d=(H, H), mode=1, P2=P2, dbias=db)
    torch.cuda.synchronize()
    assert rel_err(db, dy.sum((0, 2, 3))) < 1e-5          # bias gradient fused into the dY staging
    got = w_from_storage(dW.view(3, 3, Ci, Co))
    assert rel_err(got, w.grad) < 2e-2
    xq, dq = x.float().bfloat16().double(), dy.float().bfloat16().double()
    wq = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xq, wq, None, padding=1).backward(dq)
    assert rel_err(got, wq.grad) < 2e-5          # same bf16-rounded operands: only summation order differs


@pytest.mark.parametrize("cfg", [
    dict(N=2, H=32, W=32, Ci=128, Co=128),                 # level 0: 2 rows per step, 2 ci tiles
    dict(N=8, H=32, W=32, Ci=64, Co=256),                  # 2 co tiles, long k-slices
    dict(N=4, H=16, W=16, Ci=256, Co=256),                 # level 1: 4 rows per step
    dict(N=8, H=8, W=8, Ci=128, Co=128),                   # 8x8: a step is a whole image (half-waves read different rows)
    dict(N=16, H=8, W=8, Ci=512, Co=512),                  # level 2, 32 tiles
    dict(N=1, H=64, W=64, Ci=64, Co=64),                   # cfg 3 level 0: one row per step, co tile half empty
    dict(N=2, H=16, W=16, Ci=192, Co=96, split=128),       # skip concat (two sources) and a ragged co tile
    dict(N=1, H=16, W=8, Ci=64, Co=32),                    # non-square: halo rows inside an image at W = 8
    dict(N=3, H=32, W=32, Ci=64, Co=128, blocks=7),        # slices that start and end in the middle of an image
])
def test_conv3x3_wgrad_lds_dma(K, cfg):
    """aten::convolution_backward (weight) of Block's 3x3 conv for bf16-stored operands through the LDS-DMA + transposing-read
    kernel (mi_conv3x3_wgrad_tr): against an fp64 evaluation on the same bf16-rounded operands (only the summation order
    differs: <= 2e-5) and against the image-major register-staged kernel; twice into the same buffer = 2x (accumulate)."""
    from src.ops.lib import MiWgradDesc, load_library
    import ctypes
    N, H, W, Ci, Co = cfg["N"], cfg["H"], cfg["W"], cfg["Ci"], cfg["Co"]
    split = cfg.get("split")
    g = torch.Generator().manual_seed(41)
    x = torch.randn(N, Ci, H, W, generator=g).bfloat16()
    dy = torch.randn(N, Co, H, W, generator=g).bfloat16()
    wq = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wq, None, padding=1).backward(dy.double())

    def nhwc16(t):
        return t.permute(0, 2, 3, 1).contiguous().to(DEV)
    if split:
        P, P2 = nhwc16(x[:, :split]), nhwc16(x[:, split:])
    else:
        P, P2 = nhwc16(x), None
    Q = nhwc16(dy)
    d = MiWgradDesc(N=N, GH=H, GW=W, DH=H, DW=W, Ci=Ci, Cj=Co, KH=3, KW=3, stride=1, pad=1, gather_i=1, mode=1,
                    I1=split or Ci, ldp=P.shape[3], ldp2=P2.shape[3] if P2 is not None else 0, ldq=Co)
    lib = load_library()
    assert lib.mi_conv3x3_wgrad_tr_supported(ctypes.byref(d)) == 1
    lib.mi_debug_wgrad_tr_blocks(cfg.get("blocks", 0))
    dW = torch.zeros(9 * Ci * Co, device=DEV)
    assert K.USE_WGRAD_TR
    try:
        K.conv_wgrad(P, Q, dW, kh=3, kw=3, stride=1, pad=1, gather_i=True, Ci=Ci, Cj=Co, grid_g=(H, W), grid_d=(H, W), mode=1, P2=P2)
        torch.cuda.synchronize()
    finally:
        lib.mi_debug_wgrad_tr_blocks(0)
    got = w_from_storage(dW.view(3, 3, Ci, Co))
    assert rel_err(got, wq.grad) < 2e-5
    worst = float((got.double() - wq.grad).abs().max() / wq.grad.abs().max())
    assert worst < 1e-4, worst
    K.conv_wgrad(P, Q, dW, kh=3, kw=3, stride=1, pad=1, gather_i=True, Ci=Ci, Cj=Co, grid_g=(H, W), grid_d=(H, W), mode=1, P2=P2)
    torch.cuda.synchronize()
    assert rel_err(w_from_storage(dW.view(3, 3, Ci, Co)), 2 * wq.grad) < 2e-5
    # the register-staged kernel on the same operands
    if lib.mi_conv3x3_wgrad_supported(ctypes.byref(d)):
        K.USE_WGRAD_TR = False
        try:
            dW2 = torch.zeros(9 * Ci * Co, device=DEV)
            K.conv_wgrad(P, Q, dW2, kh=3, kw=3, stride=1, pad=1, gather_i=True, Ci=Ci, Cj=Co, grid_g=(H, W), grid_d=(H, W), mode=1, P2=P2)
            torch.cuda.synchronize()
        finally:
            K.USE_WGRAD_TR = True
        assert rel_err(dW2, dW / 2) < 2e-5


def test_conv1x1_wgrad_queue(K):
    """K.WgradQueue.push1x1: the 1x1 convs' weight gradients (to_qkv: bf16 dY; to_out / res_conv: fp32 stream gradient + fused bias
    gradient; a two-source res_conv; a ragged co tile) batched into mi_conv1x1_wgrad_tr_batch launches, against fp64 on the same
    bf16-rounded operands (fp32 dY is rounded to bf16 in LDS exactly like the register-staged kernel rounds it)."""
    g = torch.Generator().manual_seed(47)
    layers = [dict(N=8, H=32, Ci=128, Co=384, q32=False), dict(N=8, H=32, Ci=128, Co=128, q32=True, bias=True),
              dict(N=8, H=16, Ci=256, Co=384, q32=False), dict(N=8, H=16, Ci=128, Co=256, q32=True, bias=True),
              dict(N=8, H=8, Ci=1024, Co=256, q32=True, bias=True, split=512), dict(N=8, H=8, Ci=512, Co=384, q32=False),
              dict(N=4, H=8, Ci=128, Co=96, q32=True, bias=True), dict(N=8, H=16, Ci=512, Co=128, q32=True, split=256),
              dict(N=2, H=8, Ci=64, Co=32, q32=False), dict(N=8, H=8, Ci=128, Co=512, q32=True, bias=True)]
    q = K.WgradQueue(group=8)
    checks = []
    for L in layers:
        N, H, Ci, Co, split = L["N"], L["H"], L["Ci"], L["Co"], L.get("split")
        x = torch.randn(N, Ci, H, H, generator=g).bfloat16()
        dy = torch.randn(N, Co, H, H, generator=g)
        dyq = dy.bfloat16()
        wq = torch.zeros(Co, Ci, 1, 1, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.double(), wq, None).backward(dyq.double())
        nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
        P, P2 = (nh(x[:, :split]), nh(x[:, split:])) if split else (nh(x), None)
        Q = nh(dy) if L["q32"] else nh(dyq)
        dW = torch.zeros(Ci * Co, device=DEV)
        db = torch.zeros(Co, device=DEV) if L.get("bias") else None
        q.push1x1(P, Q, dW, Ci=Ci, Cj=Co, hw=(H, H), mode=1, P2=P2, dbias=db)
        checks.append((dW, db, Ci, Co, wq.grad, dy.double().sum((0, 2, 3))))
    assert q.flushed == 8 and q.pushed == 10
    q.flush()
    torch.cuda.synchronize()
    assert q.flushed == 10
    for dW, db, Ci, Co, ref, bref in checks:
        got = dW.view(Ci, Co).t().cpu().double()
        assert rel_err(got, ref.view(Co, Ci)) < 2e-5, (Ci, Co)
        if db is not None:
            assert rel_err(db, bref) < 1e-5, (Ci, Co)


def test_conv1x1_wgrad_queue_fp32_mode(K):
    """Round 4: the exact-fp32 instantiation of the batched 1x1 weight-gradient kernel (Unet.compute_mode = "fp32": fp32 X and dY,
    v_mfma_f32_32x32x2_f32) -- to_qkv / to_out / res_conv shapes, a two-source layer, a ragged co tile, fused bias gradients -- against
    fp64 at the fp32 bar, and against the generic fp32 kernel it replaces."""
    g = torch.Generator().manual_seed(53)
    layers = [dict(N=8, H=32, Ci=128, Co=384), dict(N=8, H=32, Ci=128, Co=128, bias=True), dict(N=8, H=16, Ci=256, Co=384),
              dict(N=8, H=8, Ci=1024, Co=256, bias=True, split=512), dict(N=4, H=8, Ci=128, Co=96, bias=True),
              dict(N=8, H=16, Ci=512, Co=128, split=256), dict(N=2, H=8, Ci=64, Co=32), dict(N=8, H=8, Ci=128, Co=512, bias=True)]
    q = K.WgradQueue(group=8)
    checks = []
    K.PROBE = []
    try:
        for L in layers:
            N, H, Ci, Co, split = L["N"], L["H"], L["Ci"], L["Co"], L.get("split")
            x = torch.randn(N, Ci, H, H, generator=g)
            dy = torch.randn(N, Co, H, H, generator=g)
            wq = torch.zeros(Co, Ci, 1, 1, dtype=torch.float64, requires_grad=True)
            F.conv2d(x.double(), wq, None).backward(dy.double())
            nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
            X = nh(x)
            P, P2 = (X[..., :split], X[..., split:]) if split else (X, None)   # channel slices of one tensor: pixel stride Ci
            Q = nh(dy)
            dW = torch.full((Ci * Co,), 0.25, device=DEV)                      # the kernel accumulates
            db = torch.zeros(Co, device=DEV) if L.get("bias") else None
            q.push1x1(P, Q, dW, Ci=Ci, Cj=Co, hw=(H, H), mode=0, P2=P2, dbias=db)
            dWg = torch.zeros(Ci * Co, device=DEV)
            K.conv_wgrad(P, Q, dWg, kh=1, kw=1, stride=1, pad=0, gather_i=True, Ci=Ci, Cj=Co, grid_g=(H, H), grid_d=(H, H), mode=0, P2=P2)
            checks.append((dW, db, dWg, Ci, Co, wq.grad, dy.double().sum((0, 2, 3))))
        assert q.pushed == 8 and q.flushed == 8                                # every layer went to the queue (one launch of eight)
        torch.cuda.synchronize()
        seen = [p[0] for p in K.PROBE]
    finally:
        K.PROBE = None
    assert any("wgrad1x1_f32_kernel" in n for n in seen), seen
    for dW, db, dWg, Ci, Co, ref, bref in checks:
        got = (dW - 0.25).view(Ci, Co).t().cpu().double()
        assert rel_err(got, ref.view(Co, Ci)) < 2e-6, (Ci, Co)
        assert rel_err(dW - 0.25, dWg) < 2e-6, (Ci, Co)
        if db is not None:
            assert rel_err(db, bref) < 1e-5, (Ci, Co)


@pytest.mark.parametrize("shape", [(128, 32, 32, 128), (16, 16, 16, 256), (3, 8, 8, 64), (2, 8, 8, 1024), (5, 7, 9, 36)])
def test_to_bf16_with_column_sums(K, shape):
    """mi_f32_to_bf16_colsum: the bf16 copy equals torch's round-to-nearest-even, the column sums (added onto what is there) equal an
    fp64 sum -- full tensors (two-pass through the scratch buffer) and small ones (atomics), a channel slice as input, sums alone."""
    g = torch.Generator().manual_seed(59)
    N, H, W, Cc = shape
    full = torch.randn(N, H, W, 2 * Cc, generator=g).to(DEV)
    x = full[..., :Cc]                                                   # pixel stride 2C
    out = torch.full((Cc,), 0.5, device=DEV)
    y = K.to_bf16(x, colsum_out=out)
    ref = x.double().sum((0, 1, 2)).cpu() + 0.5
    assert torch.equal(y.cpu(), x.contiguous().bfloat16().cpu())
    assert float((out.double().cpu() - ref).abs().max()) < 2e-5 * float(x.abs().double().sum((0, 1, 2)).max()), shape
    out2 = torch.zeros(Cc, device=DEV)
    K.colsum(x, out2)
    assert float((out2.double().cpu() - (ref - 0.5)).abs().max()) < 2e-5 * float(x.abs().double().sum((0, 1, 2)).max()), shape


def test_stride2_wgrad_lds_dma_queue(K):
    """K.WgradQueue.push_s2: Downsample (3x3 / stride 2 conv) and Upsample (4x4 / stride 2 transposed conv) weight gradients through
    mi_conv_s2_wgrad_tr_batch -- the cfg-2 and cfg-3 layer shapes at a small batch, a ragged small-side channel count, image
    borders on every side -- against fp64 on the same bf16 operands; layers in one launch must not disturb each other."""
    g = torch.Generator().manual_seed(53)
    layers = [dict(kind="down", N=4, h=16, C=128), dict(kind="down", N=8, h=8, C=256), dict(kind="up", N=8, h=8, C=256),
              dict(kind="up", N=4, h=16, C=128), dict(kind="down", N=2, h=32, C=64), dict(kind="up", N=2, h=32, C=64),
              dict(kind="down", N=8, h=8, C=192, Co=96), dict(kind="up", N=8, h=8, C=96, Co=192), dict(kind="up", N=4, h=16, C=64),
              dict(kind="down", N=16, h=8, C=64)]
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
    q = K.WgradQueue(group=8)
    checks = []
    for L in layers:
        N, h, Ci, Co = L["N"], L["h"], L["C"], L.get("Co", L["C"])
        if L["kind"] == "down":
            x = torch.randn(N, Ci, 2 * h, 2 * h, generator=g).bfloat16()
            dy = torch.randn(N, Co, h, h, generator=g).bfloat16()
            w = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
            F.conv2d(x.double(), w, None, stride=2, padding=1).backward(dy.double())
            dW = torch.zeros(9 * Ci * Co, device=DEV)
            ok = q.push_s2(nh(x), nh(dy), dW, k=3, Ci=Ci, Cj=Co, gather_i=True, grid_g=(2 * h, 2 * h), grid_d=(h, h), mode=1)
            checks.append((dW, 3, Ci, Co, w.grad, False))
        else:
            x = torch.randn(N, Ci, h, h, generator=g).bfloat16()
            dy = torch.randn(N, Co, 2 * h, 2 * h, generator=g).bfloat16()
            w = torch.zeros(Ci, Co, 4, 4, dtype=torch.float64, requires_grad=True)
            F.conv_transpose2d(x.double(), w, None, stride=2, padding=1).backward(dy.double())
            dW = torch.zeros(16 * Ci * Co, device=DEV)
            ok = q.push_s2(nh(x), nh(dy), dW, k=4, Ci=Ci, Cj=Co, gather_i=False, grid_g=(2 * h, 2 * h), grid_d=(h, h), mode=1)
            checks.append((dW, 4, Ci, Co, w.grad, True))
        assert ok, L
    assert q.pushed == 10 and q.flushed == 8
    q.flush()
    torch.cuda.synchronize()
    assert q.flushed == 10
    for dW, k, Ci, Co, ref, tr in checks:
        assert rel_err(w_from_storage(dW.view(k, k, Ci, Co), transposed=tr), ref) < 2e-5, (k, Ci, Co)
    # fp32 operands and other geometries are refused (the caller falls back to conv_wgrad)
    assert not q.push_s2(torch.zeros(2, 16, 16, 64, device=DEV), torch.zeros(2, 8, 8, 64, device=DEV).bfloat16(), torch.zeros(9 * 64 * 64, device=DEV),
                         k=3, Ci=64, Cj=64, gather_i=True, grid_g=(16, 16), grid_d=(8, 8), mode=1)


def test_wgrad_queue_flushed_means_every_earlier_layer_is_out(K):
    """The gradient reducer releases a parameter range once `flushed` covers the layers pushed before it.  The two kinds flush
    independently: a full group of 1x1 layers going out must NOT count a 3x3 layer pushed before them as issued."""
    mk = lambda n, h, c: torch.randn(n, h, h, c, device=DEV).bfloat16()          # noqa: E731
    q = K.WgradQueue(group=8)
    x3, d3, w3 = mk(8, 16, 128), mk(8, 16, 128), torch.zeros(9 * 128 * 128, device=DEV)
    q.push(x3, d3, w3, Ci=128, Cj=128, hw=(16, 16), mode=1)                       # layer 1 (3x3) stays queued
    keep = []
    for _ in range(8):                                                            # layers 2..9 (1x1): the eighth triggers their launch
        x1, d1, w1 = mk(8, 16, 128), mk(8, 16, 128), torch.zeros(128 * 128, device=DEV)
        keep.append((x1, d1, w1))
        q.push1x1(x1, d1, w1, Ci=128, Cj=128, hw=(16, 16), mode=1)
    assert q.pushed == 9 and q.flushed == 0 and float(w3.abs().sum()) == 0.0
    assert all(float(w1.abs().sum()) > 0 for _, _, w1 in keep)
    q.flush()
    torch.cuda.synchronize()
    assert q.flushed == 9 and float(w3.abs().sum()) > 0


@pytest.mark.parametrize("group", [8, 3])
def test_conv3x3_wgrad_queue_batches_layers(K, group):
    """K.WgradQueue: several Block convs' weight gradients in ONE launch (mi_conv3x3_wgrad_tr_batch), each on its share of the
    workgroups -- mixed image sizes, a two-source layer, a layer with as many tiles as workgroups (adds into dW directly, no
    k-slices) and one the LDS-DMA kernel cannot take (32 input channels: runs at once through the register-staged kernel) -- against fp64 on the same bf16 operands."""
    g = torch.Generator().manual_seed(43)
    layers = [dict(N=8, H=32, W=32, Ci=128, Co=128), dict(N=8, H=16, W=16, Ci=256, Co=256), dict(N=8, H=8, W=8, Ci=512, Co=512),
              dict(N=8, H=8, W=8, Ci=1024, Co=256, split=512), dict(N=8, H=16, W=16, Ci=128, Co=256), dict(N=8, H=16, W=16, Ci=32, Co=64),
              dict(N=8, H=32, W=32, Ci=64, Co=128), dict(N=8, H=8, W=8, Ci=256, Co=512), dict(N=8, H=16, W=16, Ci=512, Co=128, split=256)]
    flushes = []
    q = K.WgradQueue(group=group, on_flush=lambda: flushes.append(q.flushed))
    refs, outs = [], []
    for L in layers:
        N, H, W, Ci, Co, split = L["N"], L["H"], L["W"], L["Ci"], L["Co"], L.get("split")
        x = torch.randn(N, Ci, H, W, generator=g).bfloat16()
        dy = torch.randn(N, Co, H, W, generator=g).bfloat16()
        wq = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.double(), wq, None, padding=1).backward(dy.double())
        nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
        P, P2 = (nh(x[:, :split]), nh(x[:, split:])) if split else (nh(x), None)
        dW = torch.zeros(9 * Ci * Co, device=DEV)
        q.push(P, nh(dy), dW, Ci=Ci, Cj=Co, hw=(H, W), mode=1, P2=P2)
        refs.append(wq.grad); outs.append((dW, Ci, Co))
    q.flush()
    torch.cuda.synchronize()
    assert q.pushed == q.flushed == 8 and flushes[-1] == 8 and len(flushes) >= (2 if group == 8 else 3)
    for (dW, Ci, Co), ref in zip(outs, refs):
        assert rel_err(w_from_storage(dW.view(3, 3, Ci, Co)), ref) < 2e-5, (Ci, Co)


@pytest.mark.parametrize("group", [8, 3])
def test_conv3x3_wgrad_queue_fp32_mode(K, group):
    """The exact-fp32 instantiation of the LDS-DMA weight-gradient kernel (wgrad_tr32_kernel: v_mfma_f32_32x32x2_f32, plain ds_read_b32
    of pixel-major fp32 tiles, the same k-slices / partial tiles / reduce / batching): Block conv weight gradients in fp32 mode --
    every image width incl. 64, a two-source layer, ragged co tiles, accumulation into a non-zero dW -- against fp64 at the fp32
    mode's bar; a second run with an odd workgroup count (odd slice boundaries: steps that start inside an image)."""
    g = torch.Generator().manual_seed(107)
    layers = [dict(N=8, H=32, W=32, Ci=128, Co=128), dict(N=8, H=16, W=16, Ci=256, Co=256), dict(N=8, H=8, W=8, Ci=512, Co=512),
              dict(N=8, H=8, W=8, Ci=1024, Co=256, split=512), dict(N=4, H=64, W=64, Ci=64, Co=64), dict(N=8, H=16, W=16, Ci=128, Co=96),
              dict(N=8, H=32, W=32, Ci=64, Co=32), dict(N=8, H=16, W=16, Ci=512, Co=128, split=256)]
    for blocks in (0, 203):
        K.load_library().mi_debug_wgrad_tr_blocks(blocks)
        try:
            q = K.WgradQueue(group=group)
            refs, outs = [], []
            K.PROBE = []
            for L in layers:
                N, H, W, Ci, Co, split = L["N"], L["H"], L["W"], L["Ci"], L["Co"], L.get("split")
                x = torch.randn(N, Ci, H, W, generator=g)
                dy = torch.randn(N, Co, H, W, generator=g)
                wq = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
                F.conv2d(x.double(), wq, None, padding=1).backward(dy.double())
                nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
                P, P2 = (nh(x[:, :split]), nh(x[:, split:])) if split else (nh(x), None)
                dW = torch.full((9 * Ci * Co,), 0.5, device=DEV)
                q.push(P, nh(dy), dW, Ci=Ci, Cj=Co, hw=(H, W), mode=0, P2=P2)
                refs.append(wq.grad); outs.append((dW, Ci, Co))
            q.flush()
            torch.cuda.synchronize()
            names = [p_[0] for p_ in K.PROBE]
        finally:
            K.PROBE = None
            K.load_library().mi_debug_wgrad_tr_blocks(0)
        assert q.pushed == q.flushed == len(layers) and "wgrad_tr32_kernel" in names and not any(n.startswith("wgrad_kernel") for n in names), names
        for (dW, Ci, Co), ref in zip(outs, refs):
            assert rel_err(w_from_storage((dW - 0.5).view(3, 3, Ci, Co)), ref) < 3e-6, (Ci, Co, blocks)


@pytest.mark.parametrize("cfg", [
    dict(N=8, H=32, Ci=128, Co=384),             # to_qkv at level 0 (256-pixel tiles)
    dict(N=2, H=16, Ci=256, Co=128, split=128),  # res_conv on the skip concat
    dict(N=3, H=7, Ci=64, Co=96),                # ragged M (147 pixels) and ragged N tile
    dict(N=4, H=8, Ci=128, Co=512, residual=True),
])
def test_conv1x1_bf16w_fwd_and_dgrad(K, cfg):
    """1x1 convs (to_qkv / to_out / res_conv, ddpm.py:134,151-152) and their dgrad through the pipelined kernel."""
    N, H, Ci, Co = cfg["N"], cfg["H"], cfg["Ci"], cfg["Co"]
    split = cfg.get("split")
    g = torch.Generator().manual_seed(37)
    x = torch.randn(N, Ci, H, H, generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(Co, Ci, 1, 1, generator=g, dtype=torch.float64) / math.sqrt(Ci)).requires_grad_(True)
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    r = torch.randn(N, Co, H, H, generator=g, dtype=torch.float64) if cfg.get("residual") else None
    y = F.conv2d(x, w, b) + (r if r is not None else 0)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    flat, wd, wf, offs = _pack(K, [conv_w_storage(w.detach())])
    if split:
        xa, xb = to_nhwc_gpu(x.detach()[:, :split].float()), to_nhwc_gpu(x.detach()[:, split:].float())
    else:
        xa, xb = to_nhwc_gpu(x.detach().float()), None
    yg = K.conv3x3_bf16w(xa, wf, K=Ci, Nc=Co, flip=False, ksize=1, x2=xb, bias=b.float().to(DEV),
                         residual=to_nhwc_gpu(r.float()) if r is not None else None)
    assert yg is not None
    dxg = K.conv3x3_bf16w(to_nhwc_gpu(dy.float()), wd, K=Co, Nc=Ci, flip=True, ksize=1)
    torch.cuda.synchronize()
    xq, wq = x.detach().float().bfloat16().double(), w.detach().float().bfloat16().double()
    yq = F.conv2d(xq, wq, b) + (r if r is not None else 0)
    assert rel_err(from_nhwc(yg), yq) < 1e-5 and rel_err(from_nhwc(yg), y) < 2e-2
    assert rel_err(from_nhwc(dxg), x.grad) < 2e-2


@pytest.mark.parametrize("cfg", [dict(N=8, H=32, Ci=128, Co=384), dict(N=16, H=8, Ci=512, Co=128),
                                 dict(N=8, H=16, Ci=256, Co=64, split=128), dict(N=8, H=4, Ci=32, Co=96)])
def test_conv1x1_wgrad_fast(K, cfg):
    """Weight gradient of the 1x1 convs through the image-major MFMA kernel."""
    N, H, Ci, Co = cfg["N"], cfg["H"], cfg["Ci"], cfg["Co"]
    split = cfg.get("split")
    g = torch.Generator().manual_seed(41)
    x = torch.randn(N, Ci, H, H, generator=g, dtype=torch.float64)
    dy = torch.randn(N, Co, H, H, generator=g, dtype=torch.float64)
    xq, dq = x.float().bfloat16().double(), dy.float().bfloat16().double()
    ref = torch.einsum("nchw,nkhw->kc", xq, dq)[:, :, None, None]          # [Co,Ci,1,1]
    dW = torch.zeros(Ci * Co, device=DEV)
    P, P2 = (to_nhwc_gpu(x[:, :split].float()), to_nhwc_gpu(x[:, split:].float())) if split else (to_nhwc_gpu(x.float()), None)
    from src.ops.lib import MiWgradDesc, load_library
    import ctypes
    d = MiWgradDesc(N=N, GH=H, GW=H, DH=H, DW=H, Ci=Ci, Cj=Co, KH=1, KW=1, stride=1, pad=0, gather_i=1, mode=1,
                    I1=split or Ci, ldp=4, ldp2=4, ldq=4)
    assert load_library().mi_conv3x3_wgrad_supported(ctypes.byref(d)) == 1
    db = torch.zeros(Co, device=DEV)
    K.conv_wgrad(P, to_nhwc_gpu(dy.float()), dW, kh=1, kw=1, stride=1, pad=0, gather_i=True, Ci=Ci, Cj=Co,
                 grid_g=(H, H), grid_d=(H, H), mode=1, P2=P2, dbias=db)
    torch.cuda.synchronize()
    assert rel_err(db, dy.sum((0, 2, 3))) < 1e-5
    assert rel_err(w_from_storage(dW.view(1, 1, Ci, Co)), ref) < 2e-5


@pytest.mark.parametrize("cfg", [dict(N=3, H=8, C=64, ks=3), dict(N=8, H=16, C=128, ks=3), dict(N=4, H=8, C=128, ks=1),
                                 dict(N=2, H=7, C=64, ks=3), dict(N=5, H=8, C=256, ks=1)])
def test_small_channel_ends(K, cfg):
    """First convs Conv2d(3, C, 3, padding=1) / res_conv Conv2d(3, C, 1) and final Conv2d(C, 3, 1) (ddpm.py:134,208,236):
    fwd / dgrad / wgrad; H = 7 exercises the non-power-of-two pixel decode."""
    g = torch.Generator().manual_seed(43)
    N, H, C, ks = cfg["N"], cfg["H"], cfg["C"], cfg["ks"]
    x = torch.randn(N, 3, H, H, generator=g, dtype=torch.float64)
    w = torch.randn(C, 3, ks, ks, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(C, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, b, padding=ks // 2)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    xg = to_nhwc_gpu(x.float())
    assert K.small_cin_supported(ks, 3, C) and K.small_cin_supported(ks, 3, C, wgrad=True)
    yg = K.conv_small_cin_fwd(xg, conv_w_storage(w.detach()), b.float().to(DEV), C, ks)
    dW = torch.full((ks * ks * 3 * C,), 0.5, device=DEV)          # the kernel accumulates
    K.conv_small_cin_wgrad(xg, to_nhwc_gpu(dy.float()), dW, ks)
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(yg), y) < 1e-5
    assert rel_err(w_from_storage((dW - 0.5).view(ks, ks, 3, C)), w.grad) < 1e-5
    if C > 128:
        return
    # final conv
    h = torch.randn(N, C, H, H, generator=g, dtype=torch.float64, requires_grad=True)
    wf = torch.randn(3, C, 1, 1, generator=g, dtype=torch.float64, requires_grad=True)
    bf = torch.randn(3, generator=g, dtype=torch.float64)
    e = F.conv2d(h, wf, bf)
    de = torch.randn(e.shape, generator=g, dtype=torch.float64)
    e.backward(de)
    hg, ws = to_nhwc_gpu(h.detach().float()), conv_w_storage(wf.detach())
    eg = K.conv1x1_small_cout(0, hg, ws, bias=bf.float().to(DEV), Cs=3)
    assert eg.shape == (N, H, H, 3) and eg.stride(2) == 4
    deg = to_nhwc_gpu(de.float())
    dh = torch.empty(N, H, H, C, device=DEV)
    K.conv1x1_small_cout(1, deg, ws, out=dh)
    dWf = torch.zeros(C * 3, device=DEV)
    K.conv1x1_small_cout(2, hg, None, b=deg, out=dWf)
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(eg), e) < 1e-5
    assert rel_err(from_nhwc(dh), h.grad) < 1e-5
    assert rel_err(w_from_storage(dWf.view(1, 1, C, 3)), wf.grad) < 1e-5
    K.conv1x1_small_cout(1, deg, ws, out=dh, accumulate=True)
    assert rel_err(from_nhwc(dh), 2 * h.grad) < 1e-5


@pytest.mark.parametrize("N,H,C", [(8, 16, 128), (2, 32, 128), (4, 8, 256), (2, 64, 64)])
def test_small_channel_ends_bf16_wide_tensor(K, N, H, C):
    """Round 4: the wide tensor at the 3-channel ends stored as bf16.  Same fp32 arithmetic as the fp32-stored kernels: a bf16 output is
    the fp32 kernel's output rounded once (bitwise), a bf16 input gives exactly what its widened fp32 copy gives."""
    BF = torch.bfloat16
    g = torch.Generator().manual_seed(45)
    x = to_nhwc_gpu(torch.randn(N, 3, H, H, generator=g))
    w = torch.randn(3 * 3 * 3 * C, generator=g).to(DEV) * 0.2
    b = torch.randn(C, generator=g).to(DEV)
    if C > 128:                                                   # (the 3x3 weight gradient takes Cout <= 128: 48 KB of reduce area)
        assert not K.small_cin_bf16_supported(3, N, H, H, 3, C, 4) and not K.small_cin_supported(3, 3, C, wgrad=True)
        return
    assert K.small_cin_bf16_supported(3, N, H, H, 3, C, 4)
    y32 = K.conv_small_cin_fwd(x, w, b, C, 3)
    y16 = K.conv_small_cin_fwd(x, w, b, C, 3, out_dtype=BF)
    assert y16.dtype == BF and torch.equal(y16, y32.to(BF))
    dy16 = to_nhwc_gpu(torch.randn(N, C, H, H, generator=g)).to(BF)
    dWa, dWb = torch.zeros(27 * C, device=DEV), torch.zeros(27 * C, device=DEV)
    K.conv_small_cin_wgrad(x, dy16, dWa, 3)
    K.conv_small_cin_wgrad(x, dy16.float(), dWb, 3)
    if C >= 128:
        assert torch.equal(dWa, dWb)
    else:                                                         # (64 channels: fp32 dy takes the untiled kernel -- another summation order)
        assert rel_err(dWa, dWb) < 2e-6
    # final conv: x (op 0 / 2) and dx (op 1) as bf16
    h16 = to_nhwc_gpu(torch.randn(N, C, H, H, generator=g)).to(BF)
    wf = torch.randn(C * 3, generator=g).to(DEV) * 0.1
    bf_ = torch.randn(3, generator=g).to(DEV)
    de = to_nhwc_gpu(torch.randn(N, 3, H, H, generator=g))
    assert torch.equal(K.conv1x1_small_cout(0, h16, wf, bias=bf_, Cs=3), K.conv1x1_small_cout(0, h16.float(), wf, bias=bf_, Cs=3))
    dWa, dWb = torch.zeros(C * 3, device=DEV), torch.zeros(C * 3, device=DEV)
    K.conv1x1_small_cout(2, h16, None, b=de, out=dWa)
    K.conv1x1_small_cout(2, h16.float(), None, b=de, out=dWb)
    assert torch.equal(dWa, dWb)
    dh32 = torch.empty(N, H, H, C, device=DEV)
    dh16 = torch.empty(N, H, H, C, device=DEV, dtype=BF)
    K.conv1x1_small_cout(1, de, wf, out=dh32)
    K.conv1x1_small_cout(1, de, wf, out=dh16)
    assert torch.equal(dh16, dh32.to(BF))
    K.conv1x1_small_cout(1, de, wf, out=dh16, accumulate=True)    # += into the bf16 tensor: widened, added in fp32, rounded again
    assert torch.equal(dh16, (dh32.to(BF).float() + dh32).to(BF))
    # round 6: weight gradient and data gradient from ONE pass over (x, dy) (mi_conv1x1_small_cout_bwd): bitwise the two launches' results
    for xin, dt in ((h16, BF), (h16.float(), torch.float32)):
        dWc = torch.zeros(C * 3, device=DEV); dhc = torch.full((N, H, H, C), float("nan"), device=DEV, dtype=dt)
        K.conv1x1_small_cout_bwd(xin, de, wf, dWc, dhc)
        assert torch.equal(dWc, dWa) and torch.equal(dhc, dh32.to(dt))
        K.conv1x1_small_cout_bwd(xin, de, wf, dWc, dhc, accumulate=True)
        assert torch.equal(dhc, (dh32.to(dt).float() + dh32).to(dt)) and torch.equal(dWc, dWa + dWa)


@pytest.mark.parametrize("N,H,C,G", [(8, 32, 128, 8), (64, 32, 128, 8), (3, 16, 128, 4), (4, 16, 64, 4), (2, 6, 128, 8)])
def test_final_conv_groupnorm_mish_in_the_load(K, N, H, C, G):
    """mi_conv1x1_small_cout_gn_fwd (round 6, inference): final_conv = Block(conv -> GroupNorm -> Mish) -> Conv2d(dim, 3, 1) (reference
    ddpm.py:232-235) with the GroupNorm-apply + Mish inside the 1x1 conv's load, statistics from the epilogue sums of the Block's conv.  Against fp64
    on the stored bf16 tensor, and against the two launches it replaces (which round the normalised tensor to bf16 in between)."""
    g = torch.Generator().manual_seed(67)
    x = (torch.randn(N, H, H, C, generator=g) * 1.3 + 0.2).to(DEV).bfloat16()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.3).to(DEV)
    w = (torch.randn(C * 3, generator=g) * 0.1).to(DEV); b = torch.randn(3, generator=g).to(DEV)
    assert K.small_cout_gn_supported(C, 3, G)
    xd = x.double().view(N, H * H, C // 16, 16)
    sums = K.gn_sums_encode(torch.stack([xd.sum((1, 3)), (xd * xd).sum((1, 3))], dim=-1))
    y = K.conv1x1_small_cout_gn(x, sums, gamma, beta, w, b, 3, groups=G)
    torch.cuda.synchronize()
    assert y.shape == (N, H, H, 3) and not y.untyped_storage().nbytes() % 16 and float(y.as_strided((N, H, H, 4), (H * H * 4, H * 4, 4, 1))[..., 3].abs().max()) == 0.0
    x64 = x.double().cpu().permute(0, 3, 1, 2)
    hn = _mish64(F.group_norm(x64, G, gamma.double().cpu(), beta.double().cpu(), 1e-5))
    ref = F.conv2d(hn, w.double().cpu().view(C, 3).t().reshape(3, C, 1, 1), b.double().cpu()).permute(0, 2, 3, 1)
    assert rel_err(y.cpu(), ref) < 2e-5
    if (C // G) in (16, 32, 64) and C // G <= 128 // 8 * 8 and G == 8:
        h16, _ = K.gn_mish_fwd(x, gamma, beta, out_dtype=torch.bfloat16)
        y2 = K.conv1x1_small_cout(0, h16, w, bias=b, Cs=3)
        torch.cuda.synchronize()
        assert rel_err(y2.cpu(), ref) < 4e-3 and rel_err(y.cpu(), y2.cpu().double()) < 4e-3
        # (the plain 128 -> 3 kernel writes the padding channel of its 4-channel pixels as well: no fill in front of it)
        assert float(y2.as_strided((N, H, H, 4), (H * H * 4, H * 4, 4, 1))[..., 3].abs().max()) == 0.0


@pytest.mark.parametrize("N,H,C", [(8, 32, 128), (2, 16, 128), (4, 64, 64), (2, 8, 256)])
@pytest.mark.parametrize("out16", [False, True])
def test_small_cin_block_conv_and_res_conv_in_one_launch(K, N, H, C, out16):
    """mi_conv_small_cin_fwd_dual (round 6): the image -> features ResnetBlock's 3x3 conv and its res_conv (Conv2d(3, C, 1), reference
    ddpm.py:134,143) from one pass over the image.  Same FMA chains as the two kernels it replaces: bitwise their outputs."""
    BF = torch.bfloat16
    g = torch.Generator().manual_seed(61)
    x = to_nhwc_gpu(torch.randn(N, 3, H, H, generator=g))
    w3 = torch.randn(3 * 3 * 3 * C, generator=g).to(DEV) * 0.2; b3 = torch.randn(C, generator=g).to(DEV)
    w1 = torch.randn(3 * C, generator=g).to(DEV) * 0.5; b1 = torch.randn(C, generator=g).to(DEV)
    if out16 and not K.small_cin_bf16_supported(3, N, H, H, 3, C, 4):
        pytest.skip("bf16 output: Cout <= 128")
    assert K.small_cin_dual_supported(N, H, H, 3, C, K.ld_of(x))
    dt = BF if out16 else torch.float32
    y3, y1 = K.conv_small_cin_fwd_dual(x, w3, b3, w1, b1, C, out_dtype=dt)
    r3 = K.conv_small_cin_fwd(x, w3, b3, C, 3, out_dtype=dt)
    r1 = K.conv_small_cin_fwd(x, w1, b1, C, 1)
    torch.cuda.synchronize()
    assert y3.dtype == dt and y1.dtype == torch.float32
    assert torch.equal(y3, r3)
    assert torch.equal(y1, r1) or rel_err(y1, r1) < 2e-7
    # the chores of a forward's first launch: clear the pool of GroupNorm sums, gather the step's time-bias rows
    pool = torch.full((1001,), 7, device=DEV, dtype=torch.int64)
    table = torch.randn(50, 132, generator=g).to(DEV); idx = torch.randint(0, 50, (N,), generator=g).to(DEV)
    rows = torch.full((N, 132), float("nan"), device=DEV)
    y3b, y1b = K.conv_small_cin_fwd_dual(x, w3, b3, w1, b1, C, out_dtype=dt, zero=pool, gather=(table, idx, rows))
    torch.cuda.synchronize()
    assert torch.equal(y3b, y3) and torch.equal(y1b, y1) and not pool.any() and torch.equal(rows, table[idx])
    xd = from_nhwc(x).double()
    ref1 = F.conv2d(xd, w1.double().cpu().view(3, C).t().reshape(C, 3, 1, 1), b1.double().cpu())
    assert rel_err(from_nhwc(y1), ref1) < 2e-6


@pytest.mark.parametrize("kind", ["down", "down_dgrad", "up", "up_dgrad"])
def test_igemm_bf16_weight_copy(K, kind):
    """Stride-2 Downsample / ConvTranspose Upsample (ddpm.py:70,79) through the generic kernel fed by the bf16 weight copy."""
    g = torch.Generator().manual_seed(47)
    N, C, H = 2, 64, 16
    if kind.startswith("down"):
        x = torch.randn(N, C, H, H, generator=g, dtype=torch.float64, requires_grad=True)
        w = (torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64) / 24).requires_grad_(True)
        y = F.conv2d(x, w, None, stride=2, padding=1)
        ws = conv_w_storage(w.detach()); kk = 3
    else:
        x = torch.randn(N, C, H // 2, H // 2, generator=g, dtype=torch.float64, requires_grad=True)
        w = (torch.randn(C, C, 4, 4, generator=g, dtype=torch.float64) / 32).requires_grad_(True)
        y = F.conv_transpose2d(x, w, None, stride=2, padding=1)
        ws = conv_w_storage(w.detach(), transposed=True); kk = 4
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    flat, wd, wf, offs = _pack(K, [ws])
    xg, dyg = to_nhwc_gpu(x.detach().float()), to_nhwc_gpu(dy.float())
    ih, oh = x.shape[2], y.shape[2]
    if kind == "down":
        out = K.conv_igemm(xg, ws, kh=3, kw=3, stride=2, pad=1, transposed=False, w_kn=True, K=C, Nc=C, out_hw=(oh, oh), mode=1, wb=wf)
        ref = y
    elif kind == "down_dgrad":
        out = K.conv_igemm(dyg, ws, kh=3, kw=3, stride=2, pad=1, transposed=True, w_kn=False, K=C, Nc=C, out_hw=(ih, ih), mode=1, wb=wd)
        ref = x.grad
    elif kind == "up":
        out = K.conv_igemm(xg, ws, kh=4, kw=4, stride=2, pad=1, transposed=True, w_kn=True, K=C, Nc=C, out_hw=(oh, oh), mode=1, wb=wf)
        ref = y
    else:
        out = K.conv_igemm(dyg, ws, kh=4, kw=4, stride=2, pad=1, transposed=False, w_kn=False, K=C, Nc=C, out_hw=(ih, ih), mode=1, wb=wd)
        ref = x.grad
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(out), ref) < 2e-2


def test_bf16_block_storage_kernels(K):
    """bf16-stored block-internal tensors: halo conv (bf16 in/out), GroupNorm+Mish fwd/bwd (bf16 x / y / dout / dx) and
    the image-major wgrad (bf16 P / Q) against fp64 evaluations of the same bf16-rounded tensors."""
    g = torch.Generator().manual_seed(53)
    N, H, C = 8, 16, 64
    BF = torch.bfloat16

    def q(t):                      # value after bf16 storage
        return t.float().bfloat16().double()
    x = torch.randn(N, C, H, H, generator=g, dtype=torch.float64)
    w = torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64) / 24
    flat, wd, wf, offs = _pack(K, [conv_w_storage(w)])
    x16 = to_nhwc_gpu(x.float()).contiguous().to(BF)
    # conv: bf16 in -> bf16 out, fp32 in -> bf16 out, bf16 in -> fp32 out
    ref = F.conv2d(q(x), q(w), None, padding=1)
    for xin, od in ((x16, BF), (to_nhwc_gpu(x.float()), BF), (x16, torch.float32)):
        y = K.conv3x3_bf16w(xin, wf, K=C, Nc=C, flip=False, out_dtype=od)
        assert y.dtype == od
        tol = 6e-3 if od == BF else 1e-5
        assert rel_err(from_nhwc(y.float()), ref) < tol, (xin.dtype, od)
    # accumulate into a bf16 gradient buffer
    y0 = K.conv3x3_bf16w(x16, wd, K=C, Nc=C, flip=True, out_dtype=BF)
    y1 = K.conv3x3_bf16w(x16, wd, K=C, Nc=C, flip=True, out=y0.clone(), accumulate=True)
    assert rel_err(y1.float(), 2 * y0.float()) < 6e-3
    # GroupNorm + Mish
    c = (torch.randn(N, C, H, H, generator=g, dtype=torch.float64) * 2).requires_grad_(False)
    gamma = torch.randn(C, generator=g, dtype=torch.float64) + 1
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    cq = q(c).requires_grad_(True)
    yref = (F.group_norm(cq, 8, gamma, beta) * torch.tanh(F.softplus(F.group_norm(cq, 8, gamma, beta))))
    dy = torch.randn(N, C, H, H, generator=g, dtype=torch.float64)
    yref.backward(q(dy))
    c16 = to_nhwc_gpu(c.float()).contiguous().to(BF)
    ga, be = gamma.float().to(DEV), beta.float().to(DEV)
    y16, st = K.gn_mish_fwd(c16, ga, be, out_dtype=BF)
    assert y16.dtype == BF and rel_err(from_nhwc(y16.float()), yref) < 6e-3
    y32, _ = K.gn_mish_fwd(c16, ga, be)
    assert y32.dtype == torch.float32 and rel_err(from_nhwc(y32), yref) < 1e-5
    dy16 = to_nhwc_gpu(dy.float()).contiguous().to(BF)
    dga, dbe = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx16 = K.gn_mish_bwd(c16, st, ga, be, dy16, dgamma=dga, dbeta=dbe, out_dtype=BF)
    assert dx16.dtype == BF and rel_err(from_nhwc(dx16.float()), cq.grad) < 8e-3
    dx32 = K.gn_mish_bwd(c16, st, ga, be, dy16)
    assert rel_err(from_nhwc(dx32), cq.grad) < 5e-5
    # wgrad with bf16 P and Q
    dyq = torch.randn(N, C, H, H, generator=g, dtype=torch.float64)
    wz = torch.zeros(C, C, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(q(x), wz, None, padding=1).backward(q(dyq))
    for P, Q in ((x16, to_nhwc_gpu(dyq.float()).contiguous().to(BF)), (to_nhwc_gpu(x.float()), to_nhwc_gpu(dyq.float()).contiguous().to(BF)),
                 (x16, to_nhwc_gpu(dyq.float()))):
        dW = torch.zeros(9 * C * C, device=DEV); db = torch.zeros(C, device=DEV)
        K.conv_wgrad(P, Q, dW, kh=3, kw=3, stride=1, pad=1, gather_i=True, Ci=C, Cj=C, grid_g=(H, H), grid_d=(H, H), mode=1, dbias=db)
        torch.cuda.synchronize()
        assert rel_err(w_from_storage(dW.view(3, 3, C, C)), wz.grad) < 2e-5, (P.dtype, Q.dtype)
        assert rel_err(db, (q(dyq) if Q.dtype == BF else dyq).sum((0, 2, 3))) < 1e-5     # bias sums use the stored values


@pytest.mark.parametrize("dout16", [True, False])
def test_gn_bwd_4096_pixel_slices_bf16(K, dout16):
    """Round 4: GroupNorm backward on the 64 x 64 level of cfg 3 (C / G = 8, 4096-pixel slices: 32 units of 4-channel lanes, more than
    the register cache holds) runs on 8-channel lanes with a 16-unit packed cache (gn_mish_bwd_kernel<8, 16>) instead of the uncached
    two-pass form: against fp64 on the bf16-stored operands; dout bf16 (block-internal) and fp32 (residual-stream gradient)."""
    g = torch.Generator().manual_seed(71)
    N, H, C = 4, 64, 64
    BF = torch.bfloat16

    def q(t):
        return t.float().bfloat16().double()
    c = torch.randn(N, C, H, H, generator=g, dtype=torch.float64) * 2 + 0.3
    gamma = (torch.randn(C, generator=g, dtype=torch.float64) + 1).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_(True)
    temb = torch.randn(N, C, generator=g, dtype=torch.float64).requires_grad_(True)
    cq = q(c).requires_grad_(True)
    h = F.group_norm(cq, 8, gamma, beta)
    yref = h * torch.tanh(F.softplus(h)) + temb[:, :, None, None]
    dy = torch.randn(N, C, H, H, generator=g, dtype=torch.float64)
    dyq = q(dy) if dout16 else dy.float().double()
    yref.backward(dyq)
    c16 = to_nhwc_gpu(c.float()).contiguous().to(BF)
    ga, be = gamma.detach().float().to(DEV), beta.detach().float().to(DEV)
    _, st = K.gn_mish_fwd(c16, ga, be, temb=temb.detach().float().to(DEV), out_dtype=BF)
    dyg = to_nhwc_gpu(dy.float()).contiguous()
    dyg = dyg.to(BF) if dout16 else dyg
    dga, dbe, dbias = (torch.zeros(C, device=DEV) for _ in range(3))
    dtemb = torch.zeros(N, C, device=DEV)
    K.PROBE = []
    try:
        dx = K.gn_mish_bwd(c16, st, ga, be, dyg, dgamma=dga, dbeta=dbe, dtemb=dtemb, dbias=dbias, out_dtype=BF)
        torch.cuda.synchronize()
    finally:
        K.PROBE = None
    assert dx.dtype == BF and rel_err(from_nhwc(dx.float()), cq.grad) < 8e-3
    assert rel_err(dga, gamma.grad) < 2e-3 and rel_err(dbe, beta.grad) < 2e-3 and rel_err(dtemb, temb.grad) < 2e-3
    assert max_err(dbias, cq.grad.sum((0, 2, 3))) < 2e-2 * float(cq.grad.abs().sum((0, 2, 3)).max()) / 10


def test_bf16_attention_storage_kernels(K):
    """bf16 storage of the attention-internal tensors: the 1x1 tile kernel / 1x1 weight gradient with bf16 operands,
    LayerNorm writing bf16 / reading a bf16 gradient, and the LinearAttention core on bf16 qkv -- each against the
    fp32-storage kernel on the same (bf16-rounded) values."""
    BF = torch.bfloat16
    g = torch.Generator().manual_seed(53)
    N, H, C, HID = 8, 8, 128, 128
    q = lambda t: t.float().bfloat16().float()
    # LayerNorm
    x = to_nhwc_gpu(torch.randn(N, C, H, H, generator=g))
    gam, bet = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    y32 = K.chan_layernorm_fwd(x, gam, bet)
    y16 = K.chan_layernorm_fwd(x, gam, bet, out_dtype=BF)
    assert y16.dtype == BF and rel_err(y16.float(), y32) < 4e-3
    dy = to_nhwc_gpu(torch.randn(N, C, H, H, generator=g))
    dy16 = dy.to(BF)
    dx_a, dx_b = torch.empty_like(x), torch.empty_like(x)
    dg_a, db_a, dg_b, db_b = (torch.zeros(C, device=DEV) for _ in range(4))
    K.chan_layernorm_bwd(x, gam, dy16.float(), dx_a, False, dg_a, db_a)
    K.chan_layernorm_bwd(x, gam, dy16, dx_b, False, dg_b, db_b)
    assert rel_err(dx_b, dx_a) < 1e-6 and rel_err(dg_b, dg_a) < 1e-5 and rel_err(db_b, db_a) < 1e-5
    # 1x1 conv C -> 3*HID with every storage combination, and its weight gradient
    w = torch.randn(3 * HID, C, 1, 1, generator=g, dtype=torch.float64) / math.sqrt(C)
    flat, wd, wf, offs = _pack(K, [conv_w_storage(w)])
    ref = K.conv3x3_bf16w(q(x), wf, K=C, Nc=3 * HID, flip=False, ksize=1)
    for xin, od in ((x.to(BF), BF), (x.to(BF), torch.float32), (q(x), BF)):
        y = K.conv3x3_bf16w(xin, wf, K=C, Nc=3 * HID, flip=False, ksize=1, out_dtype=od)
        assert y.dtype == od and rel_err(y.float(), ref) < (4e-3 if od == BF else 1e-6)
    dq = to_nhwc_gpu(torch.randn(N, 3 * HID, H, H, generator=g))
    dW_ref = torch.zeros(C * 3 * HID, device=DEV)
    K.conv_wgrad(q(x), q(dq), dW_ref, kh=1, kw=1, stride=1, pad=0, gather_i=True, Ci=C, Cj=3 * HID, grid_g=(H, H), grid_d=(H, H), mode=1)
    for P, Q in ((x.to(BF), dq.to(BF)), (x.to(BF), q(dq)), (q(x), dq.to(BF))):
        dW = torch.zeros(C * 3 * HID, device=DEV)
        K.conv_wgrad(P, Q, dW, kh=1, kw=1, stride=1, pad=0, gather_i=True, Ci=C, Cj=3 * HID, grid_g=(H, H), grid_d=(H, H), mode=1)
        assert rel_err(dW, dW_ref) < 2e-5, (P.dtype, Q.dtype)
    # LinearAttention core
    qkv = to_nhwc_gpu(torch.randn(N, 3 * HID, H, H, generator=g))
    qkv16 = qkv.to(BF)
    o32, ctx32, ks32 = K.linattn_fwd(qkv16.float())
    o16, ctx16, ks16 = K.linattn_fwd(qkv16)
    # bf16 tensors: every product on the bf16 MFMA (exp(k - max) rounded where it is parked) -- ctx carries one bf16 rounding per term
    assert o16.dtype == BF and rel_err(ctx16, ctx32) < 2.5e-3 and rel_err(ks16, ks32) < 1e-6 and rel_err(o16.float(), o32) < 4e-3
    do = to_nhwc_gpu(torch.randn(N, HID, H, H, generator=g)).to(BF)
    d32 = K.linattn_bwd(qkv16.float(), ctx32, ks32, do.float())
    d16 = K.linattn_bwd(qkv16, ctx16, ks16, do)
    assert d16.dtype == BF and rel_err(d16.float(), d32) < 4e-3


@pytest.mark.parametrize("N,H,C,want16", [(64, 32, 128, True), (8, 32, 128, False), (64, 16, 256, True), (64, 8, 512, False), (2, 8, 64, False), (3, 16, 320, True)])
def test_linear_attention_folded_into_to_out(K, N, H, C, want16):
    """mi_linattn_fold_fwd + mi_conv1x1_pw_batched (round 6, inference): LinearAttention (reference ddpm.py:146-165) + to_out + the Residual add
    without the attention output -- out = ctx^T q is linear in q, so to_out(out) = (W_out blockdiag(ctx_h^T)) q: a 1x1 conv of q with per-sample
    weights.  Against fp64 on the stored bf16 qkv, and against the launches it replaces (linattn_fwd -> bf16 attention output -> to_out)."""
    BF = torch.bfloat16
    heads, HID = 4, 128
    g = torch.Generator().manual_seed(83 + C)
    qkv = (torch.randn(N, H, H, 3 * HID, generator=g) * 0.8).to(DEV).to(BF)
    w = (torch.randn(C, HID, generator=g) / math.sqrt(HID))
    bias = torch.randn(C, generator=g).to(DEV); res = torch.randn(N, H, H, C, generator=g).to(DEV)
    flat, wd, wf, offs, wdq, wfq = _pack(K, [conv_w_storage(w.double().view(C, HID, 1, 1))], frag=True)      # wf: bf16 rows [co][ci]
    r = K.linattn_to_out_folded(qkv, wf, C, bias, res, heads=heads, want16=want16)
    if K._linattn_ws(N, H * H, heads) or C % 64:                      # few (sample, head) pairs: the pixel axis is sliced -- the fold takes whole images only
        assert r is None
        return
    assert r is not None, "shape not taken"
    y = r[0] if want16 else r
    torch.cuda.synchronize()
    q64 = qkv.double().cpu().view(N, H * H, 3, heads, 32)
    qd, kd, vd = q64[:, :, 0], q64[:, :, 1], q64[:, :, 2]              # [N][n][h][d]
    P = torch.softmax(kd, dim=1)
    ctx = torch.einsum("bnhd,bnhe->bhde", P, vd)
    out = torch.einsum("bhde,bnhd->bnhe", ctx, qd).reshape(N, H, H, HID)
    ref = torch.einsum("bhwk,ck->bhwc", out, w.bfloat16().double()) + bias.double().cpu() + res.double().cpu()
    assert rel_err(y.cpu(), ref) < 4e-3
    if want16:
        assert torch.equal(r[1], y.to(BF))
    # the launches it replaces
    ao, _, _ = K.linattn_fwd(qkv, heads)
    y2 = K.conv3x3_bf16w(ao, wf, K=HID, Nc=C, flip=False, ksize=1, bias=bias, residual=res, wq=wfq)
    torch.cuda.synchronize()
    assert rel_err(y2.cpu(), ref) < 4e-3 and rel_err(y.cpu(), y2.cpu().double()) < 4e-3


@pytest.mark.parametrize("M,N,Kc", [(128, 512, 128), (128, 128, 512), (128, 3584, 128), (96, 200, 64)])
def test_small_gemm_linear(K, M, N, Kc):
    """nn.Linear of the time MLP through mi_small_gemm: forward, input gradient, weight gradient (exact fp32)."""
    g = torch.Generator().manual_seed(61)
    x = torch.randn(M, Kc, generator=g, dtype=torch.float64)
    w = torch.randn(N, Kc, generator=g, dtype=torch.float64) / math.sqrt(Kc)
    b = torch.randn(N, generator=g, dtype=torch.float64)
    dy = torch.randn(M, N, generator=g, dtype=torch.float64)
    xg, wg, bg, dyg = (t.float().to(DEV) for t in (x, w, b, dy))
    y = K.small_gemm(False, True, xg, wg, bias=bg)
    assert y is not None and rel_err(y, x @ w.t() + b) < 2e-6
    y2 = K.small_gemm(False, True, xg, wg, bias=bg)
    assert torch.equal(y, y2)                                                         # forward: no split, bit-reproducible
    dx = K.small_gemm(False, False, dyg, wg, allow_split=True)
    if N % 32:
        assert dx is None                                                             # contraction not a multiple of 32
    else:
        assert rel_err(dx, dy @ w) < 2e-6
    dW = torch.full((N, Kc), 0.25, device=DEV)
    got = K.small_gemm(True, False, dyg, xg, out=dW, accumulate=True, allow_split=True)
    if M % 32 or N % 4:
        assert got is None
    else:
        assert rel_err(dW - 0.25, dy.t() @ x) < 2e-6
    assert K.small_gemm(False, True, xg[:, :Kc - 1], wg[:, :Kc - 1]) is None          # K % 32 != 0 -> caller falls back


@pytest.mark.parametrize("n,off", [(1, 0), (3, 1), (4, 0), (1023, 3), (4096, 2), (1 << 20, 0), ((1 << 20) + 7, 1)])
def test_split_k_zero_fill_sizes_and_alignments(K, n, off):
    """mi_zero_async (the fill kernel behind every split-K output) over sizes / alignments of its vector and tail paths, through the one
    entry point that exposes it directly: a split small GEMM into a slice that starts `off` floats into a poisoned buffer."""
    I, J = (n + 31) // 32, 32
    buf = torch.full((off + I * J + 64,), 7.0, device=DEV)
    out = buf[off:off + I * J].view(I, J)
    g = torch.Generator().manual_seed(n)
    A = torch.randn(I, 448, generator=g).to(DEV); Bm = (torch.randn(448, J, generator=g) / 21.0).to(DEV)
    if K.small_gemm(False, False, A, Bm, out=out, allow_split=True) is None:
        pytest.skip("shape not taken by mi_small_gemm")
    assert rel_err(out, A.double().cpu() @ Bm.double().cpu()) < 2e-6
    assert bool((buf[:off] == 7.0).all()) and bool((buf[off + I * J:] == 7.0).all())         # nothing outside the slice was touched


def test_split_gemm_in_a_replayed_graph_starts_from_zero(K):
    """The split-K forms zero their output and add their slices with atomics.  Captured into a hipGraph that zero fill has to stay in
    stream order: as a memset node (hipMemsetAsync) it was seen to take effect BEFORE the previous writer of the same memory in replays
    (round 5: time-MLP gradients of 1e38 from the second replay on, one fresh process in ten, tools/proto/graph_nan.py); it is a kernel
    now (mi_zero_async).  Here the output buffer is poisoned inside the graph right before the GEMM, 300 replays.  (A guard for the kernel
    form, not a reproducer of the fault: the memset build passes this test too -- the fault needed the whole step, one process in ~15.)"""
    g = torch.Generator().manual_seed(7)
    dy = torch.randn(16, 448, generator=g).to(DEV)
    w = (torch.randn(448, 32, generator=g) / 21.0).to(DEV)
    ref = dy.double().cpu() @ w.double().cpu()
    out = torch.empty(16, 32, device=DEV)
    poison = torch.full((16, 32), 3e38, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert K.small_gemm(False, False, dy, w, out=out, allow_split=True) is not None       # (lazy set-up outside the capture)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            torch.mul(poison, 1.0, out=out)                                                   # the previous tenant's leftovers (a kernel node)
            K.small_gemm(False, False, dy, w, out=out, allow_split=True)
    torch.cuda.current_stream().wait_stream(s)
    worst = 0.0
    for _ in range(300):
        gr.replay()
        worst = max(worst, rel_err(out, ref))
    assert worst < 2e-6, worst


def test_halo_kernel_takes_every_bf16_layer_in_a_subprocess():
    """MI_CONV_AUTO=0: the register-staged halo kernel (the fallback of the per-shape pick, and the only kernel behind the dual-output,
    epilogue-sum and fused entry points) on the bf16-stored layers that conv_pw / conv1x1_pw take by default -- every conv kernel test and the
    end-to-end bf16 block test."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, MI_CONV_AUTO="0")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), os.path.join(here, "test_unet_gpu.py"), "-q", "-x",
                        "-p", "no:cacheprovider", "-k", "(conv and not subprocess) or bf16_block or cfg2_eps or mid_unet"],
                       capture_output=True, text=True, timeout=1200, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("variant", ["bf16", "fp32", "fp32+res+copy"])
@pytest.mark.parametrize("cfg", [(16, 32, 32, 128), (8, 16, 16, 256), (8, 16, 16, 128), (4, 8, 8, 512), (4, 8, 8, 256), (2, 4, 4, 128)])
def test_gn_mish_apply_from_epilogue_sums(K, cfg, variant):
    """mi_gn_mish_apply_sums (round 6): GroupNorm + Mish + time bias (+ residual, + bf16 copy) as ONE streaming pass fed by the sums a
    conv's epilogue leaves, against the two-phase kernel (mi_gn_mish_fwd_io / _dual) on the same bf16 tensor: same statistics (the sums
    are exact sums of the stored values; var = E[x^2] - mean^2 in double against the two-pass variance), same packed / fast Mish."""
    N, H, W, Cc = cfg
    g = torch.Generator(device=DEV).manual_seed(11)
    x = (torch.randn(N, H, W, Cc, device=DEV, generator=g) * 1.5 + 0.3).bfloat16()
    ga = torch.randn(Cc, device=DEV, generator=g); be = torch.randn(Cc, device=DEV, generator=g)
    tb = torch.randn(N, Cc, device=DEV, generator=g)
    res = torch.randn(N, H, W, Cc, device=DEV, generator=g) if "res" in variant else None
    xs = x.double().view(N, H * W, Cc // 16, 16)
    sums = K.gn_sums_encode(torch.stack([xs.sum((1, 3)), (xs * xs).sum((1, 3))], dim=-1))
    dt = torch.bfloat16 if variant == "bf16" else torch.float32
    want16 = "copy" in variant
    ref = K.gn_mish_fwd(x, ga, be, temb=tb, residual=res, out_dtype=dt, want16=want16)
    out = K.gn_mish_apply_sums(x, sums, ga, be, temb=tb, residual=res, out_dtype=dt, want16=want16)
    assert out is not None, "shape not taken"
    assert out[0].dtype == dt and torch.isfinite(out[0].float()).all()
    tol = 8e-3 if dt == torch.bfloat16 else 2e-5                 # bf16 output: one rounding flip of 2^-8; fp32: the statistics' last bits
    assert rel_err(out[0].float(), ref[0].float()) < tol
    assert float((out[1] - ref[1].view_as(out[1])).abs().max() / ref[1].abs().max()) < 2e-5      # {mean, rstd}
    if want16:
        assert rel_err(out[2].float(), ref[2].float()) < 8e-3
        assert torch.equal(out[2], out[0].bfloat16())


def test_stride2_wgrad_exact_fp32_gathered_taps(K):
    """mi_conv_s2_wgrad_f32 (round 6; fp32 mode, the mode that carries the 1e-4 bar): the weight gradients of Downsample (3x3 / stride 2)
    and Upsample (ConvTranspose 4x4 / stride 2) as gathered 1x1 problems of the exact-fp32 kernel -- cfg-2 / cfg-3 layer shapes at a
    small batch, a ragged small-side channel count, every image border -- against fp64 on the same fp32 operands, accumulating into a
    non-zero dW; other geometries are refused."""
    g = torch.Generator().manual_seed(59)
    layers = [dict(kind="down", N=4, h=16, C=128), dict(kind="down", N=8, h=8, C=256), dict(kind="up", N=8, h=8, C=256),
              dict(kind="up", N=4, h=16, C=128), dict(kind="down", N=2, h=32, C=64), dict(kind="up", N=2, h=32, C=64),
              dict(kind="down", N=8, h=8, C=192, Co=96), dict(kind="up", N=8, h=8, C=64, Co=160), dict(kind="down", N=16, h=4, C=64)]
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
    for L in layers:
        N, h, Ci, Co = L["N"], L["h"], L["C"], L.get("Co", L["C"])
        if L["kind"] == "down":
            x = torch.randn(N, Ci, 2 * h, 2 * h, generator=g); dy = torch.randn(N, Co, h, h, generator=g)
            w = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
            F.conv2d(x.double(), w, None, stride=2, padding=1).backward(dy.double())
            k, tr = 3, False
        else:
            x = torch.randn(N, Ci, h, h, generator=g); dy = torch.randn(N, Co, 2 * h, 2 * h, generator=g)
            w = torch.zeros(Ci, Co, 4, 4, dtype=torch.float64, requires_grad=True)
            F.conv_transpose2d(x.double(), w, None, stride=2, padding=1).backward(dy.double())
            k, tr = 4, True
        base = torch.randn(k * k * Ci * Co, generator=g).to(DEV)
        dW = base.clone()
        ok = K.conv_s2_wgrad_f32(nh(x), nh(dy), dW, k=k, Ci=Ci, Cj=Co, gather_i=not tr, grid_g=(2 * h, 2 * h), grid_d=(h, h))
        assert ok, L
        torch.cuda.synchronize()
        got = w_from_storage((dW - base).view(k, k, Ci, Co), transposed=tr)
        assert rel_err(got, w.grad) < 2e-6, (L, rel_err(got, w.grad))
    # bf16 operands, odd grids and channel counts the kernel does not tile are refused (the caller keeps conv_wgrad)
    z = lambda n, hh, c, dt=torch.float32: torch.zeros(n, hh, hh, c, device=DEV, dtype=dt)          # noqa: E731
    assert not K.conv_s2_wgrad_f32(z(2, 16, 64, torch.bfloat16), z(2, 8, 64), torch.zeros(9 * 64 * 64, device=DEV), k=3, Ci=64, Cj=64, gather_i=True, grid_g=(16, 16), grid_d=(8, 8))
    assert not K.conv_s2_wgrad_f32(z(2, 12, 64), z(2, 6, 64), torch.zeros(9 * 64 * 64, device=DEV), k=3, Ci=64, Cj=64, gather_i=True, grid_g=(12, 12), grid_d=(6, 6))
    assert not K.conv_s2_wgrad_f32(z(2, 16, 32), z(2, 8, 64), torch.zeros(9 * 32 * 64, device=DEV), k=3, Ci=32, Cj=64, gather_i=True, grid_g=(16, 16), grid_d=(8, 8))


@pytest.mark.parametrize("kind", ["down", "up"])
def test_stride2_wgrad_exact_fp32_launches_every_call(K, kind):
    """conv_s2_wgrad_f32 twice on the SAME three tensors adds the gradient twice (a memoised wrapper answered the second call without
    launching: dW stayed at base + g).  Downsample (k = 3) / Upsample (k = 4) at N = 2, 16x16 <-> 8x8, 64 channels, integer operands
    (x in -4..4, dy in -3..3, dW from -3..3): at most 128 * 16 terms of magnitude <= 12 per sum, so every sum is exact in fp32 in any
    order and the result equals base + 2 g bit for bit, g from float64 autograd."""
    g = torch.Generator().manual_seed(61)
    N, h, C = 2, 8, 64
    ints = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()          # noqa: E731
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)          # noqa: E731
    if kind == "down":
        x, dy = ints(-4, 4, N, C, 2 * h, 2 * h), ints(-3, 3, N, C, h, h)
        w = torch.zeros(C, C, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.double(), w, None, stride=2, padding=1).backward(dy.double())
        k, tr = 3, False
    else:
        x, dy = ints(-4, 4, N, C, h, h), ints(-3, 3, N, C, 2 * h, 2 * h)
        w = torch.zeros(C, C, 4, 4, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(x.double(), w, None, stride=2, padding=1).backward(dy.double())
        k, tr = 4, True
    base = ints(-3, 3, k * k * C * C).to(DEV)
    dW, P, Q = base.clone(), nh(x), nh(dy)
    for _ in range(2):
        assert K.conv_s2_wgrad_f32(P, Q, dW, k=k, Ci=C, Cj=C, gather_i=not tr, grid_g=(2 * h, 2 * h), grid_d=(h, h))
    torch.cuda.synchronize()
    got = w_from_storage((dW - base).view(k, k, C, C), transposed=tr)
    assert torch.equal(got.double(), 2 * w.grad), float((got.double() - 2 * w.grad).abs().max())
