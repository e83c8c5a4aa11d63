"""The atomics-free forms of the generic weight-gradient kernel and of the column sum (csrc/wgrad.hip: mi_conv_wgrad_slabs,
mi_colsum_ordered) through K.conv_wgrad(ordered=True) / K.colsum(ordered=True): against torch's float64 weight gradient with the
bound of tests/test_latent_disc_ln_kernels_gpu.py (max|hip - f64| <= 4 * max|torch_f32 - f64| + 1e-6 * max|f64|), against the default
(atomic) mode, twice for the same bits, onto a gradient that is already there, with a workspace full of NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
# (N, Cin, Cout, H, k, stride, pad, transposed): the GAN's layers at small widths -- 4x4/s2 and 3x3/s2 both ways, one input channel, one
# output channel, the whole-input 4x4 -- and a 128 x 128 layer (the wide tile); every one with three or more slices of the pixel axis
CASES = [(9, 1, 8, 28, 4, 2, 1, False), (7, 8, 16, 14, 4, 2, 1, False), (13, 16, 32, 7, 3, 2, 1, False), (200, 32, 1, 4, 4, 1, 0, False),
         (9, 16, 8, 4, 3, 2, 1, True), (5, 8, 4, 7, 4, 2, 1, True), (3, 4, 1, 14, 4, 2, 1, True), (200, 8, 16, 1, 4, 1, 0, True),
         (64, 128, 128, 4, 3, 2, 1, False)]


@pytest.fixture(scope="module")
def K():
    from src.ops import functional as K
    return K


def _check(name, got, f64, f32):
    got, f64, f32 = (np.asarray(a, dtype=np.float64) for a in (got, f64, f32))
    tol = 4.0 * float(np.abs(f32 - f64).max()) + 1e-6 * float(np.abs(f64).max())
    err = float(np.abs(got - f64).max())
    print(f"{name}: max|hip - f64| {err:.3e}  max|f32 - f64| {float(np.abs(f32 - f64).max()):.3e}  tol {tol:.3e}")
    assert np.isfinite(got).all() and err <= tol, (name, err, tol)


def _reference(x, dy, Cin, Cout, k, stride, pad, transposed, dtype):
    """dW in the kernels' layout [kh][kw][Cin][Cout] (and dbias) from torch autograd on the CPU."""
    import torch.nn.functional as F
    x, dy = x.to(dtype), dy.to(dtype)
    w = torch.zeros((Cin, Cout, k, k) if transposed else (Cout, Cin, k, k), dtype=dtype, requires_grad=True)
    b = torch.zeros(Cout, dtype=dtype, requires_grad=True)
    y = F.conv_transpose2d(x, w, b, stride=stride, padding=pad) if transposed else F.conv2d(x, w, b, stride=stride, padding=pad)
    (y * dy).sum().backward()
    dw = w.grad.permute(2, 3, 0, 1) if transposed else w.grad.permute(2, 3, 1, 0)
    return dw.contiguous().numpy(), b.grad.numpy()


def _operands(K, case, seed):
    N, Cin, Cout, H, k, stride, pad, transposed = case
    g = torch.Generator().manual_seed(seed)
    OH = (H - 1) * stride - 2 * pad + k if transposed else (H + 2 * pad - k) // stride + 1
    x, dy = torch.randn(N, Cin, H, H, generator=g), torch.randn(N, Cout, OH, OH, generator=g)
    return x, dy, K.nchw_to_nhwc(x.cuda()), K.nchw_to_nhwc(dy.cuda()), OH


def _wgrad(K, case, xn, dyn, OH, dW, dbias, ordered):
    N, Cin, Cout, H, k, stride, pad, transposed = case
    if transposed:        # FlatNet._conv_bwd's two calls
        K.conv_wgrad(xn, dyn, dW, kh=k, kw=k, stride=stride, pad=pad, gather_i=False, Ci=Cin, Cj=Cout, grid_g=(OH, OH), grid_d=(H, H), mode=0,
                     ordered=ordered)
        K.colsum(dyn, dbias, ordered=ordered)
    else:
        K.conv_wgrad(xn, dyn, dW, kh=k, kw=k, stride=stride, pad=pad, gather_i=True, Ci=Cin, Cj=Cout, grid_g=(H, H), grid_d=(OH, OH), mode=0,
                     dbias=dbias, ordered=ordered)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_ordered_weight_gradient(K, case):
    from src.ops.lib import MiWgradDesc, load_library
    N, Cin, Cout, H, k, stride, pad, transposed = case
    x, dy, xn, dyn, OH = _operands(K, case, seed=sum(case))
    w64, b64 = _reference(x, dy, Cin, Cout, k, stride, pad, transposed, torch.float64)
    w32, b32 = _reference(x, dy, Cin, Cout, k, stride, pad, transposed, torch.float32)
    lib = load_library()
    dh = H if transposed else OH
    d = MiWgradDesc(N=N, GH=OH if transposed else H, GW=OH if transposed else H, DH=dh, DW=dh, Ci=Cin, Cj=Cout, KH=k, KW=k, stride=stride,
                    pad=pad, gather_i=int(not transposed), mode=0, I1=Cin, ldp=K.ld_of(xn), ldp2=0, ldq=K.ld_of(dyn))
    need = lib.mi_conv_wgrad_slabs_workspace(C.byref(d))
    slices = need // (4 * k * k * Cin * Cout)
    assert slices >= 3 and need == slices * 4 * k * k * Cin * Cout                      # three or more partial sums: their order matters
    K._workspace(xn.device, need).fill_(float("nan"))                                   # any content will do
    runs = []
    for _ in range(2):
        dW, db = torch.zeros(k * k * Cin * Cout, device="cuda"), torch.zeros(Cout, device="cuda")
        _wgrad(K, case, xn, dyn, OH, dW, db, ordered=True)
        runs.append((dW, db))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])  # the same bits
    _check("dW", runs[0][0].cpu().numpy().reshape(w64.shape), w64, w32)
    _check("dbias", runs[0][1].cpu().numpy(), b64, b32)
    # the default mode computes the same sums in another order
    dW0, db0 = torch.zeros_like(runs[0][0]), torch.zeros_like(runs[0][1])
    _wgrad(K, case, xn, dyn, OH, dW0, db0, ordered=False)
    _check("dW (default mode)", dW0.cpu().numpy().reshape(w64.shape), w64, w32)
    # onto a gradient that is already there
    base_w, base_b = torch.randn_like(dW0), torch.randn_like(db0)
    aw, ab = base_w.clone(), base_b.clone()
    _wgrad(K, case, xn, dyn, OH, aw, ab, ordered=True)
    assert torch.equal(aw, base_w + runs[0][0]) and torch.equal(ab, base_b + runs[0][1])


@pytest.mark.parametrize("M,Cc,ld", [(1, 1, 4), (300, 1, 4), (1000, 3, 4), (777, 64, 64), (513, 70, 72), (100352, 1, 4)])
def test_ordered_column_sum(K, M, Cc, ld):
    g = torch.Generator().manual_seed(M + Cc)
    buf = torch.full((M, ld), float("nan"))
    buf[:, :Cc] = torch.randn(M, Cc, generator=g) + 0.25
    x = buf.cuda()[:, :Cc].view(M, 1, 1, Cc) if ld == Cc else buf.cuda().view(M, 1, 1, ld)[..., :Cc]
    f64 = buf[:, :Cc].double().sum(0).numpy()
    f32 = np.cumsum(buf[:, :Cc].numpy(), axis=0, dtype=np.float32)[-1]                  # the yardstick: the plain float32 sum, row after row
    K._workspace(x.device, 4 * ((M + 255) // 256) * Cc).fill_(float("nan"))
    base = torch.randn(Cc, device="cuda")
    outs = []
    for _ in range(2):
        out = base.clone()
        K.colsum(x, out, ordered=True)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    want = base.cpu().double().numpy()
    _check("colsum", outs[0].cpu().numpy(), want + f64, want + f32.astype(np.float64))


def test_refusals(K):
    from src.ops.lib import MiWgradDesc, load_library
    lib = load_library()
    P = lambda t: C.c_void_p(t.data_ptr())                                              # noqa: E731
    x, dy, dW = torch.randn(4, 8, 8, 8, device="cuda"), torch.randn(4, 4, 4, 8, device="cuda"), torch.zeros(16 * 64, device="cuda")
    d = MiWgradDesc(N=4, GH=8, GW=8, DH=4, DW=4, Ci=8, Cj=8, KH=4, KW=4, stride=2, pad=1, gather_i=1, mode=0, I1=8, ldp=8, ldp2=0, ldq=8)
    need = lib.mi_conv_wgrad_slabs_workspace(C.byref(d))
    ws = torch.empty(need // 4, device="cuda")
    assert need == 16 * 64 * 4                                                          # 64 pixels: one slice
    assert lib.mi_conv_wgrad_slabs(C.byref(d), P(x), None, P(dy), P(dW), P(ws), need, None) == 0
    assert lib.mi_conv_wgrad_slabs(C.byref(d), P(x), None, P(dy), P(dW), P(ws), need - 4, None) != 0 and lib.mi_last_error()
    assert lib.mi_conv_wgrad_slabs(C.byref(d), P(x), None, P(dy), P(dW), None, need, None) != 0
    out = torch.zeros(8, device="cuda")
    assert lib.mi_colsum_ordered_workspace(64, 8) == 32 and lib.mi_colsum_ordered_workspace(0, 8) == 0
    assert lib.mi_colsum_ordered(64, 8, P(dy), 8, P(out), P(ws), 32, None) == 0
    assert lib.mi_colsum_ordered(64, 8, P(dy), 8, P(out), P(ws), 28, None) != 0
    assert lib.mi_colsum_ordered(64, 8, P(dy), 4, P(out), P(ws), 32, None) != 0         # a pitch below C
    with pytest.raises(RuntimeError):
        K.colsum(dy.bfloat16(), out, ordered=True)
