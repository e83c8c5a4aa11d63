"""cVAE kernels (csrc/cvae_ops.hip), each alone against torch on the CPU in float64, and the generic implicit-GEMM convolution family at the
shapes the cVAE sends it to for the first time: 11 input channels in a pitch-12 buffer, the 1x1 -> 4x4 transposed conv at 256 inputs.
No test feeds a label outside [0, ncls): those guards are read, not run."""
import math

import pytest
import torch
import torch.nn.functional as F

from _util import DEV, TOL, conv_w_storage, from_nhwc, rel_err, to_nhwc_gpu, w_from_storage

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from src.ops import functional
    return functional


def _close(a, b, rel, what=""):
    """tests/test_vae_gpu.py::_close"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= rel * scale + 1e-5, f"{what}: max err {err:.3e} > {rel} * max |ref| ({scale:.3e}) + 1e-5"


# --------------------------------------------------------------------------- encoder input
@pytest.mark.parametrize("N,C,H,W,ncls", [(3, 1, 5, 7, 10),       # 11 -> pitch 12, one pad lane
                                          (2, 3, 4, 4, 10),       # 13 -> pitch 16, three pad lanes
                                          (1, 1, 1, 1, 2),
                                          (5, 1, 28, 28, 10)])
def test_pack_input_is_exactly_cat_of_image_and_onehot_planes(K, N, C, H, W, ncls):
    g = torch.Generator().manual_seed(N * 100 + C)
    x = torch.randn(N, C, H, W, generator=g)
    labels = torch.randint(0, ncls, (N,), generator=g)
    y = K.cvae_pack_input(x.to(DEV), labels.to(DEV), ncls)
    ld = (C + ncls + 3) // 4 * 4
    assert y.shape == (N, H, W, C + ncls) and y._base.shape == (N, H, W, ld) and K.ld_of(y) == ld
    planes = F.one_hot(labels, ncls).float().reshape(N, ncls, 1, 1).expand(N, ncls, H, W)
    ref = torch.cat([x, planes, torch.zeros(N, ld - C - ncls, H, W)], dim=1).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(y._base.cpu(), ref)                                     # the whole buffer, pad lanes included


# --------------------------------------------------------------------------- latent block
LATENT_SHAPES = [(7, 20, 10), (1, 1, 2), (130, 128, 10), (6, 16, 3)]


def _latent_case(N, L, ncls):
    g = torch.Generator().manual_seed(1000 * N + L)
    h = torch.randn(N, 2 * L, generator=g) * 0.5
    eps = torch.randn(N, L, generator=g)
    E = torch.randn(ncls, L, generator=g)
    dzc = torch.randn(N, 2 * L, generator=g)
    labels = torch.full((N,), ncls - 1, dtype=torch.int64) if (N, L, ncls) == (6, 16, 3) else torch.randint(0, ncls, (N,), generator=g)
    return h, eps, E, dzc, labels


def _latent_reference(h, eps, E, dzc, labels, g_kld):
    """float64 torch on the float32 operands: (z, kld, dh, dE, sum of |terms| per dE element)."""
    N, L = eps.shape
    hd = h.double().requires_grad_(True)
    mu, ls = torch.chunk(hd, 2, dim=1)
    z = mu + torch.exp(ls) * eps.double()
    kld = (-0.5 * torch.sum(1 + 2 * ls - mu ** 2 - torch.exp(2 * ls), dim=-1)).mean()
    (g_kld * kld + (z * dzc[:, :L].double()).sum()).backward()
    dE = torch.zeros(E.shape, dtype=torch.float64).index_add_(0, labels, dzc[:, L:].double())
    mag = torch.zeros(E.shape, dtype=torch.float64).index_add_(0, labels, dzc[:, L:].double().abs())
    return z.detach(), kld.detach(), hd.grad, dE, mag


@pytest.mark.parametrize("N,L,ncls", LATENT_SHAPES)
def test_latent_forward_backward_against_torch(K, N, L, ncls):
    h, eps, E, dzc, labels = _latent_case(N, L, ncls)
    z, kld, dh, dE, mag = _latent_reference(h, eps, E, dzc, labels, 3.0)
    hg, eg, Eg, dg, lg = h.to(DEV), eps.to(DEV), E.to(DEV), dzc.to(DEV), labels.to(DEV)
    zc, kk = K.cvae_latent_fwd(hg, eg, lg, Eg)
    assert zc.shape == (N, 2 * L)
    assert torch.equal(zc[:, L:].cpu(), E[labels])                             # the embedding half is a copy
    _close(zc[:, :L], z, 1e-6, "z")
    assert abs(float(kk) - float(kld)) <= 1e-5 * abs(float(kld))
    dEg = torch.zeros(ncls, L, device=DEV)
    dhg = K.cvae_latent_bwd(hg, eg, lg, dg, 3.0, dEg)
    _close(dhg, dh, 1e-5, "dh")
    # a sum of at most N fp32 terms in a fixed order: |err| <= N 2^-24 sum |terms| per element
    err = (dEg.cpu().double() - dE).abs()
    assert bool((err <= N * 2.0 ** -24 * mag).all()), float((err - N * 2.0 ** -24 * mag).max())
    # the upstream gradient as a device scalar multiplies the KL term only
    dhs = K.cvae_latent_bwd(hg, eg, lg, dg, 1.5, torch.zeros(ncls, L, device=DEV), g_dev=torch.full((1,), 2.0, device=DEV))
    assert torch.equal(dhs, dhg)


@pytest.mark.parametrize("N,L,ncls", LATENT_SHAPES)
def test_embedding_gradient_is_reproducible_and_leaves_absent_rows_alone(K, N, L, ncls):
    h, eps, E, dzc, labels = _latent_case(N, L, ncls)
    hg, eg, dg, lg = h.to(DEV), eps.to(DEV), dzc.to(DEV), labels.to(DEV)
    runs = []
    for _ in range(2):
        dE = torch.zeros(ncls, L, device=DEV)
        K.cvae_latent_bwd(hg, eg, lg, dg, 1.0, dE)
        runs.append(dE)
    assert torch.equal(runs[0], runs[1])                                       # fixed summation order: bitwise
    pattern = (torch.arange(ncls * L, dtype=torch.float32).reshape(ncls, L) * 0.37 - 5.0).to(DEV)
    dE = pattern.clone()
    K.cvae_latent_bwd(hg, eg, lg, dg, 1.0, dE)
    present = torch.zeros(ncls, dtype=torch.bool)
    present[labels] = True
    assert torch.equal(dE[~present].cpu(), pattern[~present].cpu())            # rows of absent classes: bit-identical
    assert torch.equal(dE[present].cpu(), (pattern + runs[0])[present].cpu())  # present rows: pattern + the same sum
    if (N, L, ncls) == (6, 16, 3):
        assert int(present.sum()) == 1 and float(runs[0][:ncls - 1].abs().max()) == 0.0


@pytest.mark.parametrize("N,L,ncls", LATENT_SHAPES)
def test_latent_block_on_views_of_wider_buffers(K, N, L, ncls):
    h, eps, E, dzc, labels = _latent_case(N, L, ncls)
    hg, eg, Eg, dg, lg = h.to(DEV), eps.to(DEV), E.to(DEV), dzc.to(DEV), labels.to(DEV)
    hw = torch.full((N, 2 * L + 8), float("nan"), device=DEV)
    dw = torch.full((N, 2 * L + 4), float("nan"), device=DEV)
    hw[:, :2 * L] = hg
    dw[:, :2 * L] = dg
    zc0, k0 = K.cvae_latent_fwd(hg, eg, lg, Eg)
    zc1, k1 = K.cvae_latent_fwd(hw[:, :2 * L], eg, lg, Eg)
    assert torch.equal(zc0, zc1) and torch.equal(k0, k1)
    dE0, dE1 = torch.zeros(ncls, L, device=DEV), torch.zeros(ncls, L, device=DEV)
    dh0 = K.cvae_latent_bwd(hg, eg, lg, dg, 1.0, dE0)
    dh1 = K.cvae_latent_bwd(hw[:, :2 * L], eg, lg, dw[:, :2 * L], 1.0, dE1)
    assert torch.equal(dh0, dh1) and torch.equal(dE0, dE1)


@pytest.mark.parametrize("N,L,ncls", LATENT_SHAPES)
def test_concat_only_mode_is_exact(K, N, L, ncls):
    _, z, E, _, labels = _latent_case(N, L, ncls)
    zc, kld = K.cvae_latent_fwd(None, z.to(DEV), labels.to(DEV), E.to(DEV))
    assert kld is None and torch.equal(zc.cpu(), torch.cat([z, E[labels]], dim=1))


# --------------------------------------------------------------------------- the generic conv at the new channel count
@pytest.mark.parametrize("H", [6, 28])
def test_generic_conv_at_11_channels_in_a_pitch_12_buffer(K, H):
    """Conv2d(11, 8, 4, 2, 1) -- the cVAE encoder's first layer -- forward, data gradient (11 channels out), weight + bias gradient."""
    N, Ci, Co, k, s, p = 2, 11, 8, 4, 2, 1
    g = torch.Generator().manual_seed(H)
    x = torch.randn(N, Ci, H, H, generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(Co, Ci, k, k, generator=g, dtype=torch.float64) / math.sqrt(Ci * k * k)).requires_grad_(True)
    b = torch.randn(Co, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, b, stride=s, padding=p)
    OH = y.shape[2]
    assert OH == H // 2
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    ws = conv_w_storage(w.detach())
    xg, dyg = to_nhwc_gpu(x.detach().float()), to_nhwc_gpu(dy.float())
    assert K.ld_of(xg) == 12
    yg = K.conv_igemm(xg, ws, kh=k, kw=k, stride=s, pad=p, transposed=False, w_kn=True, K=Ci, Nc=Co, out_hw=(OH, OH), mode=0,
                      bias=b.detach().float().to(DEV))
    dx = K.conv_igemm(dyg, ws, kh=k, kw=k, stride=s, pad=p, transposed=True, w_kn=False, K=Co, Nc=Ci, out_hw=(H, H), mode=0)
    dW, db = torch.zeros(k * k * Ci * Co, device=DEV), torch.zeros(Co, device=DEV)
    K.conv_wgrad(xg, dyg, dW, kh=k, kw=k, stride=s, pad=p, gather_i=True, Ci=Ci, Cj=Co, grid_g=(H, H), grid_d=(OH, OH), mode=0, dbias=db)
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(yg), y) < TOL[0]
    assert rel_err(from_nhwc(dx), x.grad) < TOL[0] and K.ld_of(dx) == 12
    assert float(dx._base[..., Ci:].abs().max()) == 0.0                        # the pad lane of the 11-channel gradient stays zero
    assert rel_err(w_from_storage(dW.view(k, k, Ci, Co)), w.grad) < TOL[0]
    assert rel_err(db, b.grad) < 2e-5


@pytest.mark.parametrize("Ci,Co", [(32, 32), (256, 128)])
def test_transposed_4x4_conv_from_a_1x1_input(K, Ci, Co):
    """ConvTranspose2d(2 L, 4 ngf, 4, 1, 0) on [z | embedding]: the cVAE decoder's first layer at the tiny and the configured size."""
    N = 6
    g = torch.Generator().manual_seed(Ci)
    x = torch.randn(N, Ci, 1, 1, generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(Ci, Co, 4, 4, generator=g, dtype=torch.float64) / math.sqrt(Ci)).requires_grad_(True)
    b = torch.randn(Co, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(x, w, b, stride=1, padding=0)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    ws = conv_w_storage(w.detach(), transposed=True)
    xg, dyg = to_nhwc_gpu(x.detach().float()), to_nhwc_gpu(dy.float())
    yg = K.conv_igemm(xg, ws, kh=4, kw=4, stride=1, pad=0, transposed=True, w_kn=True, K=Ci, Nc=Co, out_hw=(4, 4), mode=0,
                      bias=b.detach().float().to(DEV))
    dx = K.conv_igemm(dyg, ws, kh=4, kw=4, stride=1, pad=0, transposed=False, w_kn=False, K=Co, Nc=Ci, out_hw=(1, 1), mode=0)
    dW, db = torch.zeros(16 * Ci * Co, device=DEV), torch.zeros(Co, device=DEV)
    K.conv_wgrad(xg, dyg, dW, kh=4, kw=4, stride=1, pad=0, gather_i=False, Ci=Ci, Cj=Co, grid_g=(4, 4), grid_d=(1, 1), mode=0)
    K.colsum(dyg, db)
    torch.cuda.synchronize()
    assert rel_err(from_nhwc(yg), y) < TOL[0]
    assert rel_err(from_nhwc(dx), x.grad) < TOL[0]
    assert rel_err(w_from_storage(dW.view(4, 4, Ci, Co), transposed=True), w.grad) < TOL[0]
    assert rel_err(db, b.grad) < 2e-5
