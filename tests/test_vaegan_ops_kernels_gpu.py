"""The VAE-GAN kernels (csrc/vaegan_ops.hip) through their C ABI, each alone against the float64 oracle (tests/_vaegan_oracle.py, itself
checked against torch's float64 autograd in tests/test_vaegan_cpu.py).

Bounds.  The latent kernels do the arithmetic of mi_cvae_latent_fwd / bwd and take tests/test_cvae_kernels_gpu.py's bounds for them:
z within 1e-6 max|ref| + 1e-5, the KL term within 1e-5 relative, dh within 1e-5 max|ref| + 1e-5.  mi_feat_match sums in fp64 like
mi_age_image_mse and takes tests/test_age_moments_kernels_gpu.py's bounds for it: the loss within one float32 rounding (2^-23
relative), the stored gradient within 2^-23 max|ref|.  The ADDED gradient is rounded twice -- the gradient to float32, then the sum --
so it gets that bound plus half an ulp of the sum, 2^-24 max|prior + ref|.  The packings copy and multiply once: exact.
Every pitched input sits in a NaN-filled buffer, every output starts as NaN."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vaegan_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from src.ops.lib import load_library
    return load_library()


def _stream():
    from src.ops import functional as K
    return K._stream()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _pitched(x, ld):
    """x [rows, L] as a NaN-filled [rows, ld] device buffer."""
    x = np.asarray(x, dtype=np.float32)
    buf = torch.full((x.shape[0], ld), float("nan"))
    buf[:, :x.shape[1]] = torch.from_numpy(x)
    return buf.cuda()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype)


def _h(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _close(name, got, ref, rel):
    """tests/test_cvae_kernels_gpu.py::_close"""
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(f"{name}: max err {err:.3e}, max|ref| {scale:.3e}, bound {rel * scale + 1e-5:.3e}")
    assert err <= rel * scale + 1e-5, (name, err, scale)


# --------------------------------------------------------------------------- latent block
@pytest.mark.parametrize("N", (1, 5, 67))
@pytest.mark.parametrize("L", (6, 8, 100))                       # 6: two pad lanes in z, none in dh (12); 100: the shipped width
def test_latent_forward_and_backward_match_the_oracle(lib, N, L):
    r = np.random.RandomState(100 * N + L)
    h = (r.randn(N, 2 * L) * 0.5).astype(np.float32)
    eps, prior = r.randn(N, L).astype(np.float32), r.randn(N, L).astype(np.float32)
    ldh, ldz, lddh, lddz = 2 * L + 3, (L + 3) // 4 * 4, (2 * L + 3) // 4 * 4, L + 5
    dz = r.randn(2 * N, L).astype(np.float32)                     # the decoder's 2N-row input gradient: the first N rows are read
    hb, eb, pb, dzb = _pitched(h, ldh), torch.from_numpy(eps).cuda(), torch.from_numpy(prior).cuda(), _pitched(dz, lddz)
    zz_ref, kld_ref = O.latent_fwd(h, eps, prior)
    g_kld, dz_scale = 1.0, 1000.0                                 # 1 / recon_weight of the shipped MNIST run
    dh_ref = O.latent_bwd(h, eps, dz, g_kld, dz_scale)
    runs = []
    for _ in range(2):
        z, kld, dh = _nan(2 * N, ldz), _nan(1), _nan(N, lddh)
        assert lib.mi_vaegan_latent_fwd(N, L, _p(hb), ldh, _p(eb), _p(pb), _p(z), ldz, _p(kld), _stream()) == 0, lib.mi_last_error()
        assert lib.mi_vaegan_latent_bwd(N, L, _p(hb), ldh, _p(eb), _p(dzb), lddz, dz_scale, g_kld, _p(dh), lddh, _stream()) == 0, lib.mi_last_error()
        runs.append((z, kld, dh))
    assert all(_bits(a, b) for a, b in zip(*runs))                # two calls, the same bits
    z, kld, dh = (_h(t) for t in runs[0])
    assert np.isfinite(z).all() and np.isfinite(dh).all()         # every element stored
    assert (z[:, L:] == 0).all() and (dh[:, 2 * L:] == 0).all()   # pad lanes as 0
    assert np.array_equal(z[N:, :L], prior.astype(np.float64))    # the prior half is a copy
    _close("z", z[:N, :L], zz_ref[:N], 1e-6)
    print(f"kld {float(kld[0]):.9g} float64 {kld_ref:.9g}")
    assert abs(float(kld[0]) - kld_ref) <= 1e-5 * abs(kld_ref)
    _close("dh", dh[:, :2 * L], dh_ref, 1e-5)


def test_latent_wrappers_read_the_nets_buffers_in_place():
    from src.ops import functional as K
    N, L = 5, 6
    r = np.random.RandomState(1)
    h = (r.randn(N, 2 * L) * 0.5).astype(np.float32)
    eps, prior, dz = (r.randn(N, L).astype(np.float32) for _ in range(3))
    hv = _pitched(h, 2 * L).view(N, 1, 1, 2 * L)                                    # the encoder's NHWC output
    zz, kld = K.vaegan_latent_fwd(hv, torch.from_numpy(eps).cuda(), torch.from_numpy(prior).cuda())
    assert zz.shape == (2 * N, 1, 1, L) and zz._base.shape == (2 * N, 1, 1, 8) and kld.shape == ()
    ref, kref = O.latent_fwd(h, eps, prior)
    _close("z", _h(zz).reshape(2 * N, L), ref, 1e-6)
    assert abs(float(kld) - kref) <= 1e-5 * abs(kref)
    dzv = _pitched(np.concatenate([dz, dz]), 8).view(2 * N, 1, 1, 8)[..., :L]       # the decoder's input gradient, pitch 8
    dh = K.vaegan_latent_bwd(hv, torch.from_numpy(eps).cuda(), dzv, g_kld=1.0, dz_scale=1e4)
    assert dh.shape == (N, 1, 1, 2 * L) and dh._base.shape == (N, 1, 1, 12)
    _close("dh", _h(dh).reshape(N, 2 * L), O.latent_bwd(h, eps, dz, 1.0, 1e4), 1e-5)
    with pytest.raises(RuntimeError):
        K.vaegan_latent_fwd(hv.cpu(), torch.from_numpy(eps).cuda(), torch.from_numpy(prior).cuda())
    with pytest.raises(RuntimeError):
        K.vaegan_latent_fwd(hv, torch.from_numpy(eps).cuda(), torch.from_numpy(prior[:, :5]).cuda())


def test_latent_refusals_write_nothing(lib):
    N, L = 5, 6
    h, e = torch.randn(N, 2 * L, device="cuda"), torch.randn(2 * N, L, device="cuda")
    z, kld, dh = _nan(2 * N, 8), _nan(1), _nan(N, 12)
    bad_fwd = [(0, L, 2 * L, 8), (N, 0, 2 * L, 8), (N, L, 2 * L - 1, 8), (N, L, 2 * L, 6), (N, L, 2 * L, 12)]
    for n, l, ldh, ldz in bad_fwd:
        assert lib.mi_vaegan_latent_fwd(n, l, _p(h), ldh, _p(e), _p(e), _p(z), ldz, _p(kld), _stream()) != 0 and lib.mi_last_error()
    assert lib.mi_vaegan_latent_fwd(N, L, _p(h), 2 * L, _p(e), None, _p(z), 8, _p(kld), _stream()) != 0
    assert lib.mi_vaegan_latent_fwd(N, L, _p(h), 2 * L, _p(e), _p(e), C.c_void_p(z.data_ptr() + 4), 8, _p(kld), _stream()) != 0     # misaligned
    for n, l, ldh, lddz, lddh in [(0, L, 12, L, 12), (N, L, 11, L, 12), (N, L, 12, L - 1, 12), (N, L, 12, L, 13), (N, L, 12, L, 16), (N, L, 12, L, 8)]:
        assert lib.mi_vaegan_latent_bwd(n, l, _p(h), ldh, _p(e), _p(e), lddz, 1.0, 1.0, _p(dh), lddh, _stream()) != 0 and lib.mi_last_error()
    assert lib.mi_vaegan_latent_supported(0, 6) == 0 and lib.mi_vaegan_latent_supported(1 << 22, 100) == 0
    assert lib.mi_vaegan_latent_supported(128, 100) == 1
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (z, kld, dh))


# --------------------------------------------------------------------------- feature reconstruction loss
# per = 16 * 4 ndf: 256 for the tiny nets, 2048 for the shipped width.  A workgroup takes 256 four-lane groups a pass: N = 5 at 256 is
# two workgroups with a ragged last one, N = 67 seventeen, (513, 2048) more groups than the grid's 1024 workgroups hold at once (the
# strided walk, ragged too), N = 1 a quarter of one workgroup.
@pytest.mark.parametrize("N,per", [(1, 256), (5, 256), (67, 256), (1, 2048), (5, 2048), (513, 2048)])
def test_feat_match_is_exact_in_order_and_repeatable(lib, N, per):
    r = np.random.RandomState(N + per)
    act = r.randn(3 * N, per).astype(np.float32)                 # netD's last hidden activation over [fake | real | recon]
    prior = r.randn(3 * N, per).astype(np.float32)               # what network.8's input-gradient conv left in the gradient buffer
    want, gref = O.feat_match(act[N:2 * N], act[2 * N:], 3.0)
    ab = torch.from_numpy(act).cuda()
    real, recon = ab[N:2 * N], ab[2 * N:]
    n = int(lib.mi_feat_match_workspace_doubles(N, per))
    assert n == min((N * per // 4 + 255) // 256, 1024) and lib.mi_feat_match_supported(N, per) == 1
    stored, added = [], []
    for ws in (_nan(n, dtype=torch.float64), torch.full((n,), 1e300, device="cuda", dtype=torch.float64)):
        loss, g = _nan(1), _nan(N, per)
        assert lib.mi_feat_match(N, per, _p(real), _p(recon), _p(loss), _p(g), 3.0, 0, _p(ws), _stream()) == 0, lib.mi_last_error()
        stored.append((loss, g))
        loss, buf = _nan(1), torch.from_numpy(prior).cuda()
        assert lib.mi_feat_match(N, per, _p(real), _p(recon), _p(loss), _p(buf[2 * N:]), 3.0, 1, _p(ws), _stream()) == 0, lib.mi_last_error()
        added.append((loss, buf))
    for runs in (stored, added):
        assert _bits(runs[0][0], runs[1][0]) and _bits(runs[0][1], runs[1][1])
    assert _bits(stored[0][0], added[0][0])
    loss, g, buf = float(stored[0][0]), _h(stored[0][1]), _h(added[0][1])
    print(f"N={N} per={per}: loss {loss:.9g} float64 {want:.9g}, max|g - ref| {np.abs(g - gref).max():.3e}")
    assert abs(loss - want) <= 2.0 ** -23 * want
    assert np.abs(g - gref).max() <= 2.0 ** -23 * np.abs(gref).max()
    assert np.array_equal(buf[:2 * N], prior[:2 * N].astype(np.float64))                      # the other segments' rows are left alone
    total = prior[2 * N:].astype(np.float64) + gref
    assert np.abs(buf[2 * N:] - total).max() <= 2.0 ** -23 * np.abs(gref).max() + 2.0 ** -24 * np.abs(total).max()
    loss_only = _nan(1)
    assert lib.mi_feat_match(N, per, _p(real), _p(recon), _p(loss_only), None, 3.0, 0, _p(_nan(n, dtype=torch.float64)), _stream()) == 0
    assert _bits(loss_only, stored[0][0])
    assert _bits(ab, torch.from_numpy(act).cuda())                                           # the activation is read, never written


def test_feat_match_wrapper_and_refusals(lib):
    from src.ops import functional as K
    N, per = 5, 256
    r = np.random.RandomState(2)
    act = torch.from_numpy(r.randn(3 * N, 4, 4, 16).astype(np.float32)).cuda()
    want, gref = O.feat_match(_h(act[N:2 * N]), _h(act[2 * N:]), 1.0)
    g = torch.zeros_like(act)
    loss, out = K.feat_match(act[N:2 * N], act[2 * N:], drecon=g[2 * N:], accumulate=True)
    assert out.data_ptr() == g[2 * N:].data_ptr() and abs(float(loss) - want) <= 2.0 ** -23 * want
    assert float(g[:2 * N].abs().max()) == 0 and np.abs(_h(g[2 * N:]) - gref).max() <= 2.0 ** -23 * np.abs(gref).max()
    loss2, none = K.feat_match(act[N:2 * N], act[2 * N:], want_grad=False)
    assert none is None and _bits(loss2.reshape(1), loss.reshape(1))
    _, fresh = K.feat_match(act[N:2 * N], act[2 * N:])
    assert _bits(fresh, g[2 * N:])
    with pytest.raises(RuntimeError):
        K.feat_match(act[N:2 * N], act[2 * N:, :, :, :8])                                    # not dense, another shape
    with pytest.raises(RuntimeError):
        K.feat_match(act[N:2 * N], act[2 * N:], accumulate=True)                             # nothing to add into
    loss, out, ws = _nan(1), _nan(N, per), _nan(8, dtype=torch.float64)
    a = torch.randn(2 * N * per + 4, device="cuda")
    for n, p in [(0, per), (N, 0), (N, 254), (N, 2)]:
        assert lib.mi_feat_match_supported(n, p) == 0 and lib.mi_last_error()
        assert lib.mi_feat_match(n, p, _p(a), _p(a), _p(loss), _p(out), 1.0, 0, _p(ws), _stream()) != 0 and lib.mi_last_error()
    assert lib.mi_feat_match(N, per, C.c_void_p(a.data_ptr() + 4), _p(a), _p(loss), _p(out), 1.0, 0, _p(ws), _stream()) != 0             # misaligned
    assert lib.mi_feat_match(N, per, _p(a), _p(a), _p(loss), _p(out), 1.0, 0, None, _stream()) != 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (loss, out, ws))


# --------------------------------------------------------------------------- segment packing
@pytest.mark.parametrize("N,C_", [(1, 1), (5, 1), (5, 3), (2, 3)])
def test_pack_and_unpack_are_exact(lib, N, C_):
    HW, ld = 784, 4
    r = np.random.RandomState(10 * N + C_)
    dec = r.uniform(-1, 1, (2 * N * HW, C_)).astype(np.float32)
    imgs = r.uniform(-1, 1, (N, C_, HW)).astype(np.float32)
    dx = r.randn(3 * N * HW, C_).astype(np.float32)
    db, ib, dxb = _pitched(dec, ld), torch.from_numpy(imgs).cuda(), _pitched(dx, ld)          # pad lanes of the inputs are NaN: never copied
    s_recon, s_fake = np.float32(1e-3), np.float32(0.75)
    runs = []
    for _ in range(2):
        x, dy = _nan(3 * N * HW, ld), _nan(2 * N * HW, ld)
        assert lib.mi_vaegan_pack_fwd(N, C_, HW, _p(db), _p(ib), _p(x), ld, _stream()) == 0, lib.mi_last_error()
        assert lib.mi_vaegan_unpack_bwd(N, C_, HW, _p(dxb), float(s_recon), float(s_fake), _p(dy), ld, _stream()) == 0, lib.mi_last_error()
        runs.append((x, dy))
    assert all(_bits(a, b) for a, b in zip(*runs))
    x, dy = runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy()
    assert (x[:, C_:] == 0).all() and (dy[:, C_:] == 0).all()
    want = O.pack_fwd(dec.reshape(2 * N, HW, C_), imgs).reshape(3 * N * HW, C_)
    assert np.array_equal(x[:, :C_], want)
    dxs = dx.reshape(3 * N, HW, C_)
    want = np.concatenate([s_recon * dxs[2 * N:], s_fake * dxs[:N]]).reshape(2 * N * HW, C_)   # one float32 product per element
    assert want.dtype == np.float32 and np.array_equal(dy[:, :C_], want)


def test_pack_wrappers_and_refusals(lib):
    from src.ops import functional as K
    N, HW = 3, 784
    r = np.random.RandomState(4)
    dec = _pitched(r.uniform(-1, 1, (2 * N * HW, 1)), 4).view(2 * N, 28, 28, 4)[..., :1]
    imgs = torch.from_numpy(r.uniform(-1, 1, (N, 1, 28, 28)).astype(np.float32)).cuda()
    x = K.vaegan_pack_fwd(dec, imgs)
    assert x.shape == (3 * N, 28, 28, 1) and x._base.shape == (3 * N, 28, 28, 4) and float(x._base[..., 1:].abs().max()) == 0
    assert torch.equal(x[:N], dec[N:]) and torch.equal(x[2 * N:], dec[:N]) and torch.equal(x[N:2 * N], imgs.permute(0, 2, 3, 1))
    dy = K.vaegan_unpack_bwd(x, s_recon=2.0, s_fake=-1.0)
    assert dy.shape == (2 * N, 28, 28, 1) and torch.equal(dy[:N], 2.0 * dec[:N]) and torch.equal(dy[N:], -dec[N:])
    with pytest.raises(RuntimeError):
        K.vaegan_pack_fwd(dec[:N], imgs)
    with pytest.raises(RuntimeError):
        K.vaegan_pack_fwd(dec, imgs.cpu())
    out, src = _nan(3 * N * HW, 4), torch.randn(3 * N * HW * 4 + 4, device="cuda")
    for n, c, hw, ld in [(0, 1, HW, 4), (N, 0, HW, 4), (N, 1, 0, 4), (N, 5, HW, 4), (N, 1, HW, 3), (N, 1, HW, 6), (1 << 20, 1, HW, 4)]:
        assert lib.mi_vaegan_pack_supported(n, c, hw, ld) == 0 and lib.mi_last_error()
        assert lib.mi_vaegan_pack_fwd(n, c, hw, _p(src), _p(src), _p(out), ld, _stream()) != 0 and lib.mi_last_error()
        assert lib.mi_vaegan_unpack_bwd(n, c, hw, _p(src), 1.0, 1.0, _p(out), ld, _stream()) != 0 and lib.mi_last_error()
    assert lib.mi_vaegan_pack_fwd(N, 1, HW, C.c_void_p(src.data_ptr() + 4), _p(src), _p(out), 4, _stream()) != 0                          # misaligned
    assert lib.mi_vaegan_unpack_bwd(N, 1, HW, _p(src), 1.0, 1.0, None, 4, _stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
