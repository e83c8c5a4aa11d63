"""numpy float64 oracle of the VAE-GAN operators (csrc/vaegan_ops.hip; reference src/models/vae_gan.py:63-102): the latent block and its
ANALYTIC backward, the discriminator-feature reconstruction loss with its gradient, and the two segment packings.
tests/test_vaegan_cpu.py checks them against torch's float64 autograd on the reference's formulas."""
import numpy as np


def latent_fwd(h, eps, prior):
    """h [N, 2L] = [mu | log_sigma], eps [N, L], prior [N, L] -> (zz [2N, L] = [mu + exp(log_sigma) eps | prior], kld)."""
    h, eps, prior = (np.asarray(a, dtype=np.float64) for a in (h, eps, prior))
    L = eps.shape[1]
    mu, ls = h[:, :L], h[:, L:2 * L]
    kld = (-0.5 * (1 + 2 * ls - mu ** 2 - np.exp(2 * ls)).sum(axis=1)).mean()
    return np.concatenate([mu + np.exp(ls) * eps, prior]), kld


def latent_bwd(h, eps, dz, g_kld=1.0, dz_scale=1.0):
    """dh [N, 2L] for the loss g_kld * kld + dz_scale * <dz[:N], z>."""
    h, eps, dz = (np.asarray(a, dtype=np.float64) for a in (h, eps, dz))
    N, L = eps.shape
    mu, ls = h[:, :L], h[:, L:2 * L]
    d = dz_scale * dz[:N, :L]
    return np.concatenate([d + g_kld * mu / N, d * eps * np.exp(ls) + g_kld * (np.exp(2 * ls) - 1) / N], axis=1)


def feat_match(real, recon, gscale=1.0):
    """Two blocks [N, ...] -> (sum (real - recon)^2 / N, gscale * its gradient by recon)."""
    real, recon = np.asarray(real, dtype=np.float64), np.asarray(recon, dtype=np.float64)
    N = real.shape[0]
    d = recon - real
    return (d * d).sum() / N, gscale * 2.0 * d / N


def bce_logits(x, real):
    """F.binary_cross_entropy_with_logits(x, ones or zeros), mean."""
    x = np.asarray(x, dtype=np.float64)
    return np.logaddexp(0.0, -x if real else x).mean()


def pack_fwd(dec_out, imgs):
    """dec_out [2N, HW, C] = [recon | fake] (NHWC rows), imgs [N, C, HW] -> [3N, HW, C] = [fake | nhwc(imgs) | recon]."""
    N = imgs.shape[0]
    return np.concatenate([dec_out[N:], np.transpose(imgs, (0, 2, 1)), dec_out[:N]])


def unpack_bwd(dx, s_recon, s_fake):
    """dx [3N, HW, C] over [fake | real | recon] -> [2N, HW, C] = [s_recon dx_recon | s_fake dx_fake]."""
    N = dx.shape[0] // 3
    return np.concatenate([s_recon * dx[2 * N:], s_fake * dx[:N]])
