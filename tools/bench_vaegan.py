#!/usr/bin/env python3
"""VAE-GAN on MNIST shapes (`experiment=vaegan/mnist`: 1x28x28, conv_mnist nets with BatchNorm, ngf = ndf = 32, latent 100,
recon_weight 1e-3, B=128, fp32, eager) on one GPU:
  step     whole training steps (both optimizers step every batch) on the model's path -- the fused operators of csrc/vaegan_ops.hip --
           next to THE SAME STEP COMPOSED FROM THE OPERATORS THAT EXISTED BEFORE THEM, on the same nets in the same process:
           torch.cat / K.nchw_to_nhwc packing and slicing copies, K.vae_latent_fwd / bwd plus the [z | prior] cat and the 1 / recon_weight
           multiply, the feature MSE and its gradient in torch ops handed to `backward_nhwc(dfeat=tensor)`; and next to the GAN's
           generator + discriminator pair at the same batch size, for scale.  The library launches of one step of either kind are
           counted (K.LAUNCHES; torch's own launches come on top for the composed step);
  ops      the new launches alone on fixed tensors of the step's shapes -- latent forward + backward, feature match (accumulating),
           pack + unpack -- next to what they replace.
Every pair is timed three times, alternating, with a device synchronise at the end of each window; the spread between the repeats is
the noise a difference has to clear.  The shader clock is read right behind the timed windows (K.clock_probe).

    python tools/bench_vaegan.py [--batch 128] [--steps 100]
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
VM = importlib.import_module("image-generation-models_amd.src.models.vae_gan")
GM = importlib.import_module("image-generation-models_amd.src.models.gan")
K = importlib.import_module("image-generation-models_amd.src.ops.functional")
DEC = {"_target_": "src.networks.basic.ConvDecoder", "ngf": 32, "norm_type": "batch"}
ENC = {"_target_": "src.networks.basic.ConvEncoder", "ndf": 32, "norm_type": "batch"}
_base = GM._base


def timed(fn, steps, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def clock(dev):
    try:
        return K.clock_probe(dev, usec=300)
    except Exception:       # noqa: BLE001
        return None


def composed_step(m, imgs, eps, prior):
    """VAEGAN.training_step with the pieces of csrc/vaegan_ops.hip replaced by what existed before them."""
    N, L, C = imgs.shape[0], int(m.hparams.latent_dim), m.channels
    rw = float(m.hparams.recon_weight)
    E, G, D = m.encoder, m.decoder, m.netD
    optim_ae, optim_d = m.optimizers()
    h, tape_e = E.forward_nhwc(K.nchw_to_nhwc(imgs), record=True)
    hrows = h.reshape(N, -1)
    z, reg = K.vae_latent_fwd(hrows, eps)
    zz = torch.cat([z, prior])
    zin = zz.view(2 * N, 1, 1, L) if L % 4 == 0 else K.nchw_to_nhwc(zz.view(2 * N, L, 1, 1))
    out, tape_g = G.forward_nhwc(zin, record=True, segments=2)
    ob = _base(out)
    x = torch.cat([ob[N:], _base(K.nchw_to_nhwc(imgs)), ob[:N]])[..., :C]
    pred, tape_d = D.forward_nhwc(x, record=True, segments=3)
    dl = torch.zeros((2, 3 * N, 1, 1, 4), device=imgs.device, dtype=torch.float32)
    dl_ae, dl_d = dl[0][..., :1], dl[1][..., :1]
    g_adv, _, _ = K.adv_loss(pred[:N], [True], "vanilla", dlogit_out=dl_ae[:N])
    d_adv, mean_logit, _ = K.adv_loss(pred[:2 * N], [False, True], "vanilla", dlogit_out=dl_d[:2 * N])
    K.adv_loss(pred[2 * N:], [True], "vanilla", want_grad=False)
    feat = D.features_nhwc(tape_d)
    diff = feat[2 * N:] - feat[N:2 * N]
    loss = (diff * diff).sum() / N
    df = torch.zeros_like(feat)
    df[2 * N:] = diff * (2.0 / N)
    dx = D.backward_nhwc(tape_d, dl_ae, need_dx=True, param_grads=False, dfeat=df)
    dxb = _base(dx)
    dy = torch.cat([dxb[2 * N:] * rw, dxb[:N]])[..., :C]
    dzz = G.backward_nhwc(tape_g, dy, need_dx=True)
    dz = (dzz[:N].reshape(N, -1)[:, :L] * (1.0 / rw)).contiguous()
    dh = K.vae_latent_bwd(hrows, eps, dz, 1.0)
    E.backward_nhwc(tape_e, dh.view(N, 1, 1, -1), need_dx=False)
    optim_ae.step()
    D.backward_nhwc(tape_d, dl_d, need_dx=False)
    optim_d.step()
    return reg, loss, g_adv, d_adv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vaegan.py measures on an MI355X; no GPU found")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    dm = {"width": 28, "height": 28, "channels": 1, "transforms": {"normalize": True}}
    n, L = a.batch, 100

    def logging(m):
        m.logged = {}
        m.log = lambda k, v, *x, **kw: m.logged.__setitem__(k, v)
        return m
    vg = logging(VM.VAEGAN(dm, encoder=ENC, decoder=DEC, latent_dim=L, recon_weight=1e-3, b2=0.99).to(dev).train())
    ref = logging(VM.VAEGAN(dm, encoder=ENC, decoder=DEC, latent_dim=L, recon_weight=1e-3, b2=0.99).to(dev).train())
    gan = logging(GM.GAN(dm, netG=DEC, netD=ENC, latent_dim=100).to(dev).train())
    imgs = torch.rand(n, 1, 28, 28, device=dev) * 2 - 1
    eps, prior = torch.randn(n, L, device=dev), torch.randn(n, L, device=dev)

    def fused(i):
        vg.training_step((imgs, None), i, eps=eps, prior_z=prior)

    def composed(i):
        composed_step(ref, imgs, eps, prior)

    def gan_pair(i):
        gan.training_step((imgs, None), 0)
        gan.training_step((imgs, None), 1)
    launches = {}
    for name, fn in (("fused", fused), ("composed", composed)):
        fn(0)
        l0 = K.LAUNCHES
        fn(1)
        launches[name] = K.LAUNCHES - l0
    step = {"fused": [], "composed": [], "gan_pair": []}
    for _ in range(3):
        step["fused"].append(timed(fused, a.steps, a.warmup))
        step["composed"].append(timed(composed, a.steps, a.warmup))
        step["gan_pair"].append(timed(gan_pair, a.steps, a.warmup))
    sclk_step = clock(dev)

    # ---- the new launches alone, on fixed tensors of the step's shapes
    h = (torch.randn(n, 1, 1, 2 * L, device=dev) * 0.5)
    dzz = torch.randn(2 * n, 1, 1, L, device=dev)
    feat, gbuf = torch.randn(3 * n, 4, 4, 128, device=dev), torch.randn(3 * n, 4, 4, 128, device=dev)
    dec = torch.rand(2 * n, 28, 28, 4, device=dev)[..., :1]
    dx = torch.randn(3 * n, 28, 28, 4, device=dev)[..., :1]
    hrows = h.reshape(n, 2 * L)

    def latent_hip(i):
        K.vaegan_latent_fwd(h, eps, prior)
        K.vaegan_latent_bwd(h, eps, dzz, 1.0, 1e3)

    def latent_old(i):
        z, _ = K.vae_latent_fwd(hrows, eps)
        torch.cat([z, prior])
        K.vae_latent_bwd(hrows, eps, (dzz[:n].reshape(n, L) * 1e3).contiguous(), 1.0)

    def feat_hip(i):
        K.feat_match(feat[n:2 * n], feat[2 * n:], drecon=gbuf[2 * n:], accumulate=True)

    def feat_old(i):
        diff = feat[2 * n:] - feat[n:2 * n]
        (diff * diff).sum() / n
        df = torch.zeros_like(feat)
        df[2 * n:] = diff * (2.0 / n)
        K.axpby(1.0, df, gbuf, True)

    def pack_hip(i):
        K.vaegan_pack_fwd(dec, imgs)
        K.vaegan_unpack_bwd(dx, 1e-3, 1.0)

    def pack_old(i):
        ob, dxb = _base(dec), _base(dx)
        torch.cat([ob[n:], _base(K.nchw_to_nhwc(imgs)), ob[:n]])
        torch.cat([dxb[2 * n:] * 1e-3, dxb[:n]])
    reps = max(a.steps, 500)
    ops = {}
    for name, hip, old in (("latent", latent_hip, latent_old), ("feat_match", feat_hip, feat_old), ("pack", pack_hip, pack_old)):
        ops[name] = {"hip_us": [], "composed_us": []}
        for _ in range(3):
            ops[name]["hip_us"].append(round(timed(hip, reps, 50) * 1e6, 2))
            ops[name]["composed_us"].append(round(timed(old, reps, 50) * 1e6, 2))
    sclk_ops = clock(dev)
    print(json.dumps({"metric": "vaegan_mnist_28x28_train_images_per_sec", "value": round(n / min(step["fused"]), 1), "unit": "images/s",
                      "ms_per_step_fused": [round(t * 1e3, 3) for t in step["fused"]],
                      "ms_per_step_composed": [round(t * 1e3, 3) for t in step["composed"]],
                      "ms_per_gan_pair": [round(t * 1e3, 3) for t in step["gan_pair"]], "library_launches_per_step": launches,
                      "ops_alone": ops, "model_path": "csrc/vaegan_ops.hip", "sclk_mhz_after_steps": sclk_step, "sclk_mhz_after_ops": sclk_ops,
                      "batch": n, "steps_per_repeat": a.steps, "op_reps_per_repeat": reps, "dtype": "fp32",
                      "reg_loss": round(float(vg.logged["train_loss/reg_loss"]), 4),
                      "feature_recon_loss": round(float(vg.logged["train_loss/feature_recon_loss"]), 4),
                      "d_adv_loss": round(float(vg.logged["train_loss/d_adv_loss"]), 4)}))


if __name__ == "__main__":
    main()
