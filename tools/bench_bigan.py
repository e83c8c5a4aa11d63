#!/usr/bin/env python3
"""BiGAN on MNIST shapes (`experiment=bigan/mnist`: 1x28x28, conv_mnist nets with BatchNorm, ngf = ndf = 32, latent 100, hidden 128,
B=128, fp32, eager) on one GPU:
  step     whole training steps (both optimizers step every batch) with the library launches of one step (K.LAUNCHES; for the pair head
           it counts kernels), next to the GAN's generator + discriminator pair at the same batch size in the same process, for scale;
  head     the head work of one step -- forward plus both backwards -- on the fused kernels of csrc/pair_disc.hip, next to the same head
           written with torch.nn modules and autograd on the same tensors (two calls, two backwards through one retained graph, as
           the reference does it);
  bwd      the two right-hand sides of the head's backward in one call against two calls.
Every pair is timed three times, alternating, with a device synchronise at the end of each window; the spread between the repeats is
the noise a difference has to clear.  The shader clock is read right behind the timed windows (K.clock_probe).

    python tools/bench_bigan.py [--batch 128] [--steps 100]
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
BM = importlib.import_module("image-generation-models_amd.src.models.BiGAN")
GM = importlib.import_module("image-generation-models_amd.src.models.gan")
K = importlib.import_module("image-generation-models_amd.src.ops.functional")
DEC = {"_target_": "src.networks.basic.ConvDecoder", "ngf": 32, "norm_type": "batch"}
ENC = {"_target_": "src.networks.basic.ConvEncoder", "ndf": 32, "norm_type": "batch"}
H = 128


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


def torch_head(L):
    """dis_z and dis_pair as torch.nn modules: the reference's layers."""
    def block(i, o, norm):
        return [nn.Linear(i, o), norm, nn.LeakyReLU(0.2)]
    dis_z = nn.Sequential(*block(L, H, nn.GroupNorm(1, H)), *block(H, H, nn.BatchNorm1d(H)), nn.Linear(H, H), nn.LeakyReLU(0.2))
    dis_pair = nn.Sequential(*block(2 * H, H, nn.GroupNorm(1, H)), nn.Linear(H, 1))
    return dis_z, dis_pair


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bigan.py measures on an MI355X; no GPU found")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    dm = {"width": 28, "height": 28, "channels": 1, "transforms": {"normalize": True}}
    n, L = a.batch, 100

    def logging(m):
        m.logged = {}
        m.log = lambda k, v, *x, **kw: m.logged.__setitem__(k, v)
        return m
    bg = logging(BM.BiGAN(dm, encoder=ENC, decoder=DEC, latent_dim=L, hidden_dim=H).to(dev).train())
    gan = logging(GM.GAN(dm, netG=DEC, netD=ENC, latent_dim=100).to(dev).train())
    imgs = torch.rand(n, 1, 28, 28, device=dev) * 2 - 1
    z = torch.randn(n, L, device=dev)

    def bigan(i):
        bg.training_step((imgs, None), i, z=z)

    def gan_pair(i):
        gan.training_step((imgs, None), 0)
        gan.training_step((imgs, None), 1)
    bigan(0)
    l0 = K.LAUNCHES
    bigan(1)
    launches = K.LAUNCHES - l0
    step = {"bigan": [], "gan_pair": []}
    for _ in range(3):
        step["bigan"].append(timed(bigan, a.steps, a.warmup))
        step["gan_pair"].append(timed(gan_pair, a.steps, a.warmup))
    sclk_step = clock(dev)

    # ---- the head work of one step on fixed tensors of the step's shapes
    D = bg.discriminator
    e, xf = torch.randn(n, L, device=dev), torch.randn(2 * n, H, device=dev)
    params = D._params(D.dis_z._sv, D.dis_pair._sv)
    D.dis_z.flat_grads, D.dis_pair.flat_grads
    grads = D._params(D.dis_z._gv, D.dis_pair._gv)
    dxf, de, dxf_d = torch.empty(2 * n, H, device=dev), torch.empty(n, L, device=dev), torch.empty(2 * n, H, device=dev)
    bn = "model.1.norm."
    buf = D.dis_z._buffer

    def fwd():
        return K.pair_disc_fwd(params, e, z, xf, "vanilla", True, buf(bn + "running_mean"), buf(bn + "running_var"), buf(bn + "num_batches_tracked"))

    def head_hip(i):
        rec = fwd()
        K.pair_disc_bwd(params, rec, dxf=dxf, de=de)
        K.pair_disc_bwd(params, rec, grads=grads, dxf_d=dxf_d)

    def head_hip_joint(i):
        rec = fwd()
        K.pair_disc_bwd(params, rec, dxf=dxf, de=de, grads=grads, dxf_d=dxf_d)
    tz, tp = (m.to(dev).train() for m in torch_head(L))
    tparams = list(tz.parameters()) + list(tp.parameters())
    te, txf = e.clone().requires_grad_(True), xf.clone().requires_grad_(True)

    def bce(x, real):
        return F.binary_cross_entropy_with_logits(x, torch.ones_like(x) if real else torch.zeros_like(x))

    def head_torch(i):
        real = tp(torch.cat((tz(te), txf[:n]), dim=1))
        fake = tp(torch.cat((tz(z), txf[n:]), dim=1))
        g_loss = bce(real, False) + bce(fake, True)
        d_loss = bce(real, True) + bce(fake, False)
        torch.autograd.grad(g_loss, [te, txf], retain_graph=True)
        torch.autograd.grad(d_loss, tparams + [txf])
    l0 = K.LAUNCHES
    head_hip(0)
    head_launches = K.LAUNCHES - l0
    l0 = K.LAUNCHES
    head_hip_joint(0)
    joint_launches = K.LAUNCHES - l0
    reps = max(a.steps, 300)
    head = {"hip_us": [], "hip_joint_us": [], "torch_us": []}
    for _ in range(3):
        head["hip_us"].append(round(timed(head_hip, reps, 30) * 1e6, 2))
        head["hip_joint_us"].append(round(timed(head_hip_joint, reps, 30) * 1e6, 2))
        head["torch_us"].append(round(timed(head_torch, reps, 30) * 1e6, 2))
    sclk_head = clock(dev)
    print(json.dumps({"metric": "bigan_mnist_28x28_train_images_per_sec", "value": round(n / min(step["bigan"]), 1), "unit": "images/s",
                      "ms_per_step": [round(t * 1e3, 3) for t in step["bigan"]],
                      "ms_per_gan_pair": [round(t * 1e3, 3) for t in step["gan_pair"]], "library_launches_per_step": launches,
                      "head_alone": head, "head_kernels": {"two_calls": head_launches, "joint": joint_launches},
                      "model_path": "csrc/pair_disc.hip", "sclk_mhz_after_steps": sclk_step, "sclk_mhz_after_head": sclk_head,
                      "batch": n, "steps_per_repeat": a.steps, "head_reps_per_repeat": reps, "dtype": "fp32",
                      "g_loss": round(float(bg.logged["train_loss/g_loss"]), 4), "d_loss": round(float(bg.logged["train_loss/d_loss"]), 4)}))


if __name__ == "__main__":
    main()
