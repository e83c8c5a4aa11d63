#!/usr/bin/env python3
"""InfoGAN on MNIST shapes (`experiment=infogan/mnist`: 1x28x28, conv_mnist nets with BatchNorm, ngf = ndf = 32, encode_dim 1024, one
10-valued code, 2 continuous codes, 62 noise dimensions, B=128, fp32, eager) on one GPU:
  step   training throughput over whole batches (phase 0 + phase 1 = both optimizers step once), next to the GAN's figure over
         generator / discriminator pairs (tools/bench_gan.py's step loop: one pair = both of ITS optimizers step once) in the same process;
  heads  the head work of one batch alone -- phase 0: both heads forward with the three losses, backward to the feature and the Q
         gradients on features [B, 1024]; phase 1: the D head forward on [2B, 1024] with its two-segment loss, backward to the feature
         and the D-head gradients -- on the kernels of csrc/info_head.hip (4 + 4 launches) next to THE SAME HEADS WRITTEN WITH torch.nn
         MODULES AND AUTOGRAD on the GPU, on the same feature tensors.  That is what a user would otherwise write, and the only
         comparator there is: no composition of the library's other kernels covers the cross-entropy.
Every pair is timed three times, alternating, with a device synchronise at the end of each window; the spread between the repeats is
the noise a difference has to clear.  The shader clock is read right behind the timed windows (K.clock_probe), as the other bench
tools record it.

    python tools/bench_infogan.py [--batch 128] [--steps 200]
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
IM = importlib.import_module("image-generation-models_amd.src.models.info_gan")
GM = importlib.import_module("image-generation-models_amd.src.models.gan")
K = importlib.import_module("image-generation-models_amd.src.ops.functional")
NETG = {"_target_": "src.networks.basic.ConvDecoder", "ngf": 32, "norm_type": "batch"}
NETD = {"_target_": "src.networks.basic.ConvEncoder", "ndf": 32, "norm_type": "batch"}


def timed(fn, steps, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_infogan.py measures on an MI355X; no GPU found")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    dm = {"width": 28, "height": 28, "channels": 1, "transforms": {"normalize": True}}
    n = a.batch

    def logging(m):
        m.logged = {}
        m.log = lambda k, v, *x, **kw: m.logged.__setitem__(k, v)
        return m
    info = logging(IM.InfoGAN(dm, netG=NETG, netD=NETD).to(dev).train())
    gan = logging(GM.GAN(dm, netG=NETG, netD=NETD, latent_dim=100).to(dev).train())
    imgs = torch.rand(n, 1, 28, 28, device=dev) * 2 - 1

    def gan_pair(i):
        gan.training_step((imgs, None), 0)
        gan.training_step((imgs, None), 1)
    step = {"infogan": [], "gan_pair": []}
    for _ in range(3):
        step["infogan"].append(timed(lambda i: info.training_step((imgs, None), i), a.steps, a.warmup))
        step["gan_pair"].append(timed(gan_pair, a.steps, a.warmup))
    try:
        sclk_step = K.clock_probe(dev, usec=300)
    except Exception:       # noqa: BLE001
        sclk_step = None

    # ---- the heads alone, on fixed features
    hp = info.hparams
    E, Dd, V, Cc, lam = int(hp.encode_dim), int(hp.discrete_dim), int(hp.discrete_value), int(hp.continuous_dim), float(hp.lambda_I)
    f0, f1 = torch.randn(n, 1, 1, E, device=dev), torch.randn(2 * n, 1, 1, E, device=dev)
    idx, cont = torch.randint(0, V, (n, Dd), device=dev), torch.rand(n, Cc, device=dev) * 2 - 1
    pq, pd = info._head_params(True), info._head_params(False)
    gq, gd = [None, None] + info.netQ.grad_tensors(), info.netD.grad_tensors() + [None] * 4

    def hip_heads(i):
        rec = K.info_head_fwd(f0, pq, [True], codes=(idx, cont, V), lambda_I=lam)
        K.info_head_bwd(pq, rec, grads=gq)
        rec = K.info_head_fwd(f1, pd, [True, False], scale=0.5)
        K.info_head_bwd(pd, rec, grads=gd)
    netD = nn.Sequential(nn.LeakyReLU(), nn.Linear(E, 1)).to(dev)
    netQ = nn.Sequential(nn.LeakyReLU(), nn.Linear(E, 128), nn.LeakyReLU(), nn.Linear(128, Dd * V + Cc)).to(dev)
    t0, t1 = f0.view(n, E).clone().requires_grad_(True), f1.view(2 * n, E).clone().requires_grad_(True)
    ones, zeros = torch.ones(n, 1, device=dev), torch.zeros(n, 1, device=dev)
    qpar, dpar = list(netQ.parameters()), list(netD.parameters())

    def torch_heads(i):
        logit, q = netD(t0), netQ(t0)
        loss = F.binary_cross_entropy_with_logits(logit, ones) + lam * (
            F.cross_entropy(q[:, :-Cc].reshape(-1, V, Dd), idx) + F.mse_loss(q[:, -Cc:], cont))
        torch.autograd.grad(loss, [t0] + qpar)
        logit = netD(t1)
        loss = (F.binary_cross_entropy_with_logits(logit[:n], ones) + F.binary_cross_entropy_with_logits(logit[n:], zeros)) / 2
        torch.autograd.grad(loss, [t1] + dpar)
    reps = max(a.steps, 500)
    heads = {"hip_us": [], "torch_us": []}
    for _ in range(3):
        heads["hip_us"].append(timed(hip_heads, reps, 50))
        heads["torch_us"].append(timed(torch_heads, reps, 50))
    try:
        sclk_heads = K.clock_probe(dev, usec=300)
    except Exception:       # noqa: BLE001
        sclk_heads = None
    for k in heads:
        heads[k] = [round(t * 1e6, 2) for t in heads[k]]
    ips = lambda v: [round(n / t, 1) for t in v]                    # noqa: E731
    print(json.dumps({"metric": "infogan_mnist_28x28_train_images_per_sec", "value": round(n / min(step["infogan"]), 1), "unit": "images/s",
                      "images_per_sec_repeats": ips(step["infogan"]), "images_per_sec_gan_pair": ips(step["gan_pair"]),
                      "ms_per_batch": [round(t * 1e3, 3) for t in step["infogan"]],
                      "ms_per_gan_pair": [round(t * 1e3, 3) for t in step["gan_pair"]], "heads_per_batch": heads,
                      "sclk_mhz_after_steps": sclk_step, "sclk_mhz_after_heads": sclk_heads, "batch": n, "steps_per_repeat": a.steps,
                      "head_reps_per_repeat": reps, "dtype": "fp32", "g_loss": round(float(info.logged["train_loss/g_loss"]), 4),
                      "I_discrete_loss": round(float(info.logged["train_loss/I_discrete_loss"]), 4),
                      "d_loss": round(float(info.logged["train_loss/d_loss"]), 4)}))


if __name__ == "__main__":
    main()
