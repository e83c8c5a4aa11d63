#!/usr/bin/env python3
"""GAN on MNIST shapes (`experiment=vanilla_gan/mnist_conv`: 1x28x28, latent 100, conv_mnist nets with BatchNorm, ngf = ndf = 32,
B=128, fp32, eager) training throughput on one GPU over alternating generator / discriminator phases, and the time of the
discriminator phase's norm + activation work alone, on the tensors that phase normalises ([2N, 7, 7, 64] and [2N, 4, 4, 128], forward
and backward with parameter gradients):
  seg   the segmented kernels (csrc/bn_seg.hip): one two-segment call per layer and direction, 2 launches each -- 8 launches;
  base  the same tensors through K.batchnorm_fwd + K.leaky_relu_fwd and K.leaky_relu_bwd + K.batchnorm_bwd, called once per segment
        (the kernels the nets ran before the segmented ones existed): 4 launches per layer, direction and segment -- 32 launches.
Both are timed three times, alternating, with a device synchronise at the end of each window; the spread between the repeats is the
noise a difference has to clear.  The whole step is also timed with the nets switched to the per-segment kernels.

    python tools/bench_gan.py [--batch 128] [--steps 200]
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
M = importlib.import_module("image-generation-models_amd.src.models.gan")
K = importlib.import_module("image-generation-models_amd.src.ops.functional")


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
        raise SystemExit("bench_gan.py measures on an MI355X; no GPU found")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    dm = {"width": 28, "height": 28, "channels": 1, "transforms": {"normalize": True}}
    n = a.batch

    def model(segmented):
        m = M.GAN(dm, netG={"_target_": "src.networks.basic.ConvDecoder", "ngf": 32, "norm_type": "batch"},
                  netD={"_target_": "src.networks.basic.ConvEncoder", "ndf": 32, "norm_type": "batch"}, latent_dim=100).to(dev).train()
        m.netG.use_fused_norm_act(segmented)
        m.netD.use_fused_norm_act(segmented)
        m.logged = {}
        m.log = lambda k, v, *x, **kw: m.logged.__setitem__(k, v)
        return m
    imgs = torch.rand(n, 1, 28, 28, device=dev) * 2 - 1
    m_seg, m_base = model(True), model(False)
    steps = a.steps + a.steps % 2                                  # whole generator / discriminator pairs
    step = {"seg": [], "base": []}
    for _ in range(3):
        step["seg"].append(timed(lambda i: m_seg.training_step((imgs, None), i), steps, a.warmup))
        step["base"].append(timed(lambda i: m_base.training_step((imgs, None), i), steps, a.warmup))

    # the discriminator phase's norm + activation work alone
    layers = []
    for hw, c in ((7, 64), (4, 128)):
        x, dy = torch.randn(2 * n, hw, hw, c, device=dev), torch.randn(2 * n, hw, hw, c, device=dev)
        layers.append((x, dy, torch.ones(c, device=dev), torch.zeros(c, device=dev), torch.zeros(c, device=dev), torch.ones(c, device=dev),
                       torch.zeros(c, device=dev), torch.zeros(c, device=dev)))

    def seg(i):
        for x, dy, g, b, rm, rv, dg, db in layers:
            y, mean, rstd = K.bn_seg_fwd(x, g, b, 2, rm, rv, act="leaky_relu", slope=0.2)
            K.bn_seg_bwd(x, mean, rstd, g, y, dy, act="leaky_relu", slope=0.2, dgamma=dg, dbeta=db, out=dy)

    def base(i):
        for x, dy, g, b, rm, rv, dg, db in layers:
            for s in range(2):
                xs, ds = x[s * n:(s + 1) * n], dy[s * n:(s + 1) * n]
                y, mean, rstd = K.batchnorm_fwd(xs, g, b, rm, rv)
                K.leaky_relu_fwd(y, 0.2, inplace=True)
                K.leaky_relu_bwd(y, ds, 0.2, out=ds)
                K.batchnorm_bwd(xs, mean, rstd, g, ds, dgamma=dg, dbeta=db, out=ds)
    reps = max(a.steps, 500)
    norm = {"seg": [], "base": []}
    for _ in range(3):
        norm["seg"].append(timed(seg, reps, a.warmup))
        norm["base"].append(timed(base, reps, a.warmup))
    us = lambda v: [round(t * 1e6, 1) for t in v]                   # noqa: E731
    print(json.dumps({"metric": "gan_mnist_28x28_train_images_per_sec", "value": round(n / min(step["seg"]), 1), "unit": "images/s",
                      "images_per_sec_repeats": [round(n / t, 1) for t in step["seg"]],
                      "images_per_sec_per_segment_kernels": [round(n / t, 1) for t in step["base"]],
                      "ms_per_step": [round(t * 1e3, 3) for t in step["seg"]], "norm_act_seg_us": us(norm["seg"]), "norm_act_seg_launches": 8,
                      "norm_act_per_segment_us": us(norm["base"]), "norm_act_per_segment_launches": 32, "batch": n, "dtype": "fp32",
                      "model_path": "segmented" if M.SEGMENTED_NORM else "per segment",
                      "g_loss": round(float(m_seg.logged["train_loss/g_loss"]), 4), "d_loss": round(float(m_seg.logged["train_loss/d_loss"]), 4)}))


if __name__ == "__main__":
    main()
