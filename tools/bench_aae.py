#!/usr/bin/env python3
"""AAE on MNIST shapes (`experiment=aae/mnist`: 1x28x28, latent 8, conv_mnist nets with BatchNorm, ngf = ndf = 32, B=128, fp32, eager)
training-step throughput on one GPU, and the time of the step's latent-discriminator work alone:
  new   the row-local LayerNorm discriminator (csrc/latent_disc_ln.hip) as the step runs it: one 2N-row pass over [prior | q_z] forward
        and its parameter backward (4 launches), then the N-row generator pass forward and its input-gradient backward (3 launches);
  old   the same rows through the FactorVAE's BatchNorm discriminator (csrc/latent_disc.hip) the way that model runs it: two separate
        N-row passes forward with both parameter backwards into one buffer (2 + 2 + 3 + 3 launches), then the N-row generator pass
        forward and its input-gradient backward (2 + 2 launches).  A different network (BatchNorm1d in the second layer): the yardstick for
        what the batch-wide statistics cost, not an alternative implementation of the AAE.

    python tools/bench_aae.py [--batch 128] [--steps 100]
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
M = importlib.import_module("image-generation-models_amd.src.models.aae")


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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    MLPEncoder = importlib.import_module("image-generation-models_amd.src.networks.basic").MLPEncoder
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    dm = {"width": 28, "height": 28, "channels": 1, "transforms": {"normalize": True}}
    L, n = 8, a.batch
    m = M.AAE(dm, encoder={"_target_": "src.networks.basic.ConvEncoder", "ndf": 32, "norm_type": "batch"},
              decoder={"_target_": "src.networks.basic.ConvDecoder", "ngf": 32, "norm_type": "batch"}, latent_dim=L).to(dev)
    m.train()
    logged = {}
    m.log = lambda k, v, *x, **kw: logged.__setitem__(k, v)
    imgs = torch.rand(n, 1, 28, 28, device=dev) * 2 - 1
    step_s = timed(lambda i: m.training_step((imgs, None), i), a.steps, a.warmup)

    # the discriminator work of one step, alone: same rows for both networks
    prior = torch.randn(n, L, device=dev)
    qz = torch.randn(n, 1, 1, L, device=dev)[:, 0, 0, :]
    dq = torch.zeros(n, L, device=dev)
    D = m.discriminator

    def new(i):
        rec = D.disc_forward(prior, 1.0, x1=qz, target1=0.0)
        D.disc_backward(rec, 1.0, 0.0, c0=0.5, c1=0.5)
        gen = D.disc_forward(qz, 1.0)
        D.disc_backward(gen, 1.0, param_grads=False, dx0=dq)

    B = MLPEncoder(input_channel=L, hidden_dims=[256, 256], output_channel=1, width=1, height=1).to(dev).train()

    def old(i):
        real = B.disc_forward(1.0, z=prior)
        fake = B.disc_forward(0.0, z=qz)
        B.disc_backward(real, 1.0, accumulate=False, scale=0.5)
        B.disc_backward(fake, 0.0, accumulate=True, scale=0.5)
        gen = B.disc_forward(1.0, z=qz)
        B.disc_backward(gen, 1.0, param_grads=False, dz=dq)

    reps = max(a.steps, 200)
    new_s, old_s = timed(new, reps, a.warmup), timed(old, reps, a.warmup)
    new_s2, old_s2 = timed(new, reps, a.warmup), timed(old, reps, a.warmup)          # interleaved a second time: the spread is reported
    print(json.dumps({"metric": "aae_mnist_28x28_train_images_per_sec", "value": round(n / step_s, 1), "unit": "images/s",
                      "ms_per_step": round(step_s * 1e3, 3), "disc_ln_us": [round(new_s * 1e6, 1), round(new_s2 * 1e6, 1)], "disc_ln_launches": 7,
                      "disc_bn_us": [round(old_s * 1e6, 1), round(old_s2 * 1e6, 1)], "disc_bn_launches": 14, "batch": n, "dtype": "fp32",
                      "recon_loss": round(float(logged["train_loss/recon_loss"]), 4), "d_loss": round(float(logged["train_loss/d_loss"]), 4)}))


if __name__ == "__main__":
    main()
