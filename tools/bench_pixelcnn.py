#!/usr/bin/env python3
"""PixelCNN throughput on one MI355X: training images/s (B = 128, hidden 64) for MNIST 1x28x28 and CIFAR 3x32x32 in both compute
modes with the shader clock, sampler wall time for 64 x 1 x 28 x 28 and 64 x 3 x 32 x 32, and roofline fractions from the
algorithmic FLOPs and bytes kept here.  Prints one JSON line per leg.

    python tools/bench_pixelcnn.py [--steps 20] [--warmup 5] [--no-sample]
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-generation-models_amd"))

import torch  # noqa: E402

PEAK = {"fp32": 157.3e12, "bf16": 2.5e15}      # dense matrix peaks (spec); HBM 8.0 TB/s
HBM = 8.0e12
LAYERS = 11


def fwd_flops_per_pixel(C, ch):
    """Algorithmic forward FLOPs per pixel (live taps only): first convs, 11 gated layers, head."""
    first = 2 * (10 + 2) * ch * C
    layer = 2 * 6 * C * 2 * C + 2 * (2 * C + 2 * C) * 2 * C + 2 * C * C
    head = 2 * C * 256 * ch
    return first + LAYERS * layer + head


def train_bytes_per_pixel(C, ch):
    """Algorithmic HBM bytes of a training step per pixel: every activation the step writes once and reads once (fp32), forward
    (vpre 2C, vout C, hpre 2C, g C, hout C per layer) and backward (about twice that), plus the dlogits tensor (256 ch) written
    and read three times."""
    layer_fwd = (2 + 1 + 2 + 1 + 1) * C * 4 * 2
    return LAYERS * layer_fwd * 3 + 256 * ch * 4 * 4


def _dm(ch, hw):
    return types.SimpleNamespace(width=hw, height=hw, channels=ch, transforms=types.SimpleNamespace(normalize=False))


def bench_train(ch, hw, mode, B, steps, warmup):
    from src.models.pixelcnn import PixelCNN
    from src.ops import functional as K
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = PixelCNN(_dm(ch, hw), 64)
    m.compute_mode = mode
    m.to(dev).train()
    opt = m.configure_optimizers()[0][0]
    x = (torch.randint(0, 256, (B, ch, hw, hw), device=dev).float() / 255)
    for _ in range(warmup):
        m.training_step((x, None), 0).backward()
        opt.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = m.training_step((x, None), 0)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    try:
        sclk = K.clock_probe(dev, usec=300)
    except Exception:       # noqa: BLE001
        sclk = None
    px = B * hw * hw
    flops = 3 * fwd_flops_per_pixel(64, ch) * px
    byts = train_bytes_per_pixel(64, ch) * px
    return {"leg": f"train_{ch}x{hw}x{hw}_{mode}", "batch": B, "ms_per_step": round(dt * 1e3, 3), "images_per_sec": round(B / dt, 1),
            "sclk_mhz": sclk, "final_bpd": round(float(loss), 5), "tflops": round(flops / dt / 1e12, 2),
            "mfma_peak_frac": round(flops / dt / PEAK[mode], 4), "hbm_frac": round(byts / dt / HBM, 4)}


def bench_sample(ch, hw, N):
    from src.models.pixelcnn import PixelCNN
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = PixelCNN(_dm(ch, hw), 64).to(dev).eval()
    m.sample((N, ch, hw, hw))                  # capture + one run
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    img = m.sample((N, ch, hw, hw))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    flops = fwd_flops_per_pixel(64, ch) * N * hw * hw * hw * hw
    return {"leg": f"sample_{N}x{ch}x{hw}x{hw}_fp32", "wall_s": round(dt, 3), "ms_per_pixel_step": round(dt / (hw * hw) * 1e3, 3),
            "tflops": round(flops / dt / 1e12, 2), "mfma_peak_frac": round(flops / dt / PEAK["fp32"], 4),
            "finite": bool(torch.isfinite(img).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--no-sample", action="store_true")
    a = ap.parse_args()
    for ch, hw in ((1, 28), (3, 32)):
        for mode in ("fp32", "bf16"):
            print(json.dumps(bench_train(ch, hw, mode, a.batch, a.steps, a.warmup)), flush=True)
    if not a.no_sample:
        for ch, hw in ((1, 28), (3, 32)):
            print(json.dumps(bench_sample(ch, hw, 64)), flush=True)


if __name__ == "__main__":
    main()
