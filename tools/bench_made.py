#!/usr/bin/env python3
"""MADE on one MI355X against the reference's computation written fresh with PyTorch-ROCm ops on the same GPU.

Legs (one JSON line each): the training step at the reference config (B = 128, 1 x 28 x 28, hidden 1024, 3 layers) in fp32 and
bf16, eager and as the graph the trainer replays; the sampler's wall time for 64 and 128 x 1 x 28 x 28; the shader clock.  The
baseline is F.linear(x, W * mask, b) + sigmoid, F.cross_entropy and torch.optim.Adam (autocast to bf16 in the bf16 leg); its
sampler is the reference's loop of full forwards.  HIP and baseline run alternately, three repeats each; the condition per mode
is HIP <= baseline min + baseline spread (max - min), and for the sampler HIP < baseline.

    python tools/bench_made.py [--steps 10] [--warmup 3] [--no-sample]
"""
import argparse
import json
import math
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-generation-models_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK = {"fp32": 157.3e12, "bf16": 2.5e15}      # dense matrix peaks (MI355X_MICROARCH.md); HBM 8.0 TB/s spec
HBM = 8.0e12
B, CH, HW, HID, NL = 128, 1, 28, 1024, 3
D = CH * HW * HW


def dims():
    return [D] + [HID] * NL + [D * 256]


def counts(live_frac):
    """Algorithmic counts of one training step from the shapes: dense FLOPs (3 GEMM passes per layer, the input layer's data
    gradient skipped), live-only FLOPs (the same on the unmasked entries only), and HBM bytes: the head weight read by the forward,
    the dlogits recompute and the data gradient, its gradient written once, dlogits written and read twice (fp32), and Adam's pass
    (param, grad, m, v read; param, m, v written: 7 x 4 bytes per parameter)."""
    ds = dims()
    dense = live = 0.0
    for i, (fi, fo) in enumerate(zip(ds[:-1], ds[1:])):
        passes = 3 if i > 0 else 2
        if i == len(ds) - 2:
            passes += 1                                      # the head's dlogits recompute
        dense += passes * 2 * B * fi * fo
        live += passes * 2 * B * fi * fo * live_frac[i]
    nparam = sum(fi * fo + fo for fi, fo in zip(ds[:-1], ds[1:]))
    head_w = ds[-2] * ds[-1] * 4
    byts = 3 * head_w + head_w + 3 * B * ds[-1] * 4 + 7 * 4 * nparam
    return dense, live, byts, nparam


def _dm():
    return types.SimpleNamespace(width=HW, height=HW, channels=CH, transforms=types.SimpleNamespace(normalize=False))


class Baseline(torch.nn.Module):
    """The reference's computation with PyTorch ops (masked linear = F.linear(x, W * mask, b))."""

    def __init__(self, made):
        super().__init__()
        self.w = torch.nn.ParameterList()
        self.b = torch.nn.ParameterList()
        for i, layer in enumerate(made.model.layers):
            self.w.append(torch.nn.Parameter(layer.model.weight.detach().clone()))
            self.b.append(torch.nn.Parameter(layer.model.bias.detach().clone()))
            self.register_buffer(f"mask{i}", layer.mask.clone())

    @property
    def masks(self):
        return [getattr(self, f"mask{i}") for i in range(len(self.w))]

    def forward(self, x):
        n, c, h, w = x.shape
        y = x.reshape(n, -1)
        for i in range(len(self.w) - 1):
            y = torch.sigmoid(F.linear(y, self.w[i] * self.masks[i], self.b[i]))
        y = F.linear(y, self.w[-1] * self.masks[-1], self.b[-1])
        return y.reshape(n, c, h, w, 256).permute(0, 4, 1, 2, 3)

    def bpd(self, x):
        nll = F.cross_entropy(self.forward(x), (x * 255).long(), reduction="none")
        return (nll.mean([1, 2, 3]) / math.log(2.0)).mean()


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, out


def bench_train(mode, steps, warmup, x):
    from src.models.made import MADE
    from src.runtime.graphed import GraphedTrainStep
    from src.runtime.optim import FlatAdam
    dev = x.device
    torch.manual_seed(0)
    m = MADE(_dm(), HID, NL)
    m.compute_mode = mode
    live_frac = [float(l.mask.float().mean()) for l in m.model.layers]
    base = Baseline(m).to(dev)
    m.to(dev).train()
    opt = FlatAdam(m, lr=1e-3)
    gm = MADE(_dm(), HID, NL)
    gm.compute_mode = mode
    gm.to(dev).train()
    gopt = FlatAdam(gm, lr=1e-3, device_state=True)
    lab = torch.zeros(B, dtype=torch.int64, device=dev)
    bopt = torch.optim.Adam(base.parameters(), lr=1e-3)

    def hip_step():
        loss = m.training_step((x, lab), 0)
        loss.backward()
        opt.step()
        return loss

    def base_step():
        bopt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=(mode == "bf16")):
            loss = base.bpd(x)
        loss.backward()
        bopt.step()
        return loss

    for _ in range(warmup):
        hip_step()
        base_step()
    gs = GraphedTrainStep(gm, gopt, (x, lab), warmup=warmup)
    res = {"eager": [], "graph": [], "torch": []}
    for _ in range(3):
        res["eager"].append(timed(hip_step, steps)[0])
        res["graph"].append(timed(lambda: gs((x, lab)), steps)[0])
        res["torch"].append(timed(base_step, steps)[0])
    dense, live, byts, nparam = counts(live_frac)
    t = {k: min(v) for k, v in res.items()}
    spread = max(res["torch"]) - min(res["torch"])
    out = []
    for k in ("eager", "graph", "torch"):
        dt = t[k]
        bound = "mfma" if mode == "fp32" else "hbm"
        out.append({"leg": f"train_made_{mode}_{k}", "batch": B, "ms_per_step": round(dt * 1e3, 3), "images_per_sec": round(B / dt, 1),
                    "ms_repeats": [round(v * 1e3, 3) for v in res[k]],
                    "dense_tflops": round(dense / dt / 1e12, 2), "live_tflops": round(live / dt / 1e12, 2),
                    "mfma_peak_frac_dense": round(dense / dt / PEAK[mode], 4), "hbm_frac": round(byts / dt / HBM, 4),
                    "bound": bound, "params": nparam})
    cond = {"leg": f"train_made_{mode}_condition", "hip_graph_ms": round(t["graph"] * 1e3, 3), "hip_eager_ms": round(t["eager"] * 1e3, 3),
            "torch_ms": round(t["torch"] * 1e3, 3), "torch_spread_ms": round(spread * 1e3, 3),
            "ratio_torch_over_graph": round(t["torch"] / t["graph"], 3),
            "ok_graph": t["graph"] <= t["torch"] + spread, "ok_eager": t["eager"] <= t["torch"] + spread}
    return out + [cond]


def bench_sample(N, reps):
    from src.models.made import MADE
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = MADE(_dm(), HID, NL)
    base = Baseline(m).to(dev)
    m.to(dev).eval()
    m.sample((N, CH, HW, HW))                  # capture + one run

    @torch.no_grad()
    def base_sample():
        img = torch.full((N, CH, HW, HW), -1.0, device=dev)
        for h in range(HW):
            for w in range(HW):
                pred = base(img)
                probs = F.softmax(pred[:, :, :, h, w].permute(0, 2, 1), dim=-1).reshape(N * CH, 256)
                img[:, :, h, w] = (torch.multinomial(probs, 1).squeeze(-1).float() / 255).reshape(N, CH)
        return img

    hip, tor = [], []
    for _ in range(reps):
        hip.append(timed(lambda: m.sample((N, CH, HW, HW)), 1)[0])
        tor.append(timed(base_sample, 1)[0])
    return {"leg": f"sample_made_{N}x{CH}x{HW}x{HW}_fp32", "hip_wall_s": round(min(hip), 4), "torch_wall_s": round(min(tor), 4),
            "hip_repeats": [round(v, 4) for v in hip], "torch_repeats": [round(v, 4) for v in tor],
            "speedup": round(min(tor) / min(hip), 2), "ok": max(hip) < min(tor)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample-reps", type=int, default=3)
    ap.add_argument("--no-sample", action="store_true")
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    from src.ops import functional as K
    dev = torch.device("cuda:0")
    try:
        sclk = K.clock_probe(dev, usec=300)
    except Exception:       # noqa: BLE001
        sclk = None
    print(json.dumps({"leg": "sclk", "sclk_mhz": sclk}), flush=True)
    torch.manual_seed(1)
    x = torch.randint(0, 256, (B, CH, HW, HW), device=dev).float() / 255
    if not a.no_train:
        for mode in ("fp32", "bf16"):
            for rec in bench_train(mode, a.steps, a.warmup, x):
                print(json.dumps(rec), flush=True)
            torch.cuda.empty_cache()
    if not a.no_sample:
        for N in (64, 128):
            print(json.dumps(bench_sample(N, a.sample_reps)), flush=True)
    try:
        print(json.dumps({"leg": "sclk_end", "sclk_mhz": K.clock_probe(dev, usec=300)}), flush=True)
    except Exception:       # noqa: BLE001
        pass


if __name__ == "__main__":
    main()
