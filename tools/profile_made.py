#!/usr/bin/env python3
"""One graphed MADE training step at the reference config (B = 128, 1 x 28 x 28, hidden 1024, 3 layers, fp32) profiled under
`rocprofv3 --kernel-trace --stats` (profiles/made_train_kernel_stats.csv).  The capture's warm-up runs eagerly first; the
trace then holds those steps and one replay.

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/profile_made.py
"""
import os
import sys
import types

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-generation-models_amd"))

import torch  # noqa: E402


def main():
    from src.models.made import MADE
    from src.runtime.graphed import GraphedTrainStep
    from src.runtime.optim import FlatAdam
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    dm = types.SimpleNamespace(width=28, height=28, channels=1, transforms=types.SimpleNamespace(normalize=False))
    m = MADE(dm, 1024, 3).to(dev).train()
    opt = FlatAdam(m, lr=1e-3, device_state=True)
    x = torch.randint(0, 256, (128, 1, 28, 28), device=dev).float() / 255
    lab = torch.zeros(128, dtype=torch.int64, device=dev)
    gs = GraphedTrainStep(m, opt, (x, lab), warmup=1)
    gs((x, lab))
    torch.cuda.synchronize()
    print("done")


if __name__ == "__main__":
    main()
