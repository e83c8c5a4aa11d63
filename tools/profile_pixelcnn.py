#!/usr/bin/env python3
"""The PixelCNN workloads profiled under `rocprofv3 --kernel-trace --stats` (profiles/pixelcnn_*_kernel_stats.csv):
`train`: 3 class-conditional training steps at B = 128, 3 x 32 x 32, hidden 64; `sample`: one sampling run of 16 x 1 x 28 x 28.

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/profile_pixelcnn.py train|sample
"""
import os
import sys
import types

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-generation-models_amd"))

import torch  # noqa: E402


def main(what):
    from src.models.pixelcnn import PixelCNN
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if what == "train":
        dm = types.SimpleNamespace(width=32, height=32, channels=3, transforms=types.SimpleNamespace(normalize=False))
        m = PixelCNN(dm, 64, class_condition=True, n_classes=10).to(dev).train()
        opt = m.configure_optimizers()[0][0]
        x = torch.randint(0, 256, (128, 3, 32, 32), device=dev).float() / 255
        y = torch.randint(0, 10, (128,), device=dev)
        for _ in range(3):
            m.training_step((x, y), 0).backward()
            opt.step()
    else:
        dm = types.SimpleNamespace(width=28, height=28, channels=1, transforms=types.SimpleNamespace(normalize=False))
        m = PixelCNN(dm, 64).to(dev).eval()
        m.sample((16, 1, 28, 28))
    torch.cuda.synchronize()
    print("done", what)


if __name__ == "__main__":
    main(sys.argv[1])
