"""Synthetic image data (uniform noise images in [-1,1] after normalisation) for smoke runs and
benchmarks on boxes without datasets or network.  Labels are all zero unless `label_classes` = k > 0 asks for labels drawn uniformly
from [0, k) -- by a generator of their own, so the images are the same either way (the label-conditioned models)."""
import numpy as np

from .base import ArrayImageDataset, BaseDatamodule


class SyntheticDataModule(BaseDatamodule):
    def __init__(self, width=32, height=32, channels=3, batch_size: int = 128, num_workers: int = 0,
                 train_size: int = 1024, val_size: int = 128, transforms=None, seed: int = 0, label_classes: int = 0, **kargs):
        super().__init__(width, height, channels, batch_size, num_workers, kargs.get("device_resident", "auto"))
        self.train_size, self.val_size, self.transforms, self.seed = train_size, val_size, transforms, seed
        self.label_classes = int(label_classes)

    def setup(self, stage=None):
        rng = np.random.default_rng(self.seed)
        label_rng = np.random.default_rng([self.seed, 1])          # its own stream: the images do not depend on label_classes

        def make(n):
            x = rng.integers(0, 256, size=(n, self.height, self.width, self.channels), dtype=np.uint8)
            y = label_rng.integers(0, self.label_classes, size=n, dtype=np.int64) if self.label_classes > 0 else np.zeros(n, dtype=np.int64)
            return ArrayImageDataset(x, y, self.transforms)
        self.train_data, self.val_data = make(self.train_size), make(self.val_size)
