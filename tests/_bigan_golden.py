"""The BiGAN golden vectors (tools/gen_golden_bigan.py) are three files, each below the 1 MiB limit for a committed file:
bigan_kats.npz (init, tiny.sd0, tiny.vanilla, settings), bigan_modes_kats.npz (tiny.lsgan, tiny.hinge) and bigan_traj_kats.npz (traj).
`load` reads them as one mapping with np.load's surface (`files`, `[key]`)."""
import os

import numpy as np

FILES = ("bigan_kats.npz", "bigan_modes_kats.npz", "bigan_traj_kats.npz")


class Golden:
    def __init__(self, golden_dir):
        self.paths = [os.path.join(golden_dir, f) for f in FILES]
        self._parts = [np.load(p) for p in self.paths]
        self._where = {k: part for part in self._parts for k in part.files}
        self.files = list(self._where)

    def __getitem__(self, key):
        return self._where[key][key]

    def __contains__(self, key):
        return key in self._where


def load(golden_dir):
    return Golden(golden_dir)
