#!/usr/bin/env python3
"""Golden vectors for the PixelCNN path, produced by the REFERENCE PixelCNN (src/models/pixelcnn.py).

Runs only in the build container: imports the reference with the import stubs of tools/gen_golden_vae.py and writes plain arrays
to tests/golden/pixelcnn_kats.npz:
  keys / shapes : state_dict keys in order and their shapes at hidden_dim 64 (1 channel, unconditioned; 3 channels, 10 classes);
  sha64         : sha256 of the seeded init (torch.manual_seed(0)) at hidden_dim 64, 1 channel, unconditioned;
  u / c         : a tiny unconditioned net (hidden 8, 4 x 1 x 28 x 28, normalize False) and a tiny conditioned one (hidden 8,
                  3 x 3 x 8 x 8, 10 classes, normalize True): weights perturbed away from init (masked entries non-zero), inputs
                  k / 255 (2k / 255 - 1), logits at 64 fixed (sample, colour, row, col) positions, the bpd, every gradient, a
                  5-step Adam(1e-3) trajectory (per-step bpd, the parameter vector's norm under the masks after every step, every
                  tensor's displacement after step 5), and the reference's own CPU bf16-autocast logits error at the same positions
                  (max abs / max |fp32 logits|): the bf16 budget.

    python tools/gen_golden_pixelcnn.py
"""
import hashlib
import os
import types

import numpy as np
import torch

from gen_golden_vae import OUT, import_reference  # noqa: F401  (same stubs)


def _ref():
    import_reference()
    from src.models import pixelcnn
    return pixelcnn


def build(ref, hidden, ch, H, W, normalize, n_classes=None):
    dm = types.SimpleNamespace(width=W, height=H, channels=ch, transforms=types.SimpleNamespace(normalize=normalize))
    m = ref.PixelCNN(dm, hidden, class_condition=n_classes is not None, n_classes=n_classes)
    m.hparams = types.SimpleNamespace(hidden_dim=hidden, class_condition=n_classes is not None, n_classes=n_classes, lr=1e-3)
    m.input_normalize = normalize
    m.logged = {}
    return m


def sd_sha(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().contiguous().numpy().astype(np.float32).tobytes())
    return h.hexdigest()


def case(ref, out, tag, hidden, n, ch, H, W, normalize, n_classes):
    torch.manual_seed(7 + n)
    m = build(ref, hidden, ch, H, W, normalize, n_classes)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    for k, v in m.state_dict().items():
        out[f"{tag}.sd0.{k}"] = v.numpy().copy()
    k = torch.randint(0, 256, (n, ch, H, W))
    x = k.float() / 255 if not normalize else k.float() * 2 / 255 - 1
    out[f"{tag}.x"] = x.numpy()
    y = None
    if n_classes:
        lab = torch.randint(0, n_classes, (n,))
        out[f"{tag}.labels"] = lab.numpy()
        y = torch.nn.functional.one_hot(lab, n_classes).float()
    g = torch.Generator().manual_seed(3)
    pos = np.stack([torch.randint(0, s, (64,), generator=g).numpy() for s in (n, ch, H, W)], 1)
    out[f"{tag}.pos"] = pos
    pre = {kk: v.clone() for kk, v in m.state_dict().items()}
    with torch.no_grad():
        logits = m.forward(x, y)
    m.load_state_dict(pre)                              # forward masked the weights in place; the step below starts from sd0 again
    out[f"{tag}.logits"] = logits[pos[:, 0], :, pos[:, 1], pos[:, 2], pos[:, 3]].numpy()
    m.load_state_dict(pre)
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        lb = m.forward(x, y).float()
    m.load_state_dict(pre)
    sel = lambda t: t[pos[:, 0], :, pos[:, 1], pos[:, 2], pos[:, 3]]
    out[f"{tag}.bf16_err"] = np.float32(float((sel(lb) - sel(logits)).abs().max()) / float(sel(logits).abs().max()))
    bpd = m.calc_likelihood(x, y)
    bpd.backward()
    out[f"{tag}.bpd"] = np.float32(bpd.item())
    for kk, p in m.named_parameters():
        out[f"{tag}.grad.{kk}"] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
    # 5 Adam steps (StepLR steps per epoch, so lr stays 1e-3)
    m.load_state_dict(pre)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    masks = {kk[:-5]: v for kk, v in m.state_dict().items() if kk.endswith(".mask")}
    traj, wn = [], []
    for _ in range(5):
        opt.zero_grad()
        b = m.calc_likelihood(x, y)
        b.backward()
        opt.step()
        traj.append(b.item())
        sq = 0.0
        for kk, p in m.named_parameters():
            mk = masks.get(kk[:-len(".conv.weight")]) if kk.endswith(".conv.weight") else None
            sq += float(((p.detach() * mk) if mk is not None else p.detach()).double().pow(2).sum())
        wn.append(sq ** 0.5)
    out[f"{tag}.traj_bpd"] = np.array(traj, np.float32)
    out[f"{tag}.traj_wnorm"] = np.array(wn, np.float64)
    for kk, p in m.named_parameters():
        out[f"{tag}.disp.{kk}"] = (p.detach() - pre[kk]).numpy()


def main():
    ref = _ref()
    out = {}
    torch.manual_seed(0)
    m = build(ref, 64, 1, 28, 28, False)
    sd = m.state_dict()
    out["keys64"] = np.array(list(sd.keys()))
    out["shapes64"] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()])
    out["sha64"] = np.array(sd_sha(sd))
    m = build(ref, 64, 3, 32, 32, False, n_classes=10)
    sd = m.state_dict()
    out["keys64c"] = np.array(list(sd.keys()))
    out["shapes64c"] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()])
    case(ref, out, "u", 8, 4, 1, 28, 28, False, None)
    case(ref, out, "c", 8, 3, 3, 8, 8, True, 10)
    path = os.path.join(OUT, "pixelcnn_kats.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
