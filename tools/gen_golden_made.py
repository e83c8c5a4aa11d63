#!/usr/bin/env python3
"""Golden vectors for the MADE path, produced by the REFERENCE MADE (src/models/made.py).

Runs only in the build container: imports the reference with the import stubs of tools/gen_golden_vae.py and writes plain arrays
to tests/golden/made_kats.npz:
  keys / shapes / dtypes : state_dict keys in order, shapes and dtypes at the reference config (1 x 28 x 28, hidden 1024, 3 layers);
  sha                    : sha256 of that config's seeded init (torch.manual_seed(0)), every tensor's raw bytes (masks included);
  u / c                  : a tiny net (hidden 8, 2 layers) on 6 x 1 x 4 x 5 images, normalize False, and one (hidden 4, 2
                           layers) on 5 x 3 x 3 x 3 images, normalize True: the state_dict perturbed away from init (masked
                           entries included), inputs k / 255 (2k / 255 - 1), logits at 64 fixed (sample, channel, row, col)
                           positions, the bpd, every gradient, a 5-step Adam(1e-3) trajectory (per-step bpd, every tensor's
                           displacement after step 5), and the reference's own CPU bf16-autocast logits error at the same
                           positions (max abs / max |fp32 logits|): the bf16 budget.

    python tools/gen_golden_made.py
"""
import hashlib
import os
import types

import numpy as np
import torch

from gen_golden_vae import OUT, import_reference  # noqa: F401  (same stubs)


def _ref():
    import_reference()
    from src.models import made
    return made


def build(ref, hidden, n_layer, ch, H, W, normalize):
    dm = types.SimpleNamespace(width=W, height=H, channels=ch, transforms=types.SimpleNamespace(normalize=normalize))
    m = ref.MADE(dm, hidden, n_layer)
    m.hparams = types.SimpleNamespace(hidden_dim=hidden, n_layer=n_layer, lr=1e-3)
    m.input_normalize = normalize
    m.logged = {}
    return m


def sd_sha(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().contiguous().numpy().tobytes())
    return h.hexdigest()


def case(ref, out, tag, hidden, n_layer, n, ch, H, W, normalize):
    torch.manual_seed(7 + n)
    m = build(ref, hidden, n_layer, ch, H, W, normalize)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    pre = {k: v.clone() for k, v in m.state_dict().items()}
    for k, v in pre.items():
        out[f"{tag}.sd0.{k}"] = v.numpy().copy()
    k = torch.randint(0, 256, (n, ch, H, W))
    x = k.float() / 255 if not normalize else k.float() * 2 / 255 - 1
    out[f"{tag}.x"] = x.numpy()
    g = torch.Generator().manual_seed(3)
    pos = np.stack([torch.randint(0, s, (64,), generator=g).numpy() for s in (n, ch, H, W)], 1)
    out[f"{tag}.pos"] = pos
    sel = lambda t: t[pos[:, 0], :, pos[:, 1], pos[:, 2], pos[:, 3]]
    with torch.no_grad():
        logits = m.forward(x)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            lb = m.forward(x).float()
    out[f"{tag}.logits"] = sel(logits).numpy()
    out[f"{tag}.bf16_err"] = np.float32(float((sel(lb) - sel(logits)).abs().max()) / float(sel(logits).abs().max()))
    bpd = m.calc_likelihood(x)
    bpd.backward()
    out[f"{tag}.bpd"] = np.float32(bpd.item())
    for kk, p in m.named_parameters():
        out[f"{tag}.grad.{kk}"] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
    # 5 Adam steps (StepLR steps per epoch, so lr stays 1e-3)
    m.load_state_dict(pre)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    traj = []
    for _ in range(5):
        opt.zero_grad()
        b = m.calc_likelihood(x)
        b.backward()
        opt.step()
        traj.append(b.item())
    out[f"{tag}.traj_bpd"] = np.array(traj, np.float32)
    for kk, p in m.named_parameters():
        out[f"{tag}.disp.{kk}"] = (p.detach() - pre[kk]).numpy()


def main():
    ref = _ref()
    out = {}
    torch.manual_seed(0)
    m = build(ref, 1024, 3, 1, 28, 28, False)
    sd = m.state_dict()
    out["keys"] = np.array(list(sd.keys()))
    out["shapes"] = np.array([list(v.shape) + [-1] * (2 - v.dim()) for v in sd.values()])
    out["dtypes"] = np.array([str(v.dtype) for v in sd.values()])
    out["sha"] = np.array(sd_sha(sd))
    del m, sd
    case(ref, out, "u", 8, 2, 6, 1, 4, 5, False)
    case(ref, out, "c", 4, 2, 5, 3, 3, 3, True)
    path = os.path.join(OUT, "made_kats.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
