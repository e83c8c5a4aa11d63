#!/usr/bin/env python3
"""Golden vectors for the cVAE path (`experiment=cvae/mnist`), produced by the REFERENCE cVAE.training_step.

Runs only where the reference checkout is (`REF` of tools/gen_golden_vae.py): imports its src/models/cvae.py and src/networks/basic.py
with that tool's import stubs and writes plain arrays to tests/golden/cvae_kats.npz.  The reparameterisation noise is not recovered but
GIVEN: `torch.distributions.normal._standard_normal`, the one draw inside `Normal.rsample()`, hands out the stored eps, so the
reference's own code runs unchanged on a known noise tensor.
  tiny : ndf = ngf = 8, latent 16, 10 classes, 6 x 1 x 28 x 28 images with labels [3, 7, 3, 0, 9, 3] (a repeated class: the segmented
         sum; absent classes: untouched rows), every tensor perturbed away from the default init -- initial state_dict, images,
         labels, eps, the loss and the three logged scalars, every parameter gradient, the batch-norm buffers after the step, an
         evaluation-mode forward(zfix, labels_fix);
  cfg  : configs/model/cvae.yaml + configs/networks/conv_mnist.yaml sizes (latent 128, ndf = ngf = 32, batch norm), 16 images whose
         labels cover all ten classes, weights = the seeded default init (torch.manual_seed(32)) -- images, labels, eps, scalars,
         parameter names, per-parameter weight / gradient statistics, buffers, the evaluation-mode decode;
  traj : the tiny model for 3 Adam steps (lr 1e-3) with StepLR stepped between them, on fixed per-step images, labels (classes
         0, 3, 7, 9 only) and eps, run twice in the reference: in float32 and with the model in float64 -- per step the loss of
         each run, after step 3 `class_embedding.weight` of both runs.

    python tools/gen_golden_cvae.py
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_vae import OUT, import_reference as _import_vae      # noqa: E402  (same stubs)

ENC = {"_target_": "src.networks.basic.ConvEncoder", "norm_type": "batch"}
DEC = {"_target_": "src.networks.basic.ConvDecoder", "norm_type": "batch"}
LOGS = ("train_log/elbo", "train_log/kl_divergence", "train_log/log_p_x_of_z")


def import_reference():
    _import_vae()                                              # installs the stubs and the reference's path
    sys.modules["omegaconf"].OmegaConf = object
    from src.models import cvae
    return cvae


class _GivenNoise:
    """Hands `Normal.rsample()` the stored eps (in the distribution's dtype)."""

    def __init__(self):
        self.eps = None
        import torch.distributions.normal as N
        self._mod, self._orig = N, N._standard_normal
        N._standard_normal = self

    def __call__(self, shape, dtype, device):
        assert tuple(shape) == tuple(self.eps.shape), (shape, self.eps.shape)
        return self.eps.to(dtype=dtype, device=device)


def build(ref, ndf, latent, ncls, lr=1e-4):
    dm = types.SimpleNamespace(width=28, height=28, channels=1, transforms=types.SimpleNamespace(normalize=True))
    m = ref.cVAE(dm, encoder=dict(ENC, ndf=ndf), decoder=dict(DEC, ngf=ndf), latent_dim=latent, decoder_dist="gaussian", n_classes=ncls)
    m.hparams = types.SimpleNamespace(latent_dim=latent, beta=1.0, recon_weight=1.0, lr=lr, b1=0.9, b2=0.999, encode_label=True)
    m.logged = {}
    return m


def run_case(ref, noise, tag, ndf, latent, labels, seed, out, full):
    torch.manual_seed(seed)
    n, ncls = len(labels), 10
    m = build(ref, ndf, latent, ncls)
    if full:                                                # tiny case: every tensor away from the default init, stored
        with torch.no_grad():
            for p in m.parameters():
                p.add_(torch.randn_like(p) * 0.03)
        for k, v in m.state_dict().items():
            out[f"{tag}.sd0.{k}"] = v.detach().numpy().copy()
    m.train()
    imgs = torch.rand(n, 1, 28, 28) * 2 - 1
    labels = torch.tensor(labels, dtype=torch.int64)
    noise.eps = torch.randn(n, latent)
    out[f"{tag}.imgs"], out[f"{tag}.labels"], out[f"{tag}.eps"] = imgs.numpy(), labels.numpy(), noise.eps.numpy()
    loss = m.training_step((imgs, labels), 0)
    loss.backward()
    out[f"{tag}.loss"] = np.float64(loss.item())
    for k in LOGS:
        out[f"{tag}.log.{k}"] = np.float64(m.logged[k])
    out[f"{tag}.names"] = np.array(list(m.state_dict().keys()))
    out[f"{tag}.pnames"] = np.array([k for k, _ in m.named_parameters()])
    out[f"{tag}.wstats"] = np.array([[float(p.detach().double().sum()), float(p.detach().double().abs().sum())] for _, p in m.named_parameters()])
    out[f"{tag}.gstats"] = np.array([[float(p.grad.double().sum()), float(p.grad.double().norm())] for _, p in m.named_parameters()])
    if full:
        for k, p in m.named_parameters():
            out[f"{tag}.grad.{k}"] = p.grad.numpy().copy()
    for k, v in m.state_dict().items():
        if "running_" in k or "num_batches" in k:
            out[f"{tag}.buf1.{k}"] = v.detach().numpy().copy()
    m.eval()
    zfix, lfix = torch.randn(5, latent), torch.tensor([9, 0, 4, 4, 7], dtype=torch.int64)
    out[f"{tag}.zfix"], out[f"{tag}.labels_fix"] = zfix.numpy(), lfix.numpy()
    with torch.no_grad():
        out[f"{tag}.decode_eval"] = m(zfix, lfix).numpy()
    print(tag, dict(m.logged), "loss", float(loss))


TRAJ_LABELS = ([3, 7, 3, 0, 9, 3], [0, 0, 9, 7, 3, 9], [7, 3, 0, 9, 9, 0])
TRAJ_LR = 1e-3


def run_traj(ref, noise, out):
    """Starts from tiny.sd0; the float64 run sees the same float32 numbers (weights, images, eps) widened."""
    sd0 = {k[len("tiny.sd0."):]: torch.from_numpy(v) for k, v in out.items() if k.startswith("tiny.sd0.")}
    g = torch.Generator().manual_seed(77)
    imgs = [torch.rand(6, 1, 28, 28, generator=g) * 2 - 1 for _ in TRAJ_LABELS]
    eps = [torch.randn(6, 16, generator=g) for _ in TRAJ_LABELS]
    out["traj.imgs"], out["traj.eps"] = torch.stack(imgs).numpy(), torch.stack(eps).numpy()
    out["traj.labels"], out["traj.lr"] = np.array(TRAJ_LABELS, dtype=np.int64), np.float64(TRAJ_LR)
    res = {}
    for dt in (torch.float32, torch.float64):
        m = build(ref, 8, 16, 10, lr=TRAJ_LR)
        m.load_state_dict(sd0)
        m = m.to(dt).train()
        (opt,), (sch,) = m.configure_optimizers()
        losses = []
        for x, e, lab in zip(imgs, eps, TRAJ_LABELS):
            noise.eps = e
            opt.zero_grad()
            loss = m.training_step((x.to(dt), torch.tensor(lab, dtype=torch.int64)), 0)
            loss.backward()
            opt.step()
            sch.step()
            losses.append(float(loss.item()))
        res[dt] = (np.array(losses, dtype=np.float64), m.class_embedding.weight.detach().double().numpy().copy())
    out["traj.loss32"], out["traj.emb32"] = res[torch.float32]
    out["traj.loss64"], out["traj.emb64"] = res[torch.float64]
    dev = np.abs(out["traj.loss32"] - out["traj.loss64"]) / np.abs(out["traj.loss64"])
    print("traj loss64", out["traj.loss64"], "float32 run's relative deviation per step", dev)
    print("traj class_embedding.weight: float32 run's max abs deviation from float64", np.abs(out["traj.emb32"] - out["traj.emb64"]).max())


def main():
    ref = import_reference()
    noise = _GivenNoise()
    out = {}
    run_case(ref, noise, "tiny", 8, 16, [3, 7, 3, 0, 9, 3], 31, out, True)                                  # everything stored
    run_case(ref, noise, "cfg", 32, 128, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 3, 3, 7, 0, 9, 5], 32, out, False)  # cvae.yaml + conv_mnist.yaml sizes
    run_traj(ref, noise, out)
    path = os.path.join(OUT, "cvae_kats.npz")
    np.savez_compressed(path, **out)
    print("wrote cvae_kats.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
