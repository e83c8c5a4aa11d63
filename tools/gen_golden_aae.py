#!/usr/bin/env python3
"""Golden vectors for the AAE path (`experiment=aae/mnist`), produced by the REFERENCE AAE.training_step.

Runs only where the reference checkout is (`REF` of tools/gen_golden_vae.py): imports its src/models/aae.py and src/networks/basic.py
with that tool's import stubs and writes plain arrays to tests/golden/aae_kats.npz.  The reference's own code runs unchanged on known
draws: `sample_prior` hands out the stored prior.  The manual-optimization hooks the step uses are stubs (`optimizers()` returns the two
optimizers of `configure_optimizers`, `manual_backward` is a plain `loss.backward()`, `log()` records).
What the step hands its optimizers is snapshotted by wrapping their `step`: the stepped parameters' `.grad` at the moment of each of
the three optimizer steps.  (`.grad` at the end of the step is no usable pin: by then the decoder's is None and the discriminator's
holds the discriminator phase plus the generator phase.)  A forward hook records what `discriminator` read and returned in each of its
three calls.
  tiny : ndf = ngf = 4, latent 8, 6 x 1 x 28 x 28 images, recon_weight 1.5, every parameter perturbed away from its init (and rounded
         to bf16-representable values) -- initial state_dict, images (uint8: x = u8 / 127.5 - 1), prior, the five logged scalars, the
         discriminator's three inputs and outputs and max|logit| per call, the three gradient snapshots (`grad1.` encoder + decoder,
         `grad2.` discriminator, `grad3.` encoder), the state_dict after the step as its exact float32 difference `dsd1` to the
         initial one (integer buffers, and the few tensors whose difference is not a float32, as they are: `sd1`), the Adam step
         count per parameter;
  cfg  : configs/experiment/aae/mnist.yaml sizes (ndf = ngf = 32, latent 8), 8 images, weights = the seeded default init
         (torch.manual_seed(32)) -- images, prior, scalars, names, per-parameter weight statistics and gradient statistics per snapshot;
  traj : the tiny model for 3 steps at the shipped learning rates on 16 fixed images per step (16 grey levels) and fixed priors, run
         twice in the reference: in float32 and with the model in float64 -- per step the five scalars of each run, after step 3
         `discriminator.classifier.fc.weight` and `encoder.network.0.weight` of both runs, max|logit| per discriminator pass of the
         float64 run.

    python tools/gen_golden_aae.py
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
LOGS = ("train_loss/recon_loss", "train_loss/d_loss", "train_log/real_logit", "train_log/fake_logit", "train_loss/adv_encoder_loss")
LATENT = 8


def import_reference():
    _import_vae()                                              # installs the stubs and the reference's path
    from src.models import aae
    aae.AAE.optimizers = lambda self: self._opts
    aae.AAE.manual_backward = lambda self, loss: loss.backward()
    return aae


def build(ref, nf, lrG=2e-4, lrD=2e-4, recon_weight=1.0):
    dm = types.SimpleNamespace(width=28, height=28, channels=1, transforms=types.SimpleNamespace(normalize=True))
    m = ref.AAE(dm, encoder=dict(ENC, ndf=nf), decoder=dict(DEC, ngf=nf), netD=None, latent_dim=LATENT)
    m.hparams = types.SimpleNamespace(latent_dim=LATENT, loss_mode="vanilla", lrG=lrG, lrD=lrD, b1=0.5, b2=0.999, recon_weight=recon_weight,
                                      prior="normal")
    m.logged = {}
    return m


def give_prior(m, prior):
    """`sample_prior` hands out the stored draw, in the model's dtype."""
    m.sample_prior = lambda N: prior.to(next(m.parameters()).dtype).clone()


def images(n, gen=None, levels=256):
    """Random 8-bit images: stored as uint8, used as u8 / 127.5 - 1 in float32.  levels=16: 16 grey levels (multiples of 17)."""
    u8 = (torch.randint(0, levels, (n, 1, 28, 28), generator=gen, dtype=torch.int64) * (255 // (levels - 1))).to(torch.uint8)
    return u8, decode_images(u8.numpy())


def decode_images(u8):
    return torch.from_numpy(u8.astype(np.float32) / np.float32(127.5) - np.float32(1))


class _Watch:
    """Records the gradients handed to each optimizer step and what the discriminator read and returned in each call."""

    def __init__(self, m):
        self.m, self.steps, self.calls = m, [], []
        self.names = {id(p): k for k, p in m.named_parameters()}
        for opt in m._opts:
            self._wrap(opt)
        self.hook = m.discriminator.register_forward_hook(
            lambda mod, args, res: self.calls.append((args[0].detach().double().numpy().copy(), res.detach().double().numpy().copy())))

    def _wrap(self, opt):
        inner = opt.step

        def step(*a, **k):
            self.steps.append({self.names[id(p)]: p.grad.detach().clone() for g in opt.param_groups for p in g["params"] if p.grad is not None})
            return inner(*a, **k)
        opt.step = step

    def close(self):
        self.hook.remove()


def run_case(ref, tag, nf, n, seed, out, full, recon_weight):
    torch.manual_seed(seed)
    m = build(ref, nf, recon_weight=recon_weight)
    if full:                                                # tiny case: every parameter away from the default init, stored
        with torch.no_grad():
            for p in m.parameters():                        # rounded to bf16-representable values: the stored arrays compress to half
                p.copy_((p + torch.randn_like(p) * 0.03).bfloat16().float())
        for k, v in m.state_dict().items():
            out[f"{tag}.sd0.{k}"] = v.detach().numpy().copy()
    out[f"{tag}.names"] = np.array(list(m.state_dict().keys()))
    out[f"{tag}.pnames"] = np.array([k for k, _ in m.named_parameters()])
    out[f"{tag}.wstats"] = np.array([[float(p.detach().double().sum()), float(p.detach().double().abs().sum())] for _, p in m.named_parameters()])
    m.train()
    m._opts = m.configure_optimizers()
    u8, imgs = images(n)
    prior = torch.randn(n, LATENT)
    give_prior(m, prior)
    out[f"{tag}.imgs_u8"], out[f"{tag}.prior"], out[f"{tag}.recon_weight"] = u8.numpy(), prior.numpy(), np.float64(recon_weight)
    w = _Watch(m)
    m.training_step((imgs, None), 0, None)
    w.close()
    assert len(w.steps) == 3 and len(w.calls) == 3
    for k in LOGS:
        out[f"{tag}.log.{k}"] = np.float64(m.logged[k])
    out[f"{tag}.max_logit"] = np.array([np.abs(o).max() for _, o in w.calls])
    for i, snap in enumerate(w.steps, 1):
        out[f"{tag}.gnames{i}"] = np.array(list(snap.keys()))
        out[f"{tag}.gstats{i}"] = np.array([[float(g.double().sum()), float(g.double().norm())] for g in snap.values()])
    assert all(k.startswith(("encoder.", "decoder.")) for k in w.steps[0]) and all(k.startswith("discriminator.") for k in w.steps[1])
    assert all(k.startswith("encoder.") for k in w.steps[2])          # the decoder's .grad is None in the generator phase
    if full:
        for i, (x, o) in enumerate(w.calls, 1):
            out[f"{tag}.disc_in{i}"], out[f"{tag}.disc_out{i}"] = x.astype(np.float32), o.astype(np.float32)
        for i, snap in enumerate(w.steps, 1):
            for k, g in snap.items():
                out[f"{tag}.grad{i}.{k}"] = g.numpy().copy()
        for k, v in m.state_dict().items():                 # float tensors as the exact difference to sd0 (it compresses)
            v = v.detach().numpy()
            if v.dtype.kind == "f":
                d = v.astype(np.float64) - out[f"{tag}.sd0.{k}"].astype(np.float64)
                if np.array_equal(d.astype(np.float32).astype(np.float64), d):
                    out[f"{tag}.dsd1.{k}"] = d.astype(np.float32)
                else:                                       # an element crossed zero: its difference needs more than 24 bits
                    out[f"{tag}.sd1.{k}"] = v.copy()
            else:
                out[f"{tag}.sd1.{k}"] = v.copy()
        state = m._opts[0].state
        out[f"{tag}.adam_steps"] = np.array([int(state[p]["step"]) for _, p in m.named_parameters() if p in state])
        out[f"{tag}.adam_names"] = np.array([k for k, p in m.named_parameters() if p in state])
    for k, v in m.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == (3 if k.startswith("encoder.") else 1), (k, int(v))
    print(tag, dict(m.logged), "max|logit|", out[f"{tag}.max_logit"])


TRAJ_N = 16


def run_traj(ref, out):
    """Starts from tiny.sd0; the float64 run sees the same float32 numbers (weights, images, priors) widened."""
    sd0 = {k[len("tiny.sd0."):]: torch.from_numpy(v) for k, v in out.items() if k.startswith("tiny.sd0.")}
    g = torch.Generator().manual_seed(77)
    u8s, imgs = zip(*[images(TRAJ_N, g, levels=16) for _ in range(3)])
    priors = [torch.randn(TRAJ_N, LATENT, generator=g) for _ in range(3)]
    out["traj.imgs_u8"] = torch.stack(u8s).numpy()
    out["traj.prior"] = torch.stack(priors).numpy()
    out["traj.lrG"], out["traj.lrD"] = np.float64(2e-4), np.float64(2e-4)
    res = {}
    for dt in (torch.float32, torch.float64):
        m = build(ref, 4)
        m.load_state_dict(sd0)
        m = m.to(dt).train()
        m._opts = m.configure_optimizers()
        w = _Watch(m)
        logs = []
        for x, pr in zip(imgs, priors):
            give_prior(m, pr)
            m.training_step((x.to(dt), None), 0, None)
            logs.append([m.logged[k] for k in LOGS])
        w.close()
        res[dt] = (np.array(logs, dtype=np.float64), m.discriminator.classifier.fc.weight.detach().double().numpy().copy(),
                   m.encoder.network[0].weight.detach().double().numpy().copy(),
                   np.array([np.abs(o).max() for _, o in w.calls]).reshape(3, 3))
    out["traj.logs32"], out["traj.dw32"], out["traj.ew32"], _ = res[torch.float32]
    out["traj.logs64"], out["traj.dw64"], out["traj.ew64"], out["traj.max_logit64"] = res[torch.float64]
    out["traj.log_keys"] = np.array(LOGS)
    print("traj logs64", out["traj.logs64"])
    print("float32 run's relative deviation per step and scalar", np.abs(out["traj.logs32"] - out["traj.logs64"]) / np.abs(out["traj.logs64"]))
    print("discriminator.classifier.fc.weight / encoder.network.0.weight: float32 run's max abs deviation from float64",
          np.abs(out["traj.dw32"] - out["traj.dw64"]).max(), np.abs(out["traj.ew32"] - out["traj.ew64"]).max())


def main():
    ref = import_reference()
    out = {}
    run_case(ref, "tiny", 4, 6, 31, out, True, 1.5)          # everything stored
    run_case(ref, "cfg", 32, 8, 32, out, False, 1.0)         # aae/mnist.yaml sizes, seeded default init
    run_traj(ref, out)
    path = os.path.join(OUT, "aae_kats.npz")
    np.savez_compressed(path, **out)
    print("wrote aae_kats.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
