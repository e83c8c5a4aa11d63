#!/usr/bin/env python3
"""Golden vectors for the AGE path (`experiment=age/mnist`), produced by the REFERENCE AGE.training_step.

Runs only where the reference checkout is (`REF` of tools/gen_golden_vae.py): imports its src/models/age.py and src/networks/basic.py
with that tool's import stubs and writes plain arrays to tests/golden/age_kats.npz.  The reference's own training_step runs unchanged.
It is written for Lightning's automatic optimization with two optimizers of frequencies 1 and g_updates; there is no Lightning here, so
THIS TOOL DRIVES THE LOOP ITSELF, the way Lightning's loop does per batch: the optimizer is chosen by frequency (batch b is the
encoder's when b % (1 + g_updates) == 0, else the decoder's), the other net's parameters get requires_grad = False (Lightning's
toggle_optimizer), then training_step(batch, b, optimizer_idx) -> that optimizer's zero_grad() -> loss.backward() -> step().  The
prior draw is pinned: while a step runs, `torch.randn` hands out the stored draw in the model's dtype, so that the float64 run sees the
float32 numbers widened.  What each optimizer is handed is snapshotted by wrapping its `step`; what the encoder returned in each of its
calls (the code before the normalisation) is recorded by a forward hook.
  tiny  : ngf = ndf = 4, latent_dim = 6 (not a multiple of 4), 5 x 1 x 28 x 28 images, every parameter perturbed away from its init and
          rounded to bf16-representable values -- the initial state_dict `tiny.sd0.`, the images (uint8: x = u8 / 127.5 - 1), and from
          sd0 each phase alone (`tiny.<set>.E.` at batch index 0, `tiny.<set>.G.` at batch index 1) under four weight sets (SETS below):
          the draw, the logged scalars, the returned loss, the encoder's outputs call by call, the gradients handed to the stepping
          optimizer, and the state_dict after the step as its exact float32 difference `dsd1` to sd0 (or as it is: `sd1`);
  traj  : the tiny model under the shipped MNIST weights for 6 batches (E, G, G, E, G, G) at the shipped learning rates on 6 fixed
          images per batch and fixed draws, in float32 and in float64: per batch the logged scalars of both runs, and at the end the
          whole state_dict of both runs.

    python tools/gen_golden_age.py
"""
import contextlib
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_vae import OUT, import_reference as _import_vae             # noqa: E402  (same stubs)
from gen_golden_aae import decode_images, images                            # noqa: E402

ENC = {"_target_": "src.networks.basic.ConvEncoder", "norm_type": "batch"}
DEC = {"_target_": "src.networks.basic.ConvDecoder", "norm_type": "batch"}
NF, LATENT, G_UPDATES = 4, 6, 2
LRS = dict(lrE=2e-3, lrG=7e-4)                                # configs/experiment/age/mnist.yaml
SETS = {
    "mnist": dict(e_recon_x_weight=10, e_recon_z_weight=0, g_recon_x_weight=0, g_recon_z_weight=1000, norm_z=True),     # the shipped experiment
    "default": dict(e_recon_x_weight=1, e_recon_z_weight=0, g_recon_x_weight=0, g_recon_z_weight=1, norm_z=True),       # configs/model/age.yaml
    "cosine": dict(e_recon_x_weight=2, e_recon_z_weight=1000, g_recon_x_weight=10, g_recon_z_weight=3, norm_z=True),    # every term at once
    "nonorm": dict(e_recon_x_weight=10, e_recon_z_weight=5, g_recon_x_weight=0, g_recon_z_weight=100, norm_z=False),
}
E_LOGS = ("train_loss/real_kl", "train_loss/fake_kl", "train_loss/total_e_loss", "train_log/real_mu", "train_log/real_var",
          "train_log/fake_mu", "train_log/fake_var")
G_LOGS = ("train_loss/g_recon_z", "train_loss/g_loss")


def import_reference():
    _import_vae()                                              # installs the stubs and the reference's path
    from src.models import age
    return age


def build(ref, weights):
    dm = types.SimpleNamespace(width=28, height=28, channels=1, transforms=types.SimpleNamespace(normalize=True))
    kw = dict(latent_dim=LATENT, b1=0.5, b2=0.999, drop_lr_epoch=30, g_updates=G_UPDATES, **weights, **LRS)
    m = ref.AGE(dm, encoder=dict(ENC, ndf=NF), decoder=dict(DEC, ngf=NF), **kw)
    m.hparams = types.SimpleNamespace(**kw)
    m.logged = {}
    return m


def optimizers_of(m):
    cfg = m.configure_optimizers()
    assert [c["frequency"] for c in cfg] == [1, G_UPDATES]
    return [c["optimizer"] for c in cfg]


@contextlib.contextmanager
def give_draw(z, dtype=torch.float32):
    """Inside the step, `torch.randn(N, L)` returns the stored draw, exactly once."""
    inner, used = torch.randn, []

    def randn(*shape, **kw):
        assert tuple(shape) == tuple(z.shape), shape
        used.append("z")
        return z.to(dtype)
    torch.randn = randn
    try:
        yield
    finally:
        torch.randn = inner
    assert used == ["z"], used


class _Watch:
    """Records the gradients handed to each optimizer step and what the encoder returned in each call."""

    def __init__(self, m):
        self.m, self.steps, self.codes = m, [], []
        self.names = {id(p): k for k, p in m.named_parameters()}
        for opt in m._opts:
            self._wrap(opt)
        self.hook = m.encoder.register_forward_hook(
            lambda mod, args, res: self.codes.append(res.detach().double().reshape(res.shape[0], -1).numpy().copy()))

    def _wrap(self, opt):
        inner = opt.step

        def step(*a, **k):
            self.steps.append({self.names[id(p)]: p.grad.detach().clone() for g in opt.param_groups for p in g["params"] if p.grad is not None})
            return inner(*a, **k)
        opt.step = step

    def close(self):
        self.hook.remove()


def run_batch(m, batch, b, z, dtype=torch.float32):
    """What Lightning's automatic optimization does for batch b."""
    oi = 0 if b % (1 + G_UPDATES) == 0 else 1
    for p in m.encoder.parameters():
        p.requires_grad_(oi == 0)
    for p in m.decoder.parameters():
        p.requires_grad_(oi == 1)
    m.logged = {}
    with give_draw(z, dtype):
        loss = m.training_step(batch, b, oi)
    opt = m._opts[oi]
    opt.zero_grad()
    loss.backward()
    opt.step()
    return oi, float(loss)


def log_keys(oi, weights):
    if oi == 1:
        return G_LOGS
    return E_LOGS + (("train_loss/recon_x",) if weights["e_recon_x_weight"] > 0 else ())


def run_tiny_phase(ref, sd0, name, b, u8, out):
    weights = SETS[name]
    m = build(ref, weights)
    m.load_state_dict(sd0)
    m.train()
    m._opts = optimizers_of(m)
    z = torch.randn(u8.shape[0], LATENT, generator=torch.Generator().manual_seed(200 + b))
    w = _Watch(m)
    oi, total = run_batch(m, (decode_images(u8), None), b, z)
    w.close()
    tag = f"tiny.{name}.{'EG'[oi]}"
    keys = log_keys(oi, weights)
    ncalls = 2 if (oi == 0 or weights["g_recon_x_weight"] > 0) else 1
    assert set(m.logged) == set(keys) and len(w.steps) == 1 and len(w.codes) == ncalls, (m.logged, len(w.codes))
    snap = w.steps[0]
    assert snap and all(k.startswith(("encoder.", "decoder.")[oi]) for k in snap)
    rec = {"z": z.numpy(), "total": np.float64(total), "gnames": np.array(list(snap.keys()))}
    for i, cde in enumerate(w.codes):
        rec[f"code.{i}"] = cde
    for k in keys:
        rec[f"log.{k}"] = np.float64(m.logged[k])
    for k, gr in snap.items():
        rec[f"grad.{k}"] = gr.numpy().copy()
    for k, v in m.state_dict().items():                     # float tensors as the exact difference to sd0 (it compresses)
        v = v.detach().numpy()
        if v.dtype.kind == "f":
            d = v.astype(np.float64) - sd0[k].numpy().astype(np.float64)
            if np.array_equal(d.astype(np.float32).astype(np.float64), d):
                rec[f"dsd1.{k}"] = d.astype(np.float32)
                continue
        rec[f"sd1.{k}"] = v.copy()
    out.update({f"{tag}.{k}": v for k, v in rec.items()})
    print(tag, dict(m.logged), "total", total)


TRAJ_N, TRAJ_BATCHES = 6, 6


def run_traj(ref, sd0, out):
    """Starts from tiny.sd0; the float64 run sees the same float32 numbers (weights, images, draws) widened."""
    g = torch.Generator().manual_seed(78)
    u8s, imgs = zip(*[images(TRAJ_N, g, levels=16) for _ in range(TRAJ_BATCHES)])
    zs = [torch.randn(TRAJ_N, LATENT, generator=g) for _ in range(TRAJ_BATCHES)]
    out["traj.imgs_u8"] = torch.stack(u8s).numpy()
    out["traj.z"] = torch.stack(zs).numpy()
    for k, v in LRS.items():
        out[f"traj.{k}"] = np.float64(v)
    phases = []
    for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
        m = build(ref, SETS["mnist"])
        m.load_state_dict(sd0)
        m = m.to(dt).train()
        m._opts = optimizers_of(m)
        assert m._opts[0].param_groups[0]["lr"] == LRS["lrE"] and m._opts[1].param_groups[0]["lr"] == LRS["lrG"]
        for b in range(TRAJ_BATCHES):
            oi, _ = run_batch(m, (imgs[b].to(dt), None), b, zs[b], dt)
            phases.append("EG"[oi])
            assert set(m.logged) == set(log_keys(oi, SETS["mnist"]))
            for k, v in m.logged.items():
                out[f"traj.log{tag}.{b}.{k}"] = np.float64(v)
        for k, v in m.state_dict().items():
            out[f"traj.sd{tag}.{k}"] = v.detach().numpy().copy()
    assert phases[:TRAJ_BATCHES] == list("EGGEGG"), phases
    out["traj.phases"] = np.array(phases[:TRAJ_BATCHES])


def main():
    ref = import_reference()
    out = {}
    torch.manual_seed(47)
    m = build(ref, SETS["mnist"])
    assert [k.split(".")[0] for k, _ in m.named_parameters()][0] == "decoder"      # constructed first
    with torch.no_grad():
        for p in m.parameters():                            # rounded to bf16-representable values: the stored arrays compress to half
            p.copy_((p + torch.randn_like(p) * 0.03).bfloat16().float())
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for k, v in sd0.items():
        out[f"tiny.sd0.{k}"] = v.numpy().copy()
    out["tiny.names"] = np.array(list(sd0.keys()))
    out["tiny.sets"] = np.array(list(SETS))
    for name, weights in SETS.items():
        for k, v in weights.items():
            out[f"tiny.cfg.{name}.{k}"] = np.float64(v)
    out["tiny.cfg.nf"], out["tiny.cfg.latent_dim"], out["tiny.cfg.g_updates"] = np.int64(NF), np.int64(LATENT), np.int64(G_UPDATES)
    u8, _ = images(5, torch.Generator().manual_seed(5))
    out["tiny.imgs_u8"] = u8.numpy()
    for name in SETS:
        for b in (0, 1):
            run_tiny_phase(ref, sd0, name, b, u8.numpy(), out)
    run_traj(ref, sd0, out)
    path = os.path.join(OUT, "age_kats.npz")
    np.savez_compressed(path, **out)
    print("wrote age_kats.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
