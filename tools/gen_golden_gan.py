#!/usr/bin/env python3
"""Golden vectors for the GAN path (`experiment=vanilla_gan/mnist_conv`, `lsgan/conv_mnist`, `ggan/mnist_conv`), produced by the
REFERENCE GAN.training_step.

Runs only where the reference checkout is (`REF` of tools/gen_golden_vae.py): imports its src/models/gan.py and src/networks/basic.py
with that tool's import stubs and writes plain arrays to tests/golden/gan_kats.npz.  The reference's own code runs unchanged on known
draws: while a step runs, `torch.randn` hands out the stored z, and the module's `device` is its dtype, so that the reference's
`.to(self.device)` widens z for the float64 run.  The manual-optimization hooks the step uses are stubs (`optimizers()` returns the two
optimizers of `configure_optimizers`, `manual_backward` is a plain `loss.backward()`, `toggle_optimizer` / `untoggle_optimizer` accept
anything -- the reference hands the latter a loss tensor in its discriminator phase --, `log()` records).  What the step hands its
optimizer is snapshotted by wrapping `step`: the stepped parameters' `.grad` at that moment.
  tiny : ndf = ngf = 4, latent 8, 5 x 1 x 28 x 28 images, every parameter perturbed away from its init (and rounded to
         bf16-representable values) -- the initial state_dict `tiny.sd0.`, images (uint8: x = u8 / 127.5 - 1), and for each loss mode
         (vanilla, lsgan, hinge) one generator step (`.g.`, batch_idx 0) and one discriminator step (`.d.`, batch_idx 1), each from
         sd0: z, the logged scalars, max|logit| per discriminator call, the gradients handed to the optimizer, and the state_dict after
         the step as its exact float32 difference `dsd1` to sd0 (integer buffers, and the few tensors whose difference is not a
         float32, as they are: `sd1`);
  traj : the tiny model for 4 steps (G, D, G, D) in vanilla mode at the shipped learning rates on 6 fixed images per step (16 grey
         levels) and fixed z, run twice in the reference: in float32 and with the model in float64 -- per step the logged scalars and
         the gradients handed to the optimizer (float64 run), after every step the conv biases that sit in front of a BatchNorm, and
         after step 4 the whole state_dict of both runs.

    python tools/gen_golden_gan.py
"""
import contextlib
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_vae import OUT, import_reference as _import_vae      # noqa: E402  (same stubs)
from gen_golden_aae import decode_images, images                     # noqa: E402

NETD = {"_target_": "src.networks.basic.ConvEncoder", "norm_type": "batch"}
NETG = {"_target_": "src.networks.basic.ConvDecoder", "norm_type": "batch"}
G_LOGS = ("train_loss/g_loss",)
D_LOGS = ("train_loss/d_loss", "train_log/pred_real", "train_log/pred_fake")
MODES = ("vanilla", "lsgan", "hinge")
LATENT = 8
# conv biases in front of a BatchNorm layer: zero analytic gradient, a random walk under Adam (docs/kernels.md 4i)
BIASES = ("netG.network.0.bias", "netG.network.3.bias", "netG.network.6.bias", "netD.network.2.bias", "netD.network.5.bias")


def import_reference():
    _import_vae()                                              # installs the stubs and the reference's path
    from src.models import gan
    gan.GAN.optimizers = lambda self: self._opts
    gan.GAN.manual_backward = lambda self, loss: loss.backward()
    gan.GAN.toggle_optimizer = lambda self, *a, **k: None
    gan.GAN.untoggle_optimizer = lambda self, *a, **k: None    # called with a loss tensor in the discriminator phase
    gan.GAN.device = property(lambda self: next(self.parameters()).dtype)      # z.to(self.device): the model's dtype
    return gan


def build(ref, nf, loss_mode="vanilla", lrG=2e-4, lrD=2e-4):
    dm = types.SimpleNamespace(width=28, height=28, channels=1, transforms=types.SimpleNamespace(normalize=True))
    m = ref.GAN(dm, netG=dict(NETG, ngf=nf), netD=dict(NETD, ndf=nf), latent_dim=LATENT, loss_mode=loss_mode)
    m.hparams = types.SimpleNamespace(latent_dim=LATENT, loss_mode=loss_mode, lrG=lrG, lrD=lrD, b1=0.5, b2=0.999)
    m.logged = {}
    return m


@contextlib.contextmanager
def give_z(z):
    """`torch.randn(N, latent_dim)` inside the step returns the stored draw."""
    inner = torch.randn

    def randn(*shape, **kw):
        assert tuple(shape) == tuple(z.shape), shape
        return z.clone()
    torch.randn = randn
    try:
        yield
    finally:
        torch.randn = inner


class _Watch:
    """Records the gradients handed to each optimizer step and what the discriminator returned in each call."""

    def __init__(self, m):
        self.m, self.steps, self.calls = m, [], []
        self.names = {id(p): k for k, p in m.named_parameters()}
        for opt in m._opts:
            self._wrap(opt)
        self.hook = m.netD.register_forward_hook(lambda mod, args, res: self.calls.append(res.detach().double().numpy().copy()))

    def _wrap(self, opt):
        inner = opt.step

        def step(*a, **k):
            self.steps.append({self.names[id(p)]: p.grad.detach().clone() for g in opt.param_groups for p in g["params"] if p.grad is not None})
            return inner(*a, **k)
        opt.step = step

    def close(self):
        self.hook.remove()


def run_step(ref, sd0, mode, phase, u8, out):
    tag = f"tiny.{mode}.{phase}"
    m = build(ref, 4, mode)
    m.load_state_dict(sd0)
    m.train()
    m._opts = m.configure_optimizers()
    z = torch.randn(u8.shape[0], LATENT)
    out[f"{tag}.z"] = z.numpy()
    w = _Watch(m)
    with give_z(z):
        m.training_step((decode_images(u8), None), 0 if phase == "g" else 1)
    w.close()
    keys = G_LOGS if phase == "g" else D_LOGS
    assert set(m.logged) == set(keys) and len(w.steps) == 1 and len(w.calls) == (1 if phase == "g" else 2)
    for k in keys:
        out[f"{tag}.log.{k}"] = np.float64(m.logged[k])
    out[f"{tag}.max_logit"] = np.array([np.abs(o).max() for o in w.calls])
    snap = w.steps[0]
    assert all(k.startswith("netG." if phase == "g" else "netD.") for k in snap)
    out[f"{tag}.gnames"] = np.array(list(snap.keys()))
    for k, g in snap.items():
        out[f"{tag}.grad.{k}"] = g.numpy().copy()
    for k, v in m.state_dict().items():                     # float tensors as the exact difference to sd0 (it compresses)
        v = v.detach().numpy()
        if v.dtype.kind == "f":
            d = v.astype(np.float64) - sd0[k].numpy().astype(np.float64)
            if np.array_equal(d.astype(np.float32).astype(np.float64), d):
                out[f"{tag}.dsd1.{k}"] = d.astype(np.float32)
                continue
        out[f"{tag}.sd1.{k}"] = v.copy()
    for k, v in m.state_dict().items():
        if k.endswith("num_batches_tracked"):
            want = 1 if phase == "g" else (2 if k.startswith("netD.") else 1)
            assert int(v) == want, (k, int(v))
    print(tag, dict(m.logged), "max|logit|", out[f"{tag}.max_logit"])


TRAJ_N, TRAJ_STEPS = 6, 4


def run_traj(ref, sd0, out):
    """Starts from tiny.sd0; the float64 run sees the same float32 numbers (weights, images, z) widened."""
    g = torch.Generator().manual_seed(77)
    u8s, imgs = zip(*[images(TRAJ_N, g, levels=16) for _ in range(TRAJ_STEPS)])
    zs = [torch.randn(TRAJ_N, LATENT, generator=g) for _ in range(TRAJ_STEPS)]
    out["traj.imgs_u8"] = torch.stack(u8s).numpy()
    out["traj.z"] = torch.stack(zs).numpy()
    out["traj.lrG"], out["traj.lrD"] = np.float64(2e-4), np.float64(2e-4)
    out["traj.biases"] = np.array(BIASES)
    for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
        m = build(ref, 4)
        m.load_state_dict(sd0)
        m = m.to(dt).train()
        m._opts = m.configure_optimizers()
        w = _Watch(m)
        for i, (x, z) in enumerate(zip(imgs, zs)):
            m.logged = {}
            with give_z(z):
                m.training_step((x.to(dt), None), i)
            for k, v in m.logged.items():
                out[f"traj.log{tag}.{i}.{k}"] = np.float64(v)
            sd = m.state_dict()
            for b in BIASES:
                out[f"traj.bias{tag}.{i}.{b}"] = sd[b].detach().double().numpy().copy()
        w.close()
        assert len(w.steps) == TRAJ_STEPS and len(w.calls) == 6
        if dt == torch.float64:
            for i, snap in enumerate(w.steps):
                for k, gr in snap.items():
                    out[f"traj.grad64.{i}.{k}"] = gr.double().numpy().copy()
            out["traj.max_logit64"] = np.array([np.abs(o).max() for o in w.calls])
        for k, v in m.state_dict().items():
            out[f"traj.sd{tag}.{k}"] = v.detach().numpy().copy()
    worst = {}
    for k in sd0:
        a, b = out[f"traj.sd32.{k}"].astype(np.float64), out[f"traj.sd64.{k}"].astype(np.float64)
        worst[k] = float(np.abs(a - b).max())
    print("float32 run's max abs deviation from float64 after 4 steps:", {k: f"{v:.2e}" for k, v in worst.items() if "running" in k})


def main():
    ref = import_reference()
    out = {}
    torch.manual_seed(41)
    m = build(ref, 4)
    with torch.no_grad():
        for p in m.parameters():                            # rounded to bf16-representable values: the stored arrays compress to half
            p.copy_((p + torch.randn_like(p) * 0.03).bfloat16().float())
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for k, v in sd0.items():
        out[f"tiny.sd0.{k}"] = v.numpy().copy()
    out["tiny.names"] = np.array(list(sd0.keys()))
    out["tiny.pnames"] = np.array([k for k, _ in m.named_parameters()])
    u8, _ = images(5)
    out["tiny.imgs_u8"] = u8.numpy()
    for mode in MODES:
        for phase in ("g", "d"):
            run_step(ref, sd0, mode, phase, u8.numpy(), out)
    run_traj(ref, sd0, out)
    path = os.path.join(OUT, "gan_kats.npz")
    np.savez_compressed(path, **out)
    print("wrote gan_kats.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
