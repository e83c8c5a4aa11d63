#!/usr/bin/env python3
"""Golden vectors for the weight-clipped WGAN path (`experiment=wgan/mnist_conv`), produced by the REFERENCE WGAN.training_step.

(tools/gen_golden_wgan.py and tests/golden/wgan_kats.npz are the WGAN-GP's; this tool writes tests/golden/wgan_clip_kats.npz.)

Runs only where the reference checkout is (`REF` of tools/gen_golden_vae.py): imports its src/models/wgan.py and src/networks/basic.py
with that tool's import stubs and writes plain arrays.  The reference's own code runs unchanged on known draws: while a step runs,
`torch.randn` hands out the stored z (the step widens it itself with `type_as`).  `optimizers()` returns the two optimizers of
`configure_optimizers`, `manual_backward` is a plain `loss.backward()`, `log()` records.  What the step hands its optimizer is
snapshotted by wrapping `step`: the stepped parameters' `.grad` at that moment.
  tiny : ndf = ngf = 4, latent 8, 5 x 1 x 28 x 28 images, clip_weight 0.1, lr 6e-4, every parameter perturbed away from its init (and
         rounded to bf16-representable values) so that the first clip moves critic elements in both directions and leaves others
         alone, in every BatchNorm weight of the critic too -- the initial state_dict `tiny.sd0.`, images (uint8: x = u8 / 127.5 - 1),
         one generator step (`.g.`, batch_idx 0) and one critic step (`.d.`, batch_idx 1), each from sd0: z, the logged scalars,
         max|logit| per critic call, the gradients handed to the optimizer, the optimizer's square_avg after the step (`sq`), and the
         state_dict after the step as its exact float32 difference `dsd1` to sd0 (integer buffers, and the tensors whose difference
         is not a float32, as they are: `sd1`);
  traj : the tiny model with n_critic = 2 for 7 steps (G D D G D D G) at the same learning rate on 6 fixed images per step (16 grey
         levels) and fixed z, run twice in the reference: in float32 and with the model in float64 -- per step the logged scalars,
         the gradients handed to the optimizer (float64 run; `dgrad`: per tensor, how far the float32 run's gradient is from it), the
         conv biases that sit in front of a BatchNorm, and after step 7 the whole state_dict of both runs and both optimizers'
         square_avg (float64 run).

    python tools/gen_golden_wgan_clip.py
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_vae import OUT, import_reference as _import_vae      # noqa: E402  (same stubs)
from gen_golden_aae import decode_images, images                     # noqa: E402
from gen_golden_gan import give_z                                    # noqa: E402

NETD = {"_target_": "src.networks.basic.ConvEncoder", "norm_type": "batch"}
NETG = {"_target_": "src.networks.basic.ConvDecoder", "norm_type": "batch"}
G_LOGS = ("train_loss/g_loss",)
D_LOGS = ("train_loss/d_loss", "train_log/real_logit", "train_log/fake_logit")
LATENT, CLIP, LR, ALPHA = 8, 0.1, 6e-4, 0.99
# conv biases in front of a BatchNorm layer: zero analytic gradient; RMSprop turns the rounding noise into steps of up to lr / sqrt(1 - alpha)
BIASES = ("generator.network.0.bias", "generator.network.3.bias", "generator.network.6.bias", "discriminator.network.2.bias",
          "discriminator.network.5.bias")
D_NORM_WEIGHTS = ("discriminator.network.3.weight", "discriminator.network.6.weight")


def import_reference():
    _import_vae()                                              # installs the stubs and the reference's path
    from src.models import wgan
    wgan.WGAN.optimizers = lambda self: self._opts
    wgan.WGAN.manual_backward = lambda self, loss: loss.backward()
    return wgan


def build(ref, nf, n_critic=5):
    dm = types.SimpleNamespace(width=28, height=28, channels=1, transforms=types.SimpleNamespace(normalize=True))
    m = ref.WGAN(dm, netG=dict(NETG, ngf=nf), netD=dict(NETD, ndf=nf), latent_dim=LATENT)
    m.hparams = types.SimpleNamespace(latent_dim=LATENT, n_critic=n_critic, clip_weight=CLIP, lrG=LR, lrD=LR, alpha=ALPHA, eval_fid=False)
    m.logged = {}
    return m


class _Watch:
    """Records the gradients handed to each optimizer step and what the critic returned in each call."""

    def __init__(self, m):
        self.m, self.steps, self.calls = m, [], []
        self.names = {id(p): k for k, p in m.named_parameters()}
        for opt in m._opts:
            self._wrap(opt)
        self.hook = m.discriminator.register_forward_hook(lambda mod, args, res: self.calls.append(res.detach().double().numpy().copy()))

    def _wrap(self, opt):
        inner = opt.step

        def step(*a, **k):
            self.steps.append({self.names[id(p)]: p.grad.detach().clone() for g in opt.param_groups for p in g["params"] if p.grad is not None})
            return inner(*a, **k)
        opt.step = step

    def square_avg(self, opt):
        return {self.names[id(p)]: opt.state[p]["square_avg"].detach().clone() for g in opt.param_groups for p in g["params"] if p in opt.state}

    def close(self):
        self.hook.remove()


def run_step(ref, sd0, phase, u8, out):
    tag = f"tiny.{phase}"
    m = build(ref, 4)
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
    stepped = "generator." if phase == "g" else "discriminator."
    assert all(k.startswith(stepped) for k in snap)
    out[f"{tag}.gnames"] = np.array(list(snap.keys()))
    for k, g in snap.items():
        out[f"{tag}.grad.{k}"] = g.numpy().copy()
    sq_g, sq_d = (w.square_avg(o) for o in m._opts)
    assert (len(sq_d) == 0) if phase == "g" else (len(sq_g) == 0)                # the other optimizer has no state yet
    for k, v in (sq_g if phase == "g" else sq_d).items():
        out[f"{tag}.sq.{k}"] = v.numpy().copy()
    sd1 = m.state_dict()
    for k, v in sd1.items():                                # float tensors as the exact difference to sd0 (it compresses)
        v = v.detach().numpy()
        if v.dtype.kind == "f":
            d = v.astype(np.float64) - sd0[k].numpy().astype(np.float64)
            if np.array_equal(d.astype(np.float32).astype(np.float64), d):
                out[f"{tag}.dsd1.{k}"] = d.astype(np.float32)
                continue
        out[f"{tag}.sd1.{k}"] = v.copy()
    pnames = [k for k, _ in m.named_parameters()]
    for k in pnames:                                        # where the clip leaves the state: clipped after a generator step only
        if k.startswith("discriminator.") and phase == "g":
            assert torch.equal(sd1[k], sd0[k].clamp(-CLIP, CLIP)), k
    if phase == "d":
        assert any(float(sd1[k].abs().max()) > CLIP for k in pnames if k.startswith("discriminator.")), "the update leaves the range somewhere"
    for k, v in sd1.items():
        if k.endswith("num_batches_tracked"):
            want = 1 if phase == "g" else (2 if k.startswith("discriminator.") else 1)
            assert int(v) == want, (k, int(v))
    print(tag, dict(m.logged), "max|logit|", out[f"{tag}.max_logit"])


TRAJ_N, TRAJ_STEPS, TRAJ_NCRITIC = 6, 7, 2


def run_traj(ref, sd0, out):
    """Starts from tiny.sd0; the float64 run sees the same float32 numbers (weights, images, z) widened."""
    g = torch.Generator().manual_seed(78)
    u8s, imgs = zip(*[images(TRAJ_N, g, levels=16) for _ in range(TRAJ_STEPS)])
    zs = [torch.randn(TRAJ_N, LATENT, generator=g) for _ in range(TRAJ_STEPS)]
    out["traj.imgs_u8"] = torch.stack(u8s).numpy()
    out["traj.z"] = torch.stack(zs).numpy()
    out["traj.lr"], out["traj.alpha"], out["traj.clip_weight"] = np.float64(LR), np.float64(ALPHA), np.float64(CLIP)
    out["traj.n_critic"] = np.int64(TRAJ_NCRITIC)
    out["traj.biases"] = np.array(BIASES)
    for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
        m = build(ref, 4, n_critic=TRAJ_NCRITIC)
        m.load_state_dict(sd0)
        m = m.to(dt).train()
        m._opts = m.configure_optimizers()
        w = _Watch(m)
        reclipped = 0
        for i, (x, z) in enumerate(zip(imgs, zs)):
            m.logged = {}
            if i > 0 and (i - 1) % (TRAJ_NCRITIC + 1) != 0:       # the step before was a critic update: what this step's clip finds
                reclipped += sum(int((p.detach().abs() > CLIP).sum()) for p in m.discriminator.parameters())
            with give_z(z):
                m.training_step((x.to(dt), None), i)
            assert set(m.logged) == set(G_LOGS if i % (TRAJ_NCRITIC + 1) == 0 else D_LOGS), (i, m.logged)
            for k, v in m.logged.items():
                out[f"traj.log{tag}.{i}.{k}"] = np.float64(v)
            sd = m.state_dict()
            for b in BIASES:
                out[f"traj.bias{tag}.{i}.{b}"] = sd[b].detach().double().numpy().copy()
        w.close()
        assert reclipped >= 1, "no critic element is re-clipped after a critic update"
        assert len(w.steps) == TRAJ_STEPS and len(w.calls) == 3 * 1 + 4 * 2
        if dt == torch.float32:
            steps32 = w.steps
        else:
            for i, snap in enumerate(w.steps):
                for k, gr in snap.items():
                    out[f"traj.grad64.{i}.{k}"] = gr.double().numpy().copy()
                    out[f"traj.dgrad.{i}.{k}"] = np.float64((steps32[i][k].double() - gr.double()).abs().max())
            out["traj.max_logit64"] = np.array([np.abs(o).max() for o in w.calls])
            for opt in m._opts:
                for k, v in w.square_avg(opt).items():
                    out[f"traj.sq64.{k}"] = v.double().numpy().copy()
        for k, v in m.state_dict().items():
            out[f"traj.sd{tag}.{k}"] = v.detach().numpy().copy()
        print(f"float{tag}: critic elements outside the range when a step after a critic update begins: {reclipped}")
    worst = {}
    for k in sd0:
        a, b = out[f"traj.sd32.{k}"].astype(np.float64), out[f"traj.sd64.{k}"].astype(np.float64)
        worst[k] = float(np.abs(a - b).max())
    print("float32 run's max abs deviation from float64 after 7 steps:", {k: f"{v:.2e}" for k, v in worst.items()})


def main():
    ref = import_reference()
    out = {}
    torch.manual_seed(61)                                  # a seed at which both BatchNorm weights of the critic meet the assertion below
    m = build(ref, 4)
    with torch.no_grad():
        for k, p in m.named_parameters():                   # rounded to bf16-representable values: the stored arrays compress to half
            if k in D_NORM_WEIGHTS:                         # init 1: all of it would be clipped one way
                p.copy_((torch.randn_like(p) * 0.15).bfloat16().float())
            else:
                p.copy_((p + torch.randn_like(p) * (0.06 if k.startswith("discriminator.") else 0.03)).bfloat16().float())
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    up = down = kept = 0
    for k, p in m.named_parameters():
        if k.startswith("discriminator."):
            u, d, s = int((p > CLIP).sum()), int((p < -CLIP).sum()), int((p.abs() < CLIP).sum())
            up, down, kept = up + u, down + d, kept + s
            if k in D_NORM_WEIGHTS:
                assert u > 0 and d > 0 and s > 0, (k, u, d, s)
    assert up > 0 and down > 0 and kept > 0
    print(f"the first clip: {up} critic elements come down to +c, {down} up to -c, {kept} stay")
    for k, v in sd0.items():
        out[f"tiny.sd0.{k}"] = v.numpy().copy()
    out["tiny.names"] = np.array(list(sd0.keys()))
    out["tiny.pnames"] = np.array([k for k, _ in m.named_parameters()])
    out["tiny.clip_weight"], out["tiny.lr"], out["tiny.alpha"] = np.float64(CLIP), np.float64(LR), np.float64(ALPHA)
    u8, _ = images(5)
    out["tiny.imgs_u8"] = u8.numpy()
    for phase in ("g", "d"):
        run_step(ref, sd0, phase, u8.numpy(), out)
    run_traj(ref, sd0, out)
    path = os.path.join(OUT, "wgan_clip_kats.npz")
    np.savez_compressed(path, **out)
    print("wrote wgan_clip_kats.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
