#!/usr/bin/env python3
"""Golden vectors for the BiGAN path (`experiment=bigan/mnist`), produced by the REFERENCE BiGAN.training_step.

Runs only where the reference checkout is (`REF` of tools/gen_golden_vae.py): imports its src/models/BiGAN.py and
src/networks/basic.py with that tool's import stubs, plus empty stand-ins for `torchmetrics` and `torchvision`, which BiGAN.py
imports and never uses, and writes plain arrays to tests/golden/bigan_kats.npz,
bigan_modes_kats.npz and bigan_traj_kats.npz (FILES below: three files, each under 1 MiB; tests/_bigan_golden.py reads them as one).  The reference's own training_step runs unchanged
(manual optimization: it steps both of its Adams itself); the stand-in LightningModule gets the two calls it uses, `optimizers()` and
`manual_backward`, which passes its keywords (`retain_graph`, `inputs`) through.  The draw is pinned while a step runs: `torch.randn`
hands out the stored z in the model's dtype, so that the float64 run sees the float32 numbers widened.  What each optimizer is handed
is snapshotted by wrapping its `step`; what the discriminator and its dis_x returned in each of the two calls by forward hooks.
  tiny  : ndf = ngf = 4, latent_dim = 6 (pitch 8 in the encoder's output), hidden_dim = 128, 5 x 1 x 28 x 28 images, every parameter
          perturbed away from its init and rounded to bf16-representable values -- the initial state_dict `tiny.sd0.`, the images
          (uint8: x = u8 / 127.5 - 1), and from sd0 ONE step per loss mode: z, the four logged scalars, both logit vectors, the
          gradients handed to each optimizer (`grad_g.`, `grad_d.`) and the state_dict after the step as its exact float32 difference
          `dsd1` to sd0 (or as it is: `sd1`), every BatchNorm buffer and counter included.  "vanilla" stores everything, and dis_x's
          two outputs (`xf.real`, `xf.fake`: what the pair head read) as well.  A loss mode changes dlogit alone and the chain below it
          is linear, so "lsgan" and "hinge" store the scalars, the logits, the generator side's gradients in full, of the
          discriminator's gradients `dis_pair.*` only, and of the state after the step the buffers and the generator side's parameters.
          The counters are asserted here: 2 for dis_x's and dis_z's BatchNorm layers, 1 for the encoder's and the decoder's;
  init  : the reference's default-initialised state_dict under torch.manual_seed(INIT_SEED) at the tiny size: a tensor of up to
          INIT_FULL elements as it is, a larger one as the SHA-256 of its float32 bytes (`init.sha.`), which pins the same bits;
  traj  : the tiny model at the shipped learning rates for 4 batches of 6 fixed images and fixed z, in float32 and in float64: per
          batch the logged scalars of both runs and max|logit| of both calls, and at the end the float32 run's state_dict and the
          float64 run's as its difference to it, in float32.

    python tools/gen_golden_bigan.py
"""
import contextlib
import hashlib
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_vae import OUT, _stub, import_reference as _import_vae      # noqa: E402  (same stubs)
from gen_golden_aae import decode_images, images                            # noqa: E402

ENC = {"_target_": "src.networks.basic.ConvEncoder", "norm_type": "batch"}
DEC = {"_target_": "src.networks.basic.ConvDecoder", "norm_type": "batch"}
NF, LATENT, HIDDEN, INIT_SEED, INIT_FULL = 4, 6, 128, 71, 1024
CFG = dict(lrG=2e-4, lrD=2e-4, b1=0.5, b2=0.999)                            # configs/experiment/bigan/mnist.yaml
MODES = ("vanilla", "lsgan", "hinge")
# Three files, each below the repository's 1 MiB limit for a committed file; tests/_bigan_golden.py reads them as one.
FILES = {"bigan_kats.npz": "init, tiny.sd0, tiny.vanilla and the settings", "bigan_modes_kats.npz": "tiny.lsgan, tiny.hinge",
         "bigan_traj_kats.npz": "traj"}


def part_of(key):
    if key.startswith("traj."):
        return "bigan_traj_kats.npz"
    return "bigan_modes_kats.npz" if key.startswith(("tiny.lsgan.", "tiny.hinge.")) else "bigan_kats.npz"


LOGS = ("train_loss/g_loss", "train_loss/d_loss", "train_log/real_logit", "train_log/fake_logit")


def import_reference():
    _import_vae()                                              # installs the stubs and the reference's path
    _stub("torchmetrics")
    from src.models import BiGAN
    return BiGAN


def build(ref, loss_mode="vanilla"):
    dm = types.SimpleNamespace(width=28, height=28, channels=1, transforms=types.SimpleNamespace(normalize=True))
    kw = dict(latent_dim=LATENT, hidden_dim=HIDDEN, loss_mode=loss_mode, **CFG)
    m = ref.BiGAN(dm, encoder=dict(ENC, ndf=NF), decoder=dict(DEC, ngf=NF), **kw)
    m.hparams = types.SimpleNamespace(**kw)
    m.logged = {}
    return m


def arm(m):
    """The two Lightning calls the reference's manual optimization uses."""
    m._opts = list(m.configure_optimizers())
    m.optimizers = lambda: m._opts
    m.manual_backward = lambda loss, **kw: loss.backward(**kw)
    return m


@contextlib.contextmanager
def give_z(z, dtype=torch.float32):
    """Inside the step, `torch.randn(N, L)` returns z, exactly once (BiGAN.py:63)."""
    inner, used = torch.randn, []

    def randn(*shape, **kw):
        assert tuple(shape) == tuple(z.shape) and not used, (shape, used)
        used.append("z")
        return z.to(dtype)
    torch.randn = randn
    try:
        yield
    finally:
        torch.randn = inner
    assert used == ["z"], used


class _Watch:
    """Records the gradients handed to each optimizer step and what the discriminator and its dis_x returned in each call."""

    def __init__(self, m):
        self.steps, self.logits, self.xf = [], [], []
        self.names = {id(p): k for k, p in m.named_parameters()}
        for opt in m._opts:
            self._wrap(opt)
        self.hooks = [m.discriminator.register_forward_hook(lambda mod, args, res: self.logits.append(res.detach().double().numpy().copy())),
                      m.discriminator.dis_x.register_forward_hook(lambda mod, args, res: self.xf.append(res.detach().double().numpy().copy()))]

    def _wrap(self, opt):
        inner = opt.step

        def step(*a, **k):
            self.steps.append({self.names[id(p)]: p.grad.detach().clone() for g in opt.param_groups for p in g["params"] if p.grad is not None})
            return inner(*a, **k)
        opt.step = step

    def close(self):
        for h in self.hooks:
            h.remove()


def check_counters(m):
    for k, v in m.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == (2 if k.startswith("discriminator.") else 1), (k, int(v))


def run_tiny(ref, sd0, mode, u8, out):
    m = build(ref, mode)
    m.load_state_dict(sd0)
    arm(m.train())
    z = torch.randn(u8.shape[0], LATENT, generator=torch.Generator().manual_seed(300))
    w = _Watch(m)
    with give_z(z):
        m.training_step((decode_images(u8), None), 0)
    w.close()
    check_counters(m)
    full = mode == "vanilla"
    assert set(m.logged) == set(LOGS) and len(w.steps) == 2 and len(w.logits) == 2 and len(w.xf) == 2
    gg, gd = w.steps
    assert gg and gd and all(k.startswith(("encoder.", "decoder.")) for k in gg) and all(k.startswith("discriminator.") for k in gd)
    rec = {"z": z.numpy(), "gnames_g": np.array(list(gg.keys())), "gnames_d": np.array(list(gd.keys())),
           "logit.real": w.logits[0][:, 0], "logit.fake": w.logits[1][:, 0]}
    if full:
        rec["xf.real"], rec["xf.fake"] = w.xf
    for k in LOGS:
        rec[f"log.{k}"] = np.float64(m.logged[k])
    for k, gr in gg.items():
        rec[f"grad_g.{k}"] = gr.numpy().copy()
    for k, gr in gd.items():
        if full or k.startswith("discriminator.dis_pair."):
            rec[f"grad_d.{k}"] = gr.numpy().copy()
    params = {k for k, _ in m.named_parameters()}
    for k, v in m.state_dict().items():                     # float tensors as the exact difference to sd0 (it compresses)
        if not full and k in params and k.startswith("discriminator."):
            continue
        v = v.detach().numpy()
        if v.dtype.kind == "f":
            dd = v.astype(np.float64) - sd0[k].numpy().astype(np.float64)
            if np.array_equal(dd.astype(np.float32).astype(np.float64), dd):
                rec[f"dsd1.{k}"] = dd.astype(np.float32)
                continue
        rec[f"sd1.{k}"] = v.copy()
    print("tiny", mode, dict(m.logged))
    out.update({f"tiny.{mode}.{k}": v for k, v in rec.items()})


TRAJ_N, TRAJ_BATCHES = 6, 4


def run_traj(ref, sd0, out):
    """Starts from tiny.sd0; the float64 run sees the same float32 numbers (weights, images, z) widened."""
    g = torch.Generator().manual_seed(79)
    u8s, imgs = zip(*[images(TRAJ_N, g, levels=16) for _ in range(TRAJ_BATCHES)])
    zs = [torch.randn(TRAJ_N, LATENT, generator=g) for _ in range(TRAJ_BATCHES)]
    out["traj.imgs_u8"] = torch.stack(u8s).numpy()
    out["traj.z"] = torch.stack(zs).numpy()
    sds = {}
    for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
        m = build(ref, "vanilla")
        m.load_state_dict(sd0)
        arm(m.to(dt).train())
        calls = []
        m.discriminator.register_forward_hook(lambda mod, args, res: calls.append(float(res.detach().abs().max())))
        for b in range(TRAJ_BATCHES):
            m.logged = {}
            del calls[:]
            with give_z(zs[b], dt):
                m.training_step((imgs[b].to(dt), None), b)
            assert set(m.logged) == set(LOGS) and len(calls) == 2
            out[f"traj.max_logit{tag}.{b}"] = np.array(calls)              # max|logit| of the real and the fake call: the mean logits' scale
            for k, v in m.logged.items():
                out[f"traj.log{tag}.{b}.{k}"] = np.float64(v)
        sds[tag] = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    for k, v in sds["32"].items():
        out[f"traj.sd32.{k}"] = v
        if v.dtype.kind == "f":
            out[f"traj.d64.{k}"] = (sds["64"][k] - v.astype(np.float64)).astype(np.float32)
        else:
            assert np.array_equal(v, sds["64"][k])


def main():
    ref = import_reference()
    out = {}
    torch.manual_seed(INIT_SEED)
    m = build(ref)
    names = list(m.state_dict())
    assert names[0].startswith("decoder.") and names[-1].startswith("discriminator.dis_pair.")
    out["init.seed"] = np.int64(INIT_SEED)
    for k, v in m.state_dict().items():
        v = np.ascontiguousarray(v.detach().numpy())
        if v.size <= INIT_FULL:
            out[f"init.{k}"] = v.copy()
        else:
            out[f"init.sha.{k}"] = np.frombuffer(hashlib.sha256(v.tobytes()).digest(), dtype=np.uint8).copy()
    torch.manual_seed(53)
    with torch.no_grad():
        for p in m.parameters():                            # rounded to bf16-representable values: the stored arrays compress to half
            p.copy_((p + torch.randn_like(p) * 0.03).bfloat16().float())
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for k, v in sd0.items():
        out[f"tiny.sd0.{k}"] = v.numpy().copy()
    out["tiny.names"] = np.array(names)
    out["tiny.modes"] = np.array(MODES)
    for k, v in CFG.items():
        out[f"tiny.cfg.{k}"] = np.float64(v)
    out["tiny.cfg.nf"], out["tiny.cfg.latent_dim"], out["tiny.cfg.hidden_dim"] = np.int64(NF), np.int64(LATENT), np.int64(HIDDEN)
    u8, _ = images(5, torch.Generator().manual_seed(5))
    out["tiny.imgs_u8"] = u8.numpy()
    for mode in MODES:
        run_tiny(ref, sd0, mode, u8.numpy(), out)
    run_traj(ref, sd0, out)
    for name, keep in FILES.items():
        path = os.path.join(OUT, name)
        with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as zf:  # what np.load reads; 4 % smaller than savez_compressed's deflate
            for k, v in out.items():
                if part_of(k) != name:
                    continue
                buf = io.BytesIO()
                np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
                zf.writestr(k + ".npy", buf.getvalue())
        print("wrote", name, os.path.getsize(path))
        assert os.path.getsize(path) < 1 << 20, name                        # no committed file above 1 MiB


if __name__ == "__main__":
    main()
