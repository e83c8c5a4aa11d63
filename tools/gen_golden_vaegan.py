#!/usr/bin/env python3
"""Golden vectors for the VAE-GAN path (`experiment=vaegan/mnist`), produced by the REFERENCE VAEGAN.training_step.

Runs only where the reference checkout is (`REF` of tools/gen_golden_vae.py): imports its src/models/vae_gan.py and
src/networks/basic.py with that tool's import stubs and writes plain arrays to tests/golden/vaegan_kats.npz.  The reference's own
training_step runs unchanged (manual optimization: it steps both of its Adams itself); the stand-in LightningModule gets the two calls
it uses, `optimizers()` and `manual_backward`.  Both draws are pinned while a step runs: `torch.randn` hands out the stored prior draw,
and `torch.distributions.normal._standard_normal` (what `Normal.rsample` calls -- it does not go through `randn`) the stored eps, each
in the model's dtype, so that the float64 run sees the float32 numbers widened.  What each optimizer is handed is snapshotted by
wrapping its `step`; what netD returned in each of its three calls (logit and features) is recorded by a forward hook.
  tiny  : ngf = ndf = 4, latent_dim = 6 (not a multiple of 4), 5 x 1 x 28 x 28 images, every parameter perturbed away from its init and
          rounded to bf16-representable values -- the initial state_dict `tiny.sd0.`, the images (uint8: x = u8 / 127.5 - 1), and from
          sd0 ONE step under three settings (SETS below): the draws, the seven logged scalars, netD's three returns, the gradients
          handed to each optimizer (`grad_ae.`, `grad_d.`), and the state_dict after the step as its exact float32 difference `dsd1`
          to sd0 (or as it is: `sd1`).  "one" has recon_weight = 1: at the shipped weights the decoder's gradient is dominated by the
          adversarial term, and an error in the feature path could hide under its bound;
  traj  : the tiny model at the shipped MNIST setting for 4 batches on 6 fixed images per batch and fixed draws, in float32 and in
          float64: per batch the logged scalars of both runs and max|logit| of netD's three calls, and at the end the whole state_dict
          of both runs.
It also asserts on the reference that loss_mode="lsgan" gives the bits of "vanilla" (the reference never reads the setting).

    python tools/gen_golden_vaegan.py
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
NF, LATENT = 4, 6
SETS = {
    "mnist": dict(recon_weight=1e-3, lr=2e-4, b1=0.5, b2=0.999),            # configs/experiment/vaegan/mnist.yaml on the constructor's b2
    "model": dict(recon_weight=1e-4, lr=2e-4, b1=0.5, b2=0.99),             # configs/model/vae_gan.yaml
    "one": dict(recon_weight=1.0, lr=2e-4, b1=0.5, b2=0.999),               # the feature path at full weight
}
LOGS = ("train_loss/reg_loss", "train_loss/feature_recon_loss", "train_loss/g_adv_loss", "train_loss/d_adv_loss", "train_log/real_logit",
        "train_log/fake_logit", "train_log/recon_logit")


def import_reference():
    _import_vae()                                              # installs the stubs and the reference's path
    from src.models import vae_gan
    return vae_gan


def build(ref, cfg, loss_mode="vanilla"):
    dm = types.SimpleNamespace(width=28, height=28, channels=1, transforms=types.SimpleNamespace(normalize=True))
    kw = dict(latent_dim=LATENT, loss_mode=loss_mode, **cfg)
    m = ref.VAEGAN(dm, encoder=dict(ENC, ndf=NF), decoder=dict(DEC, ngf=NF), **kw)
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
def give_draws(eps, prior, dtype=torch.float32):
    """Inside the step, Normal.rsample's `_standard_normal` returns eps and `torch.randn(N, L)` the prior draw, each exactly once,
    eps first (vae_gan.py:69-70)."""
    import torch.distributions.normal as tdn
    inner_randn, inner_sn, used = torch.randn, tdn._standard_normal, []

    def randn(*shape, **kw):
        assert tuple(shape) == tuple(prior.shape) and used == ["eps"], (shape, used)
        used.append("prior")
        return prior.to(dtype)

    def standard_normal(shape, dtype, device):                      # noqa: ARG001
        assert tuple(shape) == tuple(eps.shape) and used == [], (shape, used)
        used.append("eps")
        return eps.to(dtype)
    torch.randn, tdn._standard_normal = randn, standard_normal
    try:
        yield
    finally:
        torch.randn, tdn._standard_normal = inner_randn, inner_sn
    assert used == ["eps", "prior"], used


class _Watch:
    """Records the gradients handed to each optimizer step and what netD returned in each call."""

    def __init__(self, m):
        self.m, self.steps, self.calls = m, [], []
        self.names = {id(p): k for k, p in m.named_parameters()}
        for opt in m._opts:
            self._wrap(opt)
        self.hook = m.netD.register_forward_hook(
            lambda mod, args, res: self.calls.append(tuple(r.detach().double().numpy().copy() for r in res)))

    def _wrap(self, opt):
        inner = opt.step

        def step(*a, **k):
            self.steps.append({self.names[id(p)]: p.grad.detach().clone() for g in opt.param_groups for p in g["params"] if p.grad is not None})
            return inner(*a, **k)
        opt.step = step

    def close(self):
        self.hook.remove()


def draws(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, LATENT, generator=g), torch.randn(n, LATENT, generator=g)


def run_tiny(ref, sd0, name, u8, out, loss_mode="vanilla"):
    m = build(ref, SETS[name], loss_mode)
    m.load_state_dict(sd0)
    arm(m.train())
    eps, prior = draws(u8.shape[0], 300)
    w = _Watch(m)
    with give_draws(eps, prior):
        m.training_step((decode_images(u8), None), 0)
    w.close()
    tag = f"tiny.{name}"
    assert set(m.logged) == set(LOGS) and len(w.steps) == 2 and len(w.calls) == 3, (m.logged, len(w.steps), len(w.calls))
    ae, d = w.steps
    assert ae and d and all(k.startswith(("encoder.", "decoder.")) for k in ae) and all(k.startswith("netD.") for k in d)
    rec = {"eps": eps.numpy(), "prior": prior.numpy(), "gnames_ae": np.array(list(ae.keys())), "gnames_d": np.array(list(d.keys()))}
    for call, (logit, feat) in zip(("fake", "real", "recon"), w.calls):          # the reference's order of netD calls
        assert logit.shape == (u8.shape[0], 1) and feat.shape == (u8.shape[0] * 4 * NF * 16,)
        rec[f"logit.{call}"], rec[f"feat.{call}"] = logit, feat
    for k in LOGS:
        rec[f"log.{k}"] = np.float64(m.logged[k])
    for k, gr in ae.items():
        rec[f"grad_ae.{k}"] = gr.numpy().copy()
    for k, gr in d.items():
        rec[f"grad_d.{k}"] = gr.numpy().copy()
    for k, v in m.state_dict().items():                     # float tensors as the exact difference to sd0 (it compresses)
        v = v.detach().numpy()
        if v.dtype.kind == "f":
            dd = v.astype(np.float64) - sd0[k].numpy().astype(np.float64)
            if np.array_equal(dd.astype(np.float32).astype(np.float64), dd):
                rec[f"dsd1.{k}"] = dd.astype(np.float32)
                continue
        rec[f"sd1.{k}"] = v.copy()
    print(tag, loss_mode, dict(m.logged))
    if out is not None:
        out.update({f"{tag}.{k}": v for k, v in rec.items()})
    return rec


TRAJ_N, TRAJ_BATCHES = 6, 4


def run_traj(ref, sd0, out):
    """Starts from tiny.sd0; the float64 run sees the same float32 numbers (weights, images, draws) widened."""
    g = torch.Generator().manual_seed(79)
    u8s, imgs = zip(*[images(TRAJ_N, g, levels=16) for _ in range(TRAJ_BATCHES)])
    eps = [torch.randn(TRAJ_N, LATENT, generator=g) for _ in range(TRAJ_BATCHES)]
    prior = [torch.randn(TRAJ_N, LATENT, generator=g) for _ in range(TRAJ_BATCHES)]
    out["traj.imgs_u8"] = torch.stack(u8s).numpy()
    out["traj.eps"], out["traj.prior"] = torch.stack(eps).numpy(), torch.stack(prior).numpy()
    for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
        m = build(ref, SETS["mnist"])
        m.load_state_dict(sd0)
        arm(m.to(dt).train())
        calls = []
        m.netD.register_forward_hook(lambda mod, args, res: calls.append(float(res[0].detach().abs().max())))
        for b in range(TRAJ_BATCHES):
            m.logged = {}
            del calls[:]
            with give_draws(eps[b], prior[b], dt):
                m.training_step((imgs[b].to(dt), None), b)
            assert set(m.logged) == set(LOGS) and len(calls) == 3
            out[f"traj.max_logit{tag}.{b}"] = np.array(calls)              # max|logit| of the fake, real and recon calls: the mean logits' scale
            for k, v in m.logged.items():
                out[f"traj.log{tag}.{b}.{k}"] = np.float64(v)
        for k, v in m.state_dict().items():
            out[f"traj.sd{tag}.{k}"] = v.detach().numpy().copy()


def main():
    ref = import_reference()
    out = {}
    torch.manual_seed(53)
    m = build(ref, SETS["mnist"])
    assert [k.split(".")[0] for k in m.state_dict()][0] == "decoder" and [k.split(".")[0] for k in m.state_dict()][-1] == "netD"
    with torch.no_grad():
        for p in m.parameters():                            # rounded to bf16-representable values: the stored arrays compress to half
            p.copy_((p + torch.randn_like(p) * 0.03).bfloat16().float())
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for k, v in sd0.items():
        out[f"tiny.sd0.{k}"] = v.numpy().copy()
    out["tiny.names"] = np.array(list(sd0.keys()))
    out["tiny.sets"] = np.array(list(SETS))
    for name, cfg in SETS.items():
        for k, v in cfg.items():
            out[f"tiny.cfg.{name}.{k}"] = np.float64(v)
    out["tiny.cfg.nf"], out["tiny.cfg.latent_dim"] = np.int64(NF), np.int64(LATENT)
    u8, _ = images(5, torch.Generator().manual_seed(5))
    out["tiny.imgs_u8"] = u8.numpy()
    recs = {name: run_tiny(ref, sd0, name, u8.numpy(), out) for name in SETS}
    # the reference never reads loss_mode: "lsgan" gives the bits of "vanilla"
    ls = run_tiny(ref, sd0, "mnist", u8.numpy(), None, loss_mode="lsgan")
    assert set(ls) == set(recs["mnist"]) and all(np.array_equal(ls[k], recs["mnist"][k]) for k in ls)
    run_traj(ref, sd0, out)
    path = os.path.join(OUT, "vaegan_kats.npz")
    np.savez_compressed(path, **out)
    print("wrote vaegan_kats.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
