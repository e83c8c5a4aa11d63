#!/usr/bin/env python3
"""Golden vectors for the FactorVAE path (`experiment=factor_vae/celeba`), produced by the REFERENCE FactorVAE.training_step.

Runs only where the reference checkout is (`REF` of tools/gen_golden_vae.py): imports its src/models/factor_vae.py and
src/networks/conv64.py with that tool's import stubs and writes plain arrays to tests/golden/factor_vae_kats.npz.  The reference's
own code runs unchanged on known random draws: `torch.distributions.normal._standard_normal`, the one draw inside
`Normal.rsample()`, hands out the stored eps1 then eps2, and `torch.randperm`, which `permute_dims` calls once per latent column,
hands out the stored rows of perm [L, N].  The manual-optimization hooks the step uses (`optimizers()`, `log()`) are stubs.
  tiny : ndf = ngf = 4, latent 10, 6 x 1 x 64 x 64 images (halves of 3: odd), norm_type None, adv_weight 6.4, every parameter
         perturbed away from its init (and rounded to bf16-representable values) -- initial state_dict, images (uint8: x = u8 / 127.5 - 1), eps1, eps2, perm, the six logged scalars, netD's two inputs (z1 and the permuted z2), every parameter's
         .grad after the step (encoder / decoder from the encoder loss, netD from the discriminator loss), the state_dict after
         both Adam steps as its exact float32 difference `dsd1` to the initial one (netD's running statistics among it;
         num_batches_tracked == 2 as `sd1`);
  cfg  : configs/model/factor_vae.yaml + configs/networks/conv_64.yaml sizes (ngf = ndf = 64, latent 10, 3 x 64 x 64), 8 images,
         weights = the seeded default init (torch.manual_seed(32)) -- images, draws, scalars, names, per-parameter weight / gradient
         statistics;
  traj : the tiny model for 3 steps (the shipped lr = 2e-4, lrD = 1e-4) on 16 fixed images per step (16 grey levels) and fixed
         draws, run twice in the reference: in float32
         and with the model in float64 -- per step the six scalars of each run, after step 3 `netD.classifier.fc.weight` and
         `encoder.main.0.weight` of both runs.

    python tools/gen_golden_factor_vae.py
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_vae import OUT, import_reference as _import_vae      # noqa: E402  (same stubs)

ENC = {"_target_": "src.networks.conv64.Encoder", "norm_type": None}
DEC = {"_target_": "src.networks.conv64.Decoder", "norm_type": None}
LOGS = ("train_loss/reg_loss", "train_loss/recon_loss", "train_loss/d_adv_loss", "train_loss/g_adv_loss", "train_log/real_logit",
        "train_log/fake_logit")
ADV_WEIGHT = 6.4


def import_reference():
    _import_vae()                                              # installs the stubs and the reference's path
    sys.modules["omegaconf"].OmegaConf = object
    from src.models import factor_vae
    factor_vae.FactorVAE.optimizers = lambda self: self._opts
    return factor_vae


class _GivenDraws:
    """Hands `Normal.rsample()` the queued eps tensors (in the distribution's dtype) and `torch.randperm` the queued permutations."""

    def __init__(self):
        self.eps, self.perms = [], []
        import torch.distributions.normal as N
        N._standard_normal = self._normal
        torch.randperm = self._randperm

    def give(self, eps1, eps2, perm):
        self.eps, self.perms = [eps1, eps2], [row for row in perm]

    def _normal(self, shape, dtype, device):
        e = self.eps.pop(0)
        assert tuple(shape) == tuple(e.shape), (shape, e.shape)
        return e.to(dtype=dtype, device=device)

    def _randperm(self, n, *a, **k):
        p = self.perms.pop(0)
        assert p.shape == (n,)
        return p.clone()


def build(ref, nf, channels, latent=10, lr=2e-4, lrD=1e-4):
    dm = types.SimpleNamespace(width=64, height=64, channels=channels, transforms=types.SimpleNamespace(normalize=True))
    m = ref.FactorVAE(dm, encoder=dict(ENC, ndf=nf), decoder=dict(DEC, ngf=nf), latent_dim=latent, adv_weight=ADV_WEIGHT)
    m.hparams = types.SimpleNamespace(latent_dim=latent, loss_mode="lsgan", adv_weight=ADV_WEIGHT, lr=lr, lrD=lrD, ae_b1=0.9, ae_b2=0.999,
                                      adv_b1=0.5, adv_b2=0.9)
    m.logged = {}
    return m


def images(n, channels, gen=None, levels=256):
    """Random 8-bit images: stored as uint8 (a quarter of the bytes), used as u8 / 127.5 - 1 in float32.  levels=16: 16 grey levels
    (multiples of 17), which halves the stored bytes again."""
    u8 = (torch.randint(0, levels, (n, channels, 64, 64), generator=gen, dtype=torch.int64) * (255 // (levels - 1))).to(torch.uint8)
    return u8, decode_images(u8.numpy())


def decode_images(u8):
    return torch.from_numpy(u8.astype(np.float32) / np.float32(127.5) - np.float32(1))


def draws(n, latent, gen=None):
    n1 = (n + 1) // 2
    n2 = n - n1
    eps1, eps2 = torch.randn(n1, latent, generator=gen), torch.randn(n2, latent, generator=gen)
    perm = torch.stack([torch.argsort(torch.rand(n2, generator=gen)) for _ in range(latent)])
    return eps1, eps2, perm


def run_case(ref, given, tag, nf, channels, n, seed, out, full):
    torch.manual_seed(seed)
    latent = 10
    m = build(ref, nf, channels)
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
    u8, imgs = images(n, channels)
    eps1, eps2, perm = draws(n, latent)
    given.give(eps1, eps2, perm)
    out[f"{tag}.imgs_u8"], out[f"{tag}.eps1"], out[f"{tag}.eps2"], out[f"{tag}.perm"] = u8.numpy(), eps1.numpy(), eps2.numpy(), perm.numpy()
    out[f"{tag}.adv_weight"] = np.float64(ADV_WEIGHT)
    seen = []
    hook = m.netD.register_forward_hook(lambda mod, args, res: seen.append(args[0].detach().numpy().copy()))
    m.training_step((imgs, None), 0)
    hook.remove()
    if full:                                                # what netD read: z1, then the permuted z2 (tests/test_latent_disc_cpu.py)
        out[f"{tag}.netD_in"] = np.stack(seen)
    for k in LOGS:
        out[f"{tag}.log.{k}"] = np.float64(m.logged[k])
    out[f"{tag}.gstats"] = np.array([[float(p.grad.double().sum()), float(p.grad.double().norm())] for _, p in m.named_parameters()])
    if full:
        for k, p in m.named_parameters():
            out[f"{tag}.grad.{k}"] = p.grad.numpy().copy()
        for k, v in m.state_dict().items():                 # float tensors as the exact difference to sd0 (one Adam step: it compresses)
            v = v.detach().numpy()
            if v.dtype.kind == "f":
                d = v.astype(np.float64) - out[f"{tag}.sd0.{k}"].astype(np.float64)
                assert np.array_equal(d.astype(np.float32).astype(np.float64), d), k
                out[f"{tag}.dsd1.{k}"] = d.astype(np.float32)
            else:
                out[f"{tag}.sd1.{k}"] = v.copy()
        assert int(m.netD.model[1].norm.num_batches_tracked) == 2
    print(tag, dict(m.logged))


TRAJ_LR, TRAJ_LRD, TRAJ_N = 2e-4, 1e-4, 16       # the shipped learning rates; halves of 8 rows (see run_traj)


def run_traj(ref, given, out):
    """Starts from tiny.sd0; the float64 run sees the same float32 numbers (weights, images, draws) widened.
    16 images per step, not the tiny case's 6: netD's BatchNorm1d over halves of 3 rows is so ill-conditioned that the reference's own
    float32 run leaves its float64 run by 1e-4 relative after one optimizer step (9.3e-5, 3.6e-4 at steps 2, 3 with 6 images and lr
    1e-3; 4.2e-5, 1.3e-5 at the shipped learning rates), a level at which any two float32 evaluations differ by as much and a bound of
    4x one of them is a coin toss.  With halves of 8 rows the same reference stays within 1.3e-6 of its float64 run at every step."""
    sd0 = {k[len("tiny.sd0."):]: torch.from_numpy(v) for k, v in out.items() if k.startswith("tiny.sd0.")}
    g = torch.Generator().manual_seed(77)
    u8s, imgs = zip(*[images(TRAJ_N, 1, g, levels=16) for _ in range(3)])
    dr = [draws(TRAJ_N, 10, g) for _ in range(3)]
    out["traj.imgs_u8"] = torch.stack(u8s).numpy()
    out["traj.eps1"], out["traj.eps2"], out["traj.perm"] = (torch.stack([d[i] for d in dr]).numpy() for i in range(3))
    out["traj.lr"], out["traj.lrD"] = np.float64(TRAJ_LR), np.float64(TRAJ_LRD)
    res = {}
    for dt in (torch.float32, torch.float64):
        m = build(ref, 4, 1, lr=TRAJ_LR, lrD=TRAJ_LRD)
        m.load_state_dict(sd0)
        m = m.to(dt).train()
        m._opts = m.configure_optimizers()
        logs = []
        for x, d in zip(imgs, dr):
            given.give(*d)
            m.training_step((x.to(dt), None), 0)
            logs.append([m.logged[k] for k in LOGS])
        res[dt] = (np.array(logs, dtype=np.float64), m.netD.classifier.fc.weight.detach().double().numpy().copy(),
                   m.encoder.main[0].weight.detach().double().numpy().copy())
    out["traj.logs32"], out["traj.dw32"], out["traj.ew32"] = res[torch.float32]
    out["traj.logs64"], out["traj.dw64"], out["traj.ew64"] = res[torch.float64]
    out["traj.log_keys"] = np.array(LOGS)
    print("traj logs64", out["traj.logs64"])
    print("float32 run's relative deviation per step and scalar", np.abs(out["traj.logs32"] - out["traj.logs64"]) / np.abs(out["traj.logs64"]))
    print("netD.classifier.fc.weight / encoder.main.0.weight: float32 run's max abs deviation from float64",
          np.abs(out["traj.dw32"] - out["traj.dw64"]).max(), np.abs(out["traj.ew32"] - out["traj.ew64"]).max())


def main():
    ref = import_reference()
    given = _GivenDraws()
    out = {}
    run_case(ref, given, "tiny", 4, 1, 6, 31, out, True)        # everything stored
    run_case(ref, given, "cfg", 64, 3, 8, 32, out, False)       # factor_vae.yaml + conv_64.yaml sizes, seeded default init
    run_traj(ref, given, out)
    path = os.path.join(OUT, "factor_vae_kats.npz")
    np.savez_compressed(path, **out)
    print("wrote factor_vae_kats.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
