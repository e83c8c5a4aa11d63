#!/usr/bin/env python3
"""Golden vectors for the InfoGAN path (`experiment=infogan/mnist`), produced by the REFERENCE InfoGAN.training_step.

Runs only where the reference checkout is (`REF` of tools/gen_golden_vae.py): imports its src/models/info_gan.py and
src/networks/basic.py with that tool's import stubs, plus a stub module for src.callbacks.visualization (which pulls in torchvision),
and writes plain arrays to tests/golden/infogan_kats.npz.  The reference's own training_step runs unchanged.  It is written for
Lightning's automatic optimization with two optimizers; there is no Lightning here, so THIS TOOL DRIVES THE LOOP ITSELF, the way
Lightning's loop does per batch: for optimizer_idx in (0, 1): training_step(batch, batch_idx, optimizer_idx) -> that optimizer's
zero_grad() -> loss.backward() -> step().  The draws are pinned: while a step runs, `torch.randint`, `Tensor.uniform_` and `torch.randn`
hand out stored values (`give_draws`), the last two in the model's dtype, so that the float64 run sees the float32 numbers widened.
What each optimizer is handed is snapshotted by wrapping its `step`: the stepped parameters' `.grad` at that moment.
  tiny  : ngf = ndf = 4, Dd = 2, V = 3, Cc = 3, Nz = 5, encode_dim = 36, lambda_I = 0.5, 5 x 1 x 28 x 28 images, every parameter
          perturbed away from its init and rounded to bf16-representable values -- the initial state_dict `tiny.sd0.`, the images
          (uint8: x = u8 / 127.5 - 1), and from sd0 phase 0 alone (`.p0.`) and phase 1 alone (`.p1.`): the latents, the logged scalars,
          the head outputs (logit: netD's calls one after the other; q: netQ's), the gradients handed to the stepping optimizer, and
          the state_dict after the step as its exact float32 difference `dsd1` to sd0 (or as it is: `sd1`);
  heads : ("default-heads") the two heads alone at the shipped widths, Dd = 1, V = 10, Cc = 2, encode_dim = 1024, lambda_I = 1, on random
          features [6, 1024]; the heads are the netD / netQ of a reference InfoGAN, run in float64 on float32 numbers: logit, q, the
          three losses, the gradient by the features and the Q gradients (of `1.weight` the feature rows `heads.w1_rows` only: the whole
          array would be a third of the file), and the float32 run's losses next to them (what float32 arithmetic alone costs);
  traj  : the tiny model for 3 batches (6 phases) at the shipped learning rates (lrG = 1e-3 and lrQ = 2e-4 inside one optimizer) on
          6 fixed images per batch and fixed draws, in float32 and in float64 -- per phase the logged scalars and the gradients handed
          to the optimizer (float64 run), after every phase the conv biases that sit in front of a BatchNorm, and at the end the
          whole state_dict of the float64 run and the running statistics of the float32 run;
  loss_mode : 1 if a tiny phase-0 and phase-1 step with loss_mode="lsgan" gave exactly what "vanilla" gave (asserted: the reference
          stores the hyper-parameter and never reads it).

    python tools/gen_golden_infogan.py
"""
import contextlib
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_vae import OUT, _stub, import_reference as _import_vae      # noqa: E402  (same stubs)
from gen_golden_aae import decode_images, images                            # noqa: E402

NETD = {"_target_": "src.networks.basic.ConvEncoder", "norm_type": "batch"}
NETG = {"_target_": "src.networks.basic.ConvDecoder", "norm_type": "batch"}
P0_LOGS = ("train_loss/g_loss", "train_loss/I_discrete_loss", "train_loss/I_continuous")
P1_LOGS = ("train_loss/d_loss", "train_log/pred_real", "train_log/pred_fake")
TINY = dict(nf=4, discrete_dim=2, discrete_value=3, continuous_dim=3, noise_dim=5, encode_dim=36, lambda_I=0.5)
HEADS = dict(nf=4, discrete_dim=1, discrete_value=10, continuous_dim=2, noise_dim=62, encode_dim=1024, lambda_I=1)
LRS = dict(lrG=1e-3, lrD=2e-4, lrQ=2e-4)
# conv biases in front of a BatchNorm layer: zero analytic gradient, a random walk under Adam (docs/kernels.md 4i)
BIASES = ("netG.network.0.bias", "netG.network.3.bias", "netG.network.6.bias", "common_layer.network.2.bias", "common_layer.network.5.bias")
BIAS_IN_FRONT = {"netG.network.1.running_mean": BIASES[0], "netG.network.4.running_mean": BIASES[1], "netG.network.7.running_mean": BIASES[2],
                 "common_layer.network.3.running_mean": BIASES[3], "common_layer.network.6.running_mean": BIASES[4]}


def import_reference():
    _import_vae()                                              # installs the stubs and the reference's path
    _stub("src.callbacks.visualization", get_grid_images=lambda *a, **k: None)
    from src.models import info_gan
    return info_gan


def build(ref, cfg, loss_mode="vanilla"):
    dm = types.SimpleNamespace(width=28, height=28, channels=1, transforms=types.SimpleNamespace(normalize=True))
    kw = {k: v for k, v in cfg.items() if k != "nf"}
    m = ref.InfoGAN(dm, netG=dict(NETG, ngf=cfg["nf"]), netD=dict(NETD, ndf=cfg["nf"]), loss_mode=loss_mode, **kw, **LRS)
    m.hparams = types.SimpleNamespace(loss_mode=loss_mode, b1=0.5, b2=0.999, **kw, **LRS)
    m.logged = {}
    return m


def draw(n, cfg, gen=None):
    """One phase's latents: (dis_c_index [n, Dd] int64, cont_c [n, Cc] in (-1, 1), z [n, Nz])."""
    idx = torch.randint(0, cfg["discrete_value"], (n, cfg["discrete_dim"]), generator=gen)
    cont = torch.rand(n, cfg["continuous_dim"], generator=gen) * 2 - 1
    return idx, cont, torch.randn(n, cfg["noise_dim"], generator=gen)


@contextlib.contextmanager
def give_draws(idx, cont, z, dtype=torch.float32):
    """Inside the step, `torch.randint(0, V, (N, Dd))`, `torch.zeros(N, Cc).uniform_(-1, 1)` and `torch.randn(N, Nz)` return the stored
    draws, each exactly once."""
    inner = torch.randint, torch.Tensor.uniform_, torch.randn
    used = []

    def randint(low, high, size, **kw):
        assert tuple(size) == tuple(idx.shape) and low == 0 and int(idx.max()) < high, (low, high, size)
        used.append("idx")
        return idx.clone()

    def uniform_(self, a=0.0, b=1.0, **kw):
        assert tuple(self.shape) == tuple(cont.shape) and (a, b) == (-1, 1), (self.shape, a, b)
        used.append("cont")
        return cont.to(dtype)

    def randn(*shape, **kw):
        assert tuple(shape) == tuple(z.shape), shape
        used.append("z")
        return z.to(dtype)
    torch.randint, torch.Tensor.uniform_, torch.randn = randint, uniform_, randn
    try:
        yield
    finally:
        torch.randint, torch.Tensor.uniform_, torch.randn = inner
    assert used == ["idx", "cont", "z"], used


class _Watch:
    """Records the gradients handed to each optimizer step and what netD and netQ returned in each call."""

    def __init__(self, m):
        self.m, self.steps, self.logits, self.qs = m, [], [], []
        self.names = {id(p): k for k, p in m.named_parameters()}
        for opt in m._opts:
            self._wrap(opt)
        self.hooks = [m.netD.register_forward_hook(lambda mod, args, res: self.logits.append(res.detach().double().numpy().copy())),
                      m.netQ.register_forward_hook(lambda mod, args, res: self.qs.append(res.detach().double().numpy().copy()))]

    def _wrap(self, opt):
        inner = opt.step

        def step(*a, **k):
            self.steps.append({self.names[id(p)]: p.grad.detach().clone() for g in opt.param_groups for p in g["params"] if p.grad is not None})
            return inner(*a, **k)
        opt.step = step

    def close(self):
        for h in self.hooks:
            h.remove()


def run_phase(m, batch, oi, draws, dtype=torch.float32):
    """What Lightning's automatic optimization does for optimizer `oi` of a batch."""
    m.logged = {}
    with give_draws(*draws, dtype=dtype):
        loss = m.training_step(batch, 0, oi)
    opt = m._opts[oi]
    opt.zero_grad()
    loss.backward()
    opt.step()
    return float(loss)


def stepped_prefixes(oi):
    return ("netG.", "netQ.") if oi == 0 else ("netD.", "common_layer.")


def run_tiny_phase(ref, sd0, oi, u8, out, loss_mode="vanilla", store=True):
    tag = f"tiny.p{oi}"
    m = build(ref, TINY, loss_mode)
    m.load_state_dict(sd0)
    m.train()
    m._opts = m.configure_optimizers()
    g = torch.Generator().manual_seed(100 + oi)
    draws = draw(u8.shape[0], TINY, g)
    w = _Watch(m)
    total = run_phase(m, (decode_images(u8), None), oi, draws)
    w.close()
    keys = P0_LOGS if oi == 0 else P1_LOGS
    assert set(m.logged) == set(keys) and len(w.steps) == 1 and len(w.logits) == (1, 2)[oi] and len(w.qs) == (1, 0)[oi]
    snap = w.steps[0]
    assert snap and all(k.startswith(stepped_prefixes(oi)) for k in snap)
    rec = {"idx": draws[0].numpy(), "cont": draws[1].numpy(), "z": draws[2].numpy(), "total": np.float64(total),
           "logit": np.concatenate([a.reshape(-1) for a in w.logits]), "gnames": np.array(list(snap.keys()))}
    if oi == 0:
        rec["q"] = w.qs[0]
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
    for k, v in m.state_dict().items():
        if k.endswith("num_batches_tracked"):
            want = 1 if (oi == 0 or k.startswith("netG.")) else 2
            assert int(v) == want, (k, int(v))
    if store:
        out.update({f"{tag}.{k}": v for k, v in rec.items()})
        print(tag, dict(m.logged), "total", total)
    return rec


def run_heads(ref, out):
    """The heads alone, phase 0's arithmetic on given features: g_loss + lambda_I (I_disc + I_cont)."""
    import torch.nn.functional as F
    torch.manual_seed(43)
    m = build(ref, HEADS)
    with torch.no_grad():
        for p in list(m.netD.parameters()) + list(m.netQ.parameters()):
            p.copy_(torch.round((p + torch.randn_like(p) * 0.03) * 256) / 256)          # multiples of 2^-8: the stored arrays compress
    n, cfg = 6, HEADS
    f = torch.randn(n, cfg["encode_dim"])
    idx, cont, _ = draw(n, cfg)
    out["heads.f"], out["heads.idx"], out["heads.cont"] = f.numpy(), idx.numpy(), cont.numpy()
    for name, mod in (("netD", m.netD), ("netQ", m.netQ)):
        for k, v in mod.state_dict().items():
            out[f"heads.sd.{name}.{k}"] = v.detach().numpy().copy()
    rows = np.unique(np.concatenate([np.arange(0, cfg["encode_dim"], 32), [cfg["encode_dim"] - 1]]))
    out["heads.w1_rows"] = rows
    res = {}
    for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
        netD, netQ = m.netD.to(dt), m.netQ.to(dt)
        for p in list(netD.parameters()) + list(netQ.parameters()):
            p.grad = None
        x = f.to(dt).requires_grad_(True)
        logit, q = netD(x), netQ(x)
        dis = q[:, :-cfg["continuous_dim"]].reshape(-1, cfg["discrete_value"], cfg["discrete_dim"])
        g_loss = F.binary_cross_entropy_with_logits(logit, torch.ones_like(logit))
        i_disc, i_cont = F.cross_entropy(dis, idx), F.mse_loss(q[:, -cfg["continuous_dim"]:], cont.to(dt))
        (g_loss + cfg["lambda_I"] * (i_disc + i_cont)).backward()
        res[tag] = dict(g_loss=float(g_loss), I_disc=float(i_disc), I_cont=float(i_cont))
        for k, v in res[tag].items():
            out[f"heads.{k}{tag}"] = np.float64(v)
        if tag == "64":
            out["heads.logit"], out["heads.q"] = logit.detach().numpy().reshape(-1), q.detach().numpy()
            out["heads.df"] = x.grad.numpy().copy()
            for k, p in netQ.named_parameters():
                gr = p.grad.numpy()
                out[f"heads.grad.netQ.{k}"] = (gr[:, rows] if k == "1.weight" else gr).copy()      # torch's [out, in]: the columns are the features
    print("heads", res, "float32 run's |I_disc32 - I_disc64| =", abs(res["32"]["I_disc"] - res["64"]["I_disc"]))


TRAJ_N, TRAJ_BATCHES = 6, 3


def run_traj(ref, sd0, out):
    """Starts from tiny.sd0; the float64 run sees the same float32 numbers (weights, images, draws) widened."""
    g = torch.Generator().manual_seed(77)
    u8s, imgs = zip(*[images(TRAJ_N, g, levels=16) for _ in range(TRAJ_BATCHES)])
    draws = [draw(TRAJ_N, TINY, g) for _ in range(2 * TRAJ_BATCHES)]
    out["traj.imgs_u8"] = torch.stack(u8s).numpy()
    for name, j in (("idx", 0), ("cont", 1), ("z", 2)):
        out[f"traj.{name}"] = torch.stack([d[j] for d in draws]).numpy()
    for k, v in LRS.items():
        out[f"traj.{k}"] = np.float64(v)
    out["traj.biases"] = np.array(BIASES)
    for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
        m = build(ref, TINY)
        m.load_state_dict(sd0)
        m = m.to(dt).train()
        m._opts = m.configure_optimizers()
        assert [g_["lr"] for g_ in m._opts[0].param_groups] == [LRS["lrG"], LRS["lrQ"]] and m._opts[1].param_groups[0]["lr"] == LRS["lrD"]
        w = _Watch(m)
        for i in range(2 * TRAJ_BATCHES):
            run_phase(m, (imgs[i // 2].to(dt), None), i % 2, draws[i], dt)
            assert set(m.logged) == set(P0_LOGS if i % 2 == 0 else P1_LOGS)
            for k, v in m.logged.items():
                out[f"traj.log{tag}.{i}.{k}"] = np.float64(v)
            sd = m.state_dict()
            for b in BIASES:
                out[f"traj.bias{tag}.{i}.{b}"] = sd[b].detach().double().numpy().copy()
        w.close()
        assert len(w.steps) == 2 * TRAJ_BATCHES
        if dt == torch.float64:
            for i, snap in enumerate(w.steps):
                assert all(k.startswith(stepped_prefixes(i % 2)) for k in snap)
                for k, gr in snap.items():
                    out[f"traj.grad64.{i}.{k}"] = gr.float().numpy().copy()      # rounded to float32: they only size a tolerance
        for k, v in m.state_dict().items():
            if dt == torch.float64 or "running_" in k:             # of the float32 run only what `misses` below is made from
                out[f"traj.sd{tag}.{k}"] = v.detach().numpy().copy()
            if k.endswith("num_batches_tracked"):                # G runs once per phase, the common layer once in phase 0 and twice in phase 1
                assert int(v) == (2 * TRAJ_BATCHES if k.startswith("netG.") else 3 * TRAJ_BATCHES), (k, int(v))
    out["traj.nbt.netG"], out["traj.nbt.common_layer"] = np.int64(2 * TRAJ_BATCHES), np.int64(3 * TRAJ_BATCHES)
    misses = []
    for k in sd0:
        if "running_" in k:
            a, b = torch.from_numpy(out[f"traj.sd32.{k}"]).double(), torch.from_numpy(out[f"traj.sd64.{k}"]).double()
            err, bound = float((a - b).abs().max()), 1e-5 * float(b.abs().max()) + 1e-5
            if err > bound:
                misses.append(k)
    print("running statistics whose float32 run misses 1e-5 * max|ref| + 1e-5 against the float64 run:", misses)
    assert set(misses) <= set(BIAS_IN_FRONT), misses            # only the means behind a conv bias
    out["traj.misses"] = np.array(misses, dtype=str)


def main():
    ref = import_reference()
    out = {}
    torch.manual_seed(41)
    m = build(ref, TINY)
    with torch.no_grad():
        for p in m.parameters():                            # rounded to bf16-representable values: the stored arrays compress to half
            p.copy_((p + torch.randn_like(p) * 0.03).bfloat16().float())
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for k, v in sd0.items():
        out[f"tiny.sd0.{k}"] = v.numpy().copy()
    out["tiny.names"] = np.array(list(sd0.keys()))
    out["tiny.pnames"] = np.array([k for k, _ in m.named_parameters()])
    for k, v in TINY.items():
        out[f"tiny.cfg.{k}"] = np.float64(v)
    u8, _ = images(5)
    out["tiny.imgs_u8"] = u8.numpy()
    same = True
    for oi in (0, 1):
        a = run_tiny_phase(ref, sd0, oi, u8.numpy(), out)
        b = run_tiny_phase(ref, sd0, oi, u8.numpy(), out, loss_mode="lsgan", store=False)
        same = same and set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert same, "loss_mode='lsgan' changed a number: the reference reads the hyper-parameter after all"
    out["loss_mode.lsgan_equals_vanilla"] = np.int64(same)
    print("loss_mode='lsgan' equals 'vanilla' in every recorded number:", same)
    run_heads(ref, out)
    run_traj(ref, sd0, out)
    path = os.path.join(OUT, "infogan_kats.npz")
    np.savez_compressed(path, **out)
    print("wrote infogan_kats.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
