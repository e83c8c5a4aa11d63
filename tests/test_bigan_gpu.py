"""BiGAN path (`experiment=bigan/mnist`) on the HIP kernels against the reference's vectors (tests/golden/bigan_*kats.npz, read as one by tests/_bigan_golden.py; produced by
the reference's own BiGAN.training_step: tools/gen_golden_bigan.py).  The bounds are those of tests/test_vaegan_gpu.py's docstring,
which that file takes from the AGE and GAN tests: a logged scalar within 1e-5 |ref| + 1e-6, logits within 1e-5 max|ref| + 1e-5, a
gradient handed to an optimizer within 2e-4 max|ref| + 1e-5, a running statistic within 1e-5 max|ref| + 1e-5, a stepped parameter
within its first-Adam-step bound, the counters exact.  The trajectory's final state is held to 4 x the gap between the reference's own
float32 and float64 runs, tensor by tensor; its logged scalars to 1e-5 |f64| + 1e-6, where a mean logit takes max|logit| of that call
in the float64 run as its scale.

A bias directly in front of a BatchNorm has an analytically zero gradient: what the reference records for it is the rounding noise of
its own float32 backward.  For these biases (ZERO_GRAD_BIAS: the conv biases in front of a BatchNorm in the three conv nets, and
discriminator.dis_z.model.1.fc.bias, the Linear in front of BatchNorm1d) -- and for no other tensor -- the reference's recorded noise is
the yardstick, as in tests/test_vaegan_gpu.py: this path's value, and its difference to the record, each stay within
4 max|ref| + 1e-5, and their Adam bound uses that gradient tolerance.

"lsgan" and "hinge" change dlogit alone, and the chain below it is linear: the file holds their scalars, logits, the generator side's
gradients and dis_pair's, and of the state after the step the buffers and the generator side's parameters (tools/gen_golden_bigan.py)."""
import copy
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bigan_golden  # noqa: E402

pytestmark = pytest.mark.gpu
M = importlib.import_module("image-generation-models_amd.src.models.BiGAN")
ENC = {"_target_": "src.networks.basic.ConvEncoder", "norm_type": "batch"}
DEC = {"_target_": "src.networks.basic.ConvDecoder", "norm_type": "batch"}
DM = {"width": 28, "height": 28, "channels": 1, "transforms": {"normalize": True}}
MODES = ("vanilla", "lsgan", "hinge")
ZERO_GRAD_BIAS = ("decoder.network.0.bias", "decoder.network.3.bias", "decoder.network.6.bias", "encoder.network.2.bias", "encoder.network.5.bias",
                  "discriminator.dis_x.network.2.bias", "discriminator.dis_x.network.5.bias", "discriminator.dis_z.model.1.fc.bias")
BN_UPDATES = {"decoder": 1, "encoder": 1, "discriminator": 2}


def _model(seed=None, **kw):
    if seed is not None:
        torch.manual_seed(seed)
    return M.BiGAN(DM, encoder=dict(ENC, ndf=4), decoder=dict(DEC, ngf=4), **{"latent_dim": 6, "hidden_dim": 128, **kw})


def _images(u8):
    """tools/gen_golden_aae.py::decode_images"""
    return torch.from_numpy(u8.astype(np.float32) / np.float32(127.5) - np.float32(1))


def _close(a, b, rel, what=""):
    """tests/test_gan_gpu.py::_close"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    print(f"{what}: max err {err:.3e}, max|ref| {scale:.3e}, bound {rel * scale + 1e-5:.3e}")
    assert err <= rel * scale + 1e-5, f"{what}: max err {err:.3e} > {rel} * max |ref| ({scale:.3e}) + 1e-5"


@pytest.fixture(scope="module")
def kats(golden_dir):
    return _bigan_golden.load(golden_dir)


def _cfg(g):
    return {k: float(g[f"tiny.cfg.{k}"]) for k in ("lrG", "lrD", "b1", "b2")}


def _tiny(g, mode="vanilla"):
    m = _model(loss_mode=mode, **_cfg(g))
    sd = {str(k): torch.from_numpy(g[f"tiny.sd0.{k}"]) for k in g["tiny.names"]}
    assert list(m.state_dict().keys()) == list(sd.keys())
    m.load_state_dict(sd)
    return m.cuda().train(), sd


def _net_names(m):
    D = m.discriminator
    return {id(m.encoder): "encoder", id(m.decoder): "decoder", id(D.dis_z): "discriminator.dis_z", id(D.dis_x): "discriminator.dis_x",
            id(D.dis_pair): "discriminator.dis_pair"}


def _watch_steps(m):
    """The gradients handed to each optimizer step, snapshotted by wrapping `step` like the generator does."""
    snaps, names = [], _net_names(m)
    for opt in m.optimizers():
        def step(*a, _inner=opt.step, _opt=opt, **k):
            snaps.append({f"{names[id(n)]}.{key}": p.grad.detach().clone() for n in _opt.nets for key, p in n.named_parameters()})
            return _inner(*a, **k)
        opt.step = step
    return snaps


def _watch_head(m):
    recs, inner = [], m.discriminator.pair_forward

    def pair_forward(*a, **kw):
        rec = inner(*a, **kw)
        recs.append(rec)
        return rec
    m.discriminator.pair_forward = pair_forward
    return recs


def _step(m, x, b, z):
    logged = {}
    m.log = lambda k, v, *a, **kw: logged.__setitem__(k, v)
    out = m.training_step((x, None), b, z=z)
    assert out is None                                                                 # manual optimization
    assert all(torch.is_tensor(v) and v.is_cuda for v in logged.values())              # logged scalars stay on the device
    return {k: float(v) for k, v in logged.items()}


@pytest.mark.parametrize("mode", MODES)
def test_tiny_step_matches_reference(kats, mode):
    g, tag = kats, f"tiny.{mode}"
    cfg = _cfg(g)
    m, sd0 = _tiny(g, mode)
    snaps, recs = _watch_steps(m), _watch_head(m)
    N = 5
    logged = _step(m, _images(g["tiny.imgs_u8"]).cuda(), 0, torch.from_numpy(g[f"{tag}.z"]).cuda())
    assert set(logged) == set(M.LOGS)
    for key in M.LOGS:
        print(f"{key}: {logged[key]:.8g} reference {float(g[f'{tag}.log.{key}']):.8g}")
    for key in M.LOGS:
        ref = float(g[f"{tag}.log.{key}"])
        assert abs(logged[key] - ref) <= 1e-5 * abs(ref) + 1e-6, key
    assert len(recs) == 1 and recs[0]["logit"].shape == (2 * N,)
    _close(recs[0]["logit"][:N], torch.from_numpy(g[f"{tag}.logit.real"]), 1e-5, f"{tag} logit.real")
    _close(recs[0]["logit"][N:], torch.from_numpy(g[f"{tag}.logit.fake"]), 1e-5, f"{tag} logit.fake")
    # the two optimizer steps' gradients: encoder + decoder, then the discriminator's three parts
    assert len(snaps) == 2 and sorted(snaps[0]) == sorted(str(k) for k in g[f"{tag}.gnames_g"])
    assert sorted(snaps[1]) == sorted(str(k) for k in g[f"{tag}.gnames_d"])
    gref = {**{str(k): g[f"{tag}.grad_g.{k}"] for k in g[f"{tag}.gnames_g"]},
            **{str(k): g[f"{tag}.grad_d.{k}"] for k in g[f"{tag}.gnames_d"] if f"{tag}.grad_d.{k}" in g.files}}
    if mode == "vanilla":
        assert set(gref) == set(snaps[0]) | set(snaps[1])                               # everything is held for vanilla
    else:
        assert set(gref) == set(snaps[0]) | {k for k in snaps[1] if k.startswith("discriminator.dis_pair.")}

    def dg_of(k):
        """The gradient tolerance of parameter k: 2e-4 max|ref| + 1e-5; for a zero-gradient bias 4 max|ref| + 1e-5 (the docstring)."""
        return (4.0 if k in ZERO_GRAD_BIAS else 2e-4) * float(np.abs(gref[k]).max()) + 1e-5
    bad = []
    for k, gr in {**snaps[0], **snaps[1]}.items():
        if k not in gref:
            continue
        ref = torch.from_numpy(gref[k])
        got = gr.detach().float().cpu()
        err = float((got - ref).abs().max())
        print(f"{tag} grad {k}: max|hip| {float(got.abs().max()):.3e}, max|ref| {float(ref.abs().max()):.3e}, max err {err:.3e}, bound {dg_of(k):.3e}")
        if err > dg_of(k) or (k in ZERO_GRAD_BIAS and float(got.abs().max()) > dg_of(k)):
            bad.append((k, err, dg_of(k)))
    assert not bad, bad
    # the state after the step: one Adam update (tests/test_gan_gpu.py's derivation), the BatchNorm counters, the running statistics
    sd1, checked = m.state_dict(), 0
    for k in sd0:
        lr = cfg["lrD"] if k.startswith("discriminator.") else cfg["lrG"]
        if k.endswith("num_batches_tracked"):
            assert int(sd1[k]) == int(g[f"{tag}.sd1.{k}"]) == BN_UPDATES[k.split(".")[0]], k
            continue
        if f"{tag}.sd1.{k}" in g.files:
            ref = torch.from_numpy(g[f"{tag}.sd1.{k}"]).double()
        elif f"{tag}.dsd1.{k}" in g.files:
            ref = sd0[k].double() + torch.from_numpy(g[f"{tag}.dsd1.{k}"]).double()
        else:
            assert mode != "vanilla" and k.startswith("discriminator.") and "running_" not in k, k
            continue
        checked += 1
        got = sd1[k].detach().double().cpu()
        if "running_" in k:
            _close(got, ref, 1e-5, f"{tag} {k}")
            assert float((got - sd0[k].double()).abs().max()) > 0, k
        else:
            g1 = torch.from_numpy(gref[k]).double()
            tol = torch.clamp(lr * dg_of(k) / (g1.abs() + 1e-8), max=2 * lr) + 2e-7 * float(ref.abs().max())
            over = (got - ref).abs() > tol
            assert not bool(over.any()), (k, int(over.sum()), float((got - ref).abs().max()))
            moved = float((got - sd0[k].double()).abs().max())
            assert 0 < moved <= lr + 1e-7, (k, moved)                                  # every tensor moved, by one Adam update
    if mode == "vanilla":
        assert checked == sum(not k.endswith("num_batches_tracked") for k in sd0)
    assert [o.device_step_count() for o in m.optimizers()] == [1, 1]


def test_trajectory_matches_the_float64_reference(kats):
    """4 batches from tiny.sd0 on the fixture's images and z at the shipped learning rates, against the reference's float64 run: every
    tensor of the final state within 4 x the reference's own float32-to-float64 gap for that tensor."""
    g = kats
    m, _ = _tiny(g)
    calls = {"train_log/real_logit": 0, "train_log/fake_logit": 1}
    bad = []
    for b in range(4):
        logs = _step(m, _images(g["traj.imgs_u8"][b]).cuda(), b, torch.from_numpy(g["traj.z"][b]).cuda())
        assert set(logs) == set(M.LOGS)
        for key, val in logs.items():
            ref = float(g[f"traj.log64.{b}.{key}"])
            scale = float(g[f"traj.max_logit64.{b}"][calls[key]]) if key in calls else abs(ref)
            print(f"batch {b} {key}: {val:.8g} float64 reference {ref:.8g} (its float32 run {float(g[f'traj.log32.{b}.{key}']):.8g})")
            if abs(val - ref) > 1e-5 * scale + 1e-6:
                bad.append((b, key, val, ref))
    assert not bad, bad
    sd, over = m.state_dict(), []
    for k in g["tiny.names"]:
        k = str(k)
        ref32 = g[f"traj.sd32.{k}"].astype(np.float64)
        got = sd[k].detach().double().cpu().numpy()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(ref32) == 4 * BN_UPDATES[k.split(".")[0]], k
            continue
        d64 = g[f"traj.d64.{k}"].astype(np.float64)                                     # the float64 run's state minus the float32 run's
        gap, err = float(np.abs(d64).max()), float(np.abs(got - (ref32 + d64)).max())
        print(f"{k}: max|hip - f64| {err:.3e}, the reference's max|f32 - f64| {gap:.3e}")
        if err > 4 * gap:
            over.append((k, err, gap))
    assert not over, over


def _state(m):
    out = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for i, opt in enumerate(m.optimizers()):
        sd = opt.state_dict()
        out[f"opt{i}.step"] = torch.tensor(sd["step"])
        for name in ("m", "v"):
            for j, t in enumerate(sd[name] or []):
                out[f"opt{i}.{name}{j}"] = t.detach().clone()
    return out


def _differing(a, b):
    assert set(a) == set(b)
    return {k: float((a[k].double() - b[k].double()).abs().max()) for k in a if not torch.equal(a[k], b[k])}


def _two_steps(g, mode):
    m, _ = _tiny(g, mode)
    snaps = _watch_steps(m)
    logs = [_step(m, _images(g["traj.imgs_u8"][b][:5]).cuda(), b, torch.from_numpy(g["traj.z"][b][:5]).cuda()) for b in range(2)]
    return logs, snaps, _state(m)


@pytest.mark.parametrize("mode", MODES)
def test_two_runs_are_bit_identical(kats, mode):
    """Logged scalars, the gradients handed to the optimizers, parameters, buffers and Adam moments."""
    la, ga, sa = _two_steps(kats, mode)
    lb, gb, sb = _two_steps(kats, mode)
    grads = [_differing(p, q) for p, q in zip(ga, gb)]
    assert la == lb and len(ga) == len(gb) == 4 and not any(grads) and not _differing(sa, sb), (la, lb, grads, _differing(sa, sb))
    assert int(sa["opt0.step"]) == 2 and int(sa["opt1.step"]) == 2


def test_checkpoint_resumes_bit_for_bit(kats):
    """Two batches, a checkpoint of the model and both optimizers, two more -- against a fresh model that loads the checkpoint."""
    g = kats
    x = [_images(g["traj.imgs_u8"][b]).cuda() for b in range(4)]
    z = [torch.from_numpy(g["traj.z"][b]).cuda() for b in range(4)]
    a, _ = _tiny(g)
    for b in (0, 1):
        _step(a, x[b], b, z[b])
    ck = copy.deepcopy({"model": a.state_dict(), "opts": [o.state_dict() for o in a.optimizers()]})
    la = [_step(a, x[b], b, z[b]) for b in (2, 3)]
    fresh = _model(seed=9, **_cfg(g)).cuda().train()
    fresh.load_state_dict({k: v.cpu() for k, v in ck["model"].items()})
    for o, sd in zip(fresh.optimizers(), ck["opts"]):
        o.load_state_dict(sd)
    lb = [_step(fresh, x[b], b, z[b]) for b in (2, 3)]
    assert la == lb
    diff = _differing(_state(a), _state(fresh))
    assert not diff, diff
    assert [int(_state(fresh)[f"opt{i}.step"]) for i in (0, 1)] == [4, 4]


def test_sample_validation_discriminator_and_cpu_input(kats):
    m, _ = _tiny(kats)
    y = m.sample(3)
    assert y.shape == (3, 1, 28, 28) and float(y.abs().max()) <= 1.0 and bool(torch.isfinite(y).all())
    x = _images(kats["tiny.imgs_u8"]).cuda()
    z = torch.from_numpy(kats["tiny.vanilla.z"]).cuda()
    m.eval()
    res = m.validation_step((x, torch.arange(5)), 0)
    assert res.fake_image.shape == res.recon_image.shape == res.real_image.shape == (5, 1, 28, 28) and res.encode_latent.shape == (5, 6)
    _close(res.recon_image, m(res.encode_latent), 1e-5, "recon = decoder(encoder(img))")
    # Discriminator.forward: logits without a graph in evaluation mode, one row alone included; no buffer moves
    before = {k: v.clone() for k, v in m.discriminator.state_dict().items()}
    logit = m.discriminator(x, z)
    assert logit.shape == (5, 1) and not logit.requires_grad and bool(torch.isfinite(logit).all())
    _close(m.discriminator(x[:1], z[:1]), logit[:1], 1e-5, "one pair alone")
    assert all(torch.equal(v, before[k]) for k, v in m.discriminator.state_dict().items())
    with pytest.raises(RuntimeError):
        m.discriminator(x.cpu(), z)                                                    # a CPU tensor
    m.train()
    with pytest.raises(NotImplementedError):
        m.discriminator(x, z)                                                          # the inference path is evaluation mode's
    with pytest.raises(RuntimeError):
        m.training_step((x.cpu(), None), 0)                                            # a CPU batch
    with pytest.raises(RuntimeError):
        m.training_step((x, None), 0, z=z.cpu())                                       # a CPU draw
    with pytest.raises(RuntimeError):
        m.training_step((x, None), 0, z=torch.zeros(5, 7, device="cuda"))              # a draw of the wrong width
    logged = {}
    m.log = lambda k, v, *a, **kw: logged.__setitem__(k, v)
    m.training_step((x, None), 0)                                                      # its own draw
    assert all(math.isfinite(float(v)) for v in logged.values()) and set(logged) == set(M.LOGS)
