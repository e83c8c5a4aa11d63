"""AGE path (`experiment=age/mnist`) on the HIP kernels against the reference's vectors (tests/golden/age_kats.npz, produced by the
reference's own AGE.training_step: tools/gen_golden_age.py).  The single-step tolerances are those of tests/test_gan_gpu.py and
tests/test_infogan_gpu.py for the same nets: a logged scalar within 1e-5 |ref| + 1e-6, a gradient handed to the optimizer within
2e-4 max|ref| + 1e-5, a running statistic within 1e-5 max|ref| + 1e-5, a stepped parameter within their first-Adam-step bound.  The
trajectory's final state is held to 4 x the gap between the reference's own float32 and float64 runs, tensor by tensor.

A conv bias in front of a BatchNorm has an analytically zero gradient: what the reference records for it is the rounding noise of its
own float32 backward, and the `+ 1e-5` of the gradient bound is there for that noise (tests/test_aae_gpu.py::_close says so).  The noise
is proportional to the gradient that flows through the layer, and the AGE multiplies its code terms by up to 1000, where those files'
losses carry weights of order 1: the recorded noise reaches 4e-4 here, and two float32 evaluations share none of it.  For these five
biases (ZERO_GRAD_BIAS) the reference's recorded noise is the yardstick: this path's value, and its difference to the record, each
stay within 4 max|ref| + 1e-5 -- the factor 4 over the reference's own error that the kernel tests use, the floor of those files.
Their Adam bound uses that gradient tolerance too (it sits at its clamp of 2 lr: such a gradient has no defined sign)."""
import copy
import importlib
import json
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
M = importlib.import_module("image-generation-models_amd.src.models.age")
ENC = {"_target_": "src.networks.basic.ConvEncoder", "norm_type": "batch"}
DEC = {"_target_": "src.networks.basic.ConvDecoder", "norm_type": "batch"}
DM = {"width": 28, "height": 28, "channels": 1, "transforms": {"normalize": True}}
SETS = ("mnist", "default", "cosine", "nonorm")
WEIGHTS = ("e_recon_x_weight", "e_recon_z_weight", "g_recon_x_weight", "g_recon_z_weight")
LRS = {"encoder.": 2e-3, "decoder.": 7e-4}
ZERO_GRAD_BIAS = ("decoder.network.0.bias", "decoder.network.3.bias", "decoder.network.6.bias", "encoder.network.2.bias", "encoder.network.5.bias")

def _model(nf=4, seed=None, **kw):
    if seed is not None:
        torch.manual_seed(seed)
    return M.AGE(DM, encoder=dict(ENC, ndf=nf), decoder=dict(DEC, ngf=nf), **{"latent_dim": 6, "lrE": 2e-3, "lrG": 7e-4, "drop_lr_epoch": 30, **kw})


def _images(u8):
    """tools/gen_golden_aae.py::decode_images"""
    return torch.from_numpy(u8.astype(np.float32) / np.float32(127.5) - np.float32(1))


def _close(a, b, rel, what=""):
    """tests/test_gan_gpu.py::_close"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= rel * scale + 1e-5, f"{what}: max err {err:.3e} > {rel} * max |ref| ({scale:.3e}) + 1e-5"


@pytest.fixture(scope="module")
def kats(golden_dir):
    return np.load(os.path.join(golden_dir, "age_kats.npz"))


def _weights(g, name):
    kw = {k: float(g[f"tiny.cfg.{name}.{k}"]) for k in WEIGHTS}
    kw["norm_z"] = bool(g[f"tiny.cfg.{name}.norm_z"])
    return kw


def _tiny(g, name="mnist", **kw):
    m = _model(4, **{**_weights(g, name), **kw})
    sd = {k[len("tiny.sd0."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("tiny.sd0.")}
    assert list(m.state_dict().keys()) == list(sd.keys())
    m.load_state_dict(sd)
    return m.cuda().train(), sd


def _watch_steps(m):
    """The gradients handed to each optimizer step, snapshotted by wrapping `step` like the generator does."""
    snaps = []
    names = {id(m.encoder): "encoder", id(m.decoder): "decoder"}
    for opt in m.optimizers():
        def step(*a, _inner=opt.step, _opt=opt, **k):
            snaps.append({f"{names[id(n)]}.{key}": p.grad.detach().clone() for n in _opt.nets for key, p in n.named_parameters()})
            return _inner(*a, **k)
        opt.step = step
    return snaps


def _step(m, x, b, z):
    logged = {}
    m.log = lambda k, v, *a, **kw: logged.__setitem__(k, v)
    out = m.training_step((x, None), b, z=z)
    assert out is None                                                                 # manual optimization
    assert all(torch.is_tensor(v) and v.is_cuda for v in logged.values())              # logged scalars stay on the device
    return {k: float(v) for k, v in logged.items()}


def _log_keys(ph, w):
    if ph == "G":
        return M.G_LOGS
    return M.E_LOGS + (("train_loss/recon_x",) if w["e_recon_x_weight"] > 0 else ())


@pytest.mark.parametrize("ph", ("E", "G"))
@pytest.mark.parametrize("name", SETS)
def test_tiny_phase_matches_reference(kats, name, ph):
    g, tag = kats, f"tiny.{name}.{ph}"
    m, sd0 = _tiny(g, name)
    snaps = _watch_steps(m)
    logged = _step(m, _images(g["tiny.imgs_u8"]).cuda(), 0 if ph == "E" else 1, torch.from_numpy(g[f"{tag}.z"]).cuda())
    keys = _log_keys(ph, _weights(g, name))
    assert set(logged) == set(keys)
    for key in keys:                                                                    # tests/test_gan_gpu.py's bound for a logged scalar
        ref = float(g[f"{tag}.log.{key}"])
        print(f"{key}: {logged[key]:.8g} reference {ref:.8g}")
        assert abs(logged[key] - ref) <= 1e-5 * abs(ref) + 1e-6, key
    # the one optimizer step's gradients: the encoder's in its phase, the decoder's in its own
    stepped = "encoder." if ph == "E" else "decoder."
    assert len(snaps) == 1 and sorted(snaps[0]) == sorted(g[f"{tag}.gnames"]) and all(k.startswith(stepped) for k in snaps[0])
    def dg_of(k):
        """The gradient tolerance of parameter k: 2e-4 max|ref| + 1e-5; for a zero-gradient bias 4 max|ref| + 1e-5 (the docstring)."""
        return (4.0 if k in ZERO_GRAD_BIAS else 2e-4) * float(np.abs(g[f"{tag}.grad.{k}"]).max()) + 1e-5
    for k, gr in snaps[0].items():
        ref = torch.from_numpy(g[f"{tag}.grad.{k}"])
        got = gr.detach().float().cpu()
        err = float((got - ref).abs().max())
        print(f"{tag} grad {k}: max|hip| {float(got.abs().max()):.3e}, max|ref| {float(ref.abs().max()):.3e}, max err {err:.3e}, bound {dg_of(k):.3e}")
        assert err <= dg_of(k), (tag, k, err, dg_of(k))
        if k in ZERO_GRAD_BIAS:
            assert float(got.abs().max()) <= dg_of(k), (tag, k, float(got.abs().max()), dg_of(k))
    # the state after the step: one Adam update at the net's own learning rate (tests/test_gan_gpu.py's derivation)
    sd1 = m.state_dict()
    lr = LRS[stepped]
    for k in sd0:
        if k.endswith("num_batches_tracked"):
            assert int(sd1[k]) == int(g[f"{tag}.sd1.{k}"]) >= 1, k
            continue
        ref = (torch.from_numpy(g[f"{tag}.sd1.{k}"]).double() if f"{tag}.sd1.{k}" in g.files
               else sd0[k].double() + torch.from_numpy(g[f"{tag}.dsd1.{k}"]).double())
        got = sd1[k].detach().double().cpu()
        if "running_" in k:
            _close(got, ref, 1e-5, f"{tag} {k}")                                         # both nets ran forward in training mode
            assert float((got - sd0[k].double()).abs().max()) > 0, k
        elif not k.startswith(stepped):
            assert torch.equal(got, sd0[k].double()) and torch.equal(ref, sd0[k].double()), k     # the other optimizer did not step
        else:
            g1 = torch.from_numpy(g[f"{tag}.grad.{k}"]).double()
            tol = torch.clamp(lr * dg_of(k) / (g1.abs() + 1e-8), max=2 * lr) + 2e-7 * float(ref.abs().max())
            bad = (got - ref).abs() > tol
            assert not bool(bad.any()), (k, int(bad.sum()), float((got - ref).abs().max()))
            moved = float((got - sd0[k].double()).abs().max())
            assert 0 < moved <= lr + 1e-7, (k, moved)                                  # every tensor moved, by one Adam update
    opt_e, opt_g = m.optimizers()
    assert (opt_e.device_step_count(), opt_g.device_step_count()) == ((1, 0) if ph == "E" else (0, 1))


def test_trajectory_matches_the_float64_reference(kats):
    """6 batches (E, G, G, E, G, G) from tiny.sd0 on the fixture's images and draws at lrE = 2e-3, lrG = 7e-4, against the reference's
    float64 run: every tensor of the final state within 4 x the reference's own float32-to-float64 gap for that tensor."""
    g = kats
    m, _ = _tiny(g, "mnist", lrE=float(g["traj.lrE"]), lrG=float(g["traj.lrG"]))
    w = _weights(g, "mnist")
    for b in range(6):
        logs = _step(m, _images(g["traj.imgs_u8"][b]).cuda(), b, torch.from_numpy(g["traj.z"][b]).cuda())
        ph = str(g["traj.phases"][b])
        assert m.phase(b) == ph and set(logs) == set(_log_keys(ph, w))
        for key, val in logs.items():                                                   # tests/_gan_golden.py::check_traj_logs' bound
            ref = float(g[f"traj.log64.{b}.{key}"])
            print(f"batch {b} {key}: {val:.8g} float64 reference {ref:.8g} (its float32 run {float(g[f'traj.log32.{b}.{key}']):.8g})")
            assert abs(val - ref) <= 1e-5 * abs(ref) + 1e-6, (b, key)
    sd, over = m.state_dict(), []
    for k in g["tiny.names"]:
        k = str(k)
        ref64, ref32 = g[f"traj.sd64.{k}"].astype(np.float64), g[f"traj.sd32.{k}"].astype(np.float64)
        got = sd[k].detach().double().cpu().numpy()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(ref64) == 8, k
            continue
        gap, err = float(np.abs(ref32 - ref64).max()), float(np.abs(got - ref64).max())
        print(f"{k}: max|hip - f64| {err:.3e}, the reference's max|f32 - f64| {gap:.3e}")
        if err > 4 * gap:
            over.append((k, err, gap))
    assert not over, over


@pytest.mark.parametrize("ph", ("E", "G"))
def test_frozen_net_keeps_its_bits_and_moves_its_running_statistics(kats, ph):
    g = kats
    m, _ = _tiny(g, "cosine")                                                           # every term: both nets run twice in either phase
    x, z = _images(g["tiny.imgs_u8"]).cuda(), torch.from_numpy(g["tiny.cosine.E.z"]).cuda()
    for b in (0, 1, 2):                                                                 # both optimizers have state by now
        _step(m, x, b, z)
    frozen, opt = (m.decoder, m.optimizers()[1]) if ph == "E" else (m.encoder, m.optimizers()[0])
    before = {k: v.detach().clone() for k, v in frozen.state_dict().items()}
    grads, moments = frozen.flat_grads.clone(), [t.clone() for t in opt._m + opt._v]
    count = opt.device_step_count()
    _step(m, x, 3 if ph == "E" else 4, z)
    after = frozen.state_dict()
    for k, v in before.items():
        if "running_" in k:
            assert not torch.equal(after[k], v), k
        elif k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(v) + 2, k
        else:
            assert torch.equal(after[k], v), k
    assert torch.equal(frozen.flat_grads, grads) and opt.device_step_count() == count
    assert all(torch.equal(a, b) for a, b in zip(opt._m + opt._v, moments))


def _state(m):
    out = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for i, opt in enumerate(m.optimizers()):
        sd = opt.state_dict()
        out[f"opt{i}.step"] = torch.tensor(sd["step"])
        out[f"opt{i}.lr"] = torch.tensor(sd["param_groups"][0]["lr"], dtype=torch.float64)
        for name in ("m", "v"):
            for j, t in enumerate(sd[name] or []):
                out[f"opt{i}.{name}{j}"] = t.detach().clone()
    return out


def _differing(a, b):
    assert set(a) == set(b)
    return {k: float((a[k].double() - b[k].double()).abs().max()) for k in a if not torch.equal(a[k], b[k])}


def _cycle(g, name):
    m, _ = _tiny(g, name)
    snaps = _watch_steps(m)
    logs = [_step(m, _images(g["traj.imgs_u8"][b][:5]).cuda(), b, torch.from_numpy(g["traj.z"][b][:5]).cuda()) for b in range(3)]
    return logs, snaps, _state(m)


@pytest.mark.parametrize("name", ("mnist", "cosine"))
def test_two_runs_of_a_cycle_are_bit_identical(kats, name):
    """Logged scalars, the gradients handed to the optimizers, parameters, buffers and Adam moments."""
    la, ga, sa = _cycle(kats, name)
    lb, gb, sb = _cycle(kats, name)
    grads = [_differing(p, q) for p, q in zip(ga, gb)]
    assert la == lb and len(ga) == 3 and not any(grads) and not _differing(sa, sb), (la, lb, grads, _differing(sa, sb))
    assert int(sa["opt0.step"]) == 1 and int(sa["opt1.step"]) == 2


def test_checkpoint_resumes_bit_for_bit(kats):
    """Two batches, an epoch end (drop_lr_epoch = 1: both learning rates halve), a checkpoint of the model, both optimizers and both
    schedulers, two more batches -- against a fresh model that loads the checkpoint and runs the last two."""
    g = kats
    x = [_images(g["traj.imgs_u8"][b]).cuda() for b in range(4)]
    z = [torch.from_numpy(g["traj.z"][b]).cuda() for b in range(4)]

    def epoch_end(m):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for s in m.lr_schedulers():
                s.step()
    a, _ = _tiny(g, "mnist", drop_lr_epoch=1)
    for b in (0, 1):
        _step(a, x[b], b, z[b])
    epoch_end(a)
    ck = copy.deepcopy({"model": a.state_dict(), "opts": [o.state_dict() for o in a.optimizers()],
                        "scheds": [s.state_dict() for s in a.lr_schedulers()]})
    la = [_step(a, x[b], b, z[b]) for b in (2, 3)]
    epoch_end(a)
    fresh = _model(4, seed=9, **{**_weights(g, "mnist"), "drop_lr_epoch": 1}).cuda().train()
    fresh.load_state_dict({k: v.cpu() for k, v in ck["model"].items()})
    for o, sd in zip(fresh.optimizers(), ck["opts"]):
        o.load_state_dict(sd)
    for s, sd in zip(fresh.lr_schedulers(), ck["scheds"]):
        s.load_state_dict(sd)
    assert [o.param_groups[0]["lr"] for o in fresh.optimizers()] == [1e-3, 3.5e-4]
    lb = [_step(fresh, x[b], b, z[b]) for b in (2, 3)]
    epoch_end(fresh)
    assert la == lb
    diff = _differing(_state(a), _state(fresh))
    assert not diff, diff
    assert [o.param_groups[0]["lr"] for o in fresh.optimizers()] == [5e-4, 1.75e-4]
    assert [int(_state(fresh)[f"opt{i}.step"]) for i in (0, 1)] == [2, 2]


def test_sample_encode_validation_and_cpu_input(kats):
    m, _ = _tiny(kats, "mnist")
    y = m.sample(3)
    assert y.shape == (3, 1, 28, 28) and float(y.abs().max()) <= 1.0 and bool(torch.isfinite(y).all())
    x = _images(kats["tiny.imgs_u8"]).cuda()
    m.eval()
    code = m.encode(x)
    assert code.shape == (5, 6) and float((code.double().pow(2).sum(dim=1) - 1).abs().max()) < 1e-6       # on the sphere
    kl, mu, var = m.calculate_kl(code, return_state=True)
    ref = code.double().cpu()
    want = float((ref.mean(0) ** 2 + ref.var(0) - torch.log(ref.var(0))).mean() / 2)
    assert abs(float(kl) - want) <= 1e-5 * abs(want) + 1e-6 and abs(float(var) - float(ref.var(0).mean())) <= 1e-6
    res = m.validation_step((x, None), 0)
    assert res.fake_image.shape == res.recon_image.shape == res.real_image.shape == (5, 1, 28, 28) and res.encode_latent.shape == (5, 6)
    assert torch.equal(res.encode_latent, code) and torch.equal(res.recon_image, m(code))
    m.train()
    with pytest.raises(RuntimeError):
        m.training_step((x.cpu(), None), 0)                                            # a CPU batch
    with pytest.raises(RuntimeError):
        m.training_step((x, None), 0, z=torch.zeros(5, 6))                             # a CPU draw
    with pytest.raises(RuntimeError):
        m.training_step((x, None), 0, z=torch.zeros(5, 7, device="cuda"))              # a draw of the wrong width
    logged = {}
    m.log = lambda k, v, *a, **kw: logged.__setitem__(k, v)
    m.training_step((x, None), 0)                                                      # its own draw
    assert all(math.isfinite(float(v)) for v in logged.values()) and len(logged) == 8


def test_run_py_age_end_to_end(tmp_path):
    """python run.py experiment=age/synthetic in a fresh child process: compose -> manual-optimization fit with the two epoch schedulers ->
    validate (sample and reconstruction grids) -> checkpoint; every logged loss finite."""
    import subprocess
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-generation-models_amd")
    cmd = [sys.executable, os.path.join(pkg, "run.py"), "experiment=age/synthetic", "datamodule.train_size=128", "datamodule.val_size=32",
           "datamodule.batch_size=32", "networks.encoder.ndf=8", "networks.decoder.ngf=8", "trainer.max_epochs=1", f"log_dir={tmp_path}",
           "seed=1", "print_config=False"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    run_dir = tmp_path / "runs" / "age" / "synthetic"
    assert (run_dir / "results" / "0.jpg").exists()
    ck = torch.load(next((run_dir / "checkpoints").glob("*.ckpt")))
    sd = ck["state_dict"]
    assert sd["decoder.network.0.weight"].shape == (10, 32, 4, 4) and sd["encoder.network.8.weight"].shape == (10, 32, 4, 4)
    opt_e, opt_g = ck["optimizer_states"]
    assert opt_e["step"] == 2 and opt_g["step"] == 2                                    # 4 batches: E, G, G, E
    assert opt_e["param_groups"][0]["lr"] == 2e-3 and opt_g["param_groups"][0]["lr"] == 7e-4
    assert int(sd["encoder.network.3.num_batches_tracked"]) == 6 and int(sd["decoder.network.1.num_batches_tracked"]) == 6
    seen = set()
    for line in (run_dir / "tensorboard" / "metrics.jsonl").read_text().splitlines():
        for k, v in json.loads(line).items():
            seen.add(k)
            assert math.isfinite(float(v)), (k, v)
    for key in M.E_LOGS + M.G_LOGS + ("train_loss/recon_x",):
        assert key in seen, key


def test_adam_with_host_complements_follows_torch():
    """K.adam_step(host_complements=True) (mi_adam_step_c) against Adam in float64 on the same float32 gradients, 4 steps at
    lr = 7e-4, betas (0.5, 0.999): within 4 updates x (lr x 2e-6, the rounding of a handful of float32 operations per update, + half
    an ulp of the parameter, which is rounded once per update).  The
    default path forms 1 - beta2 in fp32 and is off by lr x 2.3e-5 per update in the update's own direction (docs/kernels.md 4m)."""
    from src.ops import functional as K
    n, lr, b1, b2, eps = 4099, 7e-4, 0.5, 0.999, 1e-8                                   # an odd count: the tail past the last float4
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=gen) * 0.05
    grads = [torch.randn(n, generator=gen) * 10.0 ** float(torch.randint(-3, 2, (1,), generator=gen)) for _ in range(4)]
    ref, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t, g in enumerate(grads, 1):
        g = g.double()
        m64, v64 = m64 + (1 - b1) * (g - m64), b2 * v64 + (1 - b2) * g * g
        ref = ref - lr / (1 - b1 ** t) * m64 / (v64.sqrt() / math.sqrt(1 - b2 ** t) + eps)
    errs = {}
    for host in (True, False):
        buf = torch.zeros(4 * 4100, device="cuda")                                      # 16-byte aligned slices for the default kernel
        p, m, v, g = (buf[i * 4100:i * 4100 + n] for i in range(4))
        p.copy_(p0)
        for t, gr in enumerate(grads, 1):
            g.copy_(gr)
            K.adam_step(p, g, m, v, lr, b1, b2, eps, t, host_complements=host)
        errs[host] = float((p.double().cpu() - ref).abs().max())
    print(f"max|p - float64 Adam| after 4 steps: host complements {errs[True]:.3e}, device complements {errs[False]:.3e}")
    half_ulp = 2.0 ** -24 * (float(p0.abs().max()) + 4 * 1.2 * lr)
    assert errs[True] <= 4 * (lr * 2e-6 + half_ulp)
    assert errs[False] <= 4 * (lr * 5e-5 + half_ulp)
