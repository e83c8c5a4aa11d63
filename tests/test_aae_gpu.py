"""AAE path (`experiment=aae/mnist`) on the HIP kernels against the reference's vectors (tests/golden/aae_kats.npz, produced by the
reference's own AAE.training_step: tools/gen_golden_aae.py).  Tolerances are those of tests/test_factor_vae_gpu.py."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
M = importlib.import_module("image-generation-models_amd.src.models.aae")
LOGS = ("train_loss/recon_loss", "train_loss/d_loss", "train_log/real_logit", "train_log/fake_logit", "train_loss/adv_encoder_loss")
ENC = {"_target_": "src.networks.basic.ConvEncoder", "norm_type": "batch"}
DEC = {"_target_": "src.networks.basic.ConvDecoder", "norm_type": "batch"}
DM = {"width": 28, "height": 28, "channels": 1, "transforms": {"normalize": True}}
# BatchNorm running means whose layer sits behind a convolution WITH a bias.  Such a bias has an analytically zero gradient; what Adam
# gets is rounding noise, and its first update moves the bias by up to lr = 2e-4 in that noise's direction.  The encoder runs again after
# that update, so the noise lands in these running means with the weight 0.19: the reference's own float32 run of the `tiny` step leaves
# its float64 run by 1.8e-5 (network.3) and 6.6e-6 (network.6) there, against 1e-9 for every other running statistic and a bound of
# 1e-5 * max|ref| + 1e-5 = 1.07e-5; this path left the float32 reference by 3.4e-5 on an MI355X.  With 0.19 * bias taken out, the
# reference's two runs agree to 3e-9 and 7e-9.  test_tiny_training_step_matches_reference compares these two tensors that way.
BIAS_IN_FRONT = {"encoder.network.3.running_mean": "encoder.network.2.bias", "encoder.network.6.running_mean": "encoder.network.5.bias"}


def _model(nf, seed=None, **kw):
    if seed is not None:
        torch.manual_seed(seed)
    kw.setdefault("latent_dim", 8)
    return M.AAE(DM, encoder=dict(ENC, ndf=nf), decoder=dict(DEC, ngf=nf), netD=None, **kw)


def _images(u8):
    """tools/gen_golden_aae.py::decode_images"""
    return torch.from_numpy(u8.astype(np.float32) / np.float32(127.5) - np.float32(1))


def _close(a, b, rel, what=""):
    """tests/test_vae_gpu.py::_close"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= rel * scale + 1e-5, f"{what}: max err {err:.3e} > {rel} * max |ref| ({scale:.3e}) + 1e-5"   # 1e-5: biases in front of a batch norm have zero gradient up to rounding


@pytest.fixture(scope="module")
def kats(golden_dir):
    return np.load(os.path.join(golden_dir, "aae_kats.npz"))


def _tiny(g, **kw):
    m = _model(4, **kw)
    sd = {k[len("tiny.sd0."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("tiny.sd0.")}
    assert list(m.state_dict().keys()) == list(sd.keys())
    m.load_state_dict(sd)
    return m.cuda().train(), sd


def _watch_steps(m):
    """The gradients handed to each of the three optimizer steps, snapshotted by wrapping `step` like the generator does: the nets an
    optimizer steps are its `nets`, or the ones named in the call."""
    snaps = []
    names = {id(n): k for k, n in (("encoder", m.encoder), ("decoder", m.decoder), ("discriminator", m.discriminator))}
    for opt in m.optimizers():
        def step(*a, _inner=opt.step, _opt=opt, **k):
            snap = {}
            for n in (k.get("nets") or _opt.nets):
                for key, p in n.named_parameters():
                    snap[f"{names[id(n)]}.{key}"] = p.grad.detach().clone()
            snaps.append(snap)
            out = _inner(*a, **k)
            if len(snaps) == 1:                                                        # the encoder as the discriminator phase will run it
                snap["after"] = {"encoder." + key: v.detach().clone() for key, v in m.encoder.state_dict().items()}
            return out
        opt.step = step
    return snaps


def _step(m, g, tag, i=None):
    pick = (lambda a: a) if i is None else (lambda a: a[i])
    logged = {}
    m.log = lambda k, v, *a, **kw: logged.__setitem__(k, v)
    x = _images(pick(g[f"{tag}.imgs_u8"])).cuda()
    out = m.training_step((x, None), 0, prior=torch.from_numpy(pick(g[f"{tag}.prior"])).cuda())
    assert out is None                                                                 # manual optimization: like the reference
    assert all(torch.is_tensor(v) and v.is_cuda for v in logged.values())              # logged scalars stay on the device
    return {k: float(v) for k, v in logged.items()}


def _check_logs(logged, g, tag):
    assert set(logged) == set(LOGS)
    for key in LOGS:
        ref = float(g[f"{tag}.log." + key])
        print(f"{key}: {logged[key]:.8g} reference {ref:.8g}")
        assert abs(logged[key] - ref) <= 1e-5 * abs(ref) + 1e-6, key


def test_tiny_training_step_matches_reference(kats):
    g = kats
    m, sd0 = _tiny(g, recon_weight=float(g["tiny.recon_weight"]))
    snaps = _watch_steps(m)
    _check_logs(_step(m, g, "tiny"), g, "tiny")
    # the three per-phase gradient snapshots: encoder + decoder, discriminator, encoder alone
    assert len(snaps) == 3
    after1 = snaps[0].pop("after")
    for i, snap in enumerate(snaps, 1):
        assert sorted(snap) == sorted(g[f"tiny.gnames{i}"]), i
        for k, gr in snap.items():
            _close(gr, torch.from_numpy(g[f"tiny.grad{i}.{k}"]), 2e-4, f"phase {i} {k}")
    # the state after the step.  One Adam update moves a weight by about lr * g / (|g| + 1e-8): an error dg of the gradient moves it by at
    # most lr * dg / (|g| + 1e-8), and never by more than 2 lr (tests/test_factor_vae_gpu.py).  dg is the gradient tolerance above.  The
    # decoder and the discriminator take that one update.  The encoder takes a second one, from the gradients g1 and g3 of phases 1 and
    # 3: u = lr * mhat / sqrt(vhat) with mhat = (0.25 g1 + 0.5 g3) / 0.75 and vhat = (0.999 g1^2 + g3^2) / 1.999 (betas 0.5, 0.999), so
    # |mhat| / sqrt(vhat) <= sqrt(0.111 / 0.4997 + 0.444 / 0.5003) = 1.054 (Cauchy-Schwarz) and, with s = sqrt(vhat) >= 0.707 max(|g1|, |g3|),
    # |du/dg3| <= lr / s * (0.667 + 1.054 * 1.414 / 1.999) = 1.41 lr / s and |du/dg1| <= lr / s * (0.333 + 0.745) = 1.08 lr / s: the second
    # update moves by at most 2 lr (dg1 + dg3) / max(|g1|, |g3|), and never by more than 2 * 1.054 lr.
    sd1 = m.state_dict()
    lr = 2e-4
    dg_of = lambda gref: 2e-4 * float(gref.abs().max()) + 1e-5                          # noqa: E731
    for k in sd0:
        if k.endswith("num_batches_tracked"):
            want = 3 if k.startswith("encoder.") else 1
            assert int(sd1[k]) == int(g["tiny.sd1." + k]) == want, k
            continue
        ref = torch.from_numpy(g["tiny.sd1." + k]).double() if "tiny.sd1." + k in g.files else sd0[k].double() + torch.from_numpy(g["tiny.dsd1." + k]).double()
        got = sd1[k].detach().double().cpu()
        if "running_" in k:
            if k in BIAS_IN_FRONT:
                # r = 0.729 r0 + 0.081 (s_a + b0) + 0.19 (s_b + b1): the batch mean is the bias-free mean s plus the bias, and b1, the bias after
                # the first optimizer step, is b0 moved by Adam along a gradient that is pure rounding noise (|g1| <= 1e-8 here) -- up to lr in
                # a direction no two float32 evaluations share.  0.19 b1 is taken out on both sides: ours as it stood after that step, the
                # reference's from its stored gradient by Adam's first update, b0 - lr g1 / (|g1| + 1e-8).  The bound stays.
                b = BIAS_IN_FRONT[k]
                g1 = torch.from_numpy(g["tiny.grad1." + b]).double()
                b1_ref = sd0[b].double() - lr * g1 / (g1.abs() + 1e-8)
                scale = float(ref.abs().max())                                         # of the running mean itself, as in _close
                got, ref = got - 0.19 * after1[b].double().cpu(), ref - 0.19 * b1_ref
                err = float((got - ref).abs().max())
                print(f"{k} without 0.19 * bias: max err {err:.3e}, bound {1e-5 * scale + 1e-5:.3e}")
                assert err <= 1e-5 * scale + 1e-5, (k, err)
                continue
            _close(got, ref, 1e-5, k)
            continue
        phases = [i for i in (1, 2, 3) if f"tiny.grad{i}.{k}" in g.files]
        assert phases == ([1, 3] if k.startswith("encoder.") else [1] if k.startswith("decoder.") else [2]), k
        g1 = torch.from_numpy(g[f"tiny.grad{phases[0]}.{k}"]).double()
        tol = torch.clamp(lr * dg_of(g1) / (g1.abs() + 1e-8), max=2 * lr) + 2e-7 * float(ref.abs().max())
        if len(phases) == 2:
            g3 = torch.from_numpy(g[f"tiny.grad3.{k}"]).double()
            tol = tol + torch.clamp(2 * lr * (dg_of(g1) + dg_of(g3)) / (torch.maximum(g1.abs(), g3.abs()) + 1e-8), max=2.11 * lr)
        bad = (got - ref).abs() > tol
        assert not bool(bad.any()), (k, int(bad.sum()), float((got - ref).abs().max()))
        moved = float((got - sd0[k].double()).abs().max())
        assert moved > 0, k                                                            # every tensor moved
        assert moved <= (2.06 if len(phases) == 2 else 1.0) * lr + 1e-7, (k, moved)     # by one Adam update (lr), the encoder by two (+ 1.054 lr)
    opt_g, opt_d = m.optimizers()
    assert opt_g.step_counts() == [2, 1] and opt_d.device_step_count() == 1            # encoder, decoder; discriminator


def test_cfg_training_step_matches_reference(kats):
    """configs/experiment/aae/mnist.yaml sizes, weights from the same seeded default init."""
    g = kats
    m = _model(32, seed=32).cuda().train()
    snaps = _watch_steps(m)
    _check_logs(_step(m, g, "cfg"), g, "cfg")
    for i, snap in enumerate(snaps, 1):
        for k, ref in zip(list(g[f"cfg.gnames{i}"]), g[f"cfg.gstats{i}"]):
            assert abs(float(snap[k].double().norm()) - ref[1]) <= 2e-4 * ref[1] + 1e-5, (i, k)
    sd = m.state_dict()
    assert int(sd["encoder.network.3.num_batches_tracked"]) == 3 and int(sd["decoder.network.1.num_batches_tracked"]) == 1


@pytest.fixture(scope="module")
def traj(kats):
    """The tiny model for 3 steps on the fixture's images and priors: run once, read by two tests."""
    g = kats
    m, _ = _tiny(g, lrG=float(g["traj.lrG"]), lrD=float(g["traj.lrD"]))
    logs = [_step(m, g, "traj", i) for i in range(3)]
    sd = m.state_dict()
    return (np.array([[lg[k] for k in LOGS] for lg in logs]), sd["discriminator.classifier.fc.weight"].detach().double().cpu().numpy().copy(),
            sd["encoder.network.0.weight"].detach().double().cpu().numpy().copy())


def test_trajectory_scalars_track_the_float64_reference(kats, traj):
    """Step by step and scalar by scalar: |hip - ref64| <= 4 |ref32 - ref64| + 1e-6 * scale, scale = |ref64| for the losses and the
    float64 run's max|logit| of that pass for the mean logits (a mean of signed logits can cancel).  16 images per step."""
    g = kats
    assert list(g["traj.log_keys"]) == list(LOGS)
    logs = traj[0]
    ref64, ref32, mx = g["traj.logs64"], g["traj.logs32"], g["traj.max_logit64"]
    worst = []
    for i in range(3):
        for j, key in enumerate(LOGS):
            scale = {"train_log/real_logit": mx[i, 0], "train_log/fake_logit": mx[i, 1]}.get(key, abs(ref64[i, j]))
            tol = 4.0 * abs(ref32[i, j] - ref64[i, j]) + 1e-6 * scale
            err = abs(logs[i, j] - ref64[i, j])
            print(f"step {i} {key}: {logs[i, j]:.8g} float64 reference {ref64[i, j]:.8g} deviation {err:.3e} tolerance {tol:.3e}")
            if err > tol:
                worst.append((i, key, err, tol))
    assert not worst, worst


def test_trajectory_weights_track_the_float64_reference(kats, traj):
    g = kats
    for name, got, r32, r64 in (("discriminator.classifier.fc.weight", traj[1], g["traj.dw32"], g["traj.dw64"]),
                                ("encoder.network.0.weight", traj[2], g["traj.ew32"], g["traj.ew64"])):
        tol = 4.0 * float(np.abs(r32 - r64).max()) + 1e-6 * float(np.abs(r64).max())
        err = float(np.abs(got - r64).max())
        print(f"{name} after 3 steps: max abs deviation from the float64 reference {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, (name, err, tol)


def test_double_batchnorm_update_equals_two_forwards():
    """ConvEncoder.forward_nhwc(bn_updates=2) leaves the running statistics where two forwards of the same batch leave them."""
    from src.ops import functional as K
    a, b = _model(4, seed=3).encoder.cuda().train(), _model(4, seed=3).encoder.cuda().train()
    x = K.nchw_to_nhwc(torch.rand(5, 1, 28, 28, device="cuda") * 2 - 1)
    ya, _ = a.forward_nhwc(x, bn_updates=2)
    b.forward_nhwc(x)
    yb, _ = b.forward_nhwc(x)
    assert float((ya - yb).abs().max()) <= 1e-5 * float(yb.abs().max())             # up to the order of the last layer's split-K sums
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        if k.endswith("num_batches_tracked"):
            assert int(sa[k]) == int(sb[k]) == 2
        elif "running_" in k:
            assert float((sa[k] - sb[k]).abs().max()) <= 1e-6 * float(sb[k].abs().max()), k
            assert float((sb[k] - (0.0 if "mean" in k else 1.0)).abs().max()) > 0


def test_default_draws_at_eight_rows_and_at_one():
    m = _model(4, seed=5).cuda().train()
    logged = {}
    m.log = lambda k, v, *a, **kw: logged.__setitem__(k, v)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    m.training_step((torch.rand(8, 1, 28, 28, device="cuda") * 2 - 1, None), 0)
    assert set(logged) == set(LOGS) and all(math.isfinite(float(v)) for v in logged.values())
    after = m.state_dict()
    assert int(after["encoder.network.3.num_batches_tracked"]) == 3 and int(after["decoder.network.4.num_batches_tracked"]) == 1
    for k in ("encoder.network.0.weight", "decoder.network.9.weight", "discriminator.model.1.fc.weight", "discriminator.classifier.fc.bias"):
        assert float((after[k] - before[k]).abs().max()) > 0 and bool(torch.isfinite(after[k]).all()), k
    assert m.sample_prior(3).shape == (3, 8) and m.sample_prior(3).is_cuda
    # N = 1: the discriminator has no batch statistics, one row is a legal pass (the conv nets' BatchNorm wants more than one value per
    # channel, which a 28x28 image gives it at every layer but the 1x1 bottleneck -- which has no norm)
    D = m.discriminator
    rec = D.disc_forward(m.sample_prior(1), 1.0, x1=m.sample_prior(1), target1=0.0)
    D.disc_backward(rec, 1.0, 0.0, c0=0.5, c1=0.5)
    assert rec["logit"].shape == (2,) and math.isfinite(float(rec["d_loss"])) and bool(torch.isfinite(D.flat_grads).all())
    for loss_mode in ("vanilla", "lsgan"):
        m1 = _model(4, seed=6, loss_mode=loss_mode).cuda().train()
        logged.clear()
        m1.log = lambda k, v, *a, **kw: logged.__setitem__(k, v)
        m1.training_step((torch.rand(1, 1, 28, 28, device="cuda") * 2 - 1, None), 0)
        assert set(logged) == set(LOGS) and all(math.isfinite(float(v)) for v in logged.values()), loss_mode


def test_inference_surface():
    m = _model(4, seed=6).cuda().eval()
    x = torch.rand(4, 1, 28, 28, device="cuda") * 2 - 1
    z = m.sample_prior(4)
    assert m(z).shape == x.shape and m.sample(3).shape == (3, 1, 28, 28)
    res = m.validation_step((x, torch.zeros(4)), 0)
    assert res.encode_latent.shape == (4, 8) and res.fake_image.shape == x.shape and res.recon_image.shape == x.shape
    assert res.real_image is x and res.label.shape == (4,)
    assert float(res.recon_image.abs().max()) <= 1.0                                   # tanh output
    assert float((m(res.encode_latent) - res.recon_image).abs().max()) <= 1e-5         # forward(z) is the decoder
    logits = m.discriminator(z)
    assert logits.shape == (4, 1) and bool(torch.isfinite(logits).all())
    assert int(m.encoder._buffer("network.3.num_batches_tracked")) == 0                # evaluation mode: running statistics


def test_refusals():
    m = _model(4)
    with pytest.raises(RuntimeError):
        m.training_step((torch.rand(4, 1, 28, 28), None), 0)                           # a CPU batch
    m = m.cuda().train()
    x = torch.rand(4, 1, 28, 28, device="cuda")
    with pytest.raises(RuntimeError):
        m.training_step((x, None), 0, prior=torch.zeros(4, 8))                         # a CPU prior


def test_run_py_aae_end_to_end(tmp_path):
    """python run.py experiment=aae/synthetic: compose -> manual-optimization fit -> validate (sample grid) -> checkpoint with both
    optimizers' state."""
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-generation-models_amd")
    cmd = [sys.executable, os.path.join(pkg, "run.py"), "experiment=aae/synthetic", "datamodule.train_size=128", "datamodule.val_size=32",
           "datamodule.batch_size=32", "networks.encoder.ndf=8", "networks.decoder.ngf=8", "trainer.max_epochs=1", f"log_dir={tmp_path}",
           "seed=1", "print_config=False"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    run_dir = tmp_path / "runs" / "aae" / "synthetic"
    assert (run_dir / "results" / "0.jpg").exists()
    ck = torch.load(next((run_dir / "checkpoints").glob("*.ckpt")))
    sd = ck["state_dict"]
    assert {"decoder.network.0.weight", "encoder.network.8.bias", "discriminator.model.0.fc.weight", "discriminator.model.1.norm.weight",
            "discriminator.classifier.fc.bias"} <= set(sd)
    assert sd["discriminator.model.1.fc.weight"].shape == (256, 256) and sd["encoder.network.8.weight"].shape == (8, 32, 4, 4)
    assert int(sd["encoder.network.3.num_batches_tracked"]) == 12 and int(sd["decoder.network.1.num_batches_tracked"]) == 4   # 4 steps
    opt_g, opt_d = ck["optimizer_states"]
    assert [p["step"] for p in opt_g["parts"]] == [8, 4] and opt_d["step"] == 4        # encoder 2k, decoder k; discriminator k
    text = (run_dir / "tensorboard" / "metrics.jsonl").read_text()
    for key in ("train_loss/recon_loss", "train_loss/d_loss", "train_log/fake_logit", "train_loss/adv_encoder_loss"):
        assert key in text, key
