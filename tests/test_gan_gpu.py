"""GAN path (`experiment=vanilla_gan/mnist_conv`, `lsgan/conv_mnist`, `ggan/mnist_conv`) on the HIP kernels against the reference's
vectors (tests/golden/gan_kats.npz, produced by the reference's own GAN.training_step: tools/gen_golden_gan.py).  `_close` and the
tolerances are those of tests/test_aae_gpu.py; the trajectory's comparisons are tests/_gan_golden.py's, which tests/test_gan_cpu.py
shows the reference's own float32 run to meet."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gan_golden as GG  # noqa: E402

pytestmark = pytest.mark.gpu
M = importlib.import_module("image-generation-models_amd.src.models.gan")
NETD = {"_target_": "src.networks.basic.ConvEncoder", "norm_type": "batch"}
NETG = {"_target_": "src.networks.basic.ConvDecoder", "norm_type": "batch"}
DM = {"width": 28, "height": 28, "channels": 1, "transforms": {"normalize": True}}
LR = GG.LR


def _model(nf, seed=None, **kw):
    if seed is not None:
        torch.manual_seed(seed)
    kw.setdefault("latent_dim", 8)
    return M.GAN(DM, netG=dict(NETG, ngf=nf), netD=dict(NETD, ndf=nf), **kw)


def _images(u8):
    """tools/gen_golden_aae.py::decode_images"""
    return torch.from_numpy(u8.astype(np.float32) / np.float32(127.5) - np.float32(1))


def _close(a, b, rel, what=""):
    """tests/test_aae_gpu.py::_close"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= rel * scale + 1e-5, f"{what}: max err {err:.3e} > {rel} * max |ref| ({scale:.3e}) + 1e-5"


@pytest.fixture(scope="module")
def kats(golden_dir):
    return np.load(os.path.join(golden_dir, "gan_kats.npz"))


def _tiny(g, **kw):
    m = _model(4, **kw)
    sd = {k[len("tiny.sd0."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("tiny.sd0.")}
    assert list(m.state_dict().keys()) == list(sd.keys())
    m.load_state_dict(sd)
    return m.cuda().train(), sd


def _watch_steps(m):
    """The gradients handed to each optimizer step, snapshotted by wrapping `step` like the generator does."""
    snaps = []
    names = {id(m.netG): "netG", id(m.netD): "netD"}
    for opt in m.optimizers():
        def step(*a, _inner=opt.step, _opt=opt, **k):
            snaps.append({f"{names[id(n)]}.{key}": p.grad.detach().clone() for n in _opt.nets for key, p in n.named_parameters()})
            return _inner(*a, **k)
        opt.step = step
    return snaps


def _step(m, x, z, idx):
    logged = {}
    m.log = lambda k, v, *a, **kw: logged.__setitem__(k, v)
    out = m.training_step((x, None), idx, z=z)
    assert out is None                                                                 # manual optimization: like the reference
    assert all(torch.is_tensor(v) and v.is_cuda for v in logged.values())              # logged scalars stay on the device
    return {k: float(v) for k, v in logged.items()}


@pytest.mark.parametrize("phase", ("g", "d"))
@pytest.mark.parametrize("mode", GG.MODES)
def test_tiny_step_matches_reference(kats, mode, phase):
    g, tag = kats, f"tiny.{mode}.{phase}"
    m, sd0 = _tiny(g, loss_mode=mode)
    snaps = _watch_steps(m)
    logged = _step(m, _images(g["tiny.imgs_u8"]).cuda(), torch.from_numpy(g[f"{tag}.z"]).cuda(), 0 if phase == "g" else 1)
    keys = GG.G_LOGS if phase == "g" else GG.D_LOGS
    assert set(logged) == set(keys)
    for key in keys:                                                                    # tests/test_aae_gpu.py::_check_logs
        ref = float(g[f"{tag}.log.{key}"])
        print(f"{key}: {logged[key]:.8g} reference {ref:.8g}")
        assert abs(logged[key] - ref) <= 1e-5 * abs(ref) + 1e-6, key
    # the one optimizer step's gradients: the generator's in the generator phase, the discriminator's in the other
    assert len(snaps) == 1 and sorted(snaps[0]) == sorted(g[f"{tag}.gnames"])
    for k, gr in snaps[0].items():
        _close(gr, torch.from_numpy(g[f"{tag}.grad.{k}"]), 2e-4, f"{tag} {k}")
    # the state after the step.  One Adam update moves a weight by about lr * g / (|g| + 1e-8): an error dg of the gradient moves it by at
    # most lr * dg / (|g| + 1e-8), and never by more than 2 lr (tests/test_aae_gpu.py).  dg is the gradient tolerance above.
    sd1 = m.state_dict()
    stepped = "netG." if phase == "g" else "netD."
    dg_of = lambda gref: 2e-4 * float(gref.abs().max()) + 1e-5                          # noqa: E731
    for k in sd0:
        if k.endswith("num_batches_tracked"):
            want = 2 if (phase == "d" and k.startswith("netD.")) else 1                 # D saw two batches in its own phase
            assert int(sd1[k]) == int(g[f"{tag}.sd1.{k}"]) == want, k
            continue
        ref = (torch.from_numpy(g[f"{tag}.sd1.{k}"]).double() if f"{tag}.sd1.{k}" in g.files
               else sd0[k].double() + torch.from_numpy(g[f"{tag}.dsd1.{k}"]).double())
        got = sd1[k].detach().double().cpu()
        if "running_" in k:
            _close(got, ref, 1e-5, f"{tag} {k}")                                         # both nets ran forward in training mode
            assert float((got - sd0[k].double()).abs().max()) > 0, k
        elif not k.startswith(stepped):
            assert torch.equal(got, sd0[k].double()) and torch.equal(ref, sd0[k].double()), k     # the other net's Adam did not step
        else:
            g1 = torch.from_numpy(g[f"{tag}.grad.{k}"]).double()
            tol = torch.clamp(LR * dg_of(g1) / (g1.abs() + 1e-8), max=2 * LR) + 2e-7 * float(ref.abs().max())
            bad = (got - ref).abs() > tol
            assert not bool(bad.any()), (k, int(bad.sum()), float((got - ref).abs().max()))
            moved = float((got - sd0[k].double()).abs().max())
            assert 0 < moved <= LR + 1e-7, (k, moved)                                  # every tensor moved, by one Adam update
    opt_g, opt_d = m.optimizers()
    assert (opt_g.device_step_count(), opt_d.device_step_count()) == ((1, 0) if phase == "g" else (0, 1))


def test_trajectory_matches_the_float64_reference(kats):
    """G, D, G, D in vanilla mode from tiny.sd0 on the fixture's images and z."""
    g = kats
    m, _ = _tiny(g, lrG=float(g["traj.lrG"]), lrD=float(g["traj.lrD"]))
    logs, bias_after = [], {b: [] for b in GG.BIAS_IN_FRONT.values()}
    for i in range(GG.STEPS):
        logs.append(_step(m, _images(g["traj.imgs_u8"][i]).cuda(), torch.from_numpy(g["traj.z"][i]).cuda(), i))
        sd = m.state_dict()
        for b in bias_after:
            bias_after[b].append(sd[b].detach().double().cpu().numpy().copy())
    GG.check_traj_logs(g, logs, "hip")
    GG.check_traj_state(g, m.state_dict(), bias_after, "hip")


def _d_phase(D, x, K, segments):
    """The discriminator phase's D work on rows x = [real | fake]: one pass of 2 segments, or one pass per half, real first."""
    n = x.shape[0] // 2
    if segments == 2:
        out, tape = D.forward_nhwc(x, record=True, segments=2)
        _, _, dl = K.adv_loss(out, [True, False], "vanilla", scale=0.5)
        D.backward_nhwc(tape, dl)
        return out[:, 0, 0, 0].clone(), [t[2].clone() for t in tape[1:]], D.flat_grads.clone()
    outs, hs, grads = [], [], None
    dls = []
    for s, real in ((0, True), (1, False)):
        out, tape = D.forward_nhwc(x[s * n:(s + 1) * n], record=True)
        _, _, dl = K.adv_loss(out, [real], "vanilla", scale=0.5)
        dls.append((tape, dl))
        outs.append(out[:, 0, 0, 0].clone()); hs.append([t[2].clone() for t in tape[1:]])
    for tape, dl in dls:
        D.backward_nhwc(tape, dl)
        grads = D.flat_grads.clone() if grads is None else grads + D.flat_grads
    return torch.cat(outs), [torch.cat(p) for p in zip(*hs)], grads


def test_two_segments_equal_two_passes():
    """D on [real | fake] with segments=2 against the same model run on real, then on fake: every layer's output and the logits bit
    for bit, the running statistics bit for bit, the parameter gradients within the gradient tolerance."""
    from src.ops import functional as K
    a, b = _model(8, seed=3).netD.cuda().train(), _model(8, seed=3).netD.cuda().train()
    assert a.fused_norm_act and a.reproducible
    x = K.nchw_to_nhwc(torch.rand(14, 1, 28, 28, device="cuda") * 2 - 1)
    oa, ha, ga = _d_phase(a, x, K, 2)
    ob, hb, gb = _d_phase(b, x, K, 1)
    for i, (p, q) in enumerate(zip(ha, hb)):
        assert torch.equal(p, q), f"layer {i}"
    assert torch.equal(oa, ob)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        if "running_" in k or k.endswith("num_batches_tracked"):
            assert torch.equal(sa[k], sb[k]), k
    assert int(sa["network.3.num_batches_tracked"]) == 2
    _close(ga, gb, 2e-4, "flat gradients")
    assert float(gb.abs().max()) > 0


def _run_steps(g, mode):
    """A generator step and a discriminator step, each on a fresh model from tiny.sd0: per phase the logged scalars, the gradients
    handed to the optimizer and the state afterwards."""
    out = []
    for i, ph in enumerate(("g", "d")):
        m, _ = _tiny(g, loss_mode=mode)
        snaps = _watch_steps(m)
        logs = _step(m, _images(g["tiny.imgs_u8"]).cuda(), torch.from_numpy(g[f"tiny.{mode}.{ph}.z"]).cuda(), i)
        out.append((logs, snaps[0], {k: v.detach().clone() for k, v in m.state_dict().items()}))
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def _differing(a, b):
    """{key: max abs difference} of the tensors of two dicts that are not bit-equal."""
    return {k: float((a[k].double() - b[k].double()).abs().max()) for k in a if not torch.equal(a[k], b[k])}


@pytest.mark.parametrize("mode", ("vanilla", "hinge"))
def test_two_runs_of_a_step_are_bit_identical(kats, mode):
    """A generator step and a discriminator step, each twice from the same state: logged scalars, the gradients handed to the
    optimizer and the state afterwards.

    Every kernel of the step adds its partial sums in a fixed order: the segmented BatchNorm and the loss (csrc/bn_seg.hip), the
    discriminator's last layer off the split-K GEMM, and the weight and bias gradients through the slab mode of the generic
    weight-gradient kernel and the ordered column sum (FlatNet.reproducible, tests/test_wgrad_ordered_kernels_gpu.py)."""
    la, ga, sa = _run_steps(kats, mode)
    lb, gb, sb = _run_steps(kats, mode)
    grads = [_differing(p, q) for p, q in zip(ga, gb)]
    state = [_differing(p, q) for p, q in zip(sa, sb)]
    print(f"{mode}: logged scalars equal: {la == lb}; gradients that differ (generator step, discriminator step): {grads}; "
          f"state tensors that differ: {state}")
    assert la == lb
    assert not any(grads), grads
    assert not any(state), state


@pytest.mark.parametrize("mode", ("vanilla", "hinge"))
def test_two_runs_agree_bit_for_bit_in_scalars_buffers_and_affine_gradients(kats, mode):
    """What the segmented BatchNorm, the loss kernel and the forward and input-gradient convolutions decide: the logged scalars, every
    BatchNorm buffer and the BatchNorm layers' affine gradients (K.bn_seg_bwd's dgamma / dbeta) of two runs from the same state."""
    la, ga, sa = _run_steps(kats, mode)
    lb, gb, sb = _run_steps(kats, mode)
    assert la == lb
    norms = ("netG.network.1.", "netG.network.4.", "netG.network.7.", "netD.network.3.", "netD.network.6.")
    seen = 0
    for p, q in zip(ga, gb):
        for k in p:
            if k.startswith(norms):
                assert torch.equal(p[k], q[k]), k
                seen += 1
    assert seen == 2 * 5
    for p, q in zip(sa, sb):
        for k in p:
            if "running_" in k or k.endswith("num_batches_tracked"):
                assert torch.equal(p[k], q[k]), k


def test_sample_and_forward_in_eval_mode_use_the_running_statistics(kats):
    m, sd0 = _tiny(kats)
    z = torch.from_numpy(kats["tiny.vanilla.g.z"]).cuda()
    _step(m, _images(kats["tiny.imgs_u8"]).cuda(), z, 0)                                # running statistics away from their start
    m.eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        y1, y2 = m(z), m(z[:2])
    assert y1.shape == (5, 1, 28, 28) and float(y1.abs().max()) <= 1.0                  # tanh output
    _close(y2, y1[:2], 1e-6, "a sample's image does not depend on its batch")
    assert m.sample(3).shape == (3, 1, 28, 28)
    res = m.validation_step((torch.zeros(4, 1, 28, 28, device="cuda"), None), 0)
    assert res.fake_image.shape == (4, 1, 28, 28) and res.real_image.shape == (4, 1, 28, 28)
    after = m.state_dict()
    for k in before:
        assert torch.equal(before[k], after[k]), k                                     # nothing updated in evaluation mode
    # against torch on the same weights, BatchNorm in evaluation mode
    import torch.nn.functional as F
    sd = {k[len("netG."):]: v.detach().cpu().double() for k, v in after.items() if k.startswith("netG.")}
    h = z.cpu().double().reshape(5, 8, 1, 1)
    for i, (k, s, p) in enumerate(((4, 1, 0), (3, 2, 1), (4, 2, 1), (4, 2, 1))):
        h = F.conv_transpose2d(h, sd[f"network.{3 * i}.weight"], sd[f"network.{3 * i}.bias"], stride=s, padding=p)
        if i < 3:
            pre = f"network.{3 * i + 1}."
            h = F.relu(F.batch_norm(h, sd[pre + "running_mean"], sd[pre + "running_var"], sd[pre + "weight"], sd[pre + "bias"], False))
    _close(y1, torch.tanh(h), 1e-5, "eval-mode forward")
    m.train()
    with torch.no_grad():
        assert float((m(z) - y1).abs().max()) > 1e-4                                    # training mode: batch statistics


def test_default_path_of_the_vae_nets_is_unaffected():
    """ConvEncoder / ConvDecoder as the VAE, cVAE and AAE build them: one forward and backward of a seeded model with the new
    arguments left out against the same with them passed at their defaults."""
    from src.networks.basic import ConvDecoder, ConvEncoder
    from src.ops import functional as K

    def run(explicit):
        torch.manual_seed(11)
        e, d = ConvEncoder(1, 8, 4).cuda().train(), ConvDecoder(8, 1, 4).cuda().train()
        assert e.fused_norm_act is False and d.fused_norm_act is False
        x = K.nchw_to_nhwc(torch.rand(6, 1, 28, 28, device="cuda") * 2 - 1)
        q, te = e.forward_nhwc(x, record=True, bn_updates=1, segments=1) if explicit else e.forward_nhwc(x, record=True)
        y, td = d.forward_nhwc(q, record=True, segments=1) if explicit else d.forward_nhwc(q, record=True)
        assert all(len(t[1]) == 2 for t in td[1:4]) and te[1][1] is None               # the default tape: (mean, rstd) per norm layer
        dq = d.backward_nhwc(td, torch.ones_like(y) / y.numel(), need_dx=True)
        e.backward_nhwc(te, dq[..., :8], need_dx=False, param_grads=True) if explicit else e.backward_nhwc(te, dq[..., :8], need_dx=False)
        return q.clone(), y.clone(), e.flat_grads.clone(), d.flat_grads.clone(), e.state_dict(), d.state_dict()
    a, b = run(False), run(True)
    _close(a[0], b[0], 1e-5, "encoder output"); _close(a[1], b[1], 1e-5, "decoder output")
    _close(a[2], b[2], 2e-4, "encoder gradients"); _close(a[3], b[3], 2e-4, "decoder gradients")
    for sa, sb in ((a[4], b[4]), (a[5], b[5])):
        for k in sa:
            if "running_" in k or k.endswith("num_batches_tracked"):
                _close(sa[k].float(), sb[k].float(), 1e-5, k)


def test_default_draws_and_one_image():
    for mode in GG.MODES:
        m = _model(4, seed=5, loss_mode=mode, latent_dim=10).cuda().train()            # latent_dim % 4 != 0: z is repacked
        x = torch.rand(8, 1, 28, 28, device="cuda") * 2 - 1
        for idx in (0, 1):
            logged = {}
            m.log = lambda k, v, *a, **kw: logged.__setitem__(k, v)
            before = {k: v.clone() for k, v in m.state_dict().items()}
            m.training_step((x, None), idx)
            assert set(logged) == set(GG.G_LOGS if idx == 0 else GG.D_LOGS) and all(math.isfinite(float(v)) for v in logged.values())
            after = m.state_dict()
            moved, kept = ("netG.", "netD.") if idx == 0 else ("netD.", "netG.")
            assert float((after[moved + "network.0.weight"] - before[moved + "network.0.weight"]).abs().max()) > 0
            assert torch.equal(after[kept + "network.0.weight"], before[kept + "network.0.weight"])
        assert int(after["netD.network.3.num_batches_tracked"]) == 3 and int(after["netG.network.1.num_batches_tracked"]) == 2
    with pytest.raises(RuntimeError):
        m.training_step((x, None), 0, z=torch.zeros(8, 10))                            # a CPU z
    with pytest.raises(RuntimeError):
        m.training_step((x.cpu(), None), 1)                                            # a CPU batch


def test_run_py_gan_end_to_end(tmp_path):
    """python run.py experiment=vanilla_gan/synthetic: compose -> manual-optimization fit -> validate (sample grid) -> checkpoint."""
    import subprocess
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-generation-models_amd")
    cmd = [sys.executable, os.path.join(pkg, "run.py"), "experiment=vanilla_gan/synthetic", "datamodule.train_size=128", "datamodule.val_size=32",
           "datamodule.batch_size=32", "networks.encoder.ndf=8", "networks.decoder.ngf=8", "trainer.max_epochs=1", f"log_dir={tmp_path}",
           "seed=1", "print_config=False"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    run_dir = tmp_path / "runs" / "vanilla_gan" / "synthetic"
    assert (run_dir / "results" / "0.jpg").exists()
    ck = torch.load(next((run_dir / "checkpoints").glob("*.ckpt")))
    sd = ck["state_dict"]
    assert sd["netG.network.0.weight"].shape == (100, 32, 4, 4) and sd["netD.network.8.weight"].shape == (1, 32, 4, 4)
    # 4 steps: G, D, G, D -- G runs forward in each, D once in a generator step and twice in a discriminator step
    assert int(sd["netG.network.1.num_batches_tracked"]) == 4 and int(sd["netD.network.3.num_batches_tracked"]) == 6
    opt_g, opt_d = ck["optimizer_states"]
    assert opt_g["step"] == 2 and opt_d["step"] == 2
    text = (run_dir / "tensorboard" / "metrics.jsonl").read_text()
    for key in GG.G_LOGS + GG.D_LOGS:
        assert key in text, key
