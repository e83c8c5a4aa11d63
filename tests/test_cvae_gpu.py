"""cVAE path (`experiment=cvae/mnist`) on the HIP kernels against the reference's vectors (tests/golden/cvae_kats.npz, produced by the
reference's own cVAE.training_step: tools/gen_golden_cvae.py)."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
M = importlib.import_module("image-generation-models_amd.src.models.cvae")
DM = {"width": 28, "height": 28, "channels": 1, "transforms": {"normalize": True}}
LOGS = ("train_log/elbo", "train_log/kl_divergence", "train_log/log_p_x_of_z")


def _close(a, b, rel, what=""):
    """tests/test_vae_gpu.py::_close"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= rel * scale + 1e-5, f"{what}: max err {err:.3e} > {rel} * max |ref| ({scale:.3e}) + 1e-5"   # 1e-5: biases in front of a batch norm have zero gradient up to rounding


def _model(ndf, latent, seed=None, **kw):
    if seed is not None:
        torch.manual_seed(seed)
    kw.setdefault("n_classes", 10)
    return M.cVAE(DM, encoder={"_target_": "src.networks.basic.ConvEncoder", "ndf": ndf, "norm_type": "batch"},
                  decoder={"_target_": "src.networks.basic.ConvDecoder", "ngf": ndf, "norm_type": "batch"}, latent_dim=latent,
                  decoder_dist="gaussian", **kw)


@pytest.fixture(scope="module")
def kats(golden_dir):
    return np.load(os.path.join(golden_dir, "cvae_kats.npz"))


def _tiny(g):
    m = _model(8, 16)
    sd = {k[len("tiny.sd0."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("tiny.sd0.")}
    assert list(m.state_dict().keys()) == list(sd.keys())
    m.load_state_dict(sd)
    return m.cuda().train(), sd


def test_tiny_training_step_matches_reference(kats):
    g = kats
    m, _ = _tiny(g)
    logged = {}
    m.log = lambda k, v, *a, **kw: logged.__setitem__(k, float(v))
    batch = (torch.from_numpy(g["tiny.imgs"]).cuda(), torch.from_numpy(g["tiny.labels"]))          # labels arrive on the host
    loss = m.training_step(batch, 0, eps=torch.from_numpy(g["tiny.eps"]).cuda())
    loss.backward()
    assert abs(float(loss.detach()) - float(g["tiny.loss"])) <= 1e-5 * abs(float(g["tiny.loss"]))
    for key in LOGS:
        ref = float(g["tiny.log." + key])
        assert abs(logged[key] - ref) <= 1e-5 * abs(ref), key
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert "class_embedding.weight" in grads and list(grads) == list(g["tiny.pnames"])
    for k, gr in grads.items():
        _close(gr, torch.from_numpy(g["tiny.grad." + k]), 2e-4, k)
    eg = grads["class_embedding.weight"].cpu()
    assert float(eg[[1, 2, 4, 5, 6, 8]].abs().max()) == 0.0                   # labels [3, 7, 3, 0, 9, 3]: the other rows are exactly zero
    assert float(eg[[0, 3, 7, 9]].abs().amax(dim=1).min()) > 0
    sd1 = m.state_dict()
    for k in g.files:
        if k.startswith("tiny.buf1."):
            _close(sd1[k[len("tiny.buf1."):]].float(), torch.from_numpy(g[k]).float(), 1e-5, k)
    m.eval()
    with torch.no_grad():
        out = m(torch.from_numpy(g["tiny.zfix"]).cuda(), torch.from_numpy(g["tiny.labels_fix"]).cuda())
    _close(out, torch.from_numpy(g["tiny.decode_eval"]), 1e-4, "eval decode")


def test_cfg_training_step_matches_reference(kats):
    """configs/model/cvae.yaml + configs/networks/conv_mnist.yaml sizes, weights from the same seeded default init."""
    g = kats
    m = _model(32, 128, seed=32).cuda().train()
    m.log = lambda *a, **k: None
    batch = (torch.from_numpy(g["cfg.imgs"]).cuda(), torch.from_numpy(g["cfg.labels"]).cuda())
    loss = m.training_step(batch, 0, eps=torch.from_numpy(g["cfg.eps"]).cuda())
    loss.backward()
    assert abs(float(loss.detach()) - float(g["cfg.loss"])) <= 1e-5 * abs(float(g["cfg.loss"]))
    params = dict(m.named_parameters())
    for k, ref in zip(list(g["cfg.pnames"]), g["cfg.gstats"]):
        assert abs(float(params[k].grad.double().norm()) - ref[1]) <= 2e-4 * ref[1] + 1e-5, k
    m.eval()
    with torch.no_grad():
        out = m(torch.from_numpy(g["cfg.zfix"]).cuda(), torch.from_numpy(g["cfg.labels_fix"]).cuda())
    _close(out, torch.from_numpy(g["cfg.decode_eval"]), 1e-4, "eval decode")
    # optimizer + scheduler plumbing: ([FlatAdam over decoder, encoder, embedding], [StepLR])
    (opt,), (sch,) = m.configure_optimizers()
    assert opt.nets == [m.decoder, m.encoder, m.class_embedding]
    m.train()
    before = m.class_embedding.flat_params.clone()
    opt.step(); sch.step()
    assert abs(opt.param_groups[0]["lr"] - 1e-4 * 0.99) < 1e-12
    moved = float((m.class_embedding.flat_params - before).abs().max())
    assert 0 < moved <= 1.01e-4


@pytest.fixture(scope="module")
def traj(kats):
    """The tiny model for 3 Adam steps with StepLR between them on the fixture's images, labels and eps: run once, read by two tests."""
    g = kats
    m, sd0 = _tiny(g)
    m.log = lambda *a, **k: None
    m.hparams["lr"] = float(g["traj.lr"])
    (opt,), (sch,) = m.configure_optimizers()
    losses = []
    for x, lab, e in zip(g["traj.imgs"], g["traj.labels"], g["traj.eps"]):
        loss = m.training_step((torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()), 0, eps=torch.from_numpy(e).cuda())
        loss.backward()
        opt.step(); sch.step()
        losses.append(float(loss.detach()))
    return np.array(losses), m.state_dict()["class_embedding.weight"].detach().cpu().clone(), sd0["class_embedding.weight"].clone()


def test_trajectory_losses_track_the_float64_reference(kats, traj):
    """Measured (docs/kernels.md): the float32 reference deviates from its float64 run by 6.2e-9, 5.6e-8, 4.4e-8 relative at the three
    steps, so the floor of 1e-6 is the budget at every step; the HIP path measured the same three figures (its losses round to the
    float32 reference's)."""
    g = kats
    losses, _, _ = traj
    ref64, ref32 = g["traj.loss64"], g["traj.loss32"]
    for i in range(3):
        budget = max(4.0 * abs(ref32[i] - ref64[i]) / abs(ref64[i]), 1e-6)         # 4x the float32 reference's own deviation, floor 1e-6
        dev = abs(losses[i] - ref64[i]) / abs(ref64[i])
        print(f"step {i}: loss {losses[i]:.6f} float64 reference {ref64[i]:.6f} relative deviation {dev:.3e} budget {budget:.3e}")
        assert dev <= budget, (i, dev, budget)


def test_trajectory_embedding_table(kats, traj):
    g = kats
    _, emb, emb0 = traj
    never = [1, 2, 4, 5, 6, 8]                                                     # traj.labels holds 0, 3, 7, 9 only
    assert sorted(set(g["traj.labels"].reshape(-1).tolist())) == [0, 3, 7, 9]
    assert torch.equal(emb[never], emb0[never])                                    # Adam's moments are exactly zero there: bit-identical
    assert float((emb[[0, 3, 7, 9]] - emb0[[0, 3, 7, 9]]).abs().min()) > 0          # every seen entry moved
    tol = 4.0 * float(np.abs(g["traj.emb32"] - g["traj.emb64"]).max())              # the float32 reference's own deviation x 4
    err = float((emb.double() - torch.from_numpy(g["traj.emb64"])).abs().max())
    print(f"class_embedding.weight after 3 steps: max abs deviation from the float64 reference {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol, (err, tol)


def test_sample_is_class_major_and_conditioning_matters():
    m = _model(8, 16, seed=5).cuda().eval()
    torch.manual_seed(11)
    imgs = m.sample(3)
    assert imgs.shape == (30, 1, 28, 28)
    torch.manual_seed(11)
    z = torch.randn(30, 16)
    labels = torch.arange(10).repeat_interleave(3)
    assert labels[:6].tolist() == [0, 0, 0, 1, 1, 1]
    with torch.no_grad():
        assert torch.equal(imgs, m(z.cuda(), labels.cuda()))
        a, b = m(z.cuda(), torch.full((30,), 2).cuda()), m(z.cuda(), torch.full((30,), 7).cuda())
    assert float((a - b).abs().max()) > 1e-3                                       # same z, another class: another image


def test_encode_label_false_trains_on_the_plain_encoder_input():
    m = _model(8, 16, seed=6, encode_label=False).cuda().train()
    m.log = lambda *a, **k: None
    assert m.state_dict()["encoder.network.0.weight"].shape == (8, 1, 4, 4)
    x = torch.rand(4, 1, 28, 28, device="cuda") * 2 - 1
    loss = m.training_step((x, torch.tensor([1, 0, 9, 1])), 0)
    loss.backward()
    assert math.isfinite(float(loss.detach()))
    g = m.class_embedding.weight.grad
    assert float(g[[0, 1, 9]].abs().max()) > 0 and float(g[[2, 3, 4, 5, 6, 7, 8]].abs().max()) == 0.0
    assert float(dict(m.named_parameters())["encoder.network.0.weight"].grad.abs().max()) > 0


def test_graphed_cvae_step():
    """The cVAE step under hipGraph replay over the three flat buffers: kernel nodes only, fresh noise per replay, the loss goes down, the
    batch-norm counters advance inside the graph, and the labels are read from their static buffer at replay time."""
    G = importlib.import_module("image-generation-models_amd.src.runtime.graphed")
    OPT = importlib.import_module("image-generation-models_amd.src.runtime.optim")
    m = _model(32, 128, seed=3).cuda().train()
    m.log = lambda *a, **k: None
    opt = OPT.FlatAdam(m.flat_nets(), lr=1e-3, betas=(0.9, 0.999), device_state=True)
    x = torch.rand(64, 1, 28, 28, device="cuda") * 2 - 1
    labels = (torch.arange(64, device="cuda") % 10).to(torch.int64)
    step = G.GraphedTrainStep(m, opt, (x, labels))
    kinds = G.node_types(step.graph)
    assert kinds is None or set(kinds) == {"kernel"}, kinds
    losses = [float(step((x, labels)).detach()) for _ in range(40)]
    assert len(set(round(v, 3) for v in losses[:4])) == 4                          # fresh noise (and fresh weights) every replay
    assert sum(losses[-5:]) < sum(losses[:5])
    assert int(m.encoder._buffer("network.3.num_batches_tracked")) == 43           # 3 warm-up + 40 replays
    # labels written into the static buffer between replays change the loss: replay with frozen weights (lr = 0) and the device
    # generator rewound before each replay, so that the labels are the only thing that differs (the same labels twice: what is left
    # is the order of the atomic sums in the batch-norm statistics and the loss)
    opt.param_groups[0]["lr"] = 0.0
    opt.sync_lr()

    def frozen(lab):
        torch.cuda.manual_seed(99)
        return float(step((x, lab)).detach())
    a, a2, b = frozen(labels), frozen(labels), frozen((labels + 5) % 10)
    print(f"graphed step, frozen weights: loss {a:.6f} / {a2:.6f} on the same labels, {b:.6f} on shifted labels")
    assert a != b and abs(a - b) > 10 * abs(a - a2)


def test_run_py_cvae_end_to_end(tmp_path):
    """python run.py experiment=cvae/synthetic: compose -> fit (labels from the datamodule, Adam over three buffers) -> validate -> checkpoint."""
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-generation-models_amd")
    cmd = [sys.executable, os.path.join(pkg, "run.py"), "experiment=cvae/synthetic", "datamodule.train_size=256", "datamodule.val_size=64",
           "datamodule.batch_size=32", "trainer.max_epochs=2", f"log_dir={tmp_path}", "seed=1", "print_config=False"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    run_dir = tmp_path / "runs" / "cvae" / "synthetic"
    assert (run_dir / "results" / "0.jpg").exists()
    ck = torch.load(sorted((run_dir / "checkpoints").glob("*.ckpt"), key=lambda p: int(str(p).split("step=")[-1].split(".")[0]))[-1])
    sd = ck["state_dict"]
    assert tuple(sd["class_embedding.weight"].shape) == (10, 128) and tuple(sd["encoder.network.0.weight"].shape) == (32, 11, 4, 4)
    assert int(sd["encoder.network.3.num_batches_tracked"]) == 16                  # 2 epochs x 8 steps
    text = (run_dir / "tensorboard" / "metrics.jsonl").read_text()
    for key in LOGS + ("val_log/log_p_x_of_z",):
        assert key in text, key


def test_refusals():
    m = _model(8, 16)
    with pytest.raises(RuntimeError):
        m.training_step((torch.rand(2, 1, 28, 28), torch.tensor([1, 2])), 0)       # CPU tensors
    with pytest.raises(RuntimeError):
        m(torch.randn(2, 16), torch.tensor([1, 2]))
    enc, dec = {"_target_": "src.networks.basic.ConvEncoder", "ndf": 8}, {"_target_": "src.networks.basic.ConvDecoder", "ngf": 8}
    with pytest.raises(NotImplementedError):
        M.cVAE(DM, encoder=enc, decoder=dec, latent_dim=16, n_classes=10)           # the constructor default "guassian": rejected by the reference too
    with pytest.raises((TypeError, ValueError)):
        M.cVAE(DM, encoder=enc, decoder=dec, latent_dim=16, decoder_dist="gaussian")   # n_classes=None
