"""MADE on the MI355X: the masked-linear / head / sampling kernels against torch on the CPU, the tiny nets against the reference's
fixture (tests/golden/made_kats.npz), a full-size step against the float64 oracle, causality, the replayed sampler, the graphed
training step and run.py end to end."""
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _made_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-generation-models_amd")


def _K():
    from src.ops import functional as K
    return K


def _dm(ch, H, W, normalize=False):
    return types.SimpleNamespace(width=W, height=H, channels=ch, transforms=types.SimpleNamespace(normalize=normalize))


def _rel(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max()) / max(float(b.abs().max()), 1e-30)


def _degrees(fin, fout, first):
    din = torch.arange(fin) if first else torch.randint(0, 97, (fin,))
    dout = torch.randint(int(din.min()), int(din.max()) + 1, (fout,))
    return din.int(), dout.int()


# ------------------------------------------------------------------ 1. masked linear: forward, data gradient, weight gradient
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("n,fin,fout,first", [(128, 784, 1024, True), (128, 1024, 1024, False), (3, 27, 40, True)])
def test_masked_linear_fwd_dgrad_wgrad(n, fin, fout, first, mode):
    """fp32 mode: fp32-exact MFMA, <= 1e-5 of max |ref|.  bf16 mode: operands rounded to bf16 and fp32 accumulation: <= 2e-2 against
    the unrounded reference, and <= 1e-5 against the reference whose matrix-core operands are rounded the same way (what is left is
    fp32 accumulation order: <= 4e-7 on the CPU, tests/test_made_cpu.py::test_rounded_operands_leave_only_fp32_accumulation)."""
    K = _K()
    md, tol = (K.MODE_FP32, 1e-5) if mode == "fp32" else (K.MODE_BF16, 2e-2)
    din, dout = _degrees(fin, fout, first)
    mask = dout[:, None] >= din[None, :]
    w = torch.randn(fout, fin) / math.sqrt(fin)
    b = torch.randn(fout) * 0.1
    x = torch.rand(n, fin)
    ref = torch.sigmoid(x.double() @ (w.double() * mask).t() + b.double())
    dd = [t.to(DEV) for t in (din, dout)]
    wd = w.to(DEV)
    y = K.made_linear(x.to(DEV), wd, b.to(DEV), *dd, True, mode=md)
    assert _rel(y, ref) <= tol
    rb = mode == "bf16"
    assert _rel(y, O.masked_linear_ref(x, w, b, din, dout, True, rb)) <= 1e-5
    gy = torch.randn(n, fout)
    s_in = torch.rand(n, fin)
    dx_ref = (gy.double() @ (w.double() * mask)) * s_in.double() * (1 - s_in.double())
    dx = K.made_dgrad(gy.to(DEV), wd, *dd, s_in=s_in.to(DEV), mode=md)
    assert _rel(dx, dx_ref) <= tol
    assert _rel(dx, O.masked_dgrad_ref(gy, w, din, dout, s_in, rb)) <= 1e-5
    dw = torch.zeros(fout, fin, device=DEV)
    db = torch.full((fout,), float("nan"), device=DEV)
    K.made_wgrad(gy.to(DEV), x.to(DEV), *dd, dw, db, mode=md)
    dw_ref = (gy.double().t() @ x.double()) * mask
    assert _rel(dw, dw_ref) <= tol
    assert _rel(dw, O.masked_wgrad_ref(gy, x, din, dout, rb)[0]) <= 1e-5
    assert _rel(db, gy.double().sum(0)) <= tol
    assert float(dw.cpu()[~mask].abs().max()) == 0.0 if (~mask).any() else True   # masked entries: never written


# ------------------------------------------------------------------ 2. fused head against F.cross_entropy
@pytest.mark.parametrize("n,hd,C,H,W,normalize", [(128, 1024, 1, 28, 28, False), (3, 40, 3, 3, 3, True)])
def test_fused_head_against_cross_entropy(n, hd, C, H, W, normalize):
    K = _K()
    D = C * H * W
    dh_ = torch.randint(0, D, (hd,))
    din = dh_.int()
    dout = (torch.arange(D).repeat_interleave(256) - 1).int()
    mask = dout[:, None] >= din[None, :]
    w = torch.randn(256 * D, hd) / math.sqrt(hd)
    b = torch.randn(256 * D) * 0.1
    h = torch.rand(n, hd)
    k = torch.randint(0, 256, (n, C, H, W))
    k.view(-1)[:3] = torch.tensor([0, 255, 1])
    x = k.float() * 2 / 255 - 1 if normalize else k.float() / 255
    hr, wr, br = h.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    logits = F.linear(hr, wr * mask, br).reshape(n, C, H, W, 256).permute(0, 4, 1, 2, 3)
    ref = (F.cross_entropy(logits, O.target(x, normalize), reduction="none").mean([1, 2, 3]) / math.log(2.0)).mean()
    ref.backward()
    dd = [t.to(DEV) for t in (din, dout)]
    hd_, wd, bd, xd = h.to(DEV), w.to(DEV), b.to(DEV), x.reshape(n, D).to(DEV)
    loss, lse = K.made_head_fwd(hd_, wd, bd, *dd, xd, normalize)
    assert abs(float(loss) - float(ref)) <= 1e-5 * float(ref)
    dl = K.made_head_dlogits(hd_, wd, bd, *dd, xd, normalize, lse, gscale=torch.ones(1, device=DEV))
    dh = K.made_dgrad(dl, wd, *dd)
    assert _rel(dh, hr.grad) <= 1e-4
    dw = torch.zeros_like(wd)
    db = torch.empty_like(bd)
    K.made_wgrad(dl, hd_, *dd, dw, db)
    assert _rel(dw, wr.grad) <= 1e-4 and _rel(db, br.grad) <= 1e-4
    lg = K.made_linear(hd_, wd, bd, *dd, False)
    assert torch.equal(lg[:, :256].cpu(), b[:256].expand(n, 256))          # pixel 0: its bias only


# ------------------------------------------------------------------ 3. tiny nets against the reference's fixture
@pytest.fixture(scope="module")
def kats(golden_dir):
    return np.load(os.path.join(golden_dir, "made_kats.npz"))


def _tiny(kats, tag, mode="fp32"):
    from src.models.made import MADE
    x = torch.from_numpy(kats[tag + ".x"])
    sd = {k[len(tag) + 5:]: torch.from_numpy(kats[k]) for k in kats.files if k.startswith(tag + ".sd0.")}
    hidden = sd["model.model.0.model.weight"].shape[0]
    n_layer = sum(1 for k in sd if k.endswith(".mask")) - 1
    m = MADE(_dm(x.shape[1], x.shape[2], x.shape[3], normalize=tag == "c"), hidden, n_layer)
    m.load_state_dict(sd)
    m.compute_mode = mode
    m.to(DEV)
    return m, x.to(DEV), sd


@pytest.mark.parametrize("tag", ["u", "c"])
def test_tiny_net_logits_bpd_gradients(kats, tag):
    m, x, sd = _tiny(kats, tag)
    pos = kats[tag + ".pos"]
    logits = m(x).cpu()
    assert _rel(logits[pos[:, 0], :, pos[:, 1], pos[:, 2], pos[:, 3]], torch.from_numpy(kats[tag + ".logits"])) <= 1e-4
    m.train()
    bpd = m.calc_likelihood(x)
    bpd.backward()
    rb = float(kats[tag + ".bpd"])
    assert abs(float(bpd) - rb) <= 1e-5 * rb
    worst = 0.0
    for k, p in m.named_parameters():
        r = torch.from_numpy(kats[f"{tag}.grad.{k}"])
        g = p.grad.cpu()
        mk = sd.get(k.replace("model.weight", "mask")) if k.endswith("model.weight") else None
        if mk is not None:
            assert float(g[~mk].abs().max()) == 0.0 if (~mk).any() else True
        if float(r.abs().max()) > 0:
            worst = max(worst, _rel(g, r))
    assert worst <= 1e-4, worst


@pytest.mark.parametrize("tag", ["u", "c"])
def test_tiny_net_five_adam_steps(kats, tag):
    """5 FlatAdam steps in fp32 mode against the reference's torch Adam: per-step bpd <= 1e-4, every tensor's displacement on the
    live entries <= 2e-2 rel-L2, masked weight entries bit-identical to sd0."""
    m, x, sd = _tiny(kats, tag)
    opt = m.configure_optimizers()[0][0]
    traj = []
    m.train()
    for _ in range(5):
        opt.zero_grad()
        loss = m.calc_likelihood(x)
        loss.backward()
        opt.step()
        traj.append(float(loss))
    assert np.abs(np.array(traj) - kats[tag + ".traj_bpd"]).max() <= 1e-4, (traj, kats[tag + ".traj_bpd"])
    for k, p in m.named_parameters():
        now = p.detach().cpu()
        disp = now - sd[k]
        r = torch.from_numpy(kats[f"{tag}.disp.{k}"])
        if k.endswith("model.weight"):
            mk = sd[k.replace("model.weight", "mask")]
            assert torch.equal(now[~mk], sd[k][~mk]), k                  # masked entries: their init values, bit for bit
            disp, r = disp[mk], r[mk]
        if float(r.norm()) > 0:
            assert float((disp - r).norm()) <= 2e-2 * float(r.norm()), k
        else:
            assert float(disp.norm()) == 0.0, k


@pytest.mark.parametrize("tag", ["u", "c"])
def test_tiny_net_bf16_within_reference_budget(kats, tag):
    """bf16 mode: logits within 2x the reference's own CPU bf16-autocast error (fixture), bpd within 1e-2 relative."""
    m, x, _ = _tiny(kats, tag, mode="bf16")
    pos = kats[tag + ".pos"]
    logits = m(x).cpu()
    err = _rel(logits[pos[:, 0], :, pos[:, 1], pos[:, 2], pos[:, 3]], torch.from_numpy(kats[tag + ".logits"]))
    assert err <= 2 * float(kats[tag + ".bf16_err"]), (err, float(kats[tag + ".bf16_err"]))
    with torch.no_grad():
        bpd = float(m.calc_likelihood(x))
    assert abs(bpd - float(kats[tag + ".bpd"])) <= 1e-2 * float(kats[tag + ".bpd"])


# ------------------------------------------------------------------ 4. one full-size step against the float64 oracle
def test_full_size_step_against_oracle():
    from src.models.made import MADE
    torch.manual_seed(5)
    m = MADE(_dm(1, 28, 28), 1024, 3)
    p = {k: v.clone() for k, v in m.state_dict().items()}
    x = torch.randint(0, 256, (128, 1, 28, 28)).float() / 255
    m.to(DEV).train()
    bpd = m.calc_likelihood(x.to(DEV))
    bpd.backward()
    gw = m.model.layers[3].model.weight.grad.cpu()
    ref, grads = O.bpd_and_grads(p, x, False)
    assert abs(float(bpd) - float(ref)) <= 1e-5 * float(ref), (float(bpd), float(ref))
    assert _rel(gw, grads["model.model.3.model.weight"]) <= 1e-4


# ------------------------------------------------------------------ 5. causality: a masked-off input never meets a weight
def _causality(mode):
    from src.models.made import MADE
    torch.manual_seed(1)
    m = MADE(_dm(3, 6, 5), 64, 3)
    m.compute_mode = mode
    m.to(DEV)
    D = 90
    x = torch.randint(0, 256, (4, 3, 6, 5), device=DEV).float() / 255
    base = m(x).reshape(4, 256, D)
    for p in (0, 37, D - 1):
        xp = x.clone().reshape(4, D)
        xp[:, p:] = float("nan")
        out = m(xp.reshape_as(x)).reshape(4, 256, D)[..., :p + 1]
        assert torch.isfinite(out).all(), p
        assert torch.equal(out, base[..., :p + 1]), p


def test_causality_nan_poisoned_later_pixels():
    _causality("fp32")


def test_causality_nan_poisoned_later_pixels_bf16():
    _causality("bf16")


# ------------------------------------------------------------------ 6. sampler, teacher-forced against the oracle
def _teacher_forced(ch, N):
    from src.models.made import MADE
    torch.manual_seed(2)
    H = W = 6
    m = MADE(_dm(ch, H, W), 32, 2)
    # a peaked output distribution, as a trained net has: few uniforms then fall within the 1e-5 band of a CDF boundary
    with torch.no_grad():
        m.model.layers[-1].model.weight.mul_(40.0)
        m.model.layers[-1].model.bias.mul_(40.0)
    p = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.to(DEV)
    g = torch.Generator().manual_seed(5)
    tape = torch.rand(H * W, N * ch, generator=g)
    m.uniform_source = lambda shape, device: tape.reshape(shape).to(device)
    rec = []
    m.sample((N, ch, H, W))                               # capture
    next(iter(m._samplers.values())).run(record=rec)
    prev = torch.full((N, ch, H, W), -1.0)
    skipped = 0
    for step, img in enumerate(rec):
        img = img.cpu()
        hh, ww = divmod(step, W)
        probs = F.softmax(O.forward(p, prev)[:, :, :, hh, ww].permute(0, 2, 1), -1).reshape(N * ch, 256)
        k, dist = O.pick(probs, tape[step].double())
        want = (k.float() / 255).reshape(N, ch)
        got = img[:, :, hh, ww]
        near = dist < 1e-5
        skipped += int(near.sum())
        assert torch.equal(got.reshape(-1)[~near], want.reshape(-1)[~near]), step
        other = img.clone()
        other[:, :, hh, ww] = prev[:, :, hh, ww]
        assert torch.equal(other, prev)                   # only position (h, w) changes
        prev = img
    draws = len(rec) * N * ch
    assert skipped * 10000 <= max(draws, 10000), (skipped, draws)      # at most 1 draw in 10 000


@pytest.mark.parametrize("ch", [1, 3])
def test_sampler_teacher_forced(ch):
    _teacher_forced(ch, 4)


def test_sampler_teacher_forced_second_pass_of_the_wave_loop():
    """N * C = 24 > 16: mi_made_sample_step's 16 waves take a second unit each."""
    _teacher_forced(1, 24)


# ------------------------------------------------------------------ 7. completion semantics
def test_completion_semantics():
    from src.models.made import MADE
    torch.manual_seed(4)
    m = MADE(_dm(2, 4, 4), 16, 2).to(DEV)
    img = (torch.randint(0, 256, (3, 2, 4, 4)).float() / 255).to(DEV)
    img[1, 1, 2, 1] = -1                                   # only sample 1, channel 1 misses position (2, 1)
    img[0, :, 2, 1] = 0.3                                  # given, and off the k / 255 grid: a rewrite is visible
    img[2, :, 2, 1] = 0.3
    img[1, 0, 2, 1] = 0.3
    out = m.sample((3, 2, 4, 4), img=img.clone())
    changed = out != img
    changed[:, :, 2, 1] = False
    assert not changed.any()                              # fully given positions are untouched
    col = out[:, :, 2, 1].cpu()
    assert (col >= 0).all() and torch.equal(col, torch.round(col * 255) / 255)   # every sample and channel there gets a draw


# ------------------------------------------------------------------ 8. the graphed training step
def test_graphed_training_step_matches_eager():
    from src.models.made import MADE
    from src.runtime.graphed import GraphedTrainStep, node_types
    from src.runtime.optim import FlatAdam
    torch.manual_seed(11)
    ms = [MADE(_dm(1, 8, 8), 64, 3) for _ in range(2)]
    ms[1].load_state_dict(ms[0].state_dict())
    xa = (torch.randint(0, 256, (16, 1, 8, 8)).float() / 255).to(DEV)
    xb = (torch.randint(0, 256, (16, 1, 8, 8)).float() / 255).to(DEV)
    lab = torch.zeros(16, dtype=torch.int64, device=DEV)
    opts = []
    for i, m in enumerate(ms):
        m.to(DEV).train()
        opts.append(FlatAdam(m, lr=1e-3, device_state=(i == 0)))
        m.training_step((xa, lab), 0).backward()
        opts[-1].step()
    gs = GraphedTrainStep(ms[0], opts[0], (xa, lab), warmup=0)
    nt = node_types(gs.graph)
    assert nt is None or set(nt) <= {"kernel"}, nt
    got = float(gs((xb, lab)))
    want = ms[1].training_step((xb, lab), 1)
    want.backward()
    opts[1].step()
    assert abs(got - float(want)) <= 1e-5 * abs(float(want)), (got, float(want))
    assert _rel(ms[0].flat_params, ms[1].flat_params) <= 1e-5


# ------------------------------------------------------------------ 9. run.py end to end
def test_run_py_made_end_to_end(tmp_path):
    import subprocess
    cmd = [sys.executable, os.path.join(PKG, "run.py"), "experiment=made/synthetic", "datamodule.train_size=128",
           "datamodule.val_size=32", "datamodule.batch_size=32", "datamodule.width=8", "datamodule.height=8", "model.hidden_dim=64",
           "trainer.max_epochs=1", f"log_dir={tmp_path}", "seed=1", "print_config=False"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    run_dir = tmp_path / "runs" / "made" / "synthetic"
    assert (run_dir / "results" / "0.jpg").exists()
    assert list((run_dir / "checkpoints").glob("*.ckpt"))
    vals = [json.loads(ln) for ln in (run_dir / "tensorboard" / "metrics.jsonl").read_text().splitlines() if "val_bpd" in ln]
    assert vals and all(math.isfinite(float(v["val_bpd"])) for v in vals)
