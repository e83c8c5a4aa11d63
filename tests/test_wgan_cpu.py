"""WGAN host layer without a GPU: the experiments compose with the reference's values, the state-dict keys and their order are the
reference's (tests/golden/wgan_clip_kats.npz, produced by the reference's own WGAN: tools/gen_golden_wgan_clip.py), the optimizers are
`FlatRMSprop`, a CPU tensor raises, what is not built is refused, and the golden file is self-consistent -- the reference's float32
trajectory meets, against its float64 trajectory, the bounds tests/test_wgan_clip_gpu.py holds this package to.  Then the numpy
oracles of the three kernels (tests/_rmsprop_oracle.py) against torch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rmsprop_oracle as RO  # noqa: E402
import _wgan_golden as WG  # noqa: E402

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-generation-models_amd")
DM = {"width": 28, "height": 28, "channels": 1, "transforms": {"normalize": True}}
NETD = {"_target_": "src.networks.basic.ConvEncoder", "norm_type": "batch"}
NETG = {"_target_": "src.networks.basic.ConvDecoder", "norm_type": "batch"}


def _model(nf=4, **kw):
    from src.models.wgan import WGAN
    kw.setdefault("latent_dim", 8)
    return WGAN(DM, netG=dict(NETG, ngf=nf), netD=dict(NETD, ndf=nf), **kw)


@pytest.fixture(scope="module")
def kats(golden_dir):
    return np.load(os.path.join(golden_dir, "wgan_clip_kats.npz"))


def test_experiments_compose_with_the_reference_values():
    from src.runtime.config import Composer
    for exp, epochs in (("wgan/mnist_conv", 200), ("wgan/synthetic", 1)):
        c = Composer(os.path.join(PKG, "configs")).compose("config", [f"experiment={exp}"])
        m = c.model
        assert m._target_ == "src.models.wgan.WGAN" and m.latent_dim == 100 and c.exp_name == exp
        assert float(m.lrG) == 6e-4 and float(m.lrD) == 6e-4 and float(m.alpha) == 0.99 and m.n_critic == 5 and float(m.clip_weight) == 0.1
        assert c.trainer.max_epochs == epochs
        assert m.netG._target_ == "src.networks.basic.ConvDecoder" and m.netG.ngf == 32 and m.netG.norm_type == "batch"
        assert m.netD._target_ == "src.networks.basic.ConvEncoder" and m.netD.ndf == 32 and m.netD.norm_type == "batch"
        assert (c.datamodule.width, c.datamodule.height, c.datamodule.channels) == (28, 28, 1)
        synthetic = exp.endswith("synthetic")
        assert c.datamodule._target_ == ("src.datamodules.synthetic.SyntheticDataModule" if synthetic else "src.datamodules.mnist.MNISTDataModule")
    # the model file's own defaults are the reference's
    c = Composer(os.path.join(PKG, "configs")).compose("config", ["model=wgan", "networks=conv_mnist"])
    m = c.model
    assert (float(m.lrG), float(m.lrD), float(m.alpha), m.n_critic, float(m.clip_weight), m.latent_dim) == (5e-5, 5e-5, 0.99, 5, 0.01, 100)
    assert sorted(os.listdir(os.path.join(PKG, "configs", "experiment", "wgan"))) == ["mnist_conv.yaml", "synthetic.yaml"]


def test_config_instantiates_the_model():
    from src.runtime.config import Composer, instantiate
    c = Composer(os.path.join(PKG, "configs")).compose("config", ["experiment=wgan/mnist_conv", "networks.decoder.ngf=4", "networks.encoder.ndf=4"])
    m = instantiate(c.model, datamodule=c.datamodule)
    hp = m.hparams
    assert type(m).__name__ == "WGAN" and type(m).__module__.endswith("models.wgan")
    assert (hp.latent_dim, hp.n_critic, hp.clip_weight, hp.lrG, hp.lrD, hp.alpha, hp.eval_fid) == (100, 5, 0.1, 6e-4, 6e-4, 0.99, False)
    G, D = m.generator, m.discriminator
    assert G.input_channel == 100 and G.output_channel == 1 and D.input_channel == 1 and D.output_channel == 1
    assert G.fused_norm_act and D.fused_norm_act and G.reproducible and D.reproducible and m.automatic_optimization is False


def test_state_dict_keys_order_and_optimizers(kats):
    import src.models as models
    from src.runtime.optim import FlatRMSprop
    assert not hasattr(models, "WGAN")                                                  # src.models.wgan_gp has a WGAN too: no lazy name
    m = _model()
    assert list(m.state_dict().keys()) == list(kats["tiny.names"])
    assert [k for k, _ in m.named_parameters()] == list(kats["tiny.pnames"])
    sd = {k[len("tiny.sd0."):]: torch.from_numpy(kats[k]) for k in kats.files if k.startswith("tiny.sd0.")}
    assert list(sd) == list(kats["tiny.names"])
    m.load_state_dict(sd)
    assert torch.equal(m.state_dict()["discriminator.network.5.weight"], sd["discriminator.network.5.weight"])    # loading does not clip
    assert m.flat_nets() == [m.generator, m.discriminator]
    hp = m.hparams
    assert (hp.latent_dim, hp.n_critic, hp.clip_weight, hp.lrG, hp.lrD, hp.alpha) == (8, 5, 0.01, 5e-5, 5e-5, 0.99)     # the defaults
    opt_g, opt_d = m.configure_optimizers()
    assert type(opt_g) is FlatRMSprop and type(opt_d) is FlatRMSprop and opt_g.nets == [m.generator] and opt_d.nets == [m.discriminator]
    for grp in opt_g.param_groups + opt_d.param_groups:
        assert grp["lr"] == 5e-5 and grp["alpha"] == 0.99 and grp["eps"] == 1e-8
    opt_g, opt_d = _model(lrG=1e-3, lrD=2e-3, alpha=0.9).configure_optimizers()
    assert (opt_g.param_groups[0]["lr"], opt_d.param_groups[0]["lr"], opt_d.param_groups[0]["alpha"]) == (1e-3, 2e-3, 0.9)
    assert all(k.startswith("generator.") for k in kats["tiny.g.gnames"]) and all(k.startswith("discriminator.") for k in kats["tiny.d.gnames"])
    assert (float(kats["tiny.clip_weight"]), float(kats["tiny.lr"]), float(kats["tiny.alpha"])) == (WG.CLIP, WG.LR, WG.ALPHA)
    assert (float(kats["traj.clip_weight"]), float(kats["traj.lr"]), int(kats["traj.n_critic"])) == (WG.CLIP, WG.LR, WG.N_CRITIC)


def test_a_cpu_tensor_raises_and_what_is_not_built_is_refused():
    from src.models.wgan import WGAN
    m = _model()
    m._optimizers = list(m.configure_optimizers())
    before = {k: v.clone() for k, v in m.state_dict().items()}
    for idx in (0, 1):
        with pytest.raises(RuntimeError):
            m.training_step((torch.rand(4, 1, 28, 28), None), idx)                      # a CPU batch, either phase
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    with pytest.raises(RuntimeError):
        m(torch.randn(2, 8))                                                           # forward(z) on the CPU
    with pytest.raises(NotImplementedError):
        _model(eval_fid=True)
    with pytest.raises(NotImplementedError):                                            # the layer-norm nets are the WGAN-GP's
        WGAN(DM, netG=dict(NETG, ngf=4, norm_type="layer"), netD=dict(NETD, ndf=4), latent_dim=8)
    with pytest.raises(NotImplementedError):
        WGAN(dict(DM, width=32, height=32), netG=dict(NETG, ngf=4), netD=dict(NETD, ndf=4), latent_dim=8)
    with pytest.raises(NotImplementedError):                                            # conv32 nets: no BatchNorm there
        WGAN(dict(DM, width=32, height=32, channels=3), netG={"_target_": "src.networks.conv32.Decoder", "ngf": 8},
             netD={"_target_": "src.networks.conv32.Encoder", "ndf": 8}, latent_dim=8)


def test_flat_rmsprop_state_dict_round_trips_on_the_host():
    from src.runtime.optim import FlatAdam, FlatRMSprop
    m = _model()
    opt = FlatRMSprop(m.discriminator, lr=3e-4, alpha=0.9)
    assert not isinstance(opt, FlatAdam) and isinstance(opt, torch.optim.Optimizer)
    opt.zero_grad()                                                                     # a no-op: nothing allocated, nothing raised
    sd = opt.state_dict()
    assert sd["step"] == 0 and sd["v"] is None and sd["param_groups"] == [{k: v for k, v in opt.param_groups[0].items() if k != "params"}]
    assert sd["param_groups"][0]["lr"] == 3e-4 and sd["param_groups"][0]["alpha"] == 0.9 and sd["param_groups"][0]["eps"] == 1e-8
    n = m.discriminator.flat_params.numel()
    v = torch.rand(n)
    other = FlatRMSprop(m.discriminator)
    other.load_state_dict({"step": 7, "v": [v], "param_groups": [{"lr": 1e-3, "alpha": 0.95, "eps": 1e-6}]})
    got = other.state_dict()
    assert got["step"] == 7 and torch.equal(got["v"][0], v) and got["v"][0] is not v
    assert got["param_groups"][0] == {**got["param_groups"][0], "lr": 1e-3, "alpha": 0.95, "eps": 1e-6}
    buf = other._v[0]
    other.load_state_dict({"step": 9, "v": v * 2, "param_groups": got["param_groups"]})    # one tensor for one net; in place
    assert other._v[0] is buf and torch.equal(buf, v * 2) and other.device_step_count() == 9
    again = FlatRMSprop(m.discriminator)
    again.load_state_dict(other.state_dict())
    assert torch.equal(again.state_dict()["v"][0], v * 2) and again.state_dict()["step"] == 9
    other.load_state_dict({"step": 0, "v": None})
    assert float(other._v[0].abs().max()) == 0.0
    with pytest.raises(ValueError):
        other.load_state_dict({"step": 1, "v": [torch.zeros(n + 64)]})
    with pytest.raises(ValueError):
        other.load_state_dict({"step": 1, "v": [torch.zeros(n), torch.zeros(n)]})
    both = FlatRMSprop([m.generator, m.discriminator])
    both.load_state_dict({"step": 2, "v": [torch.ones(m.generator.flat_params.numel()), torch.ones(n)]})
    assert [t.numel() for t in both.state_dict()["v"]] == [m.generator.flat_params.numel(), n]


def test_golden_trajectories_are_self_consistent(kats):
    """The reference's float32 run against its float64 run, held to exactly what tests/test_wgan_clip_gpu.py holds this package to: the
    logged scalars, the parameters within `rmsprop_tolerance`, the running statistics.  The running means behind a conv bias miss the
    plain bound in the reference itself (the bias takes RMSprop's noise steps); with the bias part taken out they meet it."""
    g = kats
    misses = WG.reference_misses(g)
    print("running statistics outside 1e-5 * max|ref| + 1e-5 in the reference's own float32 run:", misses)
    assert set(misses) <= set(WG.BIAS_IN_FRONT) and len(misses) >= 1
    logs = [{k[len(f"traj.log32.{i}."):]: float(g[k]) for k in g.files if k.startswith(f"traj.log32.{i}.")} for i in range(WG.STEPS)]
    WG.check_traj_logs(g, logs, "reference float32")
    sd32 = {str(k): g[f"traj.sd32.{k}"] for k in g["tiny.names"]}
    bias32 = {b: WG.ref_bias_after(g, "32", b) for b in WG.BIAS_IN_FRONT.values()}
    assert list(g["traj.biases"]) == list(WG.BIAS_IN_FRONT.values())
    worst = WG.check_traj_state(g, sd32, bias32, "reference float32")
    assert all(r <= 1 for r in worst.values())
    # the biases did take the noise steps, lr g / (sqrt(1 - alpha) |g| + eps) <= lr / sqrt(1 - alpha): that is why the treatment exists
    first = WG.LR / (1 - WG.ALPHA) ** 0.5
    for b in WG.BIAS_IN_FRONT.values():
        i = WG.update_steps(b)[0]
        before = g["tiny.sd0." + b] if i == 0 else g[f"traj.bias32.{i - 1}.{b}"]
        if b.startswith(WG.D):
            before = np.clip(before, -WG.CLIP, WG.CLIP)
        moved = np.abs(g[f"traj.bias32.{i}.{b}"] - before)
        print(f"{b}: first update moves it by up to {float(moved.max()):.3e} (lr {WG.LR:g}, largest possible step {first:.3e})")
        assert 0.1 * WG.LR < float(moved.max()) <= first * (1 + 1e-3), (b, float(moved.max()))
    assert WG.update_steps("generator.x") == [0, 3, 6] and WG.update_steps("discriminator.x") == [1, 2, 4, 5]
    assert sum(WG.step_weights("generator.x")) == pytest.approx(1 - 0.9 ** 7)
    assert sum(WG.step_weights("discriminator.x")) == pytest.approx(1 - 0.9 ** 11)
    assert WG.step_weights("discriminator.x")[-1] == pytest.approx(0.1) and WG.step_weights("discriminator.x")[-2] == pytest.approx(0.09 + 0.081)
    # the tolerance's two caps
    z = torch.zeros(3, dtype=torch.float64)
    assert float(WG.rmsprop_tolerance(z, [z, z, z], False).max()) == pytest.approx(3 * 2 * first)
    assert float(WG.rmsprop_tolerance(z, [z, z, z, z], True).max()) == pytest.approx(min(4 * 2 * first, 2 * WG.CLIP))


def test_golden_steps_hold_what_the_reference_does_with_the_clip(kats):
    """After a generator step the critic's parameters are clamp(sd0): the clip changed elements in both directions and left others; after
    a critic step they are the unclipped result of the update."""
    g, c = kats, np.float32(WG.CLIP)
    up = down = kept = 0
    for k in g["tiny.pnames"]:
        k = str(k)
        if not k.startswith(WG.D):
            continue
        sd0 = g["tiny.sd0." + k]
        after_g = g[f"tiny.g.sd1.{k}"] if f"tiny.g.sd1.{k}" in g.files else (sd0.astype(np.float64) + g[f"tiny.g.dsd1.{k}"]).astype(np.float32)
        assert np.array_equal(after_g, np.clip(sd0, -c, c)), k
        up, down, kept = up + int((sd0 > c).sum()), down + int((sd0 < -c).sum()), kept + int((np.abs(sd0) < c).sum())
        if k in ("discriminator.network.3.weight", "discriminator.network.6.weight"):   # BatchNorm weights: not all on one side
            assert (sd0 > c).any() and (sd0 < -c).any() and (np.abs(sd0) < c).any(), k
    assert up > 0 and down > 0 and kept > 0
    after_d = [g[f"tiny.d.sd1.{k}"] if f"tiny.d.sd1.{k}" in g.files else g["tiny.sd0." + str(k)].astype(np.float64) + g[f"tiny.d.dsd1.{k}"]
               for k in g["tiny.pnames"] if str(k).startswith(WG.D)]
    assert max(float(np.abs(a).max()) for a in after_d) > WG.CLIP


# --------------------------------------------------------------------------- the kernel oracles against torch
def test_oracle_rmsprop_is_torch_s():
    r = np.random.RandomState(0)
    for alpha in (0.99, 0.9):
        p0 = r.randn(257)
        gs = [r.randn(257) * 10.0 ** r.randint(-4, 2, 257) for _ in range(3)]
        for g in gs:
            g[:5] = 0.0                                                                 # never a gradient: must not move
        t = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        opt = torch.optim.RMSprop([t], lr=6e-4, alpha=alpha)
        p, v = p0.copy(), np.zeros_like(p0)
        for g in gs:
            t.grad = torch.from_numpy(g * 0.5)
            opt.step()
            p, v = RO.rmsprop_step(p, g, v, 6e-4, alpha, 1e-8, gscale=0.5)
            assert np.abs(p - t.detach().numpy()).max() <= 1e-15
            assert np.abs(v - opt.state[t]["square_avg"].numpy()).max() <= 1e-15 * max(1.0, np.abs(v).max())
        assert np.array_equal(p[:5], p0[:5]) and np.array_equal(v[:5], np.zeros(5))
    p32, v32 = RO.rmsprop_step(p0.astype(np.float32), gs[0].astype(np.float32), np.zeros(257, np.float32), 6e-4)
    assert p32.dtype == np.float32 and v32.dtype == np.float32


def test_oracle_clamp_is_torch_s():
    x = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 0.1, -0.1, 0.1000001, -0.1000001, 0.05, -3.0, 1e-40], dtype=np.float32)
    lo, hi = np.float32(-0.1), np.float32(0.1)
    got, want = RO.clamp(x, lo, hi), torch.clamp(torch.from_numpy(x), float(lo), float(hi)).numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(got[0]) and np.signbit(got[3]) and got[1] == hi and got[2] == lo
    r = np.random.RandomState(1).randn(1000)
    assert np.array_equal(RO.clamp(r, -0.5, 0.25), torch.clamp(torch.from_numpy(r), -0.5, 0.25).numpy())


def test_oracle_critic_loss_is_the_reference_s_formulas():
    r = np.random.RandomState(2)
    for M in (1, 5, 64):
        real, fake = torch.from_numpy(r.randn(M)).requires_grad_(True), torch.from_numpy(r.randn(M)).requires_grad_(True)
        real_loss, fake_loss = -real.mean(), fake.mean()                                # wgan.py:81-83
        (0.5 * (real_loss + fake_loss)).backward()
        loss, mean, d = RO.critic_loss(np.concatenate([real.detach().numpy(), fake.detach().numpy()]), (True, False), scale=0.5)
        assert np.allclose(loss, [float(real_loss), float(fake_loss)], rtol=1e-14, atol=0)
        assert np.allclose(mean, [float(-real_loss), float(fake_loss)], rtol=1e-14, atol=0)
        assert np.allclose(d, np.concatenate([real.grad.numpy(), fake.grad.numpy()]), rtol=1e-14, atol=0)
        g_loss, _, dg = RO.critic_loss(fake.detach().numpy(), (True,))                  # wgan.py:72: -mean(D(G(z)))
        assert g_loss[0] == pytest.approx(-float(fake.detach().mean()), rel=1e-14) and np.allclose(dg, -1.0 / M)
