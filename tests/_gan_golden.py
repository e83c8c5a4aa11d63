"""What tests/test_gan_cpu.py and tests/test_gan_gpu.py share: the comparisons against tests/golden/gan_kats.npz (the reference's own
GAN.training_step, tools/gen_golden_gan.py) with the tolerances of tests/test_aae_gpu.py.

Conv biases in front of a BatchNorm have an analytically zero gradient: what Adam gets is rounding noise, and every update moves such
a bias by up to lr in that noise's direction (docs/kernels.md 4i).  The layer's output does not see it, its running MEAN does: the
batch mean is the bias-free mean plus the bias.  Over the 4-step trajectory (G, D, G, D) the running mean ends as
sum_j w_j (s_j + b_j) over its momentum updates j, b_j the bias at that forward.  `bias_part` is sum_j w_j b_j; the comparison takes it
out on both sides, each side with its OWN biases, and keeps the bound -- the treatment tests/test_aae_gpu.py gives BIAS_IN_FRONT.  It is
applied only to the running means for which the reference's own float32 run misses the bound against its float64 run
(`reference_misses`)."""
import numpy as np
import torch

G_LOGS = ("train_loss/g_loss",)
D_LOGS = ("train_loss/d_loss", "train_log/pred_real", "train_log/pred_fake")
MODES = ("vanilla", "lsgan", "hinge")
STEPS = 4
LR = 2e-4
BIAS_IN_FRONT = {"netG.network.1.running_mean": "netG.network.0.bias", "netG.network.4.running_mean": "netG.network.3.bias",
                 "netG.network.7.running_mean": "netG.network.6.bias", "netD.network.3.running_mean": "netD.network.2.bias",
                 "netD.network.6.running_mean": "netD.network.5.bias"}


def close_err(a, b, rel):
    """tests/test_aae_gpu.py::_close as (error, bound)."""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max()), rel * float(b.abs().max()) + 1e-5


def close(a, b, rel, what=""):
    err, bound = close_err(a, b, rel)
    assert err <= bound, f"{what}: max err {err:.3e} > bound {bound:.3e}"


def step_weights(key):
    """Per step of the trajectory, the total weight its momentum updates of running mean `key` carry in the final value.  G runs
    forward once per step; D once in a generator step (even) and twice in a discriminator step (odd)."""
    per_step = [1] * STEPS if key.startswith("netG.") else [1 if i % 2 == 0 else 2 for i in range(STEPS)]
    total, w, seen = sum(per_step), [], 0
    for n in per_step:
        w.append(sum(0.1 * 0.9 ** (total - 1 - j) for j in range(seen, seen + n)))
        seen += n
    return w


def bias_part(key, bias0, bias_after):
    """sum over steps of step_weights * the bias that step's forwards saw: the initial bias in step 0, then the bias after step i - 1."""
    seen = [np.asarray(bias0, dtype=np.float64)] + [np.asarray(b, dtype=np.float64) for b in bias_after[:STEPS - 1]]
    return sum(w * b for w, b in zip(step_weights(key), seen))


def ref_bias_after(g, tag, bias_key):
    return [g[f"traj.bias{tag}.{i}.{bias_key}"] for i in range(STEPS)]


def reference_misses(g):
    """The running means whose float32 reference run leaves its float64 run by more than the running statistics' bound."""
    out = []
    for k in g["tiny.names"]:
        if "running_" in k:
            err, bound = close_err(g[f"traj.sd32.{k}"], g[f"traj.sd64.{k}"], 1e-5)
            if err > bound:
                out.append(str(k))
    return out


def adam_tolerance(ref, g1, g3):
    """Per element, what two Adam updates (betas 0.5, 0.999) from gradients known to dg = 2e-4 max|g| + 1e-5 may differ by: the bound
    tests/test_aae_gpu.py derives for its encoder, which also takes two updates per step."""
    dg_of = lambda gr: 2e-4 * float(gr.abs().max()) + 1e-5                               # noqa: E731
    tol = torch.clamp(LR * dg_of(g1) / (g1.abs() + 1e-8), max=2 * LR) + 2e-7 * float(ref.abs().max())
    return tol + torch.clamp(2 * LR * (dg_of(g1) + dg_of(g3)) / (torch.maximum(g1.abs(), g3.abs()) + 1e-8), max=2.11 * LR)


def traj_param_grads(g, k):
    """The float64 run's two gradients of parameter k: steps 0 and 2 for the generator, 1 and 3 for the discriminator."""
    a, b = (0, 2) if k.startswith("netG.") else (1, 3)
    return torch.from_numpy(g[f"traj.grad64.{a}.{k}"]).double(), torch.from_numpy(g[f"traj.grad64.{b}.{k}"]).double()


def check_traj_state(g, sd, bias_after, what):
    """sd: a state_dict after the 4 steps; bias_after[bias key] = that bias after each step.  Against the float64 run: parameters within
    the two-update Adam bound, running statistics within 1e-5 * max|ref| + 1e-5, the bias part taken out where the reference misses."""
    misses = reference_misses(g)
    assert set(misses) <= set(BIAS_IN_FRONT), misses
    for k in g["tiny.names"]:
        k = str(k)
        ref = torch.from_numpy(g[f"traj.sd64.{k}"]).double()
        got = torch.as_tensor(sd[k]).detach().double().cpu()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(ref) == (4 if k.startswith("netG.") else 6), k
        elif "running_" in k:
            if k in misses:
                b = BIAS_IN_FRONT[k]
                scale = float(ref.abs().max())                                           # of the running mean itself, as in close()
                got = got - torch.from_numpy(bias_part(k, g["tiny.sd0." + b], bias_after[b]))
                ref = ref - torch.from_numpy(bias_part(k, g["tiny.sd0." + b], ref_bias_after(g, "64", b)))
                err = float((got - ref).abs().max())
                print(f"{what} {k} without its bias part: max err {err:.3e}, bound {1e-5 * scale + 1e-5:.3e}")
                assert err <= 1e-5 * scale + 1e-5, (what, k, err)
            else:
                close(got, ref, 1e-5, f"{what} {k}")
        else:
            tol = adam_tolerance(ref, *traj_param_grads(g, k))
            bad = (got - ref).abs() > tol
            assert not bool(bad.any()), (what, k, int(bad.sum()), float((got - ref).abs().max()))


def check_traj_logs(g, logs, what):
    """logs[i] = {key: value} of step i against the float64 run: tests/test_aae_gpu.py::_check_logs' bound."""
    for i in range(STEPS):
        keys = G_LOGS if i % 2 == 0 else D_LOGS
        assert set(logs[i]) == set(keys), (what, i)
        for key in keys:
            ref = float(g[f"traj.log64.{i}.{key}"])
            print(f"{what} step {i} {key}: {logs[i][key]:.8g} float64 reference {ref:.8g}")
            assert abs(logs[i][key] - ref) <= 1e-5 * abs(ref) + 1e-6, (what, i, key)
