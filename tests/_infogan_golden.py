"""What tests/test_infogan_cpu.py and tests/test_infogan_gpu.py share: the comparisons against tests/golden/infogan_kats.npz (the
reference's own InfoGAN.training_step, tools/gen_golden_infogan.py), with the helpers and tolerances of tests/_gan_golden.py --
imported from there, not copied.

The trajectory is 3 batches = 6 phases (0, 1, 0, 1, 0, 1): every stepped parameter takes THREE Adam updates, each at its net's own
learning rate (netG lrG, netQ lrQ, netD and common_layer lrD).  tests/_gan_golden.py::adam_tolerance is the bound for two updates at
LR = 2e-4; every term of it but the 2e-7 * max|ref| floor is proportional to the learning rate, so it is taken at another rate by
scaling those terms.  The third update gets a term of the same construction:
  update 3 = lr * mhat / (sqrt(vhat) + eps) with mhat = (4 g3 + 2 g2 + g1) / 7 (b1 = 0.5) and vhat = mean(g^2) up to 0.1 % (b2 = 0.999).
  By Cauchy-Schwarz |mhat| / sqrt(vhat) <= sqrt(3 * 21) / 7 = 1.134, so two runs' third updates differ by at most 2.27 lr: the clamp.
  With sqrt(vhat) >= max|g| / sqrt(3), d(mhat / sqrt(vhat)) / d g_i <= (sqrt(3) w_i + 1.134) / max|g| (w_i the weights of mhat), which
  summed against gradient errors dg_i is at most (sqrt(3) * 4 / 7 + 1.134) * sum(dg_i) / max|g| = 2.13 sum(dg) / max|g|: the factor 3 below is the
  "k sum(dg) / max|g| for update k" of the two terms before it and covers that.
dg is the gradient tolerance of the single-step tests, 2e-4 max|g| + 1e-5, as in adam_tolerance.

Where a gradient is tiny all three terms sit at their clamps, about 6.4 lr per element (for netG at 1e-3 that checks nothing, as
adam_tolerance's 4.1 LR checks nothing there): those elements are rounding noise under Adam in the reference too.  What pins them is
the single-phase tests of tests/test_infogan_gpu.py -- the gradient handed to the optimizer within 2e-4 max|g| + 1e-5 and one update
within its bound -- and, for the biases in front of a BatchNorm, the running means below.

Conv biases in front of a BatchNorm random-walk under Adam and show in that layer's running MEAN (tests/_gan_golden.py explains);
`bias_part` is taken out on both sides, only for the running means where the reference's own float32 run misses the bound.

`step_weights`, `bias_part`, `ref_bias_after` and `reference_misses` below restate tests/_gan_golden.py's functions of the same
names rather than import them: those are written against that module's constants (STEPS = 4, the G, D, G, D pattern, the `netD.`
prefix) and take no parameters for them, and an existing test file is not edited by a change that adds a model.  Here the count is
PHASES = 6, the pattern is phase 0 / phase 1 per batch and the encoder is `common_layer.`.  What does not depend on those constants
(`close`, `close_err`, `adam_tolerance`) is imported."""
import numpy as np
import torch

import _gan_golden as GG

P0_LOGS = ("train_loss/g_loss", "train_loss/I_discrete_loss", "train_loss/I_continuous")
P1_LOGS = ("train_loss/d_loss", "train_log/pred_real", "train_log/pred_fake")
PHASES = 6
BIAS_IN_FRONT = {"netG.network.1.running_mean": "netG.network.0.bias", "netG.network.4.running_mean": "netG.network.3.bias",
                 "netG.network.7.running_mean": "netG.network.6.bias", "common_layer.network.3.running_mean": "common_layer.network.2.bias",
                 "common_layer.network.6.running_mean": "common_layer.network.5.bias"}
close, close_err = GG.close, GG.close_err


def lr_of(g, key):
    return float(g["traj.lrG"] if key.startswith("netG.") else g["traj.lrQ"] if key.startswith("netQ.") else g["traj.lrD"])


def stepped_in(key):
    """The phases whose optimizer steps parameter `key`."""
    return (0, 2, 4) if key.startswith(("netG.", "netQ.")) else (1, 3, 5)


def step_weights(key):
    """Per phase, the total weight its momentum updates of running mean `key` carry in the final value.  G runs forward once per
    phase; the common layer once in phase 0 and twice (real, fake) in phase 1."""
    per_phase = [1] * PHASES if key.startswith("netG.") else [1 if i % 2 == 0 else 2 for i in range(PHASES)]
    total, w, seen = sum(per_phase), [], 0
    for n in per_phase:
        w.append(sum(0.1 * 0.9 ** (total - 1 - j) for j in range(seen, seen + n)))
        seen += n
    return w


def bias_part(key, bias0, bias_after):
    """sum over phases of step_weights * the bias that phase's forwards saw: the initial bias in phase 0, then the bias after phase i - 1."""
    seen = [np.asarray(bias0, dtype=np.float64)] + [np.asarray(b, dtype=np.float64) for b in bias_after[:PHASES - 1]]
    return sum(w * b for w, b in zip(step_weights(key), seen))


def ref_bias_after(g, tag, bias_key):
    return [g[f"traj.bias{tag}.{i}.{bias_key}"] for i in range(PHASES)]


def reference_misses(g):
    """The running statistics whose float32 reference run leaves its float64 run by more than the running statistics' bound."""
    out = []
    for k in g["tiny.names"]:
        if "running_" in k:
            err, bound = close_err(g[f"traj.sd32.{k}"], g[f"traj.sd64.{k}"], 1e-5)
            if err > bound:
                out.append(str(k))
    return out


def adam_tolerance3(ref, g1, g2, g3, lr):
    """Per element, what three Adam updates (betas 0.5, 0.999) at `lr` from gradients known to dg may differ by (the docstring)."""
    floor = 2e-7 * float(ref.abs().max())
    two = floor + (GG.adam_tolerance(ref, g1, g2) - floor) * (lr / GG.LR)
    dg = sum(2e-4 * float(x.abs().max()) + 1e-5 for x in (g1, g2, g3))
    gmax = torch.maximum(torch.maximum(g1.abs(), g2.abs()), g3.abs())
    return two + torch.clamp(3 * lr * dg / (gmax + 1e-8), max=2.27 * lr)


def traj_param_grads(g, k):
    return [torch.from_numpy(g[f"traj.grad64.{i}.{k}"]).double() for i in stepped_in(k)]


def check_traj_state(g, sd, bias_after, what):
    """sd: a state_dict after the 6 phases; bias_after[bias key] = that bias after each phase.  Against the float64 run."""
    misses = reference_misses(g)
    assert set(misses) <= set(BIAS_IN_FRONT), misses
    for k in g["tiny.names"]:
        k = str(k)
        ref = torch.from_numpy(g[f"traj.sd64.{k}"]).double()
        got = torch.as_tensor(sd[k]).detach().double().cpu()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(ref) == int(g["traj.nbt.netG"] if k.startswith("netG.") else g["traj.nbt.common_layer"]), k
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
            tol = adam_tolerance3(ref, *traj_param_grads(g, k), lr_of(g, k))
            bad = (got - ref).abs() > tol
            print(f"{what} {k}: max err {float((got - ref).abs().max()):.3e}, lr {lr_of(g, k):g}, elements over the bound {int(bad.sum())}")
            assert not bool(bad.any()), (what, k, int(bad.sum()), float((got - ref).abs().max()))


def check_traj_logs(g, logs, what):
    """logs[i] = {key: value} of phase i against the float64 run: tests/_gan_golden.py::check_traj_logs' bound."""
    for i in range(PHASES):
        keys = P0_LOGS if i % 2 == 0 else P1_LOGS
        assert set(logs[i]) == set(keys), (what, i)
        for key in keys:
            ref = float(g[f"traj.log64.{i}.{key}"])
            print(f"{what} phase {i} {key}: {logs[i][key]:.8g} float64 reference {ref:.8g}")
            assert abs(logs[i][key] - ref) <= 1e-5 * abs(ref) + 1e-6, (what, i, key)
