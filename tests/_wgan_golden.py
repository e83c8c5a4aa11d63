"""What tests/test_wgan_cpu.py and tests/test_wgan_clip_gpu.py share: the comparisons against tests/golden/wgan_clip_kats.npz (the
reference's own WGAN.training_step, tools/gen_golden_wgan_clip.py) in the manner of tests/_gan_golden.py, whose `close` / `close_err`
are used as they are.

The trajectory is 7 steps with n_critic = 2: G D D G D D G.  The generator takes 3 RMSprop updates, the critic 4, and the critic is
clipped to [-c, c] when every step begins.

Conv biases in front of a BatchNorm have an analytically zero gradient: what RMSprop gets is rounding noise, and from v = 0 its first
update is lr g / sqrt((1 - alpha) g^2) = lr / sqrt(1 - alpha) = 10 lr in that noise's direction, whatever its size (docs/kernels.md 4k).
The layer's output does not see it, its running MEAN does.  `bias_part` is the part of the final running mean that the biases
contributed, sum_j w_j b_j over the momentum updates j with b_j the bias AS THAT FORWARD SAW IT -- for the critic, after the step's
clip; the comparison takes it out on both sides, each side with its own biases, and keeps the bound.  It is applied only to the running
means for which the reference's own float32 run misses the bound against its float64 run (`reference_misses`)."""
import numpy as np
import torch

from _gan_golden import close, close_err  # noqa: F401

G_LOGS = ("train_loss/g_loss",)
D_LOGS = ("train_loss/d_loss", "train_log/real_logit", "train_log/fake_logit")
STEPS, N_CRITIC = 7, 2
LR, ALPHA, EPS, CLIP = 6e-4, 0.99, 1e-8, 0.1
G, D = "generator.", "discriminator."
# The trajectory does not stay on one smooth branch.  After the critic's third update the reference's float32 run hands its optimizer
# gradients that are up to 30 % away from its float64 run's in single elements although every parameter still agrees to 2e-5: the nets
# are tiny, the clipped critic's pre-norm activations are small (BatchNorm's 1 / std amplifies), and ReLU / LeakyReLU kinks flip.  From
# there on the two runs of the REFERENCE differ by up to 1e-3 in parameters and 6e-5 in the logged scalars -- more than any bound that
# assumes gradients good to 2e-4.  So every bound of the trajectory carries a second term, the project's yardstick form
# (tests/test_wgan_gpu.py): YARDSTICK times the distance of the reference's own float32 run from its float64 run in that same quantity
# (for the parameters: in the gradients, through the update's sensitivity).  The single steps from sd0 carry no such term.
YARDSTICK = 4.0
BIAS_IN_FRONT = {G + "network.1.running_mean": G + "network.0.bias", G + "network.4.running_mean": G + "network.3.bias",
                 G + "network.7.running_mean": G + "network.6.bias", D + "network.3.running_mean": D + "network.2.bias",
                 D + "network.6.running_mean": D + "network.5.bias"}


def is_g_step(i):
    return i % (N_CRITIC + 1) == 0


def update_steps(key):
    """The steps in which the net of `key` takes an optimizer update."""
    return [i for i in range(STEPS) if is_g_step(i) == key.startswith(G)]


def step_weights(key):
    """Per step of the trajectory, the total weight its momentum updates of running mean `key` carry in the final value.  G runs
    forward once per step; D once in a generator step and twice in a critic step."""
    per_step = [1] * STEPS if key.startswith(G) else [1 if is_g_step(i) else 2 for i in range(STEPS)]
    total, w, seen = sum(per_step), [], 0
    for n in per_step:
        w.append(sum(0.1 * 0.9 ** (total - 1 - j) for j in range(seen, seen + n)))
        seen += n
    return w


def bias_part(key, bias0, bias_after):
    """sum over steps of step_weights * the bias that step's forwards saw: the initial bias in step 0, then the bias after step i - 1;
    a critic bias as the step's clip left it."""
    seen = [np.asarray(bias0, dtype=np.float64)] + [np.asarray(b, dtype=np.float64) for b in bias_after[:STEPS - 1]]
    if key.startswith(D):
        seen = [np.clip(b, -CLIP, CLIP) for b in seen]
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


def rmsprop_tolerance(ref, grads, critic, own=None):
    """Per element, what the RMSprop updates (alpha, eps, lr as above, from v = 0) from the gradients `grads`, each known to
    dg_k = 2e-4 max|g_k| + 1e-5 (the repository's gradient tolerance, tests/test_gan_gpu.py), may differ by.  own[k], where given, is
    how far the reference's OWN float32 gradient of update k is from its float64 one (max over the tensor): dg_k is at least 4 times
    that, the yardstick form of tests/test_wgan_gpu.py -- see YARDSTICK above.
    Update k moves the element by lr g_k / (s_k + eps), s_k = sqrt(v_k) = the norm of (sqrt(w_kj) g_j)_j with w_kj = alpha^(k-j) (1 - alpha).
    A norm moves by at most the norm of the perturbation: |ds_k| <= sqrt(sum_j w_kj dg_j^2) =: ds_k, so
        |d(step k)| <= lr (dg_k + |g_k| ds_k / (s_k + eps)) / (max(s_k - ds_k, 0) + eps),
    and never more than twice the largest step there is, lr / sqrt(1 - alpha) (|g_k| <= s_k / sqrt(1 - alpha)) -- the whole bound for an
    element whose gradient is rounding noise.  The sum over the updates, plus float32's rounding of the parameter itself; the critic's
    parameters end inside [-c, c] (the last step's clip), so they never differ by more than 2 c."""
    dgs = [2e-4 * float(gr.abs().max()) + 1e-5 for gr in grads]
    if own is not None:
        dgs = [max(d, YARDSTICK * float(o)) for d, o in zip(dgs, own)]
    cap = 2 * LR / (1 - ALPHA) ** 0.5
    v = torch.zeros_like(grads[0])
    tol = torch.zeros_like(grads[0]) + 2e-7 * float(ref.abs().max())
    for k, gr in enumerate(grads):
        v = ALPHA * v + (1 - ALPHA) * gr * gr
        s = v.sqrt()
        ds = sum(ALPHA ** (k - j) * (1 - ALPHA) * dgs[j] ** 2 for j in range(k + 1)) ** 0.5
        b = LR * (dgs[k] + gr.abs() * ds / (s + EPS)) / (torch.clamp(s - ds, min=0) + EPS)
        tol = tol + torch.clamp(b, max=cap)
    return torch.clamp(tol, max=2 * CLIP) if critic else tol


def traj_param_grads(g, k):
    """The float64 run's gradients of parameter k, one per update of its net, and the float32 run's distance from each."""
    return ([torch.from_numpy(g[f"traj.grad64.{i}.{k}"]).double() for i in update_steps(k)],
            [float(g[f"traj.dgrad.{i}.{k}"]) for i in update_steps(k)])


def own_error(g, k, remove_bias_part=False):
    """max |float32 run - float64 run| of the reference's state tensor k after the trajectory."""
    a, b = g[f"traj.sd32.{k}"].astype(np.float64), g[f"traj.sd64.{k}"].astype(np.float64)
    if remove_bias_part:
        bk = BIAS_IN_FRONT[k]
        a = a - bias_part(k, g["tiny.sd0." + bk], ref_bias_after(g, "32", bk))
        b = b - bias_part(k, g["tiny.sd0." + bk], ref_bias_after(g, "64", bk))
    return float(np.abs(a - b).max())


def check_traj_state(g, sd, bias_after, what):
    """sd: a state_dict after the 7 steps; bias_after[bias key] = that bias after each step.  Against the float64 run: parameters within
    `rmsprop_tolerance`, running statistics within 1e-5 * max|ref| + 1e-5 plus the yardstick term, the bias part taken out where the
    reference misses.
    Returns the worst error / bound per tensor class."""
    misses = reference_misses(g)
    assert set(misses) <= set(BIAS_IN_FRONT), misses
    worst = {"parameters": 0.0, "bias in front of a norm": 0.0, "running statistics": 0.0, "running mean without its bias part": 0.0}
    for k in g["tiny.names"]:
        k = str(k)
        ref = torch.from_numpy(g[f"traj.sd64.{k}"]).double()
        got = torch.as_tensor(sd[k]).detach().double().cpu()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(ref) == (STEPS if k.startswith(G) else 3 + 2 * 4), k
        elif "running_" in k:
            if k in misses:
                b = BIAS_IN_FRONT[k]
                scale = float(ref.abs().max())                                           # of the running mean itself, as in close()
                got = got - torch.from_numpy(bias_part(k, g["tiny.sd0." + b], bias_after[b]))
                ref = ref - torch.from_numpy(bias_part(k, g["tiny.sd0." + b], ref_bias_after(g, "64", b)))
                err, bound = float((got - ref).abs().max()), 1e-5 * scale + 1e-5 + YARDSTICK * own_error(g, k, True)
                print(f"{what} {k} without its bias part: max err {err:.3e}, bound {bound:.3e}")
                worst["running mean without its bias part"] = max(worst["running mean without its bias part"], err / bound)
                assert err <= bound, (what, k, err)
            else:
                err, bound = close_err(got, ref, 1e-5)
                bound += YARDSTICK * own_error(g, k)
                worst["running statistics"] = max(worst["running statistics"], err / bound)
                assert err <= bound, (what, k, err, bound)
        else:
            grads, own = traj_param_grads(g, k)
            tol = rmsprop_tolerance(ref, grads, k.startswith(D), own)
            ratio = (got - ref).abs() / tol
            cls = "bias in front of a norm" if k in BIAS_IN_FRONT.values() else "parameters"
            worst[cls] = max(worst[cls], float(ratio.max()))
            bad = ratio > 1
            assert not bool(bad.any()), (what, k, int(bad.sum()), float((got - ref).abs().max()), float(ratio.max()))
    print(f"{what}: worst error / bound per tensor class: " + ", ".join(f"{c} {r:.3f}" for c, r in worst.items()))
    return worst


def check_traj_logs(g, logs, what):
    """logs[i] = {key: value} of step i against the float64 run: tests/_gan_golden.py::check_traj_logs' bound plus the yardstick term."""
    worst = 0.0
    for i in range(STEPS):
        keys = G_LOGS if is_g_step(i) else D_LOGS
        assert set(logs[i]) == set(keys), (what, i)
        for key in keys:
            ref = float(g[f"traj.log64.{i}.{key}"])
            print(f"{what} step {i} {key}: {logs[i][key]:.8g} float64 reference {ref:.8g}")
            bound = 1e-5 * abs(ref) + 1e-6 + YARDSTICK * abs(float(g[f"traj.log32.{i}.{key}"]) - ref)
            worst = max(worst, abs(logs[i][key] - ref) / bound)
            assert abs(logs[i][key] - ref) <= bound, (what, i, key, abs(logs[i][key] - ref), bound)
    print(f"{what}: worst error / bound of the logged scalars: {worst:.3f}")
    return worst
