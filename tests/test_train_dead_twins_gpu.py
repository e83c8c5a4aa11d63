"""The training step's data flow (Unet.step_flow = "AB", the default) against the parent's (step_flow = ""): the dim-32 / 1-2-4 UNet
in bf16 mode at B = 8, 32x32 and 16x16, forward_nhwc + backward_nhwc on one fixed batch and output gradient.

  "A": the channel LayerNorm's backward writes grad[inp] out of place, the 1x1 weight gradients are no longer flushed per attention block;
  "B": residual-stream tensors no reader takes as fp32 (Unet.dead_twins) are written as bf16 only.

Neither changes a rounding: EVERY tensor on the tape is compared bit for bit (a bf16-only tensor against the parent's bf16 copy, which is
the round-to-nearest-even of the fp32 twin), eps too; the 3x3 and stride-2 weight gradients are bit-equal (fixed-order sums over the
same operands).  The 1x1 weight gradients' k-slice plans change with the number of layers per launch, so they -- and the bias gradient
that rides with them -- are held to the project's bounds (tests/test_wgrad_tr_kernels_gpu.py: rel-L2 <= 2e-5, dbias <= 1e-5) against
the float64 product of the operands the queue was handed, and to the same 2e-5 against the parent's flow."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _util import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SIZES = [32, 16]
sizes = pytest.mark.parametrize("size", SIZES, ids=[f"b8-{s}" for s in SIZES])
_CACHE = {}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _net(flow):
    from src.models.ddpm import Unet
    torch.manual_seed(0)
    net = Unet(dim=32, dim_mults=(1, 2, 4), channels=3)
    net.compute_mode = "bf16"
    net.step_flow = flow
    return net.to(DEV).train()


def _batch(size):
    import src.ops.functional as K
    gen = torch.Generator().manual_seed(11 + size)
    x = torch.rand(8, 3, size, size, generator=gen) * 2 - 1
    t = torch.randint(0, 1000, (8,), generator=gen)
    d = torch.randn(8, 3, size, size, generator=gen) / (8 * 3 * size * size)
    return K.nchw_to_nhwc(x.to(DEV)), t.to(DEV), K.nchw_to_nhwc(d.to(DEV))


def _step(net, batch, spy=None):
    """one eager forward + backward -> (eps, tape, flat_grads clone, 1x1 launches, pushed 1x1 operands, offsets of the weight
    gradients that went through conv_wgrad: the generic kernels, whose k-slices are added atomically)"""
    import src.ops.functional as K
    x, t, d = batch
    pushed, orig = [], K.WgradQueue.push1x1
    atomic, orig_wgrad = set(), K.conv_wgrad

    def conv_wgrad(P, Q, dW, **kw):
        atomic.add((dW.data_ptr() - net.flat_grads.data_ptr()) // 4)
        return orig_wgrad(P, Q, dW, **kw)

    def push1x1(self, P, Q, dW, **kw):
        n = self.pushed
        orig(self, P, Q, dW, **kw)
        if self.pushed > n:                                 # deferred (not the conv_wgrad fallback); the operands as they are NOW
            pushed.append([P.clone(), None if kw.get("P2") is None else kw["P2"].clone(), Q.clone(), dW, kw.get("dbias")])
    net.flat_grads.fill_(float("nan"))
    K.PROBE = []
    try:
        K.conv_wgrad = conv_wgrad
        if spy:
            K.WgradQueue.push1x1 = push1x1
        eps, tape = net.forward_nhwc(x, t, record=True)
        net.backward_nhwc(tape, d)
        torch.cuda.synchronize()
        launches = sum(1 for q in K.PROBE if q[0] == "wgrad1x1_tr_kernel")
        for it in pushed:                                   # (views of flat_grads: what THIS pass left there)
            it[3], it[4] = it[3].clone(), None if it[4] is None else it[4].clone()
    finally:
        K.PROBE = None
        K.WgradQueue.push1x1 = orig
        K.conv_wgrad = orig_wgrad
    return eps, tape, net.flat_grads.clone(), launches, pushed, atomic


def _runs(size):
    """parent flow and new flow on the same weights and batch, computed once per size"""
    if size not in _CACHE:
        batch = _batch(size)
        old, new = _net(""), _net("AB")
        assert torch.equal(old.flat_params, new.flat_params)
        _CACHE[size] = (batch, old, new, _step(old, batch), _step(new, batch, spy=True))
    return _CACHE[size]


def _records(net, tape):
    """name -> the recorded tensor that Unet.dead_twins speaks of"""
    A, out = net._arch, {}
    for rec in tape:
        for L, lvl in enumerate(A.downs):
            if rec[0] == "attn" and rec[1] is lvl["attn"]:
                out[("attn_down", L)] = rec[8]
            if rec[0] == "down" and rec[1] is lvl["down"]:
                out[("down", L)] = rec[3]
        for j, lvl in enumerate(A.ups):
            if rec[0] == "attn" and rec[1] is lvl["attn"]:
                out[("attn_up", j)] = rec[8]
            if rec[0] == "up" and rec[1] is lvl["up"]:
                out[("up", j)] = rec[3]
        if rec[0] == "res" and rec[1] is A.mid2:
            out[("mid2", 0)] = rec[9]
    return out


@sizes
def test_forward_bits_and_tape(size):
    batch, old, new, (eps0, tape0, *_), (eps1, tape1, *_) = _runs(size)
    assert torch.equal(_bits(eps0), _bits(eps1)), "eps differs from the parent's flow"
    assert bool(torch.isfinite(eps1).all())
    # the tape holds bf16 tensors exactly where the rule says no reader takes fp32, and the fp32 twin nowhere
    plan = new.dead_twins(8, size, size)
    flat = {(k, i): v for k in ("down", "attn_down", "attn_up", "up") for i, v in enumerate(plan[k])}
    flat[("mid2", 0)] = plan["mid2"]
    # (32x32: a Downsample and an Upsample output, two attention outputs, mid_block2's output; 16x16: the first two and mid_block2's)
    assert sum(flat.values()) == (5 if size == 32 else 3), plan
    assert not any(v for v in old.dead_twins(8, size, size)["down"]) and not old.dead_twins(8, size, size)["mid2"]
    r0, r1 = _records(old, tape0), _records(new, tape1)
    for key, dead in flat.items():
        if key in r1:
            assert r0[key].dtype == torch.float32, key
            assert r1[key].dtype == (BF if dead else torch.float32), (key, dead, r1[key].dtype)
    s16 = next(rec[1] for rec in tape1 if rec[0] == "stream16")
    assert len(s16) == sum(flat.values()) and all(t.dtype == BF for t in s16)
    assert next(rec[1] for rec in tape0 if rec[0] == "stream16") == []
    ids16 = {id(t) for t in s16}
    # every recorded tensor, bit for bit; a bf16-only tensor against the parent's copy = RNE of the parent's fp32 tensor
    assert [r[0] for r in tape0] == [r[0] for r in tape1]
    n = 0
    for a, b in zip(tape0, tape1):
        for i, (u, v) in enumerate(zip(a, b)):
            if not (torch.is_tensor(u) and torch.is_tensor(v)):
                continue
            if u.dtype != v.dtype:
                assert id(v) in ids16 and u.dtype == torch.float32, (a[0], i)
                u = u.to(BF)
            elif u.dtype == torch.float32 and v.dtype == torch.float32:
                assert id(v) not in ids16
            assert torch.equal(_bits(u), _bits(v)), (a[0], i)
            n += 1
    assert n > 100
    # the parent's own bf16 copies of those tensors (what its consumers read) are the same bits
    for a, b in zip(tape0, tape1):
        if a[0] in ("down", "up") and b[2].dtype == BF:
            assert a[4] is not None and torch.equal(_bits(a[4]), _bits(b[2])), a[0]
            assert b[4] is b[2], "the consumer is handed the tensor itself"


@sizes
def test_gradients(size):
    batch, old, new, (_, _, g0, n0, _, at0), (_, _, g1, n1, pushed, at1) = _runs(size)
    assert at0 == at1, "the two flows send different layers to the generic weight-gradient kernel"
    assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(g0).all())
    one = exact = 0
    for e in new._arch.entries:
        a, b = g0[e.offset:e.offset + e.numel], g1[e.offset:e.offset + e.numel]
        if e.layout in ("conv", "convT"):
            kh, kw, ci, co = e.storage_view(new._flat).shape
            if kh >= 3 and ci % 64 == 0 and co >= 32 and e.offset not in at1:
                # 3x3 Block convs, Downsample (3x3 / 2), Upsample (4x4 / 2) on the batched LDS-DMA kernels: fixed-order sums
                assert torch.equal(_bits(a + 0.0), _bits(b + 0.0)), e.key
                exact += 1
            elif kh >= 3:
                # the same operands through a kernel that adds its k-slices atomically (the 3-channel end, Ci = 32, the fallbacks): two
                # summation orders, each within the project's bound of the float64 sum
                assert rel_err(b, a) <= 2e-5, (e.key, rel_err(b, a))
            else:
                assert rel_err(b, a) <= 2e-5, (e.key, rel_err(b, a))
                one += 1
    assert one >= 12 and exact >= (10 if size == 32 else 4), (one, exact)
    # against float64 on the operands the queue was handed
    assert len(pushed) >= 4, len(pushed)
    nb = 0
    for P, P2, Q, dW, dbias in pushed:
        X = P.flatten(0, 2).double() if P2 is None else torch.cat([P.flatten(0, 2), P2.flatten(0, 2)], 1).double()
        # (bf16 mode rounds an fp32 dY for the product, not for the bias sum: tests/test_wgrad_tr_kernels_gpu.py)
        ref = X.t() @ Q.flatten(0, 2).to(BF).double()                   # [Ci][Cj], the storage layout [1][1][Ci][Cj]
        assert rel_err(dW.reshape(ref.shape), ref) <= 2e-5, rel_err(dW.reshape(ref.shape), ref)
        if dbias is not None:
            assert rel_err(dbias, Q.flatten(0, 2).double().sum(0)) <= 1e-5
            nb += 1
    assert nb >= 2
    # fewer 1x1 weight-gradient launches than attention blocks (the parent: one flush per block)
    nattn = len(new._arch.downs) + 1 + len(new._arch.ups)
    assert 1 <= n1 < nattn and n1 < n0, (n0, n1, nattn)
    assert n1 == -(-len(pushed) // 8), (n1, len(pushed))


@sizes
def test_captured_step(size):
    """forward + backward captured as one graph: three replays, flat_grads NaN before each, give the eager pass's fixed-order sums."""
    batch, old, new, _, (eps1, _, g1, *_) = _runs(size)
    x, t, d = batch
    fixed = torch.zeros(new._arch.flat_numel, dtype=torch.bool)
    for e in new._arch.entries:
        if e.layout in ("conv", "convT"):
            kh, kw, ci, co = e.storage_view(new._flat).shape
            if ci % 64 == 0 and co >= 32:              # the batched LDS-DMA kernels' layers (1x1 included: the plan is the same from pass to pass)
                fixed[e.offset:e.offset + e.numel] = True
    eager = _step(new, batch)[2].cpu()
    again = _step(new, batch)[2].cpu()
    fixed &= (_bits(eager) == _bits(again)).cpu()       # (layers that took an atomic fallback are not fixed-order)
    assert int(fixed.sum()) > 100000
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            eps, tape = new.forward_nhwc(x, t, record=True)
            new.backward_nhwc(tape, d)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        new.flat_grads.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = new.flat_grads.cpu()
        assert bool(torch.isfinite(got).all())
        assert torch.equal(_bits(eps), _bits(eps1))
        assert torch.equal(_bits(got[fixed]), _bits(eager[fixed]))
        assert rel_err(got, g1) <= 2e-5


@sizes
def test_grad_ready_hook_ranges(size):
    """Data parallel: every record's range is reported exactly once, and holds its final bits when it is (after its last writer)."""
    batch, old, new, _, (_, _, g1, *_) = _runs(size)
    x, t, d = batch
    seen = []
    try:
        new.grad_ready_hook = lambda lo, hi: seen.append((lo, hi, new.flat_grads[lo:hi].clone()))
        new.flat_grads.fill_(float("nan"))
        eps, tape = new.forward_nhwc(x, t, record=True)
        new.backward_nhwc(tape, d)
    finally:
        new.grad_ready_hook = None
    torch.cuda.synchronize()
    final = new.flat_grads.clone()
    assert bool(torch.isfinite(final).all())
    A = new._arch
    want = [A.final_range, A.time_range] + [b["range"] for b in A.res_blocks] + [A.mid_attn["range"]]
    for lvl in A.downs + A.ups:
        want.append(lvl["attn"]["range"])
        want += [lvl[k]["range"] for k in ("down", "up") if lvl.get(k)]
    assert sorted((lo, hi) for lo, hi, _ in seen) == sorted(tuple(r) for r in want)
    for lo, hi, snap in seen:
        assert torch.equal(_bits(snap), _bits(final[lo:hi])), (lo, hi)
    assert rel_err(final, g1) <= 2e-5
