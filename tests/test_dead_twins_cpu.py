"""Unet.dead_twins (which residual-stream tensors the training step writes as bf16 only) against the layer list: the rule keeps the fp32
twin wherever a reader takes fp32.  Host only: the plan is a function of _Arch and of the library's `*_supported` queries.

Readers, restated from _Arch: a tensor that enters a ResnetBlock is read as fp32 by an identity residual (cin == cout: no res_conv); the
last down level's attention output enters mid_block1 (cin == cout); a ResnetBlock's res1 output enters res2 (cin == cout) and is not in
the plan at all.  Geometries: cfg 2 (128 / 1-2-4, 32x32, B = 128), cfg 3 (64 / 1-2-4-8, 64x64, B = 32), MNIST (64 / 2-4, 1 channel,
28x28, B = 128)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GEOMS = {"cfg2": (dict(dim=128, dim_mults=(1, 2, 4), channels=3), 128, 32),
         "cfg3": (dict(dim=64, dim_mults=(1, 2, 4, 8), channels=3), 32, 64),
         "mnist": (dict(dim=64, dim_mults=(2, 4), channels=1), 128, 28)}
geoms = pytest.mark.parametrize("geom", list(GEOMS))


def _net(geom, mode="bf16", **attrs):
    from src.models.ddpm import Unet
    kw, B, size = GEOMS[geom]
    net = Unet(**kw)
    net.compute_mode = mode
    for k, v in attrs.items():
        setattr(net, k, v)
    return net, B, size


def _all_false(plan):
    return not (any(plan["down"]) or any(plan["attn_down"]) or plan["mid2"] or any(plan["attn_up"]) or any(plan["up"]))


def test_cfg2_plan():
    """the tensors of the benchmark's step: both Downsample and both Upsample outputs, the four attention outputs that feed them,
    mid_block2's output; the last level's attention output keeps its twin"""
    net, B, size = _net("cfg2")
    assert net.step_flow == "AB"
    assert net.dead_twins(B, size, size) == {"down": [True, True, False], "attn_down": [True, True, False], "mid2": True,
                                             "attn_up": [True, True], "up": [True, True]}


@geoms
def test_twin_stays_where_a_reader_takes_fp32(geom):
    net, B, size = _net(geom)
    A, plan = net._arch, net.dead_twins(B, size, size)
    nl = len(A.downs)
    assert len(plan["down"]) == len(plan["attn_down"]) == nl and len(plan["up"]) == len(plan["attn_up"]) == len(A.ups) == nl - 1
    # the last down level: no Downsample, and its attention output enters mid_block1, an identity residual
    assert A.downs[-1]["down"] is None and not A.mid1["res"]
    assert not plan["down"][-1] and not plan["attn_down"][-1]
    for L in range(nl - 1):
        nxt = A.downs[L + 1]["res1"]
        if not nxt["res"]:
            assert not plan["down"][L], f"downs.{L}'s Downsample output enters an identity residual"
        j = nl - 1 - L                                    # the up level that pops level L's skip (level 0's is never popped)
        if 0 <= j < len(A.ups) and not A.ups[j]["res1"]["res"]:
            assert not plan["attn_down"][L]
    if A.ups and not A.ups[0]["res1"]["res"]:
        assert not plan["mid2"]
    for j in range(len(A.ups) - 1):
        if not A.ups[j + 1]["res1"]["res"]:
            assert not plan["up"][j]
    if geom == "cfg3":                                    # 64 / 1-2-4-8: every res1 changes its width, so the rule is decided by the kernels
        assert all(b["res"] for b in [lvl["res1"] for lvl in A.downs + A.ups])
    if geom == "mnist":                                   # 28 -> 14 -> 7: no power-of-two grids, the stride-2 tile kernels decline
        assert not any(plan["attn_down"]) and not any(plan["attn_up"]) and not any(plan["down"]) and not any(plan["up"])


@geoms
def test_identity_residual_keeps_the_twin(geom):
    """the same layer list with every res_conv taken away (cin == cout everywhere a tensor enters a block): nothing that enters a
    ResnetBlock may lose its twin; the attention outputs that feed only a Downsample / Upsample are not affected"""
    net, B, size = _net(geom)
    ref = net.dead_twins(B, size, size)
    net2, _, _ = _net(geom)
    for blk in net2._arch.res_blocks:
        blk["res"] = False
    plan = net2.dead_twins(B, size, size)
    assert not any(plan["down"]) and not plan["mid2"] and not any(plan["up"][:-1])
    assert not any(plan["attn_down"][1:])
    assert plan["attn_down"][0] == ref["attn_down"][0] and plan["attn_up"] == ref["attn_up"]
    assert plan["up"][-1:] == ref["up"][-1:]              # the last Upsample feeds final_conv.0's conv, not a ResnetBlock


@geoms
def test_declining_kernels_keep_the_twin(geom, monkeypatch):
    """res_conv on the generic kernel reads the fp32 operands; a stride-2 weight gradient on the ring kernel converts the fp32 tensor"""
    import src.ops.functional as K
    net, B, size = _net(geom)
    monkeypatch.setattr(K, "conv1x1_tile_supported", lambda *a, **k: False)
    plan = net.dead_twins(B, size, size)
    assert not any(plan["down"]) and not plan["mid2"] and not any(plan["up"][:-1]) and not any(plan["attn_down"][1:])
    monkeypatch.undo()
    net, B, size = _net(geom)
    monkeypatch.setattr(K, "s2_wgrad_supported", lambda *a, **k: False)
    plan = net.dead_twins(B, size, size)
    assert not any(plan["attn_down"]) and not any(plan["attn_up"])
    monkeypatch.undo()
    net, B, size = _net(geom)
    monkeypatch.setattr(K, "conv_gt_supported", lambda *a, **k: False)
    plan = net.dead_twins(B, size, size)
    assert not any(plan["down"]) and not any(plan["up"])


@geoms
def test_unchanged_paths(geom):
    """fp32 mode, fp32 block storage, the parent's flow, a batch the bf16 storage does not take: every twin stays"""
    for kw in (dict(mode="fp32"), dict(block_storage="fp32"), dict(step_flow=""), dict(step_flow="A"), dict(dual_out=False, s2_wgrad_tr=False)):
        net, B, size = _net(geom, **kw)
        plan = net.dead_twins(B, size, size)
        if "dual_out" in kw:
            assert not any(plan["attn_down"]) and not any(plan["attn_up"]) and not any(plan["down"]) and not any(plan["up"])
        else:
            assert _all_false(plan), kw
    net, B, size = _net(geom)
    assert _all_false(net.dead_twins(B + 4, size, size))
