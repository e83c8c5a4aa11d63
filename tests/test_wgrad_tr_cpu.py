"""tests/_wgrad_oracle.py checked without a GPU: the float64 references against torch.autograd, the restated planners and *_supported
predicates against the library (which loads without a device), the invariants of balance_shares and of the workgroup maps, and the case
lists of tests/test_wgrad_tr_kernels_gpu.py against the edges they are there to reach (an edge lost in a later edit fails here)."""
import ctypes
import os
import random
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wgrad_oracle as O  # noqa: E402

F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    from src.ops.lib import load_library
    return load_library()


def cdesc(d):
    from src.ops.lib import MiWgradDesc
    return MiWgradDesc(**d)


def carr(ds):
    from src.ops.lib import MiWgradDesc
    return (MiWgradDesc * len(ds))(*[cdesc(d) for d in ds])


def iarr(v):
    return (ctypes.c_int * len(v))(*v)


# ---------------------------------------------------------------------------------------------------- references against autograd
def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("shape", [(2, 3, 5, 4, 6, 4), (1, 1, 8, 3, 2, 2), (3, 4, 2, 5, 3, 5)])
def test_wgrad3x3_ref_against_autograd(shape):
    N, H, W, Ci, Cj, I1 = shape
    x, dy = torch.randn(N, H, W, Ci, dtype=F64), torch.randn(N, H, W, Cj, dtype=F64)
    w = torch.zeros(Cj, Ci, 3, 3, dtype=F64, requires_grad=True)
    F.conv2d(_nchw(x), w, padding=1).backward(_nchw(dy))
    got = O.wgrad3x3_ref(x[..., :I1], dy, x[..., I1:] if I1 != Ci else None)
    assert O.rel(got, w.grad.permute(2, 3, 1, 0)) <= 1e-12


def test_wgrad1x1_ref_against_autograd():
    x, dy = torch.randn(2, 3, 5, 7, dtype=F64), torch.randn(2, 3, 5, 4, dtype=F64)
    w, b = torch.zeros(4, 7, 1, 1, dtype=F64, requires_grad=True), torch.zeros(4, dtype=F64, requires_grad=True)
    F.conv2d(_nchw(x), w, b).backward(_nchw(dy))
    dW, db = O.wgrad1x1_ref(x[..., :3], dy, x[..., 3:])
    assert O.rel(dW, w.grad[:, :, 0, 0].t()) <= 1e-12 and O.rel(db, b.grad) <= 1e-12
    # the matrix product may see another dY than the bias sum
    dW2, db2 = O.wgrad1x1_ref(x, dy, dy_dw=2 * dy)
    assert O.rel(dW2, 2 * dW) <= 1e-12 and torch.equal(db2, db)


@pytest.mark.parametrize("ks", [3, 4])
@pytest.mark.parametrize("gather_i", [1, 0])
@pytest.mark.parametrize("grid", [(2, 3, 4), (1, 1, 2)])
def test_wgrad_s2_ref_against_autograd(ks, gather_i, grid):
    N, h, w = grid
    Ci, Cj = 3, 5
    if gather_i:        # Conv2d(Ci, Cj, ks, 2, 1): [2h][2w] -> [h][w]
        x, dy = torch.randn(N, 2 * h, 2 * w, Ci, dtype=F64), torch.randn(N, h, w, Cj, dtype=F64)
        wt = torch.zeros(Cj, Ci, ks, ks, dtype=F64, requires_grad=True)
        y = F.conv2d(_nchw(x), wt, stride=2, padding=1)
        want = lambda g: g.permute(2, 3, 1, 0)  # noqa: E731
    else:               # ConvTranspose2d(Ci, Cj, ks, 2, 1): [h][w] -> [2h][2w]
        x, dy = torch.randn(N, h, w, Ci, dtype=F64), torch.randn(N, 2 * h, 2 * w, Cj, dtype=F64)
        wt = torch.zeros(Ci, Cj, ks, ks, dtype=F64, requires_grad=True)
        y = F.conv_transpose2d(_nchw(x), wt, stride=2, padding=1, output_padding=4 - ks)
        want = lambda g: g.permute(2, 3, 0, 1)  # noqa: E731
    assert y.shape[2:] == dy.shape[1:3]
    y.backward(_nchw(dy))
    assert O.rel(O.wgrad_s2_ref(x, dy, ks, gather_i), want(wt.grad)) <= 1e-12


def test_bf16_round_is_nearest_even():
    one, ulp = 1.0, 2.0 ** -7
    t = torch.tensor([one + ulp / 2, one + 3 * ulp / 2, one + ulp / 2 + 2.0 ** -20, -(one + ulp / 2), 3.0], dtype=F64)
    assert O.bf16_round(t).tolist() == [one, one + 2 * ulp, one + ulp, -one, 3.0]


# ---------------------------------------------------------------------------------------------------- balance_shares, maps
def test_balance_shares_invariants():
    rng = random.Random(7)
    for _ in range(2000):
        n = rng.randint(1, 8)
        tiles = [rng.choice((1, 1, 2, 3, 4, 6, 8, 12, 16, 24)) for _ in range(n)]
        work = [float(rng.randint(1, 1 << 20) * t) for t in tiles]
        target = rng.choice((1, 7, 9, 37, 64, 203, 256))
        wgs = O.balance_shares(work, tiles, target)
        assert all(w >= t and w % t == 0 for w, t in zip(wgs, tiles))
        assert sum(wgs) <= max(target, sum(tiles))
        # greedy to the end: nobody who still fits is more loaded than everybody else
        per = [wk / w for wk, w in zip(work, wgs)]
        fits = [i for i in range(n) if sum(wgs) + tiles[i] <= target]
        assert not fits or max(per[i] for i in fits) < max(per)


def test_workgroup_maps_are_permutations():
    for wg0 in range(16):
        for W in range(1, 70):
            assert sorted(O.rank_map(wg0, W, wg) for wg in range(W)) == list(range(W)), (wg0, W)
    # rank order = (XCD, order on that XCD)
    ranks = {O.rank_map(3, 21, wg): ((3 + wg) & 7, wg) for wg in range(21)}
    assert [ranks[r] for r in range(21)] == sorted(ranks.values())
    for c in O.TR_CASES:
        for a in O.tr_plan(O.tr_descs(c), c.blocks)["layers"]:
            seen = sorted(O.tr_wg_map(a, wg) for wg in range(a["ntiles"] * a["splits"]))
            assert seen == [(s, t) for s in range(a["splits"]) for t in range(a["ntiles"])], (c, a)


def test_s2f_groups():
    assert O.s2f_groups(9) == [(0, 5), (5, 4)] and O.s2f_groups(16) == [(0, 8), (8, 8)]


# ---------------------------------------------------------------------------------------------------- planners against the library
def test_splits_against_library(lib):
    try:
        for blocks in (0, 1, 2, 3, 5, 7, 8, 12, 24, 37, 203, 1000):
            lib.mi_debug_wgrad_tr_blocks(blocks)
            for layer in ((2, 24, 32, 64, 128), (5, 3, 64, 64, 64), (3, 16, 8, 128, 160, 64), (1, 8, 8, 64, 32), (127, 8, 8, 64, 32),
                          (8, 64, 64, 256, 416), (16, 32, 32, 128, 128)):
                for mode in (0, 1):
                    d = O.d3(*layer, mode=mode)
                    assert lib.mi_conv3x3_wgrad_tr_splits(ctypes.byref(cdesc(d))) == O.tr_plan([d], blocks)["layers"][0]["splits"], (blocks, layer)
        assert lib.mi_conv3x3_wgrad_tr_splits(ctypes.byref(cdesc(dict(O.d3(1, 8, 8, 64, 32), Cj=24)))) == 0
    finally:
        lib.mi_debug_wgrad_tr_blocks(0)


def _ws(lib, kind, descs, q32=None):
    if kind == "tr":
        return lib.mi_conv3x3_wgrad_tr_batch_workspace(len(descs), carr(descs))
    if kind == "w1":
        return lib.mi_conv1x1_wgrad_tr_batch_workspace(len(descs), carr(descs), iarr(q32))
    if kind == "s2":
        return lib.mi_conv_s2_wgrad_tr_batch_workspace(len(descs), carr(descs))
    return lib.mi_conv_s2_wgrad_f32_workspace(ctypes.byref(cdesc(descs[0])))


def test_case_workspaces_against_library(lib):
    try:
        for c in O.TR_CASES:
            lib.mi_debug_wgrad_tr_blocks(c.blocks)
            ds = O.tr_descs(c)
            assert _ws(lib, "tr", ds) == O.tr_plan(ds, c.blocks)["ws_bytes"], c
            if len(ds) == 1:
                assert lib.mi_conv3x3_wgrad_tr_workspace(ctypes.byref(cdesc(ds[0]))) == O.tr_plan(ds, c.blocks)["ws_bytes"]
        for c in O.W1_CASES:
            lib.mi_debug_wgrad1x1_tr_blocks(c.blocks)
            ds, q32 = O.w1_descs(c)
            assert _ws(lib, "w1", ds, q32) == O.w1_plan(ds, q32, c.blocks)["ws_bytes"], c
        lib.mi_debug_wgrad1x1_tr_blocks(0)
        for c in O.S2_CASES:
            ds = O.s2_descs(c)
            assert _ws(lib, "s2", ds) == O.s2_plan(ds)["ws_bytes"], c
        for c in O.S2F_CASES:
            d = O.s2f_desc(c)
            assert _ws(lib, "s2f", [d]) == O.s2f_plan(d)["ws_bytes"], c
    finally:
        lib.mi_debug_wgrad_tr_blocks(0)
        lib.mi_debug_wgrad1x1_tr_blocks(0)


def _rand_tr(rng, mode):
    W = rng.choice((8, 16, 32, 64))
    TR = 64 // W
    H = TR * rng.randint(1, 12)
    Ci = 64 * rng.randint(1, 8)
    return O.d3(rng.randint(1, 64) * (1 if H * W % 64 == 0 else 64), H, W, Ci, 32 * rng.randint(1, 16), 64 * rng.randint(1, Ci // 64), mode)


def _rand_w1(rng, mode):
    Ci = 64 * rng.randint(1, 8)
    return O.d1(rng.randint(1, 300), Ci, 32 * rng.randint(1, 16), 64 * rng.randint(1, Ci // 64), mode)


def _rand_s2(rng):
    w = rng.choice((8, 16, 32))
    h = (64 // w) * rng.randint(1, 12)
    ks = rng.choice((3, 4))
    big, small = 64 * rng.randint(1, 6), 32 * rng.randint(1, 12)
    Ci, Cj = (big, small) if ks == 3 else (small, big)
    return O.ds2(rng.randint(1, 32), h, w, Ci, Cj, ks, 1 if ks == 3 else 0)


def test_random_workspaces_against_library(lib):
    """About 200 random supported batches of 1 to 8 descriptors per entry point, byte for byte, under several block targets."""
    rng = random.Random(20240905)
    try:
        for i in range(200):
            n, blocks, mode = rng.randint(1, 8), rng.choice((0, 0, 9, 37, 64, 203)), rng.randint(0, 1)
            lib.mi_debug_wgrad_tr_blocks(blocks)
            lib.mi_debug_wgrad1x1_tr_blocks(blocks)
            ds = [_rand_tr(rng, mode) for _ in range(n)]
            assert all(O.tr_ok(d) for d in ds)
            assert _ws(lib, "tr", ds) == O.tr_plan(ds, blocks)["ws_bytes"], (i, blocks, ds)
            ds = [_rand_w1(rng, mode) for _ in range(n)]
            q32 = [1 if mode == 0 else rng.randint(0, 1) for _ in range(n)]
            assert all(O.w1_ok(d, q) for d, q in zip(ds, q32))
            assert _ws(lib, "w1", ds, q32) == O.w1_plan(ds, q32, blocks)["ws_bytes"], (i, blocks, ds, q32)
            ds = [_rand_s2(rng) for _ in range(n)]
            assert all(O.s2_ok(d) for d in ds)
            assert _ws(lib, "s2", ds) == O.s2_plan(ds)["ws_bytes"], (i, ds)
            lib.mi_debug_wgrad1x1_tr_blocks(0)
            d = O.ds2(rng.choice((1, 2, 3, 4, 16, 64)), rng.choice((8, 16, 32)), rng.choice((8, 16, 32)), 64 * rng.randint(1, 4), 32 * rng.randint(1, 8),
                      rng.choice((3, 4)), rng.randint(0, 1), mode=0)
            assert O.s2f_ok(d)
            assert _ws(lib, "s2f", [d]) == O.s2f_plan(d)["ws_bytes"], (i, d)
        # refused batches report no workspace
        bad = dict(O.d3(1, 8, 8, 64, 32), Cj=24)
        assert _ws(lib, "tr", [O.d3(1, 8, 8, 64, 32), bad]) == 0 and lib.mi_conv3x3_wgrad_tr_batch_workspace(9, carr([O.d3(1, 8, 8, 64, 32)] * 9)) == 0
        assert lib.mi_conv3x3_wgrad_tr_batch_workspace(0, carr([O.d3(1, 8, 8, 64, 32)])) == 0
    finally:
        lib.mi_debug_wgrad_tr_blocks(0)
        lib.mi_debug_wgrad1x1_tr_blocks(0)


# ---------------------------------------------------------------------------------------------------- *_supported truth tables
def _mutations(base):
    """Descriptors one or two fields away from a supported one: every reason the *_supported checks list, and their neighbours."""
    out = [base]
    grid = dict(DW=(4, 8, 16, 24, 32, 64, 128), DH=(1, 2, 3, 4, 5, 6, 8, 12, 16), N=(1, 2, 3, 4, 8), Ci=(32, 64, 96, 128, 192), I1=(0, 32, 64, 96, 128),
                Cj=(8, 16, 24, 32, 48, 64, 96, 100, 160), ldp=(64, 66, 68, 72, 136), ldp2=(0, 64, 66, 68, 72), ldq=(32, 34, 36, 40, 184),
                KH=(1, 3, 4, 5), KW=(1, 3, 4), stride=(1, 2, 3), pad=(0, 1, 2), gather_i=(0, 1), mode=(0, 1, 2), GH=(8, 16, 32), GW=(8, 16, 32))
    for k, vals in grid.items():
        for v in vals:
            d = dict(base)
            d[k] = v
            if k in ("DW", "DH") and base["stride"] == 1:
                d["G" + k[1]] = v                      # keep the grids equal: the geometry itself is under test
            elif k in ("DW", "DH"):
                d["G" + k[1]] = 2 * v
            out.append(d)
            for k2, v2 in (("N", 64), ("Ci", 128), ("mode", 1 - base["mode"] if base["mode"] in (0, 1) else 0)):
                out.append(dict(d, **{k2: v2}))
    return out


def test_supported_truth_tables(lib):
    n = 0
    for base in (O.d3(2, 8, 8, 128, 96, 64), O.d3(1, 4, 16, 64, 32, mode=0), O.d3(1, 2, 32, 64, 32), O.d3(1, 1, 64, 64, 32)):
        for d in _mutations(base):
            assert bool(lib.mi_conv3x3_wgrad_tr_supported(ctypes.byref(cdesc(d)))) == O.tr_ok(d), d
            n += 1
    for base in (O.d1(2, 128, 96, 64), O.d1(1, 64, 32, mode=0)):
        for d in _mutations(base):
            for q32 in (0, 1):
                assert bool(lib.mi_conv1x1_wgrad_tr_supported(ctypes.byref(cdesc(d)), q32)) == O.w1_ok(d, q32), (d, q32)
                n += 1
    for base in (O.ds2(2, 8, 8, 64, 96, 3, 1), O.ds2(1, 4, 16, 96, 64, 4, 0), O.ds2(2, 8, 8, 64, 96, 3, 1, mode=0), O.ds2(2, 8, 8, 64, 96, 4, 1, mode=0),
                 O.ds2(1, 2, 32, 64, 32, 3, 0, mode=0)):
        for d in _mutations(base):
            assert bool(lib.mi_conv_s2_wgrad_tr_supported(ctypes.byref(cdesc(d)))) == O.s2_ok(d), d
            assert bool(lib.mi_conv_s2_wgrad_f32_supported(ctypes.byref(cdesc(d)))) == O.s2f_ok(d), d
            n += 2
    assert n > 2000


def test_supported_reasons():
    """The restatement itself, reason by reason (so that it cannot agree with the library by being empty)."""
    b = O.d3(2, 8, 8, 128, 96, 64)
    assert O.tr_ok(b) and O.tr_ok(dict(b, mode=0, ldp=68, ldp2=84, ldq=100))
    for k, v in (("DW", 24), ("DW", 128), ("Ci", 96), ("I1", 32), ("Cj", 48), ("Cj", 16), ("ldp", 68), ("ldp2", 84), ("ldq", 100), ("KH", 1), ("stride", 2),
                 ("pad", 0), ("gather_i", 0), ("mode", 2), ("N", 3)):
        d = dict(b, **{k: v})
        if k == "DW":
            d["GW"] = v
        if k == "N":
            d.update(DH=1, GH=1)                      # N * H * W = 24
        assert not O.tr_ok(d), (k, v)
    assert not O.tr_ok(O.d3(1, 3, 32, 64, 32))      # H % (64 / W)
    assert O.tr_ok(dict(b, I1=128, ldp2=3))         # the pitch of an absent second source is not looked at
    w = O.d1(2, 128, 96, 64)
    assert O.w1_ok(w, 0) and O.w1_ok(w, 1) and O.w1_ok(dict(w, ldq=100), 1) and not O.w1_ok(dict(w, ldq=100), 0)
    assert not O.w1_ok(dict(w, mode=0), 0) and O.w1_ok(dict(w, mode=0), 1) and not O.w1_ok(dict(w, ldp=68), 1) and O.w1_ok(dict(w, mode=0, ldp=68), 1)
    s = O.ds2(2, 8, 8, 64, 96, 3, 1)
    assert O.s2_ok(s) and not O.s2f_ok(s) and O.s2f_ok(dict(s, mode=0)) and not O.s2_ok(dict(s, gather_i=0)) and O.s2f_ok(dict(s, mode=0, gather_i=0))
    assert not O.s2_ok(dict(s, DW=64, GW=128)) and not O.s2_ok(dict(s, Ci=96)) and O.s2_ok(dict(s, Cj=32)) and not O.s2_ok(dict(s, I1=0))
    assert O.s2_ok(O.ds2(2, 6, 32, 64, 96, 3, 1)) and not O.s2f_ok(O.ds2(2, 6, 32, 64, 96, 3, 1, mode=0))      # the power-of-two grid
    assert O.s2_ok(O.ds2(2, 8, 8, 96, 64, 4, 0)) and not O.s2_ok(O.ds2(2, 8, 8, 64, 96, 4, 0))                # 4x4: Cj is the big side


# ---------------------------------------------------------------------------------------------------- the case lists
REQUIRED = """
tr:one_step tr32:one_step tr:direct tr32:direct tr:ragged_co_32 tr:ragged_co_96 tr:H1_W64 tr32:H1_W64 tr:H2_W32 tr32:H2_W32 tr:H4_W16 tr32:H4_W16
tr:H8_W8 tr:H16_W8 tr32:H16_W8 tr:two_sources tr32:two_sources tr:H_not_pow2 tr32:H_not_pow2 tr:H24_W32 tr:H3_W64
tr:sps1 tr:sps2 tr:sps3 tr:sps5 tr:sps7 tr32:sps1 tr32:sps2 tr32:sps3 tr32:sps5 tr32:sps7 tr:short_last_slice tr32:short_last_slice
tr:slice_starts_inside_image tr:slice_crosses_images tr32:slice_crosses_images tr32:W64_halo_prefetch_inside_image
tr:xcd_map0 tr:xcd_map1 tr:xcd_map2 tr:reduce<2> tr:reduce<8> tr:batch1 tr:batch2 tr:batch3 tr:batch8 tr:mixed_W tr:unsplit_between_split
tr32:xcd_map0 tr32:xcd_map1 tr32:xcd_map2 tr32:reduce<2> tr32:reduce<8> tr32:batch1 tr32:batch2 tr32:batch3 tr32:batch8 tr32:mixed_W
tr32:unsplit_between_split tr32:P2_null_for_some tr:P2_null_for_some tr:W8 tr:W16 tr:W32 tr:W64 tr32:W8 tr32:W16 tr32:W32 tr32:W64
w1:<Q32=0,NI=1> w1:<Q32=0,NI=2> w1:<Q32=1,NI=1> w1:<Q32=1,NI=2> w1:f32 w1:Cj32 w1:Cj96 w1:Cj160 w1:Cj416
w1:Ci64_I1_64 w1:Ci128_I1_128 w1:Ci192_I1_192 w1:Ci256_I1_64 w1:Ci256_I1_192 w1:tile_straddles_sources
w1:<Q32=1,NI=1>:dbias_gx>1 w1:<Q32=1,NI=2>:dbias_gx>1 w1:f32:dbias_gx>1 w1:<Q32=1,NI=1>:dbias_split w1:<Q32=1,NI=2>:dbias_split w1:f32:dbias_split
w1:<Q32=1,NI=2>:direct w1:<Q32=0,NI=1>:direct w1:reduce_mixed_ni w1:batch_mixed_dY_types w1:batch_null_and_set_dbias w1:batch_split_and_unsplit
w1:rank_wg0_not_8 w1:rank_wgs_not_8 w1:reduce<2> w1:reduce<8> w1:xcd_map0 w1:xcd_map1 w1:unsplit_between_split w1:batch3 w1:batch6 w1:batch8
w1:<Q32=0,NI=1>:k1 w1:<Q32=0,NI=2>:k2 w1:<Q32=1,NI=1>:k3 w1:<Q32=1,NI=2>:k4 w1:<Q32=0,NI=2>:k5 w1:<Q32=1,NI=2>:k37 w1:<Q32=0,NI=1>:k37
w1:f32:k1 w1:f32:k3 w1:f32:k5 w1:f32:k37
s2:k3:w8 s2:k3:w16 s2:k3:w32 s2:k4:w8 s2:k4:w16 s2:k4:w32 s2:k3:one_step_w8 s2:k4:one_step_w8 s2:k3:one_step_w16 s2:k4:one_step_w16
s2:k3:h16_w8 s2:k4:h16_w8 s2:k3:h_not_pow2 s2:k4:h_not_pow2 s2:small32 s2:small96 s2:small160 s2:big64 s2:big128 s2:big192
s2:k3:direct s2:k4:direct s2:xcd_map0 s2:xcd_map1 s2:rank_wg0_not_8 s2:rank_wgs_not_8 s2:reduce<2> s2:reduce<8> s2:unsplit_between_split
s2:k3:sps2 s2:k4:sps3 s2:k3:slice_crosses_images s2:k4:short_last_slice
s2:batch1 s2:batch2 s2:batch3 s2:batch8 s2:k3:slice_starts_inside_image s2:k4:slice_starts_inside_image
s2f:k3_gather1 s2f:k3_gather0 s2f:k4_gather1 s2f:k4_gather0 s2f:grid1x8x8 s2f:grid4x2x8 s2f:grid2x4x16 s2f:grid3x8x8 s2f:ragged_Cj s2f:split
s2f:groups_differ_in_workspace s2f:second_group_needs_more s2f:grid64x8x8
""".split()


def test_case_lists_reach_every_edge():
    reached = O.edges()
    required = set(REQUIRED)
    # every tail length of each reduce instantiation, behind the 8-wide main loop for <8> (64+ k-slices always enter it) and for <2>
    for tag in ("tr", "tr32", "w1", "s2"):
        required |= {f"{tag}:reduce<8>:tail{t}+main" for t in range(8)} | {f"{tag}:reduce<2>:tail{t}" for t in range(1, 8)}
        required |= {f"{tag}:reduce<2>:tail0+main", f"{tag}:reduce<2>:tail1+main", f"{tag}:reduce<2>:tail7+main"}
    # slices of the H = 24, W = 32 problem start at every row phase
    required |= {f"tr:row_phase_{k}of12" for k in range(1, 12)} | {f"tr32:row_phase_{k}of12" for k in range(1, 12)}
    assert not sorted(required - reached)


def test_case_names_are_unique_and_sizes_small():
    for cases in (O.TR_CASES, O.W1_CASES, O.S2_CASES, O.S2F_CASES):
        names = [c.name for c in cases]
        assert len(names) == len(set(names))
        for c in cases:
            assert 1 <= len(c.layers) <= O.MAXP
            for l in c.layers:
                npix = l[0] * l[1] * l[2] if cases is not O.W1_CASES else 64 * l[0]
                Ci, Cj = (l[3], l[4]) if cases is not O.W1_CASES else (l[1], l[2])
                assert npix <= 8192 and Ci <= 256 and Cj <= 416, c
                # the integer cases stay exact: |x| <= 4, |dy| <= 3, initial content |.| <= 3
                assert npix * 4 * 3 + 3 < 2 ** 24
    assert float(O.init_content(1000).abs().max()) <= 3 and bool((O.init_content(1000) != 0).any())
    p, q = O.operands((64, 8), (64, 8), "int", 1, True, True)
    assert float(p.abs().max()) == 4 and float(q.abs().max()) == 3 and torch.equal(O.bf16_round(p), p)
    p, q = O.operands((64, 8), (64, 8), "randn", 1, True, False)
    assert torch.equal(O.bf16_round(p), p) and not torch.equal(O.bf16_round(q), q) and torch.equal(q.float().double(), q)
