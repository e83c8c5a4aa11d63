"""tests/_halo_oracle.py against independent facts, without a GPU: the restated planner against the library's own queries (the library
loads without a device) over every case of the lists and a few thousand random descriptors, refused ones among them; the instantiations
and edges the case lists must keep reaching, each case by the plan it names; every host-side refusal of conv3x3_halo.hip's entry points
by the text mi_last_error carries (a call without a device fails at the launch anyway, so only the message tells the requirement; the
pointers are made-up integers -- every refusal precedes the first dereference); the exactness conditions of the integer operand families;
and the float32 emulation's figure that the fused entry points' GPU bound is four times of.

Measured here (float32 emulation of the halo's staging against the rounding model, relative to sum |h| |w| + |bias|, worst over the fused
cases, the coef and sums forms, both storages of x and eight seeds, two for the large cases; not used as a bound beyond the rounded-up
figure in the oracle): 3.9e-4, at K = 32 where one of 288 terms can be a tenth of an output's sum (1.4e-4 at K = 64 and 1.0e-4 at K = 96)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _halo_oracle as O  # noqa: E402

F64 = torch.float64
ALL_CASES = O.CASES_3X3 + O.CASES_1X1 + O.CASES_SUMS


def _lib():
    from src.ops.lib import load_library
    return load_library()


def _cdesc(d):
    from src.ops.lib import MiConvDesc
    return ctypes.byref(MiConvDesc(**d._asdict()))


def _tile(lib, d, io):
    bm, ck, sk = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.mi_conv3x3_bf16w_tile(_cdesc(d), io, ctypes.byref(bm), ctypes.byref(ck), ctypes.byref(sk))
    return None if rc else (bm.value, ck.value, sk.value)


def _fused_tile(lib, d):
    bm, ck = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.mi_conv3x3_gn_mish_tile(_cdesc(d), ctypes.byref(bm), ctypes.byref(ck))
    return None if rc else (bm.value, ck.value)


# ---------------------------------------------------------------------------------------------------- planner
def _case_descs():
    out = []
    for c in ALL_CASES:
        out += [O.case_desc(c, 0), O.case_desc(c, 1, "ra"), O.case_desc(c, 0, dense=True)]
    return out + [O.fused_desc(c) for c in O.FUSED_CASES]


def test_restated_planner_is_the_library():
    lib = _lib()
    n_ok = n_refused = n_fused = 0
    for d in _case_descs() + O.random_descs(4000):
        c = _cdesc(d)
        want = O.q_tile(d)
        for io in range(4):
            assert _tile(lib, d, io) == want, (d, io)                  # (no split-K plan: the storage mode does not enter)
        assert want is None or want[2] == 0
        assert lib.mi_conv3x3_bf16w_supported(c) == O.q_supported(d) == int(want is not None), d
        assert lib.mi_conv3x3_bf16w_uses_splitk(c) == 0, d
        fw = O.q_fused_tile(d)
        assert _fused_tile(lib, d) == fw and lib.mi_conv3x3_gn_mish_supported(c) == int(fw is not None), d
        n_ok += want is not None
        n_refused += want is None
        n_fused += fw is not None
    assert n_ok > 1000 and n_refused > 500 and n_fused > 300          # the enumeration is neither all plans nor all refusals
    # the unsupported descriptors the issue names, one by one
    for d in [O.desc(2, 8, 3, 32, 32), O.desc(2, 8, 28, 32, 32), O.desc(2, 8, 65, 32, 32), O.desc(3, 6, 8, 32, 32), O.desc(3, 4, 4, 32, 32),
              O.desc(2, 8, 8, 48, 32), O.desc(2, 8, 8, 64, 32, K1=16), O.desc(2, 8, 8, 32, 30), O.desc(2, 8, 8, 32, 32, stride=2),
              O.desc(2, 8, 8, 32, 32, mode=0), O.desc(2, 8, 8, 32, 32, IH=16)]:
        assert O.halo_ok(d) is None and lib.mi_conv3x3_bf16w_supported(_cdesc(d)) == 0, d
    assert O.halo_ok(O.desc(4, 4, 4, 32, 32)) == (64, 32) and O.halo_ok(O.desc(2, 6, 8, 32, 32)) is None and O.halo_ok(O.desc(2, 8, 8, 32, 32)) == (64, 32)


def test_case_lists_reach_every_instantiation_and_edge():
    e = O.edges()
    missing = [k for k in O.REQUIRED_EDGES if k not in e]
    assert not missing, missing
    assert {k[5:] for k in e if k.startswith("inst:")} == {repr(i) for i in O.all_instantiations()}
    assert len(O.all_instantiations()) == 46
    names = [c.name for c in ALL_CASES + O.FUSED_CASES]
    assert len(names) == len(set(names))
    lib = _lib()
    for c in ALL_CASES:
        d = O.case_desc(c)
        f = O.launch_facts(d)
        assert O.plan_name(f) == c.plan, (c, O.plan_name(f))           # a case reaches the plan it is there for ...
        t = _tile(lib, d, 0)
        assert t is not None and t[:2] == (f.BM, f.CK), (c, t)          # ... by the library's own answer
        assert O.launch_facts(O.case_desc(c, 1, "ra")) == f            # direction and epilogue flags do not move the plan
        assert O.int_family_exact(c.K, 1 if f.ks == 1 else 9)
    for c in O.FUSED_CASES:
        f = O.launch_facts(O.fused_desc(c), True)
        assert O.plan_name(f) == c.plan and _fused_tile(lib, O.fused_desc(c)) == (f.BM, f.CK), c
        assert (c.K // c.G) % 16 == 0
    large = [c for c in O.CASES_3X3 + O.CASES_1X1 if O.is_large(c)]
    assert 8 <= len(large) <= 14 and all(c.K <= 128 for c in large + [c for c in O.CASES_SUMS + O.FUSED_CASES if O.is_large(c)]), large
    # the facts of the table that first listed these cases, spelled out
    facts = {c.name: O.launch_facts(O.case_desc(c)) for c in ALL_CASES}
    assert facts["wide64_qmap_2chunks"].qmap == 2 and facts["wide64_qmap_2chunks"].P == 4 and facts["t256_qmap_w16"].skew and facts["t256_qmap_w16"].TH == 16
    assert facts["w8tile_th8"].TH == 8 and not facts["w8tile_th8"].xmap and facts["w8tile_th4_xmap_two"].TH == 4 and facts["w8tile_th4_xmap_two"].xmap
    assert facts["w8tile_ti2"].TI == 2 and facts["t256_ti4"].TI == 4 and facts["t256_ti4"].HP == 400 and facts["ti4_two_tiles_nc36"].gx == 2
    assert facts["k1_t256"].qmap == 0 and facts["k1_t256_qmap_nc384"].qmap == 1 and facts["k1_t256_qmap_nc384"].grid == (600, 1, 1)
    # every kernel-side index the remaps produce stays inside the launch: xmap and qmap are permutations of the tiles
    for c in ALL_CASES + O.FUSED_CASES:
        f = O.launch_facts(O.fused_desc(c), True) if isinstance(c, O.Fused) else O.launch_facts(O.case_desc(c))
        if f.xmap:
            ids = sorted(((b & 7) + 8 * ((b >> 3) // f.tiles_per_img)) * f.tiles_per_img + (b >> 3) % f.tiles_per_img for b in range(f.gx))
            assert ids == list(range(f.gx)), c
        if f.qmap:
            ppx, cpq = f.gx // f.P, f.gy // f.Q
            ids = sorted((((i & 7) // f.Q) * ppx + (i >> 3) // cpq, ((i & 7) % f.Q) * cpq + (i >> 3) % cpq) for i in range(f.gx * f.gy))
            assert ids == [(x, y) for x in range(f.gx) for y in range(f.gy)], c


# ---------------------------------------------------------------------------------------------------- refusals
P0 = 0x7f0000001000          # a made-up, 4096-byte aligned address: never dereferenced


def test_refusals_name_the_requirement():
    lib = _lib()
    n = [0]

    def refused(rc, text, what):
        n[0] += 1
        assert rc != 0, ("accepted", what)
        msg = lib.mi_last_error().decode()
        assert text in msg, (what, msg)

    ok = O.desc(2, 8, 8, 64, 64)
    X, X2, Wp, B, R, Y, GS, Y16 = (P0 + i * 0x10000 for i in range(8))

    def io(d, x=X, x2=None, w=Wp, bias=B, res=None, y=Y, mode=0):
        return lib.mi_conv3x3_bf16w_io(_cdesc(d) if d is not None else None, x, x2, w, bias, res, y, mode, None)

    def plain(d, x=X, x2=None, w=Wp, bias=B, res=None, y=Y):
        return lib.mi_conv3x3_bf16w(_cdesc(d), x, x2, w, bias, res, y, None)

    def gns(d, y=Y, mode=0, gs=GS, res=None):
        return lib.mi_conv3x3_bf16w_io_gnsums(_cdesc(d), X, None, Wp, B, res, y, mode, gs, None)

    def dual(d, y16=Y16, ld16=64, mode=0, y=Y):
        return lib.mi_conv3x3_bf16w_io_dual(_cdesc(d), X, None, Wp, B, None, y, y16, ld16, mode, None)

    # ---- descriptors (through the fp32 entry, the storage entry and the tile query)
    for d in [ok._replace(OW=3, IW=3), ok._replace(OW=28, IW=28), ok._replace(OW=65, IW=65), ok._replace(N=3, OH=6, IH=6), ok._replace(N=3, OH=4, IH=4, OW=4, IW=4),
              ok._replace(K=48, K1=48, ldx=48), ok._replace(K1=16, ldx=16, ldx2=48), ok._replace(Nc=30, ldy=30), ok._replace(stride=2), ok._replace(mode=0),
              ok._replace(IH=16), ok._replace(KW=1), ok._replace(pad=0)]:
        assert O.dispatch_accepts(d, has_x2=True) == "descriptor not supported by the halo kernel", d
        refused(plain(d, x2=X2), "descriptor not supported by the halo kernel", d)
        refused(io(d, x2=X2, mode=3), "descriptor not supported by the halo kernel", d)
        assert _tile(lib, d, 0) is None and "descriptor not supported" in lib.mi_last_error().decode()
    # ---- halo_dispatch's arguments
    for kw in (dict(x=None), dict(w=None), dict(y=None)):
        refused(io(ok, **kw), "null argument", kw)
    two = ok._replace(K1=32, ldx=32, ldx2=32)
    assert O.dispatch_accepts(two) == "two-source split without x2" and O.dispatch_accepts(two, has_x2=True) is None
    refused(io(two), "two-source split without x2", "x2")
    for d, kw, acc in [(ok._replace(ldx=66), {}, {}), (two._replace(ldx2=34), dict(x2=X2), dict(has_x2=True)), (ok, dict(x=X + 8), dict(off=dict(x=8))),
                       (two, dict(x2=X2 + 4), dict(has_x2=True, off=dict(x2=4))), (ok, dict(w=Wp + 8), dict(off=dict(w=8)))]:
        assert O.dispatch_accepts(d, **acc) == "16-byte aligned with ld % 4 == 0", (d, acc)
        refused(io(d, **kw), "16-byte aligned with ld % 4 == 0", (d, kw))
    # ---- the epilogue's vector accesses
    for mode in range(4):
        assert O.dispatch_accepts(ok._replace(ldy=66), mode) == "ldy % 4 == 0"
        refused(io(ok._replace(ldy=66), mode=mode), "ldy % 4 == 0", ("ldy", mode))
        refused(io(ok._replace(ldr=66), res=R, mode=mode), "ldr % 4 == 0", ("ldr", mode))
        refused(io(ok, y=Y + 4, mode=mode), "y must be 16-byte aligned (8-byte for a bf16 output)", ("y + 4", mode))
        refused(io(ok._replace(ldr=64), res=R + 8, mode=mode), "residual and bias must be 16-byte aligned", ("res", mode))
        refused(io(ok, bias=B + 4, mode=mode), "residual and bias must be 16-byte aligned", ("bias", mode))
    assert O.dispatch_accepts(ok._replace(ldr=66)) is None and O.dispatch_accepts(ok._replace(ldr=66), has_res=True) == "ldy % 4 == 0"
    for mode in (0, 1):                                                   # an fp32 y needs 16 bytes, a bf16 y 8
        assert O.dispatch_accepts(ok, mode, off=dict(y=8)) == "y must be 16-byte aligned" and O.dispatch_accepts(ok, mode | 2, off=dict(y=8)) is None
        refused(io(ok, y=Y + 8, mode=mode), "y must be 16-byte aligned", ("y + 8", mode))
    refused(plain(ok._replace(ldy=66)), "ldy % 4 == 0", "plain ldy")
    refused(plain(ok, y=Y + 8), "y must be 16-byte aligned", "plain y")
    assert O.dispatch_accepts(ok, entry="gnsums", off=dict(gsum=4)) == "gsum must be 8-byte aligned"
    refused(gns(ok, gs=GS + 4), "gsum must be 8-byte aligned", "gsum + 4")
    # 1x1 goes through the same checks
    one = O.desc1(2, 8, 8, 64, 64)
    assert O.dispatch_accepts(one) is None
    refused(io(one._replace(ldy=66)), "ldy % 4 == 0", "1x1 ldy")
    refused(io(one, bias=B + 8), "residual and bias must be 16-byte aligned", "1x1 bias")
    # ---- the entry points' own conditions
    refused(io(ok, mode=4), "io in 0..3", "io 4")
    refused(io(ok, mode=-1), "io in 0..3", "io -1")
    refused(io(None), "io in 0..3", "null d")
    refused(io(ok._replace(KH=5, KW=5, pad=2)), "3x3 or 1x1", "5x5")
    assert O.dispatch_accepts(ok, 4) == "io in 0..3"
    for d, kw in [(ok._replace(Nc=40, ldy=40), {}), (ok._replace(N=4, OH=4, IH=4, OW=4, IW=4), {}), (ok, dict(gs=None)), (ok, dict(mode=4)), (one, {})]:
        assert O.dispatch_accepts(d, kw.get("mode", 0), entry="gnsums", null=("gsum",) if "gs" in kw else ()) == "mi_conv3x3_bf16w_io_gnsums"
        refused(gns(d, **kw), "mi_conv3x3_bf16w_io_gnsums: 3x3, io in 0..3, Nc % 16 == 0, H*W % 32 == 0", (d, kw))
    for kw in (dict(mode=2), dict(mode=3), dict(ld16=66), dict(y16=Y16 + 4), dict(y16=None)):
        refused(dual(ok, **kw), "mi_conv3x3_bf16w_io_dual: 3x3 or 1x1, fp32 y (io 0 or 1), 8-byte aligned bf16 copy with ldy16 % 4 == 0", kw)
    assert O.dispatch_accepts(ok, 2, entry="dual") == O.dispatch_accepts(ok, 0, entry="dual", ldy16=66) == O.dispatch_accepts(ok, entry="dual", off=dict(y16=4)) \
        == "mi_conv3x3_bf16w_io_dual"
    refused(dual(ok, y=Y + 8), "y must be 16-byte aligned", "dual y")
    # ---- fused
    COEF = P0 + 0x100000

    def fx(d=ok, x=X, coef=COEF, bias=B, y=Y, mode=0):
        return lib.mi_conv3x3_gn_mish(_cdesc(d), x, coef, Wp, bias, y, mode, None)

    def fs(d=ok, G=4, mode=0, te=None, ldt=0, ga=COEF, y=Y, bias=B):
        return lib.mi_conv3x3_gn_mish_sums(_cdesc(d), X, GS, ga, COEF, te, ldt, G, 1e-5, Wp, bias, y, mode, None)

    for d in (ok._replace(transposed=1), two, ok._replace(OW=3, IW=3), ok._replace(N=4, OH=4, IH=4, OW=4, IW=4)):       # (the last: only multi-image tiles)
        assert O.fused_plan(d) is None
        refused(fx(d), "descriptor not supported by the fused GroupNorm+Mish+Conv3x3 kernel", d)
        refused(fs(d), "descriptor not supported by the fused GroupNorm+Mish+Conv3x3 kernel", d)
        assert _fused_tile(lib, d) is None and "descriptor not supported by the fused kernel" in lib.mi_last_error().decode()
    for mode in (1, 2, 4):
        refused(fx(mode=mode), "io 0 or 3", mode)
        refused(fs(mode=mode), "io 0 or 3", mode)
    refused(fx(coef=None), "null coef", "coef")
    refused(fx(ok._replace(accumulate=1)), "alignment / accumulate", "accumulate")
    refused(fx(ok._replace(ldx=66)), "alignment / accumulate", "ldx")
    refused(fx(x=X + 4), "alignment / accumulate", "x")
    for G in (0, 3, 8, -2):                                               # G <= 0, K % G, K / G = 8
        refused(fs(G=G), "K / G must be a multiple of 16", G)
    refused(fs(te=COEF, ldt=66), "K / G must be a multiple of 16", "ldt")
    refused(fs(ga=COEF + 8), "16-byte aligned vectors", "gamma")
    for mode in (0, 3):
        refused(fx(ok._replace(ldy=66), mode=mode), "fused_go: ldy % 4 == 0", ("fused ldy", mode))
        refused(fs(ok._replace(ldy=66), mode=mode), "fused_go: ldy % 4 == 0", ("fused sums ldy", mode))
        refused(fx(y=Y + 4, mode=mode), "y must be 16-byte aligned (8-byte for a bf16 output)", ("fused y", mode))
        refused(fx(bias=B + 8, mode=mode), "fused_go: bias must be 16-byte aligned", ("fused bias", mode))
        refused(fs(bias=B + 4, mode=mode), "fused_go: bias must be 16-byte aligned", ("fused sums bias", mode))
    refused(fx(y=Y + 8, mode=0), "y must be 16-byte aligned", "fused fp32 y + 8")
    assert n[0] >= 100


# ---------------------------------------------------------------------------------------------------- operand families
def test_integer_families_are_exact_in_fp32():
    """|x| <= 4, |w| <= 3: every partial sum of 9 K products (and bias, residual, prior content of at most 4) is an integer below 2^24 in
    magnitude whatever the order; checked on the sums over |terms| of the heaviest small case and of a two-source 1x1 case."""
    assert O.int_family_exact(128) and O.int_family_exact(1024) and not O.int_family_exact(1 << 18)
    for c in (O.CASES_3X3[5], O.CASES_1X1[2]):
        ops = O.operands(c, "int")
        ab = O.base_reference(c, ops, absolute=True)
        assert float(ab.max()) + 12 < 2 ** 24 and bool((ab == ab.round()).all())
        assert float(ops["x"].abs().max()) == 4 and float(ops["G"].abs().max()) == 3 and bool((ops["prior"] != 0).all())


@pytest.mark.parametrize("case", [c for c in O.CASES_SUMS if not O.is_large(c)] + [O.CASES_SUMS[4]], ids=repr)
def test_unit_family_keeps_the_groupnorm_sums_exact(case):
    """... per workgroup, image and slab, with the sparse residual of 300 on top; and a bf16 output rounds some of those values, so sums of
    the unrounded values are other numbers."""
    c = case
    f = O.launch_facts(O.case_desc(c))
    ops = O.sums_operands(c, True)
    ref = O.base_reference(c, ops) + ops["bias"] + ops["res"]
    for out16 in (False, True):
        y = O.stored(ref, out16)
        assert O.unit_sums_exact(y, f.BM, c.H, c.W), c
    assert not torch.equal(O.gn_sums(O.stored(ref, True)), O.gn_sums(ref))


# ---------------------------------------------------------------------------------------------------- the fused entry points' figure
def _figure(c, seed, x_f32, sums_form):
    c = c._replace(N=min(c.N, 4))                                         # the figure is a per-element statistic: four samples of the large cases
    ops = O.fused_operands(c, x_f32)
    hm = O.fused_h(ops["x"], ops["sc"], ops["sh"], ops["tb"])
    he = O.halo_h_emul32(ops["x"], ops["sc"], ops["sh"], ops["tb"], seed, ops["beta"] if sums_form else None, c.G)
    ym, ye = O.conv_ref(hm, ops["G"], bias=ops["bias"]), O.conv_ref(he, ops["G"], bias=ops["bias"])
    scale = O.conv_ref(hm, ops["G"], bias=ops["bias"], absolute=True)
    return float(((ye - ym).abs() / scale.clamp_min(1e-300)).max()), float((he != hm).double().mean())


def test_fused_emulation_figure():
    """Re-measures the figure the GPU test's per-element bound is four times of.  An h element the emulation stores differently from the
    model is one bf16 ulp off; the share is printed, the figure is what counts."""
    worst = 0.0
    for c in O.FUSED_CASES:
        for seed, x_f32, sums_form in [(s_, f_, m_) for f_ in (False, True) for m_ in (False, True) for s_ in range(2 if O.is_large(c) else 8)]:
            fig, share = _figure(c, seed + 8 * sums_form, x_f32, sums_form)
            print(f"{c.name} seed {seed} {'fp32' if x_f32 else 'bf16'} x {'sums' if sums_form else 'coef'}: figure {fig:.3g}, h elements off the model {share:.3g}")
            worst = max(worst, fig)
    print("worst figure:", worst)
    assert worst <= O.FUSED_EMUL_FIGURE, worst              # the constant the GPU bound is four times of is not below the emulation
    assert worst >= O.FUSED_EMUL_FIGURE / 2, worst          # ... nor left far above it
