"""A recording stand-in for libmi_ddpm and the call lists that drive src/ops/functional.py through it on CPU tensors: every shape
question and every launch wrapper that builds a MiConvDesc / MiWgradDesc.  tools/gen_golden_functional.py writes what the stand-in
recorded to tests/golden/functional_descs.json; tests/test_functional_queries_cpu.py replays the lists and compares.

A recorded call is [entry point, [field values of each descriptor argument], [every plain int / float argument]]; pointers, streams and
out-parameters are left out (they differ from run to run)."""
import contextlib
import ctypes as C

import torch

QUERY_SUFFIXES = ("_supported", "_tile", "_uses_splitk", "_splitk", "_workspace", "_splits", "_part_rows")


class StubLib:
    """Every attribute is an entry point that records its call.  Launches return 0 (success); a query returns answers[name], or
    answers["*"] when the name is not listed."""

    def __init__(self, answers=None):
        self.calls = []
        self.answers = {"*": 1} if answers is None else dict(answers)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def entry(*args):
            descs, nums = [], []
            for a in args:
                _note(a, descs, nums)
            self.calls.append([name, descs, nums])
            if name in self.answers:
                return self.answers[name]
            return self.answers["*"] if name.endswith(QUERY_SUFFIXES) else 0
        return entry

    def names(self):
        return [c[0] for c in self.calls]


def _fields(d):
    return [getattr(d, f) for f, _ in d._fields_]


def _note(a, descs, nums):
    if hasattr(a, "_obj"):                              # C.byref(x): a descriptor, or an out-parameter (not recorded)
        a = a._obj
        if not isinstance(a, C.Structure):
            return
    if isinstance(a, C.Structure):
        descs.append(_fields(a))
    elif isinstance(a, C.Array):
        if issubclass(a._type_, C.Structure):
            descs.extend(_fields(x) for x in a)
        elif a._type_ is C.c_int:
            nums.extend(int(x) for x in a)
    elif isinstance(a, (bool, int)):
        nums.append(int(a))
    elif isinstance(a, float):
        nums.append(a)


FLAGS = dict(USE_CONV_PW=True, USE_CONV_GT=True, USE_WGRAD_TR=True, PW_MIN_TILES=64, PROBE=None)


@contextlib.contextmanager
def stubbed(K, answers=None):
    """functional.py on the stand-in: load_library, the GPU check, the stream and the workspace replaced, the module switches at their
    defaults, every cached answer dropped on the way in and on the way out."""
    stub = StubLib(answers)
    new = dict(FLAGS, load_library=lambda: stub, _need_gpu=lambda t: None, _stream=lambda: C.c_void_p(0),
               _workspace=lambda device, nbytes: torch.empty(max((int(nbytes) + 3) // 4, 1)))
    old = {k: getattr(K, k) for k in new}
    for k, v in new.items():
        setattr(K, k, v)
    clear_all(K)
    try:
        yield stub
    finally:
        for k, v in old.items():
            setattr(K, k, v)
        clear_all(K)


def clear_all(K):
    """K._QUERY_CACHE.clear() -- and, where a function still carries a cache of its own, that one too (so that the generator can run
    on a commit that has such functions)."""
    K._QUERY_CACHE.clear()
    for name in QUESTION_NAMES + ("conv_s2_wgrad_f32",):
        own = getattr(getattr(K, name), "cache_clear", None)
        if own is not None:
            own()


# ------------------------------------------------------------------------------------------------------------------ shape questions
# cfg 2 (dim 128, mults 1-2-4, 32x32) at B = 16, the MNIST net (dim 64, mults 2-4, 28 / 14 / 7), a two-source layer (K1 < K: the skip concat).
B = 16
C3 = [(B, 32, 32, 128, 128), (B, 16, 16, 128, 256), (B, 16, 16, 256, 256), (B, 8, 8, 256, 512), (B, 8, 8, 512, 512),
      (B, 28, 28, 128, 128), (B, 14, 14, 128, 256), (B, 7, 7, 256, 256)]
C3_2SRC = [(B, 16, 16, 512, 256, 256), (B, 32, 32, 256, 128, 128), (B, 14, 14, 384, 128, 256)]
YES_NO = [{"*": 0}, {"*": 1}]
SIZES = [{"*": 0}, {"*": 4096}]
TILES = [{"*": 0}, {"*": 64}, {"*": 128}]
CONV_WGRAD = [{"mi_conv3x3_bf16w_supported": c, "mi_conv3x3_wgrad_supported": w} for c in (0, 1) for w in (0, 1)]

# name -> (answer settings, [(args, kwargs)]); the last entries of a list are shapes the Python side or the library refuses
QUESTIONS = {
    "_linattn_ws": (SIZES, [((B, n, 4), {}) for n in (1024, 256, 64, 784, 196, 49)]),
    "_cvt_colsum_ws": (SIZES, [((B * 1024, 128), {}), ((B * 256, 256), {}), ((B * 64, 512), {}), ((B * 784, 128), {}), ((B * 49, 256), {})]),
    "igemm_bf16_in_supported": (YES_NO, [((128, 128, 3, 2, False, 1, (16, 16)), {}), ((256, 256, 3, 2, False, 1, (8, 8)), {}),
                                         ((256, 256, 4, 2, True, 1, (16, 16)), {}), ((128, 128, 4, 2, True, 1, (32, 32)), {}),
                                         ((128, 128, 3, 2, False, 0, (8, 8)), {}), ((128, 128, 3, 2, False, 1, (14, 14)), {}),
                                         ((256, 256, 4, 2, True, 1, (14, 14)), {}), ((100, 60, 3, 2, False, 1, (8, 8)), {})]),
    "conv3x3_gn_mish_supported": (YES_NO, [(s, {}) for s in C3] + [((B, 8, 8, 100, 60), {})]),
    "conv3x3_pw_gn_mish_picked": (TILES, [(s, {}) for s in C3] + [((B, 8, 8, 1024, 512), {}), ((1, 8, 8, 128, 128), {})]),
    "small_cin_supported": (YES_NO, [((3, 3, 128), {}), ((1, 3, 128), {}), ((3, 1, 128), {}), ((3, 3, 128, True), {}), ((3, 3, 128), {"wgrad": True}),
                                     ((3, 1, 128), {"wgrad": True}), ((3, 3, 96), {"wgrad": True}), ((5, 3, 64), {}), ((3, 3, 2048), {})]),
    "small_cin_bf16_supported": (YES_NO, [((3, B, 32, 32, 3, 128, 4), {}), ((1, B, 32, 32, 3, 128, 4), {}), ((3, B, 28, 28, 1, 128, 4), {}),
                                          ((3, B, 32, 32, 3, 96, 3), {})]),
    "small_cout_gn_supported": (YES_NO, [((128, 3, 8), {}), ((128, 1, 8), {}), ((64, 3, 8), {}), ((100, 3, 7), {})]),
    "small_cin_dual_supported": (YES_NO, [((B, 32, 32, 3, 128, 4), {}), ((B, 28, 28, 1, 128, 4), {}), ((B, 32, 32, 3, 96, 3), {})]),
    "small_cout_supported": (YES_NO, [((op, Cc, Cs), {}) for op in (0, 1, 2) for Cc, Cs in ((128, 3), (256, 3), (32, 1), (48, 3), (128, 5))]),
    "conv_gt_supported": (YES_NO, [((B, 32, 32, 128, 128, 3, False), {}), ((B, 16, 16, 256, 256, 3, False), {}), ((B, 8, 8, 256, 256, 4, True), {}),
                                   ((B, 16, 16, 128, 128, 4, True), {}), ((B, 28, 28, 128, 128, 3, False), {}), ((B, 14, 14, 128, 128, 3, False), {}),
                                   ((B, 7, 7, 256, 256, 4, True), {}), ((B, 32, 32, 128, 100, 3, False), {})]),
    "fast3x3_supported": (CONV_WGRAD, [(s, {}) for s in C3 + C3_2SRC] + [((B, 8, 8, 100, 60), {})]),
    "fast1x1_supported": (CONV_WGRAD, [((B, 32, 32, 128, 384), {}), ((B, 32, 32, 128, 128), {}), ((B, 16, 16, 256, 384), {}), ((B, 8, 8, 512, 384), {}),
                                       ((B, 28, 28, 128, 384), {}), ((B, 14, 14, 128, 256), {}), ((B, 7, 7, 256, 384), {}), ((B, 8, 8, 100, 60), {})]),
    "conv1x1_tile_supported": (YES_NO, [((B, 32, 32, 128, 128), {}), ((B, 16, 16, 128, 256), {}), ((B, 14, 14, 128, 256), {})]
                               + [(s, {}) for s in C3_2SRC] + [((B, 8, 8, 100, 60, 36), {})]),
    "conv3x3_uses_splitk": (YES_NO, [(s, {}) for s in C3 + C3_2SRC] + [((B, 8, 8, 100, 60), {})]),
    "s2_wgrad_supported": (YES_NO, [((B, 3, 128, 128, False, (32, 32), (16, 16), 1), {}), ((B, 3, 256, 256, False, (16, 16), (8, 8), 1), {}),
                                    ((B, 4, 256, 256, True, (16, 16), (8, 8), 1), {}), ((B, 4, 128, 128, True, (32, 32), (16, 16), 1), {}),
                                    ((B, 3, 128, 128, False, (28, 28), (14, 14), 1), {}), ((B, 4, 256, 256, True, (14, 14), (7, 7), 1), {}),
                                    ((B, 3, 128, 128, False, (32, 32), (16, 16), 0), {}), ((B, 3, 100, 60, False, (6, 6), (3, 3), 1), {})]),
}
QUESTION_NAMES = tuple(QUESTIONS)
NO_FFI = ("small_cin_supported", "small_cout_supported")


def _plain(r):
    """a returned value as JSON holds it, its type kept: True != 1 in the comparison"""
    if isinstance(r, tuple):
        return {"tuple": [_plain(x) for x in r]}
    if isinstance(r, torch.Tensor):
        return {"tensor": [list(r.shape), list(r.stride()), str(r.dtype)]}
    return {type(r).__name__: r}


def replay_questions(K):
    """-> [[label, recorded calls, returned value]]: every question once per (answer setting, shape), from an empty cache."""
    out = []
    for name, (settings, shapes) in QUESTIONS.items():
        for answers in settings:
            for args, kw in shapes:
                with stubbed(K, answers) as stub:
                    r = getattr(K, name)(*args, **kw)
                out.append([f"{name}{args}{kw or ''} {answers}", stub.calls, _plain(r)])
    return out


# ------------------------------------------------------------------------------------------------------------------ launch wrappers
F32, BF = torch.float32, torch.bfloat16


def act(n, h, w, c, dt=F32, pitch=None):
    """NHWC activation; pitch: a channel slice of a wider tensor"""
    return torch.zeros(n, h, w, c if pitch is None else pitch, dtype=dt)[..., :c]


def _gn(N, Cc, groups, temb=True):
    return (torch.zeros(N * (Cc // 16) * 2, dtype=torch.int64), torch.ones(Cc), torch.zeros(Cc), torch.zeros(N, Cc) if temb else None, groups, 1e-5)


def _sums(N, Nc):
    return torch.zeros(N * (Nc // 16) * 2, dtype=torch.int64)


def _queue(K, kind, store=False):
    """two layers of one kind through a WgradQueue of group 2 (the second push flushes), then the final flush"""
    q = K.WgradQueue(group=2, store=store)
    dt = BF
    for i in range(2):
        if kind == 3:
            q.push(act(2, 8, 8, 128, dt), act(2, 8, 8, 256, dt), torch.zeros(9 * 128 * 256), Ci=128, Cj=256, hw=(8, 8), mode=K.MODE_BF16, prefill=store)
        elif kind == "3two":
            q.push(act(2, 8, 8, 128, dt), act(2, 8, 8, 128, dt), torch.zeros(9 * 384 * 128), Ci=384, Cj=128, hw=(8, 8), mode=K.MODE_BF16,
                   P2=act(2, 8, 8, 256, dt, pitch=320))
        elif kind == "3f32":
            q.push(act(2, 8, 8, 128), act(2, 8, 8, 128), torch.zeros(9 * 128 * 128), Ci=128, Cj=128, hw=(8, 8), mode=K.MODE_FP32)
        elif kind == 1:
            q.push1x1(act(2, 8, 8, 128, dt), act(2, 8, 8, 384, F32 if i else dt), torch.zeros(128 * 384), Ci=128, Cj=384, hw=(8, 8), mode=K.MODE_BF16,
                      dbias=torch.zeros(384) if i else None)
        elif kind == "1f32":
            q.push1x1(act(2, 8, 8, 128), act(2, 8, 8, 128), torch.zeros(128 * 128), Ci=128, Cj=128, hw=(8, 8), mode=K.MODE_FP32,
                      P2=None, dbias=torch.zeros(128))
        elif kind == 2:
            if i:
                q.push_s2(act(2, 8, 8, 128, dt), act(2, 16, 16, 128, dt), torch.zeros(16 * 128 * 128), k=4, Ci=128, Cj=128, gather_i=False,
                          grid_g=(16, 16), grid_d=(8, 8), mode=K.MODE_BF16)
            else:
                q.push_s2(act(2, 16, 16, 128, dt, pitch=160), act(2, 8, 8, 128, dt), torch.zeros(9 * 128 * 128), k=3, Ci=128, Cj=128, gather_i=True,
                          grid_g=(16, 16), grid_d=(8, 8), mode=K.MODE_BF16)
    q.flush()
    return q.pushed


def wrapper_cases(K):
    """-> [(label, answers, thunk)]"""
    M16, M32 = K.MODE_BF16, K.MODE_FP32
    wq = torch.zeros(8)
    gt = dict(kh=3, kw=3, stride=2, pad=1, transposed=False, K=128, Nc=128, out_hw=(8, 8))
    gtT = dict(kh=4, kw=4, stride=2, pad=1, transposed=True, K=128, Nc=256, out_hw=(16, 16))
    ig = dict(kh=3, kw=3, stride=2, pad=1, transposed=False, w_kn=False, K=128, Nc=128, out_hw=(8, 8))
    c3 = dict(K=128, Nc=128, flip=False)
    big = lambda dt: act(16, 16, 16, 128, dt)          # noqa: E731  (4096 pixels: 64 tiles of 64 pixels)
    wg = dict(kh=3, kw=3, stride=1, pad=1, gather_i=True, Ci=128, Cj=256, grid_g=(8, 8), grid_d=(8, 8))
    s2d = dict(k=3, Ci=64, Cj=64, gather_i=True, grid_g=(16, 16), grid_d=(8, 8))
    s2u = dict(k=4, Ci=64, Cj=64, gather_i=False, grid_g=(16, 16), grid_d=(8, 8))
    no_pw = {"*": 1, "mi_conv3x3_pw_tile": 0, "mi_conv3x3_pw_x32_tile": 0, "mi_conv1x1_pw_supported": 0, "mi_conv1x1_pw_x32_supported": 0}
    tile64 = {"*": 1, "mi_conv3x3_pw_tile": 64, "mi_conv3x3_pw_x32_tile": 64, "mi_conv3x3_pw_gn_mish_tile": 64, "mi_conv3x3_pw_x32_gn_mish_tile": 128}
    no_fused = {"*": 1, "mi_conv3x3_pw_gn_mish_tile": 0, "mi_conv3x3_pw_x32_gn_mish_tile": 0}
    return [
        # the tap-gather kernel
        ("conv_gt plain", None, lambda: K.conv_gt(act(2, 16, 16, 128, BF), wq, **gt)),
        ("conv_gt bf16 out", None, lambda: K.conv_gt(act(2, 16, 16, 128, BF), wq, out_dtype=BF, bias=torch.zeros(128), **gt)),
        ("conv_gt residual, pitched out, accumulate", None,
         lambda: K.conv_gt(act(2, 16, 16, 128, BF, pitch=192), wq, residual=act(2, 8, 8, 128, pitch=136), out=act(2, 8, 8, 128, pitch=256), accumulate=True, **gt)),
        ("conv_gt want16", None, lambda: K.conv_gt(act(2, 16, 16, 128, BF), wq, want16=True, **gt)),
        ("conv_gt fp32 transposed", None, lambda: K.conv_gt(act(2, 8, 8, 128), wq, mode=M32, **gtT)),
        ("conv_gt out pitch % 8", None, lambda: K.conv_gt(act(2, 16, 16, 128, BF), wq, out=act(2, 8, 8, 128, pitch=132), **gt)),
        ("conv_gt refused", {"*": 0}, lambda: K.conv_gt(act(2, 16, 16, 128, BF), wq, **gt)),
        # the generic implicit GEMM
        ("conv_igemm fp32", None, lambda: K.conv_igemm(act(2, 16, 16, 128), wq, mode=M32, **ig)),
        ("conv_igemm two sources, residual", None,
         lambda: K.conv_igemm(act(2, 16, 16, 96), wq, mode=M16, x2=act(2, 16, 16, 32, pitch=48), residual=act(2, 8, 8, 128), bias=torch.zeros(128), **ig)),
        ("conv_igemm bf16 weights, accumulate", None, lambda: K.conv_igemm(act(2, 16, 16, 128), wq, mode=M16, wb=wq, out=act(2, 8, 8, 128, pitch=160), accumulate=True, **ig)),
        ("conv_igemm bf16 in", None, lambda: K.conv_igemm(act(2, 16, 16, 128, BF), wq, mode=M16, wb=wq, **ig)),
        ("conv_igemm ragged Nc", None, lambda: K.conv_igemm(act(2, 8, 8, 128), wq, mode=M32, **dict(ig, kh=1, kw=1, stride=1, pad=0, Nc=3))),
        # conv3x3_bf16w, arm by arm
        ("bf16w refused", {"*": 0}, lambda: K.conv3x3_bf16w(act(2, 8, 8, 128, BF), wq, wq=wq, **c3)),
        ("bf16w 1x1 stream", None, lambda: K.conv3x3_bf16w(act(2, 8, 8, 128, BF), wq, ksize=1, wq=wq, **c3)),
        ("bf16w 1x1 stream want16, two sources, residual", None,
         lambda: K.conv3x3_bf16w(act(2, 8, 8, 128, BF), wq, ksize=1, wq=wq, x2=act(2, 8, 8, 128, BF, pitch=384), residual=act(2, 8, 8, 64), want16=True,
                                 K=256, Nc=64, flip=False)),
        ("bf16w 1x1 stream bf16 out, flip, accumulate", None,
         lambda: K.conv3x3_bf16w(act(2, 8, 8, 128, BF), wq, ksize=1, wq=wq, out=act(2, 8, 8, 128, BF, pitch=256), accumulate=True, K=128, Nc=128, flip=True)),
        ("bf16w 1x1 fp32 in", None, lambda: K.conv3x3_bf16w(act(2, 8, 8, 128), wq, ksize=1, wq=wq, residual=act(2, 8, 8, 128), **c3)),
        ("bf16w 1x1 halo (K % 128)", None, lambda: K.conv3x3_bf16w(act(2, 8, 8, 64, BF), wq, ksize=1, wq=wq, K=64, Nc=128, flip=False)),
        ("bf16w 1x1 halo (stream refuses)", no_pw, lambda: K.conv3x3_bf16w(act(2, 8, 8, 128, BF), wq, ksize=1, wq=wq, want16=True, **c3)),
        ("bf16w 3x3 fp32 in, pw", tile64, lambda: K.conv3x3_bf16w(big(F32), wq, wq=wq, bias=torch.zeros(128), **c3)),
        ("bf16w 3x3 fp32 in, pw, gn_sums, bf16 out", tile64, lambda: K.conv3x3_bf16w(big(F32), wq, wq=wq, gn_sums=_sums(16, 128), out_dtype=BF, **c3)),
        ("bf16w 3x3 fp32 in, too few tiles", tile64, lambda: K.conv3x3_bf16w(act(2, 8, 8, 128), wq, wq=wq, **c3)),
        ("bf16w 3x3 fp32 in, no tile", no_pw, lambda: K.conv3x3_bf16w(big(F32), wq, wq=wq, **c3)),
        ("bf16w 3x3 fp32 in, pitch % 4", tile64, lambda: K.conv3x3_bf16w(act(16, 16, 16, 128, F32, pitch=130), wq, wq=wq, **c3)),
        ("bf16w 3x3 pw gn_sums", tile64, lambda: K.conv3x3_bf16w(big(BF), wq, wq=wq, gn_sums=_sums(16, 128), out_dtype=BF, **c3)),
        ("bf16w 3x3 pw gn_sums refused -> halo", dict(tile64, mi_conv3x3_pw_supported=0), lambda: K.conv3x3_bf16w(big(BF), wq, wq=wq, gn_sums=_sums(16, 128), **c3)),
        ("bf16w 3x3 pw", tile64, lambda: K.conv3x3_bf16w(big(BF), wq, wq=wq, residual=act(16, 16, 16, 128, BF), out_dtype=BF, **c3)),
        ("bf16w 3x3 pw two sources, flip, accumulate, pitched out", tile64,
         lambda: K.conv3x3_bf16w(act(16, 16, 16, 64, BF), wq, wq=wq, x2=act(16, 16, 16, 64, BF, pitch=96), out=act(16, 16, 16, 128, pitch=144), accumulate=True,
                                 K=128, Nc=128, flip=True)),
        ("bf16w 3x3 pw, 128-pixel tiles too few", dict(tile64, mi_conv3x3_pw_tile=128), lambda: K.conv3x3_bf16w(big(BF), wq, wq=wq, **c3)),
        ("bf16w 3x3 halo want16", tile64, lambda: K.conv3x3_bf16w(big(BF), wq, wq=wq, want16=True, **c3)),
        ("bf16w 3x3 halo no wq, bf16 in", None, lambda: K.conv3x3_bf16w(act(2, 8, 8, 128, BF), wq, **c3)),
        ("bf16w 3x3 halo fp32 in and out", None, lambda: K.conv3x3_bf16w(act(2, 8, 8, 128), wq, residual=act(2, 8, 8, 128, pitch=200), **c3)),
        ("bf16w 3x3 halo gn_sums", None, lambda: K.conv3x3_bf16w(act(2, 8, 8, 128, BF), wq, gn_sums=_sums(2, 128), out_dtype=BF, **c3)),
        ("bf16w 3x3 halo two sources, accumulate", no_pw,
         lambda: K.conv3x3_bf16w(act(2, 8, 8, 96), wq, wq=wq, x2=act(2, 8, 8, 32, pitch=64), out=act(2, 8, 8, 128, pitch=256), accumulate=True, **c3)),
        # GroupNorm + Mish + conv
        ("gn_mish pw, coef", tile64, lambda: K.conv3x3_gn_mish(big(BF), torch.zeros(3, 16, 128), wq, K=128, Nc=128, wq=wq)),
        ("gn_mish pw, sums in the kernel", tile64, lambda: K.conv3x3_gn_mish(big(BF), None, wq, K=128, Nc=128, wq=wq, gn=_gn(16, 128, 8), bias=torch.zeros(128))),
        ("gn_mish pw, sums resolved first", tile64, lambda: K.conv3x3_gn_mish(big(BF), None, wq, K=128, Nc=128, wq=wq, gn=_gn(16, 128, 16, temb=False), out_dtype=F32)),
        ("gn_mish pw fp32 in, coef", tile64, lambda: K.conv3x3_gn_mish(act(32, 16, 16, 128), torch.zeros(3, 32, 128), wq, K=128, Nc=128, wq=wq)),
        ("gn_mish pw fp32 in, sums", tile64, lambda: K.conv3x3_gn_mish(act(32, 16, 16, 128), None, wq, K=128, Nc=128, wq=wq, gn=_gn(32, 128, 8), out_dtype=BF)),
        ("gn_mish pw fp32 in, sums resolved first", tile64, lambda: K.conv3x3_gn_mish(act(32, 16, 16, 128), None, wq, K=128, Nc=128, wq=wq, gn=_gn(32, 128, 16))),
        ("gn_mish halo, pitched in", no_fused, lambda: K.conv3x3_gn_mish(act(2, 8, 8, 128, BF, pitch=256), torch.zeros(3, 2, 128), wq, K=128, Nc=256, wq=wq)),
        ("gn_mish halo, sums, no wq", None, lambda: K.conv3x3_gn_mish(act(2, 8, 8, 128), None, wq, K=128, Nc=128, gn=_gn(2, 128, 8))),
        ("gn_mish refused", {"*": 0}, lambda: K.conv3x3_gn_mish(act(2, 8, 8, 128, BF), torch.zeros(3, 2, 128), wq, K=128, Nc=128, wq=wq)),
        # exact fp32
        ("conv3x3_f32 plain", tile64, lambda: K.conv3x3_f32(act(2, 8, 8, 128), wq, **c3)),
        ("conv3x3_f32 two sources, residual, accumulate, pitched out", tile64,
         lambda: K.conv3x3_f32(act(2, 8, 8, 96), wq, x2=act(2, 8, 8, 32, pitch=40), residual=act(2, 8, 8, 128, pitch=136), out=act(2, 8, 8, 128, pitch=256),
                               accumulate=True, bias=torch.zeros(128), K=128, Nc=128, flip=True)),
        ("conv3x3_f32 out pitch % 8", tile64, lambda: K.conv3x3_f32(act(2, 8, 8, 128), wq, out=act(2, 8, 8, 128, pitch=132), **c3)),
        ("conv3x3_f32 refused", {"*": 0}, lambda: K.conv3x3_f32(act(2, 8, 8, 128), wq, **c3)),
        ("conv3x3_f32 bf16 in", tile64, lambda: K.conv3x3_f32(act(2, 8, 8, 128, BF), wq, **c3)),
        ("conv1x1_f32 plain", None, lambda: K.conv1x1_f32(act(2, 8, 8, 128), wq, K=128, Nc=384, flip=False)),
        ("conv1x1_f32 two sources, residual, accumulate, pitched out", None,
         lambda: K.conv1x1_f32(act(2, 8, 8, 96), wq, x2=act(2, 8, 8, 32, pitch=40), residual=act(2, 8, 8, 128, pitch=136), out=act(2, 8, 8, 128, pitch=256),
                               accumulate=True, K=128, Nc=128, flip=True)),
        ("conv1x1_f32 residual pitch % 4", None, lambda: K.conv1x1_f32(act(2, 8, 8, 128), wq, residual=act(2, 8, 8, 128, pitch=130), **c3)),
        ("conv1x1_f32 refused", {"*": 0}, lambda: K.conv1x1_f32(act(2, 8, 8, 128), wq, **c3)),
        # weight gradients
        ("conv_wgrad ordered", None, lambda: K.conv_wgrad(act(2, 8, 8, 128), act(2, 8, 8, 256), torch.zeros(9 * 128 * 256), mode=M32, ordered=True, dbias=torch.zeros(256), **wg)),
        ("conv_wgrad tr", None, lambda: K.conv_wgrad(act(2, 8, 8, 128, BF), act(2, 8, 8, 256, BF, pitch=320), torch.zeros(9 * 128 * 256), mode=M16, **wg)),
        ("conv_wgrad fast io, two sources, dbias", None,
         lambda: K.conv_wgrad(act(2, 8, 8, 96, BF), act(2, 8, 8, 256), torch.zeros(9 * 128 * 256), mode=M16, P2=act(2, 8, 8, 32, BF, pitch=64), dbias=torch.zeros(256), **wg)),
        ("conv_wgrad fast fp32", None, lambda: K.conv_wgrad(act(2, 8, 8, 128), act(2, 8, 8, 256), torch.zeros(9 * 128 * 256), mode=M16, **wg)),
        ("conv_wgrad generic, stride 2, dbias", {"*": 0},
         lambda: K.conv_wgrad(act(2, 16, 16, 64), act(2, 8, 8, 32), torch.zeros(9 * 64 * 32), kh=3, kw=3, stride=2, pad=1, gather_i=True, Ci=64, Cj=32,
                              grid_g=(16, 16), grid_d=(8, 8), mode=M32, dbias=torch.zeros(32))),
        ("conv_wgrad generic, transposed 4x4", {"*": 0},
         lambda: K.conv_wgrad(act(2, 8, 8, 64), act(2, 16, 16, 32), torch.zeros(16 * 64 * 32), kh=4, kw=4, stride=2, pad=1, gather_i=False, Ci=64, Cj=32,
                              grid_g=(16, 16), grid_d=(8, 8), mode=M32)),
        ("conv_s2_wgrad_f32 down", {"*": 1, "mi_conv_s2_wgrad_f32_workspace": 64}, lambda: K.conv_s2_wgrad_f32(act(2, 16, 16, 64), act(2, 8, 8, 64), torch.zeros(9 * 64 * 64), **s2d)),
        ("conv_s2_wgrad_f32 up, pitched", {"*": 1, "mi_conv_s2_wgrad_f32_workspace": 64},
         lambda: K.conv_s2_wgrad_f32(act(2, 8, 8, 64, pitch=72), act(2, 16, 16, 64, pitch=80), torch.zeros(16 * 64 * 64), **s2u)),
        ("conv_s2_wgrad_f32 refused", {"*": 0}, lambda: K.conv_s2_wgrad_f32(act(2, 16, 16, 64), act(2, 8, 8, 64), torch.zeros(9 * 64 * 64), **s2d)),
        ("conv_s2_wgrad_f32 bf16", None, lambda: K.conv_s2_wgrad_f32(act(2, 16, 16, 64, BF), act(2, 8, 8, 64), torch.zeros(9 * 64 * 64), **s2d)),
        ("WgradQueue 3x3", None, lambda: _queue(K, 3)),
        ("WgradQueue 3x3 store", None, lambda: _queue(K, 3, store=True)),
        ("WgradQueue 3x3 two sources", None, lambda: _queue(K, "3two")),
        ("WgradQueue 3x3 fp32", None, lambda: _queue(K, "3f32")),
        ("WgradQueue 3x3 fallback, store", {"*": 1, "mi_conv3x3_wgrad_tr_supported": 0}, lambda: _queue(K, 3, store=True)),
        ("WgradQueue 1x1", None, lambda: _queue(K, 1)),
        ("WgradQueue 1x1 fp32", None, lambda: _queue(K, "1f32")),
        ("WgradQueue 1x1 fallback", {"*": 1, "mi_conv1x1_wgrad_tr_supported": 0}, lambda: _queue(K, 1)),
        ("WgradQueue stride 2", None, lambda: _queue(K, 2)),
        ("WgradQueue stride 2 refused", {"*": 0}, lambda: _queue(K, 2)),
        # LayerNorm + to_qkv, attention's to_out
        ("ln_conv1x1_supported", None, lambda: (K.ln_conv1x1_supported(16, 32, 32, 128, 384), K.ln_conv1x1_supported(16, 32, 32, 128, 384, ldx=256))),
        ("ln_conv1x1_supported no", {"*": 0}, lambda: K.ln_conv1x1_supported(16, 7, 7, 100, 60)),
        ("ln_conv1x1", None, lambda: K.ln_conv1x1(act(2, 8, 8, 128), torch.ones(128), torch.zeros(128), wq, Nc=384, bias=torch.zeros(384))),
        ("ln_conv1x1 want_ln, pitched", None, lambda: K.ln_conv1x1(act(2, 8, 8, 128, pitch=256), torch.ones(128), torch.zeros(128), wq, Nc=384, want_ln=True)),
        ("linattn_to_out_folded", {"*": 1, "mi_linattn_workspace": 0}, lambda: K.linattn_to_out_folded(act(2, 8, 8, 384, BF), wq, 128, torch.zeros(128), None)),
        ("linattn_to_out_folded residual, want16", {"*": 1, "mi_linattn_workspace": 0},
         lambda: K.linattn_to_out_folded(act(2, 8, 8, 384, BF), wq, 256, torch.zeros(256), act(2, 8, 8, 256, pitch=320), want16=True)),
        ("linattn_to_out_folded sliced", {"*": 1, "mi_linattn_workspace": 4096}, lambda: K.linattn_to_out_folded(act(2, 8, 8, 384, BF), wq, 128, None, None)),
    ]


def replay_wrappers(K):
    """-> [[label, recorded calls, returned value (tensors as shape / stride / dtype)]]: every case from an empty cache."""
    out = []
    for label, answers, thunk in wrapper_cases(K):
        with stubbed(K, answers) as stub:
            r = thunk()
        out.append([label, stub.calls, _plain(r)])
    return out


def replay(K):
    return {"questions": replay_questions(K), "wrappers": replay_wrappers(K)}
